"""Independent restatement of the point-seeding contract in
fp64 numpy: the box, the hull vote of every view, the nearest view and the
colour / direction lookup.  Inputs are the fp32 values the device holds (the
camera table of rays_ref.cam_row, fp32 points), widened; nothing here is
rounded to fp32 on the way."""
import numpy as np

import rays_ref as RR


def ring_cameras(F, radius=3.0):
    """The test scenes' cameras: azimuth 2 pi f / F, elevation 0.3 + 0.25 sin(3
    azimuth) rad on a sphere of ``radius``, looking at the origin with z up.
    Returns campos [F,3], camrotc2w [F,3,3] (columns right, down, forward)."""
    pos, rot = [], []
    for f in range(F):
        az = 2 * np.pi * f / F
        el = 0.3 + 0.25 * np.sin(3 * az)
        c = radius * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        pos.append(c)
        rot.append(np.stack([right, down, fwd], 1))
    return np.array(pos), np.array(rot)


def disc_alphas(F, H, W, radius, dtype=np.float32):
    """[F,H,W]: 1 inside a centred disc of ``radius`` pixels (pixel centres), else 0."""
    y, x = np.mgrid[:H, :W]
    on = (x + 0.5 - W / 2) ** 2 + (y + 0.5 - H / 2) ** 2 <= radius ** 2
    return np.broadcast_to(on.astype(dtype), (F, H, W)).copy()


def scene(N=20000, F=12, H=48, W=64, focal=60.0, radius=16.0, seed=0, float_images=False):
    """The seeding tests' scene: N points uniform in [-1,1]^3, F ring cameras,
    noise images, centred disc silhouettes."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    images = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    if float_images:
        images = rng.random((F, H, W, 3), dtype=np.float32)
    campos, camrot = ring_cameras(F)
    K = RR.focal_K(focal, H, W)
    return dict(xyz=xyz, images=images, alphas=disc_alphas(F, H, W, radius), campos=campos, camrot=camrot, K=K,
                cams=cam_table(campos, camrot, K), H=H, W=W, F=F)


def cam_table(campos, camrot, K):
    K = np.asarray(K, np.float64)
    K = np.broadcast_to(K.reshape(-1, 3, 3), (len(campos), 3, 3))
    return np.stack([RR.cam_row(campos[f], camrot[f], K[f]) for f in range(len(campos))])


def cam_coords(xyz, cams):
    """c [N,F,3] = Rc2w^T (p - campos), summed left to right."""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    cams = np.asarray(cams, np.float32).astype(np.float64)
    s = p[:, None, :] - cams[None, :, 9:12]
    R = cams[:, :9].reshape(-1, 3, 3)
    return np.stack([(s[..., 0] * R[None, :, 0, j] + s[..., 1] * R[None, :, 1, j]) + s[..., 2] * R[None, :, 2, j]
                     for j in range(3)], -1)


def pixel_pos(c, cams):
    """(u, v) [N,F]: fx cx / cz + cx0, fy cy / cz + cy0 (inf / nan where cz = 0)."""
    cams = np.asarray(cams, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = cams[None, :, 12] * c[..., 0] / c[..., 2] + cams[None, :, 14]
        v = cams[None, :, 13] * c[..., 1] / c[..., 2] + cams[None, :, 15]
    return u, v


def inside(u, v, cz, H, W):
    with np.errstate(invalid="ignore"):
        return (cz > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)


def alpha_on(alphas):
    a = np.asarray(alphas)
    if a.dtype == np.uint8:
        return a.astype(np.float32) / np.float32(255) > np.float32(0.1)
    return a.astype(np.float32) > np.float32(0.1)


def mask(xyz, cams, H, W, alphas=None, ranges=None, near_far=None, inall_img=1):
    """keep [N] bool."""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    keep = np.ones(len(p), bool)
    if ranges is not None and np.float32(ranges[0]) > -99:
        r = np.asarray(ranges, np.float32).astype(np.float64)
        keep &= np.all((p >= r[None, :3]) & (p <= r[None, 3:]), -1)
    if alphas is None and near_far is None:
        return keep
    c = cam_coords(xyz, cams)
    cz = c[..., 2]
    vote = np.ones(cz.shape, bool)
    if alphas is not None:
        on = alpha_on(alphas)
        u, v = pixel_pos(c, cams)
        ins = inside(u, v, cz, H, W)
        with np.errstate(invalid="ignore"):
            x = np.clip(np.nan_to_num(np.floor(u), nan=0.0, posinf=W - 1, neginf=0), 0, W - 1).astype(np.int64)
            y = np.clip(np.nan_to_num(np.floor(v), nan=0.0, posinf=H - 1, neginf=0), 0, H - 1).astype(np.int64)
        bit = on[np.arange(cz.shape[1])[None, :], y, x]
        if inall_img:   # outside: the border pixel; behind the camera: carved
            vote = np.where(cz > 0, bit, False)
        else:           # outside or behind: the view passes
            vote = np.where(ins, bit, True)
    if near_far is not None:
        n, f = (np.float64(np.float32(t)) for t in near_far)
        vote = vote & (cz >= n - 1.0) & (cz <= f)
    return keep & vote.all(1)


def cam_dirs(cams, H, W):
    """camdir [F,3]: the fp32 direction camera_rays gives for pixel (W//2, H//2)
    with dir_norm."""
    return np.concatenate([RR.directions([W // 2], [H // 2], cam, True) for cam in np.asarray(cams, np.float32)])


def unit_to(xyz, cams):
    """d^ [N,F,3] = d / (|d| + 1e-6) and |d| [N,F], d = p - campos."""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    d = p[:, None, :] - np.asarray(cams, np.float32).astype(np.float64)[None, :, 9:12]
    n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return d / (n + np.float64(np.float32(1e-6)))[..., None], n


def view_scores(xyz, cams, H, W):
    """[N,F]: |d| / 200 + (1.1 - d^ . camdir_f)."""
    dh, n = unit_to(xyz, cams)
    cd = cam_dirs(cams, H, W).astype(np.float64)
    dot = (dh[..., 0] * cd[None, :, 0] + dh[..., 1] * cd[None, :, 1]) + dh[..., 2] * cd[None, :, 2]
    return n / 200.0 + (np.float64(np.float32(1.1)) - dot)


def images64(images):
    im = np.asarray(images)
    return im.astype(np.float64) / 255.0 if im.dtype == np.uint8 else im.astype(np.float32).astype(np.float64)


def view(xyz, cams, images, H, W, cam_ind=None):
    """cam_ind [M], dirs [M,3], color [M,3], in_view [M] of the nearest view
    (np.argmin: the lowest index on ties), or of the views given."""
    m = len(xyz)
    if m == 0:
        return np.zeros(0, np.int64), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, bool)
    if cam_ind is None:
        cam_ind = np.argmin(view_scores(xyz, cams, H, W), 1)
    cam_ind = np.asarray(cam_ind, np.int64)
    rows = np.arange(m)
    dh, _ = unit_to(xyz, cams)
    c = cam_coords(xyz, cams)
    u, v = pixel_pos(c, cams)
    u, v, cz = u[rows, cam_ind], v[rows, cam_ind], c[rows, cam_ind, 2]
    seen = inside(u, v, cz, H, W)
    su, sv = np.where(seen, u, 0.5), np.where(seen, v, 0.5)
    sx, sy = su - 0.5, sv - 0.5
    fx, fy = np.floor(sx), np.floor(sy)
    wx, wy = (sx - fx)[:, None], (sy - fy)[:, None]
    x0, x1 = np.maximum(fx, 0).astype(np.int64), np.minimum(fx + 1, W - 1).astype(np.int64)
    y0, y1 = np.maximum(fy, 0).astype(np.int64), np.minimum(fy + 1, H - 1).astype(np.int64)
    im = images64(images)
    top = (1 - wx) * im[cam_ind, y0, x0] + wx * im[cam_ind, y0, x1]
    bot = (1 - wx) * im[cam_ind, y1, x0] + wx * im[cam_ind, y1, x1]
    color = np.where(seen[:, None], (1 - wy) * top + wy * bot, 0.0)
    return cam_ind, dh[rows, cam_ind], color, seen


def seed(xyz, cams, images, alphas=None, ranges=None, near_far=None, inall_img=1):
    """The whole contract without the voxel stage: dict(src_idx, xyz, cam_ind,
    dirs, color, in_view)."""
    H, W = np.asarray(images).shape[1:3]
    keep = mask(xyz, cams, H, W, alphas, ranges, near_far, inall_img)
    src = np.nonzero(keep)[0]
    pts = np.asarray(xyz, np.float32)[src]
    cam_ind, dirs, color, seen = view(pts, cams, images, H, W)
    return dict(src_idx=src, xyz=pts, cam_ind=cam_ind, dirs=dirs, color=color, in_view=seen, keep=keep)


# ------------------------------------------------------------ hand-built cases
def hand_camera(z=-3.0, flip=False):
    """A camera on the z axis at height z looking along +z (flip: along -z),
    x right and y down: every projection below is exact in fp32."""
    R = np.diag([-1.0, 1.0, -1.0]) if flip else np.eye(3)
    return np.array([0.0, 0.0, z]), R


HAND_H, HAND_W = 6, 8
HAND_K = np.array([[4.0, 0, 4.0], [0, 4.0, 3.0], [0, 0, 1.0]])   # u = 4 cx / cz + 4, v = 4 cy / cz + 3


def hand_cases():
    """name -> dict(xyz, cams, images, alphas, kwargs, keep) with the expected
    survivors worked out by hand; some add cam_ind / color / in_view of the
    survivors."""
    rng = np.random.default_rng(5)
    H, W = HAND_H, HAND_W

    def setup(cameras, alphas="ones"):
        pos, rot = (np.array(v) for v in zip(*cameras))
        F = len(pos)
        images = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
        al = np.ones((F, H, W), np.float32) if isinstance(alphas, str) else alphas
        return dict(campos=pos, camrot=rot, cams=cam_table(pos, rot, HAND_K), images=images, alphas=al)

    cases = {}
    # pixel (5, 1): x = (5.5 - 4) / 4, y = (1.5 - 3) / 4; two units along that ray from (0, 0, -3)
    c = setup([hand_camera()])
    cases["on_ray"] = dict(c, xyz=[[0.75, -0.75, -1.0]], kwargs={}, keep=[True], cam_ind=[0], in_view=[True],
                           color=[c["images"][0, 1, 5] / 255.0])
    # (0, 0, -5) is behind the camera (cz = -2; its mirrored pixel (4, 3) is lit, so the reference keeps it)
    c = setup([hand_camera()])
    for inall, keep in ((1, [False, True]), (0, [True, True])):
        cases[f"behind_inall{inall}"] = dict(c, xyz=[[0, 0, -5.0], [0, 0, 0]], kwargs=dict(inall_img=inall), keep=keep)
    # u = -2 (left of the image) and u = 10 (right of it), v = 3; the left border column is dark
    dark_left = np.ones((1, H, W), np.float32)
    dark_left[:, :, 0] = 0
    c = setup([hand_camera()], dark_left)
    for inall, keep in ((1, [False, True]), (0, [True, True])):
        cases[f"outside_inall{inall}"] = dict(c, xyz=[[-3.0, 0, -1.0], [3.0, 0, -1.0]], kwargs=dict(inall_img=inall),
                                              keep=keep)
    # near_far = (2, 4): 1 <= cz <= 4, closed; cz = z + 3
    one = np.float32(1)
    c = setup([hand_camera()])
    # (the steps outside the band are fp32 steps of cz, not of z: z + 3 is then exact in fp32 too)
    z = [-2.0, np.nextafter(np.float32(-2), -3 * one), 1.0, 1.0 + 2.0 ** -21]
    cases["near_far"] = dict(c, alphas=None, xyz=[[0, 0, t] for t in z], kwargs=dict(near_far=(2.0, 4.0)),
                             keep=[True, False, True, False])
    # the same pose twice: an exact tie, the lower index wins; a farther camera loses
    c = setup([hand_camera(-6.0), hand_camera(), hand_camera()])
    cases["tie"] = dict(c, xyz=[[0, 0, 0], [0.5, 0.25, 0.5]], kwargs={}, keep=[True, True], cam_ind=[1, 1])
    # the closed box, and ranges[0] <= -99 switching it off
    c = setup([hand_camera()])
    pts = [[0, 0, 0], [2.0, 0, 0], [1.0, 0, 0], [0, 0, np.nextafter(one, 2 * one)]]
    cases["ranges"] = dict(c, alphas=None, xyz=pts, kwargs=dict(ranges=(-1, -1, -1, 1, 1, 1)),
                           keep=[True, False, True, False])
    cases["ranges_off"] = dict(c, alphas=None, xyz=pts, kwargs=dict(ranges=(-100, -1, -1, 1, 1, 1)), keep=[True] * 4)
    for case in cases.values():
        case["xyz"] = np.asarray(case["xyz"], np.float32)
    return cases
