"""Independent restatement of the plane-background contract in
numpy: the ray / plane intersection, the foreground masks and the sample / fit
/ max over the source views.  Every stage takes the working dtype: float64 is
the reference, the same code in float32 (elementwise numpy operations round
once each and do not fuse) the yardstick.  Inputs are the fp32 values the
device holds (camera table of rays_ref.cam_row, fp32 rays and points), widened.

Also the tests' scene: a tilted table plane, cameras on a ring looking at
different parts of it, a small cloud standing on it, and images made by
projecting the plane."""
import itertools

import numpy as np

import rays_ref as RR

PIX_BAND, DOT_BAND, FIT_BAND = 1e-3, 1e-6, 1e-4     # where fp64 itself is within reach of fp32 rounding
BAND_CAP = 0.02                                     # share of a scene's rays the bands may hold
DOT_EPS = np.float32(1e-3)
THRESH = np.float32(0.03)
ULP1 = float(np.finfo(np.float32).eps)              # one ulp of 1.0


# ------------------------------------------------------------------ the stages
def _w(a, dt):
    """The fp32 value the device holds, in the working dtype."""
    return np.asarray(a, np.float32).astype(dt)


def intersect(campos, raydir, plane_pnt, plane_normal, dt=np.float64, hit=None):
    """(p [R,3], dot [R], hit [R]): p = campos + d * (-(n . (campos - p0)) / dot)
    where dot = n . d >= 1e-3, the world origin elsewhere.  hit: decide the
    branch from outside (the admissible other answer of a ray in the dot band)."""
    c, d, p0, n = _w(campos, dt).reshape(3), _w(raydir, dt).reshape(-1, 3), _w(plane_pnt, dt), _w(plane_normal, dt)
    dot = (n[0] * d[:, 0] + n[1] * d[:, 1]) + n[2] * d[:, 2]
    if hit is None:
        hit = dot >= DOT_EPS.astype(dt)
    w = c - p0
    nw = (n[0] * w[0] + n[1] * w[1]) + n[2] * w[2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        fac = (-nw) / dot
        p = c[None, :] + d * fac[:, None]
    return np.where(hit[:, None], p, dt(0)), dot, hit


def project(p, cams, dt=np.float64):
    """(u, v) [N,F] = (cx / cz fx + cx0, cy / cz fy + cy0), c = Rc2w^T (p -
    campos) summed left to right; texel centres at the integers."""
    p, cams = np.asarray(p, dt), _w(cams, dt)
    s = p[:, None, :] - cams[None, :, 9:12]
    R = cams[:, :9].reshape(-1, 3, 3)
    xc = [(s[..., 0] * R[None, :, 0, j] + s[..., 1] * R[None, :, 1, j]) + s[..., 2] * R[None, :, 2, j] for j in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = (xc[0] / xc[2]) * cams[None, :, 12] + cams[None, :, 14]
        v = (xc[1] / xc[2]) * cams[None, :, 13] + cams[None, :, 15]
    return u, v


def in_bounds(u, v, H, W):
    """0 <= u <= W - 1 and 0 <= v <= H - 1, both ends included; False for NaN."""
    with np.errstate(invalid="ignore"):
        return (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)


def _ceil_px(u, inb):
    return np.where(inb, np.ceil(np.where(inb, u, 0)), 0).astype(np.int64)


def fg_masks(xyz, cams, H, W, dt=np.float64):
    """[F,H,W] bool: fg[f, ceil(v), ceil(u)] for every point in bounds of view f."""
    F = len(cams)
    fg = np.zeros((F, H, W), bool)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    if len(xyz) == 0:
        return fg
    u, v = project(_w(xyz, dt), cams, dt)
    inb = in_bounds(u, v, H, W)
    n, f = np.nonzero(inb)
    fg[f, _ceil_px(v, inb)[n, f], _ceil_px(u, inb)[n, f]] = True
    return fg


def fg_mask_range(xyz, cams, H, W):
    """(lo, hi) [F,H,W] bool: the pixels every admissible mask has, and the
    pixels some admissible mask has: a point whose fp64 projection is within
    PIX_BAND of an integer (so also of a bound) in a view may mark either
    neighbour there, or none at the bound."""
    F = len(cams)
    lo, hi = np.zeros((F, H, W), bool), np.zeros((F, H, W), bool)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    if len(xyz) == 0:
        return lo, hi
    u, v = project(_w(xyz, np.float64), cams)
    with np.errstate(invalid="ignore"):
        close = (np.abs(u - np.round(u)) < PIX_BAND) | (np.abs(v - np.round(v)) < PIX_BAND)
    inb = in_bounds(u, v, H, W)
    sure = inb & ~close
    n, f = np.nonzero(sure)
    lo[f, _ceil_px(v, sure)[n, f], _ceil_px(u, sure)[n, f]] = True
    hi |= lo
    for du, dv in itertools.product((-PIX_BAND, PIX_BAND), repeat=2):
        uu, vv = u + du, v + dv
        ok = in_bounds(uu, vv, H, W) & close
        n, f = np.nonzero(ok)
        hi[f, _ceil_px(vv, ok)[n, f], _ceil_px(uu, ok)[n, f]] = True
    return lo, hi


def images_as(images, dt):
    """uint8 read as q / 255 in the working dtype, floats as their fp32 value."""
    im = np.asarray(images)
    return im.astype(dt) / dt(255) if im.dtype == np.uint8 else im.astype(np.float32).astype(dt)


def bilinear(im, f, u, v, dt=np.float64):
    """[..., 3]: images im [F,H,W,3] (working dtype) of views f at (u, v), texel
    centres at the integers, taps outside the image zero (grid_sample with
    align_corners=True, padding_mode='zeros' on u / ((W - 1) / 2) - 1)."""
    _, H, W, _ = im.shape
    u, v = np.asarray(u, dt), np.asarray(v, dt)
    fx, fy = np.floor(u), np.floor(v)
    wx, wy = (u - fx)[..., None], (v - fy)[..., None]
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)

    def tap(y, x):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(ok[..., None], im[f, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], dt(0))

    one = dt(1)
    top = (one - wx) * tap(y0, x0) + wx * tap(y0, x0 + 1)
    bot = (one - wx) * tap(y0 + 1, x0) + wx * tap(y0 + 1, x0 + 1)
    return (one - wy) * top + wy * bot


def fit_bounds(plane_color, dt=np.float64):
    """(lo, hi) [3]: plane_color -+ 0.03 formed in fp32, then widened."""
    c = np.asarray(plane_color, np.float32)
    return (c - THRESH).astype(dt), (c + THRESH).astype(dt)


def evaluate(campos, raydir, plane_pnt, plane_normal, plane_color, cams, images, fg, dt=np.float64, hit=None):
    """The whole contract for one ray batch: dict(bg [R,3], p, dot, hit, u, v
    [R,F], inb, covered, sample [R,F,3], fits, used [R,F])."""
    F, H, W, _ = np.asarray(images).shape
    p, dot, hit = intersect(campos, raydir, plane_pnt, plane_normal, dt, hit)
    u, v = project(p, cams, dt)
    inb = in_bounds(u, v, H, W)
    fidx = np.broadcast_to(np.arange(F)[None, :], u.shape)
    covered = inb & np.asarray(fg, bool)[fidx, _ceil_px(v, inb), _ceil_px(u, inb)]
    su, sv = np.where(inb, u, 0), np.where(inb, v, 0)
    sample = bilinear(images_as(images, dt), fidx, su, sv, dt)
    lo, hi = fit_bounds(plane_color, dt)
    fits = np.all((sample >= lo) & (sample <= hi), -1)
    used = inb & ~covered & fits
    bg = np.where(used.any(1)[:, None], np.max(np.where(used[..., None], sample, -np.inf), 1), 0).astype(dt)
    return dict(bg=bg, p=p, dot=dot, hit=hit, u=u, v=v, inb=inb, covered=covered, sample=sample, fits=fits, used=used)


# ------------------------------------------------------------------- the bands
def bands(ref, H, W, plane_color, fg_lo=None, fg_hi=None):
    """(banded [R] bool, open_views [R,F] bool) of an fp64 ``evaluate``: the
    rays fp64 itself puts within reach of fp32 rounding, and for each the views
    whose vote may fall either way.  A view is open when the projection is
    within PIX_BAND of an integer (the 0 / W-1 / H-1 bounds are integers) while
    within PIX_BAND of the image, when a sampled channel of a view otherwise in
    play is within FIT_BAND of a fit bound, or when its fg pixel differs
    between the admissible masks (fg_lo, fg_hi of fg_mask_range).  A ray with
    |dot - 1e-3| < DOT_BAND is banded whatever its views do."""
    u, v = ref["u"], ref["v"]
    with np.errstate(invalid="ignore"):
        near = (u >= -PIX_BAND) & (u <= W - 1 + PIX_BAND) & (v >= -PIX_BAND) & (v <= H - 1 + PIX_BAND)
        close = near & ((np.abs(u - np.round(u)) < PIX_BAND) | (np.abs(v - np.round(v)) < PIX_BAND))
    lo, hi = fit_bounds(plane_color)
    s = ref["sample"]
    edge = ((np.abs(s - lo) < FIT_BAND) | (np.abs(s - hi) < FIT_BAND)).any(-1) & ref["inb"] & ~ref["covered"]
    open_views = close | edge
    if fg_lo is not None:
        F = u.shape[1]
        fidx = np.broadcast_to(np.arange(F)[None, :], u.shape)
        y, x = _ceil_px(v, ref["inb"]), _ceil_px(u, ref["inb"])
        open_views |= ref["inb"] & (fg_lo[fidx, y, x] != fg_hi[fidx, y, x])
    dot_band = np.abs(ref["dot"] - np.float64(DOT_EPS)) < DOT_BAND
    return open_views.any(1) | dot_band, open_views


def admissible(ref, alt, open_views, r, got, tol, max_open=8):
    """Is got [3] an admissible bg of banded ray r?  Every closed view votes as
    in fp64; every open view may be in or out with its fp64 sample; ``alt`` is
    the evaluation with the other branch of the intersection (for the dot
    band) or None.  None when there are too many open views to enumerate."""
    opened = np.nonzero(open_views[r])[0]
    if len(opened) > max_open:
        return None
    for e in (ref, alt):
        if e is None:
            continue
        base = e["used"][r] & ~open_views[r]
        for pick in itertools.product((False, True), repeat=len(opened)):
            use = base.copy()
            use[opened] = pick
            want = e["sample"][r][use].max(0) if use.any() else np.zeros(3)
            if np.all(np.abs(got - want) <= tol):
                return True
    return False


def banded_share(sc):
    """Share of the scene's rays in the bands, from the fp64 reference alone."""
    ref = evaluate(sc["campos"], sc["raydir"], sc["plane_pnt"], sc["plane_normal"], sc["plane_color"], sc["cams"],
                   sc["images"], sc["fg64"])
    banded, _ = bands(ref, sc["H"], sc["W"], sc["plane_color"], *sc["fg_range"])
    return float(banded.mean()), ref


# ------------------------------------------------------------------- the scene
PLANE_PNT = np.array([0.1, -0.05, -0.2], np.float32)
PLANE_NORMAL = np.array([0.15, -0.1, -1.0], np.float32)      # not normalised; cameras sit on its negative side
COLOR_LEVELS = np.array([153, 128, 102])                     # plane_color = levels / 255
OFFSETS = np.array([0, 2, -3, 5])                            # per view and channel, in levels: all fit (|.| / 255 < 0.03)
OFF_VIEW, OFF_BY = 2, 0.05                                   # the view whose plane never fits: 13 levels = 0.051


LEAD_RAY = 148     # of the 16 x 20 frame: two views fit it with different values, a point covers it in two more


def look_at(pos, target):
    """camrotc2w (columns right, down, forward), z up."""
    fwd = (target - pos) / np.linalg.norm(target - pos)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(fwd, right), fwd], 1)


def cameras(F, seeing=None, radius=3.0):
    """F cameras on a ring above the table, each looking at its own spot 0.5
    from the plane point so that a plane point is in two or three views, not
    all; the views not in ``seeing`` look at the horizon, away from the table."""
    pos, rot = [], []
    for f in range(F):
        az = 2 * np.pi * f / F + 0.3
        el = 0.75 + 0.2 * np.sin(3 * az)
        c = PLANE_PNT + radius * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        if seeing is None or f in seeing:
            t = PLANE_PNT + 0.5 * np.array([np.cos(2.4 * f + 1.0), np.sin(2.4 * f + 1.0), 0.0])
        else:
            t = c + 30.0 * np.array([np.cos(az), np.sin(az), 0.05])
        pos.append(c)
        rot.append(look_at(c, t))
    return np.array(pos), np.array(rot)


def plane_color():
    """fp32 [3]: exactly what a uint8 image holding COLOR_LEVELS reads as."""
    return COLOR_LEVELS.astype(np.float32) / np.float32(255)


def view_levels(f, F):
    """The plane region's colour of view f, in levels [3]."""
    if f == OFF_VIEW and F > 2:
        return COLOR_LEVELS + int(round(OFF_BY * 255))
    return COLOR_LEVELS + OFFSETS[(f + np.arange(3)) % 4] * (f > 0)


def plane_images(campos, camrot, K, H, W, disc=1.0, u8=True):
    """[F,H,W,3]: through every texel centre (integer coordinates) a ray; where
    it meets the plane within ``disc`` of the plane point the view's plane
    colour, elsewhere a smooth pattern whose first channel is nowhere near."""
    F = len(campos)
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (F, 3, 3))
    y, x = np.mgrid[:H, :W].astype(np.float64)
    pattern = np.stack([0.15 + 0.1 * np.sin(x / 5.0), 0.5 + 0.3 * np.cos(y / 4.0), 0.8 + 0.1 * np.sin((x + y) / 6.0)], -1)
    n, p0 = PLANE_NORMAL.astype(np.float64), PLANE_PNT.astype(np.float64)
    out = np.empty((F, H, W, 3))
    for f in range(F):
        dc = np.stack([(x - K[f, 0, 2]) / K[f, 0, 0], (y - K[f, 1, 2]) / K[f, 1, 1], np.ones_like(x)], -1)
        d = dc @ camrot[f].T
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (n @ (p0 - campos[f])) / (d @ n)
        hit = campos[f] + d * t[..., None]
        on = (t > 0) & (np.linalg.norm(hit - p0, axis=-1) < disc)
        if u8:
            out[f] = np.where(on[..., None], view_levels(f, F), np.round(pattern * 255))
        else:   # the value a uint8 image would read as where the plane is, the pattern itself elsewhere
            out[f] = np.where(on[..., None], view_levels(f, F).astype(np.float32) / np.float32(255),
                              pattern.astype(np.float32))
    return out.astype(np.uint8 if u8 else np.float32)


def cloud(n, seed=0):
    """n points standing on the plane around the plane point (fp32 [n,3])."""
    rng = np.random.default_rng(seed)
    up = -PLANE_NORMAL.astype(np.float64) / np.linalg.norm(PLANE_NORMAL)
    side = rng.normal(0, 0.18, (n, 3))
    side -= (side @ up)[:, None] * up
    return (PLANE_PNT + side + up * rng.uniform(0, 0.5, (n, 1))).astype(np.float32)


def render_rays(h, w, focal=12.0, az=1.0, el=0.55, radius=2.0, pixels=None):
    """(campos [3], camrot, cam row, raydir [R,3] fp32) of the render camera: a
    wide view of the table from another place, its top rows above the horizon."""
    c = PLANE_PNT + radius * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    rot = look_at(c, PLANE_PNT.astype(np.float64))
    K = RR.focal_K(focal, h, w)
    row = RR.cam_row(c, rot, K)
    if pixels is None:
        i = np.arange(h * w)
        px, py = i % w, i // w
    else:
        px, py = np.asarray(pixels).T
    return row[9:12].copy(), rot, row, RR.directions(px, py, row), K


def scene(F=5, H=29, W=37, h=16, w=20, R=None, u8=True, per_frame_K=False, n_points=400, seeing=None, focal=60.0,
          seed=0):
    """The tests' scene.  R: LEAD_RAY and the first R - 1 other rays of a shuffled
    h x w frame (None: the whole frame in order)."""
    campos, camrot = cameras(F, seeing)
    K = RR.focal_K(focal, H, W)
    K[0, 2], K[1, 2] = (W - 1) / 2, (H - 1) / 2         # the principal point at the centre texel
    if per_frame_K:
        K = np.stack([K * np.array([[1 + 0.03 * (f % 3), 1, 1], [1, 1 - 0.02 * (f % 4), 1], [1, 1, 1]])
                      for f in range(F)])
    from seed_ref import cam_table
    cams = cam_table(campos, camrot, K)
    images = plane_images(campos, camrot, K, H, W, u8=u8)
    xyz = cloud(n_points, seed)
    rpos, rrot, rrow, raydir, rK = render_rays(h, w)
    if R is not None:
        pick = np.random.default_rng(seed + 7).permutation(h * w)
        pick = np.concatenate([[LEAD_RAY], pick[pick != LEAD_RAY]])[:R]
        raydir = raydir[pick]
    return dict(F=F, H=H, W=W, h=h, w=w, campos=rpos, camrot=rrot, render_K=rK, raydir=raydir, campos_f=campos,
                camrot_f=camrot, K=K, cams=cams, images=images, xyz=xyz, plane_pnt=PLANE_PNT,
                plane_normal=PLANE_NORMAL, plane_color=plane_color(), fg64=fg_masks(xyz, cams, H, W),
                fg_range=fg_mask_range(xyz, cams, H, W))


# every scene the GPU tests render, by name (the CPU test asserts the band cap on each)
TILE = 64
SCENES = {
    "F1": dict(F=1),
    "F5 uint8 frame": dict(F=5),
    "F5 float": dict(F=5, u8=False),
    "F5 per-frame K": dict(F=5, per_frame_K=True),
    "tile+1": dict(F=TILE + 1, seeing=(0, 1, 2, 3, TILE)),
    "R1": dict(F=5, R=1),
    "R65": dict(F=5, R=65),
    "R257": dict(F=5, R=257),
    "empty cloud": dict(F=5, n_points=0),
}
_BUILT = {}


def named_scene(name):
    if name not in _BUILT:
        _BUILT[name] = scene(**SCENES[name])
    return _BUILT[name]


def parallel_scene(R=70):
    """The F = 5 scene without its cloud (the origin lies inside the cloud) and
    a batch of rays parallel to the plane (dot is 0 up to rounding, far below
    1e-3): every ray takes the world origin, which four views see on the plane."""
    sc = dict(named_scene("empty cloud"))
    n = PLANE_NORMAL.astype(np.float64)
    a = np.cross(n, [0.0, 0.0, 1.0])
    b = np.cross(n, a)
    t = np.linspace(0, 2 * np.pi, R, endpoint=False)
    d = np.cos(t)[:, None] * a / np.linalg.norm(a) + np.sin(t)[:, None] * b / np.linalg.norm(b)
    sc["raydir"] = d.astype(np.float32)
    return sc


def no_fit_scene():
    """The F = 5 scene asked for a colour no image holds."""
    sc = dict(named_scene("F5 uint8 frame"))
    sc["plane_color"] = np.array([0.9, 0.1, 0.9], np.float32)
    return sc


SPECIAL = {"parallel": parallel_scene, "no view fits": no_fit_scene}


def any_scene(name):
    return SPECIAL[name]() if name in SPECIAL else named_scene(name)


# --------------------------------------------------------------- hand-built case
CORNER_H, CORNER_W = 29, 37


def corner_case():
    """One camera at (0, 0, -4) looking along +z, fx = fy = 4, principal point
    (16, 12); the plane z = 0 with normal (0, 0, 2); the rays through the
    continuous positions (u, v) of the list below.  Every operation is exact in
    fp32: the plane point of (u, v) projects back onto (u, v).  The image holds
    colours that all fit, so bg is the bilinear sample: at the four corner
    texels that texel's q / 255, outside the image zero: a quarter texel out,
    and 1/64 texel out, where a sample with u < W as the bound would still fit."""
    H, W = CORNER_H, CORNER_W
    K = np.array([[4.0, 0, 16.0], [0, 4.0, 12.0], [0, 0, 1.0]])
    pos, rot = np.array([[0.0, 0.0, -4.0]]), np.eye(3)[None]
    uv = np.array([[W - 1, H - 1], [0, 0], [W - 1, 0], [0, H - 1], [W - 0.75, H - 1], [W - 1, H - 0.75], [-0.25, 3],
                   [10.5, 7.25], [W - 1.5, H - 1], [W - 1 + 1 / 64, 5], [7, H - 1 + 1 / 64]], np.float64)
    raydir = np.stack([(uv[:, 0] - 16.0) / 4.0, (uv[:, 1] - 12.0) / 4.0, np.ones(len(uv))], -1).astype(np.float32)
    rng = np.random.default_rng(11)
    images = (COLOR_LEVELS[None, None, None, :] + rng.integers(-5, 6, (1, H, W, 3))).astype(np.uint8)
    from seed_ref import cam_table
    cams = cam_table(pos, rot, K)
    im = images[0].astype(np.float32) / np.float32(255)
    want = np.zeros((len(uv), 3), np.float32)
    for i, (x, y) in enumerate([(W - 1, H - 1), (0, 0), (W - 1, 0), (0, H - 1)]):
        want[i] = im[y, x]
    want[7] = bilinear(im[None], 0, np.float32(10.5), np.float32(7.25), np.float32)
    want[8] = bilinear(im[None], 0, np.float32(W - 1.5), np.float32(H - 1), np.float32)
    return dict(F=1, H=H, W=W, campos=pos[0].astype(np.float32), campos_f=pos, camrot_f=rot, K=K, cams=cams,
                images=images, raydir=raydir, uv=uv, plane_pnt=np.array([0.5, 0.25, 0.0], np.float32),
                plane_normal=np.array([0.0, 0.0, 2.0], np.float32), plane_color=plane_color(), want=want,
                xyz=np.zeros((0, 3), np.float32))


# ------------------------------------------------------------------ comparison
def twin_of(sc):
    """The fp32 evaluation of a scene, masks included."""
    fg32 = fg_masks(sc["xyz"], sc["cams"], sc["H"], sc["W"], np.float32)
    return evaluate(sc["campos"], sc["raydir"], sc["plane_pnt"], sc["plane_normal"], sc["plane_color"], sc["cams"],
                    sc["images"], fg32, np.float32), fg32


BANDED_TOL = 1e-4   # a banded ray against an admissible fp64 answer: the sample is 1-Lipschitz per axis in the
#                     pixel position for a [0, 1] image and |du| is a few ulp of 37 px (test_gpu_seed.py's reasoning)


def compare(name, who, sc, got_bg, got_fg=None, given_fg=None):
    """got_bg [R,3] (and got_fg [F,H,W]) of ``who`` against the fp64 reference
    by the rule of DESIGN.md 35; prints one RATIO line, asserts, returns the
    (error) / (twin error) ratio.  given_fg: the masks the caller handed in (the
    reference then uses exactly those)."""
    H, W = sc["H"], sc["W"]
    if given_fg is None:
        fg_lo, fg_hi = sc["fg_range"]
        fg64 = sc["fg64"]
    else:
        fg_lo = fg_hi = fg64 = np.asarray(given_fg, bool)
    args = (sc["campos"], sc["raydir"], sc["plane_pnt"], sc["plane_normal"], sc["plane_color"], sc["cams"],
            sc["images"])
    ref = evaluate(*args, fg64)
    banded, open_views = bands(ref, H, W, sc["plane_color"], fg_lo, fg_hi)
    share = float(banded.mean())
    assert share <= BAND_CAP, f"{name}: {share:.4f} of the rays are banded"
    if got_fg is not None:
        got_fg = np.asarray(got_fg, bool)
        assert not (fg_lo & ~got_fg).any(), f"{name}: a pixel every admissible mask has is missing"
        assert not (got_fg & ~fg_hi).any(), f"{name}: a pixel no admissible mask has is set"
    twin = evaluate(*args, fg64, np.float32)
    clear = ~banded
    # the twin's own error where it decided as fp64 did (it does everywhere outside the bands, asserted on the CPU)
    same = clear & (twin["used"] == ref["used"]).all(1)
    twin_err = float(np.abs(twin["bg"] - ref["bg"])[same].max(initial=0.0))
    bar = 4 * twin_err + ULP1
    got = np.asarray(got_bg, np.float64).reshape(-1, 3)
    err = float(np.abs(got - ref["bg"])[clear].max(initial=0.0))
    ratio = err / twin_err if twin_err > 0 else (0.0 if err == 0 else float("inf"))
    # the discrete part outside the bands: which rays are zero, exactly
    zero_ref = ~ref["used"].any(1)
    zero_got = ~got.any(1)
    wrong = clear & (zero_ref != zero_got)
    bad = 0
    alt = None
    if (np.abs(ref["dot"] - np.float64(DOT_EPS)) < DOT_BAND).any():
        alt = evaluate(*args, fg64, hit=~ref["hit"])
    for r in np.nonzero(banded)[0]:
        ok = admissible(ref, alt, open_views, r, got[r], BANDED_TOL)
        bad += ok is False
    print(f"RATIO {who:6s} {name:22s} R {len(got):4d} F {sc['F']:2d} banded {int(banded.sum()):2d} ({share:.4f}) "
          f"fit rays {int((~zero_ref).sum()):3d} err {err:.3e} twin {twin_err:.3e} err/twin {ratio:6.3f} "
          f"err/bar {err / bar:.4f} inadmissible {bad}")
    assert not wrong.any(), f"{name}: rays {np.nonzero(wrong)[0][:10]} decided differently outside the bands"
    assert err <= bar, f"{name}: |bg - fp64| {err:.3e} above the bar {bar:.3e} (twin {twin_err:.3e})"
    assert bad == 0, f"{name}: {bad} banded rays give no admissible answer"
    return ratio
