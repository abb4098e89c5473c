"""Independent restatement of the depth-map fusion contract (include/pnr.h,
DESIGN.md 25) in numpy: every valid pixel of every view against every other
view, the keep rule, the survivors.  Inputs are the fp32 values the device
holds (the camera table of rays_ref.cam_row, fp32 depths, fp32 thresholds),
widened to ``dtype``: float64 is the reference, float32 its twin, the same
operations in the same order with one fp32 rounding each, whose distance from
the reference is the yardstick of the device's."""
import numpy as np

import rays_ref as RR
import seed_ref as SR


# ------------------------------------------------------------- the geometry
def point(x, y, d, cam):
    """P(x, y, d) [...,3]: R (((x - cx0) / fx) d, ((y - cy0) / fy) d, d) + campos."""
    a = (x - cam[14]) / cam[12] * d
    b = (y - cam[15]) / cam[13] * d
    return np.stack([((cam[k * 3] * a + cam[k * 3 + 1] * b) + cam[k * 3 + 2] * d) + cam[9 + k] for k in range(3)], -1)


def cam_coords(p, cam):
    """c [...,3] = Rc2w^T (p - campos), summed left to right."""
    s = [p[..., k] - cam[9 + k] for k in range(3)]
    return np.stack([(s[0] * cam[j] + s[1] * cam[3 + j]) + s[2] * cam[6 + j] for j in range(3)], -1)


def project(c, cam):
    with np.errstate(divide="ignore", invalid="ignore"):
        return cam[12] * c[..., 0] / c[..., 2] + cam[14], cam[13] * c[..., 1] / c[..., 2] + cam[15]


def depth_ok(d):
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def sample(img, u, v):
    """(d_s, taps_ok): bilinear at (u, v), texel centres at + 0.5, taps clamped
    to the border; (u, v) must lie in the image."""
    H, W = img.shape
    one, half = img.dtype.type(1), img.dtype.type(0.5)
    sx, sy = u - half, v - half
    fx, fy = np.floor(sx), np.floor(sy)
    wx, wy = sx - fx, sy - fy
    x0, x1 = np.maximum(fx, 0).astype(np.int64), np.minimum(fx + 1, W - 1).astype(np.int64)
    y0, y1 = np.maximum(fy, 0).astype(np.int64), np.minimum(fy + 1, H - 1).astype(np.int64)
    t00, t01, t10, t11 = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    ok = depth_ok(t00) & depth_ok(t01) & depth_ok(t10) & depth_ok(t11)
    with np.errstate(invalid="ignore", over="ignore"):
        top = (one - wx) * t00 + wx * t01
        bot = (one - wx) * t10 + wx * t11
        return (one - wy) * top + wy * bot, ok


REASSIGN_BASE = 1.14869


def fuse(depths, cams, conf=None, mask=None, geo_cnsst_num=3, conf_thresh=0.0, pix_thresh=1.0, rel_thresh=0.01,
         ranges=None, reassign_conf=False, dtype=np.float64):
    """The whole contract.  Maps [F,H,W]: valid, count, visible, depth_avg,
    keep.  Per pair [F(r),F(s),H,W] (the diagonal r == s stays empty): vis,
    taps_ok (meaningful where vis), match, and u, v, dist, rel, cz2 (nan where
    not computed).  Survivors in (f, j, i) order: src_pixel, xyz, conf, count."""
    T = np.dtype(dtype).type
    dep = np.asarray(depths, np.float32).astype(dtype)
    cam = np.asarray(cams, np.float32).astype(dtype)
    F, H, W = dep.shape
    pix_t, rel_t, conf_t = (T(np.float32(t)) for t in (pix_thresh, rel_thresh, conf_thresh))
    jj, ii = np.mgrid[:H, :W]
    x, y = ii.astype(dtype) + T(0.5), jj.astype(dtype) + T(0.5)
    valid = depth_ok(dep)
    shape = (F, F, H, W)
    vis, taps_ok, match = (np.zeros(shape, bool) for _ in range(3))
    u_, v_, dist_, rel_, cz2_ = (np.full(shape, np.nan, dtype) for _ in range(5))
    count, visible = np.zeros((F, H, W), np.int64), np.zeros((F, H, W), np.int64)
    total = np.zeros((F, H, W), dtype)
    pts = np.zeros((F, H, W, 3), dtype)
    for r in range(F):
        ok = valid[r]
        d = np.where(ok, dep[r], T(1))
        p = point(x, y, d, cam[r])
        for s in range(F):
            if s == r:
                continue
            c1 = cam_coords(p, cam[s])
            u, v = project(c1, cam[s])
            see = ok & SR.inside(u, v, c1[..., 2], H, W)
            us, vs = np.where(see, u, T(0.5)), np.where(see, v, T(0.5))
            ds, tok = sample(dep[s], us, vs)
            go = see & tok
            ds = np.where(go, ds, T(1))
            c2 = cam_coords(point(us, vs, ds, cam[s]), cam[r])
            u2, v2 = project(c2, cam[r])
            with np.errstate(invalid="ignore", over="ignore"):
                du, dv = u2 - x, v2 - y
                dist = np.sqrt(du * du + dv * dv)
                rel = np.abs(c2[..., 2] - d) / d
                m = go & (c2[..., 2] > 0) & (dist < pix_t) & (rel < rel_t)
            vis[r, s], taps_ok[r, s], match[r, s] = see, tok, m
            u_[r, s], v_[r, s] = np.where(ok, u, np.nan), np.where(ok, v, np.nan)
            dist_[r, s], rel_[r, s], cz2_[r, s] = (np.where(go, a, np.nan) for a in (dist, rel, c2[..., 2]))
            visible[r] += see
            count[r] += m
            total[r] = total[r] + np.where(m, c2[..., 2], T(0))      # ascending s
        avg = (d + total[r]) / (count[r] + 1).astype(dtype)
        total[r] = np.where(ok, avg, T(0))
        pts[r] = point(x, y, total[r], cam[r])
    depth_avg = total
    keep = valid.copy()
    if F > 1:
        keep &= count >= int(geo_cnsst_num)
    cf = None
    if conf is not None:
        cf = np.asarray(conf, np.float32).astype(dtype)
        with np.errstate(invalid="ignore"):
            keep &= cf > conf_t
    if mask is not None:
        keep &= np.asarray(mask) != 0
    if ranges is not None and np.float32(ranges[0]) > -99:
        box = np.asarray(ranges, np.float32).astype(dtype)
        with np.errstate(invalid="ignore"):
            keep &= np.all((pts >= box[:3]) & (pts <= box[3:]), -1)
    src = np.nonzero(keep.reshape(-1))[0]
    out_conf = cf.reshape(-1)[src] if cf is not None else np.ones(len(src), dtype)
    cnt = count.reshape(-1)[src]
    if reassign_conf:
        factor = (1.0 - 1.0 / REASSIGN_BASE ** np.clip(cnt - int(geo_cnsst_num) + 1, 1, 10)).astype(np.float32)
        out_conf = out_conf * factor.astype(dtype)
    return dict(valid=valid, count=count, visible=visible, depth_avg=depth_avg, keep=keep, points=pts, vis=vis,
                taps_ok=taps_ok, match=match, u=u_, v=v_, dist=dist_, rel=rel_, cz2=cz2_, src_pixel=src,
                xyz=pts.reshape(-1, 3)[src], conf=out_conf, count_out=cnt)


# ------------------------------------------------------------------ the bands
PIX_BAND, REL_BAND, EDGE_BAND = 1e-3, 1e-5, 1e-4


def banded(ref, W, H, pix_thresh=1.0, rel_thresh=0.01):
    """[F,H,W] bool: pixels with a pair that fp64 itself puts within reach of an
    fp32 rounding: |dist - pix_thresh| < 1e-3 px, |rel - rel_thresh| < 1e-5, or
    u or v within 1e-4 px of 0, W or H."""
    pix_t, rel_t = np.float64(np.float32(pix_thresh)), np.float64(np.float32(rel_thresh))
    with np.errstate(invalid="ignore"):
        near = (np.abs(ref["dist"] - pix_t) < PIX_BAND) | (np.abs(ref["rel"] - rel_t) < REL_BAND)
        for a, n in ((ref["u"], W), (ref["v"], H)):
            near |= (np.abs(a) < EDGE_BAND) | (np.abs(a - n) < EDGE_BAND)
    return near.any(1)


def twin_errors(ref, twin, pix_thresh=1.0, rel_thresh=0.01, reach=10.0):
    """(max |du| or |dv| over visible pairs, max |ddist| over pairs with |dist -
    pix_thresh| < reach PIX_BAND, max |drel| over pairs with |rel - rel_thresh|
    < reach REL_BAND) between a float32 run and the fp64 reference: the errors
    of the pairs a rounding could move across a threshold.  Away from the
    thresholds the error of dist and rel is as large as the pair is
    ill-conditioned (a sample on a silhouette turns 1e-5 px of u into 5e-4 px of
    dist; where cz'' passes through 0 dist runs into the thousands of pixels)
    and decides nothing."""
    with np.errstate(invalid="ignore"):
        du = np.maximum(np.abs(twin["u"] - ref["u"]), np.abs(twin["v"] - ref["v"]))[ref["vis"]].max(initial=0.0)
        dd = np.abs(twin["dist"] - ref["dist"])[np.abs(ref["dist"] - pix_thresh) < reach * PIX_BAND].max(initial=0.0)
        dr = np.abs(twin["rel"] - ref["rel"])[np.abs(ref["rel"] - rel_thresh) < reach * REL_BAND].max(initial=0.0)
    return float(du), float(dd), float(dr)


# ------------------------------------------------------------------ the scene
def ring(F, radius=2.0, z0=0.3, z1=0.4):
    """F cameras on the circle of ``radius`` in the xy plane, azimuth 2 pi f / F,
    at heights z0 + (z1 - z0) f / F, looking at the origin with z up.
    Returns campos [F,3], camrotc2w [F,3,3] (columns right, down, forward)."""
    pos, rot = [], []
    for f in range(F):
        az = 2 * np.pi * f / F
        c = np.array([radius * np.cos(az), radius * np.sin(az), z0 + (z1 - z0) * f / F])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        right /= np.linalg.norm(right)
        pos.append(c)
        rot.append(np.stack([right, np.cross(fwd, right), fwd], 1))
    return np.array(pos), np.array(rot)


def analytic_depths(cams, H, W, sphere=0.5, plane=-0.5, far=6.0):
    """[F,H,W] fp64: camera-space z of the first hit of each pixel-centre ray
    with the sphere of radius ``sphere`` at the origin or the plane z =
    ``plane``; 0 where nothing is hit or the depth is beyond ``far``."""
    cams = np.asarray(cams, np.float32).astype(np.float64)
    jj, ii = np.mgrid[:H, :W]
    out = np.zeros((len(cams), H, W))
    for f, cam in enumerate(cams):
        R, o = cam[:9].reshape(3, 3), cam[9:12]
        dc = np.stack([(ii + 0.5 - cam[14]) / cam[12], (jj + 0.5 - cam[15]) / cam[13], np.ones((H, W))], -1)
        dw = dc @ R.T                                   # world direction per unit depth
        t = np.full((H, W), np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            tp = (plane - o[2]) / dw[..., 2]
        t = np.where(tp > 0, tp, t)
        a, b, c = (dw * dw).sum(-1), 2 * (dw @ o), o @ o - sphere ** 2
        disc = b * b - 4 * a * c
        with np.errstate(invalid="ignore"):
            ts = (-b - np.sqrt(disc)) / (2 * a)
        t = np.where((disc >= 0) & (ts > 0) & (ts < t), ts, t)
        out[f] = np.where(t <= far, t, 0.0)
    return out


def scene(F=8, H=48, W=64, focal=60.0, perturb=True, conf_seed=None):
    """The fusion tests' scene: F ring cameras of radius 2 at heights 0.3 to
    0.4, a sphere of radius 0.5 over the plane z = -0.5, depth beyond 6
    invalid; view 3 scaled by 1.02, view 5 multiplied by 1 + 0.012 sin(i / 5)
    cos(j / 7) (when F has them); depths rounded to fp32.  conf_seed: also a
    uniform [0, 1) confidence map."""
    campos, camrot = ring(F)
    K = RR.focal_K(focal, H, W)
    cams = SR.cam_table(campos, camrot, K)
    dep = analytic_depths(cams, H, W)
    if perturb and F > 3:
        dep[3] *= 1.02
    if perturb and F > 5:
        jj, ii = np.mgrid[:H, :W]
        dep[5] *= 1 + 0.012 * np.sin(ii / 5) * np.cos(jj / 7)
    s = dict(depths=dep.astype(np.float32), campos=campos, camrot=camrot, K=K, cams=cams, F=F, H=H, W=W)
    if conf_seed is not None:
        s["conf"] = np.random.default_rng(conf_seed).random((F, H, W), dtype=np.float32)
    return s


# ------------------------------------------------------------ hand-built cases
HAND_H, HAND_W = 6, 8
HAND_K = SR.HAND_K   # u = 4 cx / cz + 4, v = 4 cy / cz + 3


def hand_cases():
    """name -> dict(depths, campos, camrot, cams, kwargs, and the expected maps
    worked out by hand: count, visible, depth_avg, keep where given).  The
    cameras look along +z at the plane z = 0, x right and y down."""
    H, W = HAND_H, HAND_W

    def setup(cameras, depths, **kw):
        pos, rot = (np.array(v) for v in zip(*cameras))
        return dict(campos=pos, camrot=rot, cams=SR.cam_table(pos, rot, HAND_K),
                    depths=np.asarray(depths, np.float32), kwargs=kw)

    def cam(x=0.0, z=-4.0):
        return np.array([x, 0.0, z]), np.eye(3)

    cases = {}
    # Two fronto-parallel cameras one unit apart, the plane at depth 4: pixel (i, j) of view 0 lands on
    # (i + 0.5 - 1, j + 0.5) of view 1 (a pixel centre: weights 1 and 0) and comes back exactly.  Column 0 of
    # view 0 and column 7 of view 1 leave the other image.
    flat = np.full((2, H, W), 4.0)
    inner0, inner1 = np.zeros((H, W), int), np.zeros((H, W), int)
    inner0[:, 1:], inner1[:, :-1] = 1, 1
    both = np.stack([inner0, inner1])
    cases["plane"] = dict(setup([cam(0.0), cam(1.0)], flat, geo_cnsst_num=1), count=both, visible=both,
                          depth_avg=flat, keep=both.astype(bool))
    # view 1 reports 1.02 x the depth: |cz'' - d| / d = 0.02 either way, no match; still visible
    scaled = flat.copy()
    scaled[1] *= 1.02
    cases["scaled"] = dict(setup([cam(0.0), cam(1.0)], scaled, geo_cnsst_num=1), count=0 * both, visible=both,
                           depth_avg=scaled, keep=np.zeros((2, H, W), bool))
    # cameras half a unit apart: view 0's pixel (i, j) lands on u = i, half-way between texels i - 1 and i of
    # view 1 (at u = 0 both clamp to texel 0), v = j + 0.5 on rows j and j + 1 with weights 1 and 0.  Texel
    # (3, 2) of view 1 is invalid, so pixels i = 3, 4 of rows j = 1, 2 of view 0, whose taps straddle it, have
    # no match (a tap of weight 0 counts); the reference's blend with zero would give depth 2 on row 2.
    hole = flat.copy()
    hole[1, 2, 3] = 0.0
    cnt = np.ones((2, H, W), int)
    cnt[0, 1:3, 3:5] = 0
    cnt[1, 2, 3] = 0           # the invalid pixel itself
    cnt[1, :, 7] = 0           # u = 8 = W: outside view 0
    vis = np.ones((2, H, W), int)
    vis[1, 2, 3] = 0
    vis[1, :, 7] = 0
    cases["straddle"] = dict(setup([cam(0.0), cam(0.5)], hole, geo_cnsst_num=1), count=cnt, visible=vis,
                             keep=cnt.astype(bool))
    # view 1 stands beyond the plane, looking the same way: every point of view 0 is behind it (cz' = -1), not
    # visible.  View 1's points (z = 5) are visible in view 0, whose depth brings them back to the plane, behind
    # view 1 (cz'' = -1): no match.
    seen = np.stack([np.zeros((H, W), int), np.ones((H, W), int)])
    cases["behind"] = dict(setup([cam(0.0), cam(0.0, 1.0)], flat, geo_cnsst_num=1), count=0 * both, visible=seen,
                           depth_avg=flat, keep=np.zeros((2, H, W), bool))
    # one view: nothing to agree with, every valid pixel is kept at its own depth
    single = np.full((1, H, W), 4.0)
    single[0, 0, 0], single[0, 1, 1], single[0, 2, 2] = 0.0, np.nan, np.inf
    ok = np.ones((1, H, W), bool)
    ok[0, 0, 0] = ok[0, 1, 1] = ok[0, 2, 2] = False
    cases["single"] = dict(setup([cam(0.0)], single), count=np.zeros((1, H, W), int), visible=np.zeros((1, H, W), int),
                           depth_avg=np.where(ok, 4.0, 0.0), keep=ok)
    return cases
