"""numpy restatement of the point-growing probe
(models/neural_points_volumetric_model_ori.py:351-372): the checker of pnr_probe
and of NeuralPointsRayMarching's opt.prob == 1 outputs in the tests (test
infrastructure, not product code).  float64 is the reference; the same code with
dtype=float32 is the yardstick the tests derive their tolerances from."""
import numpy as np

from oracle import oracle as O

KEYS = ("ray_max_shading_opacity", "ray_max_sample_loc_w", "ray_max_far_dist", "shading_avg_color",
        "shading_avg_dir", "shading_avg_conf", "shading_avg_embedding")


def oracle_inputs(opt, points, params, campos, camrot, raydir, bg):
    """The CPU oracle's query, gather, aggregate (w, confc) and composite opacity
    of one scene -- what probe_maps_ref reads; computed once per scene."""
    q = O.query_points(opt, points["xyz"], campos, camrot, raydir, near=opt.near_plane, far=opt.far_plane)
    g = O.gather(points, q["sample_pidx"], campos, camrot)
    neg = 0.01 if opt.act_type == "LeakyReLU" else 0.0
    feats, rv, w, confc = O.aggregate(params, g["sampled_color"], g["sampled_Rw2c"], g["sampled_dir"],
                                      g["sampled_conf"], g["sampled_embedding"], g["sampled_xyz_pers"],
                                      g["sampled_xyz"], g["sample_pnt_mask"], q["sample_loc"], q["sample_loc_w"],
                                      q["sample_ray_dirs"], neg_slope=neg, act_super=opt.act_super,
                                      C=opt.shading_color_channel_num)
    rd = O.ray_dist(q["sample_loc"], rv, opt.vsize[2], opt.raydist_mode_unit)
    opacity = O.ray_march(rd, rv, feats, bg)[2]
    R = q["ray_mask"].shape[0]
    op_full = np.zeros((R, opt.SR), np.float32)
    op_full[q["ray_mask"] > 0] = opacity
    return dict(q=q, g=g, w=w, confc=confc, opacity=op_full)


def probe_maps_ref(q, g, w, confc, opacity, dtype=np.float64, emb_table=None):
    """The seven outputs in full ray order [R, C] (zeros for ray_mask == 0; None
    for an absent table) plus s_star [R] (-1 for ray_mask == 0).

    q: O.query_points(...); g: O.gather(...); w, confc [R'',SR,K]: O.aggregate's
    normalised weight and clamped confidence; opacity [R,SR] fp32 (full ray
    order).  torch.max's index is pinned to the lowest slot among equal maxima
    (np.argmax).  Empty slots (pidx -1) gather point 0 -- O.gather clamps like
    neural_points.py:790 -- and are not masked in the distance.  emb_table
    [N,32]: gather the embedding from this table instead of g's."""
    mask = q["ray_mask"] > 0
    R = mask.shape[0]
    op = np.asarray(opacity, np.float32)[mask]                      # [R'',SR]
    rows = np.arange(op.shape[0])
    s = np.argmax(op, axis=-1) if op.shape[0] else np.zeros(0, np.int64)
    loc = q["sample_loc_w"][rows, s]                                # [R'',3] fp32 (0 for unfilled slots)
    wk = (np.asarray(w, np.float32)[rows, s].astype(dtype) * np.asarray(confc, np.float32)[rows, s].astype(dtype))
    d = g["sampled_xyz"][rows, s].astype(dtype) - loc[:, None, :].astype(dtype)
    far = np.sqrt((d * d).sum(-1, dtype=dtype)).astype(dtype).min(-1)

    def avg(x):
        if x is None:
            return None
        return (x[rows, s].astype(dtype) * wk[..., None]).sum(-2, dtype=dtype).astype(dtype)

    emb = g["sampled_embedding"]
    if emb_table is not None:
        emb = np.asarray(emb_table, np.float32)[np.clip(q["sample_pidx"], 0, None)]
    part = dict(ray_max_shading_opacity=op[rows, s][:, None], ray_max_sample_loc_w=loc,
                ray_max_far_dist=far[:, None], shading_avg_color=avg(g["sampled_color"]),
                shading_avg_dir=avg(g["sampled_dir"]), shading_avg_conf=avg(g["sampled_conf"]),
                shading_avg_embedding=avg(emb))
    out = {}
    for k, v in part.items():
        if v is None:
            out[k] = None
            continue
        full = np.zeros((R, v.shape[-1]), v.dtype)
        full[mask] = v
        out[k] = full
    s_full = np.full(R, -1, np.int64)
    s_full[mask] = s
    out["s_star"] = s_full
    return out


def compare(got, ref64, ref32, margin=4.0, what=""):
    """The tests' rule.  ray_max_shading_opacity and ray_max_sample_loc_w are
    copies: bit-equal.  Every other tensor: max |got - ref64| <= margin * max
    |ref32 - ref64| + one fp32 ulp of max |ref64| (margin 4: another order of the
    K-sum and FMA contraction).  Every ray takes part.  Prints both errors and
    returns {key: (err_got, err_twin)}."""
    res = {}
    for k in KEYS:
        if ref64[k] is None:
            assert got[k] is None, f"{what} {k}: expected None"
            continue
        a = np.asarray(got[k]).reshape(ref64[k].shape)
        if k in ("ray_max_shading_opacity", "ray_max_sample_loc_w"):
            assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), ref64[k].view(np.uint32)), \
                f"{what} {k}: not bit-equal ({int((a != ref64[k]).sum())} values differ)"
            continue
        e_got = float(np.max(np.abs(a.astype(np.float64) - ref64[k]), initial=0.0))
        e_twin = float(np.max(np.abs(ref32[k].astype(np.float64) - ref64[k]), initial=0.0))
        ulp = float(np.spacing(np.float32(np.max(np.abs(ref64[k]), initial=0.0))))
        print(f"{what} {k}: err {e_got:.3e}  fp32 twin {e_twin:.3e}  ratio "
              f"{e_got / e_twin if e_twin else float('inf'):.2f}  ulp(max) {ulp:.3e}")
        res[k] = (e_got, e_twin)
        assert e_got <= margin * e_twin + ulp, f"{what} {k}: {e_got:.3e} > {margin} * {e_twin:.3e} + {ulp:.3e}"
    return res
