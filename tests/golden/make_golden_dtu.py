"""Generate tests/golden/aggregator_dtu.npz from the REFERENCE PointAggregator.

Like make_golden.py (which stays as it is) this runs only where the reference
tree is mounted; it imports the reference's own PointAggregator, overwrites its
parameters with formula_params (block1.0 shaped (256, 7E + 60)) and records
inputs and outputs -- data only, loaded with numpy (allow_pickle=False).

The DTU scripts' aggregator flags (dev_scripts/dtu_test_inf/*.sh, dev_scripts/ete/
dtu_dgt_d012_img0123_conf_color_dir_agg2.sh): point_features_dim 63 with
agg_intrp_order 1 and 2 on one set of gathered inputs (keys a_*), and
point_features_dim 32 with agg_intrp_order 1 on a second set (keys b_*).
R, SR, K = 6, 10, 8 with a ray without neighbours, an empty sample and
single-neighbour samples, as aggregator.npz has.

    python tests/golden/make_golden_dtu.py --ref <reference tree>
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from formula import LEGO_SHAPES, formula_params  # noqa: E402
from make_golden import lego_agg_opt  # noqa: E402

SALT = 0.2


def dtu_agg_opt(E, order):
    o = lego_agg_opt()
    o.point_features_dim, o.agg_intrp_order = E, order
    return o


def gathered(rng, E, R=6, SR=10, K=8):
    mask = rng.uniform(size=(1, R, SR, K)) < 0.7
    mask[0, 0, :, :] = False          # a ray with no neighbours at all
    mask[0, 1, 3, :] = False          # an empty sample
    mask[0, 2, :, 1:] = False         # single-neighbour samples
    sloc_w = rng.uniform(-0.5, 0.5, size=(1, R, SR, 3)).astype(np.float32)
    campos = np.array([0.2, -3.8, 1.7], np.float32)
    rot = np.array([[0.99, 0.1, 0.0], [0.0, 0.3, -0.95], [-0.1, 0.95, 0.3]], np.float32)
    sxyz = (sloc_w[..., None, :] + rng.normal(scale=0.008, size=(1, R, SR, K, 3))).astype(np.float32)

    def pers(p):
        xc = (p - campos) @ rot
        return np.stack([xc[..., 0] / xc[..., 2], xc[..., 1] / xc[..., 2], xc[..., 2]], -1).astype(np.float32)

    return dict(
        sampled_color=rng.normal(size=(1, R, SR, K, 3)).astype(np.float32),
        sampled_dir=rng.normal(size=(1, R, SR, K, 3)).astype(np.float32),
        sampled_conf=rng.uniform(-0.2, 1.3, size=(1, R, SR, K, 1)).astype(np.float32),
        sampled_embedding=rng.uniform(-0.5, 0.5, size=(1, R, SR, K, E)).astype(np.float32),
        sampled_xyz_pers=pers(sxyz), sampled_xyz=sxyz, sample_pnt_mask=mask,
        sample_loc=pers(sloc_w), sample_loc_w=sloc_w,
        sample_ray_dirs=np.ascontiguousarray(np.broadcast_to(rng.normal(size=(1, R, 1, 3)), (1, R, SR, 3))).astype(np.float32))


def run(PointAggregator, E, order, inputs):
    agg = PointAggregator(dtu_agg_opt(E, order))
    params = formula_params(dict(LEGO_SHAPES, **{"block1.0": (256, 7 * E + 60)}), salt=SALT)
    sd = agg.state_dict()
    assert set(sd.keys()) == set(params.keys()), (sorted(sd.keys()), sorted(params.keys()))
    for k in sd:
        assert tuple(sd[k].shape) == params[k].shape, (k, sd[k].shape, params[k].shape)
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in inputs.items()}
    with torch.no_grad():
        feats, ray_valid, weight, conf = agg(t["sampled_color"], torch.eye(3), t["sampled_dir"], t["sampled_conf"],
                                             t["sampled_embedding"], t["sampled_xyz_pers"], t["sampled_xyz"],
                                             t["sample_pnt_mask"], t["sample_loc"], t["sample_loc_w"],
                                             t["sample_ray_dirs"], [0.004, 0.004, 0.004], 0)
    return feats.numpy(), ray_valid.numpy(), weight.numpy(), conf.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference tree (holds models/)")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    from models.aggregators.point_aggregators import PointAggregator

    torch.set_num_threads(1)
    rng = np.random.default_rng(6363)
    out = {"salt": np.float32(SALT)}
    a = gathered(rng, 63)
    f2, rv, w, cf = run(PointAggregator, 63, 2, a)
    f1, rv1, w1, cf1 = run(PointAggregator, 63, 1, a)
    assert np.array_equal(rv, rv1) and np.array_equal(w, w1) and np.array_equal(cf, cf1)
    out.update({"a_" + k: v for k, v in a.items()})
    out.update(a_features_o2=f2, a_features_o1=f1, a_ray_valid=rv, a_weight=w, a_conf_coefficient=cf)
    b = gathered(rng, 32)
    g1, rvb, wb, cfb = run(PointAggregator, 32, 1, b)
    out.update({"b_" + k: v for k, v in b.items()})
    out.update(b_features_o1=g1, b_ray_valid=rvb, b_weight=wb, b_conf_coefficient=cfb)
    path = os.path.join(HERE, "aggregator_dtu.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
