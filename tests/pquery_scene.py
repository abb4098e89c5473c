"""The small perspective-query scene shared by the pquery tests (inputs only):
lego-like points seen from camera(30, -30, 4) in a W x H = 40 x 32 frame,
near 2, far 6, z_depth_dim 128, P 24."""
import numpy as np

from oracle import oracle as O
from pointnerf_amd import synthetic as S
from pointnerf_amd.options import lego_opt


def popt(**over):
    o = dict(wcoord_query=0, vscale=[2, 2, 1], kernel_size=[3, 3, 3], query_size=[0, 0, 0], SR=24, K=8, P=24, NN=2,
             radius_limit_scale=0.0, depth_limit_scale=0.0, z_depth_dim=128, shpnt_jitter="passfunc", grid_seed=0)
    o.update(over)
    return lego_opt(**o)


def pscene(n_points=4000, W=40, H=32, theta=30.0, seed=0, cx=None, cy=None, **opt_over):
    opt = popt(**opt_over)
    xyz = S.lego_like_points(n_points, seed=seed) if n_points else np.zeros((0, 3), np.float32)
    campos, camrot = S.camera(theta, -30.0, 4.0)
    focal = S.lego_focal(800) * 40 / 800
    intrinsic = np.array([[focal, 0, W / 2 if cx is None else cx], [0, focal, H / 2 if cy is None else cy],
                          [0, 0, 1]], np.float32)
    px, py = np.meshgrid(np.arange(W, dtype=np.int32), np.arange(H, dtype=np.int32))
    pixel_idx = np.stack([px, py], -1).reshape(-1, 2)       # (column, row), row-major frame
    pers = O.w2pers(xyz, campos, camrot) if n_points else np.zeros((0, 3), np.float32)
    return dict(opt=opt, xyz=xyz, pers=pers, campos=campos, camrot=camrot, intrinsic=intrinsic, pixel_idx=pixel_idx,
                W=W, H=H, near=2.0, far=6.0)
