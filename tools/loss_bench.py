"""Dev tool: the finetune step with the reference's objective, two ways, in
bench.py --mode train's configuration (lego flags, 2 M points, 3600 random rays
of 800 x 800 frames, fp32h2, pnr_adam_step) with C_out = 3:

  A  the reference's formulation in torch ops on the output dict
     (tests/loss_ref.py, fp32: masked_select + MSELoss + the Python branches;
     conf_coefficient / weight from last_train_aux, which reads R'' on the host)
  B  pointnerf_amd.losses.RenderLoss (native, no host read)

Items: lego.sh's three colour items (weights 1 0 0) + 1e-4 x zero-one, with
sparse_loss_weight 0 and 1e-3.  Whole steps (forward, objective, backward,
Adam) are timed in alternating blocks of --block steps, A then B, in one
process; per block: host clock between two device synchronisations / steps.
Prints one JSON line per sparse weight: median and min-max of the blocks'
ms per step.

  --variant A|B|base --sparse W --profile-steps N   one variant only, N steps, no
      timing: the run to put under rocprofv3 --kernel-trace --stats (base = no
      objective: color.backward(ones), the launches the step has without one)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build(args, device, sparse_w):
    from pointnerf_amd import synthetic as S
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.optim import Adam
    from pointnerf_amd.options import flagset_opt
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
    opt = flagset_opt("lego", shading_color_channel_num=3, sparse_loss_weight=sparse_w)
    pts = S.lego_like_points(args.points, seed=0)
    emb, color, dirs, conf = S.point_features(args.points, seed=0, default_conf=opt.default_conf)
    torch.manual_seed(0)
    agg = PointAggregator(opt).to(device).train()
    np_ = NeuralPoints(opt, device, torch.from_numpy(pts), emb, color, dirs, conf)
    model = NeuralPointsRayMarching(opt, np_, agg)
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    return opt, model, Adam(params, lr=5e-4)


def cameras(n, H, W):
    from pointnerf_amd import synthetic as S
    cams = []
    for i in range(n):
        campos, camrot = S.camera(-180.0 + 360.0 * i / n, -30.0, 4.0)
        cams.append((campos, camrot, S.pixel_rays(H, W, S.lego_focal(H), camrot)))
    return cams


class Stepper:
    def __init__(self, args, device, sparse_w):
        import loss_ref
        from pointnerf_amd.losses import RenderLoss
        self.LR = loss_ref
        self.args, self.dev = args, device
        self.opt, self.model, self.optim = build(args, device, sparse_w)
        self.render_loss = RenderLoss(self.opt)
        H = W = args.hw
        self.HW = H * W
        self.cams = [tuple(torch.from_numpy(x).to(device) for x in c) for c in cameras(8, H, W)]
        self.bg = torch.from_numpy(np.random.default_rng(1).uniform(size=3).astype(np.float32)).to(device)
        self.target = torch.rand((self.HW, 3), generator=torch.Generator().manual_seed(2)).to(device)
        self.gen = torch.Generator(device=device).manual_seed(0)
        self.ones = torch.ones((args.rays, 3), device=device)
        self.i = 0

    def step(self, variant):
        opt, model = self.opt, self.model
        campos, camrot, rd = self.cams[self.i % len(self.cams)]
        self.i += 1
        sel = torch.randint(0, self.HW, (self.args.rays,), generator=self.gen, device=self.dev)
        self.optim.zero_grad(set_to_none=True)
        color, _, _, ray_mask = model.render_rays_train(campos, camrot, rd[sel], opt.near_plane, opt.far_plane,
                                                        self.bg)
        R = color.shape[0]
        out = dict(coarse_raycolor=color.view(1, R, 3), ray_mask=ray_mask.view(1, R))
        gt = self.target[sel].view(1, R, 3)
        if variant == "A":
            aux = model.last_train_aux          # what the reference's forward returns for these losses
            out["conf_coefficient"] = aux["conf_coefficient"]
            if opt.sparse_loss_weight > 0:
                out["weight"] = aux["weight"]
            total, _ = self.LR.compute_losses(opt, out, gt)
            total.backward()
        elif variant == "B":
            total, _ = self.render_loss(out, gt, model=model)
            total.backward()
        else:
            total = None
            color.backward(self.ones)
        self.optim.step()
        return total


def timed(args, device, sparse_w):
    st = Stepper(args, device, sparse_w)
    for _ in range(args.warmup):          # untimed blocks in the timed pattern: allocator and clocks settle
        for v in ("A", "B"):
            for _ in range(args.block):
                st.step(v)
    torch.cuda.synchronize()
    ms = {"A": [], "B": []}
    last = {}
    for _ in range(args.blocks):
        for v in ("A", "B"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.block):
                last[v] = st.step(v)
            torch.cuda.synchronize()
            ms[v].append((time.perf_counter() - t0) * 1e3 / args.block)
    line = {"metric": "finetune step with the reference objective, ms per step (fwd + objective + bwd + Adam)",
            "config": {"flags": "lego", "points": args.points, "rays": args.rays, "hw": args.hw, "C_out": 3,
                       "train_precision": st.model.train_precision, "optimizer": "pnr_adam_step",
                       "items": list(st.opt.color_loss_items), "color_loss_weights": list(st.opt.color_loss_weights),
                       "zero_one_loss_weights": list(st.opt.zero_one_loss_weights),
                       "sparse_loss_weight": sparse_w},
            "steps_per_variant": args.blocks * args.block, "block_steps": args.block, "warmup_blocks_each": args.warmup,
            "timing": "alternating blocks A, B in one process; host clock between device synchronisations"}
    for v, name in (("A", "A_reference_torch_ops"), ("B", "B_render_loss")):
        line[name] = {"median_ms": round(statistics.median(ms[v]), 4), "min_ms": round(min(ms[v]), 4),
                      "max_ms": round(max(ms[v]), 4), "blocks_ms": [round(x, 4) for x in ms[v]],
                      "last_loss": float(last[v].detach())}
    a, b = line["A_reference_torch_ops"], line["B_render_loss"]
    line["ranges_overlap"] = not (b["max_ms"] < a["min_ms"] or a["max_ms"] < b["min_ms"])
    line["B_median_not_above_A"] = b["median_ms"] <= a["median_ms"]
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--rays", type=int, default=3600)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=3, help="untimed blocks per variant before the timed ones")
    ap.add_argument("--blocks", type=int, default=8, help="timed blocks per variant")
    ap.add_argument("--block", type=int, default=4, help="steps per timed block")
    ap.add_argument("--sparse", type=float, nargs="+", default=[0.0, 1e-3])
    ap.add_argument("--variant", choices=("A", "B", "base"), default=None)
    ap.add_argument("--profile-steps", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_bench needs a ROCm GPU")
    device = torch.device("cuda:0")
    if args.variant is None:
        for w in args.sparse:
            timed(args, device, w)
        return
    st = Stepper(args, device, args.sparse[0])
    for _ in range(args.profile_steps):
        st.step(args.variant)
    torch.cuda.synchronize()
    print(json.dumps({"variant": args.variant, "sparse_loss_weight": args.sparse[0], "steps": args.profile_steps}))


if __name__ == "__main__":
    main()
