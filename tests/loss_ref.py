"""compute_losses of the reference (models/base_rendering_model.py:533-664) in
torch ops, written from its lines: the colour items with the same
``masked_select`` / ``MSELoss`` calls and the Python branch on the selected
count, the zero-one items (:630-641) and the sparse loss (:652-662).  The
reference module itself cannot be imported here (it pulls in torchvision).

Run in float64 it is the truth the GPU tests measure against; run in float32 it
is the yardstick (the reference's own arithmetic): ``within`` is the rule of
DESIGN.md 19 -- an error of at most 4 x the fp32 restatement's own error vs fp64,
plus one fp32 ulp of the value (for a tensor, of its largest entry)."""
import numpy as np
import torch

FP32_ULP = float(np.finfo(np.float32).eps)   # 2^-23: the spacing of fp32 numbers in [1, 2)


def mse2psnr(x):
    return -10. * torch.log(x) / np.log(10.)     # :17


def color_item(name, output, gt_image, ray_depth_mask=None):
    """One colour item of :542-606 -> its loss.  ray_depth_mask: the per-ray
    boolean the reference gathers at :565-566."""
    l2loss = torch.nn.MSELoss()
    C = gt_image.shape[-1]    # the reference hard-codes 3 in its expand
    if name.startswith("ray_masked"):
        unmasked_name = name[len("ray_masked") + 1:]
        sel = (output["ray_mask"] > 0)[..., None].expand(-1, -1, C)
        masked_output = torch.masked_select(output[unmasked_name], sel).reshape(1, -1, C)
        masked_gt = torch.masked_select(gt_image, sel).reshape(1, -1, C)
        if masked_output.shape[1] > 0:
            return l2loss(masked_output, masked_gt)
        return torch.tensor(0.0, dtype=torch.float32, device=masked_output.device)
    if name.startswith("ray_miss"):
        unmasked_name = name[len("ray_miss") + 1:]
        sel = (output["ray_mask"] == 0)[..., None].expand(-1, -1, C)
        masked_output = torch.masked_select(output[unmasked_name], sel).reshape(1, -1, C)
        masked_gt = torch.masked_select(gt_image, sel).reshape(1, -1, C)
        if masked_output.shape[1] > 0:
            return l2loss(masked_output, masked_gt) * masked_gt.shape[1]
        return torch.tensor(0.0, dtype=torch.float32, device=masked_output.device)
    if name.startswith("ray_depth_masked"):
        unmasked_name = name[len("ray_depth_masked") + 1:]
        sel = (ray_depth_mask.reshape(1, -1) > 0)[..., None].expand(-1, -1, C)
        masked_output = torch.masked_select(output[unmasked_name], sel).reshape(1, -1, C)
        masked_gt = torch.masked_select(gt_image, sel).reshape(1, -1, C)
        return l2loss(masked_output, masked_gt)       # NaN for an empty selection
    return l2loss(output[name], gt_image)


def zero_one_item(val, zero_epsilon):
    v = torch.clamp(val, zero_epsilon, 1 - zero_epsilon)     # :636-639
    return torch.mean(torch.log(v) + torch.log(1 - v))


def sparse_item(weight, conf_coefficient):
    return torch.sum(weight * torch.abs(1 - torch.exp(-2 * conf_coefficient))) / (torch.sum(weight) + 1e-6)   # :657


def broadcast_weights(weights, n):
    """check_setup_loss (:227-234): one weight stands for every item."""
    w = [float(x) for x in weights]
    if len(w) == 1 and n > 1:
        w = w * n
    assert len(w) == n
    return w


def compute_losses(opt, output, gt_image, ray_depth_mask=None):
    """-> (loss_total, {"loss_<name>": tensor}) for the colour, zero-one and
    sparse parts, in the dtype of the tensors it is given."""
    losses = {}
    loss_total = 0
    cw = broadcast_weights(opt.color_loss_weights, len(opt.color_loss_items))
    for i, name in enumerate(opt.color_loss_items):
        loss = color_item(name, output, gt_image, ray_depth_mask)
        loss_total = loss_total + (loss * cw[i] + 1e-6)
        losses["loss_" + name] = loss
    items = list(getattr(opt, "zero_one_loss_items", []) or [])
    zw = broadcast_weights(getattr(opt, "zero_one_loss_weights", [1.0]), len(items)) if items else []
    for i, name in enumerate(items):
        if name not in output:
            continue
        loss = zero_one_item(output[name], opt.zero_epsilon)
        loss_total = loss_total + loss * zw[i]
        losses["loss_" + name] = loss
    if getattr(opt, "sparse_loss_weight", 0) > 0:
        loss = sparse_item(output["weight"], output["conf_coefficient"])
        loss_total = loss_total + loss * opt.sparse_loss_weight
        losses["loss_sparse"] = loss
    return loss_total, losses


def cast(output, dtype):
    """The dict's floating tensors in ``dtype`` (masks and non-tensors as they are)."""
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in output.items()}


def within(got, ref64, yard32, what=""):
    """The yardstick rule; returns the measured ratio err / allowed and asserts
    it is <= 1.  Every entry is compared (the maxima run over the whole tensor)."""
    g = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    r = torch.as_tensor(ref64).detach().double().cpu().reshape(-1)
    y = torch.as_tensor(yard32).detach().double().cpu().reshape(-1)
    assert g.shape == r.shape == y.shape, (what, g.shape, r.shape, y.shape)
    assert bool(torch.isfinite(g).all()), (what, "non-finite value")
    if g.numel() == 0:
        return 0.0
    err = float((g - r).abs().max())
    yerr = float((y - r).abs().max())
    big = float(r.abs().max())
    ulp = FP32_ULP * 2.0 ** np.floor(np.log2(big)) if big > 0 else 0.0
    allowed = 4.0 * yerr + ulp
    ratio = err / allowed if allowed > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{what}: err {err:.3e} yardstick {yerr:.3e} ulp {ulp:.3e} ratio {ratio:.3f}")
    assert err <= allowed, (what, err, yerr, ulp)
    return ratio
