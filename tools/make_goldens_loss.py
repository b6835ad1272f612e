#!/usr/bin/env python
"""Golden vectors for the training loss and the regression-head backward: what the REFERENCE's training step computes.

The reference's network (train_codes/Depth_Estimation_Network.py, imported where it lies, train mode, untrained) runs one forward on a
random stack; forward hooks on DFF_net.confidence / classif1 / classif2 / classif3 keep the four score volumes and retain their
gradients.  The loss is the training scripts' own text: masked_MSE_loss is compiled from train_code_Defocus.py:17-19 (plain, ranged) and
train_code_Smartphone.py:17-19 (conf), and the loss lines train_code_Defocus.py:160-165, train_code_FlyingThings.py:168-179 and
train_code_Smartphone.py:126-132 are compiled and executed in place, then Total_Loss.backward().

Stored per case (arrays only, tests/golden/loss_<case>.npz): score0..3 (the hooked volumes, squeezed to (B,N,h,w)), focus_dists, gt, mask,
conf, pred0..3 (mid_out, pred1, pred2, pred3), losses (mid, 1, 2, 3, total), grad0..3 (the .grad of the hooked volumes), weights, range.
The consumers feed the stored score volumes to the kernel / tests/loss_ref.py, so the goldens do not depend on how the network upstream ran.

usage: python tools/make_goldens_loss.py [REFERENCE_ROOT]     (default /root/reference)"""
import importlib.util
import os
import sys
import textwrap

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
TC = os.path.join(REF, "train_codes")

# case -> (script holding masked_MSE_loss, its lines, script holding the loss lines, their lines, B, N, H, W, range or None, conf, sentinel, seed)
CASES = {
    "plain": ("train_code_Defocus.py", (17, 19), "train_code_Defocus.py", (160, 165), 2, 3, 64, 96, None, False, float("nan"), 11),
    "ranged": ("train_code_Defocus.py", (17, 19), "train_code_FlyingThings.py", (168, 179), 2, 5, 32, 64, (10.0, 100.0), False, -3.0, 12),
    "ranged_conf": ("train_code_Smartphone.py", (17, 19), "train_code_Smartphone.py", (126, 132), 2, 3, 32, 64,
                    (1 / 3.91092, 1 / 0.10201), True, float("nan"), 13),
}


def compiled(script, first, last):
    path = os.path.join(TC, script)
    lines = open(path).read().split("\n")[first - 1:last]
    # keep the script's own line numbers in tracebacks
    return compile("\n" * (first - 1) + textwrap.dedent("\n".join(lines)), path, "exec")


def main():
    spec = importlib.util.spec_from_file_location("ref_den", os.path.join(TC, "Depth_Estimation_Network.py"))
    den = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(den)
    for name, (fscript, flines, lscript, llines, B, N, H, W, rng, use_conf, sentinel, seed) in CASES.items():
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(seed)
        model = den.Network().train()
        kept = {}

        def keep(key):
            def hook(_m, _i, out):
                out.retain_grad()
                kept[key] = out
            return hook
        net = model.DFF_net
        for k, m in enumerate((net.confidence, net.classif1, net.classif2, net.classif3)):
            m.register_forward_hook(keep(k))
        lo, hi = rng if rng else (0.1, 1.5)
        FS = torch.rand(B, 3, N, H, W, generator=g) * 2 - 1
        fd = (lo + (hi - lo) * torch.sort(torch.rand(B, N, generator=g), dim=1).values).reshape(B, N, 1, 1)
        mask = torch.rand(B, H, W, generator=g) < 0.7
        gt = lo + (hi - lo) * torch.rand(B, H, W, generator=g)
        gt[~mask] = sentinel
        conf = torch.rand(B, H, W, generator=g) + 0.05
        ns = {"torch": torch, "nn": torch.nn, "MSE_loss": torch.nn.MSELoss()}   # MSE_loss: the scripts' line 15
        exec(compiled(fscript, *flines), ns)
        mid_out, pred1, pred2, pred3 = model(FS, fd)
        preds = [t.detach().clone() for t in (mid_out, pred1, pred2, pred3)]
        ns.update(mid_out=mid_out, pred1=pred1, pred2=pred2, pred3=pred3, train_gt_depth=gt.clone(), train_mask=mask, train_conf=conf,
                  Weight1=0.5, Weight2=0.7, Weight3=1.0, mid_weight=0.3, valid_min_depth=lo, valid_max_depth=hi, min_depth=lo, max_depth=hi)
        exec(compiled(lscript, *llines), ns)
        ns["Total_Loss"].backward()
        out = {"focus_dists": fd.numpy(), "gt": gt.numpy(), "mask": mask.numpy(), "conf": conf.numpy() if use_conf else np.zeros(0, np.float32),
               "weights": np.array([0.3, 0.5, 0.7, 1.0], np.float32), "range": np.array(rng if rng else [], np.float64),
               "losses": np.array([float(ns[k]) for k in ("mid_loss", "Loss1", "Loss2", "Loss3", "Total_Loss")], np.float32)}
        for k in range(4):
            out["score%d" % k] = kept[k].detach().squeeze(1).numpy()
            out["grad%d" % k] = kept[k].grad.squeeze(1).numpy()
            out["pred%d" % k] = preds[k].numpy()
        path = os.path.join(ROOT, "tests", "golden", "loss_%s.npz" % name)
        np.savez_compressed(path, **out)
        print("%-12s B=%d N=%d %dx%d  max|score| %.1f  total %.6g  %d bytes" % (name, B, N, H, W, max(float(np.abs(out["score%d" % k]).max()) for k in range(4)),
                                                                               float(ns["Total_Loss"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
