"""A2C loss micro-benchmark: composed PyTorch vs the fused HIP kernel.

Times loss forward + backward from given logits and values with device
events, at the A3C-GPU config-2 shape (T=20, B=32, A=6) by default.  The
baseline is the composed math the trainer ran before the kernel
(``a2c_loss_reference`` on CUDA tensors: the GAE scan kernel + torch ops and
their autograd backward).

  python scripts/a2c_loss_micro.py                       # alternating timing
  python scripts/a2c_loss_micro.py --shape 20 256 512    # one wide shape
  python scripts/a2c_loss_micro.py --only fused --iters 100 --repeats 1
      # a fixed number of steps of one path, to count launches per step
      # under a kernel trace: (dispatches - warm-up) / iters

Prints one JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalerl_amd.ops import a2c_loss, a2c_loss_reference  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[20, 32, 6],
                    metavar=("T", "B", "A"))
    ap.add_argument("--iters", type=int, default=0,
                    help="steps per timed window; 0 sizes every path's "
                         "window to --window-s from 100 steps after warm-up")
    ap.add_argument("--window-s", type=float, default=1.5)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["composed", "fused"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("a2c_loss_micro needs a GPU")
    dev = torch.device("cuda:0")
    T, B, A = a.shape
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(T, B, A, generator=g).to(dev).requires_grad_()
    values = torch.randn(T, B, generator=g).to(dev).requires_grad_()
    boot = torch.randn(B, generator=g).to(dev)
    act = torch.randint(0, A, (T, B), generator=g).to(dev)
    r = torch.randn(T, B, generator=g).clamp(-1, 1).to(dev)
    d = (0.99 * (torch.rand(T, B, generator=g) > 0.1).float()).to(dev)
    kw = dict(lam=0.95, value_coef=0.5, entropy_coef=0.01)

    def step(fn):
        logits.grad = values.grad = None
        total, comps, _ = fn(logits, values, boot, act, r, d, **kw)
        total.backward()
        return total.detach(), comps

    paths = {"composed": a2c_loss_reference, "fused": a2c_loss}
    if a.only:
        paths = {a.only: paths[a.only]}

    def timed(fn, iters):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            step(fn)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / iters  # us per step

    iters = {}
    for name, fn in paths.items():
        timed(fn, max(a.warmup, 1))
        us = timed(fn, 100)
        iters[name] = a.iters or max(1, int(a.window_s * 1e6 / us))
    samples = {name: [] for name in paths}
    for _ in range(a.repeats):  # alternate the paths inside every repeat
        for name, fn in paths.items():
            samples[name].append(timed(fn, iters[name]))

    out = {"shape": [T, B, A], "iters": iters, "repeats": a.repeats,
           "warmup": a.warmup, "device": torch.cuda.get_device_name()}
    for name, s in samples.items():
        out[name + "_us"] = {"median": round(statistics.median(s), 2),
                             "min": round(min(s), 2),
                             "max": round(max(s), 2)}
    if len(paths) == 2:
        tc, cc = step(a2c_loss_reference)
        glc, gvc = logits.grad.clone(), values.grad.clone()
        tf, cf = step(a2c_loss)
        out["max_abs_diff"] = {
            "total": (tc - tf).abs().item(),
            "components": (cc - cf).abs().max().item(),
            "grad_logits": (glc - logits.grad).abs().max().item(),
            "grad_values": (gvc - values.grad).abs().max().item()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
