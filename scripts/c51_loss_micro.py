"""C51 loss micro-benchmark: composed PyTorch vs the fused HIP kernel.

Times loss forward + backward from given logits with device events, at the
Ape-X learner's shape (B = ApexArguments.batch_size, A=6, N=51, PER on).
The baseline is the composed math the trainers ran before the kernel:
``per_is_weights`` + ``c51_loss_reference`` on CUDA tensors.

  python scripts/c51_loss_micro.py                  # alternating timing
  python scripts/c51_loss_micro.py --only fused --iters 100 --repeats 1
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

from scalerl_amd.config import ApexArguments  # noqa: E402
from scalerl_amd.ops import (c51_loss_reference, fused_c51_loss,  # noqa: E402
                             per_is_weights)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=ApexArguments().batch_size)
    ap.add_argument("--actions", type=int, default=6)
    ap.add_argument("--atoms", type=int, default=51)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=["composed", "fused"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("c51_loss_micro needs a GPU")
    dev = torch.device("cuda:0")
    B, A, N = a.batch, a.actions, a.atoms
    v_min, v_max = -10.0, 10.0
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, A, N, generator=g).to(dev).requires_grad_()
    xo = torch.randn(B, A, N, generator=g).to(dev)
    xt = torch.randn(B, A, N, generator=g).to(dev)
    act = torch.randint(0, A, (B,), generator=g).to(dev)
    r = torch.randn(B, generator=g).to(dev)
    d = (0.99 * (torch.rand(B, generator=g) > 0.1).float()).to(dev)
    prios = (torch.rand(B, generator=g) + 0.1).to(dev)
    p_total = torch.tensor([10.0], device=dev)
    p_min = torch.tensor([0.1], device=dev)
    replay, beta = 100_000, 0.4

    def composed():
        w = per_is_weights(prios, p_total, p_min, replay, beta)
        loss, kl = c51_loss_reference(x, xo, xt, act, r, d, v_min, v_max, w)
        loss.backward()
        return loss, kl

    def fused():
        loss, kl = fused_c51_loss(x, xo, xt, act, r, d, v_min, v_max,
                                  prios=prios, p_total=p_total, p_min=p_min,
                                  beta=beta, replay_size=replay)
        loss.backward()
        return loss, kl

    paths = {"composed": composed, "fused": fused}
    if a.only:
        paths = {a.only: paths[a.only]}

    def timed(fn, iters):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            x.grad = None
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / iters  # us per step

    for fn in paths.values():
        if a.warmup:
            timed(fn, a.warmup)
    samples = {name: [] for name in paths}
    for _ in range(a.repeats):  # alternate the paths inside every repeat
        for name, fn in paths.items():
            samples[name].append(timed(fn, a.iters))

    out = {"shape": [B, A, N], "iters": a.iters, "repeats": a.repeats,
           "warmup": a.warmup, "device": torch.cuda.get_device_name()}
    for name, s in samples.items():
        out[name + "_us"] = {"median": round(statistics.median(s), 2),
                             "min": round(min(s), 2),
                             "max": round(max(s), 2)}
    if len(paths) == 2:
        x.grad = None
        lc, kc = composed()
        gc = x.grad.clone()
        x.grad = None
        lf, kf = fused()
        out["max_abs_diff"] = {
            "loss": (lc - lf).abs().item(),
            "kl": (kc - kf).abs().max().item(),
            "grad": (gc - x.grad).abs().max().item()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
