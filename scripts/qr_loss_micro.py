"""QR-DQN loss micro-benchmark: composed PyTorch vs the fused HIP kernel.

Times loss forward + backward from given quantile values with device events,
PER on, at the Ape-X shape (B=512, A=18, N=200) and the DQN shape (B=64, A=2,
N=200).  The baseline is the composed math: ``per_is_weights`` +
``qr_loss_reference`` on CUDA tensors in fp32.  The two paths alternate inside
every repeat.

  python scripts/qr_loss_micro.py
  python scripts/qr_loss_micro.py --shape 64 2 200 --iters 500

Prints one JSON line per shape.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalerl_amd.ops import (fused_qr_loss, per_is_weights,  # noqa: E402
                             qr_loss_reference)


def run(B, A, N, a, dev):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, A, N, generator=g).to(dev).requires_grad_()
    xo = torch.randn(B, A, N, generator=g).to(dev)
    xt = torch.randn(B, A, N, generator=g).to(dev)
    act = torch.randint(0, A, (B,), generator=g).to(dev)
    r = (2 * torch.rand(B, generator=g) - 1).to(dev)
    d = (0.99 * (torch.rand(B, generator=g) > 0.1).float()).to(dev)
    prios = (torch.rand(B, generator=g) + 0.1).to(dev)
    p_total = torch.tensor([10.0], device=dev)
    p_min = torch.tensor([0.1], device=dev)
    replay, beta = 100_000, 0.4

    def composed():
        w = per_is_weights(prios, p_total, p_min, replay, beta)
        loss, ql = qr_loss_reference(x, xo, xt, act, r, d, a.kappa, w)
        loss.backward()
        return loss, ql

    def fused():
        loss, ql = fused_qr_loss(x, xo, xt, act, r, d, a.kappa, prios=prios,
                                 p_total=p_total, p_min=p_min, beta=beta,
                                 replay_size=replay)
        loss.backward()
        return loss, ql

    paths = {"composed": composed, "fused": fused}

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
        timed(fn, a.warmup)
    samples = {name: [] for name in paths}
    for _ in range(a.repeats):
        for name, fn in paths.items():
            samples[name].append(timed(fn, a.iters))

    out = {"shape": [B, A, N], "kappa": a.kappa, "iters": a.iters,
           "repeats": a.repeats, "warmup": a.warmup,
           "device": torch.cuda.get_device_name()}
    for name, s in samples.items():
        out[name + "_us"] = {"median": round(statistics.median(s), 2),
                             "min": round(min(s), 2),
                             "max": round(max(s), 2)}
    x.grad = None
    lc, qc = composed()
    gc = x.grad.clone()
    x.grad = None
    lf, qf = fused()
    out["max_abs_diff"] = {"loss": (lc - lf).abs().item(),
                           "ql": (qc - qf).abs().max().item(),
                           "grad": (gc - x.grad).abs().max().item()}
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, action="append",
                    metavar=("B", "A", "N"))
    ap.add_argument("--kappa", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qr_loss_micro needs a GPU")
    for B, A, N in a.shape or [(512, 18, 200), (64, 2, 200)]:
        run(B, A, N, a, torch.device("cuda:0"))


if __name__ == "__main__":
    main()
