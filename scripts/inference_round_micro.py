#!/usr/bin/env python3
"""Inference-round microbenchmark: one AtariNet forward the way the batched
inference worker runs it (parallel/inference.py): bf16 autocast, no_grad,
train() mode (multinomial sampling), T=1 and A*E rows with LSTM state.  No
actor processes; the worker itself is not touched.  Times ROUNDS calls after
WARMUP, ending in a synchronise.  ``SCALERL_FUSED_ENCODER=0`` gives the
per-layer MIOpen encoder forward for comparison.
"""

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalerl_amd.models import AtariNet


def main():
    os.environ.setdefault("MIOPEN_FIND_MODE", "1")
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=24 * 256)
    p.add_argument("--num-actions", type=int, default=6)
    p.add_argument("--rounds", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    args = p.parse_args()

    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    R, A = args.rows, args.num_actions
    model = AtariNet((4, 84, 84), A, use_lstm=True).to(dev)
    model.train()
    inputs = {
        "obs": torch.randint(0, 256, (1, R, 4, 84, 84), dtype=torch.uint8,
                             device=dev),
        "reward": torch.randn(1, R, device=dev),
        "done": torch.rand(1, R, device=dev) < 0.01,
        "last_action": torch.randint(0, A, (1, R), device=dev),
    }
    state = model.initial_state(R, device=dev)

    def round_():
        with torch.no_grad(), \
                torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            return model(inputs, state)

    for _ in range(args.warmup):
        round_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.rounds):
        round_()
    torch.cuda.synchronize()
    ms = 1000 * (time.perf_counter() - t0) / args.rounds
    print(f"inference-round: {ms:.3f} ms/round  (rows={R}, "
          f"{args.rounds} rounds after {args.warmup})")


if __name__ == "__main__":
    main()
