#!/usr/bin/env python3
"""Learner-step microbenchmark: no actor processes, synthetic device-resident
batch.  Isolates the learner pipeline (model fwd → fused V-trace/loss →
backward → clip → fused RMSProp → publish) for rocprof kernel profiling and
launch-overhead analysis.  THIS IS NOT THE HEADLINE BENCH (bench.py runs the
full actor-learner pipeline); it measures the learner's ceiling.
"""

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalerl_amd.models import AtariNet
from scalerl_amd.ops import FusedRMSprop, clip_grad_norm_
from scalerl_amd.parallel import FlatParams


def main():
    os.environ.setdefault("MIOPEN_FIND_MODE", "1")
    p = argparse.ArgumentParser()
    p.add_argument("--rollout-length", type=int, default=80)
    p.add_argument("--batch-size", type=int, default=32)
    p.add_argument("--num-actions", type=int, default=6)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--use-lstm", type=int, default=1)
    p.add_argument("--dtype", type=str, default="bf16")
    p.add_argument("--graph", type=int, default=0, choices=(0, 1),
                   help="1: time the hipGraph-captured step the trainer "
                        "replays (runtime/graphed.py) instead of the eager one")
    args = p.parse_args()

    dev = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    torch.manual_seed(0)
    torch.backends.cudnn.benchmark = True
    T, B, A = args.rollout_length, args.batch_size, args.num_actions
    model = AtariNet((4, 84, 84), A, use_lstm=bool(args.use_lstm)).to(dev)
    flat = FlatParams(model, device=dev)
    opt = FusedRMSprop(flat.flat, lr=6e-4, alpha=0.99, eps=0.01)
    pub = torch.zeros_like(flat.flat, device="cpu").pin_memory() \
        if dev.type == "cuda" else torch.zeros_like(flat.flat)

    batch = {
        "obs": torch.randint(0, 256, (T + 1, B, 4, 84, 84), dtype=torch.uint8,
                             device=dev),
        "reward": torch.randn(T + 1, B, device=dev),
        "done": torch.rand(T + 1, B, device=dev) < 0.01,
        "last_action": torch.randint(0, A, (T + 1, B), device=dev),
        "action": torch.randint(0, A, (T + 1, B), device=dev),
        "logits": torch.randn(T + 1, B, A, device=dev),
    }
    if args.use_lstm:
        batch["core_state"] = torch.stack(model.initial_state(B, device=dev))
    autocast = (args.dtype == "bf16" and dev.type == "cuda")
    # the trainer's own step, eager or captured (runtime/graphed.py)
    from scalerl_amd.runtime.graphed import GraphedImpalaStep, impala_fwd_bwd
    step_kwargs = dict(use_lstm=bool(args.use_lstm),
                       autocast_dtype=torch.bfloat16 if autocast else None,
                       reward_clip=True, discounting=0.99, loss_kwargs={})
    if args.graph:
        assert dev.type == "cuda", "--graph 1 needs a GPU"
        fwd_bwd = GraphedImpalaStep(model, flat.flat_grad, batch,
                                    **step_kwargs).run
    else:
        def fwd_bwd(b):
            return impala_fwd_bwd(model, flat.flat_grad, b, **step_kwargs)

    def step():
        total, _ = fwd_bwd(batch)
        clip_grad_norm_(flat.flat_grad, 40.0)
        opt.step(flat.flat_grad)
        pub.copy_(flat.flat, non_blocking=True)
        return total

    for _ in range(args.warmup):
        step()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms = 1000 * dt / args.steps
    sps = T * B * args.steps / dt
    print(f"learner-micro: {ms:.2f} ms/iter  {sps:,.0f} env-steps/s "
          f"(T={T} B={B} lstm={bool(args.use_lstm)} dtype={args.dtype})")


if __name__ == "__main__":
    main()
