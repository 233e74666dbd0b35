"""hipGraph-captured learner step.

The IMPALA learner's forward+backward is hundreds of small kernel launches
(the MaskedLSTM unrolls 2 layers × (T+1) steps, each a GEMM + a fused
pointwise kernel) — measured on MI355X the HOST enqueue time dominates the
iteration (~40 ms of Python/launch per step at B=128).  Capturing
{zero-grad → model fwd → fused V-trace/loss → backward} into one hipGraph
replays the whole step as a single launch; the fused HIP kernels
(ctypes-launched onto the capture stream) capture along with torch's.

Kept OUTSIDE the graph: RCCL all-reduce (watchdog interaction), grad clip,
fused optimizer, weight publish — five launches, microseconds of enqueue.

Inputs are copied D2D from the gatherer's staging set into this object's
static buffers before each replay (cheap: device bandwidth).
"""

from __future__ import annotations

from typing import Dict, Tuple

import torch


def impala_fwd_bwd(model, flat_grad: torch.Tensor,
                   batch: Dict[str, torch.Tensor], *, use_lstm: bool,
                   autocast_dtype, reward_clip: bool, discounting: float,
                   loss_kwargs: Dict, timings=None):
    """{zero-grad → model fwd → fused V-trace/loss → backward} of the IMPALA
    learner: the one definition, run eagerly by ``ImpalaTrainer`` and
    captured by :class:`GraphedImpalaStep`.  ``timings`` marks ``forward`` /
    ``backward`` on the eager path; it is None under capture (no host
    timing belongs inside a captured region).  Returns (total, comps)."""
    from ..ops import impala_loss

    flat_grad.zero_()
    inputs = {k: batch[k] for k in ("obs", "reward", "done", "last_action")}
    core_state = ()
    if use_lstm:
        cs = batch["core_state"]
        core_state = (cs[0], cs[1])
    if autocast_dtype is not None:
        with torch.autocast(device_type="cuda", dtype=autocast_dtype):
            out, _ = model(inputs, core_state, greedy=True)
    else:
        out, _ = model(inputs, core_state, greedy=True)
    logits = out["policy_logits"].float()
    baseline = out["baseline"].float()
    rewards = batch["reward"][1:]
    if reward_clip:
        rewards = torch.clamp(rewards, -1, 1)
    discounts = (~batch["done"][1:]).float() * discounting
    total, comps, _ = impala_loss(
        batch["logits"][:-1], logits[:-1], batch["action"][:-1],
        rewards, discounts, baseline[:-1], baseline[-1].detach(),
        **loss_kwargs)
    if timings is not None:
        timings.time("forward")
    total.backward()
    if timings is not None:
        timings.time("backward")
    return total.detach(), comps


class GraphedImpalaStep:
    def __init__(self, model, flat_grad: torch.Tensor,
                 batch_example: Dict[str, torch.Tensor],
                 warmup_iters: int = 3, **step_kwargs):
        """``step_kwargs``: the keyword arguments of :func:`impala_fwd_bwd`
        (``timings`` excepted)."""
        dev = flat_grad.device

        # static input buffers (graph reads these addresses every replay),
        # initialized from the example batch — uninitialized int fields
        # (actions) would index out of bounds during warmup
        self.static: Dict[str, torch.Tensor] = {
            k: v.clone() for k, v in batch_example.items()
        }

        def run_step():
            return impala_fwd_bwd(model, flat_grad, self.static,
                                  **step_kwargs)

        # The C++ LSTM sequence loop (ops/csrc/lstm_seq.hip) drives raw
        # rocBLAS calls that are not graph-capture-safe (r2 call-2 finding:
        # HSA exception during capture with no other process on the GPU).
        # Inside a captured graph the per-step path's Python launch
        # overhead is paid once at capture time only, so force it here.
        from ..ops import lstm as _lstm_mod
        prev_seq = _lstm_mod._USE_SEQ
        _lstm_mod._USE_SEQ = False
        try:
            # torch-required warmup on a side stream before capture
            s = torch.cuda.Stream(device=dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                for _ in range(warmup_iters):
                    run_step()
            torch.cuda.current_stream(dev).wait_stream(s)

            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph,
                                  capture_error_mode="thread_local"):
                self.total, self.comps = run_step()
        finally:
            _lstm_mod._USE_SEQ = prev_seq

    def run(self, batch: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        for k, dst in self.static.items():
            dst.copy_(batch[k], non_blocking=True)
        self.graph.replay()
        return self.total, self.comps
