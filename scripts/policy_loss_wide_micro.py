"""Per-call time (forward + backward of the total, host clock around a device
synchronise) of impala_loss at T=80, B=128 and ppo_fused_loss at N=10240 for
A in {64, 121, 1024}, beside the composed references on the same GPU tensors.

  --profile           few calls, kernel path only: the run to put under
                      rocprofv3 --kernel-trace --stats
  --parent-lib PATH   also time impala_loss at (80,128,18) with the
                      impala_fused_loss of another build of _hip_ops.so,
                      alternated with this tree's
Prints one JSON line."""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scalerl_amd.ops import _backend, impala_loss, ppo_fused_loss  # noqa: E402
from scalerl_amd.ops.ppo import ppo_loss_reference  # noqa: E402
from scalerl_amd.ops.vtrace import impala_loss_reference  # noqa: E402

PROFILE = "--profile" in sys.argv
PARENT_LIB = (sys.argv[sys.argv.index("--parent-lib") + 1]
              if "--parent-lib" in sys.argv else None)
dev = "cuda:0"


def impala_inputs(T, B, A):
    g = torch.Generator().manual_seed(3)
    tl = torch.randn(T, B, A, generator=g)
    bl = tl + 0.5 * torch.randn(T, B, A, generator=g)
    a = torch.randint(0, A, (T, B), generator=g)
    r = torch.randn(T, B, generator=g).clamp(-1, 1)
    d = 0.99 * (torch.rand(T, B, generator=g) > 0.2).float()
    v = torch.randn(T, B, generator=g)
    boot = torch.randn(B, generator=g)
    return [x.to(dev) for x in (bl, tl, a, r, d, v, boot)]


def ppo_inputs(N, A):
    g = torch.Generator().manual_seed(3)
    lg = torch.randn(N, A, generator=g)
    a = torch.randint(0, A, (N,), generator=g)
    old = torch.log_softmax(lg, -1).gather(1, a[:, None])[:, 0] \
        + 0.3 * torch.randn(N, generator=g)
    adv, ret, v = torch.randn(3, N, generator=g)
    return [x.to(dev) for x in (lg, v, a, old, adv, ret)]


def impala_step(fn, inp):
    bl, tl, a, r, d, v, boot = inp
    tl = tl.detach().requires_grad_()
    v = v.detach().requires_grad_()
    out = fn(bl, tl, a, r, d, v, boot, baseline_cost=0.5, entropy_cost=0.01)
    out[0].backward()


def ppo_step(fn, inp):
    lg, v, a, old, adv, ret = inp
    lg = lg.detach().requires_grad_()
    v = v.detach().requires_grad_()
    if fn is ppo_fused_loss:
        out = fn(lg, v, a, old, adv, ret, clip_eps=0.2, vcoef=0.5, ecoef=0.01)
    else:
        out = fn(lg, a, old, adv, ret, v, 0.2, 0.5, 0.01)
    out[0].backward()


def timed(step, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def stats(xs):
    return {"median_us": round(statistics.median(xs), 1),
            "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}


def measure(step, warm, calls, reps):
    for _ in range(warm):
        step()
    return stats([timed(step, calls) for _ in range(reps)])


res = {}
WARM, CALLS, REPS = (3, 5, 1) if PROFILE else (20, 100, 7)
for A in (64, 121, 1024):
    inp = impala_inputs(80, 128, A)
    res[f"impala_80x128x{A}_kernel_path"] = measure(
        lambda: impala_step(impala_loss, inp), WARM, CALLS, REPS)
    pin = ppo_inputs(10240, A)
    res[f"ppo_10240x{A}_kernel_path"] = measure(
        lambda: ppo_step(ppo_fused_loss, pin), WARM, CALLS, REPS)
    if not PROFILE:
        # the composed reference loops over T in Python: fewer calls
        res[f"impala_80x128x{A}_composed"] = measure(
            lambda: impala_step(impala_loss_reference, inp), 3, 10, 7)
        res[f"ppo_10240x{A}_composed"] = measure(
            lambda: ppo_step(ppo_loss_reference, pin), WARM, CALLS, REPS)

if PARENT_LIB and not PROFILE:
    # narrow path: parent's library against this one, alternated
    _backend.lib()
    spec = _backend._SPECS["impala_fused_loss"]
    new_fn = spec.fn
    parent = ctypes.CDLL(os.path.abspath(PARENT_LIB))
    parent_fn = parent.impala_fused_loss
    parent_fn.argtypes = spec.argtypes
    parent_fn.restype = ctypes.c_int
    inp = impala_inputs(80, 128, 18)
    step = lambda: impala_step(impala_loss, inp)  # noqa: E731
    for fn in (parent_fn, new_fn):
        spec.fn = fn
        for _ in range(50):
            step()
    runs = {"parent": [], "new": []}
    for _ in range(10):
        for name, fn in (("parent", parent_fn), ("new", new_fn)):
            spec.fn = fn
            runs[name].append(timed(step, 300))
    spec.fn = new_fn
    res["impala_80x128x18_parent"] = stats(runs["parent"])
    res["impala_80x128x18_new"] = stats(runs["new"])
    res["impala_80x128x18_raw"] = {k: [round(x, 1) for x in v]
                                   for k, v in runs.items()}

print(json.dumps(res))
