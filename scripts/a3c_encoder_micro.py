"""A3C encoder forward micro-benchmark at the learner's shape
(N = 21 * 128 frames, C = 1): the fused HIP kernel, with and without the
saved activations, against the unfused bf16-autocast conv + elu x 4 that
``A3CAtariNet.encode`` runs otherwise, on the same tensors.

  python scripts/a3c_encoder_micro.py

Device events around 200 calls per window, 7 windows per variant, the
variants alternated; 20 warm-up calls each.  Prints the largest difference
of the two results and one JSON line (us per call: median, min, max).
"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scalerl_amd.ops.a3c_encoder import a3c_encoder_fwd  # noqa: E402

N, C = 21 * 128, 1
g = torch.Generator().manual_seed(0)
x = torch.randn(N, C, 42, 42, generator=g).cuda()
shapes = [(32, C, 3, 3)] + [(32, 32, 3, 3)] * 3
ws = [(torch.randn(s, generator=g) * 0.1).cuda().requires_grad_() for s in shapes]
bs = [(torch.randn(32, generator=g) * 0.1).cuda().requires_grad_() for _ in shapes]
wb = [w.detach().to(torch.bfloat16) for w in ws]
bd = [b.detach() for b in bs]
flat = [t for p in zip(wb, bd) for t in p]


def unfused():
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        h = x
        for w, b in zip(ws, bs):
            h = F.elu(F.conv2d(h, w, b, stride=2, padding=1))
    return h


def fused_save():
    return a3c_encoder_fwd(x, *flat, True)[3]


def fused_nosave():
    return a3c_encoder_fwd(x, *flat, False)[3]


variants = {"unfused_bf16_autocast": unfused, "fused_save": fused_save,
            "fused_nosave": fused_nosave}
torch.backends.cudnn.benchmark = True
for f in variants.values():
    for _ in range(20):
        f()
torch.cuda.synchronize()

ref = unfused().float()
got = fused_save().float()
print("max abs diff fused vs unfused", float((ref - got).abs().max()),
      "max", float(ref.abs().max()))

ITERS, ROUNDS = 200, 7
times = {k: [] for k in variants}
for _ in range(ROUNDS):
    for name, f in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            f()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / ITERS * 1e3)
res = {k: {"median_us": round(statistics.median(v), 1),
           "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
       for k, v in times.items()}
print(json.dumps({"N": N, "C": C, "iters": ITERS, "rounds": ROUNDS, **res}))
