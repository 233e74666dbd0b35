"""One-pass uint8 frame → bf16 normalisation (csrc/frame_cast.hip).

``frame_to_bf16(x)`` equals ``(x.float() / 255.0).to(torch.bfloat16)`` bit
for bit, in one pass over the frames instead of three.  It is the bf16
autocast form of the encoder's normalize-on-device divide; CPU tensors run
the torch expression (the oracle).
"""

from __future__ import annotations

import torch

from ._backend import launch


def frame_to_bf16(x: torch.Tensor) -> torch.Tensor:
    """uint8 [...] → bf16 [...] of x / 255 (round-to-nearest-even)."""
    assert x.dtype == torch.uint8, "frame_to_bf16 takes uint8 frames"
    if not x.is_cuda:
        return (x.float() / 255.0).to(torch.bfloat16)
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    launch("frame_cast_u8_bf16", x.contiguous(), out, x.numel())
    return out


def bf16_autocast_active() -> bool:
    """True when CUDA autocast is on with dtype bf16 — the one case where
    the encoder's fp32 normalize is followed by a cast to bf16."""
    return (torch.is_autocast_enabled("cuda") and
            torch.get_autocast_dtype("cuda") == torch.bfloat16)
