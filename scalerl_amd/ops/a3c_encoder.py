"""Fused A3C encoder forward (csrc/a3c_encoder_fwd.hip).

``fused_a3c_encoder(x, w1, b1, ..., w4, b4)`` runs the bf16 cast of the fp32
42x42 frames and the four 3x3 stride-2 pad-1 convolutions (bias + ELU each)
of ``A3CAtariNet.encode`` as one HIP kernel and returns the bf16
``[N, 32, 3, 3]`` feature map.  The backward pass stays on MIOpen: it calls
``aten.convolution_backward`` on the bf16 activations the kernel saved, so it
uses the same solvers as the unfused bf16 autocast path.  The ELU derivative
is taken from the saved result (``out > 0 ? g : g * (out + 1)``), so no
pre-activation is kept.

CUDA/ROCm only: the unfused path of ``A3CAtariNet.encode`` is the CPU form.
"""

from __future__ import annotations

import torch

from ._backend import launch

_HW = 42
_SIZES = (21, 11, 6, 3)


def _check(x, ws):
    if x.dtype != torch.float32:
        raise ValueError(f"fused A3C encoder needs fp32 frames, got {x.dtype}")
    if x.dim() != 4 or tuple(x.shape[2:]) != (_HW, _HW):
        raise ValueError(f"fused A3C encoder needs [N,C,42,42] frames, got "
                         f"{tuple(x.shape)}")
    c = x.shape[1]
    if not 1 <= c <= 4:
        raise ValueError(f"fused A3C encoder takes 1..4 channels, got {c}")
    for i, w in enumerate(ws):
        want = 32 * 9 * (c if i == 0 else 32)
        if w.shape[0] != 32 or w.numel() != want:
            raise ValueError(f"fused A3C encoder: w{i + 1} has shape "
                             f"{tuple(w.shape)}, expected 32 x {want // 32}")
    if not x.is_cuda:
        raise ValueError(f"fused A3C encoder needs CUDA frames, got {x.device}")


@torch.no_grad()
def a3c_encoder_fwd(x, w1, b1, w2, b2, w3, b3, w4, b4, save: bool):
    """One launch of the fused kernel.  x fp32 [N,C,42,42], C in 1..4;
    weights ``[32, Cin*9]`` (or 4-D), cast to bf16 here if they are not;
    biases fp32.  Returns ``(out1, out2, out3, out4)`` bf16 NCHW post-ELU;
    out1..out3 are None unless ``save``."""
    _check(x, (w1, w2, w3, w4))
    n, c = x.shape[:2]
    xc = x.contiguous()
    # the kernel stages frames with 16-byte loads; a channel is 441 * 16
    # bytes, so only the base matters
    assert xc.data_ptr() % 16 == 0, "a3c_encoder_fwd needs 16-byte aligned frames"
    ws = [w.to(torch.bfloat16).contiguous() for w in (w1, w2, w3, w4)]
    bs = [b.float().contiguous() for b in (b1, b2, b3, b4)]
    outs = [torch.empty((n, 32, s, s), dtype=torch.bfloat16, device=x.device)
            if save or s == 3 else None for s in _SIZES]
    launch("a3c_encoder_fwd", xc, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2],
           ws[3], bs[3], *outs, n, c)
    return tuple(outs)


class _FusedA3CEncoderFn(torch.autograd.Function):
    """Forward: one fused HIP kernel.  Backward: MIOpen, layer by layer, on
    the saved bf16 activations."""

    @staticmethod
    def forward(ctx, x, *params):
        save = any(ctx.needs_input_grad)
        # the bf16 weight casts, once per call; backward reuses them
        wb = [w.detach().to(torch.bfloat16).reshape(32, -1, 3, 3).contiguous()
              for w in params[0::2]]
        bs = [b.detach() for b in params[1::2]]
        outs = a3c_encoder_fwd(x, wb[0], bs[0], wb[1], bs[1], wb[2], bs[2],
                               wb[3], bs[3], save)
        if save:
            ctx.save_for_backward(x, *wb, *outs)
            ctx.w_shapes = [w.shape for w in params[0::2]]
        return outs[3]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x, *rest = ctx.saved_tensors
        wb, outs = rest[:4], rest[4:]
        conv_bwd = torch.ops.aten.convolution_backward
        # d elu from the result: out > 0 ? g : g * (out + 1)
        elu_bwd = torch.ops.aten.elu_backward
        # conv1 is the input layer: wgrad and bias grad only, on the same
        # bf16 frames the forward kernel computed from
        inputs = (x.to(torch.bfloat16),) + tuple(outs[:3])
        grads = [None] * 8
        g = dout.to(torch.bfloat16)
        for k in (3, 2, 1, 0):
            g = elu_bwd(g, 1.0, 1.0, 1.0, True, outs[k])
            g, dw, db = conv_bwd(g, inputs[k], wb[k], [32], [2, 2], [1, 1],
                                 [1, 1], False, [0, 0], 1,
                                 [k > 0, True, True])
            grads[2 * k] = dw.float().view(ctx.w_shapes[k])
            grads[2 * k + 1] = db.float()
        return (None, *grads)


def fused_a3c_encoder(x, w1, b1, w2, b2, w3, b3, w4, b4) -> torch.Tensor:
    """Differentiable fused A3C encoder forward: fp32 [N,C,42,42] frames and
    the four conv layers' fp32 parameters → bf16 [N,32,3,3], post-ELU."""
    _check(x, (w1, w2, w3, w4))
    return _FusedA3CEncoderFn.apply(x, w1, b1, w2, b2, w3, b3, w4, b4)
