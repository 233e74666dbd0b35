"""Fused Atari encoder forward (csrc/encoder_fwd.hip).

``fused_encoder(x, w1, b1, w2, b2, w3, b3)`` runs the uint8 normalise and the
three Nature-CNN convolutions (bias + ReLU each) of ``AtariNet.encode`` as
one HIP kernel and returns the bf16 ``[N, 64, 7, 7]`` feature map.  The
backward pass stays on MIOpen: it calls ``aten.convolution_backward`` on the
bf16 activations the kernel saved, so it uses the same solvers as the
unfused bf16 autocast path; only the forward rounding differs.

CUDA/ROCm only: the unfused path of ``AtariNet.encode`` is the CPU form.
``AtariNet.encode`` takes the fused forward by default only where gradients
are off (``models/atari.py``, ``FUSED_ENCODER_TRAIN``).
"""

from __future__ import annotations

import torch

from . import frame_cast
from ._backend import launch

_W_SHAPES = ((32, 4, 8, 8), (64, 32, 4, 4), (64, 64, 3, 3))


@torch.no_grad()
def atari_encoder_fwd(x, w1, b1, w2, b2, w3, b3, save: bool):
    """One launch of the fused kernel.  x uint8 [N,4,84,84]; weights bf16
    ``[K, C*KH*KW]`` (or 4-D) contiguous; biases fp32.  Returns
    ``(out1, out2, out3)`` bf16 NCHW post-ReLU; out1/out2 are None unless
    ``save``."""
    assert x.is_cuda and x.dtype == torch.uint8
    assert tuple(x.shape[1:]) == (4, 84, 84), x.shape
    n = x.shape[0]
    xc = x.contiguous()
    # the kernel stages images with 16-byte loads; an image is 1764 * 16
    # bytes, so only the base matters
    assert xc.data_ptr() % 16 == 0, "atari_encoder_fwd needs 16-byte aligned frames"
    ws = [w.to(torch.bfloat16).contiguous() for w in (w1, w2, w3)]
    for w, shape in zip(ws, _W_SHAPES):
        assert w.numel() == shape[0] * shape[1] * shape[2] * shape[3], w.shape
    dev = x.device
    out1 = out2 = None
    if save:
        out1 = torch.empty((n, 32, 20, 20), dtype=torch.bfloat16, device=dev)
        out2 = torch.empty((n, 64, 9, 9), dtype=torch.bfloat16, device=dev)
    out3 = torch.empty((n, 64, 7, 7), dtype=torch.bfloat16, device=dev)
    launch("atari_encoder_fwd", xc,
           ws[0], b1.float().contiguous(), ws[1], b2.float().contiguous(),
           ws[2], b3.float().contiguous(), out1, out2, out3, n)
    return out1, out2, out3


class _FusedEncoderFn(torch.autograd.Function):
    """Forward: one fused HIP kernel.  Backward: MIOpen, layer by layer, on
    the saved bf16 activations."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3):
        save = any(ctx.needs_input_grad)
        # the bf16 weight casts, once per call; backward reuses them
        wb = [w.detach().to(torch.bfloat16).contiguous() for w in (w1, w2, w3)]
        out1, out2, out3 = atari_encoder_fwd(
            x, wb[0], b1.detach(), wb[1], b2.detach(), wb[2], b3.detach(),
            save)
        if save:
            ctx.save_for_backward(x, wb[0], wb[1], wb[2], out1, out2, out3)
        return out3

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x, wb1, wb2, wb3, out1, out2, out3 = ctx.saved_tensors
        conv_bwd = torch.ops.aten.convolution_backward

        def layer_bwd(g, inp, w, stride, mask):
            return conv_bwd(g, inp, w, [w.shape[0]], [stride, stride], [0, 0],
                            [1, 1], False, [0, 0], 1, mask)

        # g = dout * (out > 0) in one kernel: the op ReLU's own backward uses
        # (the multiply with a bool mask runs an unvectorised type-promoting
        # kernel, 4x slower at the learner's shapes)
        relu_bwd = torch.ops.aten.threshold_backward

        g3 = relu_bwd(dout.to(torch.bfloat16), out3, 0)
        d2, dw3, db3 = layer_bwd(g3, out2, wb3, 1, [True, True, True])
        g2 = relu_bwd(d2, out2, 0)
        d1, dw2, db2 = layer_bwd(g2, out1, wb2, 2, [True, True, True])
        g1 = relu_bwd(d1, out1, 0)
        # conv1 is the input layer: wgrad and bias grad only, on the same
        # bf16 frames the forward kernel computed from
        xb = frame_cast.frame_to_bf16(x)
        _, dw1, db1 = layer_bwd(g1, xb, wb1, 4, [False, True, True])
        return (None, dw1.float(), db1.float(), dw2.float(), db2.float(),
                dw3.float(), db3.float())


def fused_encoder(x, w1, b1, w2, b2, w3, b3) -> torch.Tensor:
    """Differentiable fused encoder forward: uint8 [N,4,84,84] frames and the
    three conv layers' fp32 parameters → bf16 [N,64,7,7], post-ReLU."""
    return _FusedEncoderFn.apply(x, w1, b1, w2, b2, w3, b3)
