"""Hand-written MFMA Atari conv encoder (fwd + wgrad + dgrad wrappers).

All v2 kernels are hardware-validated (r2: 10/10 kernel-vs-oracle on
MI355X, tests ungated).  MIOpen remains the model default until the v3
kernels (panel-staged fwd/wgrad, stride-decomposed dgrad — written,
CPU-math-verified, gated SCALERL_EXPERIMENTAL) win the per-op A/B
(profiles/README.md).  `mfma_selftest` validates the fragment-layout
constants first; every kernel shares them.
"""

from __future__ import annotations

import torch

from ._backend import launch


def mfma_selftest() -> bool:
    """Validate the 16x16x32 bf16 fragment maps on-device."""
    g = torch.Generator().manual_seed(0)
    A = torch.randn(16, 32, generator=g).cuda()
    B = torch.randn(32, 16, generator=g).cuda()  # asymmetric (guide G9)
    D = torch.empty(16, 16, device="cuda")
    launch("mfma_selftest", A, B, D)
    want = (A.to(torch.bfloat16).float() @ B.to(torch.bfloat16).float())
    return torch.allclose(D.cpu(), want.cpu(), rtol=1e-2, atol=1e-2)


# layer -> (input [C,IH,IW], output [K,OH,OW], weight [K,C,KH,KW])
_SHAPES = {
    1: ((4, 84, 84), (32, 20, 20), (32, 4, 8, 8)),
    2: ((32, 20, 20), (64, 9, 9), (64, 32, 4, 4)),
    3: ((64, 9, 9), (64, 7, 7), (64, 64, 3, 3)),
}
_DGRAD_LAYERS = (2, 3)  # conv1 is the input layer


@torch.no_grad()
def atari_conv_fwd(layer: int, x: torch.Tensor, weight: torch.Tensor,
                   bias: torch.Tensor = None, relu: bool = True,
                   v3: bool = False) -> torch.Tensor:
    """Forward one encoder conv.  layer 1 accepts uint8 (fused /255) or
    bf16; layers 2-3 take bf16.  Returns bf16 [N, K, OH, OW].  ``v3``
    (layers 2-3): the panel-staged kernels of conv_fwd.hip, EXPERIMENTAL
    until hardware-validated (r3)."""
    in_shape, out_shape, _ = _SHAPES[layer]
    assert tuple(x.shape[1:]) == in_shape, (x.shape, in_shape)
    if v3:
        assert layer in (2, 3)
        name = f"atari_conv{layer}_fwd_v3"
    elif layer == 1:
        name = ("atari_conv1_fwd_u8" if x.dtype == torch.uint8
                else "atari_conv1_fwd_bf16")
    else:
        name = f"atari_conv{layer}_fwd"
    if name != "atari_conv1_fwd_u8":
        x = x.to(torch.bfloat16)
    out = torch.empty((x.shape[0], *out_shape), dtype=torch.bfloat16,
                      device=x.device)
    launch(name, x.contiguous(), weight.to(torch.bfloat16).contiguous(),
           bias.float().contiguous() if bias is not None else None,
           out, x.shape[0], int(relu))
    return out


def atari_conv_fwd_v3(layer, x, weight, bias=None, relu=True):
    return atari_conv_fwd(layer, x, weight, bias, relu, v3=True)


@torch.no_grad()
def atari_conv_wgrad(layer: int, x: torch.Tensor, dout: torch.Tensor,
                     split: int = 64, v3: bool = False) -> torch.Tensor:
    """dL/dW for one encoder conv (fp32 out).  Layer 1 takes uint8 x.
    ``v3``: the panel-staged kernels (conv_bwd.hip convN_wgrad_v3: both MFMA
    operands are contiguous LDS vector reads; v2's B side re-gathers im2col
    scalar by scalar per tile), EXPERIMENTAL until hardware-validated (r3)."""
    K, C, KH, KW = _SHAPES[layer][2]
    dw = torch.zeros(K, C * KH * KW, device=x.device, dtype=torch.float32)
    if layer == 1:
        assert x.dtype == torch.uint8
    else:
        x = x.to(torch.bfloat16)
    dc = dout.to(torch.bfloat16).contiguous()
    if v3:
        launch(f"atari_conv{layer}_wgrad_v3", x.contiguous(), dc, dw,
               x.shape[0])
    else:
        launch("atari_conv1_wgrad_u8" if layer == 1
               else f"atari_conv{layer}_wgrad", x.contiguous(), dc, dw,
               x.shape[0], split)
    return dw.view(K, C, KH, KW)


def atari_conv_wgrad_v3(layer, x, dout):
    return atari_conv_wgrad(layer, x, dout, v3=True)


@torch.no_grad()
def atari_conv_dgrad(layer: int, dout: torch.Tensor, weight: torch.Tensor,
                     v3: bool = False) -> torch.Tensor:
    """dL/dX for encoder convs 2-3 (bf16 out; conv1 is the input layer).
    ``v3`` (layer 2 only): parity-decomposed stride-2 dgrad, 4x less MFMA
    work than the masked v2 (conv_bwd.hip conv2_dgrad_v3), EXPERIMENTAL until
    hardware-validated (r3)."""
    assert layer in ((2,) if v3 else _DGRAD_LAYERS)
    din = torch.empty((dout.shape[0], *_SHAPES[layer][0]),
                      dtype=torch.bfloat16, device=dout.device)
    launch(f"atari_conv{layer}_dgrad" + ("_v3" if v3 else ""),
           dout.to(torch.bfloat16).contiguous(),
           weight.to(torch.bfloat16).contiguous(), din, dout.shape[0])
    return din


def atari_conv2_dgrad_v3(dout, weight):
    return atari_conv_dgrad(2, dout, weight, v3=True)


class _NativeConvFn(torch.autograd.Function):
    """Autograd over the native encoder convs (layer 2/3: full backward;
    layer 1: wgrad only — it is the input layer)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, weight, bias, layer, relu):
        out = atari_conv_fwd(layer, x, weight, bias, relu=relu)
        ctx.save_for_backward(x, weight, out)
        ctx.layer, ctx.relu = layer, relu
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        x, weight, out = ctx.saved_tensors
        layer = ctx.layer
        if ctx.relu:
            dout = dout * (out > 0)
        dw = atari_conv_wgrad(layer, x, dout)
        db = dout.float().sum(dim=(0, 2, 3))
        dx = None
        if layer in _DGRAD_LAYERS and ctx.needs_input_grad[0]:
            dx = atari_conv_dgrad(layer, dout, weight)
        return dx, dw, db, None, None


def native_conv(layer: int, x, weight, bias=None, relu: bool = True):
    """Differentiable native encoder conv (EXPERIMENTAL, opt-in via
    AtariNet(native_conv=True) / SCALERL_NATIVE_CONV=1)."""
    return _NativeConvFn.apply(x, weight, bias, layer, relu)
