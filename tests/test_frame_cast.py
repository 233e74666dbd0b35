"""One-pass uint8 → bf16 frame normalisation (csrc/frame_cast.hip) against
the three-pass torch expression it replaces, bit for bit."""

import pytest
import torch

from scalerl_amd.models import AtariNet
from scalerl_amd.ops import frame_cast


def _old(x: torch.Tensor) -> torch.Tensor:
    return (x.float() / 255.0).to(torch.bfloat16)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16)


def test_multiply_by_reciprocal_rounds_like_divide():
    """The kernel multiplies by fp32 1/255 instead of dividing: emulate that
    and its integer round-to-nearest-even for all 256 byte values."""
    x = torch.arange(256, dtype=torch.uint8)
    f = x.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    u = f.view(torch.int32)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    assert torch.equal(u.to(torch.int16), _bits(_old(x)))


def test_cpu_branch_is_the_torch_expression():
    x = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(_bits(frame_cast.frame_to_bf16(x)), _bits(_old(x)))


@pytest.mark.gpu
# 1 / 15: scalar tail only; 16: one vector group, no tail; 17 / 4099: both;
# 84672 = 3 frames of 4x84x84
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099, 84672])
def test_frame_cast_bit_equal_all_byte_values(n):
    # every length sees all 256 values that fit, at shifting positions
    x = (torch.arange(n, dtype=torch.int64) * 37 + n) % 256
    x = x.to(torch.uint8).cuda()
    if n >= 256:
        assert x.unique().numel() == 256
    got = frame_cast.frame_to_bf16(x)
    assert got.dtype == torch.bfloat16 and got.shape == x.shape
    assert torch.equal(_bits(got), _bits(_old(x)))


@pytest.mark.gpu
def test_frame_cast_all_256_values_and_unaligned_view():
    x = torch.arange(256, dtype=torch.uint8).cuda()
    assert torch.equal(_bits(frame_cast.frame_to_bf16(x)), _bits(_old(x)))
    # a view whose base is not 16-byte aligned takes the scalar path
    big = torch.arange(256 + 3, dtype=torch.int64).to(torch.uint8).cuda()
    v = big[3:]
    assert v.data_ptr() % 16 != 0
    assert torch.equal(_bits(frame_cast.frame_to_bf16(v)), _bits(_old(v)))


@pytest.mark.gpu
def test_encode_uses_cast_only_under_bf16_autocast(monkeypatch):
    torch.manual_seed(0)
    model = AtariNet((4, 84, 84), 6, use_lstm=False, native_conv=False).cuda()
    x = torch.randint(0, 256, (3, 4, 84, 84), dtype=torch.uint8,
                      device="cuda")
    calls = []
    real = frame_cast.frame_to_bf16

    def spy(t):
        calls.append(t.shape)
        return real(t)

    monkeypatch.setattr(frame_cast, "frame_to_bf16", spy)

    with torch.no_grad():
        # no autocast: the expression stays as it was; fp16 autocast does
        # not qualify either
        model.encode(x)
        assert calls == []
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            assert not frame_cast.bf16_autocast_active()

        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            new = model.encode(x)
            assert len(calls) == 1
            # the old expression path: force the else-branch
            monkeypatch.setattr(frame_cast, "bf16_autocast_active",
                                lambda: False)
            old = model.encode(x)
            assert len(calls) == 1
    assert new.dtype == old.dtype
    assert torch.equal(new, old)
