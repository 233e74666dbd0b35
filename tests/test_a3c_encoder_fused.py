"""Fused A3C encoder forward (ops/csrc/a3c_encoder_fwd.hip) against torch.

Oracles run in fp32 on the CPU, on bf16-rounded weights and inputs, so that
they do not depend on any GPU convolution library.
"""

import pytest
import torch
import torch.nn.functional as F

from scalerl_amd.config import A3CGpuArguments
from scalerl_amd.models import a3c_atari as a3c_mod
from scalerl_amd.models.a3c_atari import A3CAtariNet
from scalerl_amd.ops import fused_a3c_encoder
from scalerl_amd.ops.a3c_encoder import a3c_encoder_fwd

# one bf16 rounding of the result plus fp32 summation order of <= 288 terms
# (tests/test_encoder_fused.py sets the same figures for 576 terms)
RTOL, ATOL = 2.0 ** -8, 1e-3


def _params(c, seed=0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(32, c, 3, 3)] + [(32, 32, 3, 3)] * 3
    ws = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    bs = [torch.randn(32, generator=g) * 0.1 + shift for _ in shapes]
    return ws, bs


def _frames(n, c, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, 42, 42, generator=g)
    flat = x.view(-1)
    idx = torch.randint(0, flat.numel(), (8 * n * c,), generator=g)
    flat[idx] = 8.0 * (1 - 2 * (idx % 2)).float()      # a few entries at +-8
    return x


def _run(x, ws, bs, save):
    args = [t.cuda() for pair in zip(ws, bs) for t in pair]
    outs = a3c_encoder_fwd(x.cuda(), *args, save)
    torch.cuda.synchronize()
    return outs


def _check_layerwise(x, ws, bs, tag):
    outs = _run(x, ws, bs, save=True)
    inp = x.to(torch.bfloat16)
    for k, size in enumerate((21, 11, 6, 3)):
        w = ws[k].to(torch.bfloat16).float()
        pre = F.conv2d(inp.float().cpu(), w, bs[k], stride=2, padding=1)
        ref = F.elu(pre)
        got = outs[k]
        assert got.dtype == torch.bfloat16
        assert tuple(got.shape) == (x.shape[0], 32, size, size) == ref.shape
        err = (got.float().cpu() - ref).abs().max()
        print(f"{tag} conv{k + 1}: max abs err {err:.3e}, pre-activations "
              f"{pre.min():.2f}..{pre.max():.2f}")
        assert torch.allclose(got.float().cpu(), ref, rtol=RTOL, atol=ATOL), \
            f"{tag} conv{k + 1}: max abs err {err:.3e}"
        inp = got  # the next layer is checked on the kernel's own output


# 1061 > 2 x 512 workgroups: every workgroup reuses its LDS planes and halos
@pytest.mark.gpu
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 37, 1061])
def test_layerwise_forward_matches_torch(n, c):
    ws, bs = _params(c)
    _check_layerwise(_frames(n, c), ws, bs, f"N={n} C={c}")


@pytest.mark.gpu
def test_padding_by_hand():
    ws, bs = _params(1)
    ws[0] = torch.ones(32, 1, 3, 3)
    bs[0] = torch.zeros(32)
    out1 = _run(torch.ones(2, 1, 42, 42), ws, bs, save=True)[0].float().cpu()
    want = torch.full((21, 21), 9.0)
    want[0, :] = want[:, 0] = 6.0
    want[0, 0] = 4.0
    assert torch.equal(out1, want.expand(2, 32, 21, 21))


@pytest.mark.gpu
def test_save_and_nosave_agree_bitwise():
    ws, bs = _params(1)
    x = _frames(3, 1)
    o1, o2, o3, with_save = _run(x, ws, bs, save=True)
    n1, n2, n3, without = _run(x, ws, bs, save=False)
    assert n1 is None and n2 is None and n3 is None
    assert o1 is not None and o2 is not None and o3 is not None
    assert torch.equal(with_save.view(torch.int16), without.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [-4.0, 4.0])
def test_elu_branches(shift):
    # conv1's pre-activations (spread about 1) all land on one ELU branch
    ws, bs = _params(1, shift=shift)
    _check_layerwise(_frames(3, 1), ws, bs, f"shift={shift}")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.gpu
def test_model_gradients_no_worse_than_unfused_bf16(monkeypatch):
    T, B, A = 5, 4, 6
    torch.manual_seed(0)
    model = A3CAtariNet(1, A, fused_encoder=True).cuda()
    g = torch.Generator().manual_seed(2)
    obs = _frames(T * B, 1, seed=3).view(T, B, 1, 42, 42).cuda()
    notdone = (torch.rand(T, B, generator=g) >= 0.1).float().cuda()
    r_logits = torch.randn(T, B, A, generator=g).cuda()
    r_values = torch.randn(T, B, generator=g).cuda()
    names = [f"conv{k}.{p}" for k in (1, 2, 3, 4) for p in ("weight", "bias")]
    params = dict(model.named_parameters())
    calls = []
    real = a3c_mod.fused_a3c_encoder
    monkeypatch.setattr(a3c_mod, "fused_a3c_encoder",
                        lambda *a: (calls.append(1), real(*a))[1])

    def run(autocast, fused):
        model.fused_encoder = fused
        model.zero_grad(set_to_none=True)
        state = model.initial_state(B, device="cuda")
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16,
                            enabled=autocast):
            logits, values, _ = model.unroll(obs, notdone, state)
        loss = ((logits.float() * r_logits).sum() +
                (values.float() * r_values).sum())
        loss.backward()
        res = {"loss": loss.detach().clone()}
        for k in names:
            res[k] = params[k].grad.detach().clone()
        return res

    fp32 = run(False, True)       # no autocast: the flag alone does not fuse
    unfused = run(True, False)
    assert calls == []
    fused = run(True, True)
    assert calls == [1]

    worse = []
    for k in ["loss"] + names:
        e_unf, e_fus = _rel(unfused[k], fp32[k]), _rel(fused[k], fp32[k])
        print(f"{k}: rel L2 vs fp32  unfused {e_unf:.3e}  fused {e_fus:.3e}  "
              f"ratio {e_fus / max(e_unf, 1e-30):.2f}")
        if not e_fus <= 2.0 * e_unf:
            worse.append((k, e_unf, e_fus))
    assert not worse, worse


def test_fused_flag_leaves_cpu_model_unchanged():
    torch.manual_seed(0)
    plain = A3CAtariNet(1, 6)
    torch.manual_seed(0)
    flagged = A3CAtariNet(1, 6, fused_encoder=True)
    assert list(plain.state_dict()) == list(flagged.state_dict())
    obs = _frames(3, 1)
    state = plain.initial_state(3)
    want = plain(obs, state)
    got = flagged(obs, state)
    for a, b in zip((want[0], want[1], *want[2]), (got[0], got[1], *got[2])):
        assert torch.equal(a, b)


@pytest.mark.parametrize("what, match", [
    ("cpu", "CUDA"), ("size", "42,42"), ("channels", "1..4 channels"),
    ("dtype", "fp32"), ("w2", "w2")])
def test_fused_a3c_encoder_rejects(what, match):
    # CPU tensors throughout: the device is the last thing checked
    c = 5 if what == "channels" else 1
    ws, bs = _params(c)
    x = torch.zeros(2, c, 40 if what == "size" else 42, 42)
    if what == "dtype":
        x = x.double()
    if what == "w2":
        ws[1] = torch.zeros(32, 16, 3, 3)
    with pytest.raises(ValueError, match=match):
        fused_a3c_encoder(x, *[t for pair in zip(ws, bs) for t in pair])


def test_trainer_flag_defaults_off_and_needs_bf16():
    from scalerl_amd.runtime.a3c_gpu import A3CGpuTrainer
    assert A3CGpuArguments().fused_encoder is False
    args = A3CGpuArguments(fused_encoder=True, dtype="fp32")
    with pytest.raises(ValueError, match="bf16"):
        A3CGpuTrainer(args, device="cpu")
