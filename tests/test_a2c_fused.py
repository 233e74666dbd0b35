"""Fused GAE actor-critic loss: CPU parity with the composed loss it replaces,
the kernel's gradient formulas in fp64, and the HIP kernel against the
composed reference in fp64 on the CPU."""

import functools

import pytest
import torch
import torch.nn.functional as F

from scalerl_amd.ops import a2c_loss, a2c_loss_reference, gae
from scalerl_amd.ops.scans import A2C_MAX_T

# the project's TD-loss tolerances (tests/test_td.py, tests/test_c51_fused.py)
RTOL, ATOL = 1e-4, 1e-5
VC, EC = 0.5, 0.01
# 513 sits just above the 512 actions a wave keeps in registers.  The fp32
# composed reference alone meets RTOL/ATOL against fp64 at every shape here,
# (300,2,6) at lam = 1.0 included (checked with this seed on the CPU).
SHAPES = [(1, 1, 1), (1, 1, 2), (5, 3, 6), (8, 9, 18), (3, 17, 32), (3, 2, 33),
          (2, 3, 64), (2, 3, 65), (2, 1, 513), (300, 2, 6)]


@functools.lru_cache(maxsize=None)
def _inputs(T, B, A, scale=1.0, seed=3):
    """Seeded CPU inputs (never modified): logits, values, bootstrap, actions,
    rewards, discounts."""
    g = torch.Generator().manual_seed(seed)
    logits = scale * torch.randn(T, B, A, generator=g)
    values = torch.randn(T, B, generator=g)
    bootstrap = torch.randn(B, generator=g)
    actions = torch.randint(0, A, (T, B), generator=g)
    actions.view(-1)[0], actions.view(-1)[-1] = 0, A - 1
    rewards = torch.randn(T, B, generator=g).clamp(-1, 1)
    discounts = 0.99 * (torch.rand(T, B, generator=g) > 0.2).float()
    return logits, values, bootstrap, actions, rewards, discounts


def _with_grads(fn, inputs, dtype, dev="cpu", **kw):
    """(total, components, returns, dlogits, dvalues) of N * total, on the CPU."""
    logits, values, *rest = (
        t.to(dev, dtype if t.is_floating_point() else None, copy=True)
        for t in inputs)
    logits.requires_grad_()
    values.requires_grad_()
    total, comps, returns = fn(logits, values, *rest, value_coef=VC,
                               entropy_coef=EC, **kw)
    assert not comps.requires_grad and not returns.requires_grad
    (total * values.numel()).backward()
    return tuple(t.detach().cpu() for t in
                 (total, comps, returns, logits.grad, values.grad))


@pytest.mark.parametrize("lam", [1.0, 0.95])
def test_a2c_loss_cpu_bit_identical_to_frozen_learn_step(lam):
    lg, v, boot, a, r, d = _inputs(8, 9, 6)
    # A3CGpuTrainer.learn_step's loss as it was before a2c_loss
    logits, values = lg.clone().requires_grad_(), v.clone().requires_grad_()
    with torch.no_grad():
        adv, returns = gae(r, values.detach(), boot.detach(), d, lam)
    logp = F.log_softmax(logits, dim=-1)
    taken = logp.gather(-1, a.unsqueeze(-1)).squeeze(-1)
    pg_loss = -(taken * adv).mean()
    value_loss = 0.5 * F.mse_loss(values, returns)
    entropy = -(logp.exp() * logp).sum(-1).mean()
    total = pg_loss + VC * value_loss - EC * entropy
    total.backward()

    lg2, v2 = lg.clone().requires_grad_(), v.clone().requires_grad_()
    total2, comps, ret2 = a2c_loss(lg2, v2, boot, a, r, d, lam=lam,
                                   value_coef=VC, entropy_coef=EC,
                                   want_returns=True)
    total2.backward()
    assert torch.equal(total2, total)
    assert torch.equal(comps, torch.stack([pg_loss, value_loss, entropy]))
    assert torch.equal(ret2, returns)
    assert torch.equal(lg2.grad, logits.grad)
    assert torch.equal(v2.grad, values.grad)
    with pytest.raises(ValueError, match="rewards"):
        a2c_loss(lg, v, boot, a, r[:-1], d)


@pytest.mark.parametrize("lam", [1.0, 0.95])
def test_a2c_gradient_formulas_match_autograd_fp64(lam):
    inputs = _inputs(8, 9, 18)
    lg, v, boot, a, r, d = (t.double() if t.is_floating_point() else t
                            for t in inputs)
    _, _, _, want_gl, want_gv = _with_grads(a2c_loss_reference, inputs,
                                            torch.float64, lam=lam)
    adv, _ = gae(r, v, boot, d, lam)
    logp = F.log_softmax(lg, -1)
    p = logp.exp()
    h = (p * logp).sum(-1, keepdim=True)
    gl = (-adv.unsqueeze(-1) * (F.one_hot(a, lg.shape[-1]) - p)
          + EC * p * (logp - h))
    torch.testing.assert_close(gl, want_gl, rtol=0, atol=1e-12)
    torch.testing.assert_close(-VC * adv, want_gv, rtol=0, atol=1e-12)


def _compare(got, want):
    names = ("total", "components", "returns", "grad_logits", "grad_values")
    for name, g, w in zip(names, got, want):
        print(name, "max abs diff", (g - w).abs().max().item(),
              "max |ref|", w.abs().max().item())
    for g, w in zip(got, want):
        assert torch.isfinite(g).all()
        torch.testing.assert_close(g, w.float(), rtol=RTOL, atol=ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("lam", [1.0, 0.95])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a2c_gpu_matches_fp64_reference(shape, lam):
    inputs = _inputs(*shape)
    _compare(_with_grads(a2c_loss, inputs, torch.float32, "cuda:0", lam=lam,
                         want_returns=True),
             _with_grads(a2c_loss_reference, inputs, torch.float64, lam=lam))


@pytest.mark.gpu
def test_a2c_gpu_softmax_stability():
    inputs = _inputs(5, 3, 6, scale=30.0)
    _compare(_with_grads(a2c_loss, inputs, torch.float32, "cuda:0", lam=0.95,
                         want_returns=True),
             _with_grads(a2c_loss_reference, inputs, torch.float64, lam=0.95))


@pytest.mark.gpu
def test_a2c_gpu_is_deterministic():
    runs = [_with_grads(a2c_loss, _inputs(8, 9, 18), torch.float32, "cuda:0",
                        lam=0.95, want_returns=True) for _ in range(2)]
    for first, second in zip(runs[0][2:], runs[1][2:]):
        assert torch.equal(first, second)


@pytest.mark.gpu
def test_a2c_gpu_rollout_beyond_lds_bound_raises():
    inputs = (t.cuda() for t in _inputs(A2C_MAX_T + 1, 1, 2))
    with pytest.raises(RuntimeError, match=r"code -3 \(rollout length"):
        a2c_loss(*inputs)
