"""Wide-row (A > 32) IMPALA and PPO loss kernels against the composed
references in fp64 on the CPU."""

import functools

import pytest
import torch
import torch.nn.functional as F

from scalerl_amd.ops import impala_loss, ppo_fused_loss
from scalerl_amd.ops.ppo import ppo_loss_reference
from scalerl_amd.ops.vtrace import impala_loss_reference, vtrace_reference
from test_a2c_fused import ATOL, RTOL, _inputs

BC, EC, CLIP = 0.5, 0.01, 0.2
# 33: first wide size; 64 / 65: a full wave / one tail lane; 121: more rows
# than waves in the PPO kernel; 513 / 1025: one past the 512 actions a wave
# keeps in registers / the re-read path over three chunks with a tail;
# (300,2,33): long scan, rows not kept; (70,1,65): several kept rows per wave,
# unevenly; (2100,1,33): per-step LDS above 48 KiB.  The fp32 composed
# reference alone meets RTOL/ATOL against fp64 at every shape here (checked
# with this seed on the CPU).
IMPALA_SHAPES = [(1, 1, 33), (5, 3, 64), (3, 2, 65), (9, 2, 121), (2, 1, 513),
                 (2, 1, 1025), (300, 2, 33), (70, 1, 65), (2100, 1, 33)]
# the dispatch edge (32 takes the narrow kernel) and softmax stability
IMPALA_CASES = ([(s, 1.0) for s in IMPALA_SHAPES]
                + [((5, 3, 32), 1.0), ((5, 3, 33), 1.0), ((5, 3, 64), 30.0)])
PPO_SHAPES = [(1, 33), (7, 64), (5, 65), (300, 121), (3, 513), (2, 1025)]


def _ids(s):
    return "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def _impala_inputs(T, B, A, scale=1.0):
    """Seeded CPU inputs (never modified), in impala_loss's order."""
    target, values, bootstrap, actions, rewards, discounts = _inputs(
        T, B, A, scale)
    g = torch.Generator().manual_seed(3)
    behavior = target + 0.5 * torch.randn(T, B, A, generator=g)
    return behavior, target, actions, rewards, discounts, values, bootstrap


@functools.lru_cache(maxsize=None)
def _ppo_inputs(N, A):
    """Seeded CPU inputs (never modified), in ppo_fused_loss's order."""
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(N, A, generator=g)
    actions = torch.randint(0, A, (N,), generator=g)
    actions[0], actions[-1] = 0, A - 1
    logp = F.log_softmax(logits.double(), -1).gather(1, actions[:, None])[:, 0]
    old_logp = (logp + 0.3 * torch.randn(N, generator=g)).float()
    adv, returns, values = torch.randn(3, N, generator=g)
    ratio = (logp - old_logp).exp()
    assert ((ratio - 1).abs() - CLIP).abs().min() > 1e-4  # min() branch is safe
    return logits, values, actions, old_logp, adv, returns


def _impala(fn, inputs, dtype, dev="cpu"):
    """(total, components, vs, dlogits, dvalues) on the CPU."""
    bl, tl, a, r, d, v, boot = (
        t.to(dev, dtype if t.is_floating_point() else None, copy=True)
        for t in inputs)
    tl.requires_grad_()
    v.requires_grad_()
    kw = dict(baseline_cost=BC, entropy_cost=EC)
    if fn is impala_loss:
        total, comps, vs = fn(bl, tl, a, r, d, v, boot, want_vs=True, **kw)
    else:
        total, *comps = fn(bl, tl, a, r, d, v, boot, **kw)
        comps = torch.stack(comps)
        log_rhos = (F.log_softmax(tl, -1) - F.log_softmax(bl, -1)).gather(
            -1, a[..., None])[..., 0].detach()
        vs = vtrace_reference(log_rhos, d, r, v.detach(), boot).vs
    total.backward()
    return tuple(t.detach().cpu() for t in (total, comps, vs, tl.grad, v.grad))


def _ppo(fn, inputs, dtype, dev="cpu"):
    """(total, components, dlogits, dvalues) on the CPU."""
    lg, v, a, old, adv, ret = (
        t.to(dev, dtype if t.is_floating_point() else None, copy=True)
        for t in inputs)
    lg.requires_grad_()
    v.requires_grad_()
    if fn is ppo_fused_loss:
        total, comps = fn(lg, v, a, old, adv, ret, clip_eps=CLIP, vcoef=BC,
                          ecoef=EC)
    else:
        total, *comps = fn(lg, a, old, adv, ret, v, CLIP, BC, EC)
        comps = torch.stack(comps)
    total.backward()
    return tuple(t.detach().cpu() for t in (total, comps, lg.grad, v.grad))


def _compare(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        print(i, "max abs diff", (g - w).abs().max().item(),
              "max |ref|", w.abs().max().item())
    for g, w in zip(got, want):
        assert torch.isfinite(g).all()
        torch.testing.assert_close(g, w.float(), rtol=RTOL, atol=ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,scale", IMPALA_CASES,
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else v)
def test_impala_wide_gpu_matches_fp64_reference(shape, scale):
    inputs = _impala_inputs(*shape, scale)
    _compare(_impala(impala_loss, inputs, torch.float32, "cuda:0"),
             _impala(impala_loss_reference, inputs, torch.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PPO_SHAPES, ids=_ids)
def test_ppo_wide_gpu_matches_fp64_reference(shape):
    inputs = _ppo_inputs(*shape)
    _compare(_ppo(ppo_fused_loss, inputs, torch.float32, "cuda:0"),
             _ppo(ppo_loss_reference, inputs, torch.float64))


@pytest.mark.gpu
def test_wide_gpu_is_deterministic():
    runs = [_impala(impala_loss, _impala_inputs(9, 2, 121), torch.float32,
                    "cuda:0")[2:]
            + _ppo(ppo_fused_loss, _ppo_inputs(300, 121), torch.float32,
                   "cuda:0")[2:] for _ in range(2)]
    for first, second in zip(*runs):
        assert torch.equal(first, second)


@pytest.mark.gpu
def test_impala_wide_gpu_rollout_beyond_lds_bound_raises():
    # 8 per-step arrays: (8*5200 + 50) floats > 160 KiB
    inputs = (t.cuda() for t in _impala_inputs(5200, 1, 33))
    with pytest.raises(RuntimeError, match=r"code -3 \(rollout length"):
        impala_loss(*inputs)
