"""Fused QR-DQN quantile-Huber loss, on the GPU against the fp64 reference."""

import functools

import pytest
import torch

from scalerl_amd.config import DQNArguments
from scalerl_amd.ops import fused_qr_loss, per_is_weights, qr_loss_reference
from scalerl_amd.runtime.dqn import DQNAgent

PER = dict(p_total=10.0, p_min=0.1, replay_size=1000, beta=0.4)


def test_qr_reference_hand_golden():
    # N=2: tau = [.25, .75].  Target row 0 (mean 2.5) beats row 1 (mean -1);
    # r = d = 0.5 gives T = [0.5, 3].  Taken online row theta = [0, 1], k = 1:
    #   i=0: u = [ 0.5, 3]: .25 * .125 (quadratic), .25 * 2.5 (linear)
    #   i=1: u = [-0.5, 2]: .25 * .125 (u < 0),     .75 * 1.5 (linear)
    #   l = (.03125 + .625)/2 + (.03125 + 1.125)/2 = 0.90625
    #   dl/dtheta_0 = -(.25 * .5 + .25 * 1)/2 = -0.1875
    #   dl/dtheta_1 = -(.25 * -.5 + .75 * 1)/2 = -0.3125
    theta = torch.tensor([[[0.0, 1.0], [7.0, -7.0]]], requires_grad=True)
    xt = torch.tensor([[[0.0, 5.0], [-1.0, -1.0]]])
    loss, ql = fused_qr_loss(theta, None, xt, torch.tensor([0]),
                             torch.tensor([0.5]), torch.tensor([0.5]), 1.0)
    loss.backward()
    assert loss.item() == ql.item() == 0.90625
    assert theta.grad.tolist() == [[[-0.1875, -0.3125], [0.0, 0.0]]]


def test_fused_qr_loss_argument_checks():
    x, xo, xt, a, r, d, prios = _inputs(5, 3, 51)
    ok = (x, xo, xt, a, r, d)
    fused_qr_loss(*ok)
    for args in [
        (x[:, :, :50], xo, xt, a, r, d),    # quantile count
        (x, xo[:, :2], xt, a, r, d),        # action count
        (x, xo, xt[:4], a, r, d),           # batch
        (x, xo, xt, a, r[:4], d),
        (x[:, :, 0], xo, xt, a, r, d),      # not [B,A,N]
        (x[:, :, :1], xo[:, :, :1], xt[:, :, :1], a, r, d),
        (x, xo, xt, a, r, d, 0.0),          # kappa = 0 is another loss
        (x, xo, xt, a, r, d, -1.0),
    ]:
        with pytest.raises(ValueError):
            fused_qr_loss(*args)
    with pytest.raises(ValueError):
        fused_qr_loss(*ok, prios=prios)  # no p_total / p_min
    with pytest.raises(ValueError, match="quantile_dqn and categorical_dqn"):
        DQNAgent(DQNArguments(quantile_dqn=True, categorical_dqn=True), 4, 3)


def _agent_and_batch(per, dev="cpu", B=16):
    torch.manual_seed(0)
    args = DQNArguments(quantile_dqn=True, num_quantiles=11, hidden_dim=32)
    agent = DQNAgent(args, obs_dim=4, action_dim=3, device=dev)
    g = torch.Generator().manual_seed(1)
    batch = {"obs": torch.randn(B, 4, generator=g),
             "next_obs": torch.randn(B, 4, generator=g),
             "action": torch.randint(0, 3, (B,), generator=g),
             "reward": torch.randn(B, generator=g),
             "discount": 0.99 * (torch.rand(B, generator=g) > 0.2).float()}
    if per:
        batch["priorities"] = (torch.rand(B, generator=g) + 0.1).to(dev)
        agent.set_per_stats(torch.tensor([PER["p_total"]], device=dev),
                            torch.tensor([PER["p_min"]], device=dev))
    return args, agent, batch


@pytest.mark.parametrize("per", [False, True])
def test_quantile_dqn_learn_steps_cpu(per):
    _, agent, batch = _agent_and_batch(per)
    before = agent.flat.flat.clone()
    for _ in range(2):
        stats = agent.learn(batch, replay_size=PER["replay_size"])
        assert torch.isfinite(stats["loss"])
    assert not torch.equal(agent.flat.flat, before)


# GPU sweep, each the smallest shape at which one mechanism can break: the
# minimum; N below a wave; the lane stride at 63/64/65; the default N; the cap
# (largest LDS); more actions than waves and an odd B; B above the grid cap of
# 1024 blocks (a second grid-stride trip)
SHAPES = [(1, 1, 2), (5, 3, 51), (9, 4, 63), (9, 4, 64), (9, 4, 65),
          (7, 2, 200), (3, 5, 1024), (67, 18, 8), (1025, 1, 2)]
KAPPAS = [1.0, 0.25]

# Tolerance basis: qr_loss_reference in fp32 against itself in fp64, on the
# CPU, over SHAPES x double x per x KAPPAS (144 runs, the reference and not
# the kernel).  Largest max|err| / max|ref| of one output: loss 1.49e-7, per-
# sample loss 1.26e-7, gradient 3.92e-7.  Largest max|err| of the gradient,
# the one output with elements near zero (the sum over j cancels), where a
# relative bound says nothing: 1.19e-7.  Margin 8 on both: the kernel adds up
# to 1024 fp32 terms in another order and the loss over up to 1024 atomics.
RTOL, ATOL = 8 * 3.92e-7, 8 * 1.19e-7


@functools.lru_cache(maxsize=None)
def _inputs(B, A, N, seed=3):
    """Seeded fp32 CPU inputs, never modified; one action per sample leads."""
    g = torch.Generator().manual_seed(seed)
    x, xo, xt = (torch.randn(B, A, N, generator=g) for _ in range(3))
    for t in (xo, xt):
        t[torch.arange(B), torch.randint(0, A, (B,), generator=g)] += 1.5
    a = torch.randint(0, A, (B,), generator=g)
    r = 2 * torch.rand(B, generator=g) - 1
    d = 0.99 * (torch.rand(B, generator=g) > 0.2).float()
    prios = torch.rand(B, generator=g) + 0.1
    return x, xo, xt, a, r, d, prios


def _assert_greedy_gap(sel):
    """A clear greedy winner per sample: fp32 cannot pick another action."""
    if sel.shape[1] >= 2:
        top = sel.double().mean(-1).topk(2, dim=1).values
        gap = (top[:, 0] - top[:, 1]).min().item()
        assert gap >= 1e-3, gap


@functools.lru_cache(maxsize=None)
def _reference(shape, double, per, kappa, dtype=torch.float64):
    x, xo, xt, a, r, d, prios = _inputs(*shape)
    xo = xo if double else None
    _assert_greedy_gap(xt if xo is None else xo)
    if x.shape[2] >= 51:  # both branches of L_kappa hold >= 5 % of the pairs
        T = r[:, None, None] + d[:, None, None] * xt          # every action's
        u = T[:, :, None, :] - x[torch.arange(len(a)), a][:, None, :, None]
        assert 0.05 <= (u.abs() <= kappa).float().mean().item() <= 0.95
    w = per_is_weights(prios.to(dtype), PER["p_total"], PER["p_min"],
                       PER["replay_size"], PER["beta"]) if per else None
    xg = x.to(dtype).clone().requires_grad_()
    loss, ql = qr_loss_reference(
        xg, None if xo is None else xo.to(dtype), xt.to(dtype), a,
        r.to(dtype), d.to(dtype), kappa, w)
    loss.backward()
    return loss.detach(), ql, xg.grad


def _run_kernel(shape, double, per, kappa, dev="cuda:0"):
    x, xo, xt, a, r, d, prios = (t.to(dev) for t in _inputs(*shape))
    kw = dict(prios=prios, p_total=torch.tensor([PER["p_total"]], device=dev),
              p_min=torch.tensor([PER["p_min"]], device=dev),
              beta=PER["beta"], replay_size=PER["replay_size"]) if per else {}
    xg = x.clone().requires_grad_()
    loss, ql = fused_qr_loss(xg, xo if double else None, xt, a, r, d, kappa,
                             **kw)
    assert not ql.requires_grad
    loss.backward()
    return loss.detach().cpu(), ql.cpu(), xg.grad.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_qr_gpu_matches_fp64_reference(shape, double, per, kappa):
    want = _reference(shape, double, per, kappa)
    for g, w in zip(_run_kernel(shape, double, per, kappa), want):
        assert torch.isfinite(g).all()
        torch.testing.assert_close(g.double(), w, rtol=RTOL, atol=ATOL)


@pytest.mark.gpu
def test_fused_qr_gpu_is_deterministic():
    _, ql1, g1 = _run_kernel((67, 18, 8), True, True, 1.0)
    _, ql2, g2 = _run_kernel((67, 18, 8), True, True, 1.0)
    assert torch.equal(ql1, ql2)
    assert torch.equal(g1, g2)


@pytest.mark.gpu
def test_fused_qr_gpu_quantile_cap_raises():
    x = torch.zeros(1, 1, 1025, device="cuda:0")
    one = torch.ones(1, device="cuda:0")
    with pytest.raises(RuntimeError, match=r"code -4"):
        fused_qr_loss(x, None, x.clone(), torch.zeros_like(one).long(), one,
                      one)


@pytest.mark.gpu
def test_quantile_dqn_learn_issues_one_fused_launch(monkeypatch):
    from scalerl_amd.ops import td
    args, agent, batch = _agent_and_batch(per=True, dev="cuda:0")
    calls = []
    real_launch = td.launch
    monkeypatch.setattr(
        td, "launch", lambda n, *a: calls.append((n, a)) or real_launch(n, *a))
    agent.learn(batch, replay_size=PER["replay_size"])
    assert [c[0] for c in calls] == ["fused_td_loss"]
    # ... B, A, huber, huber_delta, atoms, v_min, v_max
    assert calls[0][1][13:16] == (2, args.huber_kappa, args.num_quantiles)
