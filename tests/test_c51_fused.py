"""Fused C51 categorical TD loss: CPU parity with the composed loss it
replaces, the kernel's formulas emulated in fp64, and the HIP kernel against
the composed reference on the CPU."""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from scalerl_amd.models.atari import CategoricalAtariQNet
from scalerl_amd.models.noisy import CategoricalQNet, c51_loss
from scalerl_amd.ops import (c51_loss_reference, fused_c51_loss,
                             per_is_weights)

V_MIN, V_MAX = -10.0, 10.0
# the project's TD-loss tolerances (tests/test_td.py)
RTOL, ATOL = 1e-4, 1e-5
PER = dict(p_total=10.0, p_min=0.1, replay_size=1000, beta=0.4)


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------

def _frozen_c51_loss(net, target_net, obs, actions, rewards, discounts,
                     next_obs, double=True, weights=None):
    """The composed loss exactly as models/noisy.py had it before the fused
    kernel: the yardstick for bit-identical CPU results."""
    B = obs.shape[0]
    with torch.no_grad():
        next_q = (net if double else target_net)(next_obs)
        astar = next_q.argmax(dim=1)
        next_dist = target_net.dist(next_obs).exp()[
            torch.arange(B), astar]                       # [B, atoms]
        tz = (rewards.unsqueeze(1)
              + discounts.unsqueeze(1) * net.support.unsqueeze(0))
        tz = tz.clamp(net.v_min, net.v_max)
        b = (tz - net.v_min) / net.delta_z
        lo = b.floor().long().clamp(0, net.num_atoms - 1)
        hi = b.ceil().long().clamp(0, net.num_atoms - 1)
        proj = torch.zeros_like(next_dist)
        # distribute mass to the two neighbouring atoms
        lo_w = (hi.float() - b).where(hi != lo, torch.ones_like(b))
        hi_w = (b - lo.float())
        proj.scatter_add_(1, lo, next_dist * lo_w)
        proj.scatter_add_(1, hi, next_dist * hi_w)
    log_p = net.dist(obs)[torch.arange(B), actions]       # [B, atoms]
    kl = -(proj * log_p).sum(dim=1)
    loss = (kl * weights).mean() if weights is not None else kl.mean()
    return loss, kl.detach()


def _nets_and_batch(seed=0, B=24, obs_dim=5, A=4, atoms=51):
    torch.manual_seed(seed)
    net = CategoricalQNet(obs_dim, A, hidden_dim=32, num_atoms=atoms)
    target = CategoricalQNet(obs_dim, A, hidden_dim=32, num_atoms=atoms)
    g = torch.Generator().manual_seed(seed + 1)
    obs = torch.randn(B, obs_dim, generator=g)
    next_obs = torch.randn(B, obs_dim, generator=g)
    actions = torch.randint(0, A, (B,), generator=g)
    rewards = 4 * torch.randn(B, generator=g)
    rewards[0], rewards[1] = 50.0, -50.0
    discounts = 0.99 * (torch.rand(B, generator=g) > 0.2).float()
    rewards[2], discounts[2] = 0.0, 1.0
    prios = torch.rand(B, generator=g) + 0.1
    return net, target, (obs, actions, rewards, discounts, next_obs), prios


@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("mode", ["plain", "weights", "prios"])
def test_c51_loss_cpu_bit_identical_to_frozen_copy(double, mode):
    net, target, batch, prios = _nets_and_batch()
    net_old = copy.deepcopy(net)
    w = per_is_weights(prios, torch.tensor(PER["p_total"]),
                       torch.tensor(PER["p_min"]), PER["replay_size"],
                       PER["beta"])
    kw = {}
    if mode == "weights":
        kw = dict(weights=w)
    elif mode == "prios":
        kw = dict(prios=prios, p_total=torch.tensor(PER["p_total"]),
                  p_min=torch.tensor(PER["p_min"]),
                  replay_size=PER["replay_size"], beta=PER["beta"])
    loss, kl = c51_loss(net, target, *batch, double=double, **kw)
    loss_old, kl_old = _frozen_c51_loss(
        net_old, target, *batch, double=double,
        weights=None if mode == "plain" else w)
    assert torch.equal(loss, loss_old)
    assert torch.equal(kl, kl_old)
    assert not kl.requires_grad
    loss.backward()
    loss_old.backward()
    for p, p_old in zip(net.parameters(), net_old.parameters()):
        assert torch.equal(p.grad, p_old.grad)
    assert all(p.grad is None for p in target.parameters())


def test_c51_reference_hand_golden():
    # N=3 on [-1,1]: z = [-1,0,1], dz = 1.  r=0.5, d=0 puts every atom of the
    # target at Tz = 0.5, b = 1.5: half the mass on atom 1, half on atom 2,
    # whatever the target distribution is.
    x = torch.tensor([[[0.3, -0.2, 1.0]]])
    tgt = torch.zeros(1, 1, 3)
    loss, kl = c51_loss_reference(
        x, None, tgt, torch.tensor([0]), torch.tensor([0.5]),
        torch.tensor([0.0]), -1.0, 1.0)
    want = torch.logsumexp(x[0, 0], 0) - 0.5 * (x[0, 0, 1] + x[0, 0, 2])
    assert kl.item() == pytest.approx(want.item(), rel=1e-6)
    assert loss.item() == pytest.approx(want.item(), rel=1e-6)
    loss2, kl2 = fused_c51_loss(
        x, None, tgt, torch.tensor([0]), torch.tensor([0.5]),
        torch.tensor([0.0]), -1.0, 1.0)
    assert torch.equal(kl2, kl) and torch.equal(loss2, loss)


@functools.lru_cache(maxsize=None)
def _inputs(B, A, N, seed=7, scale=1.0):
    """Seeded inputs of the GPU sweep (CPU tensors; never modified).  The
    seed is one for which _assert_greedy_gap holds on every shape used."""
    g = torch.Generator().manual_seed(seed)
    z = torch.linspace(V_MIN, V_MAX, N)
    x, xo, xt = (torch.randn(B, A, N, generator=g) for _ in range(3))
    xt = 3 * xt
    rows = torch.arange(B)
    for t in (x, xo, xt):  # one action per sample leans towards high returns
        t[rows, torch.randint(0, A, (B,), generator=g)] += 2 * z / V_MAX
    a = torch.randint(0, A, (B,), generator=g)
    r = 4 * torch.randn(B, generator=g)
    d = 0.99 * (torch.rand(B, generator=g) > 0.2).float()
    r[0] = 50.0
    if B > 1:
        r[1] = -50.0
    if B > 2:
        r[2], d[2] = 0.0, 1.0  # b lands on integers
    prios = torch.rand(B, generator=g) + 0.1
    return tuple(t * scale for t in (x, xo, xt)) + (a, r, d, prios)


def _assert_greedy_gap(sel, N):
    """The greedy action is a discontinuity: require a clear winner for every
    sample, so that fp32 rounding cannot pick another action."""
    if sel.shape[1] < 2:
        return
    z = torch.linspace(V_MIN, V_MAX, N, dtype=sel.dtype)
    q = (torch.softmax(sel, -1) * z).sum(-1)
    top = q.topk(2, dim=1).values
    gap = (top[:, 0] - top[:, 1]).min().item()
    assert gap >= 1e-2, gap


def _kernel_formulas(x, xo, xt, a, r, d, w):
    """c51_loss_kernel's per-sample math, vectorised, in the input dtype."""
    B, A, N = x.shape
    k = torch.arange(N, dtype=x.dtype)
    dz = (V_MAX - V_MIN) / (N - 1)
    z = V_MIN + k * dz
    rows = torch.arange(B)
    sel = xt if xo is None else xo
    e = (sel - sel.max(-1, keepdim=True).values).exp()
    astar = ((e * z).sum(-1) / e.sum(-1)).argmax(1)
    trow = xt[rows, astar]
    e = (trow - trow.max(-1, keepdim=True).values).exp()
    p = e / e.sum(-1, keepdim=True)
    b = ((r[:, None] + d[:, None] * z).clamp(V_MIN, V_MAX) - V_MIN) / dz
    tri = (1 - (b[:, :, None] - k[None, None, :]).abs()).clamp(min=0)
    m = (p[:, :, None] * tri).sum(1)                       # [B, N] over k
    orow = x[rows, a]
    logp = orow - torch.logsumexp(orow, -1, keepdim=True)
    kl = -(m * logp).sum(-1)
    grad = torch.zeros_like(x)
    grad[rows, a] = (w / B)[:, None] * (logp.exp() * m.sum(-1, keepdim=True)
                                        - m)
    return (w * kl).mean(), kl, grad, m


def _scatter_projection(xo, xt, r, d):
    """The lo/hi scatter of the composed loss, on its own."""
    B, A, N = xt.shape
    z = torch.linspace(V_MIN, V_MAX, N, dtype=xt.dtype)
    sel = xt if xo is None else xo
    astar = (torch.softmax(sel, -1) * z).sum(-1).argmax(1)
    p = torch.softmax(xt, -1)[torch.arange(B), astar]
    b = ((r[:, None] + d[:, None] * z).clamp(V_MIN, V_MAX) - V_MIN) / (
        (V_MAX - V_MIN) / (N - 1))
    lo = b.floor().long().clamp(0, N - 1)
    hi = b.ceil().long().clamp(0, N - 1)
    proj = torch.zeros_like(p)
    proj.scatter_add_(1, lo, p * (hi - b).where(hi != lo, torch.ones_like(b)))
    proj.scatter_add_(1, hi, p * (b - lo))
    return proj


@pytest.mark.parametrize("double", [True, False])
def test_c51_kernel_formula_emulation_matches_autograd(double):
    """The gather-form projection against the lo/hi scatter, and the analytic
    gradient against autograd of the composed reference, in fp64 — validates
    the kernel's math without a GPU."""
    B, A, N = 67, 6, 51
    x, xo, xt, a, r, d, prios = _inputs(B, A, N)
    x, xo, xt, r, d, prios = (t.double() for t in (x, xo, xt, r, d, prios))
    if not double:
        xo = None
    _assert_greedy_gap(xt if xo is None else xo, N)
    w = per_is_weights(prios, PER["p_total"], PER["p_min"],
                       PER["replay_size"], PER["beta"])
    loss, kl, grad, m = _kernel_formulas(x, xo, xt, a, r, d, w)

    xg = x.clone().requires_grad_()
    loss_ref, kl_ref = c51_loss_reference(xg, xo, xt, a, r, d, V_MIN, V_MAX,
                                          w)
    loss_ref.backward()
    torch.testing.assert_close(m, _scatter_projection(xo, xt, r, d),
                               rtol=0, atol=1e-12)
    torch.testing.assert_close(kl, kl_ref, rtol=0, atol=1e-12)
    torch.testing.assert_close(loss, loss_ref.detach(), rtol=0, atol=1e-12)
    torch.testing.assert_close(grad, xg.grad, rtol=0, atol=1e-12)
    torch.testing.assert_close(m.sum(-1), torch.ones(B, dtype=m.dtype),
                               rtol=0, atol=1e-12)
    # both clamped ends and the integer-b sample carry the expected mass
    assert m[0, N - 1].item() == pytest.approx(1.0, abs=1e-12)
    assert m[1, 0].item() == pytest.approx(1.0, abs=1e-12)


def test_models_expose_logits():
    torch.manual_seed(0)
    mlp = CategoricalQNet(5, 3, hidden_dim=16, num_atoms=7)
    obs = torch.randn(4, 5)
    assert mlp.logits(obs).shape == (4, 3, 7)
    assert torch.equal(mlp.dist(obs), F.log_softmax(mlp.logits(obs), -1))
    cnn = CategoricalAtariQNet((4, 84, 84), num_actions=3, num_atoms=7)
    frames = torch.randint(0, 256, (2, 4, 84, 84), dtype=torch.uint8)
    assert cnn.logits(frames).shape == (2, 3, 7)
    assert torch.equal(cnn.dist(frames), F.log_softmax(cnn.logits(frames), -1))


def test_fused_c51_loss_argument_checks():
    x, xo, xt, a, r, d, prios = _inputs(5, 3, 51)
    ok = (x, xo, xt, a, r, d, V_MIN, V_MAX)
    fused_c51_loss(*ok)
    bad = [
        (x[:, :, :50], xo, xt, a, r, d, V_MIN, V_MAX),   # atom count
        (x, xo[:, :2], xt, a, r, d, V_MIN, V_MAX),       # action count
        (x, xo, xt[:4], a, r, d, V_MIN, V_MAX),          # batch
        (x, xo, xt, a[:4], r, d, V_MIN, V_MAX),
        (x, xo, xt, a, r[:4], d, V_MIN, V_MAX),
        (x, xo, xt, a, r, d[:4], V_MIN, V_MAX),
        (x[:, :, 0], xo, xt, a, r, d, V_MIN, V_MAX),     # not [B,A,N]
        (x[:, :, :1], xo[:, :, :1], xt[:, :, :1], a, r, d, V_MIN, V_MAX),
        (x, xo, xt, a, r, d, V_MAX, V_MIN),              # empty support
    ]
    for args in bad:
        with pytest.raises(ValueError):
            fused_c51_loss(*args)
    with pytest.raises(ValueError):
        fused_c51_loss(*ok, prios=prios[:4], p_total=torch.tensor([10.0]),
                       p_min=torch.tensor([0.1]))
    with pytest.raises(ValueError):
        fused_c51_loss(*ok, prios=prios)  # no p_total / p_min


# --------------------------------------------------------------------------
# GPU: the kernel against c51_loss_reference on the CPU
# --------------------------------------------------------------------------

SHAPES = [(1, 1, 2), (5, 3, 51), (67, 18, 51), (67, 6, 64), (9, 4, 65),
          (7, 2, 200)]


def _reference(inputs, double, per):
    x, xo, xt, a, r, d, prios = inputs
    N = x.shape[2]
    if not double:
        xo = None
    _assert_greedy_gap(xt if xo is None else xo, N)
    w = None
    if per:
        w = per_is_weights(prios, torch.tensor(PER["p_total"]),
                           torch.tensor(PER["p_min"]), PER["replay_size"],
                           PER["beta"])
    xg = x.clone().requires_grad_()
    loss, kl = c51_loss_reference(xg, xo, xt, a, r, d, V_MIN, V_MAX, w)
    loss.backward()
    return loss.detach(), kl, xg.grad


def _run_kernel(inputs, double, per, dev="cuda:0"):
    x, xo, xt, a, r, d, prios = (t.to(dev) for t in inputs)
    kw = {}
    if per:
        kw = dict(prios=prios,
                  p_total=torch.tensor([PER["p_total"]], device=dev),
                  p_min=torch.tensor([PER["p_min"]], device=dev),
                  beta=PER["beta"], replay_size=PER["replay_size"])
    xg = x.clone().requires_grad_()
    loss, kl = fused_c51_loss(xg, xo if double else None, xt, a, r, d, V_MIN,
                              V_MAX, **kw)
    assert not kl.requires_grad
    loss.backward()
    return loss.detach().cpu(), kl.cpu(), xg.grad.cpu()


def _compare(got, want):
    for name, g, w in zip(("loss", "kl", "grad_logits"), got, want):
        print(name, "max abs diff", (g - w).abs().max().item(),
              "max |ref|", w.abs().max().item())
    for g, w in zip(got, want):
        assert torch.isfinite(g).all()
        torch.testing.assert_close(g, w, rtol=RTOL, atol=ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_c51_gpu_matches_reference(shape, double, per):
    inputs = _inputs(*shape)
    _compare(_run_kernel(inputs, double, per),
             _reference(inputs, double, per))


@pytest.mark.gpu
def test_fused_c51_gpu_softmax_stability():
    inputs = _inputs(5, 3, 51, scale=30.0)  # all three logits tensors x 30
    _compare(_run_kernel(inputs, True, True), _reference(inputs, True, True))


@pytest.mark.gpu
def test_fused_c51_gpu_is_deterministic():
    inputs = _inputs(67, 18, 51)
    _, kl1, g1 = _run_kernel(inputs, True, True)
    _, kl2, g2 = _run_kernel(inputs, True, True)
    assert torch.equal(kl1, kl2)
    assert torch.equal(g1, g2)


@pytest.mark.gpu
def test_fused_c51_gpu_atom_cap_raises():
    dev = "cuda:0"
    N = 1025
    x = torch.zeros(1, 1, N, device=dev)
    with pytest.raises(RuntimeError, match=r"code -4 \(atom count"):
        fused_c51_loss(x, None, x.clone(), torch.zeros(1, dtype=torch.long,
                                                       device=dev),
                       torch.zeros(1, device=dev), torch.ones(1, device=dev),
                       V_MIN, V_MAX)


@pytest.mark.gpu
@pytest.mark.parametrize("per", [False, True])
def test_categorical_dqn_learn_issues_one_fused_launch(per, monkeypatch):
    from scalerl_amd.config import DQNArguments
    from scalerl_amd.ops import td
    from scalerl_amd.runtime.dqn import DQNAgent
    dev = "cuda:0"
    torch.manual_seed(0)
    args = DQNArguments(categorical_dqn=True, num_atoms=21, hidden_dim=32,
                        seed=0)
    agent = DQNAgent(args, obs_dim=4, action_dim=3, device=dev)
    with torch.no_grad():  # online and target nets must differ
        agent.target_flat.flat.add_(
            0.1 * torch.randn_like(agent.target_flat.flat))
    g = torch.Generator().manual_seed(1)
    B = 16
    batch = {"obs": torch.randn(B, 4, generator=g),
             "next_obs": torch.randn(B, 4, generator=g),
             "action": torch.randint(0, 3, (B,), generator=g),
             "reward": torch.randn(B, generator=g),
             "discount": 0.99 * (torch.rand(B, generator=g) > 0.2).float()}
    weights = None
    if per:
        batch["priorities"] = (torch.rand(B, generator=g) + 0.1).to(dev)
        agent.set_per_stats(torch.tensor([PER["p_total"]], device=dev),
                            torch.tensor([PER["p_min"]], device=dev))
        weights = per_is_weights(batch["priorities"], PER["p_total"],
                                 PER["p_min"], PER["replay_size"],
                                 args.per_beta)

    # the expected loss, from the same nets' logits, before learn() steps them
    agent.model.train()
    with torch.no_grad():
        obs, nobs = batch["obs"].to(dev), batch["next_obs"].to(dev)
        want, want_kl = c51_loss_reference(
            agent.model.logits(obs),
            agent.model.logits(nobs) if args.double_dqn else None,
            agent.target_model.logits(nobs), batch["action"].to(dev),
            batch["reward"].to(dev), batch["discount"].to(dev), args.v_min,
            args.v_max, weights)

    calls = []
    real_launch = td.launch

    def spy(name, *a):
        calls.append((name, a))
        return real_launch(name, *a)

    monkeypatch.setattr(td, "launch", spy)
    stats = agent.learn(batch, replay_size=PER["replay_size"])
    assert [c[0] for c in calls] == ["fused_td_loss"]
    atoms = calls[0][1][15]  # ... huber, huber_delta, atoms, v_min, v_max
    assert atoms == 21
    torch.testing.assert_close(stats["loss"].cpu(), want.cpu(), rtol=RTOL,
                               atol=ATOL)
    torch.testing.assert_close(stats["td_abs"].cpu(), want_kl.cpu(),
                               rtol=RTOL, atol=ATOL)
