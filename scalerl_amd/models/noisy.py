"""NoisyNet linear layer + C51 categorical Q-network.

The reference declares ``noisy_dqn`` / ``categorical_dqn`` flags with
v_min/v_max/atoms hyperparams (rl_args.py:163-315) but ships no
implementation; these implement the published semantics (Fortunato et al.
2018 factorised-Gaussian NoisyNet; Bellemare et al. 2017 C51)."""

from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class NoisyLinear(nn.Module):
    """Factorised-Gaussian noisy linear: w = μ_w + σ_w·(ε_out ⊗ ε_in)."""

    def __init__(self, in_features: int, out_features: int,
                 sigma0: float = 0.5):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.weight_mu = nn.Parameter(torch.empty(out_features, in_features))
        self.weight_sigma = nn.Parameter(torch.empty(out_features, in_features))
        self.bias_mu = nn.Parameter(torch.empty(out_features))
        self.bias_sigma = nn.Parameter(torch.empty(out_features))
        self.register_buffer("eps_in", torch.zeros(in_features))
        self.register_buffer("eps_out", torch.zeros(out_features))
        bound = 1.0 / math.sqrt(in_features)
        nn.init.uniform_(self.weight_mu, -bound, bound)
        nn.init.uniform_(self.bias_mu, -bound, bound)
        nn.init.constant_(self.weight_sigma, sigma0 * bound)
        nn.init.constant_(self.bias_sigma, sigma0 * bound)
        self.reset_noise()

    @staticmethod
    def _f(x: torch.Tensor) -> torch.Tensor:
        return x.sign() * x.abs().sqrt()

    @torch.no_grad()
    def reset_noise(self) -> None:
        self.eps_in.copy_(self._f(torch.randn_like(self.eps_in)))
        self.eps_out.copy_(self._f(torch.randn_like(self.eps_out)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:
            w = self.weight_mu + self.weight_sigma * torch.outer(
                self.eps_out, self.eps_in)
            b = self.bias_mu + self.bias_sigma * self.eps_out
        else:
            w, b = self.weight_mu, self.bias_mu
        return F.linear(x, w, b)


def reset_noise(module: nn.Module) -> None:
    for m in module.modules():
        if isinstance(m, NoisyLinear):
            m.reset_noise()


class CategoricalQNet(nn.Module):
    """C51 distributional Q-network over ``num_atoms`` support points."""

    def __init__(self, obs_dim: int, action_dim: int, hidden_dim: int = 128,
                 num_atoms: int = 51, v_min: float = -10.0,
                 v_max: float = 10.0, noisy: bool = False):
        super().__init__()
        self.action_dim = action_dim
        self.num_atoms = num_atoms
        lin = NoisyLinear if noisy else nn.Linear
        self.body = nn.Sequential(
            nn.Linear(obs_dim, hidden_dim), nn.ReLU(),
            nn.Linear(hidden_dim, hidden_dim), nn.ReLU())
        self.head = lin(hidden_dim, action_dim * num_atoms)
        self.register_buffer(
            "support", torch.linspace(v_min, v_max, num_atoms))
        self.v_min, self.v_max = v_min, v_max
        self.delta_z = (v_max - v_min) / (num_atoms - 1)

    def logits(self, obs: torch.Tensor) -> torch.Tensor:
        """→ raw atom logits [B, A, atoms]."""
        h = self.body(obs)
        return self.head(h).view(-1, self.action_dim, self.num_atoms)

    def dist(self, obs: torch.Tensor) -> torch.Tensor:
        """→ log-probabilities [B, A, atoms]."""
        return F.log_softmax(self.logits(obs), dim=-1)

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        """Expected Q-values [B, A]."""
        return (self.dist(obs).exp() * self.support).sum(-1)


def c51_loss(net: CategoricalQNet, target_net: CategoricalQNet, obs, actions,
             rewards, discounts, next_obs, double: bool = True,
             weights=None, *, prios=None, p_total=None, p_min=None,
             beta: float = 0.4, replay_size: int = 0):
    """Categorical projection TD loss (Bellemare et al. 2017, alg. 1).

    Returns (loss scalar, |TD|-style priorities = per-sample KL).

    The nets only produce logits; the loss itself is
    :func:`scalerl_amd.ops.fused_c51_loss` — one HIP kernel on the GPU, the
    composed reference on the CPU.  PER importance-sampling weights come
    from the raw ``prios``/``p_total``/``p_min`` (computed in-kernel on the
    GPU); explicit ``weights`` instead select the composed reference on
    either device."""
    from ..ops.td import c51_loss_reference, fused_c51_loss
    if weights is not None and prios is not None:
        raise ValueError("pass either weights or prios, not both")
    with torch.no_grad():
        next_online = net.logits(next_obs) if double else None
        next_target = target_net.logits(next_obs)
    logits = net.logits(obs)
    if weights is not None:
        return c51_loss_reference(logits, next_online, next_target, actions,
                                  rewards, discounts, net.v_min, net.v_max,
                                  weights)
    return fused_c51_loss(logits, next_online, next_target, actions, rewards,
                          discounts, net.v_min, net.v_max, prios=prios,
                          p_total=p_total, p_min=p_min, beta=beta,
                          replay_size=replay_size)
