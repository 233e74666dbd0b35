"""Fused DQN TD losses — HIP on GPU, composed reference on CPU.

Scalar: double/vanilla target + Huber/MSE + PER IS weights + |TD|
priorities.  Reference semantics: dqn_agent.py:155-171 (double-DQN target +
MSE), apex/worker.py:134-161 (IS weights, priority update).

Categorical (C51, Bellemare et al. 2017 alg. 1): greedy next action from the
expected Q, projection of the target distribution onto the support, cross
entropy against the online row, the same IS weights, per-sample cross entropy
as the new priorities.  Both go through the one ``fused_td_loss`` entry point
of ``csrc/td_loss.hip``.
"""

from __future__ import annotations

from typing import Tuple

import torch

from ._backend import launch


def td_loss_reference(q, q_next_online, q_next_target, actions, rewards,
                      discounts, weights=None, huber=False, huber_delta=1.0):
    """Autograd-capable reference.  Returns (loss, |td| detached)."""
    if q_next_online is not None:
        astar = q_next_online.argmax(dim=1, keepdim=True)
    else:
        astar = q_next_target.argmax(dim=1, keepdim=True)
    target = rewards + discounts * q_next_target.gather(1, astar).squeeze(1)
    pred = q.gather(1, actions.unsqueeze(1)).squeeze(1)
    td = pred - target.detach()
    if huber:
        a = td.abs()
        l = torch.where(a <= huber_delta, 0.5 * td * td,
                        huber_delta * (a - 0.5 * huber_delta))
    else:
        l = td * td
    if weights is not None:
        l = l * weights
    return l.mean(), td.abs().detach()


def per_is_weights(prios, p_total, p_min, replay_size, beta):
    """(N*P)^-beta / max_w with P = p/total (replay_buffer.py:370-381)."""
    w = (replay_size * (prios / p_total)) ** (-beta)
    w_max = (replay_size * (p_min / p_total)) ** (-beta)
    return w / w_max


class _FusedTDLossFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, q, q_next_online, q_next_target, actions, rewards,
                discounts, prios, p_total, p_min, beta, replay_size, huber,
                huber_delta):
        B, A = q.shape
        qc = q.contiguous().float()
        grad_q = torch.zeros_like(qc)
        td_abs = torch.empty(B, device=q.device, dtype=torch.float32)
        loss_out = torch.zeros(1, device=q.device, dtype=torch.float32)
        launch("fused_td_loss", qc,
               q_next_online.contiguous().float()
               if q_next_online is not None else None,
               q_next_target.contiguous().float(),
               actions.contiguous().long(), rewards.contiguous().float(),
               discounts.contiguous().float(), prios, p_total, p_min,
               float(beta), int(replay_size), B, A, int(huber),
               float(huber_delta), 0, 0.0, 0.0, grad_q, td_abs, loss_out)
        ctx.save_for_backward(grad_q)
        ctx.mark_non_differentiable(td_abs)
        return loss_out[0], td_abs

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_loss, g_td):
        (grad_q,) = ctx.saved_tensors
        return (grad_q * g_loss,) + (None,) * 12


def fused_td_loss(q, q_next_online, q_next_target, actions, rewards,
                  discounts, *, prios=None, p_total=None, p_min=None,
                  beta: float = 0.4, replay_size: int = 0,
                  huber: bool = False, huber_delta: float = 1.0
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (loss scalar w/ autograd into q, |td| priorities [B])."""
    if q.is_cuda:
        return _FusedTDLossFn.apply(q, q_next_online, q_next_target, actions,
                                    rewards, discounts, prios, p_total, p_min,
                                    beta, replay_size, huber, huber_delta)
    weights = None
    if prios is not None:
        weights = per_is_weights(prios, p_total, p_min, replay_size, beta)
    return td_loss_reference(q, q_next_online, q_next_target, actions,
                             rewards, discounts, weights, huber, huber_delta)


def c51_loss_reference(logits, next_logits_online, next_logits_target,
                       actions, rewards, discounts, v_min, v_max,
                       weights=None):
    """Autograd-capable composed C51 loss on raw logits [B,A,N].  Returns
    (loss, per-sample cross entropy detached).  ``next_logits_online`` None
    selects the greedy action with the target net (vanilla DQN)."""
    B, _, N = logits.shape
    support = torch.linspace(v_min, v_max, N, dtype=logits.dtype,
                             device=logits.device)
    delta_z = (v_max - v_min) / (N - 1)
    rows = torch.arange(B, device=logits.device)
    with torch.no_grad():
        sel = (next_logits_online if next_logits_online is not None
               else next_logits_target)
        next_q = (torch.log_softmax(sel, dim=-1).exp() * support).sum(-1)
        astar = next_q.argmax(dim=1)
        next_dist = torch.log_softmax(next_logits_target, dim=-1).exp()[
            rows, astar]                                   # [B, atoms]
        tz = (rewards.unsqueeze(1)
              + discounts.unsqueeze(1) * support.unsqueeze(0))
        tz = tz.clamp(v_min, v_max)
        b = (tz - v_min) / delta_z
        lo = b.floor().long().clamp(0, N - 1)
        hi = b.ceil().long().clamp(0, N - 1)
        proj = torch.zeros_like(next_dist)
        # distribute mass to the two neighbouring atoms
        lo_w = (hi.float() - b).where(hi != lo, torch.ones_like(b))
        hi_w = (b - lo.float())
        proj.scatter_add_(1, lo, next_dist * lo_w)
        proj.scatter_add_(1, hi, next_dist * hi_w)
    log_p = torch.log_softmax(logits, dim=-1)[rows, actions]  # [B, atoms]
    kl = -(proj * log_p).sum(dim=1)
    loss = (kl * weights).mean() if weights is not None else kl.mean()
    return loss, kl.detach()


class _FusedC51LossFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, logits, next_logits_online, next_logits_target, actions,
                rewards, discounts, prios, p_total, p_min, beta, replay_size,
                v_min, v_max):
        B, A, N = logits.shape
        # no zero-filled gradient for the non-differentiable kl in backward
        ctx.set_materialize_grads(False)
        lc = logits.contiguous().float()
        grad = torch.empty_like(lc)  # the kernel writes every element
        kl = torch.empty(B, device=lc.device, dtype=torch.float32)
        loss_out = torch.zeros(1, device=lc.device, dtype=torch.float32)
        launch("fused_td_loss", lc,
               next_logits_online.contiguous().float()
               if next_logits_online is not None else None,
               next_logits_target.contiguous().float(),
               actions.contiguous().long(), rewards.contiguous().float(),
               discounts.contiguous().float(), prios, p_total, p_min,
               float(beta), int(replay_size), B, A, 0, 0.0, N, float(v_min),
               float(v_max), grad, kl, loss_out)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(kl)
        return loss_out[0], kl

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_loss, g_kl):
        if g_loss is None:
            return (None,) * 13
        (grad,) = ctx.saved_tensors
        return (grad * g_loss,) + (None,) * 12


def fused_c51_loss(logits, next_logits_online, next_logits_target, actions,
                   rewards, discounts, v_min: float, v_max: float, *,
                   prios=None, p_total=None, p_min=None, beta: float = 0.4,
                   replay_size: int = 0
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """C51 categorical TD loss on raw logits [B,A,N].  Returns (loss scalar
    w/ autograd into ``logits``, per-sample cross entropy [B] — the new
    priorities)."""
    if logits.dim() != 3:
        raise ValueError(f"logits must be [B,A,atoms], got shape "
                         f"{tuple(logits.shape)}")
    B, A, N = logits.shape
    if N < 2:
        raise ValueError(f"C51 needs at least 2 atoms, got {N}")
    if not v_max > v_min:
        raise ValueError(f"v_max ({v_max}) must exceed v_min ({v_min})")
    for name, t in (("next_logits_online", next_logits_online),
                    ("next_logits_target", next_logits_target)):
        if t is None and name == "next_logits_online":
            continue
        if tuple(t.shape) != (B, A, N):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, logits "
                             f"{(B, A, N)}: batch, actions and atoms must "
                             f"match")
    for name, t in (("actions", actions), ("rewards", rewards),
                    ("discounts", discounts), ("prios", prios)):
        if t is not None and tuple(t.shape) != (B,):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected "
                             f"({B},)")
    if prios is not None and (p_total is None or p_min is None):
        raise ValueError("prios needs p_total and p_min")
    if logits.is_cuda:
        return _FusedC51LossFn.apply(
            logits, next_logits_online, next_logits_target, actions, rewards,
            discounts, prios, p_total, p_min, beta, replay_size, v_min, v_max)
    weights = None
    if prios is not None:
        weights = per_is_weights(prios, p_total, p_min, replay_size, beta)
    return c51_loss_reference(logits, next_logits_online, next_logits_target,
                              actions, rewards, discounts, v_min, v_max,
                              weights)
