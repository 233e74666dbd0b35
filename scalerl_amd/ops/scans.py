"""GAE / discounted-return / n-step scan ops (HIP on GPU, reference on CPU).

Reference semantics: GAE — standard (config-only in the reference,
rl_args.py:338-340); returns — parallel_a3c.py:274-276 / generation.py:142-147;
n-step — replay_buffer.py:230-273.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from ._backend import launch

# the fused A2C loss stages 3 arrays of T*8 floats into 48 KiB of LDS
# (csrc/a2c_loss.h: A2C_MAX_T)
A2C_MAX_T = 512


@torch.no_grad()
def gae_reference(rewards, values, bootstrap_value, discounts, lam: float):
    T = rewards.shape[0]
    adv = torch.zeros_like(bootstrap_value)
    advantages = torch.empty_like(rewards)
    values_tp1 = torch.cat([values[1:], bootstrap_value.unsqueeze(0)], dim=0)
    deltas = rewards + discounts * values_tp1 - values
    for t in range(T - 1, -1, -1):
        adv = deltas[t] + discounts[t] * lam * adv
        advantages[t] = adv
    return advantages, advantages + values


@torch.no_grad()
def gae(rewards, values, bootstrap_value, discounts, lam: float = 0.95):
    """advantages, returns — [T,B] each."""
    if not rewards.is_cuda:
        return gae_reference(rewards, values, bootstrap_value, discounts, lam)
    T, B = rewards.shape
    r = rewards.contiguous().float()
    advantages = torch.empty_like(r)
    returns = torch.empty_like(r)
    launch("gae_scan", r, values.contiguous().float(),
           bootstrap_value.contiguous().float(),
           discounts.contiguous().float(), lam, T, B, advantages, returns,
           None, None, 0, 0.0, 0.0, None, None, None)
    return advantages, returns


def a2c_loss_reference(logits, values, bootstrap_value, actions, rewards,
                       discounts, *, lam: float = 1.0,
                       value_coef: float = 0.5, entropy_coef: float = 0.01):
    """Composed autograd reference of the fused A2C loss (any device and
    dtype): GAE on detached values, then policy gradient + value MSE +
    entropy as means over [T,B].

    Returns (total, components[3] = (pg, value, entropy) detached, returns).
    """
    with torch.no_grad():
        adv, returns = gae(rewards, values.detach(), bootstrap_value.detach(),
                           discounts, lam)
    logp = F.log_softmax(logits, dim=-1)
    taken = logp.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
    pg_loss = -(taken * adv).mean()
    value_loss = 0.5 * F.mse_loss(values, returns)
    entropy = -(logp.exp() * logp).sum(-1).mean()
    total = pg_loss + value_coef * value_loss - entropy_coef * entropy
    comps = torch.stack([pg_loss.detach(), value_loss.detach(),
                         entropy.detach()])
    return total, comps, returns


class _A2CFusedLossFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, logits, values, bootstrap_value, actions, rewards,
                discounts, lam, value_coef, entropy_coef, want_returns):
        T, B, A = logits.shape
        # no zero-filled gradients for components and returns in backward
        ctx.set_materialize_grads(False)
        lg = logits.contiguous().float()
        vals = values.contiguous().float()
        # the kernel writes every element of both gradients
        grad_logits = torch.empty_like(lg)
        grad_values = torch.empty_like(vals)
        loss_out = torch.zeros(3, device=lg.device, dtype=torch.float32)
        returns = torch.empty_like(vals) if want_returns else None
        launch("gae_scan", rewards.contiguous().float(), vals,
               bootstrap_value.contiguous().float(),
               discounts.contiguous().float(), float(lam), T, B, None, returns,
               lg, actions.contiguous().long(), A, float(value_coef),
               float(entropy_coef), grad_logits, grad_values, loss_out)
        ctx.save_for_backward(grad_logits, grad_values)
        total = (loss_out[0] + value_coef * loss_out[1]
                 - entropy_coef * loss_out[2])
        if returns is None:
            returns = loss_out.new_zeros(0)
        ctx.mark_non_differentiable(loss_out, returns)
        return total, loss_out, returns

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_total, g_comps, g_returns):
        if g_total is None:
            return (None,) * 10
        grad_logits, grad_values = ctx.saved_tensors
        return (grad_logits * g_total, grad_values * g_total) + (None,) * 8


def a2c_loss(logits, values, bootstrap_value, actions, rewards, discounts, *,
             lam: float = 1.0, value_coef: float = 0.5,
             entropy_coef: float = 0.01, want_returns: bool = False):
    """GAE(lambda) actor-critic loss with autograd into ``logits`` [T,B,A]
    and ``values`` [T,B].  GPU: one fused HIP launch (csrc/a2c_loss.hip), any
    A >= 1, rollout length T <= ``A2C_MAX_T`` = 512 (the scan's LDS budget;
    longer raises RuntimeError, code -3).  CPU: :func:`a2c_loss_reference`.

    Advantages and returns are constants of the loss and ``bootstrap_value``
    gets no gradient.  An action outside [0,A) makes the GPU loss and that
    row's logits gradient NaN.

    Returns (total, components[3] = (pg, value, entropy) means, returns [T,B]
    or an empty tensor unless ``want_returns``).
    """
    if logits.dim() != 3:
        raise ValueError(f"logits must be [T,B,A], got shape "
                         f"{tuple(logits.shape)}")
    T, B, A = logits.shape
    if min(T, B, A) < 1:
        raise ValueError(f"logits has an empty dimension: {(T, B, A)}")
    for name, t in (("values", values), ("actions", actions),
                    ("rewards", rewards), ("discounts", discounts)):
        if tuple(t.shape) != (T, B):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected "
                             f"{(T, B)}")
    if tuple(bootstrap_value.shape) != (B,):
        raise ValueError(f"bootstrap_value has shape "
                         f"{tuple(bootstrap_value.shape)}, expected ({B},)")
    if logits.is_cuda:
        return _A2CFusedLossFn.apply(
            logits, values, bootstrap_value, actions, rewards, discounts, lam,
            value_coef, entropy_coef, want_returns)
    total, comps, returns = a2c_loss_reference(
        logits, values, bootstrap_value, actions, rewards, discounts, lam=lam,
        value_coef=value_coef, entropy_coef=entropy_coef)
    return total, comps, returns if want_returns else returns.new_zeros(0)


@torch.no_grad()
def discounted_returns(rewards, discounts, bootstrap_value=None):
    """R_t = r_t + discount_t * R_{t+1}, seeded with bootstrap (or 0)."""
    if not rewards.is_cuda:
        T = rewards.shape[0]
        acc = (bootstrap_value.clone() if bootstrap_value is not None
               else torch.zeros_like(rewards[0]))
        out = torch.empty_like(rewards)
        for t in range(T - 1, -1, -1):
            acc = rewards[t] + discounts[t] * acc
            out[t] = acc
        return out
    T, B = rewards.shape
    r = rewards.contiguous().float()
    out = torch.empty_like(r)
    launch("discounted_returns", r, discounts.contiguous().float(),
           bootstrap_value.contiguous().float()
           if bootstrap_value is not None else None, T, B, out)
    return out


@torch.no_grad()
def nstep_fold(rewards, dones, gamma: float, n: int):
    """Per-(t,b): folded n-step reward, done-inside-window flag, steps used.

    folded_r[t] = sum_{k<m} gamma^k r[t+k] with m = min(n, steps to first
    done or end of chunk); matches MultiStepReplayBuffer insert folding.
    """
    if not rewards.is_cuda:
        T, B = rewards.shape
        fr = torch.zeros_like(rewards)
        fd = torch.zeros_like(rewards)
        su = torch.zeros(T, B, dtype=torch.int32)
        for t in range(T):
            for b in range(B):
                acc, g, m, done = 0.0, 1.0, 0, 0.0
                for k in range(n):
                    if t + k >= T:
                        break
                    acc += g * float(rewards[t + k, b])
                    g *= gamma
                    m = k + 1
                    if float(dones[t + k, b]) != 0.0:
                        done = 1.0
                        break
                fr[t, b], fd[t, b], su[t, b] = acc, done, m
        return fr, fd, su
    T, B = rewards.shape
    r = rewards.contiguous().float()
    fr = torch.empty_like(r)
    fd = torch.empty_like(r)
    su = torch.empty(T, B, dtype=torch.int32, device=r.device)
    launch("nstep_fold", r, dones.contiguous().float(), gamma, n, T, B,
           fr, fd, su)
    return fr, fd, su
