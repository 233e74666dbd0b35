"""A3C at GPU scale — batched synchronous A2C on the actor-learner runtime
(BASELINE config 2: Pong 42×42, 16 CPU actors + 1 MI355X learner).

Reference counterpart: ``parallel_a3c.py:71-513`` (hogwild A3C with the
4-conv+LSTM 42×42 policy, ``a3c/utils/atari_model.py:57-144``).  Hogwild's
shared-memory gradient publication does not scale to a GPU learner, so the
MI355X design batches it: N CPU actor processes fill shared rollout slots
(the IMPALA transport, parallel/rollout.py) with 42×42 float observations;
the learner gathers K slots into a [T+1, K*E] batch, unrolls the
A3CAtariNet over T with done-masked MaskedLSTM, computes GAE advantages and
the A2C loss (policy gradient + value MSE + entropy) with their gradients
in one fused HIP launch (ops/scans.py ``a2c_loss``), steps a fused Adam on
the flat parameter buffer, and publishes weights back to the actors with one
flat D2H copy.

The CPU-hogwild parity mode lives in :mod:`scalerl_amd.runtime.a3c`; this
module is the GPU-scale path for the same algorithm family.
"""

from __future__ import annotations

import os
import time
from functools import partial
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from ..config import A3CGpuArguments
from ..models.a3c_atari import A3CAtariNet
from ..ops import FusedAdam, a2c_loss, clip_grad_norm_
from ..parallel import FlatParams, all_reduce_flat
from ..parallel.rollout import BatchGatherer, RolloutStore, actor_loop
from ..utils.checkpoint import save_checkpoint
from .actor_learner import ActorLearnerTrainer


class A3CLocalPolicy:
    """Actor-side CPU inference for A3CAtariNet (LocalPolicy call contract,
    parallel/rollout.py): one LSTM step with done masking, multinomial
    action sampling (the reference's train-mode behavior)."""

    def __init__(self, model: A3CAtariNet, num_envs: int):
        self.model = model
        self.state = model.initial_state(num_envs)

    @torch.no_grad()
    def __call__(self, obs, reward, done, last_action, want_state=False):
        snap = None
        if want_state:
            snap = torch.stack([self.state[0], self.state[1]])  # [2,L,E,H]
        notdone = (~done).float().unsqueeze(0)  # [1,E]
        # done-mask BEFORE the step (MaskedLSTM masks in-kernel per step)
        logits, _, self.state = self.model(obs.float(), self.state, notdone)
        probs = F.softmax(logits, dim=-1)
        action = torch.multinomial(probs, 1).squeeze(-1)
        return action, logits, snap


def a3c_local_policy(model: A3CAtariNet, actor_id: int,
                     num_envs: int) -> A3CLocalPolicy:
    """Policy factory for :func:`scalerl_amd.parallel.rollout.actor_loop`
    (reference: parallel_a3c.py:327-389 rollout phase)."""
    model.eval()
    return A3CLocalPolicy(model, num_envs)


class A3CGpuTrainer(ActorLearnerTrainer):
    def __init__(self, args: A3CGpuArguments, device: Optional[str] = None):
        if args.fused_encoder and args.dtype != "bf16":
            raise ValueError(
                f"fused_encoder computes in bf16 and needs dtype='bf16', got "
                f"dtype={args.dtype!r}")
        super().__init__(args, device, "a3c-gpu")

        # probe the 42×42 wrapped env for shapes
        from ..envs.a3c_env import create_atari_env
        probe = create_atari_env(args.env_id, seed=args.seed)
        self.obs_shape = probe.observation_space.shape     # (1, 42, 42)
        self.num_actions = probe.action_space.n
        probe.close()

        E = args.envs_per_actor
        self.slots_per_batch = args.slots_per_batch
        self.local_slots = args.num_actors + 2 * self.slots_per_batch + 2
        # CPU phase (precedes any HIP initialization)
        torch.manual_seed(args.seed + self.rank)
        self.actor_model = A3CAtariNet(self.obs_shape[0], self.num_actions)
        self.actor_model.eval()
        self.shared_flat = FlatParams(self.actor_model, device="cpu",
                                      share=True)
        self.store = RolloutStore(
            self.local_slots, args.rollout_steps, E, self.obs_shape,
            self.num_actions, lstm_layers=1, lstm_hidden=256,
            obs_dtype=torch.float32)

    # -- lifecycle ---------------------------------------------------------
    def _actor_process(self, i: int):
        args = self.args
        env_spec = {"env_id": args.env_id, "envs_per_actor": args.envs_per_actor,
                    "seed": args.seed + 7919 * self.rank, "a3c_wrap": True}
        return (actor_loop, self._actor_args(i, env_spec),
                dict(policy_factory=partial(a3c_local_policy,
                                            self.actor_model),
                     seed=args.seed, episode_queue=self.episode_q),
                f"a3c-actor-{self.rank}-{i}")

    def setup_learner(self) -> None:
        args = self.args
        self.model = A3CAtariNet(
            self.obs_shape[0], self.num_actions,
            fused_encoder=args.fused_encoder).to(self.device)
        self.model.load_state_dict(self.actor_model.state_dict())
        self.flat = FlatParams(self.model, device=self.device)
        from ..parallel.dist import broadcast_flat, get_world_size as _ws
        if _ws() > 1:  # dynamic: dist may init after __init__
            broadcast_flat(self.flat.flat, src=0)  # identical init (DP)
        self.optimizer = FusedAdam(self.flat.flat, lr=args.learning_rate)
        self.gatherer = BatchGatherer(self.store, self.device,
                                      args.slots_per_batch)
        if self.device.type == "cuda":
            torch.backends.cudnn.benchmark = True
            self._pin_host_memory()
        self._publish()
        self.autocast_dtype = (torch.bfloat16 if args.dtype == "bf16" and
                               self.device.type == "cuda" else None)

    @torch.no_grad()
    def _publish(self) -> None:
        self.shared_flat.flat.copy_(self.flat.flat)

    # -- core step ---------------------------------------------------------
    def learn_step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        args = self.args
        self.model.train()
        self.flat.flat_grad.zero_()
        obs = batch["obs"].float()                       # [T+1, B, 1,42,42]
        notdone = (~batch["done"]).float()               # [T+1, B]
        cs = batch["core_state"]                         # [2, L, B, H]
        state = (cs[0], cs[1])
        if self.autocast_dtype is not None:
            with torch.autocast(device_type="cuda", dtype=self.autocast_dtype):
                logits, values, _ = self.model.unroll(obs, notdone, state)
        else:
            logits, values, _ = self.model.unroll(obs, notdone, state)
        logits = logits.float()
        values = values.float()
        T = args.rollout_steps
        rewards = torch.clamp(batch["reward"][1:], -1, 1)  # r for action[t]
        discounts = notdone[1:] * args.gamma
        total, comps, _ = a2c_loss(
            logits[:-1], values[:-1], values[-1].detach(),
            batch["action"][:-1], rewards, discounts, lam=args.gae_lambda,
            value_coef=args.value_loss_coef, entropy_coef=args.entropy_coef)
        self.timings.time("forward")
        total.backward()
        self.timings.time("backward")
        all_reduce_flat(self.flat.flat_grad, average=True)  # no-op
        # when torch.distributed is not initialized
        if args.max_grad_norm > 0:
            clip_grad_norm_(self.flat.flat_grad, args.max_grad_norm)
        self.optimizer.step(self.flat.flat_grad)
        self.timings.time("optimize")
        self._publish()
        self.timings.time("publish")
        self.gatherer.mark_consumed()
        self.learn_iters += 1
        self.global_step += T * batch["action"].shape[1]
        return {"total_loss": total.detach(), "pg_loss": comps[0],
                "value_loss": comps[1], "entropy": comps[2]}

    def train_iteration(self) -> Dict[str, torch.Tensor]:
        batch = self.next_batch()
        return self.learn_step(batch)

    def train(self) -> None:
        args = self.args
        self.start_actors()
        self.setup_learner()
        last_log, last_step = time.time(), 0
        try:
            while self.global_step < args.total_steps:
                stats = self.train_iteration()
                now = time.time()
                if self.rank == 0 and now - last_log > 5.0:
                    sps = (self.global_step - last_step) / (now - last_log)
                    last_log, last_step = now, self.global_step
                    self.log.info(f"step {self.global_step} SPS {sps:,.0f} "
                                  f"loss {float(stats['total_loss']):.3f}")
        finally:
            if self.rank == 0 and not args.disable_checkpoint:
                save_checkpoint(os.path.join(args.output_dir, "model.tar"),
                                model=self.model, optimizer=None,
                                hparam=vars(args),
                                extra={"global_step": self.global_step})
            self.shutdown()
