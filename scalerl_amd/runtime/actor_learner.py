"""The actor-learner lifecycle that IMPALA, Ape-X and A3C-GPU share.

Actor processes fill shared rollout slots (parallel/rollout.py) handed out
on ``free_q`` and announce them on ``full_q``; the learner consumes them and
recycles the ids.  This base owns the part that is the same for every such
trainer — device and start-method choice, the queues and counters, actor
spawning, the watchdogged dequeue, the prefetch pipeline over a
``BatchGatherer``, host-memory pinning and shutdown.  What a step computes,
and how weights are published, stays in the trainers.

Construction order, for every subclass: the CPU phase (shared actor model,
rollout store, this constructor) precedes any HIP initialization, and under
the spawn context ``setup_learner`` (with any graph capture) precedes
``start_actors``.
"""

from __future__ import annotations

import os
import queue
import time
from typing import Dict, List, Optional

import torch
import torch.multiprocessing as mp

from ..parallel import get_rank, get_world_size
from ..parallel.rollout import PinRegistry
from ..utils import Timings, get_logger


class ActorLearnerTrainer:
    """Subclasses set ``store``, ``shared_flat`` and ``local_slots`` in their
    constructor, ``gatherer`` and ``slots_per_batch`` if they use
    :meth:`next_batch`, and implement :meth:`_actor_process`."""

    _pills_per_actor = 1  # free-slot requests an actor blocks on per round

    def __init__(self, args, device: Optional[str], log_name: str,
                 episode_q: bool = True):
        self.args = args
        self.rank = get_rank()
        self.world_size = get_world_size()
        self.log = get_logger(log_name)
        if device is None:
            device = ("cuda" if torch.cuda.is_available() else "cpu") \
                if args.device == "auto" else args.device
        self.device = torch.device(device)

        # spawn, not fork, whenever the GPU is involved: the learner (and
        # inference worker) initialize the HIP runtime, which does not
        # survive fork on ROCm.  Shared-memory tensors travel to spawned
        # children as shm handles.  Pure-CPU runs keep fork (fast startup).
        self._mp_ctx = ("fork" if (self.device.type == "cpu"
                                   and not torch.cuda.is_initialized()
                                   and not os.environ.get(
                                       "SCALERL_FORCE_SPAWN"))
                        else "spawn")
        ctx = mp.get_context(self._mp_ctx)
        self.free_q = ctx.SimpleQueue()
        self.full_q = ctx.Queue()  # timeout-capable: the learner watchdogs it
        self.stop_event = ctx.Event()
        self.step_counter = ctx.Value("l", 0)
        self.episode_q = ctx.Queue(maxsize=256) if episode_q else None
        self.actors: List[mp.Process] = []
        self.inference_proc = None  # set by trainers that run a GPU worker
        self._started = False
        self._pins: Optional[PinRegistry] = None
        self._pending = None  # in-flight prefetched batch token
        self.global_step = 0
        self.learn_iters = 0
        self.timings = Timings()

    # -- actors --------------------------------------------------------------
    def _actor_process(self, i: int):
        """``(target, args, kwargs, name)`` of actor ``i``'s process; all of
        it must pickle (spawn context)."""
        raise NotImplementedError

    def _actor_args(self, i: int, env_spec: dict):
        """The leading arguments every actor main takes."""
        return (i, env_spec, self.store, self.free_q, self.full_q,
                self.stop_event, self.step_counter)

    def start_actors(self) -> None:
        if self._started:
            return
        ctx = mp.get_context(self._mp_ctx)
        for i in range(self.args.num_actors):
            target, args, kwargs, name = self._actor_process(i)
            p = ctx.Process(target=target, args=args, kwargs=kwargs,
                            daemon=True, name=name)
            p.start()
            self.actors.append(p)
        for s in range(self.local_slots):
            self.free_q.put(s)
        self._started = True

    def _pin_host_memory(self) -> None:
        """hipHostRegister the rollout store and the shared weights so the
        copies between them and the device are async DMA (CUDA only)."""
        if self.device.type != "cuda":
            return
        self._pins = PinRegistry()
        pinned = self._pins.pin_store(self.store)
        pinned += self._pins.pin(self.shared_flat.flat)
        self.log.info(f"pinned {pinned/1e6:.1f} MB (rollout store + "
                      f"shared weights)")

    # -- dequeue + prefetch --------------------------------------------------
    def _get_full_slot(self, timeout_s: float = 30.0, max_wait_s: float = 600.0):
        """full_q.get with a liveness watchdog: a dead actor or inference
        worker turns a silent eternal hang into a fast, explicit error."""
        waited = 0.0
        while True:
            try:
                return self.full_q.get(timeout=timeout_s)
            except queue.Empty:
                waited += timeout_s
                dead = [p.name for p in self.actors if not p.is_alive()]
                if dead:
                    raise RuntimeError(f"actor process(es) died: {dead}")
                if (self.inference_proc is not None
                        and not self.inference_proc.is_alive()):
                    raise RuntimeError("GPU inference worker died")
                if waited >= max_wait_s:
                    raise RuntimeError(
                        f"no rollout slot arrived in {waited:.0f}s "
                        f"(actors alive but not producing)")

    def _recycle_slot(self, slot: int) -> None:
        self.free_q.put(slot)

    def _start_prefetch(self):
        slot_ids = [self._get_full_slot()
                    for _ in range(self.slots_per_batch)]
        self.timings.time("dequeue")
        token = self.gatherer.start(slot_ids)
        self.timings.time("gather_start")
        return (token, slot_ids)

    def next_batch(self) -> Dict[str, torch.Tensor]:
        """Finish the pending prefetch (or do a cold gather) and kick off
        the next one — batch N+1's H2D copies overlap batch N's compute."""
        if self._pending is None:
            self._pending = self._start_prefetch()
        token, slot_ids = self._pending
        batch = self.gatherer.finish(token)
        self.timings.time("gather_wait")
        for s in slot_ids:
            self._recycle_slot(s)
        self._pending = self._start_prefetch()
        return batch

    def reset_timings(self) -> None:
        self.timings = Timings()

    # -- shutdown ------------------------------------------------------------
    def _before_join(self) -> None:
        """Unblock actors that wait on something other than free_q."""

    def _after_join(self) -> None:
        """Stop the helpers that outlive the actors."""

    def shutdown(self) -> None:
        self.stop_event.set()
        for _ in range(len(self.actors) * self._pills_per_actor):
            self.free_q.put(None)  # poison pills (impala_atari.py:480)
        self._before_join()
        # one shared grace period: an actor that is mid-rollout blocks on its
        # inference semaphore once the worker is gone and never sees its
        # pill, so a per-actor timeout would add up over all of them
        deadline = time.time() + 2.0
        for p in self.actors:
            p.join(timeout=max(0.0, deadline - time.time()))
            if p.is_alive():
                p.terminate()
        self.actors.clear()
        self._after_join()
        if self._pins is not None:
            if self.device.type == "cuda":
                torch.cuda.synchronize()
            self._pins.unpin_all()
            self._pins = None
