#!/usr/bin/env python3
"""Flagship benchmark: IMPALA on synthetic Atari (BASELINE.json config 3).

Measures env-steps/sec (whole job, all ranks): one timed "step" is one
learner iteration consuming rollout_length × batch_size env steps pulled
from live actor processes (the reference's SPS definition,
impala_atari.py:391).  The full pipeline runs during timing: CPU actor
processes stepping vectorized synthetic envs, policy inference, shared-
memory rollout transport, H2D side-stream copies, learner fwd/bwd with the
fused HIP V-trace/loss kernels, RCCL flat-grad all-reduce, fused RMSProp,
and weight publication back to the actors.

Single node, one rank per GPU (launched by torch.distributed.run for
N > 1); weak scaling — per-rank actor count and batch are fixed.

8-rank resource budget (validated CPU-side; driver runs the real SCALE):
- /dev/shm: each rank's rollout store is num_buffers × slot_bytes, slot ≈
  (T+1)·E·(4·84·84 u8 + A·4 logits + 28 scalars) ≈ 292 MB at T=80, E=128.
  Defaults give ~30 slots ≈ 8.8 GB/rank → ~70 GB at 8 ranks.  main()
  checks statvfs(/dev/shm) and halves envs_per_actor (keeping batch_size
  divisible) until the projected total fits in 80% of free shm.
- cores: per-rank actor count is sized from cpu_count()/world minus 2
  (learner + inference worker): 256 cores / 8 ranks → 24 actors each,
  ~208 processes total.
- MIOpen: MIOPEN_FIND_MODE=1 plus a shared MIOPEN_USER_DB_PATH so 8
  concurrent learners share one find cache instead of 8 find storms.
"""

from __future__ import annotations

import argparse
import json
import os
import time

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rollout-length", type=int, default=80)
    p.add_argument("--use-graph", type=int, default=1,
                   help="hipGraph-capture the learner step (measured 539k "
                        "vs 340k eager at the default config)")
    p.add_argument("--double-buffer", type=int, default=0,
                   help="two env groups per actor (SEED latency hiding)")
    p.add_argument("--batch-size", type=int, default=256)
    p.add_argument("--envs-per-actor", type=int, default=256)
    p.add_argument("--num-actors", type=int, default=0,
                   help="actor procs per rank (0 = auto from cpu count)")
    p.add_argument("--use-lstm", type=int, default=1)
    p.add_argument("--dtype", type=str, default="bf16",
                   choices=["bf16", "fp32"])
    p.add_argument("--device", type=str, default="auto")
    p.add_argument("--inference", type=str, default="auto",
                   choices=["auto", "cpu", "gpu"])
    p.add_argument("--inference-worker", type=str, default="process",
                   choices=["thread", "process"])
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="write what the last timed step computed to "
                        "DIR/<name>.npy (see _fixed_batch / _dump_outputs)")
    p.add_argument("--full", action="store_true",
                   help="also report everything beyond the headline figure: "
                        "setup-phase and per-section learner timings and "
                        "actor production (stderr)")
    args = p.parse_args()
    if args.dump_outputs is not None and args.steps < 1:
        p.error("--dump-outputs needs at least one timed step")
    return args


# --dump-outputs ------------------------------------------------------------
# The timed path is fed by live actor processes, so its batches depend on
# process scheduling and differ from run to run.  To make two builds
# comparable output for output, the LAST timed step of a --dump-outputs run
# still pulls its batch through the whole pipeline, but then learns from a
# fixed seeded batch of the same shapes, starting from the seeded initial
# weights and a zeroed optimizer state.  What that step hands its caller
# (the four loss scalars, the clipped flat gradient and the updated flat
# weights) is written out.

_DUMP_SEED = 20240229
_DUMP_MAX_ELEMS = 7 * 1024 * 1024  # per array; two float32 arrays < 64 MB


def _fixed_batch(like, num_actions):
    """A seeded batch with the keys, shapes, dtypes and device of ``like``."""
    g = torch.Generator(device="cpu").manual_seed(_DUMP_SEED)
    out = {}
    for name in sorted(like):
        ref = like[name]
        if ref.dtype == torch.uint8:
            t = torch.randint(0, 256, ref.shape, dtype=torch.uint8,
                              generator=g)
        elif ref.dtype == torch.bool:
            t = torch.rand(ref.shape, generator=g) < 0.02
        elif ref.dtype.is_floating_point:
            t = torch.randn(ref.shape, generator=g).to(ref.dtype)
            if name == "core_state":
                t.mul_(0.1)
        else:  # action ids
            t = torch.randint(0, num_actions, ref.shape, dtype=ref.dtype,
                              generator=g)
        out[name] = t.to(ref.device)
    return out


def _dump_outputs(path, stats, trainer):
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {k: v.detach().float().reshape(-1).cpu().numpy()
              for k, v in stats.items()}
    arrays["flat_grad"] = trainer.flat.flat_grad.detach().float().cpu().numpy()
    arrays["flat_params"] = trainer.flat.flat.detach().float().cpu().numpy()
    rng = np.random.default_rng(_DUMP_SEED)
    for name, a in arrays.items():
        if a.size > _DUMP_MAX_ELEMS:  # fixed seeded sample of a large output
            idx = np.sort(rng.choice(a.size, _DUMP_MAX_ELEMS, replace=False))
            a = a[idx]
        np.save(os.path.join(path, f"{name}.npy"),
                np.ascontiguousarray(a, dtype=np.float32))


_TUNED_DB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                             "tuning", "miopen")


def _install_tuned_perf_db(user_db_dir):
    """Merge the repository's tuned MIOpen perf-db records (tuning/miopen/,
    the solver parameters MIOpen's own search settled on for the default
    learner shapes) into the user db.  Without them every run in a fresh
    user db repeats that search (~45 s) before its first step.  Files are
    named by GPU arch and MIOpen version, so another version ignores them
    and tunes as before; records already in the user db are kept."""
    if not user_db_dir or not os.path.isdir(_TUNED_DB_DIR):
        return
    for fname in sorted(os.listdir(_TUNED_DB_DIR)):
        if not fname.endswith(".udb.txt"):
            continue
        dst = os.path.join(user_db_dir, fname)
        try:
            with open(os.path.join(_TUNED_DB_DIR, fname)) as f:
                ours = [ln for ln in f.read().splitlines() if "=" in ln]
            have = []
            if os.path.exists(dst):
                with open(dst) as f:
                    have = [ln for ln in f.read().splitlines() if ln]
            keys = {ln.split("=", 1)[0] for ln in have}
            new = [ln for ln in ours if ln.split("=", 1)[0] not in keys]
            if not new:
                continue
            tmp = f"{dst}.{os.getpid()}.tmp"
            with open(tmp, "w") as f:
                f.write("\n".join(have + new) + "\n")
            os.replace(tmp, dst)  # atomic: ranks may race here
        except OSError:
            pass  # read-only db dir: MIOpen tunes by itself as before


def main():
    # Consistent MIOpen behavior across boxes: full find (the hybrid default
    # has been observed to settle on naive bf16 conv kernels on fresh boxes),
    # and ONE shared find-cache db across all ranks of a node.
    os.environ.setdefault("MIOPEN_FIND_MODE", "1")
    if "MIOPEN_USER_DB_PATH" not in os.environ:
        # per user, next to MIOpen's own kernel cache: both then persist
        # together from one run to the next
        for db in (os.path.join(os.path.expanduser("~"), ".cache",
                                "scalerl_amd", "miopen"),
                   "/tmp/scalerl_miopen"):
            try:
                os.makedirs(db, exist_ok=True)
            except OSError:
                continue
            if os.access(db, os.W_OK):
                os.environ["MIOPEN_USER_DB_PATH"] = db
                break
    else:
        os.makedirs(os.environ["MIOPEN_USER_DB_PATH"], exist_ok=True)
    _install_tuned_perf_db(os.environ.get("MIOPEN_USER_DB_PATH"))
    args = parse_args()
    if args.dtype == "bf16":
        # The find re-times every applicable solver in every process.  At
        # the bf16 encoder shapes the im2col-GEMM and naive direct solvers
        # run 200-1000x slower than the implicit-GEMM winners (500-1400 ms
        # vs 0.4-2.2 ms per call) and made up ~95 of the ~100 s a find
        # took; they never win, so leaving them out changes no choice.
        for var in ("MIOPEN_DEBUG_CONV_GEMM",
                    "MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD",
                    "MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_BWD",
                    "MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_WRW"):
            os.environ.setdefault(var, "0")
    marks = [("start", time.perf_counter())]  # setup phases (--full report)

    def mark(name):
        marks.append((name, time.perf_counter()))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    use_cuda = torch.cuda.is_available() and args.device in ("auto", "cuda")
    device = f"cuda:{local_rank}" if use_cuda else "cpu"

    from scalerl_amd.config import ImpalaArguments
    from scalerl_amd.runtime.impala import ImpalaTrainer

    inference = args.inference
    if inference == "auto":
        inference = "gpu" if use_cuda else "cpu"

    if args.num_actors <= 0:
        ncpu = os.cpu_count() or 8
        # per-rank core budget: actors + learner + inference worker
        avail = max(2, ncpu // max(1, world) - 2)
        if inference == "gpu":
            # actors are pure env-steppers; a handful saturate the
            # inference worker
            args.num_actors = min(24, avail)
        else:
            # one CPU-inference actor ≈ a few hundred steps/s
            args.num_actors = min(64, avail)

    # /dev/shm budget: shrink envs_per_actor until all ranks' rollout
    # stores fit in 80% of the free space (see module docstring).
    try:
        st = os.statvfs("/dev/shm")
        shm_free = st.f_bavail * st.f_frsize
    except OSError:
        shm_free = None
    if shm_free is not None:
        def store_bytes(E):
            slots = args.num_actors + 2 * max(args.batch_size // E, 1) + 2
            slot = (args.rollout_length + 1) * E * (4 * 84 * 84 + 6 * 4 + 28)
            return slots * slot
        while (args.num_actors > 8
               and world * store_bytes(args.envs_per_actor) > 0.8 * shm_free):
            args.num_actors -= 4
            if rank == 0:
                print(f"[bench] /dev/shm pressure: num_actors -> "
                      f"{args.num_actors}", flush=True)
        while (args.envs_per_actor > 16
               and world * store_bytes(args.envs_per_actor) > 0.8 * shm_free):
            args.envs_per_actor //= 2
            if rank == 0:
                print(f"[bench] /dev/shm pressure: envs_per_actor -> "
                      f"{args.envs_per_actor}", flush=True)

    cfg = ImpalaArguments(
        rollout_length=args.rollout_length, batch_size=args.batch_size,
        envs_per_actor=args.envs_per_actor, num_actors=args.num_actors,
        use_lstm=bool(args.use_lstm), device=device, dtype=args.dtype,
        use_graph=bool(args.use_graph),
        actor_double_buffer=bool(args.double_buffer),
        inference_worker=args.inference_worker,
        inference=inference, seed=1234 + rank,
        total_steps=1 << 60, disable_checkpoint=True,
        output_dir="/tmp/scalerl_bench")

    mark("imports+args")
    trainer = ImpalaTrainer(cfg, device=device)
    trainer.rank = rank
    mark("trainer init (rollout store)")
    if trainer._mp_ctx == "fork":
        # pure-CPU path: fork actors BEFORE any device init
        trainer.start_actors()
    if world > 1:
        from scalerl_amd.parallel.dist import init_distributed
        init_distributed("nccl" if use_cuda else "gloo")
    # GPU path (spawn ctx): device init + hipGraph capture FIRST, then
    # spawn the inference worker + actors (capture must precede any other
    # process submitting on this GPU — see ImpalaTrainer.setup_learner)
    trainer.setup_learner()
    mark("learner setup (pin, graph capture)")
    trainer.start_actors()
    mark("start actors")

    def barrier_sync():
        if world > 1:
            torch.distributed.barrier()
        if use_cuda:
            torch.cuda.synchronize()

    dump = args.dump_outputs is not None
    if dump:
        init_flat = trainer.flat.flat.detach().clone()

    for _ in range(args.warmup):
        trainer.train_iteration()
    trainer.reset_timings()  # drop first-iteration autotune/compile spikes
    mark("warmup")

    # with --dump-outputs the last timed step is run apart from the others,
    # with the clock stopped while its fixed inputs are put in place
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps - 1 if dump else args.steps):
        trainer.train_iteration()
    barrier_sync()
    elapsed = time.perf_counter() - t0

    if dump:
        t0 = time.perf_counter()
        trainer.timings.reset()
        live = trainer.next_batch()
        barrier_sync()
        elapsed += time.perf_counter() - t0

        fixed = _fixed_batch(live, trainer.num_actions)
        with torch.no_grad():
            trainer.flat.flat.copy_(init_flat)
            trainer.optimizer.square_avg.zero_()
            if trainer.optimizer.momentum_buf is not None:
                trainer.optimizer.momentum_buf.zero_()

        barrier_sync()
        t0 = time.perf_counter()
        trainer.timings.reset()
        stats = trainer.learn_step(fixed)
        barrier_sync()
        elapsed += time.perf_counter() - t0
        if rank == 0:
            _dump_outputs(args.dump_outputs, stats, trainer)
    mark("timed steps")

    # max over ranks (the slowest rank defines whole-job time)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if use_cuda else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    steps_per_iter = args.rollout_length * args.batch_size
    total_env_steps = args.steps * steps_per_iter * world
    value = total_env_steps / elapsed

    if rank == 0:
        if args.full:
            import sys
            produced = trainer.step_counter.value
            phases = "\n".join(
                f"  {name}: {t1 - t0:.2f} s"
                for (_, t0), (name, t1) in zip(marks, marks[1:]))
            print(f"[bench] run phases:\n{phases}\n"
                  f"[bench] learner timings (s/iter means):\n"
                  f"{trainer.timings.summary('  ')}\n"
                  f"[bench] actor production during run: {produced} "
                  f"env-steps ({produced / elapsed:,.0f}/s incl. warmup "
                  f"overlap)", file=sys.stderr)
        result = {
            "metric": "env_steps_per_sec",
            "value": round(value, 1),
            "unit": "env-steps/s",
            "n_gpus": world if use_cuda else 0,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1000.0 * elapsed / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype if use_cuda else "fp32",
            "data": "synthetic 84x84x4 frames, random-init weights",
            "config": {
                "model": "IMPALA AtariNet (3conv+FC512+2xLSTM519)",
                "algo": "impala-vtrace",
                "rollout_length": args.rollout_length,
                "global_batch": args.batch_size * world,
                "seq_len": args.rollout_length,
                "envs_per_actor": args.envs_per_actor,
                "actors_per_rank": args.num_actors,
                "inference": trainer.inference,  # actual placement used
                "parallelism": f"dp{world}",
            },
        }
        print(json.dumps(result), flush=True)

    trainer.shutdown()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
