"""HIP kernel backend: in-tree build (hipcc, gfx950 only), ctypes loader and
the one checked launch path.

The kernels are plain HIP (no torch extension ABI): one shared library
``_hip_ops.so`` built from ``csrc/*.hip`` with
``hipcc --offload-arch=gfx950``.  Every entry point is listed once in
``_SIGNATURES``; :func:`launch` validates the tensors against that entry,
passes their raw device pointers and the current torch HIP stream, so kernels
land on the same stream as surrounding torch ops.

Policy (no silent fallbacks): on a CUDA/ROCm device every op REQUIRES the
library — a missing .so raises immediately.  CPU tensors use the pure
PyTorch reference implementations (also the test oracles).
"""

from __future__ import annotations

import ctypes
import os
import subprocess
import sys
from typing import Optional

import torch

_THIS_DIR = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_THIS_DIR, "csrc")
_SO_PATH = os.path.join(_THIS_DIR, "_hip_ops.so")

_LIB: Optional[ctypes.CDLL] = None
_LOAD_ERROR: Optional[str] = None


def hip_sources():
    return sorted(
        os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hip"))


def build(verbose: bool = True, arch: str = "gfx950") -> str:
    """Compile csrc/*.hip → _hip_ops.so in-tree.  Idempotent (mtime check)."""
    srcs = hip_sources()
    hdrs = sorted(
        os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h"))
    if os.path.exists(_SO_PATH):
        newest = max(os.path.getmtime(p) for p in srcs + hdrs)
        if os.path.getmtime(_SO_PATH) >= newest:
            return _SO_PATH
    hipcc = os.environ.get("HIPCC", "hipcc")
    cmd = [hipcc, f"--offload-arch={arch}", "-O3", "-std=c++17", "-shared",
           "-fPIC", "-lrocblas", "-o", _SO_PATH] + srcs
    if verbose:
        print("[scalerl_amd.ops] building:", " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return _SO_PATH


# Every exported ``extern "C" int NAME(..., hipStream_t)`` of csrc/*.hip, one
# word per argument in C order; the trailing stream is implicit.  Pointer
# kinds name the tensor dtype the kernel reads or writes (f32 i64 i32 bf16
# u8), with ``?`` where the kernel accepts a null pointer; ``long``, ``int``
# and ``float`` are scalars.  tests/test_backend_launch.py holds this table
# against the C prototypes.
_CONV_FWD = "bf16 bf16 f32? bf16 long int"
_CONV1_FWD_U8 = "u8 bf16 f32? bf16 long int"
_CONV_WGRAD = "bf16 bf16 f32 long long"
_CONV_WGRAD_V3 = "bf16 bf16 f32 long"
_CONV_DGRAD = "bf16 bf16 bf16 long"
_SIGNATURES = {
    "impala_fused_loss": "f32 f32 i64 f32 f32 f32 f32 float float float float"
                         " float long long long f32 f32 f32 f32?",
    "vtrace_from_log_rhos": "f32 f32 f32 f32 f32 float float float long long"
                            " f32 f32",
    "gae_scan": "f32 f32 f32 f32 float long long f32 f32",
    "discounted_returns": "f32 f32 f32? long long f32",
    "nstep_fold": "f32 f32 float long long long f32 f32 i32",
    "fused_rmsprop": "f32 f32 f32 f32? long float float float float float",
    "fused_adam": "f32 f32 f32 f32 long float float float float float long",
    "fused_polyak": "f32 f32 long float",
    "grad_clip_by_norm": "f32 long f32 float",
    "fused_td_loss": "f32 f32? f32 i64 f32 f32 f32? f32? f32? float long long"
                     " long int float long float float f32 f32 f32",
    "ppo_fused_loss": "f32 i64 f32 f32 f32 f32 float float float long long"
                      " f32 f32 f32",
    "per_update": "f32 long i64 f32 long",
    "per_sample": "f32 long long f32 long i64 f32",
    "per_leaf_min": "f32 long long i32",
    "lstm_mask_rows": "f32 f32 f32 f32 f32 long long",
    "lstm_cell_fwd": "f32 f32 f32 f32 f32? f32? f32? long long",
    "lstm_cell_bwd": "f32 f32 f32 f32 f32 f32? f32 f32 f32 long long",
    "masked_lstm_seq_fwd": "f32 f32 f32 f32 f32 f32 f32 f32 f32 long long long",
    "masked_lstm_seq_bwd": "f32 f32 f32 f32 f32 f32 f32 f32 f32 f32 long long"
                           " long",
    "frame_cast_u8_bf16": "u8 bf16 long",
    "mfma_selftest": "f32 f32 f32",
    "atari_encoder_fwd": "u8 bf16 f32 bf16 f32 bf16 f32 bf16? bf16? bf16 long",
    "atari_conv1_fwd_u8": _CONV1_FWD_U8,
    "atari_conv1_fwd_bf16": _CONV_FWD,
    "atari_conv2_fwd": _CONV_FWD,
    "atari_conv3_fwd": _CONV_FWD,
    "atari_conv2_fwd_v3": _CONV_FWD,
    "atari_conv3_fwd_v3": _CONV_FWD,
    "atari_conv1_wgrad_u8": "u8 bf16 f32 long long",
    "atari_conv2_wgrad": _CONV_WGRAD,
    "atari_conv3_wgrad": _CONV_WGRAD,
    "atari_conv1_wgrad_v3": "u8 bf16 f32 long",
    "atari_conv2_wgrad_v3": _CONV_WGRAD_V3,
    "atari_conv3_wgrad_v3": _CONV_WGRAD_V3,
    "atari_conv2_dgrad": _CONV_DGRAD,
    "atari_conv3_dgrad": _CONV_DGRAD,
    "atari_conv2_dgrad_v3": _CONV_DGRAD,
}

_DTYPES = {"f32": torch.float32, "i64": torch.int64, "i32": torch.int32,
           "bf16": torch.bfloat16, "u8": torch.uint8}
_SCALARS = {"long": ctypes.c_long, "int": ctypes.c_int,
            "float": ctypes.c_float}


class _Spec:
    """One entry point, precomputed for :func:`launch`: per argument the
    tensor dtype (None for a scalar) and whether null is accepted."""
    __slots__ = ("words", "dtypes", "nullable", "argtypes", "fn")

    def __init__(self, words):
        self.words = words
        self.dtypes = tuple(_DTYPES.get(w.rstrip("?")) for w in words)
        self.nullable = tuple(w.endswith("?") for w in words)
        self.argtypes = [_SCALARS.get(w, ctypes.c_void_p) for w in words]
        self.argtypes.append(ctypes.c_void_p)  # the stream
        self.fn = None


_SPECS = {name: _Spec(sig.split()) for name, sig in _SIGNATURES.items()}


def lib() -> ctypes.CDLL:
    """The loaded kernel library.  Raises if unavailable (no fallback)."""
    global _LIB, _LOAD_ERROR
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_SO_PATH):
        raise RuntimeError(
            f"scalerl_amd HIP kernel library not found at {_SO_PATH}. "
            f"Build it with `python -c 'from scalerl_amd.ops import _backend; "
            f"_backend.build()'` or `python setup.py build_ext --inplace`. "
            f"GPU execution without the native kernels is not supported.")
    try:
        loaded = ctypes.CDLL(_SO_PATH)
    except OSError as e:
        _LOAD_ERROR = str(e)
        raise RuntimeError(f"failed to load {_SO_PATH}: {e}") from e
    for name, spec in _SPECS.items():
        fn = getattr(loaded, name)
        fn.argtypes = spec.argtypes
        fn.restype = ctypes.c_int
        spec.fn = fn
    _LIB = loaded
    return _LIB


def available() -> bool:
    return os.path.exists(_SO_PATH)


def _reject(name: str, spec: _Spec, args) -> None:
    """Raise the exception for the first argument of ``args`` that
    ``launch`` cannot pass on.  The slow path: only runs on failure."""
    if len(args) != len(spec.words):
        raise TypeError(f"HIP kernel {name} takes {len(spec.words)} arguments "
                        f"({' '.join(spec.words)}), got {len(args)}")
    tensors = []
    for i, (a, dtype, nullable, word) in enumerate(
            zip(args, spec.dtypes, spec.nullable, spec.words)):
        where = f"HIP kernel {name}, argument {i} ({word})"
        if a is None:
            if nullable:
                continue
            raise TypeError(f"{where}: None given, the kernel takes " +
                            ("a number" if dtype is None
                             else "no null pointer") + " here")
        if dtype is None:
            continue
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{where}: expected a {dtype} tensor, got "
                            f"{type(a).__name__}")
        if a.dtype != dtype:
            raise TypeError(f"{where}: expected dtype {dtype}, got {a.dtype}")
        if not a.is_contiguous():
            raise ValueError(f"{where}: expected a contiguous tensor, got "
                             f"shape {tuple(a.shape)} stride {a.stride()}")
        tensors.append((where, a))
    for where, a in tensors:
        if not a.is_cuda:
            raise ValueError(f"{where}: expected a tensor on the current GPU, "
                             f"got device {a.device}")
    cur = torch.cuda.current_device()
    for where, a in tensors:
        if a.device.index != cur:
            raise ValueError(f"{where}: tensor is on {a.device} but the "
                             f"current device, whose stream the kernel is "
                             f"enqueued on, is cuda:{cur}")
    raise AssertionError(f"HIP kernel {name}: launch rejected valid arguments")


def launch(name: str, *args) -> None:
    """Enqueue entry point ``name`` on the current stream of the current
    device.  ``args`` are its arguments in C order without the stream:
    tensors (or None) for pointers, Python numbers for scalars.

    Every tensor is checked against ``_SIGNATURES`` before the library is
    touched: dtype, ``is_contiguous()``, and that it lives on the current
    CUDA device.  None is accepted only where the kernel takes a null
    pointer.  A mismatch raises TypeError or ValueError naming the kernel,
    the argument position and what was expected; nothing is ever copied or
    cast here, so callers keep their explicit ``.contiguous()``/``.float()``.
    Scalars are converted by ctypes, which raises on a wrong type.  A
    non-zero return code raises RuntimeError.

    Temporaries may be written inline — ``launch("k", x.contiguous(), ...)``:
    the argument tuple holds every tensor until the enqueue has returned,
    and after that the caching allocator's reuse of a freed block on the same
    stream is ordered behind the kernel.  (Taking ``data_ptr()`` of an
    unreferenced temporary at a call site, which frees the block before the
    launch, was the use-after-free that once corrupted the conv dgrad.)

    Host-only work, no allocation, no synchronisation: safe under stream
    capture.  The per-step LSTM driver comes through here about 4*T times
    per iteration, so the success path builds nothing but the pointer list.
    """
    spec = _SPECS.get(name)
    if spec is None:
        raise ValueError(f"unknown HIP kernel {name!r}")
    if len(args) != len(spec.words):
        _reject(name, spec, args)
    try:
        cur = torch.cuda.current_device()
    except (RuntimeError, AssertionError):
        cur = -2  # no usable GPU: every tensor fails the device check
    raw = []
    add = raw.append
    try:
        for a, dtype in zip(args, spec.dtypes):
            if dtype is None or a is None:  # scalar, or null: checked below
                add(a)
            elif (a.dtype is dtype and a.is_contiguous()
                  and a.get_device() == cur):
                add(a.data_ptr())
            else:
                _reject(name, spec, args)
    except AttributeError:  # a non-tensor in a pointer slot
        _reject(name, spec, args)
    if None in raw and any(a is None and not ok
                           for a, ok in zip(args, spec.nullable)):
        _reject(name, spec, args)
    fn = spec.fn
    if fn is None:
        lib()
        fn = spec.fn
    # the raw handle of torch.cuda.current_stream(), without building the
    # Stream object
    ret = fn(*raw, torch._C._cuda_getCurrentRawStream(cur))
    if ret != 0:
        hint = ""
        if ret == -2:
            hint = " (action-space size exceeds kernel MAX_A)"
        elif ret == -3:
            hint = " (rollout length exceeds LDS budget)"
        elif ret == -4:
            hint = " (atom count outside the C51 kernel's 2..1024)"
        raise RuntimeError(
            f"HIP kernel {name} failed with code {ret}{hint}; "
            f"device={torch.cuda.get_device_name()}")
