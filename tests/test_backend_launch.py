"""The one ctypes boundary (ops/_backend.py): the signature table against the
C prototypes, and what ``launch`` refuses before it touches the library."""

import glob
import os
import re

import pytest
import torch

from scalerl_amd.ops import _backend
from scalerl_amd.ops._backend import launch

_C_POINTER_DTYPE = {"float": "f32", "long": "i64", "int": "i32",
                    "unsigned int": "i32"}


def _c_prototypes():
    """name -> list of parameter strings of every ``extern "C" int NAME(...)``
    definition in csrc/*.hip, comments stripped."""
    protos = {}
    for path in glob.glob(os.path.join(_backend._CSRC, "*.hip")):
        src = open(path).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        src = re.sub(r"//[^\n]*", "", src)
        for m in re.finditer(r'extern\s+"C"\s+int\s+(\w+)\s*\(([^)]*)\)\s*\{',
                             src):
            assert m.group(1) not in protos, m.group(1)
            protos[m.group(1)] = [" ".join(p.split())
                                  for p in m.group(2).split(",")]
    return protos


def _kind(param: str) -> str:
    if "*" in param:
        return "pointer"
    for word in ("hipStream_t", "long", "int", "float"):
        if re.match(rf"(const )?{word}\b", param):
            return word
    raise AssertionError(f"unmapped C parameter {param!r}")


def test_table_matches_c_prototypes():
    protos = _c_prototypes()
    assert set(protos) == set(_backend._SIGNATURES)
    assert len(protos) == 37
    for name, params in protos.items():
        assert _kind(params[-1]) == "hipStream_t", name
        words = _backend._SIGNATURES[name].split()
        assert len(words) == len(params) - 1, name
        for i, (word, param) in enumerate(zip(words, params)):
            where = f"{name} argument {i}: table {word!r}, C {param!r}"
            kind = _kind(param)
            if kind != "pointer":
                assert word == kind, where
                continue
            dtype = word.rstrip("?")
            assert dtype in _backend._DTYPES, where
            pointee = re.sub(r"\bconst\b", "", param.split("*")[0]).strip()
            if pointee != "void":
                assert _C_POINTER_DTYPE[pointee] == dtype, where


# fused_polyak(dst f32, src f32, n long, tau float): the smallest signature
def test_wrong_dtype_raises():
    with pytest.raises(TypeError, match=r"fused_polyak, argument 1 .*float32"):
        launch("fused_polyak", torch.zeros(4), torch.zeros(4).double(), 4, 0.5)


def test_non_contiguous_raises():
    t = torch.zeros(4, 4)
    with pytest.raises(ValueError, match=r"fused_polyak, argument 0 .*contig"):
        launch("fused_polyak", t[:, ::2], torch.zeros(8), 8, 0.5)


def test_none_in_non_nullable_slot_raises():
    with pytest.raises(TypeError, match=r"fused_polyak, argument 1 .*None"):
        launch("fused_polyak", torch.zeros(4), None, 4, 0.5)


def test_non_tensor_in_pointer_slot_raises():
    with pytest.raises(TypeError, match=r"fused_polyak, argument 0 .*int"):
        launch("fused_polyak", 1234, torch.zeros(4), 4, 0.5)


def test_wrong_argument_count_raises():
    with pytest.raises(TypeError, match=r"fused_polyak takes 4 arguments"):
        launch("fused_polyak", torch.zeros(4), torch.zeros(4), 4)


def test_unknown_name_raises():
    with pytest.raises(ValueError, match="no_such_kernel"):
        launch("no_such_kernel", torch.zeros(4))


def test_cpu_tensors_raise_the_device_error():
    with pytest.raises(ValueError, match=r"fused_polyak, argument 0 .*GPU"):
        launch("fused_polyak", torch.zeros(4), torch.zeros(4), 4, 0.5)


def test_none_in_nullable_slot_passes_up_to_the_device_check():
    # fused_rmsprop's momentum buffer (argument 3) may be null: the first
    # complaint is about the device of argument 0
    p = torch.zeros(4)
    with pytest.raises(ValueError, match=r"fused_rmsprop, argument 0 .*GPU"):
        launch("fused_rmsprop", p, p.clone(), p.clone(), None, 4, 1e-3, 0.99,
               0.01, 0.0, 0.0)


@pytest.mark.gpu
def test_rmsprop_refuses_non_contiguous_grad_and_leaves_param():
    from scalerl_amd.ops import FusedRMSprop
    param = torch.arange(64, dtype=torch.float32, device="cuda")
    before = param.clone()
    grad = torch.ones(128, device="cuda")[::2]
    assert grad.numel() == 64 and not grad.is_contiguous()
    with pytest.raises(ValueError, match="contig"):
        FusedRMSprop(param, lr=0.1).step(grad)
    assert torch.equal(param, before)


@pytest.mark.gpu
def test_launch_with_inline_temporary_of_non_contiguous_frames():
    from scalerl_amd.ops import frame_to_bf16
    g = torch.Generator().manual_seed(0)
    big = torch.randint(0, 256, (2, 4, 84, 168), dtype=torch.uint8,
                        generator=g).cuda()
    x = big[..., ::2]
    assert tuple(x.shape) == (2, 4, 84, 84) and not x.is_contiguous()
    want = (x.float() / 255).to(torch.bfloat16)
    assert torch.equal(frame_to_bf16(x).view(torch.int16),
                       want.view(torch.int16))
