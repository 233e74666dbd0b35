"""Fused Atari encoder forward (ops/csrc/encoder_fwd.hip) against torch.

All tests need the GPU.  Oracles run in fp32 on the CPU so that they do not
depend on any GPU convolution library.
"""

import pytest
import torch
import torch.nn.functional as F

from scalerl_amd.models import AtariNet
from scalerl_amd.models import atari as atari_mod
from scalerl_amd.ops import frame_cast
from scalerl_amd.ops.encoder import atari_encoder_fwd, fused_encoder

pytestmark = pytest.mark.gpu

_W_SHAPES = ((32, 4, 8, 8), (64, 32, 4, 4), (64, 64, 3, 3))
_STRIDES = (4, 2, 1)

# one bf16 rounding of the result; order effects of a <=576-term fp32 sum of
# O(1)*O(0.1) products (~1e-5) and values that straddle the ReLU
RTOL, ATOL = 2.0 ** -8, 1e-3


def _bits(t):
    return t.view(torch.int16)


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    ws = [(torch.randn(s, generator=g) * 0.1).cuda() for s in _W_SHAPES]
    bs = [(torch.randn(s[0], generator=g) * 0.1).cuda() for s in _W_SHAPES]
    return ws, bs


def _frames(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 4, 84, 84), dtype=torch.uint8,
                         generator=g).cuda()


def _run(x, ws, bs, save):
    return atari_encoder_fwd(x, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], save)


# 1061 > 2 x 512: every persistent workgroup takes two or three images
@pytest.mark.parametrize("n", [1, 2, 3, 37, 1061])
def test_layerwise_forward_matches_torch(n):
    ws, bs = _params()
    x = _frames(n)
    outs = _run(x, ws, bs, save=True)
    torch.cuda.synchronize()
    inp = frame_cast.frame_to_bf16(x)
    for layer in range(3):
        w = ws[layer].to(torch.bfloat16).float().cpu()
        ref = F.relu(F.conv2d(inp.float().cpu(), w, bs[layer].cpu(),
                              stride=_STRIDES[layer]))
        got = outs[layer]
        assert got.dtype == torch.bfloat16 and got.shape == ref.shape
        err = (got.float().cpu() - ref).abs()
        print(f"N={n} conv{layer + 1}: max abs err {err.max():.3e} "
              f"(ref max {ref.abs().max():.3f})")
        assert torch.allclose(got.float().cpu(), ref, rtol=RTOL, atol=ATOL), \
            f"conv{layer + 1} N={n}: max abs err {err.max():.3e}"
        inp = got  # the next layer is checked on the kernel's own output


def test_save_and_nosave_agree_bitwise():
    ws, bs = _params()
    x = _frames(3)
    o1, o2, with_save = _run(x, ws, bs, save=True)
    n1, n2, without = _run(x, ws, bs, save=False)
    assert n1 is None and n2 is None and o1 is not None and o2 is not None
    assert torch.equal(_bits(with_save), _bits(without))


def test_all_byte_values_match_frame_cast():
    # pixels run through 0..255; channel k of conv1 picks one tap with
    # weight 1 and no bias, so out1 is the converted pixel itself
    x = (torch.arange(4 * 84 * 84) % 256).to(torch.uint8)
    x = x.view(1, 4, 84, 84).cuda()
    ws, bs = _params()
    w1 = torch.zeros(_W_SHAPES[0])
    taps = [(k % 4, (k // 4) % 8, (3 * k + 1) % 8) for k in range(32)]
    for k, (c, ky, kx) in enumerate(taps):
        w1[k, c, ky, kx] = 1.0
    ws[0] = w1.cuda()
    bs[0] = torch.zeros(32, device="cuda")
    out1, _, _ = _run(x, ws, bs, save=True)
    want = frame_cast.frame_to_bf16(x)
    seen = set()
    for k, (c, ky, kx) in enumerate(taps):
        tap = want[0, c, ky:ky + 77:4, kx:kx + 77:4]
        assert tap.shape == (20, 20)
        seen.update(x[0, c, ky:ky + 77:4, kx:kx + 77:4].flatten().tolist())
        assert torch.equal(_bits(out1[0, k]), _bits(tap.contiguous())), k
    assert len(seen) == 256


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_model_gradients_no_worse_than_unfused_bf16(monkeypatch):
    T, B, A = 5, 4, 6
    torch.manual_seed(0)
    model = AtariNet((4, 84, 84), A, use_lstm=True).cuda()
    g = torch.Generator().manual_seed(2)
    inputs = {
        "obs": torch.randint(0, 256, (T, B, 4, 84, 84), dtype=torch.uint8,
                             generator=g).cuda(),
        "reward": torch.randn(T, B, generator=g).cuda(),
        "done": (torch.rand(T, B, generator=g) < 0.1).cuda(),
        "last_action": torch.randint(0, A, (T, B), generator=g).cuda(),
    }
    r_logits = torch.randn(T, B, A, generator=g).cuda()
    r_base = torch.randn(T, B, generator=g).cuda()
    names = [f"{m}.{p}" for m in ("conv1", "conv2", "conv3", "fc")
             for p in ("weight", "bias")]
    params = dict(model.named_parameters())

    def run(autocast, fused):
        monkeypatch.setattr(atari_mod, "FUSED_ENCODER", fused)
        monkeypatch.setattr(atari_mod, "FUSED_ENCODER_TRAIN", fused)
        model.zero_grad(set_to_none=True)
        state = model.initial_state(B, device="cuda")
        if autocast:
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                out, _ = model(inputs, state, greedy=True)
        else:
            out, _ = model(inputs, state, greedy=True)
        loss = ((out["policy_logits"].float() * r_logits).sum() +
                (out["baseline"].float() * r_base).sum())
        loss.backward()
        res = {"loss": loss.detach().clone()}
        for k in names:
            res[k] = params[k].grad.detach().clone()
        return res

    calls = []
    real = atari_mod.fused_encoder
    monkeypatch.setattr(atari_mod, "fused_encoder",
                        lambda *a: (calls.append(1), real(*a))[1])
    fp32 = run(False, False)
    unfused = run(True, False)
    assert calls == []
    fused = run(True, True)
    assert calls == [1]

    worse = []
    for k in ["loss"] + names:
        e_unf, e_fus = _rel(unfused[k], fp32[k]), _rel(fused[k], fp32[k])
        print(f"{k}: rel L2 vs fp32  unfused {e_unf:.3e}  fused {e_fus:.3e}  "
              f"ratio {e_fus / max(e_unf, 1e-30):.2f}")
        if not e_fus <= 2.0 * e_unf:
            worse.append((k, e_unf, e_fus))
    assert not worse, worse


def test_encode_takes_fused_path_only_without_grad(monkeypatch):
    """Default switches: fused forward under no_grad (the inference worker),
    per-layer path where gradients are on (the learner), and for a view of
    the frames that is not 16-byte aligned."""
    monkeypatch.setattr(atari_mod, "FUSED_ENCODER", True)
    monkeypatch.setattr(atari_mod, "FUSED_ENCODER_TRAIN", False)
    torch.manual_seed(0)
    model = AtariNet((4, 84, 84), 6, use_lstm=False).cuda()
    explicit = AtariNet((4, 84, 84), 6, use_lstm=False, native_conv=False)
    both = AtariNet((4, 84, 84), 6, use_lstm=False, native_conv=False,
                    fused_encoder=True)
    assert model.fused_encoder and both.fused_encoder
    assert not explicit.fused_encoder
    x = _frames(3)
    calls = []
    real = atari_mod.fused_encoder
    monkeypatch.setattr(atari_mod, "fused_encoder",
                        lambda *a: (calls.append(1), real(*a))[1])
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        with_grad = model.encode(x)
        assert calls == [] and with_grad.requires_grad
        with torch.no_grad():
            fused = model.encode(x)
            assert calls == [1]
            flat = torch.zeros(x.numel() + 1, dtype=torch.uint8, device="cuda")
            flat[1:] = x.flatten()
            odd = flat[1:].view_as(x)
            assert odd.data_ptr() % 16 != 0
            unaligned = model.encode(odd)
            assert calls == [1]
        monkeypatch.setattr(atari_mod, "FUSED_ENCODER_TRAIN", True)
        model.encode(x)
        assert calls == [1, 1]
    # All three are the same features.  The paths differ by bf16 roundings
    # of the activations (2**-8 relative each, three layers and the fc), so
    # by about 1 % of the largest feature; 2 % leaves room and still catches
    # a wrong path or wrong frames.
    for other in (with_grad.detach(), unaligned):
        diff = float((fused.float() - other.float()).abs().max())
        print(f"fused vs per-layer features: max abs diff {diff:.3e} "
              f"(max {float(other.abs().max()):.3f})")
        assert diff <= 0.02 * float(other.abs().max())


@pytest.fixture
def deterministic_convs():
    # MIOpen's default weight-gradient solvers accumulate with atomics: two
    # eager runs on the same input already differ in the last bf16 bits of
    # dw.  Bit-equality needs the deterministic solvers on both sides, and
    # torch's MIOpen binding takes them only with benchmark mode off (with it
    # on, the find picks the fastest solver whatever the flag says).  Trainers
    # built by earlier tests in the same process leave benchmark mode on.
    prev = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = prev


def test_capture_replays_bit_equal_to_eager(deterministic_convs):
    n = 4
    ws, bs = _params()
    leaves = [t.requires_grad_() for pair in zip(ws, bs) for t in pair]
    g = torch.Generator().manual_seed(3)
    r = torch.randn(n, 64, 7, 7, generator=g).cuda()
    static_x = _frames(n, seed=10)

    def step():
        out = fused_encoder(static_x, *leaves)
        grads = torch.autograd.grad((out.float() * r).sum(), leaves)
        return out, grads

    # side-stream warm-up, then capture, as runtime/graphed.py does
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        g_out, g_grads = step()

    for seed in (11, 12):
        static_x.copy_(_frames(n, seed=seed))
        graph.replay()
        torch.cuda.synchronize()
        got = [g_out.clone()] + [t.clone() for t in g_grads]
        e_out, e_grads = step()
        want = [e_out] + list(e_grads)
        same = [bool(torch.equal(a, b)) for a, b in zip(got, want)]
        diff = [float((a.float() - b.float()).abs().max())
                for a, b in zip(got, want)]
        print(f"seed {seed}: out,dw1,db1,dw2,db2,dw3,db3 equal={same} "
              f"max abs diff={diff}")
        assert all(a.dtype == b.dtype for a, b in zip(got, want))
        assert all(same), (seed, same, diff)
