"""Fused LSTM cell kernels (csrc/lstm.hip) and the two drivers built on them.

CPU part: a torch emulation of the fused step order — the forward kernel
writing the NEXT step's masked state, the backward kernel masking the raw
recurrent product with notdone[t+1], the in-place dc carry and the
d_h0/d_c0 epilogue — against the per-step autograd Function on CPU (the
oracle), in the style of test_lstm_seq_formulas.py and at its tolerances.

GPU part: CUDA MaskedLSTM against CPU MaskedLSTM over shapes that cover one
block, several blocks with a ragged tail and the real hidden size, under
every done pattern that exercises a mask edge; per-step driver against the
C++ driver; and a captured graph replayed against eager.
"""

import functools

import pytest
import torch

import scalerl_amd.ops.lstm as lstm_mod
from scalerl_amd.ops.lstm import MaskedLSTM, _MaskedLSTMFn

PATTERNS = ("none", "first", "last", "all", "random")


def _notdone(pattern: str, T: int, B: int, gen: torch.Generator):
    nd = torch.ones(T, B)
    if pattern == "first":
        nd[0] = 0.0
    elif pattern == "last":
        nd[T - 1] = 0.0
    elif pattern == "all":
        nd.zero_()
    elif pattern == "random":
        nd = (torch.rand(T, B, generator=gen) >= 0.3).float()
    return nd


# -- CPU: emulation of the fused step order ---------------------------------

def emu_fused_fwd(xg, w_hh, nd, h0, c0):
    """Mirror of the fused forward loop, including buffer roles.  Buffers
    start as NaN so a slot the loop never writes cannot pass."""
    T, B, H4 = xg.shape
    H = H4 // 4
    nan = float("nan")
    hs = torch.full((T, B, H), nan)
    hs_in = torch.full((T, B, H), nan)
    cs_in = torch.full((T, B, H), nan)
    cs_out = torch.full((T, B, H), nan)
    gates = xg.clone()
    # lstm_mask_rows before the loop
    hs_in[0] = h0 * nd[0].unsqueeze(1)
    cs_in[0] = c0 * nd[0].unsqueeze(1)
    for t in range(T):
        gates[t] += hs_in[t] @ w_hh.t()           # GEMM, beta = 1, in place
        pre = gates[t]
        i = torch.sigmoid(pre[:, 0 * H:1 * H])
        f = torch.sigmoid(pre[:, 1 * H:2 * H])
        g = torch.tanh(pre[:, 2 * H:3 * H])
        o = torch.sigmoid(pre[:, 3 * H:4 * H])
        c = f * cs_in[t] + i * g
        h = o * torch.tanh(c)
        gates[t] = torch.cat([i, f, g, o], dim=1)
        hs[t], cs_out[t] = h, c
        if t + 1 < T:                              # nd_next non-null
            hs_in[t + 1] = h * nd[t + 1].unsqueeze(1)
            cs_in[t + 1] = c * nd[t + 1].unsqueeze(1)
    return hs, hs[T - 1].clone(), cs_out[T - 1].clone(), gates, hs_in, \
        cs_in, cs_out


def emu_fused_bwd(gates, cs_in, cs_out, d_hs, d_hT, d_cT, nd, w_hh):
    """Mirror of the fused backward loop: raw g masked by nd[t+1] on use,
    dc carry updated in place, d_h0/d_c0 epilogue."""
    T, B, H4 = gates.shape
    H = H4 // 4
    dgates_all = torch.full_like(gates, float("nan"))
    dc_carry = d_cT.clone()
    g_raw = None
    for t in range(T - 1, -1, -1):
        i = gates[t][:, 0 * H:1 * H]
        f = gates[t][:, 1 * H:2 * H]
        g = gates[t][:, 2 * H:3 * H]
        o = gates[t][:, 3 * H:4 * H]
        tc = torch.tanh(cs_out[t])
        gm = d_hT if t == T - 1 else g_raw * nd[t + 1].unsqueeze(1)
        dh = d_hs[t] + gm
        dc = dc_carry + dh * o * (1 - tc * tc)
        dgates_all[t] = torch.cat([dc * g * i * (1 - i),
                                   dc * cs_in[t] * f * (1 - f),
                                   dc * i * (1 - g * g),
                                   dh * tc * o * (1 - o)], dim=1)
        dc_carry.copy_((dc * f) * nd[t].unsqueeze(1))   # in place
        g_raw = dgates_all[t] @ w_hh                    # raw, unmasked
    d_h0 = g_raw * nd[0].unsqueeze(1)
    return dgates_all, d_h0, dc_carry


CPU_CASES = [
    # (T, B, pattern)
    (1, 3, "random"),
    (2, 3, "random"),
    (5, 4, "first"),
    (6, 4, "last"),
    (4, 3, "all"),
]


@pytest.mark.parametrize("T,B,pattern", CPU_CASES)
def test_fused_step_order_matches_per_step_function(T, B, pattern):
    gen = torch.Generator().manual_seed(1000 + 10 * T + B)
    I, H = 7, 11
    ml = MaskedLSTM(I, H, num_layers=1)
    x = torch.randn(T, B, I, generator=gen).requires_grad_()
    nd = _notdone(pattern, T, B, gen)
    h0 = (torch.randn(B, H, generator=gen) + 0.5).requires_grad_()
    c0 = (torch.randn(B, H, generator=gen) - 0.5).requires_grad_()
    params = (ml.weight_ih_l0, ml.weight_hh_l0, ml.bias_ih_l0, ml.bias_hh_l0)

    hs_ref, hT_ref, cT_ref = _MaskedLSTMFn.apply(
        x, nd.unsqueeze(-1), h0, c0, *params)
    d_hs = torch.randn(T, B, H, generator=gen)
    d_hT = torch.randn(B, H, generator=gen)
    d_cT = torch.randn(B, H, generator=gen)
    grads_ref = torch.autograd.grad(
        (hs_ref, hT_ref, cT_ref), (x, h0, c0) + params, (d_hs, d_hT, d_cT))

    with torch.no_grad():
        xg = (x.reshape(T * B, I) @ ml.weight_ih_l0.t()
              + ml.bias_ih_l0 + ml.bias_hh_l0).view(T, B, 4 * H)
        hs, hT, cT, gates, hs_in, cs_in, cs_out = emu_fused_fwd(
            xg, ml.weight_hh_l0, nd, h0, c0)
        torch.testing.assert_close(hs, hs_ref, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(hT, hT_ref, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(cT, cT_ref, rtol=1e-5, atol=1e-6)

        dgates_all, dh0, dc0 = emu_fused_bwd(
            gates, cs_in, cs_out, d_hs, d_hT, d_cT, nd, ml.weight_hh_l0)
        dg2 = dgates_all.reshape(T * B, 4 * H)
        dx = (dg2 @ ml.weight_ih_l0).view(T, B, I)
        dw_ih = dg2.t() @ x.reshape(T * B, I)
        dw_hh = dg2.t() @ hs_in.reshape(T * B, H)
        db = dg2.sum(0)
    got = (dx, dh0, dc0, dw_ih, dw_hh, db, db)
    for a, r in zip(got, grads_ref):
        torch.testing.assert_close(a, r, rtol=1e-4, atol=1e-5)
    if pattern in ("first", "all"):
        assert torch.count_nonzero(dh0) == 0
        assert torch.count_nonzero(dc0) == 0


# -- GPU: CUDA MaskedLSTM vs CPU MaskedLSTM ---------------------------------

SHAPES = [
    # (T, B, I, H, L)
    (1, 1, 3, 5, 1),
    (2, 3, 4, 5, 2),
    (3, 5, 8, 130, 1),     # B*H = 650: three blocks, ragged tail
    (5, 2, 519, 519, 2),   # the real hidden size
]


def _param_names(L):
    return [f"{n}_l{k}" for k in range(L)
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


@functools.lru_cache(maxsize=None)
def _case(shape, pattern):
    """Inputs, loss weights and the CPU result of one case (computed once,
    shared by every test that needs it; never modified)."""
    T, B, I, H, L = shape
    gen = torch.Generator().manual_seed(
        7919 * SHAPES.index(shape) + PATTERNS.index(pattern))
    ml = MaskedLSTM(I, H, num_layers=L)
    with torch.no_grad():
        for p in ml.parameters():
            p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * H ** -0.5)
    inp = {
        "x": torch.randn(T, B, I, generator=gen),
        "nd": _notdone(pattern, T, B, gen),
        "h0": torch.randn(L, B, H, generator=gen) + 0.25,
        "c0": torch.randn(L, B, H, generator=gen) - 0.25,
        "w_out": torch.randn(T, B, H, generator=gen),
        "w_h": torch.randn(L, B, H, generator=gen),
        "w_c": torch.randn(L, B, H, generator=gen),
    }
    ref = _run(ml, inp, "cpu")
    return ml.state_dict(), inp, ref


def _run(ml, inp, device):
    """Forward + backward of the weighted loss; everything back on CPU."""
    d = {k: v.to(device) for k, v in inp.items()}
    x = d["x"].clone().requires_grad_()
    h0 = d["h0"].clone().requires_grad_()
    c0 = d["c0"].clone().requires_grad_()
    ml.zero_grad()
    out, (hN, cN) = ml(x, d["nd"], (h0, c0))
    loss = ((out * d["w_out"]).sum() + (hN * d["w_h"]).sum()
            + (cN * d["w_c"]).sum())
    loss.backward()
    res = {"out": out, "hN": hN, "cN": cN, "dx": x.grad, "dh0": h0.grad,
           "dc0": c0.grad}
    for n in _param_names(ml.num_layers):
        res["d" + n] = getattr(ml, n).grad
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def _run_gpu(shape, pattern, use_seq):
    sd, inp, _ = _case(shape, pattern)
    T, B, I, H, L = shape
    mg = MaskedLSTM(I, H, num_layers=L).cuda()
    mg.load_state_dict(sd)
    prev = lstm_mod._USE_SEQ
    lstm_mod._USE_SEQ = use_seq
    try:
        return _run(mg, inp, "cuda")
    finally:
        lstm_mod._USE_SEQ = prev


def _tol(key):
    """Tolerances of test_masked_lstm_gpu_matches_cpu: forward values as its
    `out`, input-side gradients as its x.grad, parameter gradients as its
    weight_hh grad."""
    if key in ("out", "hN", "cN"):
        return dict(rtol=1e-4, atol=1e-4)
    if key in ("dx", "dh0", "dc0"):
        return dict(rtol=1e-3, atol=1e-4)
    return dict(rtol=1e-3, atol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_lstm_gpu_matches_cpu_and_drivers_agree(shape, pattern):
    _, _, ref = _case(shape, pattern)
    step = _run_gpu(shape, pattern, use_seq=False)   # per-step driver
    seq = _run_gpu(shape, pattern, use_seq=True)     # C++ driver (T > 1)
    for name, got in (("per-step", step), ("seq", seq)):
        for k, r in ref.items():
            torch.testing.assert_close(got[k], r, **_tol(k),
                                       msg=lambda m: f"{name} {k}: {m}")
        if pattern in ("first", "all"):
            assert torch.count_nonzero(got["dh0"]) == 0, name
            assert torch.count_nonzero(got["dc0"]) == 0, name
    # driver equality, tolerances of
    # test_masked_lstm_seq_path_matches_python_path
    for k in ref:
        torch.testing.assert_close(seq[k], step[k], rtol=1e-4, atol=1e-5,
                                   msg=lambda m: f"seq vs per-step {k}: {m}")


@pytest.mark.gpu
def test_fused_lstm_graph_replay_equals_eager():
    """Capture forward+backward of the per-step driver (the one the learner
    graph holds), replay on two different inputs and masks copied into the
    static buffers; results must be bit-equal to eager."""
    T, B, I, H, L = 4, 3, 6, 10, 2
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(4242)
    ml = MaskedLSTM(I, H, num_layers=L).to(dev)
    params = [getattr(ml, n) for n in _param_names(L)]
    w_out = torch.randn(T, B, H, generator=gen).to(dev)
    w_h = torch.randn(L, B, H, generator=gen).to(dev)
    w_c = torch.randn(L, B, H, generator=gen).to(dev)

    def make_inputs(pattern):
        return (torch.randn(T, B, I, generator=gen).to(dev),
                _notdone(pattern, T, B, gen).to(dev),
                (torch.randn(L, B, H, generator=gen) + 0.25).to(dev),
                (torch.randn(L, B, H, generator=gen) - 0.25).to(dev))

    def fwd_bwd(x, nd, h0, c0):
        out, (hN, cN) = ml(x, nd, (h0, c0))
        loss = (out * w_out).sum() + (hN * w_h).sum() + (cN * w_c).sum()
        grads = torch.autograd.grad(loss, [x, h0, c0] + params)
        return [out, hN, cN] + list(grads)

    static = [t.clone() for t in make_inputs("random")]
    for i in (0, 2, 3):
        static[i].requires_grad_()

    prev = lstm_mod._USE_SEQ
    lstm_mod._USE_SEQ = False
    try:
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(2):
                fwd_bwd(*static)
        torch.cuda.current_stream(dev).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            static_out = fwd_bwd(*static)

        for pattern in ("random", "first"):
            fresh = make_inputs(pattern)
            with torch.no_grad():
                for dst, src in zip(static, fresh):
                    dst.copy_(src)
            graph.replay()
            got = [t.detach().clone() for t in static_out]
            eager_in = [t.clone() for t in fresh]
            for i in (0, 2, 3):
                eager_in[i].requires_grad_()
            want = fwd_bwd(*eager_in)
            torch.cuda.synchronize()
            for k, (g, w) in enumerate(zip(got, want)):
                assert torch.equal(g, w.detach()), \
                    f"{pattern}: output {k} differs between replay and eager"
    finally:
        lstm_mod._USE_SEQ = prev
