"""Done-masked multi-layer LSTM core.

Reference semantics: AtariNet's per-step unroll with done-masking
(algorithms/utils/atari_model.py:109-120) — `state *= notdone` each step,
then one LSTM step.  The reference calls nn.LSTM per step from Python; here:

- input-side GEMM for ALL T steps is hoisted into one rocBLAS GEMM
  ([T*B, in] @ W_ih^T);
- the sequential loop does one rocBLAS GEMM (h @ W_hh^T) + ONE fused HIP
  pointwise kernel per step (csrc/lstm.hip), forward and backward;
- CPU path uses the same structure with torch ops (the oracle).

Weights are plain nn.LSTM-layout parameters (weight_ih_l{k} etc.) so
checkpoints interop with torch LSTMs.
"""

from __future__ import annotations

from typing import List, Tuple

import torch
import torch.nn as nn

from ._backend import launch


def _pointwise_fwd(gates: torch.Tensor, c_prev: torch.Tensor,
                   out_h: torch.Tensor = None, out_c: torch.Tensor = None):
    """CPU oracle of one cell step.  Returns (h, c); `gates` is overwritten
    with activated gates, matching the GPU kernel's in-place contract."""
    i, f, g, o = gates.chunk(4, dim=1)
    i, f, g, o = i.sigmoid(), f.sigmoid(), g.tanh(), o.sigmoid()
    c_new = f * c_prev + i * g
    h_new = o * torch.tanh(c_new)
    gates.copy_(torch.cat([i, f, g, o], dim=1))
    if out_h is not None:
        out_h.copy_(h_new)
        h_new = out_h
    if out_c is not None:
        out_c.copy_(c_new)
        c_new = out_c
    return h_new, c_new


def _pointwise_bwd(gates_act, c_prev, c_out, dh, dc_in,
                   out_dgates: torch.Tensor = None,
                   out_dc_prev: torch.Tensor = None):
    """CPU oracle of one cell step's backward."""
    i, f, g, o = gates_act.chunk(4, dim=1)
    tc = torch.tanh(c_out)
    dc = dh * o * (1 - tc * tc)
    if dc_in is not None:
        dc = dc + dc_in
    di = dc * g * i * (1 - i)
    df = dc * c_prev * f * (1 - f)
    dg = dc * i * (1 - g * g)
    do = dh * tc * o * (1 - o)
    dgates = torch.cat([di, df, dg, do], dim=1)
    dc_prev = dc * f
    if out_dgates is not None:
        out_dgates.copy_(dgates)
        dgates = out_dgates
    if out_dc_prev is not None:
        out_dc_prev.copy_(dc_prev)
        dc_prev = out_dc_prev
    return dgates, dc_prev


def _grad_epilogue(dgates_all, x, hs_in, w_ih):
    """The four whole-sequence products every backward driver ends with."""
    T, B, I = x.shape
    dg2 = dgates_all.reshape(T * B, dgates_all.shape[-1])
    dx = (dg2 @ w_ih).view(T, B, I)
    dw_ih = dg2.t() @ x.reshape(T * B, I)
    dw_hh = dg2.t() @ hs_in.reshape(T * B, hs_in.shape[-1])
    db = dg2.sum(0)
    return dx, dw_ih, dw_hh, db


class _MaskedLSTMFn(torch.autograd.Function):
    """One LSTM layer unrolled over T with per-step done masking.

    x: [T,B,I]; notdone: [T,B,1]; h0,c0: [B,H]; weights nn.LSTM layout.
    Strategy: xW^T for all T hoisted to one GEMM; per step one GEMM + one
    fused cell kernel (csrc/lstm.hip) in each direction — the kernel also
    does the done-masking, so no other launch sits in the loop.  Saves
    activated gates + cell states for backward.  This is the driver that
    runs inside the captured learner graph.  CPU tensors take the pure
    torch branch (the oracle).
    """

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, notdone, h0, c0, w_ih, w_hh, b_ih, b_hh):
        T, B, I = x.shape
        H = w_hh.shape[1]
        xg = torch.addmm(b_ih + b_hh, x.reshape(T * B, I), w_ih.t()).view(T, B, 4 * H)
        hs = torch.empty(T, B, H, device=x.device, dtype=x.dtype)
        cs_in = torch.empty(T, B, H, device=x.device, dtype=x.dtype)
        cs_out = torch.empty(T, B, H, device=x.device, dtype=x.dtype)
        hs_in = torch.empty(T, B, H, device=x.device, dtype=x.dtype)
        w_hh_t = w_hh.t()
        ctx.H = H
        if x.is_cuda:
            nd = notdone.reshape(T, B).contiguous()
            launch("lstm_mask_rows", h0.contiguous(), c0.contiguous(), nd[0],
                   hs_in[0], cs_in[0], B, H)
            for t in range(T):
                # the recurrent product accumulates into the hoisted
                # x-side preactivations: xg doubles as the saved gate
                # buffer, no per-step copy
                xg[t].addmm_(hs_in[t], w_hh_t)
                last = t == T - 1
                launch("lstm_cell_fwd",
                       xg[t], cs_in[t], hs[t], cs_out[t],
                       None if last else nd[t + 1],
                       None if last else hs_in[t + 1],
                       None if last else cs_in[t + 1], B, H)
            ctx.save_for_backward(x, nd, hs_in, cs_in, cs_out, xg, w_ih,
                                  w_hh)
            return hs, hs[T - 1].clone(), cs_out[T - 1].clone()
        h, c = h0.contiguous(), c0.contiguous()
        gates_all = torch.empty(T, B, 4 * H, device=x.device, dtype=x.dtype)
        for t in range(T):
            nd = notdone[t]
            h = torch.mul(h, nd, out=hs_in[t])
            c = torch.mul(c, nd, out=cs_in[t])
            torch.addmm(xg[t], h, w_hh_t, out=gates_all[t])
            h, c = _pointwise_fwd(gates_all[t], c, out_h=hs[t],
                                  out_c=cs_out[t])
        ctx.save_for_backward(x, notdone, hs_in, cs_in, cs_out, gates_all,
                              w_ih, w_hh)
        # final h/c alias hs[T-1]/cs_out[T-1] after the out=-form loop;
        # clone so the Function's outputs don't share storage
        return hs, h.clone(), c.clone()

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, d_hs, d_hT, d_cT):
        (x, notdone, hs_in, cs_in, cs_out, gates_all, w_ih,
         w_hh) = ctx.saved_tensors
        T, B, I = x.shape
        dgates_all = torch.empty_like(gates_all)
        if x.is_cuda:
            H = ctx.H
            nd = notdone  # [T,B] contiguous, from forward
            d_hs_c = d_hs.contiguous()
            d_hT_c = d_hT.contiguous()
            dc_carry = d_cT.contiguous().clone()
            g = torch.empty_like(dc_carry)  # raw dgates[t+1] @ w_hh
            for t in range(T - 1, -1, -1):
                last = t == T - 1
                launch("lstm_cell_bwd",
                       gates_all[t], cs_in[t], cs_out[t],
                       d_hs_c[t], d_hT_c if last else g,
                       None if last else nd[t + 1], nd[t],
                       dc_carry, dgates_all[t], B, H)
                torch.mm(dgates_all[t], w_hh, out=g)
            dh0 = g.mul_(nd[0].unsqueeze(1))
            dx, dw_ih, dw_hh, db = _grad_epilogue(dgates_all, x, hs_in, w_ih)
            return dx, None, dh0, dc_carry, dw_ih, dw_hh, db, db
        dh_carry = d_hT.contiguous().clone()
        dc_carry = d_cT.contiguous().clone()
        dh_buf = torch.empty_like(dh_carry)
        dc_prev_buf = torch.empty_like(dc_carry)
        for t in range(T - 1, -1, -1):
            dh = torch.add(d_hs[t], dh_carry, out=dh_buf)
            dgates, dc_prev = _pointwise_bwd(
                gates_all[t], cs_in[t], cs_out[t], dh, dc_carry,
                out_dgates=dgates_all[t], out_dc_prev=dc_prev_buf)
            nd = notdone[t]
            torch.mm(dgates, w_hh, out=dh_carry)
            dh_carry.mul_(nd)
            torch.mul(dc_prev, nd, out=dc_carry)
        dx, dw_ih, dw_hh, db = _grad_epilogue(dgates_all, x, hs_in, w_ih)
        return dx, None, dh_carry, dc_carry, dw_ih, dw_hh, db, db


class _MaskedLSTMSeqFn(torch.autograd.Function):
    """One LSTM layer unrolled over T with the loop driven from C++
    (csrc/lstm_seq.hip): per step one rocBLAS SGEMM + one fused cell kernel,
    all enqueued natively — removes the ~20 ms/iter of Python launch
    overhead the per-step path pays in eager mode (profiles/README.md).
    Same kernels and numerics as :class:`_MaskedLSTMFn`; GPU only."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, notdone, h0, c0, w_ih, w_hh, b_ih, b_hh):
        T, B, I = x.shape
        H = w_hh.shape[1]
        dev = x.device
        xg = torch.addmm(b_ih + b_hh, x.reshape(T * B, I),
                         w_ih.t()).view(T, B, 4 * H).contiguous()
        hs = torch.empty(T, B, H, device=dev)
        hs_in = torch.empty(T, B, H, device=dev)
        cs_in = torch.empty(T, B, H, device=dev)
        cs_out = torch.empty(T, B, H, device=dev)
        nd = notdone.reshape(T, B).contiguous()
        w_hh_c = w_hh.contiguous()
        launch("masked_lstm_seq_fwd", xg, w_hh_c, nd, h0.contiguous(),
               c0.contiguous(), hs, hs_in, cs_in, cs_out, T, B, H)
        ctx.save_for_backward(x, nd, hs_in, cs_in, cs_out, xg, w_ih, w_hh_c)
        ctx.H = H
        return hs, hs[T - 1].clone(), cs_out[T - 1].clone()

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, d_hs, d_hT, d_cT):
        x, nd, hs_in, cs_in, cs_out, gates_all, w_ih, w_hh = ctx.saved_tensors
        T, B, I = x.shape
        H = ctx.H
        dev = x.device
        dgates_all = torch.empty(T, B, 4 * H, device=dev)
        dh_carry = torch.empty(B, H, device=dev)
        dc_carry = d_cT.contiguous().clone()
        launch("masked_lstm_seq_bwd", gates_all, cs_in, cs_out,
               d_hs.contiguous(), d_hT.contiguous(), nd, w_hh, dgates_all,
               dh_carry, dc_carry, T, B, H)
        dx, dw_ih, dw_hh, db = _grad_epilogue(dgates_all, x, hs_in, w_ih)
        return dx, None, dh_carry, dc_carry, dw_ih, dw_hh, db, db


_USE_SEQ = None


def _use_seq_path() -> bool:
    """C++-driven sequence loop (hardware-validated r2: oracle tests pass,
    25.5 vs 28.2 ms/iter at B=256 on the learner micro).  Default ON on
    GPU; SCALERL_LSTM_SEQ=0 falls back to the per-step Python path."""
    global _USE_SEQ
    if _USE_SEQ is None:
        import os
        _USE_SEQ = os.environ.get("SCALERL_LSTM_SEQ", "1") != "0"
    return _USE_SEQ


class MaskedLSTM(nn.Module):
    """Multi-layer done-masked LSTM with nn.LSTM-compatible parameters."""

    def __init__(self, input_size: int, hidden_size: int, num_layers: int = 1):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.num_layers = num_layers
        for k in range(num_layers):
            in_sz = input_size if k == 0 else hidden_size
            w_ih = nn.Parameter(torch.empty(4 * hidden_size, in_sz))
            w_hh = nn.Parameter(torch.empty(4 * hidden_size, hidden_size))
            b_ih = nn.Parameter(torch.empty(4 * hidden_size))
            b_hh = nn.Parameter(torch.empty(4 * hidden_size))
            # match nn.LSTM defaults: ALL params uniform(-H^-0.5, H^-0.5),
            # biases included, so fresh-training dynamics match the
            # reference's torch LSTM core (atari_model.py:51-55)
            for w in (w_ih, w_hh, b_ih, b_hh):
                nn.init.uniform_(w, -hidden_size ** -0.5, hidden_size ** -0.5)
            setattr(self, f"weight_ih_l{k}", w_ih)
            setattr(self, f"weight_hh_l{k}", w_hh)
            setattr(self, f"bias_ih_l{k}", b_ih)
            setattr(self, f"bias_hh_l{k}", b_hh)

    def initial_state(self, batch_size: int, device=None):
        z = torch.zeros(self.num_layers, batch_size, self.hidden_size,
                        device=device)
        return (z, z.clone())

    def forward(self, x: torch.Tensor, notdone: torch.Tensor,
                state: Tuple[torch.Tensor, torch.Tensor]):
        """x [T,B,I], notdone [T,B] → out [T,B,H], (hN, cN) [L,B,H]."""
        h0, c0 = state
        # The recurrent core runs fp32 (it is tiny and latency-bound; the
        # fused pointwise kernels are fp32) even when the encoder is bf16.
        x = x.float()
        nd = notdone.unsqueeze(-1).float()
        hs_out: List[torch.Tensor] = []
        cs_out: List[torch.Tensor] = []
        out = x
        # The C++ seq loop drives a process-global rocBLAS handle, which is
        # NOT safe to call from two threads at once (the thread-mode
        # inference worker shares the process with the learner).  T==1 has
        # no launch-overhead to amortize anyway, so single-step forwards
        # (the inference worker's shape) take the per-step path, keeping
        # the seq loop learner-only.
        fn = (_MaskedLSTMSeqFn if (x.is_cuda and x.shape[0] > 1 and
                                   _use_seq_path())
              else _MaskedLSTMFn)
        for k in range(self.num_layers):
            out, hN, cN = fn.apply(
                out.contiguous(), nd, h0[k], c0[k],
                getattr(self, f"weight_ih_l{k}"),
                getattr(self, f"weight_hh_l{k}"),
                getattr(self, f"bias_ih_l{k}"),
                getattr(self, f"bias_hh_l{k}"))
            hs_out.append(hN)
            cs_out.append(cN)
        return out, (torch.stack(hs_out), torch.stack(cs_out))
