"""Per-tick fp64 restatement of the encoder LSTM stack (oracle/arcvae_oracle.py: mlx_lstm semantics, M1).

The step-level parity tests see the encoder sweeps only through sums over t (the parameter gradients) and the last tick
(mu / logvar / z).  At the default init the gate gradients shrink by about half per tick going back in time, so most ticks
add nothing visible to those sums.  The functions here judge every tick (l, t) on its own scale instead:

* forward_local: h, c and the post-activation gates of every tick, each from the GPU's own h_{t-1}, c_{t-1} and layer input;
* bptt: the gate gradients dG, chained in fp64 from the GPU's own forward states and dh_top (forward rounding never enters);
* dgo_local: the o-gate quarter of dG[l, t] from the GPU's own dG^l[t+1] and dG^{l+1}[t] (a local check of the dh path);
* wgrad_from: the stack's parameter gradients as fp64 sums over the GPU's own dG and h;
* tick_check: |got - ref| <= rtol*|ref| + atol_frac*max|ref[l, t]|, per tick.

Semantics: gate order i, f, g, o; at t = 0 there is no recurrent term and c_0 = i*g; layer 0 reads embedding[x], layer
l > 0 reads h^{l-1}_t; dG is the gradient w.r.t. the gate pre-activations, [L, T, R, 4H] (include/arcvae_hip.h); dWh pairs
dG[t] with h[t-1], for t >= 1 only.

Rows are independent in both recurrences, so every function takes a `rows` index into the batch: x is the whole [B, T]
token batch, and the state arrays ([L, T, *, H] / [L, T, *, 4H]) hold either all B rows or exactly `rows`, in that order.
"""
from __future__ import annotations

import dataclasses
from typing import Dict

import numpy as np
import torch

F64 = np.float64


def _p(params, l: int, leaf: str, dtype=F64) -> np.ndarray:
    return np.asarray(params[f"encoder.lstm_layer_{l}.{leaf}"], dtype=dtype)


def num_layers(params) -> int:
    return sum(1 for k in params if k.startswith("encoder.lstm_layer_") and k.endswith(".Wh"))


def _rows(a, rows):
    """The `rows` of a state array [L, T, B or R, ...] (already the subset when its row axis has len(rows) entries)."""
    a = np.asarray(a)
    return a if a.shape[2] == len(rows) else a[:, :, rows]


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _act(pre):
    """Post-activation gates (i, f, g, o) of pre-activations [..., 4H]."""
    H = pre.shape[-1] // 4
    out = _sig(pre)
    out[..., 2 * H:3 * H] = np.tanh(pre[..., 2 * H:3 * H])
    return out


def _inputs(params, x, rows, dtype=F64):
    """Layer-0 input embedding[x] of the rows, time-major [T, R, E]."""
    emb = np.asarray(params["encoder.embedding.weight"], dtype=dtype)
    return emb[np.asarray(x)[rows].T]


def run_forward(params, x, rows, dtype=F64):
    """A free-running forward of the stack in `dtype` (every tick from this run's own states): hseq, cseq [L, T, R, H] and
    the post-activation gates [L, T, R, 4H].  Stands in for a GPU forward in the CPU tests."""
    L = num_layers(params)
    inp = _inputs(params, x, rows, dtype)
    T, R = inp.shape[0], inp.shape[1]
    H = _p(params, 0, "Wh").shape[1]
    hs = np.zeros((L, T, R, H), dtype)
    cs = np.zeros((L, T, R, H), dtype)
    gs = np.zeros((L, T, R, 4 * H), dtype)
    for l in range(L):
        Wx, Wh, b = _p(params, l, "Wx", dtype), _p(params, l, "Wh", dtype), _p(params, l, "bias", dtype)
        xw = inp @ Wx.T + b
        for t in range(T):
            pre = xw[t] + hs[l, t - 1] @ Wh.T if t > 0 else xw[t]
            g = _act(pre)
            H1, H2, H3 = H, 2 * H, 3 * H
            c = g[:, :H1] * g[:, H2:H3]
            if t > 0:
                c = c + g[:, H1:H2] * cs[l, t - 1]
            cs[l, t], gs[l, t] = c, g
            hs[l, t] = g[:, H3:] * np.tanh(c)
        inp = hs[l]
    return hs, cs, gs


def forward_local(params, x, hseq, cseq, rows):
    """fp64 h, c and post-activation gates of every tick (l, t), each from the given h^l_{t-1}, c^l_{t-1} and layer input
    (embedding[x_t] or h^{l-1}_t): a strictly local check.  Returns (h, c, gates) of the rows, [L, T, R, H|4H]."""
    L = num_layers(params)
    hs = _rows(hseq, rows).astype(F64)
    cs = _rows(cseq, rows).astype(F64)
    H = hs.shape[-1]
    gates = np.empty(hs.shape[:3] + (4 * H,), F64)
    for l in range(L):
        inp = _inputs(params, x, rows) if l == 0 else hs[l - 1]
        pre = inp @ _p(params, l, "Wx").T + _p(params, l, "bias")
        pre[1:] += hs[l, :-1] @ _p(params, l, "Wh").T       # all ticks as one batched product
        gates[l] = _act(pre)
    i, f, g, o = (gates[..., k * H:(k + 1) * H] for k in range(4))
    c = i * g
    c[:, 1:] += f[:, 1:] * cs[:, :-1]
    return o * np.tanh(c), c, gates


def bptt(params, x, hseq, cseq, dh_top, rows, gates=None, dtype=F64):
    """dG [L, T, R, 4H] of the rows, chained from the given forward states (gates recomputed from them unless passed in)
    and dh_top [R or B, H] = d/d h^{L-1}_{T-1}.  dtype float32 gives a plain fp32 restatement of the same chain."""
    L = num_layers(params)
    hs = _rows(hseq, rows)
    cs = _rows(cseq, rows).astype(dtype)
    if gates is None:
        gates = forward_local(params, x, hs, cs, rows)[2]
    gates = np.asarray(gates, dtype=dtype)
    dh_top = np.asarray(dh_top)
    dh_top = (dh_top if dh_top.shape[0] == len(rows) else dh_top[rows]).astype(dtype)
    T, R, H = cs.shape[1], cs.shape[2], cs.shape[3]
    # dh^l_t = dG^l[t+1] Wh_l + dG^{l+1}[t] Wx_{l+1}: one product per tick and layer over the stacked weights
    wcat = [np.concatenate([_p(params, l, "Wh", dtype)] + ([_p(params, l + 1, "Wx", dtype)] if l + 1 < L else []), 0)
            for l in range(L)]
    dG = np.zeros((L, T, R, 4 * H), dtype)
    dc = [np.zeros((R, H), dtype) for _ in range(L)]
    zero = np.zeros((R, 4 * H), dtype)
    for t in range(T - 1, -1, -1):
        for l in range(L - 1, -1, -1):
            src = [dG[l, t + 1] if t + 1 < T else zero] + ([dG[l + 1, t]] if l + 1 < L else [])
            dh = np.concatenate(src, 1) @ wcat[l]
            if l == L - 1 and t == T - 1:
                dh = dh + dh_top
            g = gates[l, t]
            i, f, gg, o = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
            tc = np.tanh(cs[l, t])
            d_c = dh * o * (1 - tc * tc)
            if t + 1 < T:
                d_c = d_c + dc[l] * gates[l, t + 1, :, H:2 * H]
            dc[l] = d_c
            out = dG[l, t]
            out[:, :H] = d_c * gg * i * (1 - i)
            if t > 0:
                out[:, H:2 * H] = d_c * cs[l, t - 1] * f * (1 - f)
            out[:, 2 * H:3 * H] = d_c * i * (1 - gg * gg)
            out[:, 3 * H:] = dh * tc * o * (1 - o)
    return dG


def dgo_local(params, x, hseq, cseq, dG, dh_top, rows, gates=None):
    """fp64 o-gate quarter [L, T, R, H] of dG[l, t], each from the given dG^l[t+1] Wh_l + dG^{l+1}[t] Wx_{l+1} (+ dh_top at
    the top layer, T-1) and the tick's own o, c: a wrong dh at one tick shows at that tick, with no accumulation."""
    L = num_layers(params)
    hs = _rows(hseq, rows)
    cs = _rows(cseq, rows).astype(F64)
    dg = _rows(dG, rows).astype(F64)
    if gates is None:
        gates = forward_local(params, x, hs, cs, rows)[2]
    dh_top = np.asarray(dh_top)
    dh_top = (dh_top if dh_top.shape[0] == len(rows) else dh_top[rows]).astype(F64)
    H = cs.shape[-1]
    dh = np.zeros(cs.shape, F64)
    for l in range(L):
        dh[l, :-1] = dg[l, 1:] @ _p(params, l, "Wh")
        if l + 1 < L:
            dh[l] += dg[l + 1] @ _p(params, l + 1, "Wx")
    dh[L - 1, -1] += dh_top
    o = np.asarray(gates, F64)[..., 3 * H:]
    return dh * np.tanh(cs) * o * (1 - o)


def wgrad_from(params, x, hseq, dG) -> Dict[str, torch.Tensor]:
    """fp64 sums over ALL rows of the given dG [L, T, B, 4H] and hseq [L, T, B, H] (numpy arrays or torch tensors; the sums
    are formed with torch on their device): encoder.lstm_layer_l.{Wx, Wh, bias} and encoder.embedding.weight."""
    hs = torch.as_tensor(hseq)
    dG = torch.as_tensor(dG)
    dev = hs.device
    L, T, B, H = hs.shape
    G = 4 * H

    def w(name):
        return torch.as_tensor(np.asarray(params[name]), dtype=torch.float64, device=dev)

    tok = torch.as_tensor(np.ascontiguousarray(np.asarray(x).T), device=dev).reshape(-1).long()   # time-major, as dG
    out = {}
    for l in range(L):
        pre = f"encoder.lstm_layer_{l}."
        g = dG[l].to(torch.float64).reshape(T * B, G)
        out[pre + "bias"] = g.sum(0)
        if T > 1:
            out[pre + "Wh"] = g[B:].t() @ hs[l, :-1].reshape((T - 1) * B, H).to(torch.float64)
        else:
            out[pre + "Wh"] = torch.zeros(G, H, dtype=torch.float64, device=dev)
        if l == 0:
            # sum over the tokens first: d(token table) [V, 4H], then both factors of table0 = embedding . Wx_0^T
            emb = w("encoder.embedding.weight")
            dtab = torch.zeros(emb.shape[0], G, dtype=torch.float64, device=dev).index_add_(0, tok, g)
            out[pre + "Wx"] = dtab.t() @ emb
            out["encoder.embedding.weight"] = dtab @ w(pre + "Wx")
        else:
            out[pre + "Wx"] = g.t() @ hs[l - 1].reshape(T * B, H).to(torch.float64)
        del g
    return out


@dataclasses.dataclass
class TickReport:
    worst: float              # worst ratio |got - ref| / bound over the judged ticks (<= 1 passes)
    where: tuple              # (l, t, index within the tick) of the worst element
    skipped: int              # ticks whose fp64 scale is below the floor
    per_tick: np.ndarray      # [L, T] worst ratio per tick (0 for skipped ticks)

    def __str__(self):
        return f"worst {self.worst:.3g} at (l, t, i) = {self.where}, {self.skipped} ticks below the floor"


def tick_check(got, ref, rtol: float = 1e-4, atol_frac: float = 4e-6, floor: float = 1e-30) -> TickReport:
    """Per tick (l, t) of [L, T, ...] arrays: the worst |got - ref| / (rtol*|ref| + atol_frac*max|ref[l, t]|) and where it
    is.  Ticks with max|ref[l, t]| < floor are skipped and counted.  A non-finite `got` is an infinite ratio."""
    got = np.asarray(got)
    ref = np.asarray(ref, dtype=F64)
    L, T = ref.shape[:2]
    a = got.reshape(L, T, -1).astype(F64)
    b = ref.reshape(L, T, -1)
    scale = np.abs(b).max(axis=2)
    keep = scale >= floor
    per_tick = np.zeros((L, T))
    where, worst = None, 0.0
    for l in range(L):
        for t in range(T):
            if not keep[l, t]:
                continue
            r = np.abs(a[l, t] - b[l, t]) / (rtol * np.abs(b[l, t]) + atol_frac * scale[l, t])
            r[~np.isfinite(r)] = np.inf
            i = int(np.argmax(r))
            per_tick[l, t] = r[i]
            if where is None or r[i] > worst:
                worst, where = float(r[i]), (l, t, i)
    return TickReport(worst, where, int((~keep).sum()), per_tick)


def tick_scales(a) -> np.ndarray:
    """max|a[l, t]| per tick, [L, T]."""
    a = np.asarray(a)
    return np.abs(a.reshape(a.shape[0], a.shape[1], -1)).max(axis=2)


def long_memory(params, cfg) -> Dict[str, np.ndarray]:
    """A copy of the parameters with the encoder's forget-gate bias slice bias[H:2H] += 3 and Wh x 0.5 in every layer: the
    gate gradients then stay within a few percent of the largest tick over T = 128, so every tick reaches the sums."""
    H = cfg.H
    out = {k: np.array(v, copy=True) for k, v in params.items()}
    for l in range(cfg.L):
        b = out[f"encoder.lstm_layer_{l}.bias"]
        b[H:2 * H] += np.float32(3.0)
        out[f"encoder.lstm_layer_{l}.Wh"] = (out[f"encoder.lstm_layer_{l}.Wh"] * np.float32(0.5)).astype(np.float32)
    return out
