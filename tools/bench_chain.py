#!/usr/bin/env python3
"""Exact MAP decoding and exact chain marginals at BASELINE.json configs[4]'s shape on 1 MI355X: 10 000 molecules as
9 x bs 1024 + 784, the default AR-CVAE (random-init weights), max_length 80 and 128, early stopping on (the API default) --
next to the greedy sampler (captured decode pass) and generate_beam at K = 1, 4, 32 in the same process, every method once per
repetition, median of --reps.

One generate_map batch = the dense decoder pass over B*V rows + arcvae_dec_row_lse + arcvae_dec_viterbi, launched eagerly, plus
the host read of the lengths for early stopping; one token_marginals batch = the same two passes + arcvae_dec_chain_marginals.
Also reported: the share of the 10 000 rows whose MAP score is strictly above the beam's best hypothesis at each K (it is never
below), and a kernel-level split of one bs-1024 batch from device events around each launch (median of --reps).  Prints one
JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlx-vae_amd"))
import torch  # noqa: E402
from arcvae_hip._lib import call, ptr, stream_ptr  # noqa: E402
from models.vae import ARCVAE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--widths", default="1,4,32")
ap.add_argument("--max-lengths", default="80,128")
ap.add_argument("--out", default="")
args = ap.parse_args()

vae = ARCVAE(vocab_size=80, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
             generator=torch.Generator().manual_seed(0))
samp = vae.decoder_sampling
rs = np.random.RandomState(0)
conds = [torch.tensor(rs.standard_normal((b, 1)).astype(np.float32), device="cuda") for b in [1024] * 9 + [784]]
zs = [torch.zeros(c.shape[0], 128, device="cuda") for c in conds]      # z is accepted and unused (Q2)
widths = [int(k) for k in args.widths.split(",")]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def med(v):
    return sorted(v)[len(v) // 2]


def kernel_split(T):
    """Device time of each launch of one bs-1024 batch: the dense pass, the lse, the Viterbi and the marginals kernels."""
    dec, cond = samp.decoder, conds[0]
    V = dec.vocab_size
    ws, B = dec.load_conditions(cond, T)
    lse = torch.empty(B * V, dtype=torch.float32, device="cuda")         # (row_lse is timed as a bare launch into this buffer)
    scratch = dec.scratch("viterbi", B, V, T)
    tok = torch.empty(B, T, dtype=torch.int32, device="cuda")
    sc = torch.empty(B, dtype=torch.float32, device="cuda")
    ln = torch.empty(B, dtype=torch.int32, device="cuda")
    alive = torch.empty(B, T, V, dtype=torch.float32, device="cuda")
    steps = {
        "dense_pass": lambda: dec.dense_table(ws),
        "row_lse": lambda: call("arcvae_dec_row_lse", ptr(ws.logits), ptr(lse), B * V, V, 1.0, stream_ptr()),
        "viterbi": lambda: call("arcvae_dec_viterbi", ptr(ws.logits), ptr(lse), ptr(tok), ptr(sc), ptr(ln), ptr(scratch),
                                scratch.numel(), B, V, T, 0, samp.end_token, samp.pad_token, 1.0, stream_ptr()),
        "chain_marginals": lambda: call("arcvae_dec_chain_marginals", ptr(ws.logits), ptr(lse), ptr(alive), B, V, T,
                                        samp.end_token, 1.0, stream_ptr()),
    }
    out = {}
    for name, fn in steps.items():
        ts = []
        for _ in range(args.reps + 1):                                   # (the first one warms up)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        out[name + "_ms"] = round(med(ts[1:]), 4)
    return out


def run(T):
    def greedy():
        return sum(samp.generate_with_temperature(z, c, max_length=T).numel() for c, z in zip(conds, zs))

    def beam(K):
        return torch.cat([samp.generate_beam(z, c, max_length=T, beam_width=K)[1][:, 0] for c, z in zip(conds, zs)])

    def exact():
        out = [samp.generate_map(z, c, max_length=T) for c, z in zip(conds, zs)]
        return torch.cat([s for _, s in out]), float(np.mean([t.shape[1] for t, _ in out]))

    def marginals():
        return sum(samp.token_marginals(c, max_length=T).shape[0] for c in conds)

    for c, z in ((conds[0], zs[0]), (conds[-1], zs[-1])):                # warm-up: both batch shapes, every method
        samp.generate_with_temperature(z, c, max_length=T)
        samp.generate_map(z, c, max_length=T)
        samp.token_marginals(c, max_length=T)
        for K in widths:
            samp.generate_beam(z, c, max_length=T, beam_width=K)
    torch.cuda.synchronize()
    times = {k: [] for k in ["greedy", "map", "marginals"] + [f"beam_{K}" for K in widths]}
    best = {}
    for _ in range(args.reps):
        times["greedy"].append(timed(greedy)[0])
        for K in widths:
            dt, best[K] = timed(lambda: beam(K))
            times[f"beam_{K}"].append(dt)
        dt, (map_sc, map_len) = timed(exact)
        times["map"].append(dt)
        times["marginals"].append(timed(marginals)[0])
    m = {k: med(v) for k, v in times.items()}
    assert all(bool((map_sc >= best[K]).all()) for K in widths), "the MAP score fell below a beam's best hypothesis"
    return {"greedy_ms_per_10k": round(1e3 * m["greedy"], 3),
            "beam_ms_per_10k": {str(K): round(1e3 * m[f"beam_{K}"], 3) for K in widths},
            "map_ms_per_10k": round(1e3 * m["map"], 3),
            "token_marginals_ms_per_10k": round(1e3 * m["marginals"], 3),
            "map_vs_beam_4": round(m["map"] / m["beam_4"], 3) if 4 in widths else None,
            "map_mean_returned_length": round(map_len, 2),
            "share_of_rows_map_strictly_above_beam": {str(K): round(float((map_sc > best[K]).float().mean()), 4) for K in widths},
            "kernels_bs1024": kernel_split(T),
            "all_ms_per_10k": {k: [round(1e3 * t, 3) for t in v] for k, v in times.items()}}


res = {"metric": "exact MAP decoding and chain marginals vs greedy and beam search, 10k molecules = 9 x bs 1024 + 784, default "
                 "AR-CVAE (random init), early stopping on, 1x MI355X, fp32; host wall time incl. the per-batch early-stop "
                 "read; kernels_bs1024 = device events around single launches",
       "reps": args.reps,
       "max_length": {str(T): run(int(T)) for T in args.max_lengths.split(",")}}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
