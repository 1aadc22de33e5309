#!/usr/bin/env python3
"""Exact K-best decoding at BASELINE.json configs[4]'s shape on 1 MI355X: 10 000 molecules as 9 x bs 1024 + 784, the default
AR-CVAE (random-init weights), max_length 80 and 128, early stopping on (the API default) -- generate_kbest at K = 4 and 16 next
to generate_beam at the same widths and generate_map in the same process, every method once per repetition, median of --reps.

One generate_kbest batch = the dense decoder pass over B*V rows + arcvae_dec_row_lse + arcvae_dec_kbest, launched eagerly, plus the
host read of the lengths for early stopping.  Also reported: the share of the 10 000 rows in which some rank of the exact list is
strictly above the beam's at the same K (none is ever below: asserted), the mean probability mass exp(scores).sum(1) the list
covers, and the kernel alone on one bs-1024 batch from device events around single launches (median of --reps).  Prints one JSON
line (and writes it to --out when given)."""
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--widths", default="4,16")
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


def kernel_alone(T):
    """Device time of arcvae_dec_kbest alone on one bs-1024 batch, per K (the dense pass and the lse are made once before)."""
    dec, cond = samp.decoder, conds[0]
    V = dec.vocab_size
    ws, B = dec.load_conditions(cond, T)
    dec.dense_table(ws)
    lse = dec.table_lse(ws, 1.0)
    out = {}
    for K in widths:
        scratch = dec.scratch("kbest", B, V, K, T)
        tok = torch.empty(B, K, T, dtype=torch.int32, device="cuda")
        sc = torch.empty(B, K, dtype=torch.float32, device="cuda")
        ln = torch.empty(B, K, dtype=torch.int32, device="cuda")
        ts = []
        for _ in range(args.reps + 1):                                   # (the first one warms up)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            call("arcvae_dec_kbest", ptr(ws.logits), ptr(lse), ptr(tok), ptr(sc), ptr(ln), ptr(scratch), scratch.numel(), B, V, K, T,
                 0, samp.end_token, samp.pad_token, 1.0, stream_ptr())
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        out[str(K)] = {"kbest_kernel_ms": round(med(ts[1:]), 4), "scratch_mb": round(scratch.numel() / 2 ** 20, 1)}
    return out


def run(T):
    def beam(K):
        return torch.cat([samp.generate_beam(z, c, max_length=T, beam_width=K)[1] for c, z in zip(conds, zs)])

    def kbest(K):
        return torch.cat([samp.generate_kbest(z, c, max_length=T, num_best=K)[1] for c, z in zip(conds, zs)])

    def exact():
        return torch.cat([samp.generate_map(z, c, max_length=T)[1] for c, z in zip(conds, zs)])

    for c, z in ((conds[0], zs[0]), (conds[-1], zs[-1])):                # warm-up: both batch shapes, every method
        samp.generate_map(z, c, max_length=T)
        for K in widths:
            samp.generate_beam(z, c, max_length=T, beam_width=K)
            samp.generate_kbest(z, c, max_length=T, num_best=K)
    torch.cuda.synchronize()
    times = {k: [] for k in ["map"] + [f"beam_{K}" for K in widths] + [f"kbest_{K}" for K in widths]}
    bsc, ksc = {}, {}
    for _ in range(args.reps):
        dt, msc = timed(exact)
        times["map"].append(dt)
        for K in widths:
            dt, bsc[K] = timed(lambda: beam(K))
            times[f"beam_{K}"].append(dt)
            dt, ksc[K] = timed(lambda: kbest(K))
            times[f"kbest_{K}"].append(dt)
    m = {k: med(v) for k, v in times.items()}
    for K in widths:
        assert bool((ksc[K] >= bsc[K]).all()), "a rank of the exact list fell below the beam's"
        assert bool((ksc[K][:, 0] == msc).all()), "rank 0 is not the MAP score"
    return {"map_ms_per_10k": round(1e3 * m["map"], 3),
            "beam_ms_per_10k": {str(K): round(1e3 * m[f"beam_{K}"], 3) for K in widths},
            "kbest_ms_per_10k": {str(K): round(1e3 * m[f"kbest_{K}"], 3) for K in widths},
            "kbest_vs_beam": {str(K): round(m[f"kbest_{K}"] / m[f"beam_{K}"], 3) for K in widths},
            "share_of_rows_with_a_rank_strictly_above_the_beam": {str(K): round(float((ksc[K] > bsc[K]).any(1).float().mean()), 4)
                                                                  for K in widths},
            "mean_mass_covered": {str(K): float(ksc[K].double().exp().sum(1).mean()) for K in widths},
            "kernel_alone_bs1024": kernel_alone(T),
            "all_ms_per_10k": {k: [round(1e3 * t, 3) for t in v] for k, v in times.items()}}


res = {"metric": "exact K-best decoding vs beam search at the same width and exact MAP, 10k molecules = 9 x bs 1024 + 784, default "
                 "AR-CVAE (random init), early stopping on, 1x MI355X, fp32; host wall time incl. the per-batch early-stop "
                 "read; kernel_alone_bs1024 = device events around single launches",
       "reps": args.reps,
       "max_length": {str(T): run(int(T)) for T in args.max_lengths.split(",")}}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
