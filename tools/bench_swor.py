#!/usr/bin/env python3
"""Sampling without replacement at BASELINE.json configs[4]'s shape on 1 MI355X: 10 000 rows as 9 x bs 1024 + 784, the default
AR-CVAE (random-init weights), max_length 80, early stopping on (the API default) -- generate_without_replacement at K = 4 and
16 next to generate_beam at the same widths and to K calls of sample=True, in the same process, every method once per
repetition, median of --reps.

One generate_without_replacement batch = the replay of the captured pass (dense decoder pass over B*V rows, arcvae_dec_row_lse,
arcvae_dec_swor), the seed written into its device word before the replay, plus the host read of the lengths for early stopping
and the copies of the outputs.  Also reported: the kernel alone on one bs-1024 batch from device events around single launches,
and THE POINT OF THE FEATURE: on a peaked ("trained-like") table -- the same decoder with fc_out scaled by --sharpen, which is
what training does to it (several factors) -- the mean number of DISTINCT sequences among K sample=True draws per row, next to K (which
generate_without_replacement returns by construction: asserted), and the mean probability mass the K distinct sequences cover.
Prints one JSON line (and writes it to --out when given)."""
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
ap.add_argument("--max-length", type=int, default=80)
ap.add_argument("--sharpen", default="6,12,24")
ap.add_argument("--out", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_swor.py measures on a GPU: there is no CPU path"

vae = ARCVAE(vocab_size=80, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
             generator=torch.Generator().manual_seed(0))
samp = vae.decoder_sampling
V, T = 80, args.max_length
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


def swor(K, seed):
    return [samp.generate_without_replacement(z, c, max_length=T, num_samples=K, seed=seed * 16 + i)[0].shape[2]
            for i, (c, z) in enumerate(zip(conds, zs))]


def beam(K):
    return [samp.generate_beam(z, c, max_length=T, beam_width=K)[0].shape[2] for c, z in zip(conds, zs)]


def repeated(K, seed):
    return [samp.generate_with_temperature(z, c, max_length=T, sample=True, seed=(seed * 16 + i) * 64 + k).shape[1]
            for i, (c, z) in enumerate(zip(conds, zs)) for k in range(K)]


def kernel_alone():
    """Device time of arcvae_dec_swor (and arcvae_dec_beam_search) alone on one bs-1024 batch, per K: the dense pass and the lse
    are made once before."""
    dec, cond = samp.decoder, conds[0]
    ws, B = dec.load_conditions(cond, T)
    dec.dense_table(ws)
    lse = dec.table_lse(ws, 1.0)
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = {}
    for K in widths:
        tok = torch.empty(B, K, T, dtype=torch.int32, device="cuda")
        sc, G = torch.empty(B, K, dtype=torch.float32, device="cuda"), torch.empty(B, K, dtype=torch.float32, device="cuda")
        ln = torch.empty(B, K, dtype=torch.int32, device="cuda")
        thr = torch.empty(B, dtype=torch.float32, device="cuda")
        s_ws, b_ws = dec.scratch("swor", B, K, T), dec.scratch("beam", B, K, T)
        launches = {
            "swor_kernel_ms": lambda: call("arcvae_dec_swor", ptr(ws.logits), ptr(lse), ptr(seed), ptr(tok), ptr(sc), ptr(G), ptr(ln),
                                           ptr(thr), ptr(s_ws), s_ws.numel(), B, V, K, T, samp.end_token, samp.pad_token, 1.0,
                                           stream_ptr()),
            "beam_kernels_ms": lambda: call("arcvae_dec_beam_search", ptr(ws.logits), ptr(lse), ptr(tok), ptr(sc), ptr(ln), ptr(b_ws),
                                            b_ws.numel(), B, V, K, T, 0, samp.end_token, samp.pad_token, 1.0, stream_ptr())}
        out[str(K)] = {}
        for name, fn in launches.items():
            ts = []
            for _ in range(args.reps + 1):                                   # (the first one warms up)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
            out[str(K)][name] = round(med(ts[1:]), 4)
    return out


def distinct_on_a_peaked_table(sharpen):
    """fc_out scaled by `sharpen` (a peaked next-token distribution, as after training; the end token's bias raised so that
    sequences end): per row, the number of distinct sequences among K sample=True draws (compared up to the first end_token),
    next to generate_without_replacement's K, on one bs-1024 batch."""
    dec, cond, z = samp.decoder, conds[0], zs[0]
    saved = dec.store.flat.clone()
    dec.store.p("fc_out.weight").mul_(sharpen)
    dec.store.p("fc_out.bias")[samp.end_token] += 2.0
    out = {}
    try:
        for K in widths:
            draws = np.stack([samp.generate_with_temperature(z, cond, max_length=T, early_stopping=False, sample=True,
                                                             seed=1000 + k).cpu().numpy() for k in range(K)], axis=1)   # [B, K, T]
            ended = np.cumsum(draws == samp.end_token, axis=2) - (draws == samp.end_token) > 0
            draws = np.where(ended, samp.pad_token, draws)               # (sample=True keeps generating after the end token)
            distinct = np.array([len({tuple(s) for s in row}) for row in draws])
            tok, lp, _, _ = samp.generate_without_replacement(z, cond, max_length=T, num_samples=K, seed=1000, early_stopping=False)
            tok, lp = tok.cpu().numpy(), lp.double().cpu().numpy()
            ours = np.array([len({tuple(s) for s in row}) for row in tok])
            assert np.all(ours == K), "generate_without_replacement returned a duplicate"
            top1 = samp.generate_map(z, cond, max_length=T)[1].double().exp().mean().item()
            out[str(K)] = {"distinct_among_K_sample_true_draws_mean": round(float(distinct.mean()), 3),
                           "distinct_among_K_sample_true_draws_min": int(distinct.min()),
                           "distinct_without_replacement": K,
                           "mass_covered_by_the_K_distinct_mean": round(float(np.exp(lp).sum(1).mean()), 4),
                           "most_probable_sequence_mass_mean": round(top1, 4)}
    finally:
        dec.store.flat.copy_(saved)
    return out


for c, z in ((conds[0], zs[0]), (conds[-1], zs[-1])):                # warm-up / capture: both batch shapes, every method
    samp.generate_with_temperature(z, c, max_length=T, sample=True)
    for K in widths:
        samp.generate_beam(z, c, max_length=T, beam_width=K)
        samp.generate_without_replacement(z, c, max_length=T, num_samples=K)
        samp.generate_without_replacement(z, c, max_length=T, num_samples=K, seed=1)     # (the first replay)
torch.cuda.synchronize()
names = [f"{m}_{K}" for K in widths for m in ("swor", "beam", "sample_x")]
times = {n: [] for n in names}
for rep in range(args.reps):
    for K in widths:
        times[f"swor_{K}"].append(timed(lambda: swor(K, rep))[0])
        times[f"beam_{K}"].append(timed(lambda: beam(K))[0])
        times[f"sample_x_{K}"].append(timed(lambda: repeated(K, rep))[0])
m = {n: med(v) for n, v in times.items()}
res = {"metric": "sampling without replacement (K distinct sequences per row) vs beam search at the same width and K calls of "
                 "sample=True, 10k rows = 9 x bs 1024 + 784, default AR-CVAE (random init), max_length %d, early stopping on, "
                 "1x MI355X, fp32; host wall time incl. the per-batch early-stop read, median of reps; kernel_alone_bs1024 = "
                 "device events around single launches; peaked_table = fc_out x the factor given, bs 1024" % T,
       "reps": args.reps, "max_length": T,
       "swor_ms_per_10k": {str(K): round(1e3 * m[f"swor_{K}"], 3) for K in widths},
       "beam_ms_per_10k": {str(K): round(1e3 * m[f"beam_{K}"], 3) for K in widths},
       "K_calls_of_sample_true_ms_per_10k": {str(K): round(1e3 * m[f"sample_x_{K}"], 3) for K in widths},
       "swor_vs_beam": {str(K): round(m[f"swor_{K}"] / m[f"beam_{K}"], 3) for K in widths},
       "swor_vs_K_calls_of_sample_true": {str(K): round(m[f"swor_{K}"] / m[f"sample_x_{K}"], 3) for K in widths},
       "kernel_alone_bs1024": kernel_alone(),
       "peaked_table": {f"fc_out_x_{f:g}": distinct_on_a_peaked_table(f) for f in (float(x) for x in args.sharpen.split(","))},
       "all_ms_per_10k": {n: [round(1e3 * t, 3) for t in v] for n, v in times.items()}}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
