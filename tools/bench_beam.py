#!/usr/bin/env python3
"""Beam search at BASELINE.json configs[4]'s shape on 1 MI355X: 10 000 molecules as 9 x bs 1024 + 784, the default AR-CVAE
(random-init weights), max_length 80, early stopping on (the API default), widths K = 1, 4, 8, 16, 32 -- next to the greedy
sampler (captured decode pass) in the same process, alternating the two per repetition.

One beam batch = the dense decoder pass over B*V rows + arcvae_dec_row_lse + the pre-pass and the walk of
arcvae_dec_beam_search, launched eagerly, plus the host read of the lengths for early stopping.  Prints one JSON line (and
writes it to --out when given).  The per-kernel split comes from a separate profiler run of this script with --reps 1."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlx-vae_amd"))
import torch  # noqa: E402
from models.vae import ARCVAE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--widths", default="1,4,8,16,32")
ap.add_argument("--max-length", type=int, default=80)
ap.add_argument("--out", default="")
args = ap.parse_args()

vae = ARCVAE(vocab_size=80, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
             generator=torch.Generator().manual_seed(0))
samp = vae.decoder_sampling
rs = np.random.RandomState(0)
conds = [torch.tensor(rs.standard_normal((b, 1)).astype(np.float32), device="cuda") for b in [1024] * 9 + [784]]
zs = [torch.zeros(c.shape[0], 128, device="cuda") for c in conds]      # z is accepted and unused (Q2)
T = args.max_length
widths = [int(k) for k in args.widths.split(",")]


def greedy():
    return sum(samp.generate_with_temperature(z, c, max_length=T).numel() for c, z in zip(conds, zs))


def beam(K):
    n = 0
    for c, z in zip(conds, zs):
        tok, _ = samp.generate_beam(z, c, max_length=T, beam_width=K)
        n += tok.shape[2]
    return n / len(conds)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


for c, z in ((conds[0], zs[0]), (conds[-1], zs[-1])):                 # warm-up: both batch shapes, every width
    samp.generate_with_temperature(z, c, max_length=T)
    for K in widths:
        samp.generate_beam(z, c, max_length=T, beam_width=K)
torch.cuda.synchronize()
times = {"greedy": []}
mean_len = {}
for K in widths:
    times[f"beam_{K}"] = []
for _ in range(args.reps):
    for K in widths:                                                   # greedy and each width alternate
        times["greedy"].append(timed(greedy)[0])
        dt, mean_len[K] = timed(lambda: beam(K))
        times[f"beam_{K}"].append(dt)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
res = {"metric": "beam search vs greedy, 10k molecules = 9 x bs 1024 + 784, default AR-CVAE (random init), max_length "
                 f"{T}, early stopping on, 1x MI355X, fp32; host wall time incl. the per-batch early-stop read",
       "greedy_ms_per_10k": round(1e3 * med["greedy"], 3),
       "beam": {str(K): {"ms_per_10k": round(1e3 * med[f"beam_{K}"], 3),
                         "vs_greedy": round(med[f"beam_{K}"] / med["greedy"], 3),
                         "mean_returned_length": round(mean_len[K], 2),
                         "ms_per_10k_all": [round(1e3 * t, 3) for t in times[f"beam_{K}"]]} for K in widths},
       "greedy_ms_per_10k_all": [round(1e3 * t, 3) for t in times["greedy"]],
       "reps": args.reps}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
