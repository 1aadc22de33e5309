#!/usr/bin/env python3
"""Top-k / nucleus sampling at BASELINE.json configs[4]'s shape on 1 MI355X: 10 000 molecules as 9 x bs 1024 + 784, the default
AR-CVAE (random-init weights), max_length 80 and 128, early stopping on (the API default) -- greedy, sample=True, top_k=20,
top_p=0.9 and both, in the same process, the five alternating per repetition.

One truncated batch = the captured dense decoder pass (mode 0) + arcvae_dec_sample_chain_topkp, the seed written into its
device word before the replay, plus the host read of first_end for early stopping.  Next to it, by device events on one bs-1024
table: one arcvae_dec_sample_chain_topkp call (pre-pass over all B * V rows + walk) and the inspection kernel over the same rows.
Prints one JSON line (and writes it to --out when given).  Per-kernel times: a separate profiler run with --reps 1."""
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
ap.add_argument("--max-lengths", default="80,128")
ap.add_argument("--out", default="")
args = ap.parse_args()

vae = ARCVAE(vocab_size=80, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
             generator=torch.Generator().manual_seed(0))
samp = vae.decoder_sampling
V = 80
rs = np.random.RandomState(0)
conds = [torch.tensor(rs.standard_normal((b, 1)).astype(np.float32), device="cuda") for b in [1024] * 9 + [784]]
zs = [torch.zeros(c.shape[0], 128, device="cuda") for c in conds]      # z is accepted and unused (Q2)
MODES = {"greedy": {}, "sample": dict(sample=True), "top_k_20": dict(sample=True, top_k=20),
         "top_p_0.9": dict(sample=True, top_p=0.9), "top_k_20_top_p_0.9": dict(sample=True, top_k=20, top_p=0.9)}


def run(T, kw, seed):
    n = 0
    for i, (c, z) in enumerate(zip(conds, zs)):
        extra = dict(seed=seed * 16 + i) if kw else {}
        n += samp.generate_with_temperature(z, c, max_length=T, **kw, **extra).shape[1]
    return n / len(conds)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def events(fn, n=20):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


res = {"metric": "top-k / nucleus sampling vs greedy and sample=True, 10k molecules = 9 x bs 1024 + 784, default AR-CVAE (random "
                 "init), early stopping on, 1x MI355X, fp32; host wall time incl. the per-batch early-stop read; median of reps",
       "reps": args.reps, "results": {}, "kernels": {}}
for T in [int(t) for t in args.max_lengths.split(",")]:
    for c, z in ((conds[0], zs[0]), (conds[-1], zs[-1])):             # warm-up / capture: both batch shapes, every mode
        for kw in MODES.values():
            samp.generate_with_temperature(z, c, max_length=T, **kw)
    torch.cuda.synchronize()
    times = {m: [] for m in MODES}
    mean_len = {}
    for rep in range(args.reps):
        for m, kw in MODES.items():
            dt, mean_len[m] = timed(lambda: run(T, kw, rep))
            times[m].append(dt)
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    res["results"][f"max_length={T}"] = {
        m: {"ms_per_10k": round(1e3 * med[m], 3), "vs_greedy": round(med[m] / med["greedy"], 3),
            "mean_returned_length": round(mean_len[m], 2), "ms_per_10k_all": [round(1e3 * t, 3) for t in times[m]]} for m in MODES}
    # the truncated path's own kernels by device events on one bs-1024 table: the pre-pass over all B * V rows and the walk
    # (pre-pass + walk = one arcvae_dec_sample_chain_topkp call), next to the inspection kernel over the same rows
    B = 1024
    samp.generate_with_temperature(zs[0], conds[0], max_length=T, sample=True, top_k=20)
    table = samp.decoder.workspace(B, T).logits
    tok = torch.empty(B, T, dtype=torch.int32, device="cuda")
    fe = torch.empty(B, dtype=torch.int32, device="cuda")
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    cnt = torch.empty(B * V, dtype=torch.int32, device="cuda")
    rtok = torch.empty(B * V, V, dtype=torch.int32, device="cuda")
    rcum = torch.empty(B * V, V, dtype=torch.float32, device="cuda")
    pl = {}
    for name, k, p in (("top_k_20", 20, 1.0), ("top_p_0.9", 0, 0.9), ("top_k_20_top_p_0.9", 20, 0.9)):
        ws = samp.decoder.scratch("topkp", B, V, k)
        chain = events(lambda: call("arcvae_dec_sample_chain_topkp", ptr(table), ptr(tok), ptr(fe), ptr(ws), ws.numel(), B, V, T, 2,
                                    1.0, k, p, ptr(seed), stream_ptr()))
        rows = events(lambda: call("arcvae_dec_topkp_rows", ptr(table), B * V, None, B * V, V, 1.0, k, p, ptr(cnt), ptr(rtok),
                                   ptr(rcum), stream_ptr()))
        pl[name] = {"prepass_plus_walk_ms_per_batch": round(chain, 4), "inspect_all_rows_ms_per_batch": round(rows, 4),
                    "workspace_MB": round(ws.numel() / 1e6, 2)}
    res["kernels"][f"max_length={T}"] = pl
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
