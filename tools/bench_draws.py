#!/usr/bin/env python3
"""N draws per condition row (generate_many, arcvae_dec_sample_draws) against today's way of getting 10 000 molecules for ONE
condition row on 1 MI355X: the default AR-CVAE (random-init weights), V 80, max_length 80 and 128, early stopping on (the API
default), everything in one process.

(a) today's way: generate_with_temperature(sample=True, top_p=0.9) over ten batches (9 x bs 1024 + 784) of the repeated row.
(b) generate_many(row, 10 000) with top_p 0.9, with no truncation, with typical_p 0.9 and with top_p 0.9 + min_length 10.
(c) the grid: 16 condition rows x 640 draws, top_p 0.9.
Protocol: every method of every repetition is run twice in a row and the second run is timed (host wall time, the early-stop read
included); median of --reps.  Next to it, between device events, the phases of (b) and (c): the dense pass; the whole
arcvae_dec_sample_draws call; the pre-pass alone, timed as arcvae_dec_sample_chain_trunc at max_len = 1 on the same table (the
same pre-pass launch and a one-step walk of B waves: the pre-pass to a few microseconds, and nothing staged in LDS); and their
difference, the walk WITH the staging of its lists.  (The draws call at N = 1, max_len = 1 is no pre-pass probe: its one workgroup
still stages the whole list image, 25 us a set at 64 threads, so subtracting it hides more staging the smaller the workgroup is.)

--variants: before anything else, fresh child processes time those phases under ARCVAE_DRAWS_WG = 64 / 128 / 256, staged and with
ARCVAE_DRAWS_LDS_CAP = 0 (the lists read through L2 instead of staged in LDS).  The variants are compared by call_ms, the whole
call: it holds everything in which they differ.
Prints one JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--max-lengths", default="80,128")
ap.add_argument("--variants", action="store_true", help="time the walk's workgroup sizes and the unstaged form in child processes")
ap.add_argument("--phases-only", action="store_true", help="(the child processes of --variants) device-event phases only")
ap.add_argument("--out", default="")
args = ap.parse_args()
lengths = [int(t) for t in args.max_lengths.split(",")]

variants = None
if args.variants:                                                    # child processes first: this one has not opened the GPU yet
    variants = {}
    for name, env in (("wg64", dict(ARCVAE_DRAWS_WG="64")), ("wg128", dict(ARCVAE_DRAWS_WG="128")),
                      ("wg256", dict(ARCVAE_DRAWS_WG="256")), ("wg64_through_L2", dict(ARCVAE_DRAWS_WG="64", ARCVAE_DRAWS_LDS_CAP="0")),
                      ("wg128_through_L2", dict(ARCVAE_DRAWS_WG="128", ARCVAE_DRAWS_LDS_CAP="0")),
                      ("wg256_through_L2", dict(ARCVAE_DRAWS_WG="256", ARCVAE_DRAWS_LDS_CAP="0"))):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-only", "--max-lengths", args.max_lengths],
                             capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        if out.returncode != 0:
            sys.exit(f"variant {name} failed ({out.returncode}):\n{out.stderr[-2000:]}")
        variants[name] = json.loads(out.stdout.strip().splitlines()[-1])["phases"]

sys.path.insert(0, os.path.join(HERE, "mlx-vae_amd"))
import torch  # noqa: E402
from arcvae_hip._lib import call, ptr, stream_ptr  # noqa: E402
from models.vae import ARCVAE  # noqa: E402

vae = ARCVAE(vocab_size=80, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
             generator=torch.Generator().manual_seed(0))
samp = vae.decoder_sampling
V, N_ALL = 80, 10000
rs = np.random.RandomState(0)
row = rs.standard_normal((1, 1)).astype(np.float32)
grid = rs.standard_normal((16, 1)).astype(np.float32)
row_d, grid_d = torch.tensor(row, device="cuda"), torch.tensor(grid, device="cuda")
repeated = [torch.tensor(np.repeat(row, b, axis=0), device="cuda") for b in [1024] * 9 + [784]]
RULES = {"top_p_0.9": dict(top_p=0.9), "no_truncation": {}, "typical_p_0.9": dict(typical_p=0.9),
         "top_p_0.9_min_length_10": dict(top_p=0.9, min_length=10)}


def today(T, seed):
    return sum(samp.generate_with_temperature(None, c, max_length=T, sample=True, top_p=0.9, seed=seed * 16 + i).shape[1]
               for i, c in enumerate(repeated)) / len(repeated)


def many(T, seed, cond, n, kw):
    return samp.generate_many(cond, n, max_length=T, seed=seed, **kw)[0].shape[2]


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


def phases(T):
    """Device-event times of one decode pass: B condition rows x n draws, per rule."""
    out = {}
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    for shape, cond, B, n in (("1x10000", row_d, 1, N_ALL), ("16x640", grid_d, 16, 640)):
        dec = samp.decoder
        ws, _ = dec.load_conditions(cond, T)
        dec.dense_table(ws)
        tok = torch.empty(B, n, T, dtype=torch.int32, device="cuda")
        fe = torch.empty(B, n, dtype=torch.int32, device="cuda")
        res = {"dense_pass_ms": round(events(lambda: dec.dense_table(ws)), 4)}
        for name, kw in RULES.items():
            k, p, mp, tp, m = samp._check_trunc(1.0, kw.get("top_k"), kw.get("top_p"), None, kw.get("typical_p"),
                                                kw.get("min_length", 0), T)
            scratch = dec.scratch("sample_draws", B, V, k, m)

            def draws(n_, T_, pad):
                call("arcvae_dec_sample_draws", ptr(ws.logits), ptr(tok), ptr(fe), ptr(scratch), scratch.numel(), B, n_, V, T_,
                     min(m, T_), 2, pad, 1.0, k, p, mp, tp, ptr(seed), stream_ptr())

            one, one_end = torch.empty(B, 1, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")

            def prepass():                                            # the same pre-pass launch, a one-step walk, no staging
                call("arcvae_dec_sample_chain_trunc", ptr(ws.logits), ptr(one), ptr(one_end), ptr(scratch), scratch.numel(), B, V, 1,
                     min(m, 1), 2, 1.0, k, p, mp, tp, ptr(seed), stream_ptr())

            r = {"call_ms": round(events(lambda: draws(n, T, 0)), 4), "call_no_pad_ms": round(events(lambda: draws(n, T, -1)), 4),
                 "prepass_ms": round(events(prepass), 4)}
            r["walk_with_staging_ms"] = round(r["call_ms"] - r["prepass_ms"], 4)
            res[name] = r
        out[shape] = res
    return out


res = {"metric": "10 000 molecules for one condition row: today's repeated-row batches vs generate_many; default AR-CVAE (random "
                 "init), V 80, early stopping on, 1x MI355X, fp32; host wall ms incl. the early-stop read, each method timed after "
                 "an untimed run of itself, median of reps; phases between device events",
       "reps": args.reps, "walk_env": {k: os.environ.get(k) for k in ("ARCVAE_DRAWS_WG", "ARCVAE_DRAWS_LDS_CAP")}, "results": {},
       "phases": {}}
if variants:
    res["walk_variants"] = variants
for T in lengths:
    if not args.phases_only:
        METHODS = {"a_today_repeated_rows_top_p_0.9": lambda s: today(T, s)}
        for name, kw in RULES.items():
            METHODS["b_generate_many_" + name] = lambda s, kw=kw: many(T, s, row_d, N_ALL, kw)
        METHODS["c_grid_16x640_top_p_0.9"] = lambda s: many(T, s, grid_d, 640, dict(top_p=0.9))
        for fn in METHODS.values():                                  # warm-up / capture
            fn(0)
        torch.cuda.synchronize()
        times = {m: [] for m in METHODS}
        mean_len = {}
        for rep in range(args.reps):
            for m, fn in METHODS.items():
                fn(rep + 1)                                          # untimed
                dt, mean_len[m] = timed(lambda: fn(rep + 1))
                times[m].append(dt)
        med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
        base = med["a_today_repeated_rows_top_p_0.9"]
        n_of = lambda m: 16 * 640 if m.startswith("c_") else N_ALL   # noqa: E731
        res["results"][f"max_length={T}"] = {
            m: {"ms": round(1e3 * med[m], 3), "molecules": n_of(m), "ms_per_10k": round(1e3 * med[m] * N_ALL / n_of(m), 3),
                "vs_today": round(med[m] * N_ALL / n_of(m) / base, 4), "returned_length": round(float(mean_len[m]), 2),
                "ms_all": [round(1e3 * t, 3) for t in times[m]]} for m in METHODS}
    res["phases"][f"max_length={T}"] = phases(T)
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
