#!/usr/bin/env python3
"""Min-p, locally typical and minimum-length sampling at BASELINE.json configs[4]'s shape on 1 MI355X: 10 000 molecules as
9 x bs 1024 + 784, the default AR-CVAE (random-init weights), V 80, max_length 80 and 128, early stopping on (the API default) --
greedy, sample=True, top_p 0.9, min_p 0.05, typical_p 0.9, typical_p 0.9 with top_k 20, top_p 0.9 with min_length 10, in one
process.  Protocol: every method of every repetition is run twice in a row and the second run is timed (each method is timed after
an untimed run of itself); median of --reps.

One truncated batch = the captured dense decoder pass (mode 0) + arcvae_dec_sample_chain_trunc (or _topkp), the seed written into
its device word before the replay, plus the host read of first_end for early stopping.  Next to it, between device events on one
bs-1024 table: one whole call (pre-pass + walk) per rule, the same call at max_len = 1 (the pre-pass and a one-step walk: the
pre-pass alone, to a few microseconds) and their difference (the walk alone).

--root DIR imports the package from another checkout of this repository (a build of the parent commit, which has none of the new
entry points: only greedy, sample=True, top_p 0.9 and the arcvae_dec_sample_chain_topkp call are then timed).
--ab DIR runs that A/B in the same session before anything else: --ab-runs times in turn a fresh child process on DIR and one on
this tree (which of the two goes first alternates), each timing only the existing call; reported per run, with the spread between
the runs of one build next to the difference between the builds.  Prints one JSON line (and writes it to --out when given)."""
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
ap.add_argument("--root", default=HERE)
ap.add_argument("--existing-only", action="store_true", help="time only what the parent commit has (implied by an older --root)")
ap.add_argument("--ab", default="", help="a built checkout of the parent commit: A/B of the existing top-k / top-p call first")
ap.add_argument("--ab-runs", type=int, default=2)
ap.add_argument("--out", default="")
args = ap.parse_args()
lengths = [int(t) for t in args.max_lengths.split(",")]

ab = None
if args.ab:                                                          # child processes first: this one has not opened the GPU yet
    runs = {"parent": [], "this": []}
    for i in range(args.ab_runs):
        for name, root in (("parent", os.path.abspath(args.ab)), ("this", HERE))[::-1 if i % 2 else 1]:   # who goes first alternates
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--existing-only", "--reps",
                                  str(args.reps), "--max-lengths", args.max_lengths], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                sys.exit(f"A/B child on {root} failed ({out.returncode}):\n{out.stderr[-2000:]}")
            runs[name].append(json.loads(out.stdout.strip().splitlines()[-1]))
    ab = {"what": "arcvae_dec_sample_chain_topkp (top_p 0.9) on one bs-1024 table, ms per call between device events, and top_p 0.9 "
                  "per 10k molecules (host wall ms); fresh processes, parent and this tree in turn", "runs": args.ab_runs}
    for T in lengths:
        row = {}
        for key, pick in (("chain_topkp_ms", lambda r: r["kernels"][f"max_length={T}"]["top_p_0.9"]["chain_ms"]),
                          ("top_p_0.9_ms_per_10k", lambda r: r["results"][f"max_length={T}"]["top_p_0.9"]["ms_per_10k"])):
            a, b = [pick(r) for r in runs["parent"]], [pick(r) for r in runs["this"]]
            row[key] = {"parent": a, "this": b, "spread_parent": round(max(a) - min(a), 4), "spread_this": round(max(b) - min(b), 4),
                        "this_minus_parent_of_means": round(sum(b) / len(b) - sum(a) / len(a), 4)}
        ab[f"max_length={T}"] = row

sys.path.insert(0, os.path.join(os.path.abspath(args.root), "mlx-vae_amd"))
import torch  # noqa: E402
from arcvae_hip import _lib  # noqa: E402
from arcvae_hip._lib import call, ptr, stream_ptr  # noqa: E402
from models.vae import ARCVAE  # noqa: E402

NEW = "arcvae_dec_sample_chain_trunc" in _lib.SIGNATURES and not args.existing_only
vae = ARCVAE(vocab_size=80, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
             generator=torch.Generator().manual_seed(0))
samp = vae.decoder_sampling
V = 80
rs = np.random.RandomState(0)
conds = [torch.tensor(rs.standard_normal((b, 1)).astype(np.float32), device="cuda") for b in [1024] * 9 + [784]]
zs = [torch.zeros(c.shape[0], 128, device="cuda") for c in conds]      # z is accepted and unused (Q2)
MODES = {"greedy": {}, "sample": dict(sample=True), "top_p_0.9": dict(sample=True, top_p=0.9)}
if NEW:
    MODES.update({"min_p_0.05": dict(sample=True, min_p=0.05), "typical_p_0.9": dict(sample=True, typical_p=0.9),
                  "typical_p_0.9_top_k_20": dict(sample=True, typical_p=0.9, top_k=20),
                  "top_p_0.9_min_length_10": dict(sample=True, top_p=0.9, min_length=10)})


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


res = {"metric": "min-p / typical / min-length sampling vs greedy, sample=True and top_p, 10k molecules = 9 x bs 1024 + 784, default "
                 "AR-CVAE (random init), early stopping on, 1x MI355X, fp32; host wall time incl. the per-batch early-stop read; each "
                 "method timed after an untimed run of itself; median of reps",
       "reps": args.reps, "new_entry_points": NEW, "results": {}, "kernels": {}}
if ab:
    res["ab_existing_call"] = ab
for T in lengths:
    for c, z in ((conds[0], zs[0]), (conds[-1], zs[-1])):             # warm-up / capture: both batch shapes, every mode
        for kw in MODES.values():
            samp.generate_with_temperature(z, c, max_length=T, **kw)
    torch.cuda.synchronize()
    times = {m: [] for m in MODES}
    mean_len = {}
    for rep in range(args.reps):
        for m, kw in MODES.items():
            run(T, kw, rep)                                           # untimed
            dt, mean_len[m] = timed(lambda: run(T, kw, rep))
            times[m].append(dt)
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    res["results"][f"max_length={T}"] = {
        m: {"ms_per_10k": round(1e3 * med[m], 3), "vs_greedy": round(med[m] / med["greedy"], 3),
            "mean_returned_length": round(mean_len[m], 2), "ms_per_10k_all": [round(1e3 * t, 3) for t in times[m]]} for m in MODES}
    # the truncated paths' own kernels between device events on one bs-1024 table: a whole call, and the call at max_len = 1
    B = 1024
    samp.generate_with_temperature(zs[0], conds[0], max_length=T, sample=True, top_p=0.9)
    table = samp.decoder.workspace(B, T).logits
    tok = torch.empty(B, T, dtype=torch.int32, device="cuda")
    fe = torch.empty(B, dtype=torch.int32, device="cuda")
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    pl = {}
    ws = samp.decoder.scratch("topkp", B, V, 0)
    pl["top_p_0.9"] = {"entry_point": "arcvae_dec_sample_chain_topkp", "workspace_MB": round(ws.numel() / 1e6, 2)}
    for name, L in (("chain_ms", T), ("chain_max_len_1_ms", 1)):
        pl["top_p_0.9"][name] = round(events(lambda: call("arcvae_dec_sample_chain_topkp", ptr(table), ptr(tok), ptr(fe), ptr(ws),
                                                          ws.numel(), B, V, L, 2, 1.0, 0, 0.9, ptr(seed), stream_ptr())), 4)
    if NEW:
        for name, k, p, mp, tp, m in (("top_p_0.9_via_trunc", 0, 0.9, 0.0, 1.0, 0), ("min_p_0.05", 0, 1.0, 0.05, 1.0, 0),
                                      ("typical_p_0.9", 0, 1.0, 0.0, 0.9, 0), ("typical_p_0.9_top_k_20", 20, 1.0, 0.0, 0.9, 0),
                                      ("top_p_0.9_min_length_10", 0, 0.9, 0.0, 1.0, 10)):
            ws = samp.decoder.scratch("trunc", B, V, k, m)
            pl[name] = {"entry_point": "arcvae_dec_sample_chain_trunc", "workspace_MB": round(ws.numel() / 1e6, 2)}
            for key, L in (("chain_ms", T), ("chain_max_len_1_ms", 1)):
                pl[name][key] = round(events(lambda: call("arcvae_dec_sample_chain_trunc", ptr(table), ptr(tok), ptr(fe), ptr(ws),
                                                          ws.numel(), B, V, L, min(m, L), 2, 1.0, k, p, mp, tp, ptr(seed),
                                                          stream_ptr())), 4)
    for v in pl.values():
        v["walk_ms"] = round(v["chain_ms"] - v["chain_max_len_1_ms"], 4)
    res["kernels"][f"max_length={T}"] = pl
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
