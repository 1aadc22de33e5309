#!/usr/bin/env python3
"""Length-normalised exact decoding and the per-length profile at BASELINE.json configs[4]'s shape on 1 MI355X: 10 000 molecules
as 9 x bs 1024 + 784, the default AR-CVAE (random-init weights), max_length 80 and 128, early stopping on (the API default) --
generate_map and generate_kbest (K = 4, 16) without a penalty and with length_penalty = --alpha, best_by_length and
generate_of_length (every row at max_length // 2), every method in every repetition in the same process (run twice in a row,
the second run timed: timed once each in turn, whichever method came after generate_kbest at K 16 measured about 0.3 ms per
10 k slower than in any other position -- cause not examined), median of --reps.

The yardstick of every normalised call is the un-normalised one of the same run.  Also reported: device-event times of the single
launches on one bs-1024 batch -- arcvae_dec_viterbi against arcvae_dec_viterbi_norm without and with the profile outputs,
arcvae_dec_kbest against arcvae_dec_kbest_norm, and arcvae_dec_viterbi_trace -- and the lengths the penalty chooses.

--root DIR imports the package from another checkout of this repository (a build of the parent commit, which has none of the new
entry points: only the existing methods and kernels are then timed, for an A/B of those against this tree).  Prints one JSON line
(and writes it to --out when given)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--widths", default="4,16")
ap.add_argument("--max-lengths", default="80,128")
ap.add_argument("--alpha", type=float, default=0.5)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default="")
args = ap.parse_args()

sys.path.insert(0, os.path.join(os.path.abspath(args.root), "mlx-vae_amd"))
import torch  # noqa: E402
from arcvae_hip import _lib  # noqa: E402
from arcvae_hip._lib import call, ptr, stream_ptr  # noqa: E402
from models.vae import ARCVAE  # noqa: E402

NEW = "arcvae_dec_viterbi_norm" in _lib.SIGNATURES                       # (False for a --root that predates this tool)
vae = ARCVAE(vocab_size=80, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
             generator=torch.Generator().manual_seed(0))
samp = vae.decoder_sampling
rs = np.random.RandomState(0)
conds = [torch.tensor(rs.standard_normal((b, 1)).astype(np.float32), device="cuda") for b in [1024] * 9 + [784]]
widths = [int(k) for k in args.widths.split(",")]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def med(v):
    return sorted(v)[len(v) // 2]


def kernels(T):
    """Device time of single launches on one bs-1024 batch (the dense pass and the lse are made once before)."""
    dec, cond = samp.decoder, conds[0]
    V = dec.vocab_size
    ws, B = dec.load_conditions(cond, T)
    dec.dense_table(ws)
    lse = dec.table_lse(ws, 1.0)
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    tok, sc, raw, ln = torch.empty(B, T, **i32), torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, **i32)
    byl, op = torch.empty(B, T, **f32), torch.empty(B, **f32)
    div = torch.as_tensor(np.array([float(n) ** args.alpha for n in range(1, T + 1)]).astype(np.float32), device="cuda")
    want = torch.full((B,), T // 2, **i32)
    vws = dec.scratch("viterbi", B, V, T)
    tail = (B, V, T, 0, samp.end_token, samp.pad_token, 1.0, stream_ptr())
    steps = {"viterbi": lambda: call("arcvae_dec_viterbi", ptr(ws.logits), ptr(lse), ptr(tok), ptr(sc), ptr(ln), ptr(vws),
                                     vws.numel(), *tail)}
    if NEW:
        def vnorm(profile):
            call("arcvae_dec_viterbi_norm", ptr(ws.logits), ptr(lse), ptr(div), ptr(tok), ptr(sc), ptr(raw), ptr(ln),
                 ptr(byl) if profile else None, ptr(op) if profile else None, ptr(vws), vws.numel(), *tail)
        steps["viterbi_norm"] = lambda: vnorm(False)
        steps["viterbi_norm_profile"] = lambda: vnorm(True)
        steps["viterbi_trace"] = lambda: call("arcvae_dec_viterbi_trace", ptr(vws), vws.numel(), ptr(want), ptr(tok), B, V, T,
                                              samp.end_token, samp.pad_token, stream_ptr())
    keep = []
    for K in widths:
        kws = dec.scratch("kbest", B, V, K, T)
        ktok, ksc, kraw, kln = torch.empty(B, K, T, **i32), torch.empty(B, K, **f32), torch.empty(B, K, **f32), torch.empty(B, K, **i32)
        keep.append((kws, ktok, ksc, kraw, kln))
        ktail = (B, V, K, T, 0, samp.end_token, samp.pad_token, 1.0, stream_ptr())
        steps[f"kbest_{K}"] = lambda a=keep[-1], kt=ktail: call("arcvae_dec_kbest", ptr(ws.logits), ptr(lse), ptr(a[1]), ptr(a[2]),
                                                                ptr(a[4]), ptr(a[0]), a[0].numel(), *kt)
        if NEW:
            steps[f"kbest_norm_{K}"] = lambda a=keep[-1], kt=ktail: call("arcvae_dec_kbest_norm", ptr(ws.logits), ptr(lse), ptr(div),
                                                                         ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(a[4]), ptr(a[0]),
                                                                         a[0].numel(), *kt)
    ts = {name: [] for name in steps}
    for _ in range(args.reps + 1):                                       # (the first round warms up; the launches alternate)
        for name, fn in steps.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[name].append(a.elapsed_time(b))
    return {"median_ms": {k: round(med(v[1:]), 4) for k, v in ts.items()},
            "all_ms": {k: [round(t, 4) for t in v[1:]] for k, v in ts.items()}}


def run(T):
    def over(fn):
        return [fn(c) for c in conds]

    methods = {"map": lambda: over(lambda c: samp.generate_map(None, c, max_length=T))}
    for K in widths:
        methods[f"kbest_{K}"] = lambda K=K: over(lambda c: samp.generate_kbest(None, c, max_length=T, num_best=K))
    if NEW:
        methods["map_norm"] = lambda: over(lambda c: samp.generate_map(None, c, max_length=T, length_penalty=args.alpha))
        for K in widths:
            methods[f"kbest_norm_{K}"] = lambda K=K: over(lambda c: samp.generate_kbest(None, c, max_length=T, num_best=K,
                                                                                       length_penalty=args.alpha))
        methods["best_by_length"] = lambda: over(lambda c: samp.best_by_length(c, max_length=T))
        methods["generate_of_length"] = lambda: over(lambda c: samp.generate_of_length(c, T // 2, max_length=T))
    for fn in methods.values():                                          # warm-up: both batch shapes, every method
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in methods}
    last = {}
    for _ in range(args.reps):
        for k, fn in methods.items():
            fn()                                                         # untimed: every timed run follows a run of itself
            dt, last[k] = timed(fn)
            times[k].append(dt)
    m = {k: med(v) for k, v in times.items()}
    out = {"ms_per_10k": {k: round(1e3 * v, 3) for k, v in m.items()},
           "all_ms_per_10k": {k: [round(1e3 * t, 3) for t in v] for k, v in times.items()},
           "kernels_bs1024": kernels(T)}
    if NEW:
        out["norm_vs_plain"] = {"map": round(m["map_norm"] / m["map"], 3),
                                **{f"kbest_{K}": round(m[f"kbest_norm_{K}"] / m[f"kbest_{K}"], 3) for K in widths}}
        out["mean_returned_length"] = {"map": round(float(np.mean([t.shape[1] for t, _ in last["map"]])), 2),
                                       "map_norm": round(float(np.mean([t.shape[1] for t, _, _ in last["map_norm"]])), 2)}
        ended = torch.cat([(t == samp.end_token).any(1) for t, _, _ in last["map_norm"]])
        out["share_of_rows_map_norm_ends"] = round(float(ended.float().mean()), 4)
    return out


res = {"metric": "length-normalised exact decoding vs the un-normalised calls of the same run, 10k molecules = 9 x bs 1024 + 784, "
                 "default AR-CVAE (random init), early stopping on, 1x MI355X, fp32; host wall time incl. the per-batch early-stop "
                 "read; kernels_bs1024 = device events around single launches",
       "root": os.path.basename(os.path.abspath(args.root)), "new_entry_points": NEW, "alpha": args.alpha, "reps": args.reps,
       "max_length": {str(T): run(int(T)) for T in args.max_lengths.split(",")}}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
