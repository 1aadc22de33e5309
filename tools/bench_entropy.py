#!/usr/bin/env python3
"""Exact entropy and divergence of the molecule distribution at BASELINE.json configs[4]'s shape on 1 MI355X: one bs-1024 batch,
the default AR-CVAE (random-init weights: a nearly flat chain -- the numbers are times, not statements about trained weights),
V 80, max_length 80 and 128.  In one process, every method timed --reps times after an untimed run of itself, median:

  sequence_entropy        the dense pass + arcvae_dec_row_lse + arcvae_dec_row_costs + arcvae_dec_chain_expect
  sequence_divergence     against other conditions: a copy of P's table, a second dense pass and lse, the same two launches
  marginals_route         the route there was for the same entropy: token_marginals (alive [B, T, V] written to memory), then the
                          row entropies and the reductions by torch
  kernels                 device events around single launches: the two new ones, and arcvae_dec_chain_marginals beside them

Host wall time around work that ends in a device synchronise; the kernels by device events.  The entropy of the two routes is
compared (they sum in different orders).  Prints one JSON line (and writes it to --out when given)."""
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
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--max-lengths", default="80,128")
ap.add_argument("--out", default="")
args = ap.parse_args()

vae = ARCVAE(vocab_size=80, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
             generator=torch.Generator().manual_seed(0))
samp = vae.decoder_sampling
dec = samp.decoder
V, END, B = dec.vocab_size, samp.end_token, args.batch
rs = np.random.RandomState(0)
cond = torch.tensor(rs.standard_normal((B, 1)).astype(np.float32), device="cuda")
cond_q = cond + 1.0


def med(v):
    return sorted(v)[len(v) // 2]


def wall(fn):
    """Median host wall time (ms) of fn + synchronise over --reps runs, after one untimed run; and the last result."""
    r = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return med(ts), ts, r


def device(fn):
    """Median device time (ms) between events around one launch over --reps runs, after one untimed run."""
    ts = []
    for _ in range(args.reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(med(ts[1:]), 4)


def marginals_route(T):
    """The same entropy by what there was: alive through memory, everything else by torch."""
    alive = samp.token_marginals(cond, max_length=T)
    lp = torch.log_softmax(dec.workspace(B, T).logits, dim=1)
    p = lp.exp()
    h = -torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(dim=1).view(B, V)
    cont = alive[:, :T - 1, :].sum(dim=1)
    cont[:, END] = 0.0
    return h[:, 0] + (h * cont).sum(dim=1)


def kernels(T):
    ws, _ = dec.load_conditions(cond, T)
    dec.dense_table(ws)
    lse = dec.table_lse(ws, 1.0)
    cost = torch.empty(2, B * V, dtype=torch.float32, device="cuda")
    totals = torch.empty(B, 2, dtype=torch.float32, device="cuda")
    alive = torch.empty(B, T, V, dtype=torch.float32, device="cuda")
    return {
        "row_costs_h_ms": device(lambda: call("arcvae_dec_row_costs", ptr(ws.logits), ptr(lse), 1.0, None, None, 1.0, ptr(cost[0]),
                                              None, B * V, V, stream_ptr())),
        "row_costs_h_and_c_ms": device(lambda: call("arcvae_dec_row_costs", ptr(ws.logits), ptr(lse), 1.0, ptr(ws.logits), ptr(lse),
                                                    1.0, ptr(cost[0]), ptr(cost[1]), B * V, V, stream_ptr())),
        "chain_expect_1_cost_ms": device(lambda: call("arcvae_dec_chain_expect", ptr(ws.logits), ptr(lse), ptr(cost), 1, ptr(totals),
                                                      None, None, B, V, T, END, 1.0, stream_ptr())),
        "chain_expect_2_costs_ms": device(lambda: call("arcvae_dec_chain_expect", ptr(ws.logits), ptr(lse), ptr(cost), 2,
                                                       ptr(totals), None, None, B, V, T, END, 1.0, stream_ptr())),
        "chain_marginals_ms": device(lambda: call("arcvae_dec_chain_marginals", ptr(ws.logits), ptr(lse), ptr(alive), B, V, T, END,
                                                  1.0, stream_ptr())),
        "alive_bytes": alive.numel() * 4,
    }


def run(T):
    t_h, all_h, H = wall(lambda: samp.sequence_entropy(cond, max_length=T))
    t_d, all_d, (kl, _, _) = wall(lambda: samp.sequence_divergence(cond, other_conditions=cond_q, max_length=T))
    t_m, all_m, Hm = wall(lambda: marginals_route(T))
    gap = float(((H.double() - Hm.double()).abs() / Hm.double().abs()).max())
    return {"sequence_entropy_ms": round(t_h, 3), "sequence_divergence_ms": round(t_d, 3), "marginals_route_ms": round(t_m, 3),
            "sequence_entropy_vs_marginals_route": round(t_h / t_m, 3),
            "max_rel_gap_between_the_two_routes": gap,
            "entropy_nats_min_max": [float(H.min()), float(H.max())], "kl_nats_min_max": [float(kl.min()), float(kl.max())],
            "kernels": kernels(T),
            "all_ms": {"sequence_entropy": [round(t, 3) for t in all_h], "sequence_divergence": [round(t, 3) for t in all_d],
                       "marginals_route": [round(t, 3) for t in all_m]}}


res = {"metric": "exact entropy / divergence of the molecule distribution, one bs-%d batch, default AR-CVAE (random init), V 80, "
                 "1x MI355X, fp32; host wall time per batch ending in a synchronise, median; kernels = device events around "
                 "single launches" % B,
       "reps": args.reps,
       "max_length": {str(T): run(int(T)) for T in args.max_lengths.split(",")}}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
