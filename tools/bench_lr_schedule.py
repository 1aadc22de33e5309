#!/usr/bin/env python3
"""What a learning-rate schedule costs in the default training step (bs 64, T 128, the default AR-CVAE, random-init weights),
four ways, each on its own identical model in the same process:

  a  by-value rate, constant              (today's step: the rate is a launch argument baked into the captured segments)
  b  device rate, constant                (lr_device=True: the rate word is written once, every later write is skipped)
  c  device rate, changed every step      (one eager one-word fill in front of each replay)
  d  by-value rate, changed every step    (every step is a fresh eager warm-up + capture + one more runner set: --recapture-steps
                                           steps only, host wall time per step, to put a number on the re-capture)

a, b, c alternate per repetition (`measuring-on-mi355x`: no ordering bias, the same clocks); one repetition = --warmup steps,
then --steps steps bracketed by events.  ms/step per repetition and the medians go into one JSON line (and --out).
--root DIR imports the package from another checkout of this repository (a build of the parent commit, which has variants a
and d only): the baseline of the same session.  --variants picks a subset."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--recapture-steps", type=int, default=30)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--variants", default="a,b,c,d")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default="")
args = ap.parse_args()

sys.path.insert(0, os.path.join(os.path.abspath(args.root), "mlx-vae_amd"))
import torch  # noqa: E402
from arcvae_hip import api  # noqa: E402
from models.vae import ARCVAE  # noqa: E402

B, T, V = args.batch, 128, 80
BASE = 2e-4
HYPER = dict(beta=0.05, lambda_collapse=0.001, free_bits=1.0, lambda_mi=0.01, target_mi=4.85)


def variant(device_rate: bool, changing: bool):
    vae = ARCVAE(vocab_size=V, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
                 generator=torch.Generator().manual_seed(0))
    rs = np.random.RandomState(0)
    x = torch.tensor(rs.randint(3, V, size=(B, T)), dtype=torch.int32, device="cuda")
    cond = torch.tensor(rs.standard_normal((B, 1)).astype(np.float32), device="cuda")
    eps = torch.tensor(rs.standard_normal((B, 128)).astype(np.float32), device="cuda")
    coins = torch.tensor((rs.rand(T) < 0.9).astype(np.uint8), device="cuda")
    kw = dict(lr_device=True) if device_rate else {}
    state = {"s": 0}

    def step():
        s = state["s"]
        state["s"] = s + 1
        lr = BASE * (1.0 - 0.5 * (s % 1000) / 1000.0) if changing else BASE      # a new fp32 value every step
        out, _ = api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=lr, **kw, **HYPER)
        state["out"] = out
    return step, state, vae


def timed(step) -> float:
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.steps


names = [n for n in args.variants.split(",") if n]
out = {"batch": B, "T": T, "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "root": os.path.basename(
    os.path.abspath(args.root))}
loop = [n for n in names if n in "abc"]
made = {n: variant(device_rate=n in "bc", changing=n == "c") for n in loop}
res = {n: [] for n in loop}
for rep in range(args.reps):
    for n in (loop if rep % 2 == 0 else loop[::-1]):
        res[n].append(timed(made[n][0]))
for n in loop:
    out[f"{n}_ms"] = [round(v, 4) for v in res[n]]
    out[f"{n}_median_ms"] = round(statistics.median(res[n]), 4)
    out[f"{n}_spread_ms"] = round(max(res[n]) - min(res[n]), 4)
    eng = api.engine_for(made[n][2].encoder, made[n][2].decoder)
    out[f"{n}_runner_sets"] = len(eng._runners)
    if n in "bc":
        out[f"{n}_last_lr"] = float(made[n][1]["out"]["lr"])
for n in loop:
    if n != "a" and "a" in loop:
        out[f"{n}_minus_a_us"] = round(1000 * (out[f"{n}_median_ms"] - out["a_median_ms"]), 2)
if "d" in names:
    step, _, vae = variant(device_rate=False, changing=True)
    step()                                                   # the first capture is paid by every variant
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.recapture_steps):
        step()
    torch.cuda.synchronize()
    out["d_recapture_steps"] = args.recapture_steps
    out["d_wall_ms_per_step"] = round(1e3 * (time.perf_counter() - t0) / args.recapture_steps, 3)
    out["d_runner_sets"] = len(api.engine_for(vae.encoder, vae.decoder)._runners)
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
