#!/usr/bin/env python3
"""What the weight EMA costs in the default training step (bs 64, T 128, the default AR-CVAE, random-init weights), each
variant on its own identical model in the same process:

  off  the step alone                     (today's launches: nothing of the EMA runs)
  on   the step + WeightEMA.update()      (one launch behind the step on its stream, guards of the step's workspace)

off and on alternate per repetition (`measuring-on-mi355x`: no ordering bias, the same clocks); one repetition = --warmup steps,
then --steps steps bracketed by events.  The two kernels alone (update and swap over the model's stores, back to back on an idle
device, --kernel-iters launches between two events) are timed too.  ms/step per repetition, the medians and the kernel times go
into one JSON line (and --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--kernel-iters", type=int, default=200)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--decay", type=float, default=0.9999)
ap.add_argument("--out", default="")
args = ap.parse_args()

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlx-vae_amd"))
import torch  # noqa: E402
from arcvae_hip import api  # noqa: E402
from arcvae_hip.ema import WeightEMA  # noqa: E402
from models.vae import ARCVAE  # noqa: E402

B, T, V = args.batch, 128, 80
HYPER = dict(beta=0.05, lambda_collapse=0.001, free_bits=1.0, lambda_mi=0.01, target_mi=4.85)


def variant(with_ema: bool):
    vae = ARCVAE(vocab_size=V, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
                 generator=torch.Generator().manual_seed(0))
    rs = np.random.RandomState(0)
    x = torch.tensor(rs.randint(3, V, size=(B, T)), dtype=torch.int32, device="cuda")
    cond = torch.tensor(rs.standard_normal((B, 1)).astype(np.float32), device="cuda")
    eps = torch.tensor(rs.standard_normal((B, 128)).astype(np.float32), device="cuda")
    coins = torch.tensor((rs.rand(T) < 0.9).astype(np.uint8), device="cuda")
    ema = WeightEMA({"encoder": vae.encoder.store, "decoder": vae.decoder.store}, args.decay) if with_ema else None

    def step():
        api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=2e-4, **HYPER)
        if ema is not None:
            ema.update(guards=api.last_step_guards(vae.encoder, vae.decoder))
    return step, vae, ema


def timed(fn, warmup: int, iters: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


made = {"off": variant(False), "on": variant(True)}
loop = ["off", "on"]
res = {n: [] for n in loop}
for rep in range(args.reps):
    for n in (loop if rep % 2 == 0 else loop[::-1]):
        res[n].append(timed(made[n][0], args.warmup, args.steps))
ema = made["on"][2]
out = {"batch": B, "T": T, "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "decay": args.decay,
       "ema_floats": int(sum(st.flat.numel() for st in ema.stores.values())), "num_updates": ema.num_updates}
for n in loop:
    out[f"{n}_ms"] = [round(v, 4) for v in res[n]]
    out[f"{n}_median_ms"] = round(statistics.median(res[n]), 4)
    out[f"{n}_spread_ms"] = round(max(res[n]) - min(res[n]), 4)
out["on_minus_off_us"] = round(1000 * (out["on_median_ms"] - out["off_median_ms"]), 2)
# the kernels alone: back-to-back launches on an idle device (a launch-bound figure: each includes its launch gap)
out["update_kernel_us"] = round(1000 * timed(ema.update, 20, args.kernel_iters), 3)
out["swap_kernel_us"] = round(1000 * timed(ema._swap, 20, 2 * (args.kernel_iters // 2)), 3)      # an even count: weights restored
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
