#!/usr/bin/env python3
"""The property predictor's cost in the default training step (bs 64, T 128, the default AR-CVAE): the captured step
without a predictor and with one of hidden width --hidden (default 64), on two identical random-init models in the same
process, alternating the two per repetition (`measuring-on-mi355x`: no ordering bias, both under the same clocks).

One repetition = --warmup steps, then --steps steps bracketed by events; ms/step per repetition and the medians go into
one JSON line (and --out).  --only plain|prop runs one variant (the separate `rocprofv3 --kernel-trace --stats` run that
gives the predictor kernels' device time).  --kernels B1,B2,..: instead, each predictor entry point alone (training launch,
reduction) at those batch sizes, --steps back-to-back launches bracketed by events: device time per launch."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlx-vae_amd"))
import torch  # noqa: E402
from arcvae_hip import api  # noqa: E402
from models import PropertyPredictor  # noqa: E402
from models.vae import ARCVAE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--hidden", type=int, default=64)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--only", choices=["plain", "prop"], default=None)
ap.add_argument("--kernels", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

B, T, V = args.batch, 128, 80
HYPER = dict(beta=0.05, lambda_collapse=0.001, free_bits=1.0, lambda_mi=0.01, target_mi=4.85)


def variant(with_pred: bool):
    vae = ARCVAE(vocab_size=V, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
                 generator=torch.Generator().manual_seed(0))
    pred = PropertyPredictor(128, 1, args.hidden, generator=torch.Generator().manual_seed(1)) if with_pred else None
    rs = np.random.RandomState(0)
    x = torch.tensor(rs.randint(3, V, size=(B, T)), dtype=torch.int32, device="cuda")
    cond = torch.tensor(rs.standard_normal((B, 1)).astype(np.float32), device="cuda")
    eps = torch.tensor(rs.standard_normal((B, 128)).astype(np.float32), device="cuda")
    coins = torch.tensor((rs.rand(T) < 0.9).astype(np.uint8), device="cuda")
    hyper = dict(HYPER, lambda_prop=0.1) if with_pred else HYPER

    def step():
        api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=2e-4, predictor=pred, **hyper)
    return step


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


def kernels_alone(B: int) -> dict:
    import ctypes as C
    from arcvae_hip._lib import call, ptr, stream_ptr
    from models.property_predictor import ws_floats
    Z, Cn, Hp = 128, 1, args.hidden
    pred = PropertyPredictor(Z, Cn, Hp, generator=torch.Generator().manual_seed(1))
    st = pred.store
    g = torch.Generator(device="cuda").manual_seed(0)
    z, eps, mu_raw, lv_raw, dmu, dlv = (torch.randn(B, Z, device="cuda", generator=g) for _ in range(6))
    cond = torch.randn(B, Cn, device="cuda", generator=g)
    hyper = torch.zeros(8, device="cuda")
    hyper[5] = 0.1
    ws = torch.empty(ws_floats(B, Z, Cn, Hp), device="cuda")
    sc = torch.zeros(16, device="cuda")
    W = [ptr(st.p(n)) for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")]
    dW = [ptr(st.g(n)) for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")]

    def rows():
        call("arcvae_prop_backward", ptr(z), ptr(cond), ptr(eps), ptr(mu_raw), ptr(lv_raw), *W, ptr(hyper), ptr(dmu), ptr(dlv),
             None, ptr(ws), C.c_long(ws.numel()), B, Z, Cn, Hp, stream_ptr())

    def reduce():
        call("arcvae_prop_wgrad", ptr(z), ptr(ws), C.c_long(ws.numel()), ptr(hyper), *dW, ptr(sc), B, Z, Cn, Hp, stream_ptr())

    out = {}
    for name, fn in (("rows_us", rows), ("reduce_us", reduce)):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name] = round(1000 * e0.elapsed_time(e1) / args.steps, 2)
    return out


if args.kernels:
    res = {"hidden": args.hidden, "Z": 128, "C": 1, "launches": args.steps,
           "by_batch": {b: kernels_alone(int(b)) for b in args.kernels.split(",")}}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    sys.exit(0)

names = [args.only] if args.only else ["plain", "prop"]
steps = {n: variant(n == "prop") for n in names}
res = {n: [] for n in names}
for rep in range(args.reps):
    order = names if rep % 2 == 0 else names[::-1]
    for n in order:
        res[n].append(timed(steps[n]))
out = {"batch": B, "T": T, "hidden": args.hidden, "steps": args.steps, "reps": args.reps,
       **{f"{n}_ms": [round(v, 4) for v in res[n]] for n in names},
       **{f"{n}_median_ms": round(statistics.median(res[n]), 4) for n in names}}
if len(names) == 2:
    out["added_us"] = round(1000 * (out["prop_median_ms"] - out["plain_median_ms"]), 1)
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
