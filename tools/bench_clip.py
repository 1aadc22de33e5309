#!/usr/bin/env python3
"""The global-norm clip's cost in the default training step (bs 64, T 128, the default AR-CVAE): the captured step with the
clip off and with it on (--max_norm, default 1.0 as train.py's --grad_clip: above the random-init model's gradient norm of
about 0.2, so nothing is scaled -- the launches are the same either way), on two identical random-init models in the same
process, alternating the two per repetition (`measuring-on-mi355x`: no ordering bias, both under the same clocks).

One repetition = --warmup steps, then --steps steps bracketed by events; ms/step per repetition and the medians go into
one JSON line (and --out).  --only off|on runs one variant (for a separate `rocprofv3 --kernel-trace --stats` run).
--kernels: instead, the clip's kernels alone over the default model's encoder and decoder stores (sum of squares, clipped
Adam) next to the plain Adam update, --steps back-to-back launches bracketed by events: device time per launch."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlx-vae_amd"))
import torch  # noqa: E402
from arcvae_hip import api  # noqa: E402
from models.vae import ARCVAE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--max_norm", type=float, default=1.0)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--only", choices=["off", "on"], default=None)
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()

B, T, V = args.batch, 128, 80
HYPER = dict(beta=0.05, lambda_collapse=0.001, free_bits=1.0, lambda_mi=0.01, target_mi=4.85)


def model():
    return ARCVAE(vocab_size=V, embedding_dim=128, hidden_dim=256, latent_dim=128, num_conditions=1, num_layers=2,
                  generator=torch.Generator().manual_seed(0))


def variant(clip: bool):
    vae = model()
    rs = np.random.RandomState(0)
    x = torch.tensor(rs.randint(3, V, size=(B, T)), dtype=torch.int32, device="cuda")
    cond = torch.tensor(rs.standard_normal((B, 1)).astype(np.float32), device="cuda")
    eps = torch.tensor(rs.standard_normal((B, 128)).astype(np.float32), device="cuda")
    coins = torch.tensor((rs.rand(T) < 0.9).astype(np.uint8), device="cuda")
    gc = args.max_norm if clip else None
    last = {}

    def step():
        out, _ = api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=2e-4, grad_clip=gc, **HYPER)
        last["out"] = out
    return step, last


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


def kernels_alone() -> dict:
    from arcvae_hip._lib import call, load, ptr, stream_ptr
    vae = model()
    stores = {"encoder": vae.encoder.store, "decoder": vae.decoder.store}
    cnt = {}
    for k, st in stores.items():
        n = C.c_long(0)
        load().arcvae_grad_sumsq_partials(C.c_long(st.numel_padded), C.byref(n))
        cnt[k] = n.value
        st.grad.normal_()
    part = torch.zeros(sum(cnt.values()), device="cuda")
    offs = {"encoder": 0, "decoder": cnt["encoder"]}
    out = {}
    for k, st in stores.items():
        n = C.c_long(st.numel_padded)
        p_off = C.c_void_p(part.data_ptr() + 4 * offs[k])

        def sumsq(st=st, n=n, p_off=p_off, c=cnt[k]):
            call("arcvae_grad_sumsq", ptr(st.grad), n, p_off, C.c_long(c), stream_ptr())

        def adam(st=st, n=n):
            call("arcvae_adam_update", ptr(st.flat), ptr(st.grad), ptr(st.adam_m), ptr(st.adam_v), n, 0.0, 0.9, 0.999, 1e-8,
                 None, None, stream_ptr())

        def adam_clip(st=st, n=n):
            call("arcvae_adam_update_clipped", ptr(st.flat), ptr(st.grad), ptr(st.adam_m), ptr(st.adam_v), n, 0.0, 0.9, 0.999,
                 1e-8, None, None, ptr(part), C.c_long(part.numel()), 1.0, None, stream_ptr())

        res = {"floats": st.numel_padded, "partials": cnt[k]}
        for name, fn in (("sumsq_us", sumsq), ("adam_us", adam), ("adam_clipped_us", adam_clip)):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name] = round(1000 * e0.elapsed_time(e1) / args.steps, 2)
        out[k] = res
    return out


if args.kernels:
    res = {"launches": args.steps, "note": "lr 0: the parameters stay put between launches", **kernels_alone()}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    sys.exit(0)

names = [args.only] if args.only else ["off", "on"]
steps = {n: variant(n == "on") for n in names}
res = {n: [] for n in names}
for rep in range(args.reps):
    order = names if rep % 2 == 0 else names[::-1]
    for n in order:
        res[n].append(timed(steps[n][0]))
out = {"batch": B, "T": T, "max_norm": args.max_norm, "steps": args.steps, "reps": args.reps,
       **{f"{n}_ms": [round(v, 4) for v in res[n]] for n in names},
       **{f"{n}_median_ms": round(statistics.median(res[n]), 4) for n in names}}
if "on" in steps:
    o = steps["on"][1]["out"]
    out["last_grad_norm"], out["last_clip_scale"] = float(o["grad_norm"]), float(o["clip_scale"])
if len(names) == 2:
    out["added_us"] = round(1000 * (out["on_median_ms"] - out["off_median_ms"]), 1)
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
