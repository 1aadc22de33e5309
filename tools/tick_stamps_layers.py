"""Tick anatomy of the layer-split forward sweep (lstm_fwd_persist_split), one chain per layer: the diagnostic library
(tools/build_stamps.sh) writes four stamps per tick and chain of one block; this prints the median gaps (us) over the
steady-state ticks, the forward sweep ALONE.  usage: ARCVAE_HIP_LIB=ab_libs/libarcvae_stamps.so python tools/tick_stamps_layers.py [batch]
stamps per chain (epilogue wave of the layer): 0 tick top | 1 flag line seen (poll, or the LDS word of the polling wave) |
2 the layer's four partials (and, layer 1, its ring slot) in LDS | 3 cell epilogue done, h stores acknowledged, flag stored"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("ARCVAE_HIP_LIB", os.path.join(ROOT, "ab_libs", "libarcvae_stamps.so"))
for p in ("mlx-vae_amd", "tests", "oracle"): sys.path.insert(0, os.path.join(ROOT, p))
import torch
import arcvae_hip.engine as E
from helpers import DEFAULT, HYPER, build_engine, make_case
BS = int(sys.argv[1]) if len(sys.argv) > 1 else 64
T = 128
params, x, cond, eps, coins = make_case(DEFAULT, BS, T, 0.9)
eng, enc, dec = build_engine(DEFAULT, params)
ws = eng.workspace(BS, T)
ws.trace_fwd = torch.zeros(8 * (T + 8), dtype=torch.int64, device=eng.device)
eng.set_hyper(ws, **HYPER); eng.load_inputs(ws, x, cond, eps, coins)
eng.mode = "eager"
eng.run_step(ws, 2e-4, False); torch.cuda.synchronize(); eng.check_gates()
d = eng.d
for rep in range(3):
    E.encoder_forward(enc, ws, d, 1.0); torch.cuda.synchronize()
    st = ws.trace_fwd.cpu().numpy().reshape(-1, 8)[:T].astype(np.float64) / 100.0   # us
    lo, hi = 8, T - 8
    for ly in range(2):
        s = st[:, 4 * ly:4 * ly + 4]
        gaps = np.diff(s[lo:hi], axis=1)
        tick = s[lo + 1:hi + 1, 0] - s[lo:hi, 0]
        print(f"layer {ly}: tick {np.median(tick):.2f} us (p10 {np.percentile(tick, 10):.2f}, p90 {np.percentile(tick, 90):.2f}) | "
              f"poll {np.median(gaps[:, 0]):.2f} | products + partials {np.median(gaps[:, 1]):.2f} | epilogue + ack + flag "
              f"{np.median(gaps[:, 2]):.2f}")
    lead = st[lo:hi, 4] - st[lo:hi, 0]
    print(f"layer 1 tick t starts {np.median(lead):.2f} us after layer 0 tick t")
print("err word", int(ws.psync[500].item()))
