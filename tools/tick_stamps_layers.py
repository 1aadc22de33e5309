"""Tick anatomy of the layer-split forward sweep (lstm_fwd_persist_split), one chain per layer: the diagnostic library
(tools/build_stamps.sh) writes five stamps per tick, chain and stamped wave of one block, and HW_ID of its eight waves; this
prints the median gaps (us) over the steady-state ticks, the forward sweep ALONE, for the form ARCVAE_LS_ROLES selects.
usage: ARCVAE_HIP_LIB=ab_libs/libarcvae_stamps.so [ARCVAE_LS_ROLES=n] python tools/tick_stamps_layers.py [batch]
stamped waves per chain: the epilogue wave and the polling wave.  stamps: 0 tick top | 1 flag line seen (poll, or the LDS
word of the polling wave) | 2 the wave's partial counted (epilogue wave: all four partials of the layer seen) | 3 cell epilogue
done, h stores acknowledged, flag stored (= 2 in the polling wave) | 4 layer 0: a ring slot is free (after it: cross product
Wx1 h0 + ring store, up to the next tick's 0); layer 1: the ring slot of the tick is filled (between 1 and 2)"""
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
W = 32                                                   # trace row: [layer][epilogue wave, polling wave][8]
params, x, cond, eps, coins = make_case(DEFAULT, BS, T, 0.9)
eng, enc, dec = build_engine(DEFAULT, params)
ws = eng.workspace(BS, T)
ws.trace_fwd = torch.zeros(W * (T + 8), dtype=torch.int64, device=eng.device)
eng.set_hyper(ws, **HYPER); eng.load_inputs(ws, x, cond, eps, coins)
eng.mode = "eager"
eng.run_step(ws, 2e-4, False); torch.cuda.synchronize(); eng.check_gates()
d = eng.d
med = lambda v: float(np.median(v))
print(f"ARCVAE_LS_ROLES={os.environ.get('ARCVAE_LS_ROLES', '(default)')} ARCVAE_STEP_PRIO={os.environ.get('ARCVAE_STEP_PRIO', '(default)')} batch {BS}")
for rep in range(3):
    E.encoder_forward(enc, ws, d, 1.0); torch.cuda.synchronize()
    raw = ws.trace_fwd.cpu().numpy()
    st = raw.reshape(-1, W)[:T + 1].astype(np.float64) / 100.0   # us
    lo, hi = 8, T - 8
    for ly in range(2):
        for w, name in ((0, "epilogue wave"), (1, "polling wave ")):
            s = st[:, 16 * ly + 8 * w:16 * ly + 8 * w + 5]
            a, b = s[lo:hi], s[lo + 1:hi + 1]
            tick = b[:, 0] - a[:, 0]
            line = (f"layer {ly} {name}: tick {med(tick):.2f} us (p10 {np.percentile(tick, 10):.2f}, p90 {np.percentile(tick, 90):.2f}) | "
                    f"poll {med(a[:, 1] - a[:, 0]):.2f} | ")
            if ly == 0:
                line += (f"products + partials {med(a[:, 2] - a[:, 1]):.2f} | epilogue + ack + flag {med(a[:, 3] - a[:, 2]):.2f} | "
                         f"ring-slot wait {med(a[:, 4] - a[:, 3]):.2f} | cross product + ring store {med(b[:, 0] - a[:, 4]):.2f}")
            else:
                line += (f"ring-slot wait {med(a[:, 4] - a[:, 1]):.2f} | products + partials {med(a[:, 2] - a[:, 4]):.2f} | "
                         f"epilogue + ack + flag {med(a[:, 3] - a[:, 2]):.2f} | rest {med(b[:, 0] - a[:, 3]):.2f}")
            if w == 1: line += f" | failed polls per tick {med(st[lo:hi, 16 * ly + 13] * 100.0):.0f}"
            print(line)
    lead = st[lo:hi, 16] - st[lo:hi, 0]
    tick0 = st[lo + 1:hi + 1, 0] - st[lo:hi, 0]
    print(f"layer 1 tick t starts {med(lead):.2f} us after layer 0 tick t ({med(lead) / med(tick0):.2f} ticks); "
          f"sweep, first to last stamp: {(st[T - 1, 19] - st[0, 0]):.1f} us")
hw = raw[W * (T + 1):W * (T + 1) + 8]
print("SIMD of waves 0-7 (HW_ID bits 5:4):", " ".join(str(int(h >> 4) & 3) for h in hw),
      "| CU key (bits 15:8):", " ".join(f"{int(h >> 8) & 0xff:02x}" for h in hw))
print("err word", int(ws.psync[500].item()))
