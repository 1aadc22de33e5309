"""The token-table fold alone at the default shape (V 80, E 128, 4H 1024): arcvae_table_finalize (f32 FMAs from LDS,
atomics) against arcvae_table_fold (exact-f32 MFMA, one owner per element), without and with the decoder's dead forget
quarter.  Each form is captured as a graph of N back-to-back launches; HIP events around every replay; one JSON line with
the median per launch over the replays.   python tools/bench_fold.py [--replays 200] [--per-graph 20]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlx-vae_amd"))
import torch
from arcvae_hip import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--replays", type=int, default=200)
ap.add_argument("--per-graph", type=int, default=20)
args = ap.parse_args()
V, E, G = 80, 128, 1024
dev = "cuda"
dT = torch.randn(V, G, device=dev); dT2 = torch.randn(V, G, device=dev)
Wx0 = torch.randn(G, E, device=dev); emb = torch.randn(V, E, device=dev)
dEmb = torch.zeros(V, E, device=dev); dWx0 = torch.zeros(G, E, device=dev); db0 = torch.zeros(G, device=dev)
p = _lib.ptr


def old():
    _lib.call("arcvae_table_finalize", p(dT), p(Wx0), E, p(emb), p(dEmb), p(dWx0), p(db0), V, E, G, _lib.stream_ptr())


def new(two=False, lo=0, hi=0):
    _lib.call("arcvae_table_fold", p(dT), p(dT2 if two else None), p(Wx0), E, p(emb), p(dEmb), p(dWx0), p(db0), V, E, G, lo, hi,
              _lib.stream_ptr())


forms = {"table_finalize": old, "table_fold": new, "table_fold_two_tables": lambda: new(True),
         "table_fold_dead_quarter": lambda: new(False, G // 4, G // 2)}
res = {"shape": {"V": V, "E": E, "G": G}, "launches_per_graph": args.per_graph, "replays": args.replays, "us_per_launch": {}}
side = torch.cuda.Stream()
for name, fn in forms.items():
    with torch.cuda.stream(side):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(args.per_graph):
                fn()
        for _ in range(5):
            g.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side); g.replay(); e1.record(side)
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1) / args.per_graph)
        dEmb.zero_(); dWx0.zero_(); db0.zero_()
    ts.sort()
    res["us_per_launch"][name] = {"median": round(statistics.median(ts), 2), "p10": round(ts[len(ts) // 10], 2),
                                  "p90": round(ts[len(ts) * 9 // 10], 2)}
print(json.dumps(res))
