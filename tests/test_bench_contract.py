"""The bench line the driver parses (bench.py prints exactly this object on stdout): schema check on the newest
committed run profiles/r*_bench.json, so that a change to bench.py that drops or renames a field fails on CPU; and the
self-launch path of `python bench.py --gpus N` (no GPU needed: --dry-launch prints the command of the child)."""
import glob
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _newest_bench():
    return json.load(open(sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench.json")))[-1]))


def test_gpus_n_without_a_launcher_starts_its_own_ranks():
    """`python bench.py --gpus 8` (the command shape the driver uses at N = 1) must not die on a missing WORLD_SIZE:
    it launches torch.distributed.run as a child.  --dry-launch shows that command without touching a GPU."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "7", "--warmup", "3",
                        "--dry-launch"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    cmd = json.loads(r.stdout.strip().splitlines()[-1])["launch"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    tail = cmd[cmd.index(os.path.join(ROOT, "bench.py")) + 1:]
    assert tail == ["--gpus", "8", "--steps", "7", "--warmup", "3"]        # same arguments, minus --dry-launch
    # one GPU: nothing to launch
    r1 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-launch"], capture_output=True, text=True,
                        env=env, timeout=120)
    assert r1.returncode == 0 and json.loads(r1.stdout.strip())["launch"] is None


def test_committed_bench_line_has_every_contract_field():
    d = _newest_bench()
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "sequences/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1
    # the legs reported NEXT TO the fp32 headline (never instead of it): strong scaling, throughput mode, configs[2]
    s = d["strong"]
    assert s["global_batch"] == 2048 and s["scaling"] == "strong" and s["value"] > 0
    b = d["bf16_mode"]
    assert b["dtype"] == "bf16" and b["ms_per_step"] > 0 and "tolerance" in b and "NOT" in b["tolerance"]
    o = d["other_configs"]["configs[2]"]
    assert o["fp32"]["dtype"] == "f32" and o["bf16"]["dtype"] == "bf16"
    # (SURVEY 8(d)'s ratio for configs[2] is algorithmic f32 FLOP over the f32 MFMA peak; the three-piece kernels issue bf16 products,
    # so since round 4 it can pass 1 -- then the line must say so, and the fraction of the pipe in use must be a fraction)
    assert 0.0 < o["fp32"]["frac_of_f32_mfma_peak"] < 1.5 and 0.0 < o["bf16"]["frac_of_bf16_mfma_peak"] < 1.0
    assert 0.0 < o["fp32"]["executed_frac_of_bf16_pipe"] < 1.0
    if o["fp32"]["frac_of_f32_mfma_peak"] >= 1.0:
        assert "frac_note" in o["fp32"]


def test_bench_source_names_the_contract_fields():
    src = open(os.path.join(ROOT, "bench.py")).read()
    for k in ('"metric"', '"n_gpus"', '"ms_per_step"', '"higher_is_better"', '"scaling"', '"vs_baseline"', '"dtype"',
              '"roofline"', '"cpu_baseline"', '"workload"', '"strong"', '"n_ranks_seen"', '"step_tflops_executed"',
              '"tick_model"', '"limiter"', '"bf16_mode"', '"other_configs"'):
        assert k in src, k


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dry-launch"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_dump_outputs_keeps_to_its_budget_with_a_fixed_sample(tmp_path):
    """Arrays that fit are written whole; past the budget the largest ones become fixed samples (same positions every run)."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rs = np.random.RandomState(5)
    named = {"small": rs.rand(10).astype(np.float32), "scalar": np.asarray(np.float32(2.5)),
             "big": rs.rand(600, 1000).astype(np.float32), "mid": rs.rand(100, 1000).astype(np.float64)}
    bench.dump_outputs(str(tmp_path / "whole"), named)
    for k, a in named.items():
        assert np.array_equal(np.load(tmp_path / "whole" / f"{k}.npy"), a), k
    budget = 10 ** 6
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), named, budget=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget
    assert "small.npy" in files and "scalar.npy" in files and "big_sample.npy" in files
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    s = np.load(tmp_path / "a" / "big_sample.npy")
    assert s.ndim == 1 and 0 < s.size < named["big"].size and np.isin(s, named["big"]).all()


@pytest.mark.gpu
def test_dump_outputs_is_the_last_timed_step(tmp_path):
    """--dump-outputs on the headline leg: the loss it writes is the line's, every parameter has its gradient and its post-Adam
    value, all float32 and finite, within 64 MB."""
    import numpy as np
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--cpu-steps", "0",
                        "--no-roofline", "--strong-global-batch", "0", "--bf16-steps", "0", "--configs2-steps", "0",
                        "--sampler-reps", "0", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    arrs = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 * 10 ** 6
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert float(arrs["total_loss"]) == line["elbo"]["total"] and float(arrs["recon_loss"]) == line["elbo"]["recon"]
    assert arrs["logits"].shape == (64, 128, 80) and arrs["mu"].shape == arrs["z"].shape == (64, 128)
    sys.path.insert(0, os.path.join(ROOT, "mlx-vae_amd"))
    from arcvae_hip.store import decoder_shapes, encoder_shapes
    for mod, shapes in (("encoder", encoder_shapes(80, 128, 256, 128, 1, 2)), ("decoder", decoder_shapes(80, 128, 256, 128, 1, 2))):
        for n, shp in shapes.items():
            assert arrs[f"grad.{mod}.{n}"].shape == arrs[f"param.{mod}.{n}"].shape == tuple(shp), (mod, n)
