"""The quiet weight-gradient kernel's selectors agree everywhere they are written down: the C header, the ctypes binding
and the `parts` bit that csrc/lstm.hip reads (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_gemm_flag_in_header_and_binding_agree():
    from arcvae_hip import _lib
    header = _read("include", "arcvae_hip.h")
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define ARCVAE_GEMM_(\w+) (\d+)", header)}
    assert flags["QUIET"] == _lib.GEMM_QUIET == 1024
    others = [v for k, v in flags.items() if k != "QUIET"]
    assert len(set(flags.values())) == len(flags) and all(v & flags["QUIET"] == 0 for v in others)   # a free bit
    for name in ("ACCUMULATE", "SPLITK", "BF16", "SPLIT3"):
        assert flags[name] == getattr(_lib, "GEMM_" + name)


def test_parts_bit_in_binding_kernel_file_and_header_agree():
    from arcvae_hip import _lib
    assert _lib.WGRAD_QUIET == 1 << 9
    lstm = _read("mlx-vae_amd", "csrc", "lstm.hip")
    assert re.search(r"\(parts & 512\) \? 16 : 0", lstm)             # bit 9 -> allow_split bit 4 of the grouped GEMM
    assert "bit 9 =" in lstm and "bit 9 =" in _read("include", "arcvae_hip.h")
    gemm = _read("mlx-vae_amd", "csrc", "gemm.hip")
    assert "(allow_split & 16)" in gemm and "flags & ARCVAE_GEMM_QUIET" in gemm
    # no other reader of the bit in the weight-gradient entry point
    body = lstm[lstm.index('extern "C" int arcvae_enc_lstm_wgrad'):]
    body = body[:body.index("\n}\n")]
    assert body.count("parts & 512") == 1


def test_switch_defaults_and_override(monkeypatch):
    from arcvae_hip import engine
    monkeypatch.delenv("ARCVAE_WGRAD_QUIET", raising=False)
    assert engine.wgrad_quiet() == (engine.WGRAD_QUIET_DEFAULT != "0")
    monkeypatch.setenv("ARCVAE_WGRAD_QUIET", "0")
    assert not engine.wgrad_quiet()
    monkeypatch.setenv("ARCVAE_WGRAD_QUIET", "1")
    assert engine.wgrad_quiet()
