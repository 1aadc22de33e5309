"""The top-k / nucleus sampling entry points: declared in include/arcvae_hip.h, bound with the header's arity and types, defined in
csrc/sample.hip and built; argument errors are return codes and ValueErrors raised before any device work (no GPU needed)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

from test_abi import HEADER, ROOT, _ctype_of, _declared_args

NAMES = ("arcvae_dec_topkp_rows", "arcvae_dec_topkp_ws_bytes", "arcvae_dec_sample_chain_topkp")
ERR_ARG = -1
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call below is refused on the host before any launch
CSRC = os.path.join(ROOT, "mlx-vae_amd", "csrc")


def _lib():
    from arcvae_hip import _lib
    return _lib.load()


def test_declared_bound_and_defined():
    from arcvae_hip import _lib
    decl = _declared_args()
    src = open(os.path.join(CSRC, "sample.hip")).read()
    assert re.search(r"^SRCS\s*:=.*\bsample\.hip\b", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    for name in NAMES:
        assert name in decl, name
        assert re.search(r'extern "C"\s+int\s+' + name + r"\s*\(", src), name
        want = [_ctype_of(d) for d in decl[name]]
        assert _lib.SIGNATURES[name] == want, name
        assert hasattr(_lib.load(), name)
    assert "const unsigned long long* seed" in " ".join(decl["arcvae_dec_sample_chain_topkp"])   # a device word, not a value


def _ws_bytes(B=4, V=80, k=20):
    n = C.c_long(-1)
    rc = _lib().arcvae_dec_topkp_ws_bytes(B, V, k, C.byref(n))
    return rc, n.value


def _walk(V=80, temp=1.0, k=20, p=0.9, seed=FAKE, tokens=FAKE, B=4, max_len=8, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = _ws_bytes(B, min(max(V, 1), 256), max(k, 0))[1]
    return _lib().arcvae_dec_sample_chain_topkp(FAKE, tokens, FAKE, ws, ws_bytes, B, V, max_len, 2, temp, k, p, seed, None)


def _rows(V=80, temp=1.0, k=20, p=0.9, table_rows=320, rows=None, R=320, count=FAKE):
    return _lib().arcvae_dec_topkp_rows(FAKE, table_rows, rows, R, V, temp, k, p, count, FAKE, FAKE, None)


@pytest.mark.parametrize("bad", [dict(k=-1), dict(p=0.0), dict(p=1.5), dict(p=float("nan")), dict(p=-0.5), dict(V=257), dict(V=0),
                                 dict(temp=0.0), dict(temp=-1.0), dict(temp=float("nan"))])
def test_argument_errors(bad):
    assert _walk(**bad) == ERR_ARG
    assert _rows(**bad) == ERR_ARG


def test_workspace_size_query():
    R = 1024 * 80
    assert _ws_bytes(1024, 80, 0) == (0, R * 4 + R * 80 * 5)             # count i32 | cum [R, |K|] f32 | tokens [R, |K|] u8
    assert _ws_bytes(1024, 80, 20) == (0, R * 4 + R * 20 * 5)
    assert _ws_bytes(1024, 80, 500) == _ws_bytes(1024, 80, 0)
    for bad in ((0, 80, 0), (4, 0, 0), (4, 257, 0), (4, 80, -1)):
        assert _ws_bytes(*bad)[0] == ERR_ARG, bad


def test_pointer_and_shape_errors():
    assert _walk(ws=None) == ERR_ARG
    assert _walk(ws_bytes=_ws_bytes()[1] - 1) == ERR_ARG
    assert _walk(seed=None) == ERR_ARG
    assert _walk(tokens=None) == ERR_ARG
    assert _walk(B=0) == ERR_ARG and _walk(max_len=0) == ERR_ARG
    assert _rows(count=None) == ERR_ARG
    assert _rows(table_rows=0) == ERR_ARG and _rows(R=0) == ERR_ARG
    assert _rows(R=321) == ERR_ARG                          # all rows of a 320-row table, asked for 321


def _sampler(V=80):
    from models.decoder_sampling import MLXAutoregressiveDecoderSampling
    s = MLXAutoregressiveDecoderSampling.__new__(MLXAutoregressiveDecoderSampling)
    s.decoder = SimpleNamespace(vocab_size=V)
    s._graphs = {}
    return s


@pytest.mark.parametrize("kw", [dict(top_k=5), dict(top_p=0.9), dict(top_k=5, top_p=0.9, sample=False),
                                dict(top_k=0, sample=True), dict(top_k=-3, sample=True), dict(top_p=0.0, sample=True),
                                dict(top_p=1.5, sample=True), dict(top_p=float("nan"), sample=True), dict(top_p=1e-50, sample=True),
                                dict(top_k=5, sample=True, temperature=0.0)])
def test_python_value_errors(kw):
    with pytest.raises(ValueError):
        _sampler().generate_with_temperature(None, None, max_length=8, **kw)


def test_python_refuses_large_vocabularies():
    with pytest.raises(ValueError):
        _sampler(257).generate_with_temperature(None, None, max_length=8, sample=True, top_k=5)
