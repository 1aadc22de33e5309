"""The min-p / typical / minimum-length sampling entry points: declared in include/arcvae_hip.h, bound with the header's arity and
types, defined in csrc/sample.hip and built; argument errors are return codes and ValueErrors raised before any device work (no
GPU needed)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

from test_abi import ROOT, _ctype_of, _declared_args

NAMES = ("arcvae_dec_trunc_rows", "arcvae_dec_trunc_ws_bytes", "arcvae_dec_sample_chain_trunc")
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
    for name in NAMES:
        assert name in decl, name
        assert re.search(r'extern "C"\s+int\s+' + name + r"\s*\(", src), name
        want = [_ctype_of(d) for d in decl[name]]
        assert _lib.SIGNATURES[name] == want, name
        assert hasattr(_lib.load(), name)
    assert "const unsigned long long* seed" in " ".join(decl["arcvae_dec_sample_chain_trunc"])   # a device word, not a value
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()


def _ws_bytes(B=4, V=80, k=20, min_len=0):
    n = C.c_long(-1)
    rc = _lib().arcvae_dec_trunc_ws_bytes(B, V, k, min_len, C.byref(n))
    return rc, n.value


def _walk(V=80, temp=1.0, k=20, p=1.0, mp=0.0, tp=1.0, min_len=0, end=2, seed=FAKE, tokens=FAKE, B=4, max_len=8, ws=FAKE,
          ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = _ws_bytes(B, min(max(V, 1), 256), max(k, 0), max(min_len, 0))[1]
    return _lib().arcvae_dec_sample_chain_trunc(FAKE, tokens, FAKE, ws, ws_bytes, B, V, max_len, min_len, end, temp, k, p, mp, tp,
                                                seed, None)


def _rows(V=80, temp=1.0, k=20, p=1.0, mp=0.0, tp=1.0, ban=-1, table_rows=320, rows=None, R=320, count=FAKE):
    return _lib().arcvae_dec_trunc_rows(FAKE, table_rows, rows, R, V, temp, k, p, mp, tp, ban, count, FAKE, FAKE, None, None, None)


@pytest.mark.parametrize("bad", [dict(k=-1), dict(p=0.0), dict(p=1.5), dict(p=float("nan")), dict(V=257), dict(V=0),
                                 dict(temp=0.0), dict(temp=float("nan")), dict(mp=-0.1), dict(mp=1.0), dict(mp=float("nan")),
                                 dict(tp=0.0), dict(tp=1.5), dict(tp=-0.5), dict(tp=float("nan")), dict(tp=0.9, p=0.9),
                                 dict(tp=0.9, mp=0.1)])
def test_argument_errors(bad):
    assert _walk(**bad) == ERR_ARG
    assert _rows(**bad) == ERR_ARG


@pytest.mark.parametrize("bad", [dict(min_len=-1), dict(min_len=9), dict(min_len=1, end=-1), dict(min_len=1, end=80),
                                 dict(min_len=1, V=1, end=0)])
def test_min_len_errors(bad):
    assert _walk(**bad) == ERR_ARG


@pytest.mark.parametrize("bad", [dict(ban=-2), dict(ban=80), dict(ban=0, V=1)])
def test_ban_token_errors(bad):
    assert _rows(**bad) == ERR_ARG


def test_workspace_size_query():
    R = 1024 * 80
    one = R * 4 + R * 20 * 5                                             # count i32 | cum [R, |K|] f32 | tokens [R, |K|] u8
    assert _ws_bytes(1024, 80, 20, 0) == (0, one)
    assert _ws_bytes(1024, 80, 20, 1) == (0, 2 * one) and _ws_bytes(1024, 80, 20, 77) == (0, 2 * one)
    assert _ws_bytes(1024, 80, 0, 3) == (0, 2 * (R * 4 + R * 80 * 5)) and _ws_bytes(1024, 80, 500, 0) == _ws_bytes(1024, 80, 0, 0)
    for bad in ((0, 80, 0, 0), (4, 0, 0, 0), (4, 257, 0, 0), (4, 80, -1, 0), (4, 80, 0, -1)):
        assert _ws_bytes(*bad)[0] == ERR_ARG, bad


def test_pointer_and_shape_errors():
    assert _walk(ws=None) == ERR_ARG
    assert _walk(ws_bytes=_ws_bytes()[1] - 1) == ERR_ARG
    assert _walk(min_len=1, ws_bytes=_ws_bytes(min_len=0)[1]) == ERR_ARG     # min_len > 0 needs the second list set
    assert _walk(min_len=1, ws_bytes=_ws_bytes(min_len=1)[1] - 1) == ERR_ARG
    assert _walk(seed=None) == ERR_ARG
    assert _walk(tokens=None) == ERR_ARG
    assert _walk(B=0) == ERR_ARG and _walk(max_len=0) == ERR_ARG
    assert _rows(count=None) == ERR_ARG
    assert _rows(table_rows=0) == ERR_ARG and _rows(R=0) == ERR_ARG
    assert _rows(R=321) == ERR_ARG


def _sampler(V=80):
    from models.decoder_sampling import MLXAutoregressiveDecoderSampling
    s = MLXAutoregressiveDecoderSampling.__new__(MLXAutoregressiveDecoderSampling)
    s.decoder = SimpleNamespace(vocab_size=V, end_token=2)
    s._graphs = {}
    return s


@pytest.mark.parametrize("kw", [dict(min_p=0.1), dict(typical_p=0.9), dict(min_length=3), dict(min_p=0.1, sample=False),
                                dict(min_p=-0.1, sample=True), dict(min_p=1.0, sample=True), dict(min_p=float("nan"), sample=True),
                                dict(min_p=1.0 - 1e-12, sample=True),            # rounds to 1.0f
                                dict(typical_p=0.0, sample=True), dict(typical_p=1.5, sample=True),
                                dict(typical_p=1e-50, sample=True),              # rounds to 0.0f
                                dict(typical_p=float("nan"), sample=True), dict(typical_p=0.9, top_p=0.9, sample=True),
                                dict(typical_p=0.9, min_p=0.1, sample=True), dict(min_length=-1, sample=True),
                                dict(min_length=9, sample=True), dict(min_p=0.1, top_k=0, sample=True),
                                dict(min_p=0.1, top_p=0.0, sample=True), dict(min_p=0.1, sample=True, temperature=0.0)])
def test_python_value_errors(kw):
    with pytest.raises(ValueError):
        _sampler().generate_with_temperature(None, None, max_length=8, **kw)


def test_python_refuses_what_the_vocabulary_cannot_hold():
    with pytest.raises(ValueError):
        _sampler(257).generate_with_temperature(None, None, max_length=8, sample=True, min_p=0.1)
    with pytest.raises(ValueError):
        _sampler(1).generate_with_temperature(None, None, max_length=8, sample=True, min_length=2)
