"""The N-draws-per-row sampling entry points: declared in include/arcvae_hip.h, bound with the header's arity and types, defined
in csrc/sample.hip and built; argument errors are return codes and ValueErrors raised before any device work (no GPU needed)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

from test_abi import ROOT, _ctype_of, _declared_args

NAMES = ("arcvae_dec_sample_draws_ws_bytes", "arcvae_dec_sample_draws")
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
    assert "const unsigned long long* seed" in " ".join(decl["arcvae_dec_sample_draws"])   # a device word, not a value
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()


def _ws_bytes(B=4, V=80, k=20, min_len=0, name="arcvae_dec_sample_draws_ws_bytes"):
    n = C.c_long(-1)
    rc = getattr(_lib(), name)(B, V, k, min_len, C.byref(n))
    return rc, n.value


def _draws(V=80, temp=1.0, k=20, p=1.0, mp=0.0, tp=1.0, min_len=0, end=2, pad=-1, seed=FAKE, tokens=FAKE, first_end=FAKE,
           table=FAKE, B=4, N=3, max_len=8, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = _ws_bytes(B, min(max(V, 1), 256), max(k, 0), max(min_len, 0))[1]
    return _lib().arcvae_dec_sample_draws(table, tokens, first_end, ws, ws_bytes, B, N, V, max_len, min_len, end, pad, temp, k, p, mp,
                                          tp, seed, None)


def test_workspace_query_is_the_truncated_walks():
    for dims in ((1024, 80, 20, 0), (1, 80, 0, 10), (16, 256, 0, 0), (3, 3, 500, 1)):
        assert _ws_bytes(*dims) == _ws_bytes(*dims, name="arcvae_dec_trunc_ws_bytes") and _ws_bytes(*dims)[0] == 0
    for bad in ((0, 80, 0, 0), (4, 0, 0, 0), (4, 257, 0, 0), (4, 80, -1, 0), (4, 80, 0, -1)):
        assert _ws_bytes(*bad)[0] == ERR_ARG, bad
    assert _lib().arcvae_dec_sample_draws_ws_bytes(4, 80, 0, 0, None) == ERR_ARG


@pytest.mark.parametrize("bad", [dict(N=0), dict(N=-1), dict(pad=256), dict(pad=-2), dict(min_len=9), dict(min_len=-1),
                                 dict(min_len=1, end=-1), dict(min_len=1, end=80), dict(min_len=1, V=1, end=0),
                                 dict(temp=float("nan")), dict(temp=0.0), dict(k=-1), dict(p=0.0), dict(p=float("nan")),
                                 dict(mp=1.0), dict(tp=0.0), dict(tp=0.9, p=0.9), dict(tp=0.9, mp=0.1), dict(V=257), dict(V=0),
                                 dict(B=0), dict(max_len=0), dict(table=None), dict(tokens=None), dict(first_end=None),
                                 dict(ws=None), dict(seed=None),
                                 dict(B=4, N=2 ** 30),                    # B * N = 2^32: beyond the int a draw's index is
                                 dict(B=1, N=2 ** 30, max_len=2 ** 31 - 1),   # B * N * max_len ~ 2^61: beyond the output bound
                                 dict(B=2 ** 24, N=1, V=1, k=0),          # B * (N + 255) = 2^32: beyond what one launch holds
                                 dict(B=2 ** 26, N=1, V=1, k=0)])
def test_argument_errors(bad):
    assert _draws(**bad) == ERR_ARG


def test_workspace_size_is_checked():
    assert _draws(ws_bytes=_ws_bytes()[1] - 1) == ERR_ARG
    assert _draws(min_len=1, ws_bytes=_ws_bytes(min_len=0)[1]) == ERR_ARG     # min_len > 0 needs the second list set
    assert _draws(min_len=1, ws_bytes=_ws_bytes(min_len=1)[1] - 1) == ERR_ARG


def _sampler(V=80):
    from models.decoder_sampling import MLXAutoregressiveDecoderSampling
    s = MLXAutoregressiveDecoderSampling.__new__(MLXAutoregressiveDecoderSampling)
    s.decoder = SimpleNamespace(vocab_size=V, end_token=2)
    s.pad_token, s.end_token = 0, 2
    s._graphs = {}
    return s


@pytest.mark.parametrize("kw", [dict(num_draws=0), dict(num_draws=-3), dict(top_k=0), dict(top_p=0.0), dict(top_p=1.5),
                                dict(min_p=1.0), dict(min_p=-0.1), dict(min_p=float("nan")), dict(typical_p=0.0),
                                dict(typical_p=0.9, top_p=0.9), dict(typical_p=0.9, min_p=0.1), dict(min_length=-1),
                                dict(min_length=9), dict(temperature=0.0)])
def test_python_value_errors(kw):
    kw = dict(dict(num_draws=4), **kw)
    with pytest.raises(ValueError):
        _sampler().generate_many(None, max_length=8, **kw)


def test_python_refuses_what_the_vocabulary_or_the_pad_token_cannot_hold():
    with pytest.raises(ValueError):
        _sampler(257).generate_many(None, 4, max_length=8)
    with pytest.raises(ValueError):
        _sampler(1).generate_many(None, 4, max_length=8, min_length=2)
    s = _sampler()
    s.pad_token = 300
    with pytest.raises(ValueError):
        s.generate_many(None, 4, max_length=8)


@pytest.mark.parametrize("kw", [dict(num_draws=3), dict(sample=True, num_draws=3, beam_width=4),
                                dict(sample=True, num_draws=3, num_samples=2), dict(sample=True, num_draws=3, exact=True),
                                dict(sample=True, num_draws=3, num_best=2), dict(sample=True, num_draws=3, length_penalty=1.0)])
def test_generate_refuses_num_draws_with_the_other_decoders(kw):
    from models.vae import ARCVAE
    vae = ARCVAE.__new__(ARCVAE)
    vae.decoder_sampling = _sampler()
    vae.latent_dim = 4
    with pytest.raises(ValueError):
        vae.generate(2, None, max_length=8, **kw)
