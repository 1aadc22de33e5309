"""Which library entry points every sampler method runs, in what order and how often: the Python path from conditions to the
dense table and its decoders launches exactly this, so a change of that plumbing that adds, drops, reorders or repeats a launch
(a second dense pass, a capture that is taken again, a replay that launches from Python) fails here.  Recorded through
_lib.check, which every module's call() resolves at call time; the host-only *_ws_bytes size queries are left out."""
import numpy as np
import pytest
import torch

import arcvae_oracle as O
from helpers import TINY, lib, sampling_vae

pytestmark = pytest.mark.gpu
B, T = 3, 6
DENSE = "arcvae_dec_forward_dense"
GREEDY = "arcvae_dec_sample_chain"
TOPKP = "arcvae_dec_sample_chain_topkp"
LSE = "arcvae_dec_row_lse"


@pytest.fixture(scope="module")
def params():
    return O.init_params(TINY, 1234)


@pytest.fixture
def case(params, monkeypatch):
    """(a fresh sampler, conditions, the list the recorder appends to)"""
    samp = sampling_vae(TINY, params).decoder_sampling
    cond = np.random.RandomState(3).standard_normal((B, TINY.C)).astype(np.float32)
    L = lib()
    real, names = L.check, []

    def recorder(rc, what):
        if not what.endswith("_ws_bytes"):
            names.append(what)
        real(rc, what)

    monkeypatch.setattr(L, "check", recorder)
    return samp, cond, names


def _took(names):
    got = list(names)
    names.clear()
    return got


@pytest.mark.parametrize("kw,walk", [(dict(), GREEDY), (dict(sample=True, top_k=5, top_p=0.9), TOPKP)])
def test_captured_paths(case, kw, walk):
    """First call of a key: eagerly, then once more under capture; the replay launches nothing from Python; use_graph=False once."""
    samp, cond, names = case
    first = samp.generate_with_temperature(None, cond, max_length=T, **kw)
    assert _took(names) == [DENSE, walk, DENSE, walk]
    again = samp.generate_with_temperature(None, cond, max_length=T, **kw)
    assert _took(names) == []
    assert torch.equal(first, again)
    samp.generate_with_temperature(None, cond, max_length=T, use_graph=False, **kw)
    assert _took(names) == [DENSE, walk]
    assert len(samp._graphs) == 1


def test_eager_greedy_on_a_fresh_sampler(case):
    samp, cond, names = case
    samp.generate_with_temperature(None, cond, max_length=T, use_graph=False)
    assert _took(names) == [DENSE, GREEDY]


def test_categorical_is_eager(case):
    samp, cond, names = case
    for _ in range(2):
        samp.generate_with_temperature(None, cond, max_length=T, sample=True)
        assert _took(names) == [DENSE, "arcvae_dec_sample_chain_categorical"]


@pytest.mark.parametrize("method,kw,last", [("generate_beam", dict(z=None), "arcvae_dec_beam_search"),
                                            ("generate_map", dict(z=None), "arcvae_dec_viterbi"),
                                            ("generate_kbest", dict(z=None), "arcvae_dec_kbest"),
                                            ("token_marginals", dict(), "arcvae_dec_chain_marginals")])
def test_table_decoders(case, method, kw, last):
    samp, cond, names = case
    getattr(samp, method)(conditions=cond, max_length=T, **kw)
    assert _took(names) == [DENSE, LSE, last]


def test_sequence_log_prob(case):
    samp, cond, names = case
    tokens = np.random.RandomState(4).randint(0, TINY.V, size=(B, T)).astype(np.int32)
    samp.decoder.sequence_log_prob(tokens, cond)
    assert _took(names) == [DENSE, LSE, "arcvae_dec_sequence_logprob"]
