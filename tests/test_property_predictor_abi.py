"""Argument errors of the property predictor's entry points are return codes (no launch, no device needed), and the
predictor is refused together with data parallelism before anything runs."""
import ctypes as C
from types import SimpleNamespace

import pytest

ERR_ARG = -1
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call below is refused on the host before any launch


def _lib():
    from arcvae_hip import _lib
    return _lib.load()


def _ws_floats(B, Z, Cn, Hp):
    n = C.c_long(-1)
    rc = _lib().arcvae_prop_ws_floats(B, Z, Cn, Hp, C.byref(n))
    return rc, n.value


def test_workspace_size_query():
    assert _ws_floats(64, 128, 1, 64) == (0, 64 * (2 * 64 + 1 + 1))
    assert _ws_floats(2048, 512, 8, 256) == (0, 2048 * (2 * 256 + 8 + 1))
    for bad in ((0, 128, 1, 64), (64, 0, 1, 64), (64, 513, 1, 64), (64, 128, 0, 64), (64, 128, 9, 64), (64, 128, 1, 0),
                (64, 128, 1, 257)):
        assert _ws_floats(*bad)[0] == ERR_ARG, bad


def _backward(ws_floats, B=64, Z=128, Cn=1, Hp=64, cond=FAKE):
    return _lib().arcvae_prop_backward(FAKE, cond, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE,
                                       ws_floats, B, Z, Cn, Hp, None)


def _wgrad(ws_floats, B=64, Z=128, Cn=1, Hp=64):
    return _lib().arcvae_prop_wgrad(FAKE, FAKE, ws_floats, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, B, Z, Cn, Hp, None)


def _forward(ws_floats, scalars, cond, B=64, Z=128, Cn=1, Hp=64, pred=FAKE):
    return _lib().arcvae_prop_forward(FAKE, cond, FAKE, FAKE, FAKE, FAKE, FAKE, pred, scalars, FAKE, ws_floats, B, Z, Cn,
                                      Hp, None)


def test_undersized_workspace_is_an_argument_error():
    need = _ws_floats(64, 128, 1, 64)[1]
    assert _backward(need - 1) == ERR_ARG
    assert _wgrad(need - 1) == ERR_ARG
    assert _forward(need - 1, FAKE, FAKE) == ERR_ARG


def test_bad_dimensions_are_argument_errors():
    need = _ws_floats(2048, 512, 8, 256)[1]
    assert _backward(need, Cn=9) == ERR_ARG
    assert _backward(need, Hp=0) == ERR_ARG
    assert _backward(need, Hp=257) == ERR_ARG
    assert _backward(need, Z=513) == ERR_ARG
    assert _backward(need, B=0) == ERR_ARG
    assert _wgrad(need, Cn=9) == ERR_ARG
    assert _forward(need, FAKE, FAKE, Hp=300) == ERR_ARG


def test_missing_condition_with_a_loss_requested_is_an_argument_error():
    need = _ws_floats(64, 128, 1, 64)[1]
    assert _forward(need, FAKE, None) == ERR_ARG        # scalars asked for, no cond
    assert _backward(need, cond=None) == ERR_ARG
    assert _forward(need, None, None, pred=None) == ERR_ARG   # nothing to compute


def test_engine_data_parallel_refuses_a_predictor_engine():
    from arcvae_hip.dp import EngineDataParallel
    with pytest.raises(ValueError, match="data parallelism"):
        EngineDataParallel(SimpleNamespace(prop=object()))


def test_train_cli_refuses_a_predictor_with_several_ranks():
    import train
    with pytest.raises(ValueError, match="data parallelism"):
        train.main(["--synthetic", "10", "--property_predictor_hidden", "8", "--world_size", "2"])
