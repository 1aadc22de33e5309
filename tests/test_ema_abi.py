"""Host side of the weight EMA: the two entry points of csrc/ema.hip are bound with the header's arity, their argument errors
are return codes checked before any launch (no device needed), the CLI lists the flags, and the trainer keeps its checkpoint
keys without an EMA and carries the EMA's state with one."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

ERR_ARG = -1
FAKE = 0x1000                    # never dereferenced: every call below is refused on the host before any launch
MAX_SEG = 4


def _lib():
    from arcvae_hip import _lib
    return _lib.load()


def _ptrs(vals):
    arr = (C.c_void_p * len(vals))(*vals)
    return C.cast(arr, C.POINTER(C.c_void_p)), arr


def _longs(vals):
    return (C.c_long * len(vals))(*vals)


def _update(a="ok", b="ok", n="ok", segments=2, omd=0.1):
    keep = []

    def arr(x, default):
        if x is None:
            return None
        p, k = _ptrs(default if x == "ok" else x)
        keep.append(k)
        return p
    nn = None if n is None else _longs([1024, 7, 5, 3] if n == "ok" else n)
    return _lib().arcvae_ema_update(arr(a, [FAKE] * MAX_SEG), arr(b, [FAKE] * MAX_SEG), nn, segments, omd, None, None, None)


def _swap(a="ok", b="ok", n="ok", segments=2):
    keep = []

    def arr(x, default):
        if x is None:
            return None
        p, k = _ptrs(default if x == "ok" else x)
        keep.append(k)
        return p
    nn = None if n is None else _longs([1024, 7, 5, 3] if n == "ok" else n)
    return _lib().arcvae_ema_swap(arr(a, [FAKE] * MAX_SEG), arr(b, [FAKE] * MAX_SEG), nn, segments, None)


def test_symbols_are_bound_with_the_headers_arity():
    from arcvae_hip import _lib
    assert len(_lib.SIGNATURES["arcvae_ema_update"]) == 8 and len(_lib.SIGNATURES["arcvae_ema_swap"]) == 5
    assert _lib.SIGNATURES["arcvae_ema_update"][:3] == [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_long)]
    assert _lib.SIGNATURES["arcvae_ema_update"][4] is C.c_double
    lib = _lib.load()
    assert lib.arcvae_ema_update.argtypes is not None and lib.arcvae_ema_swap.argtypes is not None
    assert _lib.EMA_MAX_SEGMENTS == MAX_SEG
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "arcvae_hip.h")).read()
    assert "#define ARCVAE_EMA_MAX_SEGMENTS 4" in header


@pytest.mark.parametrize("fn", [_update, _swap], ids=["update", "swap"])
def test_shared_argument_errors(fn):
    for kw in (dict(a=None), dict(b=None), dict(n=None), dict(segments=0), dict(segments=-1), dict(segments=MAX_SEG + 1),
               dict(n=[1024, 0, 5, 3]), dict(n=[-1, 7, 5, 3]), dict(n=[1024, -7, 5, 3]),
               dict(a=[FAKE, None, FAKE, FAKE]), dict(b=[None, FAKE, FAKE, FAKE]),
               dict(a=[FAKE, FAKE, FAKE, None], segments=4), dict(n=[1, 1, 1, 0], segments=4)):
        assert fn(**kw) == ERR_ARG, kw


def test_update_refuses_a_weight_outside_the_unit_interval():
    for bad in (0.0, -0.1, 1.0000001, 2.0, math.inf, -math.inf, math.nan):
        assert _update(omd=bad) == ERR_ARG, bad


def test_train_cli_lists_the_ema_flags(capsys):
    import train
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--help"])
    out = capsys.readouterr().out
    for flag in ("--ema_decay", "--ema_warmup", "--ema_eval"):
        assert flag in out
    args = train.parse_args([])
    assert args.ema_decay is None and args.ema_warmup is False and args.ema_eval is False
    args = train.parse_args(["--ema_decay", "0.999", "--ema_warmup", "--ema_eval"])
    assert (args.ema_decay, args.ema_warmup, args.ema_eval) == (0.999, True, True)
    args = train.parse_args(["--ema_decay", "0.9"])
    assert (args.ema_decay, args.ema_warmup, args.ema_eval) == (0.9, False, False)
    for alone in (["--ema_warmup"], ["--ema_eval"], ["--ema_warmup", "--ema_eval"]):
        with pytest.raises(SystemExit):
            train.parse_args(alone)
        assert "--ema_decay" in capsys.readouterr().err
    for bad in ("0", "1", "-0.1", "nan"):
        with pytest.raises(SystemExit):
            train.parse_args(["--ema_decay", bad])
        capsys.readouterr()
    # the flags combine with the other extensions
    args = train.parse_args(["--ema_decay", "0.99", "--lr_schedule", "cosine", "--grad_clip_mode", "global_norm",
                             "--property_predictor_hidden", "32"])
    assert args.ema_decay == 0.99 and args.lr_schedule == "cosine"


def _stub(tmp_path, name, **kw):
    from trainer import ARCVAETrainerWithLoss

    class Stub(ARCVAETrainerWithLoss):
        saved = None

        def _make_engine(self, encoder, decoder):
            return None

        def _rank_world(self):
            return 0, 1

        def _modules(self):
            return []

        @staticmethod
        def _save_checkpoint(checkpoint, path):
            Stub.saved = dict(checkpoint)

    return Stub(None, None, None, None, checkpoint_dir=str(tmp_path / name), **kw), Stub


def test_trainer_checkpoint_keys_and_ema_validation(tmp_path, capsys):
    plain, plain_cls = _stub(tmp_path, "a")
    assert plain.ema is None and plain.ema_eval is False
    plain.save_checkpoint(epoch=0)
    assert set(plain_cls.saved) == {"epoch", "history_json", "learning_rate"}    # today's keys, nothing else

    for bad in (0, 1, -0.1, 0.0, 1.0, math.nan, "0.9", True):
        with pytest.raises(ValueError, match="decay"):
            _stub(tmp_path, "b", ema_decay=bad)
    for alone in (dict(ema_warmup=True), dict(ema_eval=True), dict(ema_warmup=True, ema_eval=True)):
        with pytest.raises(ValueError, match="ema_decay"):
            _stub(tmp_path, "b", **alone)

    on, cls = _stub(tmp_path, "c", ema_decay=0.999, ema_warmup=True, ema_eval=True)
    assert on.ema is not None and on.ema_eval is True and on.ema.num_updates == 0
    assert on.ema.state() == {"decay": 0.999, "warmup": True, "num_updates": 0}
    on.ema.num_updates = 7
    on.save_checkpoint(epoch=2)
    assert set(cls.saved) == {"epoch", "history_json", "learning_rate", "ema_json"}
    assert json.loads(str(cls.saved["ema_json"])) == {"decay": 0.999, "warmup": True, "num_updates": 7}
    # ... and load_checkpoint restores it into a trainer whose own EMA was built afresh
    path = tmp_path / "ck.npz"
    np.savez(str(path), **cls.saved)
    fresh, _ = _stub(tmp_path, "d", ema_decay=0.999, ema_warmup=True)
    assert fresh.ema.num_updates == 0
    assert fresh.load_checkpoint(str(path)) == 2
    assert fresh.ema.num_updates == 7 and fresh.ema.state() == on.ema.state()
    assert fresh.ema.decay_at(7) == min(0.999, 8 / 17)
    # a trainer without an EMA reading that checkpoint stays one
    plain2, _ = _stub(tmp_path, "e")
    assert plain2.load_checkpoint(str(path)) == 2 and plain2.ema is None
    # an EMA trainer reading a checkpoint without an EMA restarts the average, and says so
    plain.save_checkpoint(epoch=4)
    path2 = tmp_path / "ck2.npz"
    np.savez(str(path2), **plain_cls.saved)
    again, _ = _stub(tmp_path, "f", ema_decay=0.9)
    again.ema.num_updates = 3
    capsys.readouterr()
    assert again.load_checkpoint(str(path2)) == 4 and again.ema.num_updates == 0
    assert "no weight EMA" in capsys.readouterr().out


def test_weight_ema_host_side_rules():
    from arcvae_hip.ema import WeightEMA
    for bad in (0, 1, -0.1, math.nan, "0.9", None):
        with pytest.raises(ValueError):
            WeightEMA({}, bad)
    with pytest.raises(ValueError, match="at most"):
        WeightEMA({str(i): None for i in range(MAX_SEG + 1)}, 0.9)
    ema = WeightEMA({}, 0.9, warmup=True)
    with ema.applied():
        with pytest.raises(RuntimeError):
            ema.update()
        with pytest.raises(RuntimeError):
            with ema.applied():
                pass
    ema.update()
    assert ema.num_updates == 1
    ema.load_state({"decay": 0.5, "warmup": False, "num_updates": 11})
    assert ema.state() == {"decay": 0.5, "warmup": False, "num_updates": 11}
