"""Host side of the device-resident learning rate: argument errors of arcvae_adam_step (csrc/clip.hip) are return codes checked
before any launch (no device needed); the CLI lists the schedule flags; the trainer keeps its checkpoint keys without a
schedule and validates the schedule object it is given."""
import ctypes as C
import math

import pytest

ERR_ARG = -1
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call below is refused on the host before any launch


def _lib():
    from arcvae_hip import _lib
    return _lib.load()


def _step(p=FAKE, g=FAKE, m=FAKE, v=FAKE, n=1024, lr=FAKE, rowloss=None, B=0, stats=None, scalars=None, Z=0, T=0, part=None,
          npart=0, max_norm=0.0):
    return _lib().arcvae_adam_step(p, g, m, v, C.c_long(n), lr, 0.9, 0.999, 1e-8, None, None, rowloss, B, stats, scalars,
                                   Z, T, part, C.c_long(npart), max_norm, None)


FIN = dict(rowloss=FAKE, B=8, stats=FAKE, scalars=FAKE, Z=8, T=12)
CLIP = dict(part=FAKE, npart=4, max_norm=1.0, scalars=FAKE)
BAD_NORMS = (0.0, -1.0, math.inf, -math.inf, math.nan)


def test_symbol_is_bound():
    from arcvae_hip import _lib
    assert "arcvae_adam_step" in _lib.SIGNATURES and len(_lib.SIGNATURES["arcvae_adam_step"]) == 21
    assert _lib.load().arcvae_adam_step.argtypes is not None


@pytest.mark.parametrize("parts", [{}, FIN, CLIP, {**FIN, **CLIP}], ids=["plain", "finalize", "clipped", "finalize_clipped"])
def test_common_argument_errors(parts):
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(lr=None), dict(n=0), dict(n=-1)):
        assert _step(**{**parts, **kw}) == ERR_ARG, kw


@pytest.mark.parametrize("clip", [{}, CLIP], ids=["finalize", "finalize_clipped"])
def test_finalize_part_argument_errors(clip):
    for kw in (dict(stats=None), dict(scalars=None), dict(B=0), dict(B=-1), dict(Z=0), dict(Z=-2), dict(T=0), dict(T=-1)):
        assert _step(**{**FIN, **clip, **kw}) == ERR_ARG, kw


@pytest.mark.parametrize("fin", [{}, FIN], ids=["clipped", "finalize_clipped"])
def test_clip_part_argument_errors(fin):
    for kw in (dict(scalars=None), dict(npart=0), dict(npart=-1), dict(npart=4097)):
        assert _step(**{**fin, **CLIP, **kw}) == ERR_ARG, kw
    for bad in BAD_NORMS:
        assert _step(**{**fin, **CLIP, "max_norm": bad}) == ERR_ARG, bad


def test_host_side_rate_checks():
    """StepEngine.set_rate refuses before it touches the device (checked here on an engine-less call: the value test comes
    first)."""
    from arcvae_hip.engine import LR_DEVICE, DeviceRate, StepEngine, lr_key
    for bad in (-1e-4, math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="learning rate"):
            StepEngine.set_rate(None, None, bad)
    # capture keys: the value for a by-value rate (as before), one fixed marker for every device rate
    assert lr_key(2e-4) == 2e-4 and isinstance(lr_key(1), float)
    assert lr_key(DeviceRate(None)) == LR_DEVICE == lr_key(DeviceRate(None))


def test_train_cli_lists_the_schedule_flags(capsys):
    import train
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--help"])
    out = capsys.readouterr().out
    for flag in ("--lr_schedule", "--warmup_steps", "--min_lr_ratio"):
        assert flag in out
    for kind in ("constant", "linear", "cosine"):
        assert kind in out
    args = train.parse_args([])
    assert args.lr_schedule is None and args.warmup_steps is None and args.min_lr_ratio is None
    args = train.parse_args(["--lr_schedule", "cosine", "--warmup_steps", "7", "--min_lr_ratio", "0.25"])
    assert (args.lr_schedule, args.warmup_steps, args.min_lr_ratio) == ("cosine", 7, 0.25)
    with pytest.raises(SystemExit):
        train.parse_args(["--lr_schedule", "exponential"])
    for alone in (["--warmup_steps", "5"], ["--min_lr_ratio", "0.1"]):
        with pytest.raises(SystemExit):
            train.parse_args(alone)
        assert "--lr_schedule" in capsys.readouterr().err
    # the flags combine with the other extensions
    args = train.parse_args(["--lr_schedule", "linear", "--grad_clip_mode", "global_norm", "--property_predictor_hidden", "32",
                             "--world_size", "2"])
    assert args.lr_schedule == "linear" and args.grad_clip_mode == "global_norm" and args.world_size == 2


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


def test_trainer_checkpoint_keys_and_schedule_validation(tmp_path):
    import json

    import numpy as np
    from lr_schedule import LRSchedule

    plain, cls = _stub(tmp_path, "a")
    assert plain.lr_schedule is None
    plain.save_checkpoint(epoch=0)
    assert set(cls.saved) == {"epoch", "history_json", "learning_rate"}          # today's keys, nothing else
    assert "global_step" not in cls.saved and "lr_schedule_json" not in cls.saved

    for bad in ("cosine", 3, dict(kind="cosine"), lambda s: 1e-4):
        with pytest.raises(ValueError, match="lr_schedule"):
            _stub(tmp_path, "b", lr_schedule=bad)

    sch = LRSchedule(2e-4, "cosine", warmup_steps=2, total_steps=6, min_lr_ratio=0.1)
    on, cls = _stub(tmp_path, "c", lr_schedule=sch)
    assert on.global_step == 0 and on.history["learning_rate"] == []
    on.global_step = 5
    on.save_checkpoint(epoch=1)
    assert int(cls.saved["global_step"]) == 5
    assert json.loads(str(cls.saved["lr_schedule_json"])) == sch.state()
    # ... and load_checkpoint restores both, into a trainer whose own schedule was built afresh
    path = tmp_path / "ck.npz"
    np.savez(str(path), **cls.saved)
    fresh, _ = _stub(tmp_path, "d", lr_schedule=LRSchedule(2e-4, "cosine", warmup_steps=2, min_lr_ratio=0.1))
    assert fresh.load_checkpoint(str(path)) == 1
    assert fresh.global_step == 5 and fresh.lr_schedule.state() == sch.state()
    assert fresh.lr_schedule.lr(5) == sch.lr(5)
    # a one-rate trainer reading that checkpoint stays a one-rate trainer
    plain2, _ = _stub(tmp_path, "e")
    plain2.load_checkpoint(str(path))
    assert plain2.lr_schedule is None and plain2.global_step == 0
