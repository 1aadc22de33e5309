"""Argument errors of the global-norm clip's entry points (csrc/clip.hip) are return codes checked on the host before any
launch (no device needed); the size query returns the documented partial counts; the CLI and the trainer expose the mode."""
import ctypes as C
import math

import pytest

ERR_ARG = -1
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call below is refused on the host before any launch


def _lib():
    from arcvae_hip import _lib
    return _lib.load()


def _partials(n):
    cnt = C.c_long(-1)
    rc = _lib().arcvae_grad_sumsq_partials(C.c_long(n), C.byref(cnt))
    return rc, cnt.value


def test_partials_size_query():
    # P = min(256, ceil(ceil(n / 4) / 256))
    for n, p in ((1, 1), (4, 1), (1024, 1), (1025, 2), (2048, 2), (4096, 4), (65536, 64), (262144, 256), (262145, 256),
                 (1324288, 256), (10_000_000, 256)):
        assert _partials(n) == (0, p), n
    for n in (0, -1):
        assert _partials(n)[0] == ERR_ARG
    assert _lib().arcvae_grad_sumsq_partials(C.c_long(16), None) == ERR_ARG


def _sumsq(g=FAKE, n=4096, part=FAKE, cap=4):
    return _lib().arcvae_grad_sumsq(g, C.c_long(n), part, C.c_long(cap), None)


def test_sumsq_argument_errors():
    assert _sumsq(g=None) == ERR_ARG
    assert _sumsq(part=None) == ERR_ARG
    assert _sumsq(n=0) == ERR_ARG and _sumsq(n=-5) == ERR_ARG
    assert _sumsq(n=4096, cap=3) == ERR_ARG                  # needs 4
    assert _sumsq(n=10_000_000, cap=255) == ERR_ARG          # needs 256
    assert _sumsq(n=1, cap=0) == ERR_ARG


def _clipped(p=FAKE, g=FAKE, m=FAKE, v=FAKE, n=1024, part=FAKE, npart=4, max_norm=1.0):
    return _lib().arcvae_adam_update_clipped(p, g, m, v, C.c_long(n), 2e-4, 0.9, 0.999, 1e-8, None, None, part,
                                             C.c_long(npart), max_norm, None, None)


def _finalize(p=FAKE, g=FAKE, m=FAKE, v=FAKE, n=1024, rowloss=FAKE, B=8, stats=FAKE, scalars=FAKE, Z=8, T=12, part=FAKE,
              npart=4, max_norm=1.0):
    return _lib().arcvae_adam_update_finalize_clipped(p, g, m, v, C.c_long(n), 2e-4, 0.9, 0.999, 1e-8, None, None, rowloss,
                                                      B, stats, scalars, Z, T, part, C.c_long(npart), max_norm, None)


BAD_NORMS = (0.0, -1.0, math.inf, -math.inf, math.nan)


def test_clipped_update_argument_errors():
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(part=None), dict(n=0), dict(n=-1),
               dict(npart=0), dict(npart=4097)):
        assert _clipped(**kw) == ERR_ARG, kw
    for bad in BAD_NORMS:
        assert _clipped(max_norm=bad) == ERR_ARG, bad


def test_clipped_finalize_argument_errors():
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(part=None), dict(rowloss=None), dict(stats=None),
               dict(scalars=None), dict(n=0), dict(B=0), dict(Z=0), dict(T=0), dict(npart=0), dict(npart=4097)):
        assert _finalize(**kw) == ERR_ARG, kw
    for bad in BAD_NORMS:
        assert _finalize(max_norm=bad) == ERR_ARG, bad


def test_host_side_clip_norm_checks():
    from arcvae_hip.engine import check_clip_norm
    assert check_clip_norm(None) is None
    assert check_clip_norm(1) == 1.0 and isinstance(check_clip_norm(1), float)
    for bad in BAD_NORMS:
        with pytest.raises(ValueError):
            check_clip_norm(bad)


def test_train_cli_lists_the_clip_mode(capsys):
    import train
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--help"])
    out = capsys.readouterr().out
    assert "--grad_clip_mode" in out and "global_norm" in out
    args = train.build_parser().parse_args([])
    assert args.grad_clip_mode == "reference" and args.grad_clip == 1.0
    assert train.build_parser().parse_args(["--grad_clip_mode", "global_norm"]).grad_clip_mode == "global_norm"
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--grad_clip_mode", "torch"])


def test_trainer_refuses_an_unknown_clip_mode(tmp_path):
    from trainer import ARCVAETrainerWithLoss

    class Stub(ARCVAETrainerWithLoss):
        def _make_engine(self, encoder, decoder):
            return None

        def _rank_world(self):
            return 0, 1

    with pytest.raises(ValueError, match="grad_clip_mode"):
        Stub(None, None, None, None, checkpoint_dir=str(tmp_path / "a"), grad_clip_mode="torch")
    ref = Stub(None, None, None, None, checkpoint_dir=str(tmp_path / "b"))
    assert ref.clip_norm is None and "grad_norm" not in ref.history
    on = Stub(None, None, None, None, checkpoint_dir=str(tmp_path / "c"), grad_clip=0.5, grad_clip_mode="global_norm")
    assert on.clip_norm == 0.5 and on.history["grad_norm"] == []
    off = Stub(None, None, None, None, checkpoint_dir=str(tmp_path / "d"), grad_clip=0.0, grad_clip_mode="global_norm")
    assert off.clip_norm is None and "grad_norm" not in off.history
