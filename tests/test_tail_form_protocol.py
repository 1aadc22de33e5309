"""Model check of the gate protocol in the tail form ARCVAE_TAIL_FORM=1 (engine._encoder_backward_gated, quiet regime): side
accumulates one token table over the chunks and folds it once, main forms the last chunk's layer GEMMs behind its own
sweep, aux's last segment only waits and reports.  Recorder and replays are those of tests/test_gate_protocol.py; the
plan here says `quiet`.  No GPU needed."""
import pytest

import test_gate_protocol as P
from test_gate_protocol import E, _record_step, _replay, _replay_first_step


class _QuietPlan(P._Plan):
    quiet = True


PIECES = {1: {"wh", "wx"}, 2: {"table"}, 3: {"wh", "wx", "table"}, 4: {"wx"}, 5: {"wh", "wx"}, 6: {"wx", "table"},
          7: {"wh", "wx", "table"}, 8: {"wh"}}


def _owners(ops, streams):
    done = {}
    for s in streams:
        for op in ops[s]:
            if op[0] == "wgrad":
                for b in PIECES[op[2]]:
                    assert (op[1], b) not in done, (op[1], b)      # every (chunk, piece) exactly once
                    done[(op[1], b)] = s.name
    return done


@pytest.mark.parametrize("dp", [False, True])
@pytest.mark.parametrize("T,L,fractions", [(128, 2, (0.7, 1.0)), (128, 2, (0.8, 1.0)), (12, 2, (0.7, 1.0)), (9, 1, (0.5, 1.0)),
                                           (20, 2, (0.7, 1.0)), (128, 2, (0.3, 0.6, 0.85, 1.0))])
def test_tail_form_1_never_blocks_and_swaps_main_and_side(T, L, fractions, dp, monkeypatch):
    monkeypatch.setattr(P, "_Plan", _QuietPlan)
    monkeypatch.setattr(E, "_tables_on_main", lambda plan, ws: True)
    env = {"ARCVAE_TAIL_FORM": "1"}
    ops, streams, nc = _record_step(T, L, fractions, True, env, monkeypatch, dp)
    assert nc >= 2
    ops1, streams1, _ = _record_step(T, L, fractions, True, env, monkeypatch, dp, first_step=True)
    _replay_first_step(ops1, streams1, _record_step.host)          # the eager, synchronising first step does not block for good
    steps = 5
    flags, advanced = _replay(ops, streams, steps)                  # asserts: no deadlock, no piece ahead of its sweep chunk
    G = E.Gates
    assert flags[G.P] == steps * G.STRIDE
    assert flags[G.R] == 2 * steps and flags[G.NM] == steps
    assert flags[G.NS] == steps and flags[G.NA] == steps
    assert flags[G.D] == steps
    assert flags[G.HG] == steps
    if dp:
        assert len(_replay.reduced_early) == steps and all(_replay.reduced_early)
        assert len(_replay.heads_reduced_early) == steps and all(_replay.heads_reduced_early)
    assert all(v == 1 for v in advanced.values())
    done = _owners(ops, streams)
    assert len(done) == 3 * nc
    last = nc - 1
    assert done[(last, "wh")] == "main" and done[(last, "wx")] == "main" and done[(last, "table")] == "side"
    for c in range(nc - 1):                                         # earlier chunks: layers on aux beside the sweep, table on side
        assert done[(c, "wh")] == "aux" and done[(c, "wx")] == "aux" and done[(c, "table")] == "side"
    main = streams[0]
    kinds = [op[0] for op in ops[main]]
    assert "wait" not in kinds[:kinds.index("wgrad")]              # no cross-stream wait in front of main's tail launch


@pytest.mark.parametrize("env", [{"ARCVAE_TAIL_FORM": "0"}, {"ARCVAE_TAIL_FORM": "1", "ARCVAE_WX_ON_SIDE": "1"},
                                 {"ARCVAE_TAIL_FORM": "1", "ARCVAE_TABLE_ON_SIDE": "0"}])
def test_other_settings_keep_form_0(env, monkeypatch):
    """Knob 0, and form 1 asked for where side carries the dWx GEMMs or not every chunk's table: the quiet plan keeps the
    schedule in which the last chunk's layer GEMMs run on aux behind the gate and its table is not side's accumulated one."""
    monkeypatch.setattr(P, "_Plan", _QuietPlan)
    monkeypatch.setattr(E, "_tables_on_main", lambda plan, ws: True)
    ops, streams, nc = _record_step(128, 2, (0.7, 1.0), True, env, monkeypatch)
    _replay(ops, streams, 3)
    done = _owners(ops, streams)
    assert len(done) == 3 * nc
    assert done[(nc - 1, "wh")] == "aux"
    assert done[(nc - 1, "table")] == ("side" if env.get("ARCVAE_TABLE_ON_SIDE") == "0" else "main")
    assert done[(0, "table")] == ("aux" if env.get("ARCVAE_TABLE_ON_SIDE") == "0" else "side")
