"""Model check of the device-side gate protocol (engine._encoder_backward_gated + the decoder's gate + the join): the
gate operations each stream would enqueue are recorded through a fake `Gates`, then several steps are replayed with
the device semantics of csrc/misc.hip (a wait passes when flag >= steps * stride + offset and may advance `steps`; a
stream runs its operations in order).  Checked: no stream ever blocks for good, every ticket counter advances exactly
once per step, and a chunk's gradient pieces never run before the sweep chunk that completes their time range.
No GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlx-vae_amd"))

import torch  # noqa: E402
from arcvae_hip import engine as E  # noqa: E402


class _Stream:
    def __init__(self, name):
        self.name = name

    def wait_stream(self, other):
        raise AssertionError("the gated path must not fall back to an event wait here")


class _Recorder(E.Gates):
    """Records gate operations instead of launching them."""

    def __init__(self):  # no device memory
        self.ops = {}
        self.cur = None

    def signal(self, w, add=1):
        self.ops[self.cur].append(("signal", w, add))

    def wait(self, w, steps, stride, offset, advance=False):
        self.ops[self.cur].append(("wait", w, steps, stride, offset, advance))

    def word(self, i):
        return ("word", i)

    def note(self, *what):
        self.ops[self.cur].append(what)


class _Plan:
    def __init__(self, g, T, L, fractions, persistent):
        self.g, self.persistent = g, persistent
        self.chunks = E.EncoderBackwardPlan.chunk_schedule(T, L, fractions)

    def heads(self, phase):
        self.g.note("heads", phase)             # 1: the dcomb chain (main, in front of the sweep); 2: the heads' parameter gradients

    def sweep(self, s0, s1, start_signal=None, chunk_index=0):
        c = [i for i, ch in enumerate(self.chunks) if ch[0] == s0][0]
        if start_signal is not None:            # raised by the first launch of the chunk when it starts
            assert start_signal == ("word", E.Gates.P if c > 0 else E.Gates.H)   # chunk 0: "the BPTT sweep has started"
            self.g.note("signal", start_signal[1], 1)
        self.g.note("sweep_done", c)

    def wgrad(self, t_lo, t_hi, first, last, parts=3, table=None):
        c = [i for i, ch in enumerate(self.chunks) if ch[2] == t_lo and ch[3] == t_hi][0]
        if parts & 15:
            self.g.note("wgrad", c, parts & 15)     # bits 4, 5, 8 choose kernels / workspaces / the zero fill, not pieces


def _record_step(T, L, fractions, persistent, env, monkeypatch, dp=False, first_step=False):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = _Recorder()
    main, side, aux = _Stream("main"), _Stream("side"), _Stream("aux")
    g.ops = {s: [] for s in (main, side, aux)}
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: main)
    plan = _Plan(g, T, L, fractions, persistent)
    nc = len(plan.chunks)

    host = []                                    # host enqueue order: (stream, ops enqueued on it so far, first use synchronises?)

    def run(key, fn, stream):
        g.cur = stream
        fn()
        host.append((stream, len(g.ops[stream]), True))     # a recorded segment: eager + stream.synchronize() on its first use

    def prologue():                              # the forward sweep raises signal #1 when it starts
        g.note("signal", E.Gates.P, 1)

    def decoder_after_main():                    # StepEngine.enqueue_decoder(gate=(g, nc < 2))
        g.cur = side
        g.wait(E.Gates.P, E.Gates.NS, E.Gates.STRIDE, 1, advance=nc < 2)
        g.signal(E.Gates.D, 1)

    if dp:                                       # dp.py: forward and decoder are enqueued on their own, the backward after them
        g.cur = main
        prologue()
        host.append((main, len(g.ops[main]), True))          # gated:enc_fwd
        decoder_after_main()
        host.append((side, len(g.ops[side]), True))          # gated:dec_all
        g.cur = side                             # EngineOps (gated): CE sum, all-reduce of [dec.grad | CE sum] and the decoder's
        g.note("dec_reduce")                     # Adam are side's NEXT operations (stream order: no gate, no event)
        # round 4: behind them, still on side, the encoder HEADS' bucket -- gated on "aux has formed those gradients" (word HG;
        # dp.EngineOps.seam_buckets: offset 0 when the decoder's own gate already advanced side's ticket, i.e. single-chunk sweeps).
        # A driver's FIRST step (it records the segments) issues it behind the backward instead: EngineOps.seam_issue_early.
        if not first_step:
            g.wait(E.Gates.HG, E.Gates.NS, 1, 0 if nc < 2 else 1)
            g.note("heads_reduce")
        host.append((side, len(g.ops[side]), False))         # plain launches and enqueued collectives: the host does not wait
        E._encoder_backward_gated(plan, None, aux, side, run, None, None, g)
        if first_step:
            g.cur = side
            g.wait(E.Gates.HG, E.Gates.NS, 1, 0)
            g.note("heads_reduce")
            host.append((side, len(g.ops[side]), False))
    else:
        E._encoder_backward_gated(plan, None, aux, side, run, prologue, decoder_after_main, g)
    g.cur = main
    if nc >= 2:
        g.join()                                 # enqueue_finish / _join_gated
    host.append((main, len(g.ops[main]), True))
    _record_step.host = host
    return g.ops, (main, side, aux), nc


def _replay_first_step(ops, streams, host):
    """The FIRST step of a driver: every recorded segment runs eagerly, the host then waits for that segment's stream to drain
    (SegmentRunner: stream.synchronize()) and the capture that follows begins with a DEVICE-WIDE synchronize (torch.cuda.graph) --
    so every gate pending on ANY stream at that point must be releasable by what the host has enqueued so far.  Replays the
    host's enqueue order with that rule; returns normally iff the host never blocks for good."""
    flags, pc, limit = {}, {s: 0 for s in streams}, {s: 0 for s in streams}

    def advance():
        moved = True
        while moved:
            moved = False
            for s in streams:
                while pc[s] < limit[s]:
                    op = ops[s][pc[s]]
                    if op[0] == "wait":
                        _, w, cnt, stride, offset, adv = op
                        if flags.get(w, 0) < flags.get(cnt, 0) * stride + offset:
                            break
                        if adv:
                            flags[cnt] = flags.get(cnt, 0) + 1
                    elif op[0] == "signal":
                        flags[op[1]] = flags.get(op[1], 0) + op[2]
                    pc[s] += 1
                    moved = True

    for s, n, sync in host:
        limit[s] = max(limit[s], n)
        advance()
        if sync:
            for q in streams:
                assert pc[q] == limit[q], (f"first step: the host synchronises the device at a segment of {s.name} while {q.name} sits "
                                           f"behind {ops[q][pc[q]]} -- nothing enqueued so far releases it")
    assert all(pc[s] == len(ops[s]) for s in streams)


def _replay(ops, streams, steps):
    main, side, aux = streams
    flags = {}
    pc = {s: 0 for s in streams}
    prog = {s: ops[s] * steps for s in streams}
    per = {s: len(ops[s]) for s in streams}
    sweeps_done = set()                          # (step, chunk)
    heads1_done = set()                          # steps whose dcomb chain (heads phase 1) has run
    heads2_done = set()                          # steps whose heads' parameter gradients (phase 2, on aux) are formed
    heads_reduced_early = []
    advanced = {}
    reduced_early = []
    nc_last = max([op[1] for op in ops[main] if op[0] == "sweep_done"], default=0)
    # adversarial schedule: side and aux run as far as their gates let them, main then executes ONE operation -- a
    # gradient piece that can start too early will
    while any(pc[s] < len(prog[s]) for s in streams):
        moved = False
        for s in (side, aux, main):
            budget = 1 if s is main else 1 << 30
            while pc[s] < len(prog[s]) and budget > 0:
                budget -= 1
                op = prog[s][pc[s]]
                step = pc[s] // per[s] if per[s] else 0
                if op[0] == "wait":
                    _, w, cnt, stride, offset, adv = op
                    if flags.get(w, 0) < flags.get(cnt, 0) * stride + offset:
                        break
                    if adv:
                        flags[cnt] = flags.get(cnt, 0) + 1
                        advanced[(cnt, step)] = advanced.get((cnt, step), 0) + 1
                elif op[0] == "signal":
                    flags[op[1]] = flags.get(op[1], 0) + op[2]
                elif op[0] == "sweep_done":
                    sweeps_done.add((step, op[1]))
                elif op[0] == "heads":
                    if op[1] == 1:
                        heads1_done.add(step)
                    else:                        # the heads' parameter gradients read what the dcomb chain of THIS step wrote
                        assert step in heads1_done, f"{s.name}: heads' parameter gradients before the dcomb chain (step {step})"
                        heads2_done.add(step)
                elif op[0] == "heads_reduce":        # dp: the heads' bucket is reduced once THIS step's gradients are formed ...
                    assert step in heads2_done, f"{s.name}: heads' bucket reduced before its gradients were formed (step {step})"
                    # ... and before main has JOINED this step (its reduce must be inside what the join covers: side reports on R
                    # behind it in stream order).  (In this model a chunk is one operation and the heads' gradients are formed behind
                    # chunk 0, so "before the sweep's last chunk is done" cannot be asked here as it is of the decoder's bucket.)
                    heads_reduced_early.append(flags.get(E.Gates.NM, 0) <= step)
                elif op[0] == "wgrad":
                    assert (step, op[1]) in sweeps_done, f"{s.name}: gradients of chunk {op[1]} before its sweep (step {step})"
                elif op[0] == "dec_reduce":          # the decoder's bucket is reduced beside the sweep: before its LAST chunk is done
                    reduced_early.append((step, nc_last) not in sweeps_done)
                pc[s] += 1
                moved = True
        assert moved, "deadlock: " + ", ".join(f"{s.name} at {prog[s][pc[s]] if pc[s] < len(prog[s]) else 'end'}" for s in streams)
    _replay.reduced_early = reduced_early
    _replay.heads_reduced_early = heads_reduced_early
    return flags, advanced


@pytest.mark.parametrize("env", [{}, {"ARCVAE_TABLE_ON_SIDE": "0"}, {"ARCVAE_WX_ON_SIDE": "1"}, {"ARCVAE_WX_ON_SIDE": "0"},
                                 {"ARCVAE_HEADS_EARLY": "1"}])
@pytest.mark.parametrize("persistent", [False, True])
@pytest.mark.parametrize("T,L,fractions", [(128, 2, (0.3, 0.6, 0.85, 1.0)), (128, 2, (0.63, 1.0)), (12, 2, (0.63, 1.0)),
                                           (40, 4, (0.1, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0)), (9, 1, (0.5, 1.0)), (5, 3, (0.3, 0.6, 0.85, 1.0)),
                                           (128, 2, (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 1.0))])
@pytest.mark.parametrize("dp", [False, True])
@pytest.mark.parametrize("tables_on_main", [False, True])
def test_gated_backward_never_blocks_and_keeps_its_order(T, L, fractions, persistent, env, dp, tables_on_main, monkeypatch):
    # tables_on_main: every chunk folds its own token table, main forms the last chunk's behind its own sweep (round 2)
    monkeypatch.setattr(E, "_tables_on_main", lambda plan, ws: tables_on_main)
    ops, streams, nc = _record_step(T, L, fractions, persistent, env, monkeypatch, dp)
    host_early = _record_step.host
    assert nc >= 2
    ops1, streams1, _ = _record_step(T, L, fractions, persistent, env, monkeypatch, dp, first_step=True)
    _replay_first_step(ops1, streams1, _record_step.host)      # the eager, synchronising first step does not block for good
    if dp:   # ... and it would, had the first step put the heads' gate on side ahead of the backward's enqueue (seen on the GPU: 15 s, ERR)
        with pytest.raises(AssertionError, match="first step"):
            _replay_first_step(ops, streams, host_early)
    steps = 5
    flags, advanced = _replay(ops, streams, steps)
    G = E.Gates
    assert flags[G.P] == steps * G.STRIDE                      # main: exactly STRIDE signals per step
    assert flags[G.R] == 2 * steps and flags[G.NM] == steps    # aux and side report once each; main joins once
    assert flags[G.NS] == steps and flags[G.NA] == steps       # every waiter's ticket counter: once per step
    assert flags[G.D] == steps                                 # decoder segments reported
    assert flags[G.HG] == steps                                # aux raised "heads' gradients formed" once per step
    if dp:   # the decoder's all-reduce is issued (and can run) before the BPTT sweep has finished, in every step
        assert len(_replay.reduced_early) == steps and all(_replay.reduced_early)
        # ... the encoder heads' (second bucket) never before aux has formed those gradients, always inside the join
        assert len(_replay.heads_reduced_early) == steps and all(_replay.heads_reduced_early)
    assert all(v == 1 for v in advanced.values())
    # every chunk's gradient pieces are formed exactly once per step, between the streams
    done = {}
    for s in streams:
        for op in ops[s]:
            if op[0] == "wgrad":
                c, parts = op[1], op[2]
                bits = {1: {"wh", "wx"}, 2: {"table"}, 3: {"wh", "wx", "table"}, 4: {"wx"}, 5: {"wh", "wx"}, 6: {"wx", "table"},
                        7: {"wh", "wx", "table"}, 8: {"wh"}}[parts]
                for b in bits:
                    assert (c, b) not in done, (c, b)
                    done[(c, b)] = s.name
    assert len(done) == 3 * nc
