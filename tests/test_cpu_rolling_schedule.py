# coding: utf-8
"""The host-side book of rolling admission (decode_program.RollingSchedule) and its simulation: no GPU, no model.

On the LJSpeech-shaped length distribution (SURVEY 8d cfg2, 256 utterances, seed 1234, 64 slots, chunks of 8 steps) the
simulation gives 704 decoder steps for rolling admission against 868 for four rigid waves of 64 run to each wave's
exact maximum (896 when a wave, too, runs whole chunks): a step ratio of 0.811 (0.786).  The utterances' own steps sum
to 36363, i.e. 568.2 steps of 64 full slots: rolling admission fills 80.7 % of the slot-steps it executes, the waves
65.5 %.  test_cfg2_rolling_beats_waves recomputes these figures and asserts the inequality, not the constants.
"""
import random

import pytest

from deepvoice3_pytorch_amd.decode_program import (RollingSchedule, cfg2_step_counts, simulate_rolling,
                                                   simulate_waves)


def _drive(counts, slots, chunk, arrivals=None):
    """run the schedule by hand the way RollingSynthesizer.poll does, checking the invariants after every round;
    arrivals: {round: [tickets submitted before that round]} (default: everything before round 0)"""
    sch = RollingSchedule(slots, chunk)
    arrivals = arrivals or {0: list(range(len(counts)))}
    submitted, admitted_order, t_off, retired = [], [], {}, {}
    rnd = 0
    while sch.pending() or any(r >= rnd for r in arrivals):
        for tk in arrivals.get(rnd, []):
            sch.submit(tk)
            submitted.append(tk)
        t_before = sch.t
        free_before = [s for s in range(slots) if sch.slot_ticket[s] is None]
        new = sch.admit()
        for tk, s in new:
            assert s in free_before, "slot %d double-booked" % s
            assert sch.slot_t_off[s] == t_before                        # t_off = the admission step
            t_off[tk] = t_before
            admitted_order.append(tk)
        assert len(set(s for _, s in new)) == len(new)
        busy = sch.busy()
        tickets = [sch.slot_ticket[s] for s in busy]
        assert len(set(tickets)) == len(tickets), "a ticket sits in two slots"
        if busy:
            sch.advance()
            for s in busy:
                tk = sch.slot_ticket[s]
                assert sch.steps_run(s) == sch.t - t_off[tk]
                if sch.steps_run(s) >= counts[tk]:
                    assert tk not in retired, "ticket %d retired twice" % tk
                    assert sch.retire(s) == tk
                    retired[tk] = sch.t
                    assert sch.slot_ticket[s] is None
        rnd += 1
        assert rnd < 100000
    return sch, submitted, admitted_order, t_off, retired


@pytest.mark.parametrize("slots,chunk,n", [(1, 1, 5), (4, 8, 12), (4, 3, 40), (64, 8, 256), (7, 5, 3)])
def test_schedule_invariants(slots, chunk, n):
    rng = random.Random(slots * 1000 + chunk * 10 + n)
    counts = [rng.randint(1, 60) for _ in range(n)]
    sch, submitted, admitted, t_off, retired = _drive(counts, slots, chunk)
    assert admitted == submitted == list(range(n))                       # first in, first out
    assert sorted(retired) == list(range(n))                             # every ticket retires, once (_drive: not twice)
    assert len(sch.log) == n and sorted(tk for tk, _, _, _ in sch.log) == list(range(n))
    for tk, slot, off, at in sch.log:
        assert off == t_off[tk] and at == retired[tk]
        assert off % chunk == 0 and at - off == -(-counts[tk] // chunk) * chunk      # whole chunks, no more than needed
    # no slot holds two tickets at once: a slot's occupancies are disjoint intervals of the global step
    for s in range(slots):
        iv = sorted((off, at) for _, slot, off, at in sch.log if slot == s)
        assert all(a[1] <= b[0] for a, b in zip(iv[:-1], iv[1:]))
    # the steps executed are the simulation's
    steps, sim = simulate_rolling(counts, slots, chunk)
    assert steps == sch.steps == sch.t
    assert sim.log == sch.log


def test_late_arrivals_are_admitted_between_chunks():
    counts = [20, 3, 9, 30, 4, 4]
    arrivals = {0: [0, 1], 1: [2], 4: [3, 4, 5]}
    sch, submitted, admitted, t_off, retired = _drive(counts, 2, 4, arrivals)
    assert admitted == submitted == [0, 1, 2, 3, 4, 5]
    assert t_off[2] == 4                 # ticket 1 (3 steps) freed its slot after the first chunk; 2 arrived in time for it
    assert t_off[3] >= 16                # arrived before round 4 = global step 16 (or later when both slots are taken)
    assert sorted(retired) == [0, 1, 2, 3, 4, 5]
    assert sch.steps == sch.t


def test_schedule_refuses_nonsense():
    with pytest.raises(ValueError):
        RollingSchedule(0, 8)
    with pytest.raises(ValueError):
        RollingSchedule(4, 0)
    with pytest.raises(RuntimeError):
        RollingSchedule(2, 2).retire(1)
    with pytest.raises(ValueError):
        simulate_rolling([3, 0], 2, 2)


def test_wave_count():
    assert simulate_waves([5, 9, 2, 7, 1], 2) == 9 + 7 + 1
    assert simulate_waves([5, 9, 2, 7, 1], 2, chunk=4) == 12 + 8 + 4
    assert simulate_waves([], 4) == 0


def test_cfg2_rolling_beats_waves():
    """cfg2 lengths, 256 utterances, seed 1234, 64 slots, chunk 8: rolling admission executes strictly fewer decoder
    steps than waves of 64, even when a wave is charged only its exact maximum (no chunk rounding).  The simulation's
    figures (printed; quoted in this file's docstring and DESIGN.md 3.6c): rolling 704, waves 868 (896 in whole
    chunks), ratio 0.811 (0.786)."""
    counts = cfg2_step_counts(256, 1234)
    assert len(counts) == 256 and min(counts) >= 30 and max(counts) <= 217
    rolling, sch = simulate_rolling(counts, 64, 8)
    waves, waves_chunked = simulate_waves(counts, 64), simulate_waves(counts, 64, 8)
    useful = sum(counts)
    print("cfg2: rolling %d steps, waves %d (%d in whole chunks), ratio %.3f (%.3f); slot-steps used %.3f vs %.3f" % (
        rolling, waves, waves_chunked, rolling / waves, rolling / waves_chunked, useful / (64.0 * rolling),
        useful / (64.0 * waves)))
    assert rolling < waves <= waves_chunked
    assert rolling * 64 >= useful                                         # no schedule does more than fill every slot
    assert len(sch.log) == 256
