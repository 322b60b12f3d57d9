# coding: utf-8
"""Per-utterance synthesis, host side: the per-item stop rule (decode_program.item_stops) and the per-item valid
lengths (ops.ItemLengths).  No GPU."""
import pytest
import torch

from deepvoice3_pytorch_amd import ops
from deepvoice3_pytorch_amd.decode_program import item_stops


def _reference_stop(done_b, min_steps, max_steps):
    """the reference's B = 1 loop (deepvoice3.py:469-473): steps taken by one utterance"""
    t = 0
    while True:
        t += 1
        if (t > min_steps and done_b[t - 1] > 0.5) or t > max_steps:
            return t


@pytest.mark.parametrize("chunk", [1, 3, 8])
def test_item_stops_is_the_b1_rule_per_item(chunk):
    g = torch.Generator().manual_seed(0)
    B, min_steps, max_steps = 9, 4, 20
    done = torch.rand(max_steps + 1, B, generator=g)
    done[:, 0] = 0.0                  # never done: stops at max_steps + 1
    done[:, 1] = 1.0                  # always done: stops right after min_steps
    want = [_reference_stop(done[:, b].tolist(), min_steps, max_steps) for b in range(B)]
    stops, t, finished = [0] * B, 0, False
    while not finished:
        n = min(chunk, max_steps + 1 - t)
        finished = item_stops((done[t:t + n] > 0.5).tolist(), t, min_steps, max_steps, stops)
        t += n
        assert finished or t <= max_steps
    assert stops == want
    assert max(stops) <= t < max(stops) + chunk       # the batch ends in the chunk of its last item
    assert want[0] == max_steps + 1 and want[1] == min_steps + 1
    assert len(set(want)) >= 3


def test_item_stops_keeps_the_first_stop():
    stops = [0, 0]
    assert not item_stops([[True, False]], 5, 2, 10, stops)
    assert stops == [6, 0]
    assert item_stops([[False, True]], 6, 2, 10, stops)
    assert stops == [6, 7]


def test_item_lengths_axes():
    vl = ops.ItemLengths(torch.tensor([7, 3, 5]), 9)
    ptr, tail = vl.text()
    assert ptr.dtype == torch.int32 and ptr.tolist() == [7, 3, 5] and tail == 6
    with pytest.raises(RuntimeError):
        vl.axis_for(12)                                 # before the decode has ended
    vl.set_dec(torch.tensor([4, 6, 2]), 6)
    assert vl.dec()[1] == 4
    ptr, tail, mult = vl.axis_for(24)                   # decoder steps x r x converter upsampling
    assert ptr.tolist() == [4, 6, 2] and mult == 4 and tail == 16
    with pytest.raises(RuntimeError):
        vl.axis_for(13)
