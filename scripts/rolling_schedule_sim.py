# coding: utf-8
"""Decoder steps of rolling admission against rigid waves, on the host (no GPU): the scheduler of
synthesis.RollingSynthesizer (decode_program.RollingSchedule) driven by known per-utterance step counts.
Default: the LJSpeech-shaped length distribution of SURVEY 8d cfg2 (mel frames ~ N(566, 180) clipped to [120, 870],
r = 4), 256 utterances, seed 1234, 64 slots, chunks of 8 steps.
Usage: python scripts/rolling_schedule_sim.py [n_utterances [slots [chunk [seed]]]]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from deepvoice3_pytorch_amd.decode_program import cfg2_step_counts, simulate_rolling, simulate_waves
    args = [int(a) for a in sys.argv[1:]]
    n, slots, chunk, seed = (args + [256, 64, 8, 1234][len(args):])[:4]
    counts = cfg2_step_counts(n, seed)
    rolling, sch = simulate_rolling(counts, slots, chunk)
    waves, waves_chunked = simulate_waves(counts, slots), simulate_waves(counts, slots, chunk)
    useful = sum(counts)
    print(json.dumps(dict(
        utterances=n, slots=slots, chunk=chunk, seed=seed, item_steps=dict(min=min(counts), max=max(counts), mean=useful / n),
        rolling_steps=rolling, wave_steps=waves, wave_steps_whole_chunks=waves_chunked,
        step_ratio=rolling / waves, step_ratio_whole_chunks=rolling / waves_chunked,
        slot_steps_used=dict(rolling=useful / (slots * rolling), waves=useful / (slots * waves)),
        lower_bound_steps=useful / slots), indent=1))


if __name__ == "__main__":
    main()
