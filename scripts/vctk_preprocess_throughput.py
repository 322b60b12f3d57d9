# coding: utf-8
"""Throughput of the waveform preparation in front of VCTK features (audio.resample_items -> dv3_resample_items_f32,
audio.trim_items -> dv3_trim_items_f32, audio.gather_spans) and the split of one B = 64 batch.

  launch        device-resident VCTK-shaped utterances (lengths uniform in 3..6 s at 48 kHz, seeded: silence, a
                speech-like stretch, silence) at 16, 64 and 256 per launch; the resampler 48 kHz -> 22.05 kHz
                (147 / 320) and the trim of its output.  Device time of one call = (one pair of events around 20
                back-to-back calls) / 20, median of 5 such windows after 3 warm-up calls.  Input samples per second =
                samples read / that time.  The resampler's arithmetic is 2 T flops per output, T = 2 H + 2 = 282 taps;
                its share of the vector FP32 peak (157.3 TFLOP/s) is that over the kernel time.
  per_batch_b64 one B = 64 batch from host arrays: packing into a pinned buffer (host clock), the host-to-device copy,
                the three preparation kernels incl. the one host read (audio.prepare_items' device part) and the
                feature launch (audio.features_items), by events; prepare_items + features_items as wall time.
Usage: python scripts/vctk_preprocess_throughput.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32 = 157.3e12
SRC, DST = 48000, 22050


def utterances(rng, n):
    out = []
    for L in (rng.uniform(3.0, 6.0, n) * SRC).astype(np.int64):
        lo, hi = int(0.1 * L), int(0.85 * L)
        t = np.arange(hi - lo) / float(SRC)
        x = 1e-4 * rng.randn(L)
        x[lo:hi] += 0.3 * np.sin(2 * np.pi * rng.uniform(100, 300) * t) + 0.03 * rng.randn(hi - lo)
        out.append(x.astype(np.float32))
    return out


def window_ms(fn, launches=20, windows=5, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / launches)
    return float(np.median(ts)), float(np.min(ts))


def wall_ms(fn, reps=10, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    from deepvoice3_pytorch_amd import _lib, audio
    from deepvoice3_pytorch_amd.ops import _stream
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    up, down = audio.resample_ratio(SRC, DST)
    T = 2 * audio.resample_half_width(up, down) + 2
    res = {"measured_on": "MI355X (gfx950), one GPU", "lengths": "uniform 3..6 s at 48000 Hz (seeded)",
           "ratio": [up, down], "taps": T, "peak_vector_fp32_flops": PEAK_FP32,
           "timing": "device events around 20 back-to-back calls, / 20; median (min) of 5 windows after 3 warm-up calls",
           "launch": {}}
    tile = _lib.lib().dv3_resample_tile(up, down)
    for B in (16, 64, 256):
        wavs = utterances(rng, B)
        flat, lengths = audio.pack_waveforms(wavs, pin=False)
        x = flat.to(dev)
        n_in = int(lengths.sum())
        # the resampler: the whole Python call (three small offset uploads + the launch), and the launch alone
        y, rlen = audio.resample_items(x, lengths, up, down)
        n_out = int(rlen.sum())
        call_ms, _ = window_ms(lambda: audio.resample_items(x, lengths, up, down))
        tiles = -(-rlen // tile)
        ioff, ooff = audio._sample_offsets(lengths, dev), audio._sample_offsets(rlen, dev)
        toff = torch.from_numpy(np.concatenate([[0], np.cumsum(tiles)]).astype(np.int32)).to(dev)
        table = audio.resample_table(dev, up, down)
        args = (x.data_ptr(), ioff.data_ptr(), ooff.data_ptr(), toff.data_ptr(), B, int(tiles.sum()), up, down,
                table.data_ptr(), y.data_ptr())
        k_ms, k_min = window_ms(lambda: _lib.call("dv3_resample_items_f32", *args, _stream()))
        flops = 2.0 * T * n_out
        # trim of the resampled items
        starts = np.concatenate([[0], np.cumsum(rlen)[:-1]])
        t_ms, t_min = window_ms(lambda: audio.trim_items(y, starts, rlen, 15.0))
        ts, tn = audio.trim_items(y, starts, rlen, 15.0)
        g_ms, _ = window_ms(lambda: audio.gather_spans(y, ts, tn))
        res["launch"]["B%d" % B] = dict(
            utterances=B, input_samples=n_in, output_samples=n_out, audio_s=n_in / float(SRC),
            resample_kernel_ms=k_ms, resample_kernel_ms_min=k_min, resample_call_ms=call_ms,
            resample_input_samples_per_s=n_in / (k_ms * 1e-3), resample_flops=flops,
            resample_fraction_of_vector_fp32_peak=flops / (k_ms * 1e-3) / PEAK_FP32,
            trim_call_ms=t_ms, trim_call_ms_min=t_min, trim_input_samples_per_s=n_out / (t_ms * 1e-3),
            trimmed_samples=int(tn.sum().item()), gather_call_with_host_read_ms=g_ms)
    # one B = 64 batch from host arrays
    wavs = utterances(rng, 64)
    pack_ms = wall_ms(lambda: audio.pack_waveforms(wavs))
    flat, lengths = audio.pack_waveforms(wavs)
    h2d_ms, _ = window_ms(lambda: flat.to(dev, non_blocking=True))
    x = flat.to(dev)

    def device_part():
        y, rlen = audio.resample_items(x, lengths, up, down)
        starts = np.concatenate([[0], np.cumsum(rlen)[:-1]])
        ts, tn = audio.trim_items(y, starts, rlen, 15.0)
        return audio.gather_spans(y, ts, tn)

    prep_ms, _ = window_ms(device_part)
    pf, pl = device_part()
    feat_ms, _ = window_ms(lambda: audio.features_items(pf, pl))
    total_ms = wall_ms(lambda: audio.features_items(*audio.prepare_items(wavs, SRC, None, None, 15.0, dev)))
    res["per_batch_b64"] = dict(utterances=64, source_samples=int(lengths.sum()), bytes_h2d=int(lengths.sum()) * 4,
                                trimmed_samples=int(pl.sum()), frames=int(sum(audio.lws_num_frames(int(n), 256) for n in pl)),
                                pack_host_ms=pack_ms, h2d_ms=h2d_ms, resample_trim_gather_ms=prep_ms,
                                features_items_ms=feat_ms, prepare_and_features_wall_ms=total_ms)
    line = json.dumps(res, indent=1)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
