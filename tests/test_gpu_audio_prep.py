# coding: utf-8
"""Waveform preparation on the GPU (audio.resample_items / trim_items / gather_spans / prepare_items, ABI 46) and the
VCTK preprocessing built on it:

  * the resampler against its fp64 restatement (tests/audio_prep_ref.py) within the bound its roundings give;
  * resample, trim and the chained prepare_items are batch-invariant bit for bit;
  * the trimmed spans equal the restatement's as integers (on inputs whose every frame is clear of its threshold);
  * features of prepare_items' output equal, bit for bit, features of the same spans sliced on the host;
  * preprocess.build_from_path(name="vctk") on a synthetic corpus, read back and trained on for one step.
"""
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from tests import audio_prep_ref as R

pytestmark = pytest.mark.gpu

RATIOS = [(147, 320), (1, 2), (160, 147), (2, 1),
          (441, 160)]          # beyond the issue's list: up > 320, the kernel's path without shared coefficients


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _speechlike(n, rng, sr=48000.0):
    t = np.arange(n) / sr
    x = rng.uniform(0.1, 0.5) * np.sin(2 * np.pi * rng.uniform(90, 300) * t) \
        + rng.uniform(0.02, 0.1) * np.sin(2 * np.pi * rng.uniform(1000, 9000) * t + 1.0) + 0.03 * rng.randn(n)
    return x.astype(np.float32)


def _resample(wavs, up, down, dev):
    from deepvoice3_pytorch_amd import audio
    flat, lengths = audio.pack_waveforms(wavs, pin=False)
    y, out_len = audio.resample_items(flat.to(dev), lengths, up, down)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    o = np.concatenate([[0], np.cumsum(out_len)])
    return [y[o[i]:o[i + 1]] for i in range(len(wavs))]


@pytest.mark.parametrize("up,down", RATIOS)
def test_resampler_against_the_restatement(dev, up, down):
    """|y - y64| <= (T + 2) 2^-24 sum_k |h_k x_k| per output, T = 2H + 2 taps: the coefficients' one fp32 rounding
    (relative 2^-24 each) plus an fmaf chain of T terms (T 2^-24 of the same sum, to first order)"""
    from deepvoice3_pytorch_amd import _lib
    rng = np.random.RandomState(up * 1000 + down)
    H = R.half_width(up, down)
    T = 2 * H + 2
    tile = _lib.lib().dv3_resample_tile(up, down)
    assert tile > 0
    five_s = 5 * 48000 if down > up else 5 * 22050
    # 1 sample, H, H + 1, one tile's worth of input plus a bit (not a multiple of the tile), about 5 s
    lengths = [1, H, H + 1, 2, (3 * tile * down) // up + 17, 4097, five_s + 123]
    wavs = [_speechlike(n, rng) for n in lengths]
    got = _resample(wavs, up, down, dev)
    worst = 0.0
    for L, w, g in zip(lengths, wavs, got):
        want, mag = R.resample(w.astype(np.float64), up, down, with_bound=True)
        assert g.shape == want.shape == (-(-L * up // down),), (L, g.shape)
        bound = (T + 2) * 2.0 ** -24 * mag
        err = np.abs(g.astype(np.float64) - want)
        ratio = float((err / np.maximum(bound, 1e-300)).max()) if np.any(bound > 0) else 0.0
        worst = max(worst, ratio)
        print("ratio %d/%d L = %d: max error %.3e, max error / bound %.3f" % (up, down, L, err.max(), ratio))
        assert np.all(err <= bound), (up, down, L, float(err.max()), ratio)
    assert worst > 0.0                                       # fp32 did round somewhere: the comparison is not vacuous


def test_equal_rates_return_the_input_without_a_launch(dev):
    from deepvoice3_pytorch_amd import audio
    rng = np.random.RandomState(5)
    x = torch.from_numpy(_speechlike(5000, rng)).to(dev)
    for up, down in ((1, 1), (7, 7)):
        y, n = audio.resample_items(x, [2000, 3000], up, down)
        assert y.data_ptr() == x.data_ptr() and y.shape == x.shape and list(n) == [2000, 3000]
    # the definition at ratio 1 is NOT the identity (roll-off < 1), which is why it is never launched
    assert abs(R.resample(np.array([1.0]), 1, 1)[0] - R.ROLLOFF) < 1e-15


# ---- trim ----
def _trim_signals():
    """noise bursts between near-silent stretches -> [(float32 signal, top_db)]"""
    rng = np.random.RandomState(11)
    out = []

    def sig(n, bursts, floor):
        x = floor * rng.randn(n)
        for lo, hi, level in bursts:
            x[lo:hi] = level * rng.randn(hi - lo)
        return x.astype(np.float32)

    out.append((sig(30000, [(7000, 19000, 0.3)], 1e-4), 15.0))
    out.append((sig(30000, [(7000, 19000, 0.3)], 1e-4), 25.0))
    out.append((sig(41234, [(3000, 9000, 0.05), (20000, 33000, 0.4)], 3e-5), 15.0))       # two levels
    out.append((sig(41234, [(3000, 9000, 0.05), (20000, 33000, 0.4)], 3e-5), 25.0))
    out.append((sig(41234, [(3000, 9000, 0.004), (20000, 33000, 0.4)], 3e-5), 25.0))      # the first burst is too quiet
    out.append((sig(25000, [(0, 8000, 0.2)], 1e-4), 15.0))                                # touches the start
    out.append((sig(25000, [(16000, 25000, 0.2)], 1e-4), 25.0))                           # touches the end
    out.append((sig(25001, [(0, 25001, 0.1)], 0.0), 15.0))                                # nothing to trim
    out.append((np.zeros(6000, np.float32), 15.0))                                        # all silent: kept whole
    out.append((sig(9000, [], 1e-4), 25.0))                                               # near-silent throughout
    out.append((sig(1024, [(300, 600, 0.3)], 1e-4), 15.0))                                # too short to pad
    out.append((sig(700, [(0, 100, 0.3)], 0.0), 25.0))
    out.append((sig(1025, [(500, 1025, 0.3)], 1e-5), 15.0))                               # the shortest that is framed
    out.append((sig(110250, [(30000, 31000, 0.5), (60000, 90000, 0.04)], 2e-5), 25.0))    # 5 s, loud click then speech
    out.append((sig(110250, [(30000, 31000, 0.5), (60000, 90000, 0.04)], 2e-5), 15.0))
    out.append((sig(2048, [(1000, 1100, 0.3)], 1e-5), 15.0))
    return out


def _trim(items, dev):
    """-> [(start relative to the item, length)] via audio.trim_items on the items packed back to back"""
    from deepvoice3_pytorch_amd import audio
    wavs = [w for w, _ in items]
    flat, lengths = audio.pack_waveforms(wavs, pin=False)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    s, n = audio.trim_items(flat.to(dev), starts, lengths, [t for _, t in items])
    assert s.is_cuda and n.is_cuda and s.dtype == n.dtype == torch.int64
    s, n = s.cpu().numpy(), n.cpu().numpy()
    return [(int(s[i] - starts[i]), int(n[i])) for i in range(len(items))]


def test_trim_against_the_restatement(dev):
    items = _trim_signals()
    # condition on the inputs, from the restatement alone: no frame within 0.05 dB of its threshold (the fp32 mean of
    # 2048 squares is good to about 2048 * 2^-24 relative = 5e-4 dB, so the decision can not legitimately flip)
    left_out = 0
    for w, top_db in items:
        if len(w) >= 1025:
            margin = np.abs(R.trim_frame_db(w.astype(np.float64)) + top_db).min()
            left_out += int(margin < 0.05)
    assert left_out == 0
    want = [R.trim(w.astype(np.float64), t) for w, t in items]
    got = _trim(items, dev)
    print("trim spans:", got)
    assert got == want
    # the cases are what they claim to be
    # a burst 18 dB under the loudest is cut at 15 dB and kept at 25 dB; one 40 dB under is cut at 25 dB too
    assert want[2][0] >= 19 * 512 and want[3][0] < 9000 and want[4][0] >= 19 * 512
    assert want[5][0] == 0 and want[6][0] + want[6][1] == 25000 and want[7] == (0, 25001)
    assert want[8] == (0, 6000) and want[10] == (0, 1024) and want[11] == (0, 700)
    assert want[13] != want[14]


# ---- batch invariance, bit for bit ----
def _prepare(wavs, spans, top_db, dev):
    from deepvoice3_pytorch_amd import audio
    flat, lengths = audio.prepare_items(wavs, 48000, None, spans, top_db, dev)
    torch.cuda.synchronize()
    flat = flat.cpu().numpy()
    o = np.concatenate([[0], np.cumsum(lengths)])
    return [flat[o[i]:o[i + 1]] for i in range(len(wavs))]


def _utterances(n, seed, sr=48000):
    """silence / speech-like / silence at 48 kHz, 0.3 - 1.2 s; a few with label cuts -> (wavs, spans, top_db)"""
    rng = np.random.RandomState(seed)
    wavs, spans, top_db = [], [], []
    for i in range(n):
        L = int(rng.randint(int(0.3 * sr), int(1.2 * sr)))
        lo, hi = sorted(rng.randint(0, L, 2))
        x = 1e-4 * rng.randn(L)
        x[lo:hi] += _speechlike(hi - lo, rng)
        wavs.append(x.astype(np.float32))
        if i % 3 == 1:
            out = -(-L * 147 // 320)
            spans.append((int(0.1 * out), int(0.9 * out)))
            top_db.append(25.0)
        else:
            spans.append(None)
            top_db.append(15.0)
    return wavs, spans, top_db


def test_batch_invariance(dev):
    """each item alone, in a batch of 16 and in reversed order: the same bits (the pattern of
    test_gpu_wav_features.py::test_rows_are_batch_invariant)"""
    rng = np.random.RandomState(2)
    # resample: ragged lengths incl. 1 sample, below the filter's half width, tile edges
    lengths = [1, 100, 141, 2560, 2561, 5119, 48000, 33333, 7, 1280, 29999, 64000]
    wavs = [_speechlike(n, rng) for n in lengths]
    extra = [_speechlike(n, rng) for n in (3000, 40000, 257, 9999)]
    for up, down in ((147, 320), (2, 1), (441, 160)):
        batched = _resample(wavs, up, down, dev)
        in16 = _resample(extra[:2] + wavs + extra[2:], up, down, dev)
        rev = _resample(wavs[::-1], up, down, dev)
        for b in range(len(wavs)):
            alone = _resample([wavs[b]], up, down, dev)[0]
            assert np.array_equal(alone, batched[b]), (up, down, b)
            assert np.array_equal(in16[b + 2], batched[b]), (up, down, b)
            assert np.array_equal(rev[len(wavs) - 1 - b], batched[b]), (up, down, b)
    # trim: the spans are integers; equal alone, among others and reversed
    items = _trim_signals()[:12]
    more = _trim_signals()[12:]
    batched = _trim(items, dev)
    assert _trim(more[:2] + items + more[2:], dev)[2:2 + len(items)] == batched
    assert _trim(items[::-1], dev)[::-1] == batched
    for b in range(len(items)):
        assert _trim([items[b]], dev) == [batched[b]], b
    # the chain: 48 kHz utterances -> resampled, label-cut, trimmed, packed
    wavs, spans, top_db = _utterances(12, 7)
    ew, es, et = _utterances(4, 8)
    batched = _prepare(wavs, spans, top_db, dev)
    assert all(0 < len(g) < len(w) * 147 / 320 for g, w in zip(batched, wavs))        # every item was trimmed
    in16 = _prepare(ew[:2] + wavs + ew[2:], es[:2] + spans + es[2:], et[:2] + top_db + et[2:], dev)
    rev = _prepare(wavs[::-1], spans[::-1], top_db[::-1], dev)
    for b in range(len(wavs)):
        alone = _prepare([wavs[b]], [spans[b]], [top_db[b]], dev)[0]
        assert np.array_equal(alone, batched[b]), b
        assert np.array_equal(in16[b + 2], batched[b]), b
        assert np.array_equal(rev[len(wavs) - 1 - b], batched[b]), b


def test_gather_spans_copies_any_alignment(dev):
    from deepvoice3_pytorch_amd import audio
    rng = np.random.RandomState(4)
    x = rng.randn(50000).astype(np.float32)
    starts = np.array([0, 1, 2, 3, 4, 1001, 20002, 30003, 777, 49999, 100, 12345], dtype=np.int64)
    lens = np.array([5, 4, 0, 1, 4099, 3, 8191, 19997, 2, 1, 16, 4096], dtype=np.int64)
    xd = torch.from_numpy(x).to(dev)
    for s, n in ((starts, lens), (starts[::-1].copy(), lens[::-1].copy())):
        want = np.concatenate([x[a:a + b] for a, b in zip(s, n)])
        y, out_len = audio.gather_spans(xd, s, n)                                           # host spans
        assert np.array_equal(out_len, n) and np.array_equal(y.cpu().numpy(), want)
        y, out_len = audio.gather_spans(xd, torch.from_numpy(s).to(dev), torch.from_numpy(n).to(dev))
        assert np.array_equal(out_len, n) and np.array_equal(y.cpu().numpy(), want)
    with pytest.raises(ValueError):
        audio.gather_spans(xd, [49999], [2])


def test_features_of_prepared_items_equal_features_of_host_slices(dev):
    """the new path adds no rounding of its own after the resampler: features_items on prepare_items' output against
    features_items on the same spans sliced on the host from the resampled buffer"""
    from deepvoice3_pytorch_amd import audio
    wavs, spans, top_db = _utterances(9, 21)
    flat, lengths = audio.prepare_items(wavs, 48000, None, spans, top_db, dev)
    assert lengths.min() > 0
    got = audio.features_items(flat, lengths, rescaling=0.999)
    # the same by hand: resample, cut, trim, read the spans back, slice on the host, upload
    src, src_len = audio.pack_waveforms(wavs, pin=False)
    res, rlen = audio.resample_items(src.to(dev), src_len, 147, 320)
    starts = np.concatenate([[0], np.cumsum(rlen)[:-1]])
    lens = rlen.copy()
    for b, sp in enumerate(spans):
        if sp is not None:
            starts[b] += sp[0]
            lens[b] = sp[1] - sp[0]
    ts, tn = audio.trim_items(res, starts, lens, top_db)
    ts, tn = ts.cpu().numpy(), tn.cpu().numpy()
    assert np.array_equal(tn, lengths)
    res_h = res.cpu().numpy()
    sliced = np.concatenate([res_h[a:a + n] for a, n in zip(ts, tn)])
    assert np.array_equal(sliced, flat.cpu().numpy())
    want = audio.features_items(torch.from_numpy(sliced).to(dev), tn, rescaling=0.999)
    assert np.array_equal(got[2], want[2])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- end to end: a synthetic VCTK tree ----
SPEAKERS = ["p225", "p226", "p301"]


def _vctk_tree(root, seed=13):
    """3 speakers + one without transcripts, 12 utterances of 0.4 - 0.9 s at 48 kHz PCM16, one with a label file"""
    rng = np.random.RandomState(seed)
    rows = []
    for spk in SPEAKERS + ["p315"]:
        os.makedirs(os.path.join(root, "wav48", spk))
        if spk != "p315":
            os.makedirs(os.path.join(root, "txt", spk))
        for k in range(1, 5):
            L = int(rng.randint(19200, 43200))
            lo = int(rng.randint(2000, 6000))
            hi = L - int(rng.randint(2000, 6000))
            x = 1e-4 * rng.randn(L)
            x[lo:hi] += _speechlike(hi - lo, rng)
            stem = "%s_%03d" % (spk, k)
            wavfile.write(os.path.join(root, "wav48", spk, stem + ".wav"), 48000,
                          np.clip(x * 32768, -32768, 32767).astype(np.int16))
            if spk == "p315":
                continue
            text = "utterance %d of speaker %s, long enough to train on" % (k, spk)
            with open(os.path.join(root, "txt", spk, stem + ".txt"), "w") as f:
                f.write(text + "\n")
            rows.append((stem, text, SPEAKERS.index(spk), L, lo, hi))
    # p226_002 has HTS labels: pau | speech | pau, in 100 ns units of the 48 kHz recording
    stem, _, _, L, lo, hi = rows[5]
    assert stem == "p226_002"
    os.makedirs(os.path.join(root, "lab", "p226"))
    u = lambda n: int(round(n / 48000.0 * 1e7))
    with open(os.path.join(root, "lab", "p226", stem + ".lab"), "w") as f:
        f.write("0 %d pau\n%d %d a\n%d %d b\n%d %d pau\n" % (u(lo), u(lo), u((lo + hi) // 2), u((lo + hi) // 2), u(hi),
                                                           u(hi), u(L)))
    return rows


def _t2s(text):
    return [2 + ord(c) % 38 for c in text]


@pytest.fixture(scope="module")
def vctk(tmp_path_factory, dev):
    from deepvoice3_pytorch_amd import preprocess
    base = tmp_path_factory.mktemp("vctk")
    in_dir, out_dir = str(base / "VCTK-Corpus"), str(base / "out")
    rows = _vctk_tree(in_dir)
    # a small budget of source samples, so the corpus takes several launches
    md = preprocess.build_from_path(in_dir, out_dir, device=dev, max_batch_samples=100000, name="vctk")
    return in_dir, out_dir, rows, md


def test_build_from_path_vctk(dev, vctk):
    from deepvoice3_pytorch_amd import audio, data, preprocess
    in_dir, out_dir, rows, md = vctk
    assert len(md) == len(rows) == 12
    with open(os.path.join(out_dir, "speakers.json")) as f:
        speakers = json.load(f)
    assert speakers == {"p225": 0, "p226": 1, "p301": 2}
    with open(os.path.join(out_dir, "train.txt"), encoding="utf-8") as f:
        lines = f.read().splitlines()
    assert len(lines) == 12
    for k, ((stem, text, sid, L, lo, hi), m, line) in enumerate(zip(rows, md, lines)):
        assert m[:2] == ("vctk-spec-%05d.npy" % (k + 1), "vctk-mel-%05d.npy" % (k + 1)) and m[3:] == (text, sid)
        assert line == "%s|%s|%d|%s|%d" % (m[0], m[1], m[2], text, speakers[stem[:4]])
        spec, mel = np.load(os.path.join(out_dir, m[0])), np.load(os.path.join(out_dir, m[1]))
        assert spec.shape == (m[2], 513) and mel.shape == (m[2], 80) and spec.dtype == mel.dtype == np.float32
        # trimmed: fewer frames than the whole resampled recording has, at least what the speech itself needs less one
        # 512-sample trim hop on each side
        whole = audio.lws_num_frames(-(-L * 147 // 320), 256)
        speech = (hi - lo) * 147 // 320
        assert audio.lws_num_frames(max(speech - 1024, 1), 256) <= m[2] < whole, (stem, m[2], whole)
    cfg = data.read_audio_config(out_dir)
    assert (cfg["sample_rate"], cfg["hop_size"], cfg["fft_size"], cfg["num_mels"]) == (22050, 256, 1024, 80)
    assert cfg["convention"] == "lws" and cfg["rescaling"] is False
    assert cfg["trim_top_db"] == {"labels": 25.0, "plain": 15.0}
    assert cfg["resample"]["source_rates"] == [48000]
    assert (cfg["resample"]["zeros"], cfg["resample"]["rolloff"], cfg["resample"]["beta"]) == (R.ZEROS, R.ROLLOFF, R.BETA)
    assert (cfg["trim_frame_length"], cfg["trim_hop_length"]) == (2048, 512)
    # the stored features of one utterance are what its own preparation, alone, gives
    for k in (2, 5):                                                    # 5 is the labelled one
        w, sr = preprocess.load_wav(os.path.join(in_dir, "wav48", rows[k][0][:4], rows[k][0] + ".wav"), None)
        assert sr == 48000
        span, top = None, 15.0
        lab = preprocess.vctk_label_path(os.path.join(in_dir, "wav48", rows[k][0][:4], rows[k][0] + ".wav"))
        assert os.path.exists(lab) == (k == 5)
        if k == 5:
            b, e = preprocess.read_hts_labels(lab)
            span, top = (int(b * 1e-7 * 22050), int(e * 1e-7 * 22050)), 25.0
        flat, n = audio.prepare_items([w], sr, None, [span], top, dev)
        lin, mel, frames = audio.features_items(flat, n)
        assert int(frames[0]) == md[k][2]
        assert np.array_equal(lin.cpu().numpy(), np.load(os.path.join(out_dir, md[k][0])))
        assert np.array_equal(mel.cpu().numpy(), np.load(os.path.join(out_dir, md[k][1])))


def test_vctk_directory_trains(dev, vctk):
    from deepvoice3_pytorch_amd import builder, data, train_step
    in_dir, out_dir, rows, md = vctk
    ds = data.PreprocessedDataset(out_dir, _t2s)
    assert ds.multi_speaker and len(ds) == 12 and ds.frame_lengths == [m[2] for m in md]
    idx = [7, 0, 10, 5, 3, 8]
    batch = data.device_collate(data.pack_batch([ds[i] for i in idx]), dev, 1, 4)
    assert batch.speaker_ids.cpu().reshape(-1).tolist() == [rows[i][2] for i in idx]
    assert batch.target_lengths_host.tolist() == [md[i][2] for i in idx]
    assert batch.input_lengths_host.tolist() == [len(_t2s(rows[i][1])) for i in idx]
    hp = dict(n_vocab=40, embed_dim=32, mel_dim=80, linear_dim=513, r=1, downsample_step=4, n_speakers=3,
              speaker_embed_dim=8, padding_idx=0, dropout=0.05, kernel_size=3, encoder_channels=64, decoder_channels=32,
              converter_channels=32, use_memory_mask=True, force_monotonic_attention=True,
              use_decoder_state_for_postnet_input=True, key_projection=True, value_projection=True, max_positions=256)
    torch.manual_seed(0)
    model = builder.deepvoice3_multispeaker(**hp).to(dev)
    tr = train_step.Trainer(model, train_step.TrainConfig(max_positions=256))
    out = tr.step(batch)
    assert np.isfinite(float(out["loss"]))
