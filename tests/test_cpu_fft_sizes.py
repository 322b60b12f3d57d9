# coding: utf-8
"""The host side of the three frame sizes (fft_size 512, 1024, 2048): the configuration, the window tables, the frame /
sample arithmetic, the mel filterbank and the C header's `_n` entry points.  No GPU.  The kernels themselves are held
to the oracle in tests/test_gpu_fft_sizes.py."""
import numpy as np
import pytest

from oracle import audio_oracle as A

SIBLINGS = ("dv3_istft_frames_f32", "dv3_overlap_add_f32", "dv3_gl_project_f32", "dv3_stft_phase_f32",
            "dv3_lws_stft_f32", "dv3_lws_istft_frames_f32", "dv3_lws_overlap_add_f32", "dv3_lws_gl_project_f32",
            "dv3_gl_istft_items_f32", "dv3_overlap_add_items_f32", "dv3_gl_project_items_f32", "dv3_analysis_items_f32")


def test_audio_config_takes_the_three_sizes_and_names_the_others():
    from deepvoice3_pytorch_amd import audio
    assert audio.FFT_SIZES == (512, 1024, 2048)
    for n, hop, sr in ((512, 128, 16000), (2048, 512, 48000), (1024, 256, 22050)):
        cfg = audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=sr)
        assert (cfg.fft_size, cfg.hop_size, cfg.sample_rate) == (n, hop, sr)
        assert abs(cfg.window_scale - np.sqrt(2.0 * hop / n)) < 1e-15          # the hop normalisation follows the size
    for bad in (4096, 768, 256):
        with pytest.raises(ValueError, match=r"fft_size=%d\b.*512, 1024, 2048" % bad):
            audio.AudioConfig(fft_size=bad, hop_size=bad // 4)
    with pytest.raises(ValueError, match="hop_size"):
        audio.AudioConfig(fft_size=512, hop_size=513)
    with pytest.raises(ValueError, match="1025.*513|513.*1025"):                # a spectrogram of the wrong width: both numbers
        audio.check_bins(513, 2048, "test")


@pytest.mark.parametrize("n,hop", [(512, 128), (512, 96), (2048, 512), (2048, 384)])
def test_lws_windows_are_the_oracles(n, hop):
    import torch
    from deepvoice3_pytorch_amd import audio
    aw, sw = A.lws_windows(n, hop)
    a2, s2 = audio.lws_windows_np(n, hop)
    assert a2.shape == s2.shape == (n,)
    assert np.abs(a2 - aw).max() < 1e-12 and np.abs(s2 - sw).max() < 1e-12
    # the device tables (here on the CPU): the same numbers rounded once to fp32, cached per size
    a3, s3 = audio.lws_windows(torch.device("cpu"), hop, None, n)
    assert a3.dtype == torch.float32 and tuple(a3.shape) == tuple(s3.shape) == (n,)
    assert np.array_equal(a3.numpy(), aw.astype(np.float32)) and np.array_equal(s3.numpy(), sw.astype(np.float32))
    a1024, _ = audio.lws_windows(torch.device("cpu"), hop)                      # another size at the same hop: its own entry
    assert tuple(a1024.shape) == (1024,)
    # overlap-add of awin * swin over every window position is the identity
    Q = -(-n // hop)
    ola = np.zeros(n + (Q - 1) * hop)
    for q in range(Q):
        ola[q * hop:q * hop + n] += a2 * s2
    assert np.abs(ola[(Q - 1) * hop:n] - 1.0).max() < 1e-12


@pytest.mark.parametrize("n,hop", [(512, 128), (512, 96), (2048, 512), (2048, 384), (1024, 256)])
def test_frame_and_sample_counts_follow_the_size(n, hop):
    from deepvoice3_pytorch_amd import audio
    for T in (4, 7, 12, 100):
        assert audio.lws_num_samples(T, hop, n) == (T + 1) * hop - n
        assert audio.num_samples(T, hop, "lws", n) == (T + 1) * hop - n
        assert audio.num_samples(T, hop, "torch", n) == hop * (T - 1)
    for L in (1, hop, 5 * hop, 5 * hop + 1, 1000, 4801):
        T = audio.lws_num_frames(L, hop, n)
        assert T == A.lws_num_frames(L, n, hop) == A.lws_stft(np.zeros(L), n, hop).shape[0]
        assert audio.lws_num_samples(T - 1, hop, n) < L <= audio.lws_num_samples(T, hop, n)     # what the C side requires
    # the fewest frames each framing takes: a positive length (lws), a signal longer than the reflect padding (torch)
    t = audio.min_frames(hop, "lws", n)
    assert (t + 1) * hop - n > 0 and (t == 2 or t * hop - n <= 0)
    t = audio.min_frames(hop, "torch", n)
    assert hop * (t - 1) > n // 2 and (t == 2 or hop * (t - 2) <= n // 2)


@pytest.mark.parametrize("sr,n", [(16000, 512), (48000, 2048)])
def test_mel_basis_at_the_new_sizes(sr, n):
    from deepvoice3_pytorch_amd import audio
    W = audio.mel_basis(sr, n, 80, 125.0, 7600.0)
    want = A.slaney_mel_basis(sr=sr, n_fft=n, n_mels=80, fmin=125.0, fmax=7600.0)
    assert W.shape == (80, n // 2 + 1) and W.dtype == np.float32
    assert np.abs(W - want).max() < 1e-6 * want.max()                           # tests/test_audio.py's bound


def test_header_declares_the_twelve_siblings_and_abi_49():
    from deepvoice3_pytorch_amd import _lib
    import ctypes
    assert _lib.CONSTS["DV3_ABI_VERSION"] == 50        # (the siblings came with 49; 50 added the switch table's entry points)
    for name in SIBLINGS:
        _, parent = _lib.FUNCS[name]
        assert name + "_n" in _lib.FUNCS, name
        _, sib = _lib.FUNCS[name + "_n"]
        # the parent's arguments, then int32_t n_fft in front of the stream
        assert sib == parent[:-1] + [ctypes.c_int32, ctypes.c_void_p], name
    assert sum(1 for f in _lib.FUNCS if f.endswith("_n")) == 12


def test_waveform_dataset_counts_frames_at_the_configs_size(tmp_path):
    from scipy.io import wavfile
    from deepvoice3_pytorch_amd import audio, data
    rng = np.random.RandomState(0)
    rows = []
    for i, L in enumerate((4800, 3001)):
        p = str(tmp_path / ("u%d.wav" % i))
        wavfile.write(p, 16000, (rng.randn(L) * 3000).astype(np.int16))
        rows.append((p, "text %d" % i))
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000)
    ds = data.WaveformDataset(rows, lambda t: [1, 2, 3], cfg=cfg)
    assert ds.frame_lengths == [A.lws_num_frames(4800, 512, 128), A.lws_num_frames(3001, 512, 128)]
    assert ds.frame_lengths != data.WaveformDataset(rows, lambda t: [1, 2, 3], hop_size=128, sample_rate=16000).frame_lengths
    assert ds.frame_lengths == data.WaveformDataset(rows, lambda t: [1, 2, 3], 128, 16000, 512).frame_lengths
