# coding: utf-8
"""Spectrogram -> waveform on the GPU: the device-side counterpart of the reference's
audio.inv_spectrogram (audio.py:37-43) and its helpers (audio.py:26-28,84-93), and the forward analysis
audio.spectrogram / audio.melspectrogram (audio.py:31-35,46-51), with the waveform preparation of the multi-speaker
corpora in front of it: resampling (audio.py:12-13, librosa.load) and silence trimming (vctk.py:52-67).

The reference hands framing and phase reconstruction to the third-party `lws` package on the host
(audio.py:40-42,54-55); here they run on hand-written HIP FFT kernels (csrc/audio.hip), batched over utterances, so
synthesis never leaves the device (synthesis.py:64-71 copies the spectrogram to the CPU first).

Conventions (AudioConfig.convention):
  "lws"    (default) the framing of `lws.lws(fft_size, hop, mode="speech")` the reference's features are made with and
           its inverse is framed by: sqrt-symmetric-Hann analysis window, perfect-reconstruction synthesis window,
           fft_size - hop zeros of padding on both sides -- T frames <-> (T + 1) * hop - fft_size samples (1024 / 256:
           L = 256 k -> k + 3 frames).
           Restated from the package's published source in oracle/audio_oracle.py (lws_windows / lws_stft / lws_istft).
           Phase reconstruction is Griffin-Lim on that framing (north_star), not lws's own run_lws iterations; like
           run_lws it can start from a single-pass phase estimate instead of zero phase (spsi_phasor, csrc/spsi.hip;
           AudioConfig(griffin_lim_init="spsi"), opt-in).
  "torch"  torch.stft / torch.istft conventions (periodic Hann, center=True reflect padding, L = hop * (T - 1)): rounds
           1-3's form, kept for A/B runs and for callers that pair it with torch-made features.

Frame size: AudioConfig.fft_size is 512, 1024 (every reference preset) or 2048 -- the sizes the FFT kernels are built for
(FFT_SIZES); 16 kHz corpora use 512 / 128, 44.1 and 48 kHz voices 2048 / 512.  The functions below that take a hop
instead of a config take the size as `fft_size=` (default 1024).

A mel spectrogram is vocoded through the same path: mel_to_linear inverts the filterbank per frame (csrc/mel_inverse.hip),
inv_melspectrogram_batch / inv_melspectrogram put its result through inv_spectrogram_batch.

Speaking rate and pitch: inv_spectrogram_batch(..., prosody=Prosody(rate, semitones)) puts the
magnitudes through warp_magnitudes (csrc/prosody.hip) before the phase is built: the frames resampled in time, the
harmonics moved along the frequency axis under the spectral envelope.  Off by default: without the keyword nothing runs.

Prosody marks: the same controls inside an item.  ProsodyMarks holds spans with their own rate, semitones and gain_db,
breaks and a transition; plan_prosody turns the segments into per-output-frame position, ratio and gain tables (two small
kernels around one host read), warp_magnitudes_curve follows such tables -- a caller's own just as well --, plan_map
carries timings onto the new time axis; inv_spectrogram_batch(..., prosody=marks) composes them.

Pitch: yin_items tracks F0 per frame of the packed waveforms features_items takes (csrc/pitch.hip), voiced() decides
which frames to believe (PitchConfig); synthesis.waveform_distortion builds the F0 and voicing error of an evaluation on it.

Deliverable audio (csrc/master.hip): the reference ends at save_wav (audio.py:16-18: peak-normalise, int16, a file).
wave_levels measures every utterance, wave_gains turns levels into gains under a Mastering, wave_master places, scales,
fades and quantises in one launch; master_items / to_pcm16 apply them to a padded batch, save_wav writes the file.
synthesis.join_utterances builds a document of several utterances on them.  Off by default: nothing runs unasked.

Loudness (csrc/loudness.hip): Mastering(level="lufs") levels to a LUFS target under a sample-peak or
true-peak ceiling.  wave_loudness measures ITU-R BS.1770 integrated loudness and the 4x true peak of spans or groups of
spans on the device (k_weighting and true_peak_table make its float64 coefficients and its interpolator on the host),
loudness_gains turns its rows into gains.  Mastering(limiter=Limiter()) (csrc/limiter.hip) holds the
ceiling with a look-ahead limiter instead of the static gain, so that the target is met where one loud syllable sets
the peak: limit_spans is the kernel's wrapper, master_source what master_items and join_utterances take their source
and gains from.
"""
import numpy as np
import torch

from . import _lib
from .ops import _stream, _chk, _c

N_FFT = 1024                       # the default frame size (every reference preset)
N_BIN = N_FFT // 2 + 1
FFT_SIZES = (512, 1024, 2048)      # the sizes csrc/audio.hip instantiates (include/dv3hip.h: the `_n` entry points)


def check_fft_size(fft_size):
    """-> fft_size as an int when the HIP FFT kernels are built for it, else ValueError naming it"""
    if isinstance(fft_size, bool) or fft_size not in FFT_SIZES or int(fft_size) != fft_size:
        raise ValueError("fft_size=%r is not supported: the HIP FFT kernels are built for fft_size in %s (4096 would "
                         "need 96 KB of LDS per workgroup)" % (fft_size, ", ".join(str(n) for n in FFT_SIZES)))
    return int(fft_size)


def check_bins(n_bins, fft_size, what):
    """a spectrogram's last dimension must be fft_size // 2 + 1 (the kernels read that many bins per frame)"""
    if int(n_bins) != fft_size // 2 + 1:
        raise ValueError("%s: the spectrogram has %d bins, but fft_size=%d frames %d (fft_size // 2 + 1)"
                         % (what, n_bins, fft_size, fft_size // 2 + 1))


def check_momentum(momentum):
    """-> the fast Griffin-Lim momentum as a float when it lies in [0, 1), else ValueError naming it (nan included)"""
    if isinstance(momentum, bool) or not isinstance(momentum, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(momentum) < 1.0:
        raise ValueError("griffin_lim_momentum=%r must lie in [0, 1): 0 is plain Griffin-Lim, 0.99 the usual fast one"
                         % (momentum,))
    return float(momentum)


GRIFFIN_LIM_INITS = ("zero", "spsi")


def check_init(init):
    """-> the Griffin-Lim starting phase's name when it is one of GRIFFIN_LIM_INITS, else ValueError naming both"""
    if not isinstance(init, str) or init not in GRIFFIN_LIM_INITS:
        raise ValueError("griffin_lim_init=%r must be 'zero' (zero phase) or 'spsi' (single pass spectrogram inversion)"
                         % (init,))
    return init


def resolve_window_scale(window_scale, hop, fft_size=N_FFT):
    """None / "hop_normalized" -> sqrt(2 hop / fft_size) (the default, see AudioConfig); else the positive number given"""
    if window_scale is None or window_scale == "hop_normalized":
        return float(np.sqrt(2.0 * hop / fft_size))
    if not (isinstance(window_scale, (int, float)) and window_scale > 0):
        raise ValueError("window_scale must be a positive number or 'hop_normalized'")
    return float(window_scale)


class AudioConfig(object):
    """The hparams audio.py reads (hparams.py:38-43,124)."""

    def __init__(self, fft_size=1024, hop_size=256, sample_rate=22050, preemphasis=0.97,
                 min_level_db=-100, ref_level_db=20, power=1.4, griffin_lim_iters=60, convention="lws",
                 window_scale="hop_normalized", griffin_lim_momentum=0.0, griffin_lim_init="zero"):
        """griffin_lim_init: the phase Griffin-Lim starts from when the caller gives no init_phasor -- "zero" (default:
        zero phase, the path every call has run) or "spsi" (spsi_phasor: a single-pass estimate from the spectral peaks;
        AudioConfig(griffin_lim_init="spsi", griffin_lim_iters=10, griffin_lim_momentum=0.99) ends below the 60 plain
        iterations from zero on speech-like magnitudes).  It is an option of the inverse, not a property
        of stored features.
        griffin_lim_momentum: the momentum of the fast Griffin-Lim algorithm (see griffin_lim), in [0, 1); 0.0 (default)
        is the plain alternation, 0.99 what librosa and torchaudio default to -- AudioConfig(griffin_lim_iters=30,
        griffin_lim_momentum=0.99) ends below the spectral convergence of the 60 plain iterations on speech-like magnitudes
        in half the projections ("Fast Griffin-Lim").
        window_scale (lws framing only): amplitude factor of the analysis window, the one constant of the third-party
        package this repository holds by recollection only (audio).  "hop_normalized" (default since
        round 6) = sqrt(2 * hop / fft_size) (0.7071 at 1024 / 256): `lws.lws(fsize, fshift)` with an integer first argument
        builds `awin = sqrt(hann(fsize, symmetric) * 2 * fshift / fsize)` as two independent recollections of lws.pyx
        have it.  1.0 = plain sqrt(hann) (rounds 4-5's default) stays selectable.  The two differ in ONE observable: every
        magnitude by 3.01 dB, i.e. every normalised [0, 1] feature by 0.0301, and an inverted waveform's amplitude by the
        inverse factor (tests/test_audio.py::test_window_scale_is_the_unconfirmed_constant); perfect reconstruction, the
        frame count and Griffin-Lim's fixed points do not depend on it (the synthesis window carries the inverse factor).
        tests/test_audio.py compares with the real package wherever it is importable."""
        fft_size = check_fft_size(fft_size)
        if not 0 < hop_size <= fft_size:
            raise ValueError("hop_size=%r must lie in [1, fft_size=%d]" % (hop_size, fft_size))
        if convention not in ("lws", "torch"):
            raise ValueError("convention must be 'lws' (the reference's framing) or 'torch'")
        window_scale = resolve_window_scale(window_scale, hop_size, fft_size)
        self.window_scale = float(window_scale)
        self.fft_size, self.hop_size, self.sample_rate = fft_size, hop_size, sample_rate
        self.preemphasis, self.min_level_db, self.ref_level_db = preemphasis, min_level_db, ref_level_db
        self.power, self.griffin_lim_iters = power, griffin_lim_iters
        self.convention = convention
        self.griffin_lim_momentum = check_momentum(griffin_lim_momentum)
        self.griffin_lim_init = check_init(griffin_lim_init)


# ---------------------------------------------------------------------------------------------
# lws framing (audio.py:54-55): window tables, frame / sample counts
# ---------------------------------------------------------------------------------------------
def lws_windows_np(fsize=N_FFT, fshift=256, scale=None):
    """(awin, swin) of lws.lws(fsize, fshift) as float64 numpy: `scale` x sqrt of the symmetric Hann window, and the
    synthesis window awin / overlap-added(awin^2) that makes overlap-add reconstruct perfectly (lws.pyx: hann, synthwin)."""
    k = np.arange(fsize, dtype=np.float64)
    awin = resolve_window_scale(scale, fshift, fsize) * np.sqrt(0.5 * (1.0 - np.cos(2.0 * np.pi * k / (fsize - 1))))
    Q = -(-fsize // fshift)
    w = np.concatenate([awin * awin, np.zeros(Q * fshift - fsize)]).reshape(Q, fshift).sum(0)
    w = np.tile(w, Q)[:fsize]
    if w.min() <= 0:
        raise ValueError("The normalizer is not strictly positive")
    return awin, awin / w


_WIN_CACHE = {}


def lws_windows(device, hop, scale=None, fft_size=N_FFT):
    """the two tables as float32 device tensors (cached per device, frame size, hop and window scale)"""
    scale = resolve_window_scale(scale, hop, fft_size)
    key = (str(device), int(fft_size), int(hop), float(scale))
    if key not in _WIN_CACHE:
        a, s = lws_windows_np(fft_size, hop, scale)
        _WIN_CACHE[key] = (torch.from_numpy(a.astype(np.float32)).to(device), torch.from_numpy(s.astype(np.float32)).to(device))
    return _WIN_CACHE[key]


def lws_num_frames(length, hop, fsize=N_FFT):
    """frames lws.stft makes of `length` samples (zero padding of fsize - hop on both sides, the last frame completed)"""
    pad = fsize - hop
    return -(-(length + 2 * pad - fsize) // hop) + 1      # ceil: also right for hops that do not divide fsize


def lws_num_samples(T, hop, fsize=N_FFT):
    """samples lws.istft returns for T frames"""
    return (T + 1) * hop - fsize


def magnitudes(linear_outputs, cfg):
    """(B, T, fft_size // 2 + 1) normalised spectrogram (the model's linear_outputs) -> magnitudes ** power."""
    x = _c(_chk(linear_outputs, "linear_outputs"))
    mag = torch.empty_like(x)
    _lib.call("dv3_gl_prepare_f32", x.data_ptr(), mag.data_ptr(), x.numel(), float(cfg.min_level_db),
              float(cfg.ref_level_db), float(cfg.power), _stream())
    return mag


def num_samples(T, hop, convention, fft_size=N_FFT):
    """samples the inverse makes of T frames: (T + 1) * hop - fft_size on the lws framing, hop * (T - 1) on the torch one"""
    return lws_num_samples(T, hop, fft_size) if convention == "lws" else hop * (T - 1)


def min_frames(hop, convention, fft_size=N_FFT):
    """the fewest frames the inverse takes at this hop: the lws framing needs a positive signal length, the torch one a
    signal longer than its reflect padding of fft_size // 2 (csrc/audio.hip: items_tlo)"""
    t = 2
    while num_samples(t, hop, convention, fft_size) <= (0 if convention == "lws" else fft_size // 2):
        t += 1
    return t


def istft(mag, phasor, hop, convention="torch", window_scale=None, tlen=None, fft_size=N_FFT):
    """mag (B,T,F), phasor (B,T,F,2) or None, F = fft_size // 2 + 1 -> y (B, hop*(T-1)); lws framing: (B, (T+1)*hop -
    fft_size).  tlen (device int32[B]): item b has only its first tlen[b] frames -- its own signal, zeros after it."""
    fft_size = check_fft_size(fft_size)
    B, T, F = mag.shape
    check_bins(F, fft_size, "istft")
    if phasor is not None and tuple(phasor.shape) != (B, T, F, 2):
        raise ValueError("istft: phasor must be (%d, %d, %d, 2), got %s" % (B, T, F, tuple(phasor.shape)))
    frames = torch.empty((B, T, fft_size), dtype=torch.float32, device=mag.device)
    if tlen is not None:
        lws = convention == "lws"
        swin = lws_windows(mag.device, hop, window_scale, fft_size)[1] if lws else None
        _lib.call("dv3_gl_istft_items_f32_n", mag.data_ptr(), phasor.data_ptr() if phasor is not None else None,
                  swin.data_ptr() if lws else None, frames.data_ptr(), B, T, hop, tlen.data_ptr(), int(lws), fft_size,
                  _stream())
        y = torch.empty((B, num_samples(T, hop, convention, fft_size)), dtype=torch.float32, device=mag.device)
        _lib.call("dv3_overlap_add_items_f32_n", frames.data_ptr(), y.data_ptr(), B, T, hop, tlen.data_ptr(), int(lws),
                  fft_size, _stream())
        return y
    if convention == "lws":
        _, swin = lws_windows(mag.device, hop, window_scale, fft_size)
        _lib.call("dv3_lws_istft_frames_f32_n", mag.data_ptr(), phasor.data_ptr() if phasor is not None else None,
                  swin.data_ptr(), frames.data_ptr(), B, T, fft_size, _stream())
        y = torch.empty((B, lws_num_samples(T, hop, fft_size)), dtype=torch.float32, device=mag.device)
        _lib.call("dv3_lws_overlap_add_f32_n", frames.data_ptr(), y.data_ptr(), B, T, hop, fft_size, _stream())
        return y
    _lib.call("dv3_istft_frames_f32_n", mag.data_ptr(), phasor.data_ptr() if phasor is not None else None,
              frames.data_ptr(), B, T, fft_size, _stream())
    y = torch.empty((B, hop * (T - 1)), dtype=torch.float32, device=mag.device)
    _lib.call("dv3_overlap_add_f32_n", frames.data_ptr(), y.data_ptr(), B, T, hop, fft_size, _stream())
    return y


def stft(y, T, hop, want_phasor=True, want_spec=False, convention="torch", window_scale=None, fft_size=N_FFT):
    """y (B, hop*(T-1)) -> unit phasors and/or the complex STFT, each (B,T,fft_size // 2 + 1,2); lws framing: T =
    lws_num_frames(L, hop, fft_size)."""
    fft_size = check_fft_size(fft_size)
    y = _c(_chk(y, "y"))
    B = y.shape[0]
    n_bin = fft_size // 2 + 1
    ph = torch.empty((B, T, n_bin, 2), dtype=torch.float32, device=y.device) if want_phasor else None
    sp = torch.empty((B, T, n_bin, 2), dtype=torch.float32, device=y.device) if want_spec else None
    if convention == "lws":
        assert T == lws_num_frames(y.shape[1], hop, fft_size)
        awin, _ = lws_windows(y.device, hop, window_scale, fft_size)
        _lib.call("dv3_lws_stft_f32_n", y.data_ptr(), awin.data_ptr(), ph.data_ptr() if ph is not None else None,
                  sp.data_ptr() if sp is not None else None, None, B, T, hop, y.shape[1], fft_size, _stream())
        return ph, sp
    assert y.shape[1] == hop * (T - 1)
    _lib.call("dv3_stft_phase_f32_n", y.data_ptr(), ph.data_ptr() if ph is not None else None,
              sp.data_ptr() if sp is not None else None, None, B, T, hop, fft_size, _stream())
    return ph, sp


# ---------------------------------------------------------------------------------------------
# forward analysis: audio.spectrogram / audio.melspectrogram (audio.py:31-35,46-51)
# ---------------------------------------------------------------------------------------------
def mel_basis(sample_rate=22050, n_fft=1024, n_mels=80, fmin=125.0, fmax=7600.0):
    """The Slaney-style triangular filterbank librosa.filters.mel builds by default (htk=False,
    norm='slaney'), restated: audio.py:70-76 with hparams.py fmin/fmax.  (num_mels, n_fft // 2 + 1) float32."""
    def hz_to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        mel = f / (200.0 / 3)
        lin_end = 1000.0 / (200.0 / 3)
        logstep = np.log(6.4) / 27.0
        return np.where(f >= 1000.0, lin_end + np.log(np.maximum(f, 1e-30) / 1000.0) / logstep, mel)

    def mel_to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        lin_end = 1000.0 / (200.0 / 3)
        logstep = np.log(6.4) / 27.0
        return np.where(m >= lin_end, 1000.0 * np.exp(logstep * (m - lin_end)), m * (200.0 / 3))
    fftfreqs = np.linspace(0, sample_rate / 2.0, n_fft // 2 + 1)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


def _analysis_mag(wav, cfg):
    """(B, L) waveform -> |STFT(preemphasis(wav))| as (B, fft_size // 2 + 1, T).  lws framing (default): any L, T =
    lws_num_frames(L) (1024 / 256: L = 256 k -> k + 3 frames, as the reference's preprocessing produces them); torch
    framing: L = hop * (T - 1)."""
    wav = _c(_chk(wav, "wav"))
    B, L = wav.shape
    hop, n_fft = cfg.hop_size, cfg.fft_size
    pre = torch.empty_like(wav)
    _lib.call("dv3_preemphasis_f32", wav.data_ptr(), pre.data_ptr(), B, L, float(cfg.preemphasis), _stream())
    if cfg.convention == "lws":
        T = lws_num_frames(L, hop, n_fft)
        awin, _ = lws_windows(wav.device, hop, cfg.window_scale, n_fft)
        mag = torch.empty((B, n_fft // 2 + 1, T), dtype=torch.float32, device=wav.device)
        _lib.call("dv3_lws_stft_f32_n", pre.data_ptr(), awin.data_ptr(), None, None, mag.data_ptr(), B, T, hop, L, n_fft,
                  _stream())
        return mag
    if L % hop:
        raise ValueError("waveform length must be a multiple of hop_size (%d)" % hop)
    T = L // hop + 1
    mag = torch.empty((B, n_fft // 2 + 1, T), dtype=torch.float32, device=wav.device)
    _lib.call("dv3_stft_phase_f32_n", pre.data_ptr(), None, None, mag.data_ptr(), B, T, hop, n_fft, _stream())
    return mag


def _db_norm(x, cfg):
    out = torch.empty_like(x)
    _lib.call("dv3_amp_to_db_norm_f32", x.data_ptr(), out.data_ptr(), x.numel(), float(cfg.min_level_db),
              float(cfg.ref_level_db), _stream())
    return out


def spectrogram_batch(wav, cfg=None):
    """audio.spectrogram (audio.py:31-35) for a (B, L) device batch -> (B, fft_size // 2 + 1, T) in [0, 1]."""
    cfg = cfg or AudioConfig()
    return _db_norm(_analysis_mag(wav, cfg), cfg)


def melspectrogram_batch(wav, cfg=None, num_mels=80, fmin=125.0, fmax=7600.0):
    """audio.melspectrogram (audio.py:46-51) for a (B, L) device batch -> (B, num_mels, T) in [0, 1]:
    the filterbank product runs on the tap-GEMM kernel as a 1x1 convolution over the fft_size // 2 + 1 bins."""
    from . import ops
    cfg = cfg or AudioConfig()
    mag = _analysis_mag(wav, cfg)
    B, F, T = mag.shape
    basis = torch.from_numpy(mel_basis(cfg.sample_rate, cfg.fft_size, num_mels, fmin, fmax)).to(wav.device)
    pk = ops.pack_weights(basis.unsqueeze(-1).contiguous(), None, need_bwd=False)
    mel = ops.conv_gemm(mag, pk.fwd, pk.lda, 0, B=B, Cin=F, Tin=T, M=num_mels, Tout=T, a_split=pk.fwd_s)
    return _db_norm(mel, cfg)


def griffin_lim(mag, hop, n_iter, init_phasor=None, convention="torch", window_scale=None, tlen=None, fft_size=N_FFT,
                momentum=0.0):
    """Griffin & Lim: alternate projections between the given magnitudes (B, T, fft_size // 2 + 1) and consistent STFTs.
    tlen (device int32[B]): per-item frame counts -- item b iterates on its own first tlen[b] frames and signal (see
    istft).
    momentum (alpha, in [0, 1)): the fast Griffin-Lim algorithm of Perraudin, Balazs & Sondergaard (2013).  With c_n =
    STFT(y_{n-1}), iteration n takes its phase from t_n = c_n + alpha (c_n - c_{n-1}) (t_1 = c_1) instead of c_n:
    y_n = iSTFT(mag * t_n / |t_n|).  Only the phase of t_n is used, so alpha is exactly the `momentum` of librosa.griffinlim
    and torchaudio.transforms.GriffinLim: their c_n - alpha / (1 + alpha) c_{n-1} is t_n / (1 + alpha).  0 (default) is
    the plain algorithm on the kernels it has always run, bit for bit; otherwise the projections run the momentum form
    of the fused kernel (include/dv3hip.h: dv3_gl_project_momentum_f32), which keeps c_{n-1} in one (B, T, bins, 2)
    scratch tensor allocated per call (211 MB at 64 x 804 x 513)."""
    momentum = check_momentum(momentum)
    y = istft(mag, init_phasor, hop, convention, window_scale, tlen, fft_size)
    B, T, _ = mag.shape
    if n_iter > 0:
        frames = torch.empty((B, T, fft_size), dtype=torch.float32, device=mag.device)
        y2 = torch.empty_like(y)
        lws = convention == "lws"
        if lws:
            awin, swin = lws_windows(mag.device, hop, window_scale, fft_size)
        if momentum > 0.0:
            cprev = torch.empty((B, T, fft_size // 2 + 1, 2), dtype=torch.float32, device=mag.device)
            ola = "dv3_overlap_add_items_f32_n" if tlen is not None else \
                "dv3_lws_overlap_add_f32_n" if lws else "dv3_overlap_add_f32_n"
            tail = (tlen.data_ptr(), int(lws)) if tlen is not None else ()
            for i in range(n_iter):
                _lib.call("dv3_gl_project_momentum_f32", y.data_ptr(), mag.data_ptr(), awin.data_ptr() if lws else None,
                          swin.data_ptr() if lws else None, cprev.data_ptr(), frames.data_ptr(), B, T, hop,
                          tlen.data_ptr() if tlen is not None else None, int(lws), fft_size, momentum, int(i == 0),
                          _stream())
                _lib.call(ola, frames.data_ptr(), y2.data_ptr(), B, T, hop, *(tail + (fft_size, _stream())))
                y, y2 = y2, y
            return y
        for _ in range(n_iter):
            if tlen is not None:
                _lib.call("dv3_gl_project_items_f32_n", y.data_ptr(), mag.data_ptr(), awin.data_ptr() if lws else None,
                          swin.data_ptr() if lws else None, frames.data_ptr(), B, T, hop, tlen.data_ptr(), int(lws),
                          fft_size, _stream())
                _lib.call("dv3_overlap_add_items_f32_n", frames.data_ptr(), y2.data_ptr(), B, T, hop, tlen.data_ptr(),
                          int(lws), fft_size, _stream())
                y, y2 = y2, y
                continue
            # stft -> unit phase -> x magnitude -> inverse FFT -> window in one launch (the phasors never reach HBM)
            if lws:
                _lib.call("dv3_lws_gl_project_f32_n", y.data_ptr(), mag.data_ptr(), awin.data_ptr(), swin.data_ptr(),
                          frames.data_ptr(), B, T, hop, fft_size, _stream())
                _lib.call("dv3_lws_overlap_add_f32_n", frames.data_ptr(), y2.data_ptr(), B, T, hop, fft_size, _stream())
            else:
                _lib.call("dv3_gl_project_f32_n", y.data_ptr(), mag.data_ptr(), frames.data_ptr(), B, T, hop, fft_size,
                          _stream())
                _lib.call("dv3_overlap_add_f32_n", frames.data_ptr(), y2.data_ptr(), B, T, hop, fft_size, _stream())
            y, y2 = y2, y
    return y


def spsi_phasor(mag, hop, tlen=None, fft_size=N_FFT):
    """Single Pass Spectrogram Inversion (Beauregard, Harish & Wyse 2015): mag (B, T, fft_size // 2 + 1) on the device ->
    unit phasors (B, T, bins, 2), what istft and griffin_lim take as init_phasor -- a starting phase built from the
    magnitudes alone in one pass over the frames.  Per frame every spectral peak's phase advances by hop x the peak's
    instantaneous frequency (the vertex of the parabola through its three bins) and is given to the bins of its lobe;
    include/dv3hip.h (dv3_spsi_phasor_f32) states every step, tests/spsi_ref.py restates it in numpy.  tlen (device
    int32[B]): item b has only its first tlen[b] frames; the rows past them are (1, 0), and its own rows are those of
    its B = 1 call bit for bit."""
    fft_size = check_fft_size(fft_size)
    mag = _c(_chk(mag, "mag"))
    if mag.dim() != 3 or min(mag.shape) < 1:
        raise ValueError("spsi_phasor: non-empty (B, T, bins) magnitudes expected, got %s" % (tuple(mag.shape),))
    B, T, F = mag.shape
    check_bins(F, fft_size, "spsi_phasor")
    if isinstance(hop, bool) or int(hop) != hop or not 0 < hop <= fft_size:
        raise ValueError("spsi_phasor: hop=%r must be an integer in [1, fft_size=%d]" % (hop, fft_size))
    if tlen is not None and (tlen.dtype != torch.int32 or tuple(tlen.shape) != (B,) or tlen.device != mag.device):
        raise ValueError("spsi_phasor: tlen must be int32[%d] on the device of mag" % B)
    phasor = torch.empty((B, T, F, 2), dtype=torch.float32, device=mag.device)
    _lib.call("dv3_spsi_phasor_f32", mag.data_ptr(), phasor.data_ptr(), B, T, int(hop),
              _c(tlen).data_ptr() if tlen is not None else None, fft_size, _stream())
    return phasor


def _start_phasor(mag, cfg, init_phasor, tlen=None):
    """the phasor Griffin-Lim starts from: the caller's, else cfg.griffin_lim_init's ("zero": None, no launch)"""
    if init_phasor is None and cfg.griffin_lim_init == "spsi":
        return spsi_phasor(mag, cfg.hop_size, tlen, cfg.fft_size)
    return init_phasor


# ---------------------------------------------------------------------------------------------
# speaking rate and pitch at vocoding: a warp of the magnitudes Griffin-Lim starts from (csrc/prosody.hip)
# ---------------------------------------------------------------------------------------------
def _numbers(v, what, lo, hi):
    """a scalar or a sequence of numbers in [lo, hi] -> (is_scalar, [floats]); ValueError naming the offending value"""
    scalar = not isinstance(v, (list, tuple, np.ndarray, torch.Tensor))
    vals = [v] if scalar else (v.tolist() if isinstance(v, (np.ndarray, torch.Tensor)) else list(v))
    if not scalar and (len(vals) == 0 or isinstance(vals[0], list)):
        raise ValueError("Prosody: %s=%r must be a number or a flat, non-empty sequence of numbers" % (what, v))
    out = []
    for x in vals:
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not lo <= float(x) <= hi:
            raise ValueError("Prosody: %s=%r must be a number in [%g, %g]" % (what, x, lo, hi))      # (nan fails the test)
        out.append(float(x))
    return scalar, out


class Prosody(object):
    """How an utterance is spoken, applied where it is vocoded (warp_magnitudes): rate, the speaking-rate
    multiplier in [0.25, 4] (above 1 is faster: T frames become about T / rate); semitones in [-24, 24], the pitch shift
    (every frequency times 2 ** (semitones / 12)) -- each a scalar for every item or one value per item;
    preserve_envelope (True): shift the harmonics under the spectral envelope so that formants stay where they are, else
    the whole frame moves along the frequency axis; envelope_hz (400): the half width of the triangular smoother that
    defines the envelope, in Hz -- half_width(cfg) bins, which must lie in [1, DV3_PROSODY_MAX_HALF_WIDTH].
    Refused by value (ValueError naming it)."""

    def __init__(self, rate=1.0, semitones=0.0, preserve_envelope=True, envelope_hz=400.0):
        self._scalar_rate, self.rate = _numbers(rate, "rate", 0.25, 4.0)
        self._scalar_semitones, self.semitones = _numbers(semitones, "semitones", -24.0, 24.0)
        if not self._scalar_rate and not self._scalar_semitones and len(self.rate) != len(self.semitones):
            raise ValueError("Prosody: %d rates and %d semitones" % (len(self.rate), len(self.semitones)))
        if isinstance(envelope_hz, bool) or not isinstance(envelope_hz, (int, float, np.integer, np.floating)) or \
                not 0.0 < float(envelope_hz) < float("inf"):
            raise ValueError("Prosody: envelope_hz=%r must be a positive number of Hz" % (envelope_hz,))
        self.preserve_envelope, self.envelope_hz = bool(preserve_envelope), float(envelope_hz)

    def half_width(self, cfg=None):
        """W = round(envelope_hz * fft_size / sample_rate) (halves up) bins; ValueError outside [1, 64]"""
        cfg = cfg or AudioConfig()
        W = int(np.floor(self.envelope_hz * cfg.fft_size / float(cfg.sample_rate) + 0.5))
        top = _lib.CONSTS["DV3_PROSODY_MAX_HALF_WIDTH"]
        if not 1 <= W <= top:
            raise ValueError("Prosody: envelope_hz=%r is %d bins at fft_size=%d and sample_rate=%r: outside [1, %d]"
                             % (self.envelope_hz, W, cfg.fft_size, cfg.sample_rate, top))
        return W

    def per_item(self, B):
        """-> (rates, semitones), B floats each; a per-item list of another length is refused"""
        out = []
        for scalar, vals, what in ((self._scalar_rate, self.rate, "rate"),
                                   (self._scalar_semitones, self.semitones, "semitones")):
            if not scalar and len(vals) != B:
                raise ValueError("Prosody: %d values of %s=%r for %d items" % (len(vals), what, vals, B))
            out.append(vals * B if scalar else list(vals))
        return out[0], out[1]

    def neutral(self):
        """every rate is 1 and every shift 0: nothing to do"""
        return all(r == 1.0 for r in self.rate) and all(s == 0.0 for s in self.semitones)


def _active(prosody, what):
    """the `prosody=` keyword -> the Prosody to apply, or None when there is none or it changes nothing"""
    if prosody is None:
        return None
    if not isinstance(prosody, Prosody):
        raise ValueError("%s: prosody must be an audio.Prosody, got %r" % (what, prosody))
    return None if prosody.neutral() else prosody


def _active_marks(prosody, B, what):
    """the `prosody=` keyword when it holds ProsodyMarks (one, or a sequence of one or None per item, in frames)
    -> (True, the list of B or None when nothing changes anything); (False, None) when it holds something else"""
    if isinstance(prosody, ProsodyMarks) or (isinstance(prosody, (list, tuple)) and len(prosody) > 0 and
                                             all(m is None or isinstance(m, ProsodyMarks) for m in prosody)):
        return True, item_marks(prosody, B, "frames", what)
    return False, None


def warped_frames(T, rate, cfg=None):
    """T' = max(min_frames, floor((T - 1) / rate + 0.5) + 1): the frames an item of T frames has at speaking rate `rate`
    (host float64, like every other length here)"""
    cfg = cfg or AudioConfig()
    return max(min_frames(cfg.hop_size, cfg.convention, cfg.fft_size),
               int(np.floor((int(T) - 1) / float(rate) + 0.5)) + 1)


def warp_magnitudes(mag, frame_lengths, cfg, prosody):
    """Change rate and pitch of magnitudes on their way into Griffin-Lim: mag (B, T, fft_size // 2 + 1) on the device, what
    magnitudes() made; frame_lengths: B host ints (item b has only its first frame_lengths[b] frames; the rest is never
    read) or None (all T); prosody: a Prosody.  -> (out (B, max T'_b, bins), T' int64[B] on the host), T'_b =
    warped_frames(T_b, rate_b, cfg); item b's rows past T'_b are zero.  Output frame j of item b is the item's source at
    frame j * rate_b (linear interpolation, the last frame held), read along the frequency axis at k / ratio_b -- under
    the envelope when prosody.preserve_envelope; include/dv3hip.h (dv3_prosody_warp_f32) states every step,
    tests/prosody_ref.py restates it.  An item at rate 1 and 0 semitones comes back bit for bit, and every item's rows
    depend on that item alone.  One launch, whatever the settings."""
    cfg = cfg or AudioConfig()
    if not isinstance(prosody, Prosody):
        raise ValueError("warp_magnitudes: prosody must be an audio.Prosody, got %r" % (prosody,))
    mag = _c(_chk(mag, "mag"))
    if mag.dim() != 3 or min(mag.shape) < 1:
        raise ValueError("warp_magnitudes: non-empty (B, T, bins) magnitudes expected, got %s" % (tuple(mag.shape),))
    B, T, F = mag.shape
    check_bins(F, cfg.fft_size, "warp_magnitudes")
    fl = torch.full((B,), T, dtype=torch.int64) if frame_lengths is None else \
        _host_lengths(frame_lengths, B, 1, T, "warp_magnitudes")
    rates, semis = prosody.per_item(B)
    W = prosody.half_width(cfg)
    out_len = torch.tensor([warped_frames(int(n), r, cfg) for n, r in zip(fl, rates)], dtype=torch.int64)
    T_out = int(out_len.max())
    dev = mag.device
    rate = torch.tensor(rates, dtype=torch.float64).to(dev)
    ratio = torch.tensor([2.0 ** (s / 12.0) for s in semis], dtype=torch.float64).to(dev)
    tlen_in, tlen_out = fl.to(torch.int32).to(dev), out_len.to(torch.int32).to(dev)      # (named: both live through the call)
    out = torch.empty((B, T_out, F), dtype=torch.float32, device=dev)
    _lib.call("dv3_prosody_warp_f32", mag.data_ptr(), out.data_ptr(), B, T, T_out, F, tlen_in.data_ptr(),
              tlen_out.data_ptr(), rate.data_ptr(), ratio.data_ptr(), W, int(prosody.preserve_envelope), _stream())
    return out, out_len


# ---------------------------------------------------------------------------------------------
# prosody marks: rate, pitch, level and pauses that vary within an utterance
# ---------------------------------------------------------------------------------------------
class MarksNotApplied(UserWarning):
    """synthesis found no admissible monotonic path for an utterance that carries ProsodyMarks in tokens: there are no
    token bounds to place the marks at, and the utterance was vocoded as if it had none"""


_MARK_LIMITS = (("rate", 0.25, 4.0, 1.0), ("semitones", -24.0, 24.0, 0.0), ("gain_db", -40.0, 20.0, 0.0))
MAX_BREAK_SECONDS = 10.0


def _index(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0:
        raise ValueError("ProsodyMarks: %s=%r must be a non-negative integer" % (what, v))
    return int(v)


class ProsodyMarks(object):
    """How the PARTS of one utterance are spoken -- what <prosody>, <emphasis> and <break> say:
    spans: [(first, last_exclusive, dict(rate=, semitones=, gain_db=)), ...] in ascending order without overlap, each
    value optional -- rate in [0.25, 4] (above 1: faster), semitones in [-24, 24], gain_db in [-40, 20];
    breaks: [(after_index, seconds), ...]: silence of at most MAX_BREAK_SECONDS put in after unit after_index;
    units: "tokens" (input tokens: synthesis.tts_batch(marks=) places them by the utterance's monotonic path) or
    "frames" (frames of the spectrogram: inv_spectrogram_batch(prosody=) takes them as they stand);
    transition_ms: semitones and gain_db glide linearly over this long around a boundary between two parts that follow
    each other without a break (0: they step; the rate always steps); preserve_envelope, envelope_hz: as Prosody takes
    them.  What lies between and around the spans is spoken as the model made it.  The utterance is cut at every span
    edge and every break: at most DV3_PROSODY_MAX_SEGMENTS parts.  Refused by value (ValueError naming it)."""

    def __init__(self, spans=(), breaks=(), units="tokens", transition_ms=0.0, preserve_envelope=True, envelope_hz=400.0):
        if units not in ("tokens", "frames"):
            raise ValueError("ProsodyMarks: units=%r must be \"tokens\" or \"frames\"" % (units,))
        self.units = units
        self._envelope = Prosody(1.0, 0.0, preserve_envelope, envelope_hz)
        self.preserve_envelope, self.envelope_hz = self._envelope.preserve_envelope, self._envelope.envelope_hz
        if isinstance(transition_ms, bool) or not isinstance(transition_ms, (int, float, np.integer, np.floating)) or \
                not 0.0 <= float(transition_ms) < float("inf"):
            raise ValueError("ProsodyMarks: transition_ms=%r must be a number of milliseconds >= 0" % (transition_ms,))
        self.transition_ms = float(transition_ms)
        self.spans, at = [], 0
        for span in spans:
            if not isinstance(span, (list, tuple)) or len(span) != 3 or not isinstance(span[2], dict):
                raise ValueError("ProsodyMarks: span %r must be (first, last_exclusive, dict of settings)" % (span,))
            first, last = _index(span[0], "span first"), _index(span[1], "span last_exclusive")
            if last <= first:
                raise ValueError("ProsodyMarks: span [%d, %d) is empty" % (first, last))
            if first < at:
                raise ValueError("ProsodyMarks: span [%d, %d) overlaps or precedes the span that ends at %d" % (first, last, at))
            unknown = sorted(set(span[2]) - {name for name, _, _, _ in _MARK_LIMITS})
            if unknown:
                raise ValueError("ProsodyMarks: span [%d, %d) has unknown settings %r (rate, semitones, gain_db)"
                                 % (first, last, unknown))
            vals = []
            for name, lo, hi, dflt in _MARK_LIMITS:
                x = span[2].get(name, dflt)
                if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not lo <= float(x) <= hi:
                    raise ValueError("ProsodyMarks: %s=%r must be a number in [%g, %g]" % (name, x, lo, hi))
                vals.append(float(x))
            self.spans.append((first, last) + tuple(vals))
            at = last
        self.breaks = {}
        for brk in breaks:
            if not isinstance(brk, (list, tuple)) or len(brk) != 2:
                raise ValueError("ProsodyMarks: break %r must be (after_index, seconds)" % (brk,))
            after, sec = _index(brk[0], "break after_index"), brk[1]
            if isinstance(sec, bool) or not isinstance(sec, (int, float, np.integer, np.floating)) or \
                    not 0.0 <= float(sec) <= MAX_BREAK_SECONDS:
                raise ValueError("ProsodyMarks: break seconds=%r must be a number in [0, %g]" % (sec, MAX_BREAK_SECONDS))
            if after in self.breaks:
                raise ValueError("ProsodyMarks: two breaks after index %d" % after)
            self.breaks[after] = float(sec)
        cuts = {c for s in self.spans for c in s[:2] if c > 0} | {a + 1 for a in self.breaks}
        self.cuts = sorted(cuts)
        top = _lib.CONSTS["DV3_PROSODY_MAX_SEGMENTS"]
        if len(self.cuts) + 1 > top:
            raise ValueError("ProsodyMarks: %d segments (one more than the span edges and breaks), at most %d"
                             % (len(self.cuts) + 1, top))

    def half_width(self, cfg=None):
        return self._envelope.half_width(cfg)

    def neutral(self):
        """no span changes anything and no break is longer than nothing"""
        return all(s[2:] == (1.0, 0.0, 0.0) for s in self.spans) and not any(self.breaks.values())

    def ramp_frames(self, cfg=None):
        """transition_ms in frames (halves up); ValueError beyond DV3_PROSODY_MAX_RAMP"""
        cfg = cfg or AudioConfig()
        R = int(np.floor(self.transition_ms * 1e-3 * cfg.sample_rate / float(cfg.hop_size) + 0.5))
        if R > _lib.CONSTS["DV3_PROSODY_MAX_RAMP"]:
            raise ValueError("ProsodyMarks: transition_ms=%r is %d frames, at most %d" % (
                self.transition_ms, R, _lib.CONSTS["DV3_PROSODY_MAX_RAMP"]))
        return R

    def key(self):
        """the settings a launch shares: marks with equal keys can be planned and warped together"""
        return (self.preserve_envelope, self.envelope_hz, self.transition_ms)

    def segments(self, cfg=None):
        """the segment table: dict of "start" (int64[S], each segment's first unit; segment s ends where s + 1 starts, the
        last one with the utterance), "rate", "semitones", "gain_db" (float64[S]) and "break_frames" (int32[S]: seconds
        times sample_rate / hop_size, halves up -- the silence after the segment).  Gaps between spans are neutral."""
        cfg = cfg or AudioConfig()
        start = [0] + self.cuts
        rows = []
        for s, c in enumerate(start):
            vals = (1.0, 0.0, 0.0)
            for first, last, rate, semi, db in self.spans:
                if first <= c < last:
                    vals = (rate, semi, db)
            end = start[s + 1] if s + 1 < len(start) else None
            sec = self.breaks.get(end - 1, 0.0) if end is not None else 0.0
            rows.append(vals + (int(np.floor(sec * cfg.sample_rate / float(cfg.hop_size) + 0.5)),))
        cols = list(zip(*rows))
        return {"start": np.asarray(start, dtype=np.int64), "rate": np.asarray(cols[0], dtype=np.float64),
                "semitones": np.asarray(cols[1], dtype=np.float64), "gain_db": np.asarray(cols[2], dtype=np.float64),
                "break_frames": np.asarray(cols[3], dtype=np.int32)}


def item_marks(marks, B, units, what):
    """one ProsodyMarks, or a sequence of B entries each a ProsodyMarks or None -> None when nothing changes anything,
    else the list of B (None: that item is left alone).  Another type, count or unit is refused."""
    if marks is None:
        return None
    items = [marks] * B if isinstance(marks, ProsodyMarks) else list(marks)
    if len(items) != B:
        raise ValueError("%s: %d marks for %d items" % (what, len(items), B))
    for m in items:
        if m is not None and not isinstance(m, ProsodyMarks):
            raise ValueError("%s: marks must be audio.ProsodyMarks (or None), got %r" % (what, m))
        if m is not None and m.units != units:
            raise ValueError("%s: marks in %r given where %r are expected" % (what, m.units, units))
    items = [None if m is None or m.neutral() else m for m in items]
    return items if any(m is not None for m in items) else None


def marks_tables(marks, cfg=None):
    """a list of ProsodyMarks (None: a neutral item) that share key() -> the padded host tables of the batch: dict of
    "nseg" int32[B], "start" int64[B][S + 1] (a segment's first unit; padded with the largest int32), "rate", "semitones",
    "gain_db" float64[B][S], "break_frames" int32[B][S], S the most segments of any item"""
    keys = {m.key() for m in marks if m is not None}
    if len(keys) > 1:
        raise ValueError("plan_prosody: the marks of one call must share preserve_envelope, envelope_hz and transition_ms, "
                         "got %s" % sorted(keys))
    segs = [(m or ProsodyMarks()).segments(cfg) for m in marks]
    B, S = len(segs), max(len(t["rate"]) for t in segs)
    out = {"nseg": np.array([len(t["rate"]) for t in segs], dtype=np.int32),
           "start": np.full((B, S + 1), 2 ** 31 - 1, dtype=np.int64), "rate": np.ones((B, S)),
           "semitones": np.zeros((B, S)), "gain_db": np.zeros((B, S)), "break_frames": np.zeros((B, S), dtype=np.int32)}
    for b, t in enumerate(segs):
        n = len(t["rate"])
        out["start"][b, :n] = t["start"]
        for k in ("rate", "semitones", "gain_db", "break_frames"):
            out[k][b, :n] = t[k]
    return out


def plan_prosody(bounds, frame_lengths, marks, cfg=None, usable=None):
    """Where every output frame of a batch under ProsodyMarks comes from (dv3_curve_plan_f64, dv3_curve_fill_f64;
    include/dv3hip.h states both, tests/prosody_curve_ref.py restates them).  marks: B entries, each a ProsodyMarks or
    None, sharing key(); frame_lengths: B host ints, each item's source frames; bounds: device int (B, S + 1), the source
    frame every segment starts at (column s for segment s; the kernels clamp them, make them non-decreasing and end the
    last segment with the item) -- None: the marks are in frames and their own starts are the bounds; usable: None or a
    device bool[B] -- an item where it is false is planned as if it had no marks (synthesis: no monotonic path), all on
    the device.  ONE host read sits between the two launches: the items' output frame counts T'_b, which size the tables
    and give Griffin-Lim its lengths (`usable` rides in the same transfer); there is no other synchronisation.
    -> dict: "out_lengths" int64[B] (host), "tlen_in", "tlen_out" int32[B], "nseg", "c" (the repaired bounds) and "o"
    int32 (B, S + 1), "rate" float64 (B, S), "break_frames" int32 (B, S), "pos", "ratio" float64 and "gain" float32
    (B, max T'_b): device tensors; "usable": B host bools; "W", "preserve_envelope": the warp's settings."""
    cfg = cfg or AudioConfig()
    marks = list(marks)
    B = len(marks)
    t = marks_tables(marks, cfg)
    S = t["rate"].shape[1]
    first = next((m for m in marks if m is not None), None) or ProsodyMarks()
    W, R = first.half_width(cfg), first.ramp_frames(cfg)
    fl = _host_lengths(frame_lengths, B, 1, 2 ** 31 - 1, "plan_prosody")
    if bounds is None:
        if any(m is not None and m.units != "frames" for m in marks):
            raise ValueError("plan_prosody: marks in tokens need the token bounds in frames")
        bounds = torch.from_numpy(np.minimum(t["start"], int(fl.max())).astype(np.int32))
    if not torch.is_tensor(bounds) or tuple(bounds.shape) != (B, S + 1):
        raise ValueError("plan_prosody: bounds must be a (%d, %d) integer tensor" % (B, S + 1))
    dev = bounds.device if bounds.is_cuda else torch.device("cuda", torch.cuda.current_device())
    put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    bounds = _c(bounds.to(dev).to(torch.int32))
    nseg, rate = put(t["nseg"], torch.int32), put(t["rate"], torch.float64)
    semi, db, brk = put(t["semitones"], torch.float64), put(t["gain_db"], torch.float64), put(t["break_frames"], torch.int32)
    tlen_in = fl.to(torch.int32).to(dev)
    if usable is not None:                 # an item without a usable path: one neutral segment, chosen on the device
        ok = usable.to(dev).to(torch.bool)
        rate, semi, db = [torch.where(ok[:, None], v, torch.full_like(v, x)) for v, x in ((rate, 1.0), (semi, 0.0), (db, 0.0))]
        brk, nseg = torch.where(ok[:, None], brk, torch.zeros_like(brk)), torch.where(ok, nseg, torch.ones_like(nseg))
    T_in = int(fl.max())
    o = torch.empty((B, S + 1), dtype=torch.int32, device=dev)
    tlen_out = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.call("dv3_curve_plan_f64", tlen_in.data_ptr(), B, T_in, S, nseg.data_ptr(), bounds.data_ptr(), rate.data_ptr(),
              brk.data_ptr(), min_frames(cfg.hop_size, cfg.convention, cfg.fft_size), o.data_ptr(), tlen_out.data_ptr(),
              _stream())
    host = (tlen_out if usable is None else torch.stack([tlen_out, ok.to(torch.int32)])).cpu()      # the one host read
    out_len = (host if usable is None else host[0]).to(torch.int64)
    T_out = int(out_len.max())
    pos = torch.empty((B, T_out), dtype=torch.float64, device=dev)
    ratio, gain = torch.empty_like(pos), torch.empty((B, T_out), dtype=torch.float32, device=dev)
    _lib.call("dv3_curve_fill_f64", tlen_in.data_ptr(), B, T_in, S, nseg.data_ptr(), bounds.data_ptr(), rate.data_ptr(),
              semi.data_ptr(), db.data_ptr(), brk.data_ptr(), o.data_ptr(), tlen_out.data_ptr(), T_out, R, pos.data_ptr(),
              ratio.data_ptr(), gain.data_ptr(), _stream())
    n = tlen_in[:, None]
    col = torch.arange(S + 1, device=dev)[None, :]
    c = torch.cummax(torch.where(col == 0, torch.zeros_like(bounds), torch.minimum(bounds.clamp(min=0), n)), dim=1)[0]
    c = torch.where(col >= nseg[:, None], n.expand_as(c), c).to(torch.int32)
    return {"out_lengths": out_len, "tlen_in": tlen_in, "tlen_out": tlen_out, "nseg": nseg, "c": c, "o": o, "rate": rate,
            "break_frames": brk, "pos": pos, "ratio": ratio, "gain": gain, "W": W, "preserve_envelope": first.preserve_envelope,
            "usable": [True] * B if usable is None else [bool(v) for v in host[1]]}


def plan_map(plan, frames, side="start"):
    """Source frames -> output frames under a plan, in float64, for timings: frames (B, N) integer or float tensor on the
    plan's device.  A frame x in segment s (c_s <= x < c_{s+1} for side "start", c_s < x <= c_{s+1} for "end": where a
    token starts, and where one ends) maps to o_s + len_s (x - c_s) / (c_{s+1} - c_s), len_s = o_{s+1} - break_s - o_s the
    segment's own output frames: the segment's source frames spread evenly over them (len_s is (c_{s+1} - c_s) / rate_s
    rounded to whole frames), so a token that ends at a break ends BEFORE the silence, the next one starts after it --
    the gap is break_s frames exactly -- and without a break the two meet.  Monotone in x; torch only, no
    synchronisation (it runs on host tensors just as well)."""
    if side not in ("start", "end"):
        raise ValueError("plan_map: side=%r must be \"start\" or \"end\"" % (side,))
    c, o = plan["c"].to(torch.float64), plan["o"].to(torch.float64)
    x = frames.to(torch.float64)
    s = torch.searchsorted(c.contiguous(), x.contiguous(), right=(side == "start")) - 1
    s = torch.minimum(s.clamp(min=0), (plan["nseg"].to(torch.int64) - 1)[:, None])
    take = lambda v: torch.gather(v, 1, s)
    c0, o0 = take(c[:, :-1]), take(o[:, :-1])
    width, frames_out = take(c[:, 1:]) - c0, take(o[:, 1:]) - take(plan["break_frames"].to(torch.float64)) - o0
    along = torch.where(width > 0, (x - c0) / width.clamp(min=1.0), torch.zeros_like(x)).clamp(0.0, 1.0)
    return o0 + frames_out * along


def warp_magnitudes_curve(mag, frame_lengths, cfg, pos, ratio, gain, out_lengths, preserve_envelope=True,
                          envelope_hz=400.0, check=True):
    """warp_magnitudes along per-output-frame curves (dv3_curve_warp_f32; include/dv3hip.h states every step): pos, ratio
    float64 and gain float32, each (B, T_out) on the device -- output frame j of item b is the item's source at frame
    pos[b, j] (the last frame held beyond it; a negative or NaN position is a silent frame), read along the frequency
    axis at k / ratio[b, j] and multiplied by gain[b, j]; out_lengths: B host ints in [1, T_out], rows past them are
    zero.  A caller with a pitch track passes ratio = target / f0 (audio.yin_items).  check: the gains must be finite and
    >= 0 and the ratios positive where they are used -- the kernel does not look -- which costs one host read; plans made
    by plan_prosody are inside the limits by construction and skip it.  -> out (B, T_out, bins).  One launch."""
    cfg = cfg or AudioConfig()
    mag = _c(_chk(mag, "mag"))
    if mag.dim() != 3 or min(mag.shape) < 1:
        raise ValueError("warp_magnitudes_curve: non-empty (B, T, bins) magnitudes expected, got %s" % (tuple(mag.shape),))
    B, T, F = mag.shape
    check_bins(F, cfg.fft_size, "warp_magnitudes_curve")
    fl = torch.full((B,), T, dtype=torch.int64) if frame_lengths is None else \
        _host_lengths(frame_lengths, B, 1, T, "warp_magnitudes_curve")
    W = Prosody(1.0, 0.0, preserve_envelope, envelope_hz).half_width(cfg)
    for name, v, dt in (("pos", pos, torch.float64), ("ratio", ratio, torch.float64), ("gain", gain, torch.float32)):
        if not torch.is_tensor(v) or v.dtype != dt or v.dim() != 2 or v.shape[0] != B or v.shape[1] < 1 or \
                v.shape != pos.shape or v.device != mag.device:
            raise ValueError("warp_magnitudes_curve: %s must be a (%d, T_out) %s tensor on the device of mag" % (name, B, dt))
    T_out = int(pos.shape[1])
    ol = _host_lengths(out_lengths, B, 1, T_out, "warp_magnitudes_curve (out_lengths)")
    if check:
        live = (torch.arange(T_out)[None, :] < ol[:, None]).to(mag.device) & (pos >= 0)
        bad = live & ~(torch.isfinite(gain) & (gain >= 0) & torch.isfinite(ratio) & (ratio > 0))
        if bool(bad.any()):
            b, j = [int(v) for v in torch.nonzero(bad)[0]]
            raise ValueError("warp_magnitudes_curve: gain=%r, ratio=%r at item %d, frame %d: a finite gain >= 0 and a finite "
                             "ratio > 0 expected" % (float(gain[b, j]), float(ratio[b, j]), b, j))
    pos, ratio, gain = _c(pos), _c(ratio), _c(gain)
    tlen_in, tlen_out = fl.to(torch.int32).to(mag.device), ol.to(torch.int32).to(mag.device)
    out = torch.empty((B, T_out, F), dtype=torch.float32, device=mag.device)
    _lib.call("dv3_curve_warp_f32", mag.data_ptr(), out.data_ptr(), B, T, T_out, F, tlen_in.data_ptr(), tlen_out.data_ptr(),
              pos.data_ptr(), ratio.data_ptr(), gain.data_ptr(), W, int(bool(preserve_envelope)), _stream())
    return out


def warp_magnitudes_marks(mag, frame_lengths, cfg, marks, bounds=None, usable=None):
    """plan_prosody and warp_magnitudes_curve in a row -> (out (B, max T'_b, bins), the plan)"""
    cfg = cfg or AudioConfig()
    B, T = mag.shape[0], mag.shape[1]
    fl = torch.full((B,), T, dtype=torch.int64) if frame_lengths is None else \
        _host_lengths(frame_lengths, B, 1, T, "warp_magnitudes_marks")
    if bounds is None:
        if any(m is not None and m.units != "frames" for m in marks):
            raise ValueError("warp_magnitudes_marks: marks in tokens need the token bounds in frames")
        bounds = torch.from_numpy(np.minimum(marks_tables(marks, cfg)["start"], T).astype(np.int32)).to(mag.device)
    plan = plan_prosody(bounds, fl, marks, cfg, usable)
    first = next(m for m in marks if m is not None)
    out = warp_magnitudes_curve(mag, fl, cfg, plan["pos"], plan["ratio"], plan["gain"], plan["out_lengths"],
                                first.preserve_envelope, first.envelope_hz, check=False)
    return out, plan


def inv_preemphasis_(y, coef):
    """de-emphasis filter (audio.py:26-28) of (B, L) waveforms -> a new tensor"""
    out = torch.empty_like(y)
    _lib.call("dv3_deemphasis_f32", y.data_ptr(), out.data_ptr(), y.shape[0], y.shape[1], float(coef), _stream())
    return out


def inv_spectrogram_batch(linear_outputs, cfg=None, init_phasor=None, frame_lengths=None, prosody=None):
    """(B, T, fft_size // 2 + 1) device tensor (model linear_outputs) -> waveforms on the device: (B, (T+1)*hop -
    fft_size) on the lws framing (what the reference's processor.istft returns for T frames), (B, hop*(T-1)) on the torch
    framing.  A spectrogram of another width than cfg.fft_size // 2 + 1 is refused (ValueError).
    init_phasor (B, T, bins, 2): the phase Griffin-Lim starts from; None: cfg.griffin_lim_init -- zero phase, or
    spsi_phasor of the magnitudes made here (per item with frame_lengths).  An explicit init_phasor wins.
    frame_lengths (B host ints): a batch of utterances padded to T frames; item b is inverted from its own first
    frame_lengths[b] frames exactly as its B = 1 call on the trimmed spectrogram, its samples past its own length are
    zero.  -> (waveforms, sample lengths (int64[B], host)) in that case.
    prosody (an audio.Prosody): speaking rate and pitch -- the magnitudes go through warp_magnitudes before the phase
    is built, item b is inverted from its T'_b = warped_frames(T_b, rate_b) frames (T_b = T without frame_lengths) and the
    return is (waveforms, sample lengths) either way, the lengths num_samples(T'_b).  An init_phasor cannot be given
    with it (it would describe the frames before the warp).  None, or one whose every rate is 1 and shift 0: nothing is
    launched for it and the call is the one without the keyword.
    prosody may instead be an audio.ProsodyMarks in frames, or a list of one (or None) per item, which must share their
    envelope and transition settings: rate, pitch, level and pauses that vary within the item --
    plan_prosody, then warp_magnitudes_curve in the place of warp_magnitudes; everything above holds, with T'_b the
    plan's frame counts (one host read).  Marks that change nothing launch nothing."""
    cfg = cfg or AudioConfig()
    if linear_outputs.dim() != 3:
        raise ValueError("inv_spectrogram_batch: a (B, T, bins) spectrogram expected, got %s" % (tuple(linear_outputs.shape),))
    check_bins(linear_outputs.shape[-1], cfg.fft_size, "inv_spectrogram_batch")
    is_marks, marks = _active_marks(prosody, linear_outputs.shape[0], "inv_spectrogram_batch")
    prosody = marks if is_marks else _active(prosody, "inv_spectrogram_batch")
    if prosody is not None:
        if init_phasor is not None:
            raise ValueError("inv_spectrogram_batch: init_phasor describes the frames before the warp; it cannot be "
                             "combined with prosody")
        if frame_lengths is None:
            frame_lengths = [linear_outputs.shape[1]] * linear_outputs.shape[0]
        return _inv_spectrogram_items(linear_outputs, cfg, None, frame_lengths, prosody)
    if frame_lengths is not None:
        return _inv_spectrogram_items(linear_outputs, cfg, init_phasor, frame_lengths)
    mag = magnitudes(linear_outputs, cfg)
    y = griffin_lim(mag, cfg.hop_size, cfg.griffin_lim_iters, _start_phasor(mag, cfg, init_phasor), cfg.convention,
                    cfg.window_scale, fft_size=cfg.fft_size, momentum=cfg.griffin_lim_momentum)
    return inv_preemphasis_(y, cfg.preemphasis)


def inv_spectrogram(spectrogram, cfg=None, device="cuda:0"):
    """Drop-in for audio.inv_spectrogram (audio.py:37-43): (fft_size // 2 + 1, T) numpy -> waveform numpy."""
    s = torch.as_tensor(np.ascontiguousarray(np.asarray(spectrogram, dtype=np.float32).T)).unsqueeze(0)
    y = inv_spectrogram_batch(s.to(device), cfg)
    return y[0].cpu().numpy()


def _inv_spectrogram_items(linear_outputs, cfg, init_phasor, frame_lengths, prosody=None, bounds=None, usable=None,
                           want_plan=False):
    """prosody: None, a Prosody, or a list of ProsodyMarks / None per item -- then bounds, usable: plan_prosody's (None:
    marks in frames), and with want_plan the plan is a third element of the return"""
    B, T = linear_outputs.shape[0], linear_outputs.shape[1]
    fl = torch.as_tensor(frame_lengths).reshape(-1).to(torch.int64).cpu()
    hop, n_fft = cfg.hop_size, cfg.fft_size
    tmin = min_frames(hop, cfg.convention, n_fft)
    if fl.numel() != B or int(fl.min()) < tmin or int(fl.max()) > T:
        raise ValueError("inv_spectrogram_batch: %d frame lengths in [%d, %d] expected, got %s" % (
            B, tmin, T, fl.tolist()))
    mag = magnitudes(linear_outputs, cfg)
    if isinstance(prosody, list):      # ProsodyMarks in frames: the items have their planned frame counts
        mag, plan = warp_magnitudes_marks(mag, fl, cfg, prosody, bounds, usable)
        fl = plan["out_lengths"]
    elif prosody is not None:          # from here on the items have their warped frame counts
        mag, fl = warp_magnitudes(mag, fl, cfg, prosody)
    tlen = fl.to(torch.int32).to(linear_outputs.device)
    y = griffin_lim(mag, hop, cfg.griffin_lim_iters, _start_phasor(mag, cfg, init_phasor, tlen), cfg.convention,
                    cfg.window_scale, tlen, n_fft, cfg.griffin_lim_momentum)
    lengths = torch.tensor([num_samples(int(n), hop, cfg.convention, n_fft) for n in fl], dtype=torch.int64)
    out = torch.empty_like(y)
    _lib.call("dv3_deemphasis_items_f32", y.data_ptr(), out.data_ptr(), B, y.shape[1],
              lengths.to(torch.int32).to(y.device).data_ptr(), float(cfg.preemphasis), _stream())
    return (out, lengths, plan) if want_plan else (out, lengths)


def inv_spectrogram_marks(linear_outputs, cfg, frame_lengths, marks, bounds, usable=None):
    """inv_spectrogram_batch(..., prosody=marks) for marks whose bounds the caller brings (synthesis: token bounds from the
    monotonic path, device int (B, S + 1) source frames; usable: device bool[B], false where there is no path)
    -> (waveforms, sample lengths, the plan of plan_prosody)"""
    cfg = cfg or AudioConfig()
    check_bins(linear_outputs.shape[-1], cfg.fft_size, "inv_spectrogram_marks")
    return _inv_spectrogram_items(linear_outputs, cfg, None, frame_lengths, list(marks), bounds, usable, want_plan=True)


# ---------------------------------------------------------------------------------------------
# ragged forward analysis: features of utterances of different lengths in one launch (preprocessing,
# on-the-fly training features; audio.py:31-35,46-51 as ljspeech.py:40-76 calls them)
# ---------------------------------------------------------------------------------------------
_MEL_CACHE = {}


def mel_tables(device, sample_rate=22050, num_mels=80, fmin=125.0, fmax=7600.0, fft_size=N_FFT):
    """(basis (num_mels, fft_size // 2 + 1) float32, band int32 (num_mels, 2)) on `device`: band[m] = [first, last + 1) of
    filter m's nonzero bins (the kernel's dot skips the bins outside it -- exact zeros, so the fp32 sum is the same)"""
    key = (str(device), int(sample_rate), int(num_mels), float(fmin), float(fmax), int(fft_size))
    if key not in _MEL_CACHE:
        w = mel_basis(sample_rate, fft_size, num_mels, fmin, fmax)
        _MEL_CACHE[key] = (torch.from_numpy(w).to(device), torch.from_numpy(filter_bands_np(w)).to(device))
    return _MEL_CACHE[key]


def filter_bands_np(w):
    """(num_mels, 2) int32: band[m] = [first, last + 1) of filter m's nonzero bins, (0, 0) for an empty filter"""
    band = np.zeros((w.shape[0], 2), dtype=np.int32)
    for m in range(w.shape[0]):
        nz = np.nonzero(w[m])[0]
        band[m] = (nz[0], nz[-1] + 1) if nz.size else (0, 0)
    return band


def bin_bands_np(band, n_bins):
    """(n_bins, 2) int32 from filter_bands_np's table: [first, last + 1) of the filters whose band holds bin k, (0, 0)
    for a bin under no filter.  A filterbank whose filters over some bin are not a contiguous range is refused (the
    inversion kernel walks the range)."""
    band = np.asarray(band, dtype=np.int64)
    k = np.arange(int(n_bins), dtype=np.int64)[:, None]
    over = (band[None, :, 0] <= k) & (k < band[None, :, 1])                  # (n_bins, num_mels)
    count = over.sum(axis=1)
    first = np.where(count > 0, over.argmax(axis=1), 0)
    last = np.where(count > 0, over.shape[1] - over[:, ::-1].argmax(axis=1), 0)
    if np.any(last - first != count):
        raise ValueError("bin_bands_np: the filters over bin %d are not a contiguous range"
                         % int(np.nonzero(last - first != count)[0][0]))
    return np.stack([first, last], axis=1).astype(np.int32)


_MEL_INVERSE_CACHE = {}


def mel_inverse_tables(device, sample_rate=22050, num_mels=80, fmin=125.0, fmax=7600.0, fft_size=N_FFT):
    """mel_tables' (basis, band) with what the inversion adds, cached beside them: (basis, band, bin_band int32
    (fft_size // 2 + 1, 2) on `device`, 1 / sum(basis) as a float)"""
    key = (str(device), int(sample_rate), int(num_mels), float(fmin), float(fmax), int(fft_size))
    if key not in _MEL_INVERSE_CACHE:
        basis, band = mel_tables(device, sample_rate, num_mels, fmin, fmax, fft_size)
        w = mel_basis(sample_rate, fft_size, num_mels, fmin, fmax)
        total = float(w.astype(np.float64).sum())
        if not total > 0.0:
            raise ValueError("mel_inverse_tables: the filterbank (%d bands, %g .. %g Hz at %d Hz, fft_size=%d) is empty"
                             % (num_mels, fmin, fmax, sample_rate, fft_size))
        bins = torch.from_numpy(bin_bands_np(filter_bands_np(w), w.shape[1])).to(device)
        _MEL_INVERSE_CACHE[key] = (basis, band, bins, 1.0 / total)
    return _MEL_INVERSE_CACHE[key]


class MelInverse(object):
    """Options of the mel-to-linear inversion (mel_to_linear): iters, the number of multiplicative updates, an int in
    [0, DV3_MELINV_MAX_ITERS] (0: the flat start; 32 leaves a mean round-trip error below 1e-3 of the normalised range
    on speech-like frames); fmin, fmax: the band edges in Hz the mel was made with (hparams.fmin /
    fmax), 0 <= fmin < fmax.  Refused by value (ValueError naming it)."""

    def __init__(self, iters=32, fmin=125.0, fmax=7600.0):
        top = _lib.CONSTS["DV3_MELINV_MAX_ITERS"]
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= int(iters) <= top:
            raise ValueError("MelInverse: iters=%r must be an int in [0, %d]" % (iters, top))
        number = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))
        if not number(fmin) or not number(fmax) or not 0.0 <= float(fmin) < float(fmax) < float("inf"):
            raise ValueError("MelInverse: fmin=%r, fmax=%r must be numbers with 0 <= fmin < fmax" % (fmin, fmax))
        self.iters, self.fmin, self.fmax = int(iters), float(fmin), float(fmax)


_CEPSTRA_CACHE = {}


def mel_cepstra_table_np(num_mels, order):
    """(num_mels, order) float64: column k - 1 is (1 / sqrt 2) (1 / M) cos(pi k (m + 1/2) / M), k = 1 .. order"""
    M = int(num_mels)
    if not 1 <= int(order) <= M - 1:
        raise ValueError("mel_cepstra: order = %d outside [1, %d] (M = %d mel bands; c0 is left out)" % (order, M - 1, M))
    m = np.arange(M, dtype=np.float64)[:, None] + 0.5
    k = np.arange(1, int(order) + 1, dtype=np.float64)[None, :]
    return np.cos(np.pi * k * m / M) / (np.sqrt(2.0) * M)


def mel_cepstra(mel, cfg=None, order=13):
    """Cepstral features of the model's and the dataset's NORMALISED mel spectrogram, (..., M) in [0, 1] -> (..., order):

        f_k = (1 / sqrt 2) (1 / M) sum_m dB_m cos(pi k (m + 1/2) / M),   k = 1 .. order   (c0, the level, is left out)
        dB  = clip(mel, 0, 1) * (-cfg.min_level_db) + cfg.min_level_db

    With c_k the cepstrum of the natural-log amplitude (ln a = dB ln 10 / 20) and the usual
    MCD = (10 / ln 10) sqrt(2 sum_k (delta c_k)^2), the Euclidean distance of two feature vectors IS the frame's
    mel-cepstral distortion in dB -- which is what ops.dtw sums along its path (synthesis.mel_distortion).
    These are cepstra of the M-band (80) mel spectrogram, NOT SPTK mel-generalised cepstra of a spectral envelope: the
    figures compare checkpoints, presets and ablations of this model with each other, not with MCD values quoted in
    papers.  One matmul against a cached (M, order) table; any device (no kernel of its own)."""
    cfg = cfg or AudioConfig()
    M = int(mel.shape[-1])
    key = (str(mel.device), M, int(order))
    if key not in _CEPSTRA_CACHE:
        _CEPSTRA_CACHE[key] = torch.from_numpy(mel_cepstra_table_np(M, order).astype(np.float32)).to(mel.device)
    span = -float(cfg.min_level_db)
    db = mel.to(torch.float32).clamp(0.0, 1.0) * span - span
    return torch.matmul(db, _CEPSTRA_CACHE[key])


# ---------------------------------------------------------------------------------------------
# vocoding from a mel spectrogram: the filterbank inverted per frame, then the path above
# ---------------------------------------------------------------------------------------------
def _host_lengths(frame_lengths, B, lo, hi, what):
    fl = torch.as_tensor(frame_lengths).reshape(-1).to(torch.int64).cpu()
    if fl.numel() != B or int(fl.min()) < lo or int(fl.max()) > hi:
        raise ValueError("%s: %d frame lengths in [%d, %d] expected, got %s" % (what, B, lo, hi, fl.tolist()))
    return fl


def mel_to_linear(mel, cfg=None, frame_lengths=None, upsample=1, options=None):
    """(B, T, num_mels) normalised mel on the device (the model's mel outputs, or the rows features_items / preprocess
    write) -> (B, T * upsample, cfg.fft_size // 2 + 1) normalised linear spectrogram, the model's linear_outputs format:
    per frame the non-negative magnitudes s that best explain the mel amplitudes under the filterbank W =
    mel_basis(cfg.sample_rate, cfg.fft_size, num_mels, options.fmin, options.fmax) -- options.iters multiplicative
    updates s <- s * W^T a / W^T W s from a flat start (include/dv3hip.h: dv3_mel_to_linear_f32 states every step).
    num_mels is mel's last dimension.  upsample (1 .. 16): output frame t is interpolated in the normalised domain
    between mel frames t // upsample and the next one of the same item (frame i * upsample is mel frame i exactly; the
    last upsample - 1 frames hold the item's last frame).  frame_lengths (B host ints, in mel frames, 0 .. T): item b has
    only its first frame_lengths[b] frames; its output rows past upsample * frame_lengths[b] are zero.  Every row depends
    on its own item alone.  Bins under no filter (outside fmin .. fmax) come back as 0.  options: a MelInverse."""
    cfg = cfg or AudioConfig()
    opt = options if options is not None else MelInverse()
    if not isinstance(opt, MelInverse):
        raise ValueError("mel_to_linear: options must be a MelInverse, got %r" % (options,))
    mel = _c(_chk(mel, "mel"))
    if mel.dim() != 3 or min(mel.shape) < 1:
        raise ValueError("mel_to_linear: a non-empty (B, T, num_mels) mel expected, got %s" % (tuple(mel.shape),))
    B, T, M = mel.shape
    if isinstance(upsample, bool) or not isinstance(upsample, (int, np.integer)) or not 1 <= int(upsample) <= 16:
        raise ValueError("mel_to_linear: upsample=%r must be an int in [1, 16]" % (upsample,))
    if M > _lib.CONSTS["DV3_MELINV_MAX_MELS"]:
        raise ValueError("mel_to_linear: %d mel bands, at most %d" % (M, _lib.CONSTS["DV3_MELINV_MAX_MELS"]))
    u, F = int(upsample), cfg.fft_size // 2 + 1
    tlen = None
    if frame_lengths is not None:
        tlen = _host_lengths(frame_lengths, B, 0, T, "mel_to_linear").to(torch.int32).to(mel.device)
    basis, band, bins, inv_sum = mel_inverse_tables(mel.device, cfg.sample_rate, M, opt.fmin, opt.fmax, cfg.fft_size)
    lin = torch.empty((B, T * u, F), dtype=torch.float32, device=mel.device)
    _lib.call("dv3_mel_to_linear_f32", mel.data_ptr(), tlen.data_ptr() if tlen is not None else None, basis.data_ptr(),
              band.data_ptr(), bins.data_ptr(), inv_sum, lin.data_ptr(), B, T, M, F, u, opt.iters,
              float(cfg.min_level_db), float(cfg.ref_level_db), _stream())
    return lin


def inv_melspectrogram_batch(mel, cfg=None, frame_lengths=None, upsample=1, options=None, init_phasor=None):
    """(B, T, num_mels) normalised mel on the device -> waveforms: exactly inv_spectrogram_batch(mel_to_linear(mel, cfg,
    frame_lengths, upsample, options), cfg, init_phasor, frame_lengths * upsample), with its return forms (the waveforms;
    with frame_lengths, in mel frames: (waveforms, sample lengths)).  For speaking rate and pitch write that composition
    out and give inv_spectrogram_batch the prosody= keyword (synthesis.tts_batch(from_mel=True, rate=...) does)."""
    cfg = cfg or AudioConfig()
    lin = mel_to_linear(mel, cfg, frame_lengths, upsample, options)
    if frame_lengths is None:
        return inv_spectrogram_batch(lin, cfg, init_phasor)
    fl = torch.as_tensor(frame_lengths).reshape(-1).to(torch.int64).cpu()
    return inv_spectrogram_batch(lin, cfg, init_phasor, fl * int(upsample))


def inv_melspectrogram(mel, cfg=None, device="cuda:0", options=None):
    """The numpy sibling of inv_spectrogram for a mel: (num_mels, T) normalised numpy -> waveform numpy."""
    m = torch.as_tensor(np.ascontiguousarray(np.asarray(mel, dtype=np.float32).T)).unsqueeze(0)
    y = inv_melspectrogram_batch(m.to(device), cfg, options=options)
    return y[0].cpu().numpy()


def _check_lws(cfg, what):
    if cfg.convention != "lws":
        raise ValueError("%s: only the lws framing (the reference's features) is supported; the torch framing has no "
                         "ragged rule for its reflect padding" % what)


def item_gains(wav_flat, lengths, rescaling_max, device_offsets=None):
    """hparams.rescaling (ljspeech.py:59-60) per item: device float32[B], gain[b] = rescaling_max / max|x_b| in fp32
    (1 for a silent item).  The host formula: np.float32(rescaling_max) / np.abs(x_b).max()."""
    wav_flat = _c(_chk(wav_flat, "wav_flat"))
    soff = device_offsets if device_offsets is not None else _sample_offsets(lengths, wav_flat.device)
    B = len(lengths)
    gain = torch.empty(B, dtype=torch.float32, device=wav_flat.device)
    _lib.call("dv3_item_gain_f32", wav_flat.data_ptr(), soff.data_ptr(), B, float(rescaling_max), gain.data_ptr(),
              _stream())
    return gain


def _sample_offsets(lengths, device):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(device, non_blocking=True)


def features_items(wav_flat, lengths, cfg=None, num_mels=80, fmin=125, fmax=7600, rescaling=None):
    """Linear and mel features of B utterances packed back to back in `wav_flat` (a 1-D float32 device tensor; item b
    is the next lengths[b] samples) -> (lin (sum T_b, fft_size // 2 + 1), mel (sum T_b, num_mels), frames int64[B] on the
    host), T_b = lws_num_frames(lengths[b], hop, fft_size): the rows of PackedBatch.lin / .mel (data.py), item b's at
    frames[:b].sum() ... frames[:b + 1].sum().  Each row depends on its own item only: the linear rows are bit for bit
    spectrogram_batch(item[None])[0].T, and the mel rows are a fixed-order sum (see include/dv3hip.h:
    dv3_analysis_items_f32).  rescaling: None / False, or rescaling_max (hparams.rescaling_max) -- item b is analysed
    as x_b * item_gains(...)[b]."""
    cfg = cfg or AudioConfig()
    _check_lws(cfg, "features_items")
    wav_flat = _c(_chk(wav_flat, "wav_flat"))
    if wav_flat.dim() != 1:
        raise ValueError("features_items: wav_flat must be 1-D (the items back to back)")
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    B = lengths.size
    if B == 0 or int(lengths.min()) < 1 or int(lengths.sum()) != wav_flat.numel():
        raise ValueError("features_items: %d samples do not split into items of lengths %s (each >= 1)"
                         % (wav_flat.numel(), lengths.tolist()))
    hop, n_fft = cfg.hop_size, cfg.fft_size
    frames = np.array([lws_num_frames(int(n), hop, n_fft) for n in lengths], dtype=np.int64)
    nf = int(frames.sum())
    if nf >= 2 ** 31 or int(lengths.max()) >= 2 ** 31 - n_fft:
        raise ValueError("features_items: batch too large for one launch (%d frames)" % nf)
    dev = wav_flat.device
    soff = _sample_offsets(lengths, dev)
    foff = torch.from_numpy(np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)).to(dev, non_blocking=True)
    awin, _ = lws_windows(dev, hop, cfg.window_scale, n_fft)
    basis, band = mel_tables(dev, cfg.sample_rate, num_mels, fmin, fmax, n_fft)
    gain = item_gains(wav_flat, lengths, rescaling, soff) if rescaling else None
    lin = torch.empty((nf, n_fft // 2 + 1), dtype=torch.float32, device=dev)
    mel = torch.empty((nf, num_mels), dtype=torch.float32, device=dev)
    _lib.call("dv3_analysis_items_f32_n", wav_flat.data_ptr(), soff.data_ptr(), foff.data_ptr(), B, nf, hop,
              float(cfg.preemphasis), awin.data_ptr(), gain.data_ptr() if gain is not None else None, basis.data_ptr(),
              band.data_ptr(), num_mels, float(cfg.min_level_db), float(cfg.ref_level_db), lin.data_ptr(),
              mel.data_ptr(), n_fft, _stream())
    return lin, mel, frames


def pack_waveforms(wavs, pin=None):
    """[1-D float arrays] -> (one flat float32 host tensor, pinned when CUDA is present; lengths int64[B])"""
    lengths = np.array([len(w) for w in wavs], dtype=np.int64)
    if pin is None:
        pin = torch.cuda.is_available()
    flat = torch.empty(int(lengths.sum()), dtype=torch.float32, pin_memory=bool(pin))
    fv = flat.numpy()
    o = 0
    for w, n in zip(wavs, lengths):
        fv[o:o + n] = w
        o += n
    return flat, lengths


def features_from_arrays(wavs, cfg=None, device="cuda:0", **kw):
    """features_items for a list of 1-D host waveforms: one pinned staging buffer, one host-to-device copy."""
    flat, lengths = pack_waveforms(wavs)
    return features_items(flat.to(device, non_blocking=True), lengths, cfg, **kw)


# ---------------------------------------------------------------------------------------------
# pitch tracking: YIN per frame of the packed waveforms (csrc/pitch.hip; include/dv3hip.h: dv3_yin_items_f32)
# ---------------------------------------------------------------------------------------------
class PitchConfig(object):
    """Options of the pitch tracker (yin_items): fmin, fmax in Hz bound the search -- lags tau_min = max(2,
    floor(sample_rate / fmax)) up to tau_max = floor(sample_rate / fmin) -- and fmin=None means max(60.0, 2 * sample_rate
    / fft_size) of the audio config, the lowest pitch whose period fits the kernel's limit tau_max <= fft_size / 2;
    threshold in (0, 1]: YIN's absolute threshold on the normalised difference (0.1 - 0.15 in the paper); silence_db:
    frames whose mean square is at or below 10 ** (silence_db / 10) count as unvoiced (voiced()).  Refused by value."""

    def __init__(self, fmin=None, fmax=500.0, threshold=0.15, silence_db=-60.0):
        number = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and \
            np.isfinite(float(v))
        if fmin is not None and not (number(fmin) and float(fmin) > 0.0):
            raise ValueError("PitchConfig: fmin=%r must be None or a positive number of Hz" % (fmin,))
        if not (number(fmax) and float(fmax) > 0.0) or (fmin is not None and not float(fmin) < float(fmax)):
            raise ValueError("PitchConfig: fmax=%r must be a positive number of Hz above fmin=%r" % (fmax, fmin))
        if not (number(threshold) and 0.0 < float(threshold) <= 1.0):
            raise ValueError("PitchConfig: threshold=%r must lie in (0, 1]" % (threshold,))
        if not number(silence_db):
            raise ValueError("PitchConfig: silence_db=%r must be a finite number of dB" % (silence_db,))
        self.fmin = None if fmin is None else float(fmin)
        self.fmax, self.threshold, self.silence_db = float(fmax), float(threshold), float(silence_db)

    def resolved_fmin(self, cfg=None):
        cfg = cfg or AudioConfig()
        return self.fmin if self.fmin is not None else max(60.0, 2.0 * float(cfg.sample_rate) / cfg.fft_size)

    def lags(self, cfg=None):
        """-> (tau_min, tau_max) at cfg's sample rate and frame size; ValueError for a pair the kernel refuses"""
        cfg = cfg or AudioConfig()
        sr, n_fft, fmin = float(cfg.sample_rate), int(cfg.fft_size), self.resolved_fmin(cfg)
        tau_min, tau_max = max(2, int(sr // self.fmax)), int(sr // fmin)
        if tau_max > n_fft // 2 or tau_min + 1 >= tau_max:
            raise ValueError("PitchConfig: fmin=%g Hz at sample_rate=%g and fft_size=%d searches lags [%d, %d): the longest "
                             "must not exceed fft_size / 2 = %d (fmin >= %g Hz) and the range must hold two lags (fmax=%g)"
                             % (fmin, sr, n_fft, tau_min, tau_max, n_fft // 2, 2.0 * sr / n_fft, self.fmax))
        return tau_min, tau_max


def yin_items(wav_flat, lengths, cfg=None, pitch=None, want_lag=False):
    """YIN pitch estimates for every frame of B utterances packed back to back in `wav_flat` (packed exactly as
    features_items takes them: a 1-D float32 device tensor, item b the next lengths[b] samples) -> (f0 (sum T_b,) in Hz,
    ap (sum T_b,), power (sum T_b,), frames int64[B] on the host), and with want_lag a fifth element, the chosen lag
    (sum T_b,) int32: (f0, ap, power, frames, lag).  Row t of item b describes the samples of that item's
    features_items row t (the lws framing, no pre-emphasis, no window).  ap is the normalised difference d' at the
    chosen lag (small = periodic), power the frame's mean square; an estimate is given for every frame and voiced(ap,
    power, pitch) decides which to believe.  include/dv3hip.h (dv3_yin_items_f32) states every step and the bounds."""
    cfg = cfg or AudioConfig()
    pitch = pitch if pitch is not None else PitchConfig()
    if not isinstance(pitch, PitchConfig):
        raise ValueError("yin_items: pitch must be a PitchConfig, got %r" % (pitch,))
    _check_lws(cfg, "yin_items")
    tau_min, tau_max = pitch.lags(cfg)
    wav_flat = _c(_chk(wav_flat, "wav_flat"))
    if wav_flat.dim() != 1:
        raise ValueError("yin_items: wav_flat must be 1-D (the items back to back)")
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    B = lengths.size
    if B == 0 or int(lengths.min()) < 1 or int(lengths.sum()) != wav_flat.numel():
        raise ValueError("yin_items: %d samples do not split into items of lengths %s (each >= 1)"
                         % (wav_flat.numel(), lengths.tolist()))
    hop, n_fft = cfg.hop_size, cfg.fft_size
    frames = np.array([lws_num_frames(int(n), hop, n_fft) for n in lengths], dtype=np.int64)
    nf = int(frames.sum())
    if nf >= 2 ** 31 or int(lengths.max()) >= 2 ** 31 - n_fft:
        raise ValueError("yin_items: batch too large for one launch (%d frames)" % nf)
    dev = wav_flat.device
    soff = _sample_offsets(lengths, dev)
    foff = torch.from_numpy(np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)).to(dev, non_blocking=True)
    f0, ap, power = (torch.empty(nf, dtype=torch.float32, device=dev) for _ in range(3))
    lag = torch.empty(nf, dtype=torch.int32, device=dev) if want_lag else None
    _lib.call("dv3_yin_items_f32", wav_flat.data_ptr(), soff.data_ptr(), foff.data_ptr(), B, nf, hop, n_fft, tau_min,
              tau_max, pitch.threshold, float(cfg.sample_rate), f0.data_ptr(), ap.data_ptr(), power.data_ptr(),
              lag.data_ptr() if lag is not None else None, _stream())
    return (f0, ap, power, frames, lag) if want_lag else (f0, ap, power, frames)


def f0_from_arrays(wavs, cfg=None, device="cuda:0", pitch=None):
    """yin_items for a list of 1-D host waveforms: one pinned staging buffer, one host-to-device copy."""
    flat, lengths = pack_waveforms(wavs)
    return yin_items(flat.to(device, non_blocking=True), lengths, cfg, pitch)


def voiced(ap, power, pitch):
    """-> bool tensor: (ap < pitch.threshold) & (power > 10 ** (pitch.silence_db / 10)); any device, no kernel"""
    return (ap < pitch.threshold) & (power > 10.0 ** (pitch.silence_db / 10.0))


# ---------------------------------------------------------------------------------------------
# waveform preparation for multi-speaker corpora (ABI 46): librosa.load(sr=...) (audio.py:12-13) and
# librosa.effects.trim (vctk.py:52-67) as ragged launches, in front of features_items
# ---------------------------------------------------------------------------------------------
RESAMPLE_ZEROS = 64                        # the published design of resampy's "kaiser_best" filter
RESAMPLE_ROLLOFF = 0.9475937167399596
RESAMPLE_BETA = 14.769656459379492
TRIM_FRAME, TRIM_HOP = 2048, 512           # librosa.effects.trim's defaults


def resample_ratio(source_rate, target_rate):
    """-> (up, down) in lowest terms with target = source * up / down (48000 -> 22050: 147 / 320)"""
    import math
    source_rate, target_rate = int(source_rate), int(target_rate)
    if source_rate < 1 or target_rate < 1:
        raise ValueError("resample_ratio: rates must be positive integers")
    g = math.gcd(source_rate, target_rate)
    return target_rate // g, source_rate // g


def resample_half_width(up, down):
    """H: taps reach H samples below and H + 1 above floor(position): ceil(64 / min(1, up / down))"""
    return RESAMPLE_ZEROS if up >= down else -(-RESAMPLE_ZEROS * down // up)


def resample_table_np(up, down):
    """float64 [2H + 2][up]: table[j][r] = h(H - j + ((r down) mod up) / up) of include/dv3hip.h
    (dv3_resample_items_f32): the windowed sinc, evaluated in closed form"""
    s = min(1.0, up / down)
    H = resample_half_width(up, down)
    frac = ((np.arange(up, dtype=np.int64) * down) % up).astype(np.float64) / up
    t = (H - np.arange(2 * H + 2, dtype=np.float64))[:, None] + frac[None, :]
    u = np.abs(t) * s / RESAMPLE_ZEROS
    w = np.where(u < 1.0, np.i0(RESAMPLE_BETA * np.sqrt(np.clip(1.0 - u * u, 0.0, 1.0))) / np.i0(RESAMPLE_BETA), 0.0)
    return s * RESAMPLE_ROLLOFF * np.sinc(RESAMPLE_ROLLOFF * s * t) * w


_RESAMPLE_CACHE = {}


def resample_table(device, up, down):
    """the coefficient table as a float32 device tensor (computed in fp64, rounded once; cached per device and ratio)"""
    key = (str(device), int(up), int(down))
    if key not in _RESAMPLE_CACHE:
        _RESAMPLE_CACHE[key] = torch.from_numpy(resample_table_np(up, down).astype(np.float32)).to(device)
    return _RESAMPLE_CACHE[key]


def _item_lengths(lengths, total, what):
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.size == 0 or int(lengths.min()) < 0 or int(lengths.sum()) != total:
        raise ValueError("%s: %d samples do not split into items of lengths %s" % (what, total, lengths.tolist()))
    return lengths


def resample_items(wav_flat, lengths, up, down):
    """Band-limited resampling of B utterances packed back to back (item b = the next lengths[b] samples of the 1-D
    float32 device tensor) by up / down -> (flat, lengths): item b becomes ceil(lengths[b] * up / down) samples, the
    length librosa.resample gives.  The filter is resampy's kaiser_best design in closed form (include/dv3hip.h:
    dv3_resample_items_f32 states it and its roundings); each output is a function of its own item only.  up == down
    returns the input without a launch (the filter itself is NOT the identity at ratio 1: its roll-off low-passes)."""
    import math
    wav_flat = _c(_chk(wav_flat, "wav_flat"))
    if wav_flat.dim() != 1:
        raise ValueError("resample_items: wav_flat must be 1-D (the items back to back)")
    lengths = _item_lengths(lengths, wav_flat.numel(), "resample_items")
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError("resample_items: up and down must be positive")
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if up == down:
        return wav_flat, lengths
    tile = _lib.lib().dv3_resample_tile(up, down)
    if tile <= 0:
        raise ValueError("resample_items: the ratio %d / %d is not supported (terms up to 4096, a bounded window)"
                         % (up, down))
    out_len = -(-lengths * up // down)
    tiles = -(-out_len // tile)
    if int(tiles.sum()) >= 2 ** 31:
        raise ValueError("resample_items: batch too large for one launch")
    dev = wav_flat.device
    y = torch.empty(int(out_len.sum()), dtype=torch.float32, device=dev)
    if int(tiles.sum()) == 0:
        return y, out_len
    ioff = _sample_offsets(lengths, dev)
    ooff = _sample_offsets(out_len, dev)
    toff = torch.from_numpy(np.concatenate([[0], np.cumsum(tiles)]).astype(np.int32)).to(dev, non_blocking=True)
    table = resample_table(dev, up, down)
    _lib.call("dv3_resample_items_f32", wav_flat.data_ptr(), ioff.data_ptr(), ooff.data_ptr(), toff.data_ptr(),
              lengths.size, int(tiles.sum()), up, down, table.data_ptr(), y.data_ptr(), _stream())
    return y, out_len


def trim_num_frames(length):
    """frames librosa.effects.trim looks at: 1 + length // 512; 0 for a span too short to reflect-pad (< 1025)"""
    return 1 + int(length) // TRIM_HOP if length > TRIM_FRAME // 2 else 0


def _spans(wav_flat, starts, lengths, what):
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if starts.size == 0 or starts.size != lengths.size or int(lengths.min()) < 0 or int(starts.min()) < 0 or \
            int((starts + lengths).max()) > wav_flat.numel():
        raise ValueError("%s: spans must lie inside the %d samples of wav_flat" % (what, wav_flat.numel()))
    return starts, lengths


def trim_items(wav_flat, starts, lengths, top_db=15.0):
    """librosa.effects.trim(y, top_db) at its defaults for B spans of a flat float32 device tensor: span b =
    wav_flat[starts[b] : starts[b] + lengths[b]] (host integers -- the frame counts size the launch).  top_db: one number
    or one per span.  -> (starts, lengths) of the trimmed spans as int64 DEVICE tensors, starts absolute in wav_flat.
    A span shorter than 1025 samples can not be reflect-padded and is returned unchanged.  See include/dv3hip.h
    (dv3_trim_items_f32) for the definition."""
    wav_flat = _c(_chk(wav_flat, "wav_flat"))
    starts, lengths = _spans(wav_flat, starts, lengths, "trim_items")
    B = starts.size
    top = np.broadcast_to(np.asarray(top_db, dtype=np.float32), (B,)).copy()
    frames = np.array([trim_num_frames(n) for n in lengths], dtype=np.int64)
    nf = int(frames.sum())
    if nf >= 2 ** 31:
        raise ValueError("trim_items: batch too large for one launch")
    dev = wav_flat.device
    # one upload: starts | lengths as int64, then the frame offsets and the thresholds
    sl = torch.from_numpy(np.concatenate([starts, lengths])).to(dev, non_blocking=True)
    foff = torch.from_numpy(np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)).to(dev, non_blocking=True)
    top_d = torch.from_numpy(top).to(dev, non_blocking=True)
    mse = torch.empty(max(nf, 1), dtype=torch.float32, device=dev)
    out = torch.empty((2, B), dtype=torch.int64, device=dev)
    _lib.call("dv3_trim_items_f32", wav_flat.data_ptr(), sl[:B].data_ptr(), sl[B:].data_ptr(), foff.data_ptr(), B, nf,
              top_d.data_ptr(), mse.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), _stream())
    return out[0], out[1]


def gather_spans(wav_flat, starts, lengths):
    """the spans wav_flat[starts[b] : starts[b] + lengths[b]] copied back to back -> (flat, lengths int64[B] on the
    host).  starts / lengths: int64 device tensors (trim_items' result) or host integers.  The lengths are read back to
    the host here when they live on the device (they size the output)."""
    wav_flat = _c(_chk(wav_flat, "wav_flat"))
    dev = wav_flat.device
    if torch.is_tensor(starts) and torch.is_tensor(lengths) and starts.is_cuda:
        host = torch.stack([starts.to(torch.int64), lengths.to(torch.int64)]).cpu().numpy()       # the one host read
        starts_h, lengths_h = _spans(wav_flat, host[0], host[1], "gather_spans")
        starts_d, lengths_d = _c(starts.to(torch.int64)), _c(lengths.to(torch.int64))
    else:
        starts_h, lengths_h = _spans(wav_flat, starts, lengths, "gather_spans")
        sl = torch.from_numpy(np.concatenate([starts_h, lengths_h])).to(dev, non_blocking=True)
        starts_d, lengths_d = sl[:starts_h.size], sl[starts_h.size:]
    B = starts_h.size
    if B > 65535:
        raise ValueError("gather_spans: at most 65535 spans per call")
    y = torch.empty(int(lengths_h.sum()), dtype=torch.float32, device=dev)
    if y.numel():
        ooff = _sample_offsets(lengths_h, dev)
        _lib.call("dv3_gather_spans_f32", wav_flat.data_ptr(), starts_d.data_ptr(), lengths_d.data_ptr(),
                  ooff.data_ptr(), B, int(lengths_h.max()), y.data_ptr(), _stream())
    return y, lengths_h.copy()


def prepare_items(wavs, source_rate, cfg=None, spans=None, top_db=15.0, device="cuda:0"):
    """The reference's multi-speaker waveform preparation (vctk.py:52-67 after audio.load_wav) for a list of 1-D host
    waveforms recorded at source_rate: resample to cfg.sample_rate, cut item b to spans[b] = (begin, end) in resampled
    samples where given (None / no entry: the whole item; the HTS label cut), trim silence at top_db (a number or one
    per item), and pack the results back to back -> (wav_flat on `device`, lengths int64[B] on the host), what
    features_items takes.  An item trimmed to nothing has length 0 (features_items wants those dropped from `lengths`;
    they occupy no samples).  One host-to-device copy, one host read (the trimmed spans: the frame counts size the
    feature buffers)."""
    cfg = cfg or AudioConfig()
    flat, lengths = pack_waveforms(wavs)
    up, down = resample_ratio(source_rate, cfg.sample_rate)
    res, rlen = resample_items(flat.to(device, non_blocking=True), lengths, up, down)
    starts = np.concatenate([[0], np.cumsum(rlen)[:-1]]).astype(np.int64)
    lens = rlen.copy()
    if spans is not None:
        if len(spans) != len(wavs):
            raise ValueError("prepare_items: one span (or None) per waveform expected")
        for b, sp in enumerate(spans):
            if sp is None:
                continue
            lo = min(max(int(sp[0]), 0), int(rlen[b]))
            hi = min(max(int(sp[1]), lo), int(rlen[b]))
            starts[b] += lo
            lens[b] = hi - lo
    t_starts, t_lens = trim_items(res, starts, lens, top_db)
    return gather_spans(res, t_starts, t_lens)


# ---------------------------------------------------------------------------------------------
# deliverable audio: levels, gains, and one launch that places, scales, fades and quantises (csrc/master.hip)
# ---------------------------------------------------------------------------------------------
LEVEL_COLUMNS = ("peak", "sumsq", "sum", "over", "nonfinite")      # the columns of a level row (dv3_wave_levels_f32)
_MASTER_MODES = {"float32": "DV3_MASTER_F32", "int16": "DV3_MASTER_I16"}
_GAIN_POLICIES = {"peak": "DV3_GAIN_PEAK", "rms": "DV3_GAIN_RMS", "reference": "DV3_GAIN_REFERENCE"}


def _span_tables(wav_flat, starts, lengths, max_len, what):
    """host integers or int64 device tensors -> (starts_d, lengths_d, B, max_len): device tensors need max_len, a bound
    on every length (the kernel clamps at it), because nothing is read back here"""
    dev = wav_flat.device
    if torch.is_tensor(starts) and torch.is_tensor(lengths) and starts.is_cuda and lengths.is_cuda:
        if max_len is None:
            raise ValueError("%s: spans on the device need max_len= (a bound on the lengths; nothing is read back)" % what)
        return _c(starts.to(torch.int64)), _c(lengths.to(torch.int64)), int(starts.numel()), int(max_len)
    starts_h, lengths_h = _spans(wav_flat, starts, lengths, what)
    sl = torch.from_numpy(np.concatenate([starts_h, lengths_h])).to(dev, non_blocking=True)
    return sl[:starts_h.size], sl[starts_h.size:], int(starts_h.size), int(lengths_h.max())


def wave_levels(wav_flat, starts, lengths, max_len=None):
    """The level of B spans of a flat float32 device tensor, span b = wav_flat[starts[b] : starts[b] + lengths[b]] (host
    integers, or int64 device tensors together with max_len=, a bound on the lengths) -> float64 (B, 5) on the device,
    columns LEVEL_COLUMNS: peak = max |x| and sumsq, sum over the finite samples (fp64 accumulation in a fixed order),
    over = samples with |x| >= 1, nonfinite = NaN or infinite samples.  A padded (B, L) batch is B spans at b * L of its
    flattened view, nothing repacked.  Row b is a function of item b's samples alone (include/dv3hip.h:
    dv3_wave_levels_f32).  No host read."""
    wav_flat = _c(_chk(wav_flat, "wav_flat")).reshape(-1)
    starts_d, lengths_d, B, max_len = _span_tables(wav_flat, starts, lengths, max_len, "wave_levels")
    if not 1 <= B <= 65535:
        raise ValueError("wave_levels: %d spans, at most 65535 per call" % B)
    dev = wav_flat.device
    nchunk = -(-max_len // _lib.CONSTS["DV3_LEVELS_CHUNK"])
    scratch = torch.empty(max(B * nchunk * len(LEVEL_COLUMNS), 1), dtype=torch.float64, device=dev)
    levels = torch.empty((B, len(LEVEL_COLUMNS)), dtype=torch.float64, device=dev)
    _lib.call("dv3_wave_levels_f32", wav_flat.data_ptr(), starts_d.data_ptr(), lengths_d.data_ptr(), B, max_len,
              scratch.data_ptr(), levels.data_ptr(), _stream())
    return levels


def _db(v, what, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not lo <= float(v) <= hi:
        raise ValueError("Mastering: %s=%r must be a number in [%g, %g]" % (what, v, lo, hi))
    return float(v)


class Limiter(object):
    """A look-ahead peak limiter for Mastering(limiter=) (limit_spans; csrc/limiter.hip): the gain is
    turned down lookahead_ms before a peak that would pass the ceiling, over a box of that length, held while the peak
    lasts, and released exponentially with the time constant release_ms; passes: how often the loudness target is
    re-aimed from the limited result (1 .. 4; more than one needs level="lufs").  lookahead_ms >= 0, release_ms > 0.
    The defaults are starting points, not measurements: nothing here was heard on a trained voice.
    Refused by value (ValueError naming it)."""

    def __init__(self, lookahead_ms=1.5, release_ms=50.0, passes=1):
        num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and \
            np.isfinite(float(v))
        if not num(lookahead_ms) or float(lookahead_ms) < 0.0:
            raise ValueError("Limiter: lookahead_ms=%r must be a finite number >= 0" % (lookahead_ms,))
        if not num(release_ms) or float(release_ms) <= 0.0:
            raise ValueError("Limiter: release_ms=%r must be a finite number > 0" % (release_ms,))
        if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or not 1 <= int(passes) <= 4:
            raise ValueError("Limiter: passes=%r must be an integer in [1, 4]" % (passes,))
        self.lookahead_ms, self.release_ms, self.passes = float(lookahead_ms), float(release_ms), int(passes)

    def lookahead(self, sample_rate):
        """A = floor(lookahead_ms * sample_rate / 1000 + 0.5) samples; ValueError above DV3_LIMIT_MAX_LOOKAHEAD"""
        A = int(np.floor(self.lookahead_ms * float(sample_rate) / 1000.0 + 0.5))
        if A > _lib.CONSTS["DV3_LIMIT_MAX_LOOKAHEAD"]:
            raise ValueError("Limiter: lookahead_ms=%r is %d samples at %r Hz, at most %d" % (
                self.lookahead_ms, A, sample_rate, _lib.CONSTS["DV3_LIMIT_MAX_LOOKAHEAD"]))
        return A

    def rho(self, sample_rate):
        """the release factor per sample, exp(-1000 / (release_ms * sample_rate))"""
        return float(np.exp(-1000.0 / (self.release_ms * float(sample_rate))))


class Mastering(object):
    """How synthesised waveforms become deliverable audio (master_items, synthesis.join_utterances).
    level: None (gain 1), "peak" (the largest |x| goes to target_db dBFS), "rms" (the RMS goes to target_db dBFS, but
    no peak above ceiling_db), "lufs" (the BS.1770 integrated loudness goes to target_db LUFS, but no peak above
    ceiling_db; true_peak=True makes that a dBTP ceiling on the 4x oversampled true peak; it needs a sample rate:
    wave_loudness) or "reference" (the reference's save_wav, audio.py:16-18: x * 32767 / max(0.01, peak)
    truncated to int16 -- it takes dtype "int16", no dither and no fades); scope: "item" (every utterance its own gain)
    or "document" (one gain from the combined levels of all of them; under "lufs" the items' blocks are pooled, the
    standard's integrated loudness of the whole programme); target_db: default -1 for "peak", -20 for "rms", -23 for
    "lufs" (EBU R 128); max_gain_db caps the gain of "peak", "rms" and "lufs" (a near-silent item is not blown up); fade_ms: the raised-cosine fade
    at a document's joins and edges (join_utterances; master_items fades nothing); dither, seed: TPDF dither of +-1 LSB
    before the int16 rounding, a function of (seed, sample index); dtype: "int16" or "float32".
    limiter: None, or a Limiter -- with level None, "rms" or "lufs" the static gain no longer gives way to
    the ceiling (it is min(target gain, max_gain), or 1): a look-ahead limiter holds every utterance under ceiling_db
    instead, with the sample-peak or, under true_peak=True, the true-peak detector; "peak" (its target is itself a
    peak) and "reference" take none, and Limiter(passes > 1) re-aims a loudness target, so it needs "lufs".
    The defaults are starting points, not measurements: nothing here was heard on a trained voice.
    Refused by value (ValueError naming it)."""

    def __init__(self, level=None, scope="item", target_db=None, ceiling_db=-1.0, max_gain_db=30.0, fade_ms=5.0,
                 dither=False, seed=0, dtype="int16", true_peak=False, limiter=None):
        if level is not None and level != "lufs" and level not in _GAIN_POLICIES:
            raise ValueError("Mastering: level=%r must be None, 'peak', 'rms', 'lufs' or 'reference'" % (level,))
        if not isinstance(true_peak, (bool, np.bool_)):
            raise ValueError("Mastering: true_peak=%r must be True or False" % (true_peak,))
        if true_peak and level != "lufs":
            raise ValueError("Mastering: true_peak=True needs level='lufs' (the other levels' ceiling is a sample peak)")
        if scope not in ("item", "document"):
            raise ValueError("Mastering: scope=%r must be 'item' or 'document'" % (scope,))
        if dtype not in _MASTER_MODES:
            raise ValueError("Mastering: dtype=%r must be 'int16' or 'float32'" % (dtype,))
        if not isinstance(dither, (bool, np.bool_)):
            raise ValueError("Mastering: dither=%r must be True or False" % (dither,))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError("Mastering: seed=%r must be an integer in [0, 2^64)" % (seed,))
        if target_db is None:
            target_db = {"rms": -20.0, "lufs": -23.0}.get(level, -1.0)
        self.level, self.scope, self.dtype, self.true_peak = level, scope, dtype, bool(true_peak)
        self.target_db = _db(target_db, "target_db", -120.0, 0.0)
        self.ceiling_db = _db(ceiling_db, "ceiling_db", -120.0, 0.0)
        self.max_gain_db = _db(max_gain_db, "max_gain_db", 0.0, 120.0)
        self.fade_ms = _db(fade_ms, "fade_ms", 0.0, 1000.0)
        self.dither, self.seed = bool(dither), int(seed)
        if self.dither and dtype != "int16":
            raise ValueError("Mastering: dither=True needs dtype='int16'")
        if level == "reference" and (dtype != "int16" or self.dither):
            raise ValueError("Mastering: level='reference' is the reference's save_wav: dtype='int16' and no dither")
        if limiter is not None:
            if not isinstance(limiter, Limiter):
                raise ValueError("Mastering: limiter=%r must be None or an audio.Limiter" % (limiter,))
            if level in ("peak", "reference"):
                raise ValueError("Mastering: limiter= goes with level None, 'rms' or 'lufs', not %r (a peak target leaves "
                                 "a limiter nothing to hold; 'reference' is the reference's save_wav)" % (level,))
            if limiter.passes > 1 and level != "lufs":
                raise ValueError("Mastering: Limiter(passes=%d) re-aims a loudness target: it needs level='lufs'"
                                 % limiter.passes)
        self.limiter = limiter

    def mode(self):
        """the DV3_MASTER_* output mode"""
        return _lib.CONSTS["DV3_MASTER_I16_REFERENCE" if self.level == "reference" else _MASTER_MODES[self.dtype]]

    def fade_samples(self, sample_rate):
        """F = round(fade_ms * sample_rate / 1000) (halves up), 0 under the "reference" level; ValueError above
        DV3_MASTER_MAX_FADE"""
        if self.level == "reference":
            return 0
        F = int(np.floor(self.fade_ms * float(sample_rate) / 1000.0 + 0.5))
        if F > _lib.CONSTS["DV3_MASTER_MAX_FADE"]:
            raise ValueError("Mastering: fade_ms=%r is %d samples at %r Hz, at most %d" % (
                self.fade_ms, F, sample_rate, _lib.CONSTS["DV3_MASTER_MAX_FADE"]))
        return F


def check_mastering(mastering, what):
    """the `mastering=` keyword -> None or the Mastering; anything else is refused"""
    if mastering is not None and not isinstance(mastering, Mastering):
        raise ValueError("%s: mastering must be an audio.Mastering, got %r" % (what, mastering))
    return mastering


_NO_CEILING = 1e30      # a finite linear ceiling that cannot bind: the gain entries refuse an infinite one


def wave_gains(levels, lengths, mastering, groups=None, ceiling=None):
    """Levels -> the per-item values the master launch takes, float32 (B,) on the device: levels (B, 5) from wave_levels,
    lengths int64 (B,) on the device, mastering.level the policy ("peak", "rms": a multiplier; "reference": the divisor
    max(0.01, peak)), groups: None (mastering.scope decides: every item alone, or all of them one group) or the group
    offsets, ascending host ints from 0 to B.  ceiling: None (mastering.ceiling_db) or a LINEAR ceiling in its place (a
    limiter's pre-gain takes one that cannot bind).  fp64 on the device, rounded once (include/dv3hip.h:
    dv3_wave_gains_f32)."""
    if mastering.level is None:
        raise ValueError("wave_gains: mastering.level is None (the gain is 1: nothing to compute)")
    if mastering.level == "lufs":
        raise ValueError("wave_gains: level='lufs' is measured by wave_loudness and turned into gains by loudness_gains")
    B = int(levels.shape[0])
    if tuple(levels.shape) != (B, len(LEVEL_COLUMNS)) or levels.dtype != torch.float64 or not levels.is_cuda:
        raise ValueError("wave_gains: levels must be wave_levels' float64 (B, 5) device table")
    if lengths.numel() != B or lengths.dtype != torch.int64 or not lengths.is_cuda:
        raise ValueError("wave_gains: lengths must be an int64 device tensor of %d items" % B)
    if groups is None:
        groups = list(range(B + 1)) if mastering.scope == "item" else [0, B]
    goff = np.asarray(groups, dtype=np.int64).reshape(-1)
    if goff.size < 2 or goff[0] != 0 or goff[-1] != B or np.any(np.diff(goff) < 0):
        raise ValueError("wave_gains: groups must ascend from 0 to %d, got %s" % (B, goff.tolist()))
    dev = levels.device
    goff_d = torch.from_numpy(goff.astype(np.int32)).to(dev, non_blocking=True)
    gain = torch.empty(B, dtype=torch.float32, device=dev)
    lin = lambda db: 10.0 ** (db / 20.0)
    _lib.call("dv3_wave_gains_f32", _c(levels).data_ptr(), _c(lengths).data_ptr(), goff_d.data_ptr(), B, goff.size - 1,
              _lib.CONSTS[_GAIN_POLICIES[mastering.level]], lin(mastering.target_db),
              lin(mastering.ceiling_db) if ceiling is None else float(ceiling), lin(mastering.max_gain_db), gain.data_ptr(),
              _stream())
    return gain


# ---- loudness: BS.1770 integrated loudness and true peak (csrc/loudness.hip) --------------------------
LOUDNESS_COLUMNS = ("lufs", "blocks", "gated_abs", "gated_rel", "momentary_max", "true_peak", "flags")
_K_SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416)     # f0, G dB, Q, Vb exponent
_K_HIGHPASS = (38.13547087602444, 0.5003270373238773)                                        # f0, Q
_KW_CACHE = {}
_TP_CACHE = []


def loudness_step(sample_rate):
    """h = floor(0.1 fs + 0.5): the step of the gating blocks (a block is 4 h samples); ValueError outside 8000 .. 192000"""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, float, np.integer, np.floating)) or \
            not 8000 <= float(sample_rate) <= 192000:
        raise ValueError("loudness: sample_rate=%r must be a number in [8000, 192000]" % (sample_rate,))
    return int(np.floor(0.1 * float(sample_rate) + 0.5))


def k_weighting(sample_rate):
    """The K-weighting of BS.1770 at `sample_rate`, in float64 by the bilinear transform of the analogue prototypes
    (include/dv3hip.h states the formulas) -> {"shelf": (b, a), "highpass": (b, a), "coef": the 10 doubles
    dv3_wave_loudness_f64 takes, "A": the 4x4 zero-input transition of the cascade's state, "h": the step, "Ah": A^h}"""
    h = loudness_step(sample_rate)
    key = float(sample_rate)
    if key in _KW_CACHE:
        return _KW_CACHE[key]
    f0, G, Q, e = _K_SHELF
    K = np.tan(np.pi * f0 / key)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** e
    a0 = 1.0 + K / Q + K * K
    sb = np.array([Vh + Vb * K / Q + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Q + K * K], dtype=np.float64) / a0
    sa = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)
    f0, Q = _K_HIGHPASS
    K = np.tan(np.pi * f0 / key)
    a0 = 1.0 + K / Q + K * K
    pb = np.array([1.0, -2.0, 1.0], dtype=np.float64)
    pa = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)
    A = np.array([[-sa[1], 1.0, 0.0, 0.0],
                  [-sa[2], 0.0, 0.0, 0.0],
                  [pb[1] - pa[1] * pb[0], 0.0, -pa[1], 1.0],
                  [pb[2] - pa[2] * pb[0], 0.0, -pa[2], 0.0]], dtype=np.float64)
    out = {"shelf": (sb, sa), "highpass": (pb, pa), "coef": np.concatenate([sb, sa[1:], pb, pa[1:]]), "A": A, "h": h,
           "Ah": np.ascontiguousarray(np.linalg.matrix_power(A, h))}
    _KW_CACHE[key] = out
    return out


def true_peak_table():
    """The 4x interpolator of the true-peak estimate: g[i] = sinc(i / 4) kaiser(49, beta=8)[i + 24], i = -24 .. 24, in
    float64, cut into its phases 1 .. 3 of 12 taps (phase 0 is the identity) and rounded once -> float32 (3, 12),
    table[p - 1][j] = g[p + 4 (j - 6)], the tap of x[m + 6 - j] in y[4 m + p]"""
    if not _TP_CACHE:
        i = np.arange(-24, 25, dtype=np.float64)
        g = np.sinc(i / 4.0) * np.kaiser(49, 8.0)
        _TP_CACHE.append(np.array([[g[24 + p + 4 * (j - 6)] for j in range(12)] for p in (1, 2, 3)]).astype(np.float32))
    return _TP_CACHE[0].copy()


def _group_offsets(groups, B, what):
    goff = np.asarray(groups, dtype=np.int64).reshape(-1)
    if goff.size < 2 or goff[0] != 0 or goff[-1] != B or np.any(np.diff(goff) < 0) or goff.size - 1 > B:
        raise ValueError("%s: groups must ascend from 0 to %d in at most %d groups, got %s" % (what, B, B, goff.tolist()))
    return goff.astype(np.int32)


def wave_loudness(wav_flat, starts, lengths, sample_rate, groups=None, true_peak=False, max_len=None, levels=None,
                  want_tables=False):
    """BS.1770 integrated loudness of B spans of a flat float32 device tensor (spans as wave_levels takes them: host
    integers, or int64 device tensors with max_len=), mono: K-weighting in float64 from a zero state at every span's own
    first sample, 400 ms blocks every 100 ms, the absolute gate at -70 and the relative gate 10 below the gated mean.
    groups: None (every span its own row) or group offsets, ascending host ints from 0 to B: a group's blocks are
    pooled.  -> float64 (G, 7) on the device, columns LOUDNESS_COLUMNS: lufs, blocks, gated_abs, gated_rel,
    momentary_max, true_peak, flags (bit 0: no complete block, measured ungated; bit 1: silent, lufs is -inf).
    true_peak=True: the peak column is the 4x oversampled true peak (true_peak_table), else the sample peak (from
    `levels`, wave_levels' table of the same spans, measured here when None).  want_tables: -> (rows, energy (B, K),
    states (B, K, 4)), the sub-block energies and every chunk's start state.  include/dv3hip.h states every step
    (dv3_wave_loudness_f64, dv3_loudness_gate_f64); tests/loudness_ref.py restates them.  No host read."""
    import ctypes
    wav_flat = _c(_chk(wav_flat, "wav_flat")).reshape(-1)
    kw = k_weighting(sample_rate)
    h = kw["h"]
    starts_d, lengths_d, B, max_len = _span_tables(wav_flat, starts, lengths, max_len, "wave_loudness")
    if not 1 <= B <= 65535:
        raise ValueError("wave_loudness: %d spans, at most 65535 per call" % B)
    if max_len > 2 ** 30:
        raise ValueError("wave_loudness: max_len=%d, at most 2^30 samples per span" % max_len)
    goff = _group_offsets(list(range(B + 1)) if groups is None else groups, B, "wave_loudness")
    G = goff.size - 1
    dev = wav_flat.device
    K = -(-max_len // h)
    f64 = dict(dtype=torch.float64, device=dev)
    states = torch.empty((B, max(K, 1), 4), **f64)
    energy = torch.empty((B, max(K, 1)), **f64)
    coef = (ctypes.c_double * 10)(*kw["coef"].tolist())
    Ah = (ctypes.c_double * 16)(*kw["Ah"].reshape(-1).tolist())
    if true_peak:
        table = (ctypes.c_float * 36)(*true_peak_table().reshape(-1).tolist())
        peak = torch.empty(B, **f64)
        scratch = torch.empty(max(B * -(-max_len // _lib.CONSTS["DV3_TRUE_PEAK_CHUNK"]), 1), **f64)
        stride = 1
    else:
        table = scratch = None
        peak = wave_levels(wav_flat, starts_d, lengths_d, max_len) if levels is None else _c(levels)
        if tuple(peak.shape) != (B, len(LEVEL_COLUMNS)) or peak.dtype != torch.float64 or not peak.is_cuda:
            raise ValueError("wave_loudness: levels must be wave_levels' float64 (B, 5) device table")
        stride = len(LEVEL_COLUMNS)
    _lib.call("dv3_wave_loudness_f64", wav_flat.data_ptr(), starts_d.data_ptr(), lengths_d.data_ptr(), B, max_len, h,
              ctypes.addressof(coef), ctypes.addressof(Ah), ctypes.addressof(table) if true_peak else None,
              states.data_ptr(), energy.data_ptr(), scratch.data_ptr() if true_peak else None,
              peak.data_ptr() if true_peak else None, _stream())
    goff_d = torch.from_numpy(goff).to(dev, non_blocking=True)
    rows = torch.empty((G, len(LOUDNESS_COLUMNS)), **f64)
    _lib.call("dv3_loudness_gate_f64", energy.data_ptr(), lengths_d.data_ptr(), goff_d.data_ptr(), peak.data_ptr(), stride,
              B, G, max_len, h, rows.data_ptr(), _stream())
    if want_tables:
        return rows, energy[:, :K], states[:, :K]
    return rows


def loudness_gains(rows, groups, mastering, ceiling=None, max_gain=None):
    """wave_loudness' rows -> float32 (B,) gains on the device, B = groups[-1]: group g (items groups[g] ..
    groups[g + 1] - 1) gets g = min(10^((target_db - lufs) / 20), ceiling / peak, max_gain), 1 when it is silent; float64
    on the device, rounded once (include/dv3hip.h: dv3_loudness_gains_f32).  mastering: a Mastering("lufs"); ceiling,
    max_gain: None (the Mastering's) or LINEAR values in their place (a limiter's pre-gain takes a ceiling that cannot
    bind)."""
    if not isinstance(mastering, Mastering) or mastering.level != "lufs":
        raise ValueError("loudness_gains: a Mastering with level='lufs' expected")
    G = int(rows.shape[0]) if torch.is_tensor(rows) and rows.dim() == 2 else -1
    if G < 1 or tuple(rows.shape) != (G, len(LOUDNESS_COLUMNS)) or rows.dtype != torch.float64 or not rows.is_cuda:
        raise ValueError("loudness_gains: rows must be wave_loudness' float64 (G, 7) device table")
    B = int(np.asarray(groups).reshape(-1)[-1]) if len(groups) else 0
    goff = _group_offsets(groups, B, "loudness_gains")
    if goff.size - 1 != G:
        raise ValueError("loudness_gains: %d rows for %d groups" % (G, goff.size - 1))
    dev = rows.device
    goff_d = torch.from_numpy(goff).to(dev, non_blocking=True)
    gain = torch.empty(B, dtype=torch.float32, device=dev)
    lin = lambda db: 10.0 ** (db / 20.0)
    _lib.call("dv3_loudness_gains_f32", _c(rows).data_ptr(), goff_d.data_ptr(), B, G, float(mastering.target_db),
              lin(mastering.ceiling_db) if ceiling is None else float(ceiling),
              lin(mastering.max_gain_db) if max_gain is None else float(max_gain), gain.data_ptr(), _stream())
    return gain


def span_gains(wav_flat, starts_d, lengths_d, max_len, mastering, sample_rate=None, ceiling=None):
    """the gains of B spans (int64 device tensors and a bound on the lengths) under a Mastering with a level: wave_levels
    and wave_gains, or under "lufs" wave_levels (the ceiling's sample peak), wave_loudness and loudness_gains; ceiling:
    None, or the LINEAR ceiling wave_gains / loudness_gains take in the Mastering's place"""
    if mastering.level != "lufs":
        return wave_gains(wave_levels(wav_flat, starts_d, lengths_d, max_len), lengths_d, mastering, ceiling=ceiling)
    levels = None if mastering.true_peak else wave_levels(wav_flat, starts_d, lengths_d, max_len)
    if sample_rate is None:
        raise ValueError("Mastering: level='lufs' needs a sample rate")
    B = int(starts_d.numel())
    groups = list(range(B + 1)) if mastering.scope == "item" else [0, B]
    rows = wave_loudness(wav_flat, starts_d, lengths_d, sample_rate, groups, mastering.true_peak, max_len, levels)
    return loudness_gains(rows, groups, mastering, ceiling=ceiling)


# ---- look-ahead peak limiter (csrc/limiter.hip) -----------------------------------------------------------
LIMITER_COLUMNS = ("gain_min", "over_samples")


def rho_powers(rho):
    """rho^(2^i), i = 0 .. log2(DV3_LIMIT_TILE), each one float64 pow (repeated squaring would double the relative error
    at every step): what dv3_wave_limit_f32 takes"""
    return np.array([float(rho) ** (2 ** i) for i in range(_lib.CONSTS["DV3_LIMIT_RHO_POWERS"])], dtype=np.float64)


def limit_spans(wav_flat, starts_d, lengths_d, max_len, gain, ceiling, lookahead, rho, true_peak=False):
    """The look-ahead limiter over B spans of a flat float32 device tensor (spans as wave_levels takes them: host
    integers, or int64 device tensors with max_len): span b times gain[b] (a float32 (B,) device tensor, or one number),
    held under `ceiling` (LINEAR) by a gain that turns down `lookahead` samples ahead of a peak and releases by the
    factor `rho` per sample; true_peak: the detector also reads the 4x interpolants (true_peak_table).  -> (a float32
    buffer of wav_flat's layout: the span samples limited, zeros elsewhere; float64 (B, 2) on the device, columns
    LIMITER_COLUMNS: the smallest gain the limiter applied and the number of samples that demanded a reduction).
    include/dv3hip.h (dv3_wave_limit_f32) states every step; tests/limiter_ref.py restates it.  No host read."""
    import ctypes
    wav_flat = _c(_chk(wav_flat, "wav_flat")).reshape(-1)
    starts_d, lengths_d, B, max_len = _span_tables(wav_flat, starts_d, lengths_d, max_len, "limit_spans")
    if not 1 <= B <= 65535:
        raise ValueError("limit_spans: %d spans, at most 65535 per call" % B)
    if max_len > 2 ** 30:
        raise ValueError("limit_spans: max_len=%d, at most 2^30 samples per span" % max_len)
    dev = wav_flat.device
    if not torch.is_tensor(gain):
        gain = torch.full((B,), float(gain), dtype=torch.float32, device=dev)
    if gain.numel() != B or gain.dtype != torch.float32 or not gain.is_cuda:
        raise ValueError("limit_spans: gain must be a number or a float32 device tensor of %d values" % B)
    T = _lib.CONSTS["DV3_LIMIT_TILE"]
    scratch = torch.empty(max(B * -(-max_len // T) * (T + 3), 1), dtype=torch.float64, device=dev)
    out = torch.zeros_like(wav_flat)
    report = torch.empty((B, len(LIMITER_COLUMNS)), dtype=torch.float64, device=dev)
    powers = (ctypes.c_double * _lib.CONSTS["DV3_LIMIT_RHO_POWERS"])(*rho_powers(rho).tolist())
    table = (ctypes.c_float * 36)(*true_peak_table().reshape(-1).tolist()) if true_peak else None
    _lib.call("dv3_wave_limit_f32", wav_flat.data_ptr(), starts_d.data_ptr(), lengths_d.data_ptr(), B, max_len,
              _c(gain).data_ptr(), float(ceiling), int(lookahead), ctypes.addressof(powers),
              ctypes.addressof(table) if true_peak else None, scratch.data_ptr(), out.data_ptr(), report.data_ptr(),
              _stream())
    return out, report


def master_source(wav_flat, starts_d, lengths_d, max_len, mastering, sample_rate=None):
    """What the master launch reads under a Mastering: -> (source buffer, per-span gains or None).  Without a limiter
    that is (wav_flat, span_gains(...)) -- None when the level is None.  With mastering.limiter the pre-gain drops the
    ceiling term (min(target gain, max_gain), or 1), limit_spans holds the spans under the ceiling, and the limited
    buffer comes back; Limiter(passes=P): P - 1 times the limited spans are measured by wave_loudness with the same
    groups, each group's pre-gain is multiplied by 10^((target - L) / 20) (capped at max_gain; a silent group's stays) and
    the ORIGINAL samples are limited again.  Under the true-peak detector the gain varies across an interpolant's 12 taps,
    so the limited buffer's true peak is measured once more and the gains are the trim min(1, ceiling / peak); under the
    sample-peak one they are None.  No host read."""
    lim = mastering.limiter
    if lim is None:
        if mastering.level is None:
            return wav_flat, None
        return wav_flat, span_gains(wav_flat, starts_d, lengths_d, max_len, mastering, sample_rate)
    if sample_rate is None:
        raise ValueError("Mastering: limiter= needs a sample rate (its look-ahead and release are times)")
    A, rho = lim.lookahead(sample_rate), lim.rho(sample_rate)
    lin = lambda db: 10.0 ** (db / 20.0)
    c, cap = lin(mastering.ceiling_db), lin(mastering.max_gain_db)
    B = int(starts_d.numel())
    if mastering.level is None:
        pre = torch.ones(B, dtype=torch.float32, device=wav_flat.device)
    else:
        pre = span_gains(wav_flat, starts_d, lengths_d, max_len, mastering, sample_rate, ceiling=_NO_CEILING)
    out, _ = limit_spans(wav_flat, starts_d, lengths_d, max_len, pre, c, A, rho, mastering.true_peak)
    groups = list(range(B + 1)) if mastering.scope == "item" else [0, B]
    for _ in range(lim.passes - 1):
        rows = wave_loudness(out, starts_d, lengths_d, sample_rate, groups, False, max_len)
        step = loudness_gains(rows, groups, mastering, ceiling=_NO_CEILING, max_gain=_NO_CEILING)
        pre = torch.clamp(pre * step, max=cap)
        out, _ = limit_spans(wav_flat, starts_d, lengths_d, max_len, pre, c, A, rho, mastering.true_peak)
    if not mastering.true_peak:
        return out, None
    peak = wave_loudness(out, starts_d, lengths_d, sample_rate, None, True, max_len)[:, LOUDNESS_COLUMNS.index("true_peak")]
    return out, torch.clamp(c / peak, max=1.0).to(torch.float32)


_FADE_CACHE = {}


def fade_table_np(F):
    """the rising half of a raised cosine sampled at the half-sample points: fade[i] = 0.5 - 0.5 cos(pi (i + 0.5) / F) in
    float64, rounded once to float32; fade[i] + fade[F - 1 - i] is 1 within one ulp"""
    i = np.arange(int(F), dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / float(F))).astype(np.float32) if F else np.zeros(0, np.float32)


def fade_table(device, F):
    key = (str(device), int(F))
    if key not in _FADE_CACHE:
        _FADE_CACHE[key] = torch.from_numpy(fade_table_np(F)).to(device)
    return _FADE_CACHE[key]


def check_segments(src, length, dst, total, N, reference=False):
    """the layout rules of dv3_wave_master_f32 on host integers -> (src, len, dst) int64 arrays; ValueError on a span
    outside the `total` source samples or the N output samples, on starts or ends that do not ascend, on an output sample
    under three segments, and in the reference mode on any overlap"""
    src, length, dst = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (src, length, dst))
    S = src.size
    if S < 1 or length.size != S or dst.size != S or S > _lib.CONSTS["DV3_MASTER_MAX_SEGMENTS"]:
        raise ValueError("wave_master: %d / %d / %d entries of src / len / dst (1 .. %d segments)" % (
            src.size, length.size, dst.size, _lib.CONSTS["DV3_MASTER_MAX_SEGMENTS"]))
    if int(length.min()) < 0 or int(src.min()) < 0 or int((src + length).max()) > int(total):
        raise ValueError("wave_master: a segment's span lies outside the %d source samples" % int(total))
    end = dst + length
    if int(dst.min()) < 0 or int(end.max()) > int(N):
        raise ValueError("wave_master: a segment lies outside the %d output samples" % int(N))
    if np.any(np.diff(dst) < 0) or np.any(np.diff(end) < 0):
        raise ValueError("wave_master: segments are not sorted (dst and dst + len must both ascend)")
    live = np.flatnonzero(length > 0)                     # an empty segment covers nothing
    if reference and live.size > 1 and np.any(dst[live][1:] < end[live][:-1]):
        raise ValueError("wave_master: the reference mode takes no overlapping segments")
    if live.size > 2 and np.any(dst[live][2:] < end[live][:-2]):
        raise ValueError("wave_master: an output sample is covered by three segments (at most two: a crossfade)")
    return src, length, dst


def wave_master(wav_flat, src, length, dst, gain, flags, N, fade_samples=0, dtype="int16", reference=False, dither=False,
                seed=0):
    """ONE launch that builds N output samples from S segments of a flat float32 device tensor: segment s =
    wav_flat[src[s] : src[s] + length[s]] goes to out[dst[s] : dst[s] + length[s]] times gain[s] (a float32 device
    tensor, or None: 1), faded in over its first / out over its last fade_samples samples where flags[s] has bit 0 / bit
    1; two segments laid over each other are added (a crossfade), samples under no segment are zero.  src, length, dst,
    flags: host integers, checked here (check_segments).  dtype "float32", or "int16" (round to nearest even of y *
    32767, saturating; dither=True adds TPDF dither from (seed, sample index) first); reference=True: int16 as the
    reference's save_wav makes it, gain[s] the DIVISOR max(0.01, peak).  include/dv3hip.h (dv3_wave_master_f32) states
    every step; tests/master_ref.py restates it.  -> the (N,) output; no host read."""
    wav_flat = _c(_chk(wav_flat, "wav_flat")).reshape(-1)
    N, F = int(N), int(fade_samples)
    src, length, dst = check_segments(src, length, dst, wav_flat.numel(), N, reference)
    S = src.size
    flags = np.array(np.broadcast_to(np.asarray(flags, dtype=np.int32), (S,)))        # (a writable copy)
    if dtype not in _MASTER_MODES or (reference and dtype != "int16"):
        raise ValueError("wave_master: dtype=%r (reference=%r)" % (dtype, reference))
    if not 0 <= F <= _lib.CONSTS["DV3_MASTER_MAX_FADE"]:
        raise ValueError("wave_master: fade_samples=%d outside [0, %d]" % (F, _lib.CONSTS["DV3_MASTER_MAX_FADE"]))
    dev = wav_flat.device
    tab = torch.from_numpy(np.concatenate([src, length, dst])).to(dev, non_blocking=True)
    flags_d = torch.from_numpy(flags).to(dev, non_blocking=True)
    if gain is None:
        gain = torch.ones(S, dtype=torch.float32, device=dev)
    if gain.numel() != S or gain.dtype != torch.float32 or not gain.is_cuda:
        raise ValueError("wave_master: gain must be a float32 device tensor of %d values" % S)
    gain = _c(gain)
    fade = fade_table(dev, F) if F else None
    mode = _lib.CONSTS["DV3_MASTER_I16_REFERENCE" if reference else _MASTER_MODES[dtype]]
    out = torch.empty(N, dtype=torch.int16 if dtype == "int16" else torch.float32, device=dev)
    if N == 0:                                            # (every segment empty: nothing to launch)
        return out
    _lib.call("dv3_wave_master_f32", wav_flat.data_ptr(), tab[:S].data_ptr(), tab[S:2 * S].data_ptr(), tab[2 * S:].data_ptr(),
              gain.data_ptr(), flags_d.data_ptr(), S, fade.data_ptr() if F else None, F, mode, int(bool(dither)), int(seed),
              out.data_ptr(), N, _stream())
    return out


def master_items(wavs, samples, mastering, sample_rate=None):
    """Every utterance of a padded batch mastered ALONE: wavs (B, L) float32 on the device (tts_batch's Griffin-Lim
    output), samples: B host ints (item b is its first samples[b] samples; the lengths are already on the host, so
    nothing is read back), mastering: a Mastering.  -> (B, L) of mastering.dtype, item b's samples first and zeros behind
    them (a view of a buffer whose rows are padded to 16 bytes).  Levels, gains (they stay on the device) and one master
    launch; with dither one master launch per item, each counting its samples from 0, so that an item's bits do not
    depend on what shares its batch.  No fades: fade_ms is for join_utterances.  sample_rate: needed by level "lufs"
    and by a limiter (master_source, which gives the launch its source and gains)."""
    mastering = check_mastering(mastering, "master_items")
    if mastering is None:
        raise ValueError("master_items: mastering is None")
    wavs = _c(_chk(wavs, "wavs"))
    if wavs.dim() != 2 or min(wavs.shape) < 1:
        raise ValueError("master_items: a non-empty (B, L) batch expected, got %s" % (tuple(wavs.shape),))
    B, L = wavs.shape
    samples = np.asarray(torch.as_tensor(samples).cpu() if torch.is_tensor(samples) else samples, dtype=np.int64).reshape(-1)
    if samples.size != B or int(samples.min()) < 0 or int(samples.max()) > L:
        raise ValueError("master_items: %d lengths in [0, %d] expected, got %s" % (B, L, samples.tolist()))
    flat = wavs.reshape(-1)
    starts = np.arange(B, dtype=np.int64) * L
    gain = None
    if mastering.level == "lufs" and sample_rate is None:
        raise ValueError("master_items: level='lufs' needs sample_rate= (the loudness measure is defined per sample rate)")
    if mastering.limiter is not None and sample_rate is None:
        raise ValueError("master_items: limiter= needs sample_rate= (its look-ahead and release are times)")
    if mastering.level is not None or mastering.limiter is not None:
        starts_d, lengths_d, _, max_len = _span_tables(flat, starts, samples, None, "master_items")
        flat, gain = master_source(flat, starts_d, lengths_d, max_len, mastering, sample_rate)
    Lp = -(-L // 8) * 8
    kw = dict(dtype=mastering.dtype, reference=mastering.level == "reference", seed=mastering.seed)
    if not mastering.dither:
        out = wave_master(flat, starts, samples, np.arange(B, dtype=np.int64) * Lp, gain, 0, B * Lp, **kw)
        return out.view(B, Lp)[:, :L]
    out = torch.empty((B, Lp), dtype=torch.int16, device=wavs.device)
    for b in range(B):
        out[b] = wave_master(flat, starts[b:b + 1], samples[b:b + 1], [0], None if gain is None else gain[b:b + 1], 0, Lp,
                             dither=True, **kw)
    return out[:, :L]


def to_pcm16(wavs, samples):
    """the reference's save_wav samples (audio.py:16-18) of a padded batch, on the device: item b becomes
    (x * 32767 / max(0.01, max |x|)).astype(int16) over its own samples[b] samples, bit for bit numpy's float32
    evaluation -> int16 (B, L)"""
    return master_items(wavs, samples, Mastering(level="reference"))


def save_wav(path, pcm, sample_rate):
    """write mono 16-bit PCM with the standard library's `wave`: pcm a 1-D int16 tensor (any device) or array -- what
    master_items, to_pcm16 or synthesis.join_utterances return under dtype "int16"; float data is refused, not scaled"""
    import wave
    if torch.is_tensor(pcm):
        pcm = pcm.detach().cpu().numpy()
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16 or pcm.ndim != 1:
        raise ValueError("save_wav: 1-D int16 samples expected, got %s of shape %s (master with dtype='int16' first)"
                         % (pcm.dtype, pcm.shape))
    sr = int(sample_rate)
    if sr < 1 or sr != sample_rate:
        raise ValueError("save_wav: sample_rate=%r must be a positive integer" % (sample_rate,))
    w = wave.open(path, "wb")
    try:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(pcm.astype("<i2")).tobytes())
    finally:
        w.close()
