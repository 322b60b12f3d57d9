# coding: utf-8
"""Batched synthesis of different utterances (the batched counterpart of the reference's synthesis.tts,
synthesis.py:42-73, without its text frontend): every utterance comes back as if it had been synthesised alone.

    from deepvoice3_pytorch_amd import synthesis
    for mel, linear, alignment, wav in synthesis.tts_batch(model, [seq0, seq1, ...]):
        ...

The model part is MultiSpeakerTTSModel.synthesize_batch (per-utterance attention, stop and zero tails on the HIP
kernels); the waveforms are ONE batched Griffin-Lim call with per-item frame counts (audio.inv_spectrogram_batch(...,
frame_lengths=)), each item equal to the inverse of its own trimmed spectrogram.

Rolling admission: tts_batch is one rigid wave -- every item starts at step 0 and nothing new starts
before the slowest item has stopped.  RollingSynthesizer keeps a fixed number of decode SLOTS busy instead: an utterance
is admitted into a slot as soon as one frees, decodes at its own step index next to neighbours that are further along,
and retires (post-net + Griffin-Lim) when its own stop rule fires.

    rs = synthesis.RollingSynthesizer(model, slots=64, max_text_len=200)
    ticket = rs.submit(ids)                      # queued; admitted when a slot frees
    for ticket, mel, linear, alignment, wav in rs.poll(): ...     # one chunk of decoder steps; what retired in it
    for ... in rs.drain(): ...                   # until the queue and the slots are empty
    for index, mel, linear, alignment, wav in synthesis.tts_stream(model, sequences, slots=64): ...   # completion order

Alignment diagnostics and the end-of-text stop, both opt-in on all three entry points:
diagnostics=True appends to every result the utterance's alignment statistics (ops.alignment_stats: one small reduction
on the device over the stored attention rows, one device read per returned group) as a dict keyed by ALIGNMENT_COLUMNS
plus "flags" (alignment_flags); stall_limit=K stops an utterance K steps after its attention first reached its last
key when the done flag has not fired by then (decode_program.stall_stop).

    for mel, linear, alignment, wav, stats in synthesis.tts_batch(model, seqs, diagnostics=True, stall_limit=8):
        if stats["flags"]: ...                   # e.g. ("incomplete", "stalled")

Token timings, opt-in on all three entry points: timings=True appends to every result (after the
diagnostics element, if there is one) the utterance's timing dict -- the best monotonic path through its stored
attention rows (ops.monotonic_path) and, from it, the span of the waveform every input token is spoken in.  Device
tensors, no host read.  They are the best monotonic reading of THIS model's attention at decoder-step resolution (one
step is r mel frames, r * upsampling hops of the waveform), not a phonetic aligner's output.

    for mel, linear, alignment, wav, timing in synthesis.tts_batch(model, seqs, timings=True):
        for token, t0, t1 in zip(seq, timing["start"].tolist(), timing["end"].tolist()): ...     # seconds

Vocoding from the mel, opt-in on all three entry points: from_mel=True (or an audio.MelInverse) skips
the post-net -- a model trained with train_postnet=False has a random one -- and inverts the decoder's mel instead:
`linear` is audio.mel_to_linear of the utterance's own mel frames at the post-net's upsampling, `wav` its Griffin-Lim
inversion.  A preview of the seq2seq half: the mel is interpolated in time and bins outside the mel band stay at the
floor.

    for mel, linear, alignment, wav in synthesis.tts_batch(model, seqs, from_mel=True): ...

Speaking rate and pitch, opt-in on all three entry points (per ticket on RollingSynthesizer.submit):
rate= (above 1: faster) and semitones=, a scalar or one value per utterance, and prosody= (an audio.Prosody: the envelope
settings) are applied where the utterance is vocoded -- audio.warp_magnitudes between the magnitudes and Griffin-Lim --,
so `wav` changes and mel, linear and alignment stay what the model made; token spans follow the new time axis.

    for mel, linear, alignment, wav in synthesis.tts_batch(model, seqs, rate=[0.8, 1.0], semitones=[0, 3]): ...

Prosody marks, opt-in on all three entry points (per ticket on RollingSynthesizer.submit): marks= takes
one audio.ProsodyMarks per utterance (or None) -- spans of TOKENS with their own rate, semitones and gain_db, breaks after
tokens, an optional transition.  The utterance's monotonic path (ops.monotonic_path) turns token spans into frame spans
on the device, audio.plan_prosody turns those into per-frame tables and the warp follows them; only `wav` changes, and
with timings a slowed token gets longer and a break is the gap between two tokens.  Not together with rate=, semitones=
or prosody=.  An utterance without an admissible path is vocoded without its marks (audio.MarksNotApplied warning).
tts_document does not take marks: it trims and joins what tts_batch returns.

    marks = audio.ProsodyMarks(spans=[(4, 9, dict(rate=0.8))], breaks=[(9, 0.3)], transition_ms=30)
    for mel, linear, alignment, wav in synthesis.tts_batch(model, [seq0, seq1], marks=[marks, None]): ...

Deliverable audio, opt-in: mastering= (an audio.Mastering) on all three entry points turns every `wav`
into the mastered one (audio.master_items: each utterance alone, so the three agree); join_utterances joins any list of
device waveforms into one document -- silence trimmed, levelled, sentences crossfaded or separated by faded pauses,
quantised, in one launch after one host read --, and tts_document speaks a text longer than one utterance, sentence by
sentence, with every token's span on the document's time axis.  Mastering("lufs") levels to a BS.1770 loudness target
(DESIGN.md 3.6l): per utterance, or with scope="document" from the pooled blocks of all sentences; the entry points
pass their audio_cfg.sample_rate.  Mastering(..., limiter=audio.Limiter()) holds the ceiling with a look-ahead limiter
instead of the static gain: every utterance is limited alone, before any join.

    wav, spans = synthesis.tts_document(model, [seq0, seq1, ...], mastering=audio.Mastering("rms", "document"))
    audio.save_wav("document.wav", wav, 22050)

Free-running evaluation: how far is the model's own synthesis of a held-out sentence from its
recording?  evaluate_synthesis decodes (no Griffin-Lim), aligns each utterance with its target by dynamic time warping
(ops.dtw) under the mel-cepstral distance (audio.mel_cepstra) and returns one row per utterance; SynthEvalTotals folds
the rows of a set into its MCD (dB per aligned frame pair) and duration ratio.

    totals = synthesis.SynthEvalTotals()
    for ids, seqs, mels in held_out_batches:
        totals.add(synthesis.evaluate_synthesis(model, seqs, mels, downsample_step=4), ids)
    print(totals.result()["mcd"], totals.result()["duration_ratio"])

The same at the waveform: evaluate_synthesis_audio synthesises with tts_batch under the AudioConfig
being judged and compares each waveform with its recording -- both analysed alike, the distortion along the DTW path and,
from audio.yin_items' pitch tracks along that same path, the F0 error in cents and the voicing disagreement
(waveform_distortion, pitch_distortion); WaveEvalTotals folds a set.

    totals = synthesis.WaveEvalTotals()
    for ids, seqs, recordings in held_out_batches:
        totals.add(synthesis.evaluate_synthesis_audio(model, seqs, recordings, audio_cfg=cfg), ids)
    r = totals.result(); print(r["mcd"], r["f0_rmse_cents"], r["vuv_error"], r["duration_ratio"])
"""
import collections

import numpy as np
import torch

from . import audio
from .decode_program import ALIGNMENT_COLUMNS, RollingSchedule, end_of_text_stops, item_stops

# Thresholds of alignment_flags.  The defaults are starting points for a user to tune on their own voice: they are NOT
# measured on any trained model (the repository holds no trained weights).
#   end_tolerance  "incomplete": furthest_key < keys - 1 - end_tolerance
#   back_steps     "regressed":  back_steps > back_steps
#   max_jump       "skipped":    max_jump > max_jump
#   stall          "stalled":    longest_stall > stall
#   focus          "unfocused":  focus_mean < focus
AlignmentLimits = collections.namedtuple("AlignmentLimits", "end_tolerance back_steps max_jump stall focus")
AlignmentLimits.__new__.__defaults__ = (1, 2, 3, 8, 0.3)


def alignment_flags(row, max_steps=None, limits=None):
    """What an alignment-statistics row says went wrong, on the host: row is a dict keyed by ALIGNMENT_COLUMNS (extra
    keys ignored) or the 13 values in that order; max_steps: the cap the utterance decoded under (None: "capped" is not
    judged); limits: an AlignmentLimits (None: the untuned defaults).  -> a sorted tuple of
    "bad_rows" (some row had no usable maximum), "capped" (ran max_steps + 1 steps: the done flag never fired),
    "incomplete", "regressed", "skipped", "stalled", "unfocused" (see AlignmentLimits)."""
    if not isinstance(row, dict):
        row = dict(zip(ALIGNMENT_COLUMNS, row))
    lim = limits or AlignmentLimits()
    flags = []
    if row["bad_rows"] > 0:
        flags.append("bad_rows")
    if max_steps is not None and row["steps"] == int(max_steps) + 1:
        flags.append("capped")
    if row["furthest_key"] < row["keys"] - 1 - lim.end_tolerance:
        flags.append("incomplete")
    if row["back_steps"] > lim.back_steps:
        flags.append("regressed")
    if row["max_jump"] > lim.max_jump:
        flags.append("skipped")
    if row["longest_stall"] > lim.stall:
        flags.append("stalled")
    if row["focus_mean"] < lim.focus:
        flags.append("unfocused")
    return tuple(sorted(flags))


def _diagnose(alignments, steps, lengths, caps):
    """alignments (B, T, Tk) on the device, item b's rows < steps[b] and keys < lengths[b]; caps: each item's
    max_decoder_steps -> one dict per item: its statistics as Python numbers, and "flags" (one device read)"""
    from . import ops
    dev = alignments.device
    as_i32 = lambda v: torch.tensor([int(x) for x in v], dtype=torch.int32).to(dev)
    rows = ops.alignment_stats(alignments, as_i32(steps), as_i32(lengths), "btk").tolist()
    out = []
    for vals, cap in zip(rows, caps):
        row = {k: (float(v) if k.startswith("focus") else int(v)) for k, v in zip(ALIGNMENT_COLUMNS, vals)}
        row["flags"] = alignment_flags(row, cap)
        out.append(row)
    return out


# the columns of a timing summary row (include/dv3hip.h: dv3_mono_path_f32), in order
TIMING_COLUMNS = ("feasible", "steps", "keys", "score", "skipped_keys", "longest")


def seconds_per_step(audio_cfg, r, upsampling):
    """the waveform time of one decoder step: r mel frames of `upsampling` linear frames of hop_size samples each"""
    cfg = audio_cfg or audio.AudioConfig()
    return float(int(r) * int(upsampling) * cfg.hop_size) / float(cfg.sample_rate)


def token_spans(durations, seconds_per_step):
    """durations (..., N) integer steps per key -> (start, end) float64 of the same shape, in seconds:
    start[n] = seconds_per_step * sum_{m < n} durations[m], end[n] = start[n] + seconds_per_step * durations[n] (both as
    seconds_per_step times an exact integer sum, so end[-1] is exactly the steps times seconds_per_step)"""
    upto = torch.cumsum(durations.to(torch.int64), dim=-1)
    sps = float(seconds_per_step)
    return (upto - durations).to(torch.float64) * sps, upto.to(torch.float64) * sps


def fit_durations(durations, total_steps, min_steps=0):
    """One utterance's per-token step counts scaled to an exact total, on the host: the "exact length"
    and "rate at the model" helper in front of tts_batch(durations=...).  durations: N non-negative ints (a list, an
    array or a tensor); total_steps: what the result sums to; min_steps: what every token gets at least.
    Token n's weight is w[n] = max(durations[n] - min_steps, 0); it gets min_steps + w[n] * R / sum(w) of the
    R = total_steps - N * min_steps steps left, rounded by largest remainder in exact integer arithmetic (ties: the
    earlier token).  So with min_steps = 0 a token of duration 0 stays 0; a token with the larger duration never gets
    fewer steps; and total_steps = sum(durations) with every duration >= min_steps gives the durations back.  Weights
    that are all zero under a min_steps > 0 share R evenly.  -> a list of N ints.
    ValueError: a negative duration, min_steps < 0, total_steps < N * min_steps, or nothing to scale (all durations 0
    at min_steps = 0 and total_steps > 0)."""
    d = [int(v) for v in (durations.tolist() if hasattr(durations, "tolist") else durations)]
    total, m, N = int(total_steps), int(min_steps), len(d)
    if N == 0 or min(d) < 0 or m < 0:
        raise ValueError("fit_durations: at least one duration, none negative, and min_steps >= 0 expected")
    R = total - N * m
    if R < 0:
        raise ValueError("fit_durations: %d steps do not hold %d tokens of at least %d steps" % (total, N, m))
    w = [max(v - m, 0) for v in d]
    S = sum(w)
    if S == 0:
        if m == 0 and R > 0:
            raise ValueError("fit_durations: all durations are 0: there is nothing to scale to %d steps" % total)
        w, S = [1] * N, N
    out = [m + v * R // S for v in w]
    left = total - sum(out)                          # < N: one more step each, by remainder, the earlier token first
    order = sorted(range(N), key=lambda n: (-(w[n] * R % S), n))
    for n in order[:left]:
        out[n] += 1
    return out


def search_path(alignments, steps, lengths, layout="btk", max_advance=1):
    """ops.monotonic_path with host step and key counts -> (summary rows, path, durations) on the device, no host read"""
    from . import ops
    as_i32 = lambda v: torch.tensor([int(n) for n in v], dtype=torch.int32).to(alignments.device)
    return ops.monotonic_path(alignments, as_i32(steps), as_i32(lengths), layout, max_advance)


def token_timings(alignments, steps, lengths, seconds_per_step, layout="btk", max_advance=1):
    """Where every input token is spoken: alignments / layout as ops.monotonic_path takes them (read in place), item b's
    rows < steps[b] and keys < lengths[b] (host ints); seconds_per_step: the waveform time of one decoder step;
    max_advance: the search's J (1: no token is skipped).  One library call for the batch, no host synchronisation.
    -> one dict of device tensors per item, trimmed to the item: "path" (T_b,) int32, the key of every step;
    "durations" (N_b,) int32, the steps of every key; "start" and "end" (N_b,) float64, token_spans of them in seconds;
    "summary" (len(TIMING_COLUMNS),) fp32, the item's row.  An item without an admissible path (summary[0] = 0) has a
    path of -1, zero durations and empty spans at 0."""
    return timings_of_path(search_path(alignments, steps, lengths, layout, max_advance), steps, lengths, seconds_per_step)


def timings_of_path(searched, steps, lengths, seconds_per_step):
    """token_timings' dicts from what search_path returned for the same steps and lengths (a caller that needs the
    durations for something else too searches once)"""
    steps, lengths = [int(n) for n in steps], [int(n) for n in lengths]
    out, path, durations = searched
    start, end = token_spans(durations, seconds_per_step)
    T, Tk = path.size(1), durations.size(1)
    res = []
    for b, (t, n) in enumerate(zip(steps, lengths)):
        t, n = min(max(t, 0), T), min(max(n, 1), Tk)
        res.append({"path": path[b, :t], "durations": durations[b, :n], "start": start[b, :n], "end": end[b, :n],
                    "summary": out[b]})
    return res


def check_linear_dim(model, audio_cfg, what):
    """the model's linear_dim must be the audio config's fft_size // 2 + 1 (513 at 1024, 257 at 512, 1025 at 2048):
    refused here, once, with both numbers, instead of inside Griffin-Lim after the decode"""
    cfg = audio_cfg or audio.AudioConfig()
    audio.check_bins(model.linear_dim, cfg.fft_size, "%s: model.linear_dim = %d" % (what, model.linear_dim))


def postnet_upsampling(model):
    """linear frames per mel frame of the model's post-net, without a forward: the product of the strides of its
    transposed convolutions, 2 ** (the number of conv layers with transposed = True)"""
    from . import conv
    return 2 ** sum(1 for m in model.postnet.modules() if isinstance(m, conv._WNLayer) and m.transposed)


def mel_options(from_mel):
    """the `from_mel=` keyword of the entry points -> None (off), or the audio.MelInverse to vocode the mel with:
    True means MelInverse(), an instance is used as given"""
    if from_mel is None or from_mel is False:
        return None
    if from_mel is True:
        return audio.MelInverse()
    if not isinstance(from_mel, audio.MelInverse):
        raise ValueError("from_mel must be False, True or an audio.MelInverse, got %r" % (from_mel,))
    return from_mel


def utterance_prosody(rate, semitones, prosody, B, what):
    """the `rate=`, `semitones=`, `prosody=` keywords of the entry points -> None (nothing asked for, or nothing that
    changes anything), or an audio.Prosody with what applies to the B utterances: rate and semitones (a scalar or one
    value per utterance) where given, else the prosody's own; the envelope settings are the prosody's (default: an
    audio.Prosody()).  Values and lengths are refused as audio.Prosody refuses them."""
    if rate is None and semitones is None and prosody is None:
        return None
    if prosody is not None and not isinstance(prosody, audio.Prosody):
        raise ValueError("%s: prosody must be an audio.Prosody, got %r" % (what, prosody))
    base = prosody if prosody is not None else audio.Prosody()
    own = lambda scalar, vals: vals[0] if scalar else vals
    p = audio.Prosody(own(base._scalar_rate, base.rate) if rate is None else rate,
                      own(base._scalar_semitones, base.semitones) if semitones is None else semitones,
                      base.preserve_envelope, base.envelope_hz)
    p.per_item(B)
    return None if p.neutral() else p


def utterance_marks(marks, rate, semitones, prosody, B, what):
    """the `marks=` keyword of the entry points -> None (nothing asked for, or nothing that changes anything) or a list of
    B entries, each an audio.ProsodyMarks in tokens or None.  One mechanism per call: marks together with rate,
    semitones or prosody are refused."""
    if marks is None:
        return None
    if rate is not None or semitones is not None or prosody is not None:
        raise ValueError("%s: marks cannot be combined with rate, semitones or prosody: one mechanism per call" % what)
    return audio.item_marks(marks, B, "tokens", what)


def token_bounds(durations, marks, step_frames, audio_cfg=None):
    """the source frame every segment of the items' marks starts at: durations (G, Tk) steps per key on the device (zero
    past an item's keys), marks: G ProsodyMarks in tokens, step_frames: linear frames per decoder step (r * upsampling)
    -> int32 (G, S + 1) on the device: the running sum of the durations gathered at the segments' first tokens (a token
    index past the text gives the utterance's end) times step_frames.  No host read.  Decoder-step resolution."""
    start = audio.marks_tables(marks, audio_cfg)["start"]
    upto = torch.nn.functional.pad(torch.cumsum(durations.to(torch.int64), dim=1), (1, 0))
    idx = torch.from_numpy(np.minimum(start, durations.size(1))).to(durations.device)
    return (torch.gather(upto, 1, idx) * int(step_frames)).to(torch.int32)


def _spans_under_plan(span, plan, row, step_frames, audio_cfg):
    """a timing dict on the time axis of an utterance spoken under a plan (audio.plan_map): a token's start is mapped as a
    start, its end as an end, so a break shows as the gap between one token's end and the next one's start"""
    cfg = audio_cfg or audio.AudioConfig()
    one = {k: (v[row:row + 1] if torch.is_tensor(v) and v.dim() >= 1 and k != "out_lengths" else v) for k, v in plan.items()}
    upto = torch.cumsum(span["durations"].to(torch.int64), dim=0)
    sec = float(cfg.hop_size) / float(cfg.sample_rate)
    out = dict(span)
    out["start"] = audio.plan_map(one, ((upto - span["durations"]) * int(step_frames))[None], "start")[0] * sec
    out["end"] = audio.plan_map(one, (upto * int(step_frames))[None], "end")[0] * sec
    return out


def _vocode_marked(linear, audio_cfg, frame_lengths, settings, marks, searched, step_frames, what):
    """_vocode for a group in which some items carry ProsodyMarks (marks: per item one or None; searched: search_path's
    result for the group).  The marked items are vocoded in one audio.inv_spectrogram_marks call per key() -- token bounds
    from the path's durations, all on the device --, the others by _vocode; every item's waveform depends on the item
    alone.  An item whose path is infeasible is vocoded without its marks, and an audio.MarksNotApplied warning names it
    (the flag rides in the plan's one host read).  -> (waveforms, sample lengths, per item None or (plan, row))"""
    import warnings
    G, dev = len(marks), linear.device
    fl = torch.as_tensor(frame_lengths).reshape(-1).to(torch.int64)
    feasible, durations = searched[0][:, 0] > 0, searched[2]
    groups = {}
    for g, m in enumerate(marks):
        if m is not None:
            groups.setdefault(m.key(), []).append(g)
    rest = [g for g in range(G) if marks[g] is None]
    parts, plans = [], [None] * G
    if rest:
        parts.append((rest,) + tuple(_vocode(linear[torch.tensor(rest, device=dev)], audio_cfg, fl[rest],
                                             [settings[g] for g in rest])))
    for key in sorted(groups):
        idx = groups[key]
        at = torch.tensor(idx, device=dev)
        sub_marks = [marks[g] for g in idx]
        bounds = token_bounds(durations[at], sub_marks, step_frames, audio_cfg)
        w, n, plan = audio.inv_spectrogram_marks(linear if len(idx) == G else linear[at], audio_cfg, fl[idx], sub_marks,
                                                 bounds, feasible[at])
        parts.append((idx, w, n))
        for row, g in enumerate(idx):
            plans[g] = (plan, row)
        lost = [g for row, g in enumerate(idx) if not plan["usable"][row]]
        if lost:
            warnings.warn(audio.MarksNotApplied("%s: no monotonic path for item(s) %s of the group: vocoded without their "
                                                "marks" % (what, lost)))
    if len(parts) == 1:
        return parts[0][1], parts[0][2], plans
    wavs = linear.new_zeros((G, max(w.size(1) for _, w, _ in parts)))
    samples = torch.zeros(G, dtype=torch.int64)
    for idx, w, n in parts:
        wavs[torch.tensor(idx, device=dev), :w.size(1)] = w
        samples[idx] = n
    return wavs, samples, plans


def _spans_at_rate(span, rate):
    """a timing dict on the time axis of an utterance spoken at `rate`: start and end in seconds divided by it (the
    summary's columns are counts of steps and keys and a score, none in seconds: they stay)"""
    if rate == 1.0:
        return span
    out = dict(span)
    out["start"], out["end"] = span["start"] / rate, span["end"] / rate
    return out


def _vocode(linear, audio_cfg, frame_lengths, settings):
    """one retiring group's Griffin-Lim: settings holds per item None or that ticket's scalar audio.Prosody.  Items whose
    envelope settings agree (and those without any) share ONE inv_spectrogram_batch call with per-item rates and shifts;
    a group that mixes envelope settings is vocoded in one call per setting -- every item's waveform depends on the
    item alone, so the split changes no result.  -> (waveforms (G, L), sample lengths int64[G])"""
    keys = sorted({(p.preserve_envelope, p.envelope_hz) for p in settings if p is not None})
    if not keys:
        return audio.inv_spectrogram_batch(linear, audio_cfg, frame_lengths=frame_lengths)
    fl = torch.as_tensor(frame_lengths).reshape(-1).to(torch.int64)
    parts = []
    for n, key in enumerate(keys):
        idx = [g for g, p in enumerate(settings)
               if (p is None and n == 0) or (p is not None and (p.preserve_envelope, p.envelope_hz) == key)]
        pros = audio.Prosody([1.0 if settings[g] is None else settings[g].rate[0] for g in idx],
                             [0.0 if settings[g] is None else settings[g].semitones[0] for g in idx], key[0], key[1])
        sub = linear if len(idx) == len(settings) else linear[torch.tensor(idx, device=linear.device)]
        parts.append((idx,) + tuple(audio.inv_spectrogram_batch(sub, audio_cfg, frame_lengths=fl[idx], prosody=pros)))
    if len(parts) == 1:
        return parts[0][1], parts[0][2]
    wavs = linear.new_zeros((len(settings), max(w.size(1) for _, w, _ in parts)))
    samples = torch.zeros(len(settings), dtype=torch.int64)
    for idx, w, s in parts:
        wavs[torch.tensor(idx, device=linear.device), :w.size(1)] = w
        samples[idx] = s
    return wavs, samples


def tts_batch(model, sequences, speaker_ids=None, audio_cfg=None, diagnostics=False, stall_limit=None, timings=False,
              timing_advance=1, rate=None, semitones=None, prosody=None, marks=None, mastering=None, durations=None,
              guide_window=None, from_mel=False):
    """sequences: a list of int id sequences (one per utterance); speaker_ids: None or one id per utterance.
    -> a list of (mel (T_b, mel_dim), linear (T_b * upsampling, linear_dim), alignment (steps_b, Tt_b), wav (L_b,)),
    device tensors, each trimmed to its own utterance.  diagnostics: a fifth element, the utterance's alignment
    statistics (see the module text); stall_limit: the end-of-text stop (synthesize_batch applies it after the decode:
    the batch still decodes until its slowest item's done flag, the stopped items' frames past the rule are dropped).
    timings: one more element, after the statistics if they are there: the utterance's timing dict (token_timings, with
    max_advance = timing_advance and the seconds per decoder step of audio_cfg); off: nothing is launched for it.
    from_mel (False; True or an audio.MelInverse): vocode the decoder's MEL instead of the post-net's output -- the
    post-net is not run (a model trained without it has a random one), `linear` is audio.mel_to_linear of the
    utterance's own mel frames at the post-net's upsampling (postnet_upsampling; audio_cfg's bins, not the model's
    linear_dim) and `wav` its inversion.  A preview of the seq2seq half, not the post-net's quality.
    rate, semitones (a scalar or one value per utterance), prosody (an audio.Prosody: the envelope settings, and the
    rates and shifts where the two keywords do not give them): how each utterance is spoken -- applied
    to the magnitudes on their way into Griffin-Lim (audio.warp_magnitudes), so only `wav` changes, to
    audio.num_samples(audio.warped_frames(frames, rate)) samples; mel, linear and alignment stay what the model made,
    and with timings every token's start and end are divided by the utterance's rate.
    mastering (an audio.Mastering): `wav` becomes audio.master_items of the batch's waveforms -- every utterance levelled
    and quantised alone; nothing else in the result changes.
    marks (one audio.ProsodyMarks in tokens per utterance, None entries allowed): rate, pitch, level and
    pauses that vary WITHIN the utterance.  The token bounds are the running sums of the monotonic path's durations
    (ops.monotonic_path at max_advance = timing_advance) times r * upsampling, gathered on the device; only `wav` changes,
    to audio.num_samples(T'_b) samples under the plan's frame count; with timings every token's start and end go through
    audio.plan_map -- tokens in a slowed span get longer and a break is the gap between two tokens.  An utterance
    without an admissible path is vocoded without its marks under an audio.MarksNotApplied warning.  marks together with
    rate, semitones or prosody are refused; marks that change nothing launch nothing.
    durations: decoder steps per token, one list of len(sequence) ints per utterance or an int32
    (B, longest sequence) device tensor -- the decode is guided (synthesize_batch(durations=...)): utterance b has
    exactly sum(durations[b]) decoder steps and every step attends around the token that owns it; guide_window
    (backward, ahead) replaces the attention layers' own window.  Not together with stall_limit (the stop is
    prescribed).  Everything else -- diagnostics, timings, from_mel, rate / semitones / marks, mastering -- works on
    what the guided decode stored."""
    if len(sequences) == 0:
        return []
    if durations is not None and stall_limit is not None:
        raise ValueError("tts_batch: durations prescribe every utterance's stop; stall_limit cannot be combined with them")
    audio.check_mastering(mastering, "tts_batch")
    marks = utterance_marks(marks, rate, semitones, prosody, len(sequences), "tts_batch")
    pros = utterance_prosody(rate, semitones, prosody, len(sequences), "tts_batch")
    mel_opt = mel_options(from_mel)
    if mel_opt is None:
        check_linear_dim(model, audio_cfg, "tts_batch")
    dev = next(model.parameters()).device
    lengths = [len(s) for s in sequences]
    if min(lengths) < 1:
        raise ValueError("tts_batch: empty sequence")
    B, Tt = len(sequences), max(lengths)
    pad = model.seq2seq.encoder.embed_tokens.padding_idx
    text = torch.full((B, Tt), 0 if pad is None else pad, dtype=torch.long)
    for b, s in enumerate(sequences):
        text[b, :len(s)] = torch.as_tensor(s, dtype=torch.long)
    text = text.to(dev)
    spk = None
    if speaker_ids is not None:
        spk = torch.as_tensor(speaker_ids, dtype=torch.long).reshape(-1).to(dev)
    model.eval()
    guided = {} if durations is None and guide_window is None else dict(durations=durations, guide_window=guide_window)
    mel, linear, alignments, _, frames = model.synthesize_batch(text, lengths, spk, stall_limit=stall_limit,
                                                                postnet=mel_opt is None, **guided)
    up = linear.size(1) // mel.size(1) if mel_opt is None else postnet_upsampling(model)
    steps_per_frame = mel.size(1) // alignments.size(1)        # r
    with torch.no_grad():
        if mel_opt is not None:
            linear = audio.mel_to_linear(mel, audio_cfg, frames, up, mel_opt)
        steps = [int(n) // steps_per_frame for n in frames]
        searched = plans = None
        if marks is not None:
            searched = search_path(alignments, steps, lengths, "btk", timing_advance)
            wavs, samples, plans = _vocode_marked(linear, audio_cfg, frames * up, [None] * B, marks, searched,
                                                  steps_per_frame * up, "tts_batch")
        else:
            wavs, samples = audio.inv_spectrogram_batch(linear, audio_cfg, frame_lengths=frames * up, prosody=pros)
        if mastering is not None:
            wavs = audio.master_items(wavs, samples, mastering, (audio_cfg or audio.AudioConfig()).sample_rate)
    stats = None
    if diagnostics:
        steps = [int(n) // steps_per_frame for n in frames]
        stats = _diagnose(alignments, steps, lengths, [model.seq2seq.decoder.max_decoder_steps] * B)
    spans = None
    if timings:
        steps, sps = [int(n) // steps_per_frame for n in frames], seconds_per_step(audio_cfg, steps_per_frame, up)
        spans = token_timings(alignments, steps, lengths, sps, "btk", timing_advance) if searched is None else \
            timings_of_path(searched, steps, lengths, sps)
        if pros is not None:
            spans = [_spans_at_rate(s, r) for s, r in zip(spans, pros.per_item(B)[0])]
        if plans is not None:
            spans = [s if p is None else _spans_under_plan(s, p[0], p[1], steps_per_frame * up, audio_cfg)
                     for s, p in zip(spans, plans)]
    out = []
    for b in range(B):
        n = int(frames[b])
        res = (mel[b, :n], linear[b, :n * up], alignments[b, :n // steps_per_frame, :lengths[b]],
               wavs[b, :int(samples[b])])
        if diagnostics:
            res += (stats[b],)
        if timings:
            res += (spans[b],)
        out.append(res)
    return out


class RollingSynthesizer(object):
    """Synthesis with rolling admission: `slots` decode slots that are refilled as utterances finish.

    The decoder's step program is built once in slot mode (Decoder.slot_program) and lives across utterances.  Between
    two chunks of `chunk` decoder steps, queued requests are admitted first in first out into the free slots: the
    encoder runs on the admitted group under ops.ItemLengths (the per-utterance path of synthesize_batch) and its
    outputs go into the slot rows.  After a chunk, every busy slot's own done flags are put to the reference's B = 1
    stop rule (decode_program.item_stops) at the slot's own step index; the slots that stopped are freed, and the
    retired group goes through the post-net under ItemLengths and ONE Griffin-Lim call with per-item frame counts.
    Everything runs on the current stream, admission and retirement included.  Inference only; a decoder the fused
    step kernels do not take is refused (no module-by-module fallback)."""

    def __init__(self, model, slots=64, max_text_len=256, audio_cfg=None, chunk=8, diagnostics=False, stall_limit=None,
                 timings=False, timing_advance=1, mastering=None, from_mel=False):
        """diagnostics: every retired result gains a last element, the utterance's alignment statistics (one device
        read per retired group); stall_limit: the end-of-text stop -- after every chunk one statistics call runs in
        place on the program's stacked alignment buffer over the busy slots, and a slot whose attention reached its
        last key stall_limit steps ago retires then, if its done flag has not retired it first.  An item's step count
        does not depend on the chunk size.  timings: every retired result gains one more element, after the statistics
        if they are there: the utterance's timing dict (token_timings with max_advance = timing_advance), searched in
        place on the program's stacked alignment buffer over the retiring slots.  from_mel (True or an
        audio.MelInverse): retirement vocodes the group's mel instead of running the post-net, as tts_batch does.
        mastering (an audio.Mastering): every retired `wav` is the mastered one, as tts_batch makes it.
        All off by default: no launch and no result changes."""
        self.mastering = audio.check_mastering(mastering, "RollingSynthesizer")
        if slots < 1 or max_text_len < 1 or chunk < 1:
            raise ValueError("RollingSynthesizer: slots, max_text_len and chunk must be positive")
        if stall_limit is not None and int(stall_limit) < 0:
            raise ValueError("RollingSynthesizer: stall_limit must be >= 0 (or None: off)")
        self.diagnostics, self.timings, self.timing_advance = bool(diagnostics), bool(timings), int(timing_advance)
        self.stall_limit = None if stall_limit is None else int(stall_limit)
        model.eval()
        self.model, self.audio_cfg = model, audio_cfg
        self.max_text_len = int(max_text_len)
        self.dec = model.seq2seq.decoder
        if not hasattr(self.dec, "slot_program"):
            raise RuntimeError("RollingSynthesizer: %r has no slot-mode step program" % type(self.dec))
        self.prog = self.dec.slot_program(slots, self.max_text_len)
        self.mel_options = mel_options(from_mel)
        if self.mel_options is None:
            check_linear_dim(model, audio_cfg, "RollingSynthesizer")     # retirement ends in Griffin-Lim on audio_cfg's framing
        self.schedule = RollingSchedule(slots, chunk)
        self.min_steps = int(self.dec.min_decoder_steps)
        self.max_steps = int(self.dec.max_decoder_steps)        # = the program's t_cap - 1
        self._req = {}
        self._next = 0

    def submit(self, ids, speaker_id=None, max_decoder_steps=None, rate=None, semitones=None, prosody=None, marks=None):
        """queue one utterance (a sequence of int ids) -> its ticket (0, 1, 2, ... in submission order).
        max_decoder_steps: this request's own cap (default and upper limit: the decoder's); rate, semitones (scalars),
        prosody (an audio.Prosody): how THIS utterance is spoken, as tts_batch takes them -- retirement gathers the
        group's values into its one Griffin-Lim call; marks (an audio.ProsodyMarks in tokens): THIS utterance's marks, as
        tts_batch takes them (not together with the other three)"""
        ids = [int(i) for i in ids]
        marks = utterance_marks(marks, rate, semitones, prosody, 1, "RollingSynthesizer.submit")
        if marks is not None:
            marks[0].half_width(self.audio_cfg), marks[0].ramp_frames(self.audio_cfg)        # refused here, not at retirement
        for name, v in (("rate", rate), ("semitones", semitones)):
            if v is not None and isinstance(v, (list, tuple, np.ndarray, torch.Tensor)):
                raise ValueError("RollingSynthesizer.submit: %s=%r must be one number: a ticket is one utterance" % (name, v))
        pros = utterance_prosody(rate, semitones, prosody, 1, "RollingSynthesizer.submit")
        if pros is not None:
            pros.half_width(self.audio_cfg)          # refused here, not when the utterance retires
        if len(ids) < 1:
            raise ValueError("RollingSynthesizer.submit: empty sequence")
        if len(ids) > self.max_text_len:
            raise ValueError("RollingSynthesizer.submit: %d ids, the slots hold max_text_len = %d" % (
                len(ids), self.max_text_len))
        cap = self.max_steps if max_decoder_steps is None else int(max_decoder_steps)
        if cap < 0 or cap > self.max_steps:
            raise ValueError("RollingSynthesizer.submit: max_decoder_steps %d outside [0, %d] (the decoder's own)" % (
                cap, self.max_steps))
        multi = getattr(self.model, "n_speakers", 1) > 1
        if multi != (speaker_id is not None):
            raise ValueError("RollingSynthesizer.submit: speaker_id is %s for a model of %d speakers" % (
                "missing" if multi else "given", getattr(self.model, "n_speakers", 1)))
        ticket = self._next
        self._next += 1
        self._req[ticket] = (ids, speaker_id, cap, pros, None if marks is None else marks[0])
        self.schedule.submit(ticket)
        return ticket

    def pending(self):
        return self.schedule.pending()

    def _speaker_embed(self, tickets, dev):
        if getattr(self.model, "n_speakers", 1) <= 1:
            return None
        spk = torch.tensor([int(self._req[t][1]) for t in tickets], dtype=torch.long).to(dev)
        return self.model.embed_speakers(spk)

    def _admit(self, admitted):
        from . import ops
        model = self.model
        dev = self.prog.dev
        tickets = [t for t, _ in admitted]
        seqs = [self._req[t][0] for t in tickets]
        lengths = [len(s) for s in seqs]
        n, Tt = len(seqs), max(lengths)
        pad = model.seq2seq.encoder.embed_tokens.padding_idx
        text = torch.full((n, Tt), 0 if pad is None else pad, dtype=torch.long)
        for b, s in enumerate(seqs):
            text[b, :len(s)] = torch.as_tensor(s, dtype=torch.long)
        text = text.to(dev)
        tl = torch.tensor(lengths, dtype=torch.int64)
        pos = torch.arange(1, Tt + 1, device=dev)[None, :].expand(n, Tt)
        text_positions = torch.where(pos <= tl.to(dev)[:, None], pos, torch.zeros_like(pos))
        prev, ops.valid = ops.valid, ops.ItemLengths(tl, Tt, dev)
        try:
            with torch.no_grad():
                se = self._speaker_embed(tickets, dev)
                memory = model.seq2seq.encoder(text, lengths=None, speaker_embed=se)
                self.prog.admit([s for _, s in admitted], memory, text_positions, tl, se)
        finally:
            ops.valid = prev

    def _retire(self, retired):
        """retired: [(ticket, slot, steps)] -> [(ticket, mel, linear, alignment, wav)] (+ the statistics dict)"""
        from . import ops
        model = self.model
        dev = self.prog.dev
        tickets = [t for t, _, _ in retired]
        steps = [n for _, _, n in retired]
        lengths = [len(self._req[t][0]) for t in tickets]
        G, Td = len(retired), max(steps)
        with torch.no_grad():
            outputs, alignments, states = self.prog.read_slots([s for _, s, _ in retired], steps)
            self.prog.release([s for _, s, _ in retired])
            mel = outputs.reshape(G, -1, model.mel_dim)
            r = mel.size(1) // Td
            frames = torch.tensor(steps, dtype=torch.int64) * r
            if self.mel_options is not None:        # vocode the mel: no post-net
                up = postnet_upsampling(model)
                linear = audio.mel_to_linear(mel, self.audio_cfg, frames, up, self.mel_options)
            else:
                post_in = states.view(G, mel.size(1), -1) if model.use_decoder_state_for_postnet_input else mel
                vl = ops.ItemLengths(lengths, max(lengths), dev)
                vl.set_dec(steps, Td)
                prev, ops.valid = ops.valid, vl
                try:
                    linear = model.postnet(post_in, self._speaker_embed(tickets, dev)).contiguous()
                    ops.zero_frames(linear, vl.dec_len, min(steps), linear.size(1) // Td)
                finally:
                    ops.valid = prev
                up = linear.size(1) // mel.size(1)
            settings = [self._req[t][3] for t in tickets]
            marks = [self._req[t][4] for t in tickets]
            searched = plans = None
            if any(m is not None for m in marks):
                searched = search_path(alignments, steps, lengths, "btk", self.timing_advance)
                wavs, samples, plans = _vocode_marked(linear, self.audio_cfg, frames * up, settings, marks, searched, r * up,
                                                      "RollingSynthesizer (tickets %s)" % (tickets,))
            else:
                wavs, samples = _vocode(linear, self.audio_cfg, frames * up, settings)
            if self.mastering is not None:
                wavs = audio.master_items(wavs, samples, self.mastering,
                                          (self.audio_cfg or audio.AudioConfig()).sample_rate)
        stats = None
        if self.diagnostics:
            stats = _diagnose(alignments, steps, lengths, [self._req[t][2] for t in tickets])
        spans = None
        if self.timings:            # a released slot's stacked rows stay as they are until it is admitted again
            sps = seconds_per_step(self.audio_cfg, r, up)
            spans = self._timings(retired, lengths, alignments, sps) if searched is None else \
                timings_of_path(searched, steps, lengths, sps)
            spans = [s if p is None else _spans_at_rate(s, p.rate[0]) for s, p in zip(spans, settings)]
            if plans is not None:
                spans = [s if p is None else _spans_under_plan(s, p[0], p[1], r * up, self.audio_cfg)
                         for s, p in zip(spans, plans)]
        out = []
        for b, t in enumerate(tickets):
            n = int(frames[b])
            res = (t, mel[b, :n], linear[b, :n * up], alignments[b, :steps[b], :lengths[b]], wavs[b, :int(samples[b])])
            if self.diagnostics:
                res += (stats[b],)
            if self.timings:
                res += (spans[b],)
            out.append(res)
            del self._req[t]
        return out

    def _timings(self, retired, lengths, alignments, sps):
        """the timing dicts of a retiring group, in its order.  The search reads the program's stacked (t_cap, slots, Tk)
        buffer in place ("tbk") with zero steps for every slot that is not retiring; a program whose stored rows carry
        a scale (align_scale != 1: they are not the probabilities the results hold) is searched on the group's scaled
        copy instead, so that either way the dict is that of the returned alignment."""
        prog = self.prog
        steps = [n for _, _, n in retired]
        if prog.align_scale != 1.0:
            return token_timings(alignments, steps, lengths, sps, "btk", self.timing_advance)
        ran, keys = [0] * prog.B, [1] * prog.B
        for (_, s, n), k in zip(retired, lengths):
            ran[s], keys[s] = n, k
        rows = token_timings(prog.aligns, ran, keys, sps, "tbk", self.timing_advance)
        return [rows[s] for _, s, _ in retired]

    def poll(self):
        """one round: admit what fits, run one chunk of decoder steps, retire what stopped
        -> a list of (ticket, mel (T, mel_dim), linear (T * upsampling, linear_dim), alignment (steps, Tt), wav (L,)),
        each as tts_batch returns an utterance; empty when nothing retired (or nothing is pending)"""
        sch = self.schedule
        admitted = sch.admit()
        if admitted:
            self._admit(admitted)
        busy = sch.busy()
        if not busy:
            return []
        n = sch.advance()
        self.prog.run_steps(n)
        flags = self.prog.done_flags()
        stall = None
        if self.stall_limit is not None:
            ran = [0] * sch.n_slots
            for s in busy:
                ran[s] = min(sch.steps_run(s), self.prog.t_cap)
            stall = end_of_text_stops(self.prog.aligns, "tbk", ran, self.prog.key_len, self.stall_limit, self.min_steps)
        retired = []
        for s in busy:
            t1 = sch.steps_run(s)
            t0 = t1 - n
            rows = [[flags[t][s]] for t in range(t0, min(t1, self.prog.t_cap))]
            stop = [0]
            item_stops(rows, t0, self.min_steps, self._req[sch.slot_ticket[s]][2], stop)
            if stall is not None and stall[s] and (stop[0] == 0 or stall[s] < stop[0]):
                stop[0] = stall[s]
            if stop[0]:
                retired.append((sch.retire(s), s, stop[0]))
        return self._retire(retired) if retired else []

    def drain(self):
        """poll until the queue and the slots are empty"""
        while self.schedule.pending():
            for res in self.poll():
                yield res


def tts_stream(model, sequences, speaker_ids=None, slots=64, max_text_len=None, audio_cfg=None, chunk=8,
               max_decoder_steps=None, diagnostics=False, stall_limit=None, timings=False, timing_advance=1,
               rate=None, semitones=None, prosody=None, marks=None, mastering=None, durations=None, from_mel=False):
    """Rolling-admission counterpart of tts_batch, as a generator: sequences (any iterable of id lists; speaker_ids an
    iterable alongside, or None; max_decoder_steps None, one cap, or an iterable of per-utterance caps) are submitted
    in order as slots free -- at most `slots` are queued ahead -- and every utterance is yielded when it retires, in
    COMPLETION order: (index in `sequences`, mel, linear, alignment, wav), the entries as tts_batch returns them.
    max_text_len None: the longest sequence (the iterable is then read up front).  diagnostics, stall_limit: as
    RollingSynthesizer takes them (a last element per result; the end-of-text stop); timings, timing_advance: as there
    (one more element per result, the utterance's timing dict); from_mel: as tts_batch takes it (the mel is vocoded, the
    post-net is not run); rate, semitones: None, one number, or an iterable of per-utterance values alongside
    `sequences`; prosody: an audio.Prosody carrying the envelope settings (RollingSynthesizer.submit takes all three);
    mastering: an audio.Mastering, as tts_batch takes it; marks: None or an iterable alongside `sequences` of one
    audio.ProsodyMarks in tokens (or None) per utterance, each handed to its submit.  durations: refused -- a guided
    decode (tts_batch(durations=...)) does not run in slot mode."""
    if durations is not None:
        raise ValueError("tts_stream: durations are not taken: rolling admission decodes in slot mode, where every slot "
                         "runs at its own step, and the guided attention kernel has one step axis for the batch; use "
                         "tts_batch(durations=...)")
    if max_text_len is None:
        sequences = [list(s) for s in sequences]
        if not sequences:
            return
        max_text_len = max(len(s) for s in sequences)
    rs = RollingSynthesizer(model, slots=slots, max_text_len=max_text_len, audio_cfg=audio_cfg, chunk=chunk,
                            diagnostics=diagnostics, stall_limit=stall_limit, timings=timings,
                            timing_advance=timing_advance, from_mel=from_mel, mastering=mastering)
    it = iter(sequences)
    spk = iter(speaker_ids) if speaker_ids is not None else None
    caps = None
    if max_decoder_steps is not None and not isinstance(max_decoder_steps, int):
        caps = iter(max_decoder_steps)
    number = lambda v: v is None or isinstance(v, (int, float, np.integer, np.floating))
    rates = None if number(rate) else iter(rate)
    shifts = None if number(semitones) else iter(semitones)
    if isinstance(marks, audio.ProsodyMarks):
        raise ValueError("tts_stream: marks must be an iterable of one audio.ProsodyMarks (or None) per utterance")
    each = None if marks is None else iter(marks)
    more = True
    while more or rs.pending():
        while more and len(rs.schedule.queue) < slots:
            try:
                ids = next(it)
            except StopIteration:
                more = False
                break
            rs.submit(ids, next(spk) if spk is not None else None,
                      next(caps) if caps is not None else max_decoder_steps,
                      rate=float(next(rates)) if rates is not None else rate,
                      semitones=float(next(shifts)) if shifts is not None else semitones, prosody=prosody,
                      marks=next(each) if each is not None else None)
        for res in rs.poll():
            yield res


# ----------------------------------------------------------------------------------------------------------------------
# deliverable audio: a document of several utterances
# ----------------------------------------------------------------------------------------------------------------------
def plan_document(lengths, sample_rate, pauses=0.25, fade_samples=0, starts=None, lead=0.0, tail=0.0):
    """Where every sentence of a document goes -- a pure host function.  lengths: the S sentences' samples; pauses: seconds
    of silence between neighbours, one number or S - 1 of them (rounded to samples, halves up); fade_samples: F; starts:
    each sentence's first sample in the source buffer (None: back to back); lead, tail: seconds of silence before the
    first and after the last sentence.  -> (table, N): table a dict of arrays "src", "len", "dst" (int64) and "flags"
    (int32: bit 0 fade-in, bit 1 fade-out), what audio.wave_master takes, and N the document's samples.
      * a sentence of at least F samples fades in and out (flags 3): at the document's edges, into and out of every
        pause, and across a pause of 0, where the next sentence starts F samples before this one ends -- the crossfade;
      * a sentence shorter than F gets no fade (flags 0), and a join it takes part in is a plain butt join;
      * a pause of 0 is also a butt join (both fades kept, no overlap) where the crossfade would put a third sentence
        over a sample: the next sentence never starts before the one before this one has ended."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    S, F, sr = lengths.size, int(fade_samples), float(sample_rate)
    if S < 1 or int(lengths.min()) < 0:
        raise ValueError("plan_document: at least one sentence of >= 0 samples expected, got %s" % (lengths.tolist(),))
    if not sr > 0 or F < 0 or F != fade_samples:
        raise ValueError("plan_document: sample_rate=%r must be positive and fade_samples=%r a non-negative integer"
                         % (sample_rate, fade_samples))
    gaps = np.broadcast_to(np.asarray(pauses, dtype=np.float64), (S - 1,)) if np.ndim(pauses) == 0 else \
        np.asarray(pauses, dtype=np.float64).reshape(-1)
    if gaps.size != S - 1 or not np.all(gaps >= 0) or not np.all(np.isfinite(gaps)):
        raise ValueError("plan_document: pauses=%r must be one number or %d of them, each >= 0 seconds" % (pauses, S - 1))
    if not (0 <= float(lead) < float("inf") and 0 <= float(tail) < float("inf")):
        raise ValueError("plan_document: lead=%r and tail=%r must be >= 0 seconds" % (lead, tail))
    to_samples = lambda sec: int(np.floor(float(sec) * sr + 0.5))
    if starts is None:
        src = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    else:
        src = np.asarray(starts, dtype=np.int64).reshape(-1)
        if src.size != S or (S and int(src.min()) < 0):
            raise ValueError("plan_document: %d starts for %d sentences" % (src.size, S))
    faded = (lengths >= F) & (lengths > 0) & (F > 0)
    dst = np.zeros(S, dtype=np.int64)
    dst[0] = to_samples(lead)
    for k in range(1, S):
        end, gap = int(dst[k - 1] + lengths[k - 1]), to_samples(gaps[k - 1])
        before = int(dst[k - 2] + lengths[k - 2]) if k >= 2 else 0
        cross = gap == 0 and faded[k - 1] and faded[k] and end - F >= before
        dst[k] = end - F if cross else end + gap
    N = int(dst[-1] + lengths[-1]) + to_samples(tail)
    return {"src": src, "len": lengths.copy(), "dst": dst, "flags": np.where(faded, 3, 0).astype(np.int32)}, N


def join_utterances(wavs, sample_rate, pauses=0.25, trim_db=40.0, mastering=None, lead=0.0, tail=0.0, return_plan=False):
    """One document from a list of 1-D float32 device waveforms (tts_batch's `wav` elements, say).  trim_db: silence at
    each utterance's edges is cut by audio.trim_items at that threshold (None: nothing is cut; an utterance under 1025
    samples comes back untrimmed, as trim_items leaves it); mastering: an audio.Mastering (None:
    Mastering("peak", scope="document")) -- its level and scope give every utterance's gain from audio.wave_levels of
    the TRIMMED spans, its fade_ms the fades, its dtype and dither the output; pauses, lead, tail: plan_document's.
    Trim, levels, gains, the plan and ONE master launch (audio.wave_master); exactly one host read -- the trimmed spans,
    which size the output (none when trim_db is None).  -> (the document (N,), [(start, end) of every utterance in
    seconds]); return_plan: a third element, plan_document's table with "N" and "starts" (each utterance's first sample
    in the packed source, before trimming) added.  The defaults of trim_db, pauses and the Mastering are starting
    points, not measurements: nothing here was heard on a trained voice."""
    mastering = audio.check_mastering(mastering, "join_utterances") or audio.Mastering("peak", scope="document")
    if len(wavs) == 0:
        raise ValueError("join_utterances: no waveforms")
    for w in wavs:
        if not torch.is_tensor(w) or not w.is_cuda or w.dim() != 1 or w.dtype != torch.float32:
            raise ValueError("join_utterances: 1-D float32 device tensors expected")
    lengths = np.array([int(w.numel()) for w in wavs], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    if int(lengths.sum()) == 0:
        raise ValueError("join_utterances: every waveform is empty")
    flat = torch.cat(list(wavs))
    if trim_db is not None:
        t_starts, t_lens = audio.trim_items(flat, starts, lengths, trim_db)
        host = torch.stack([t_starts, t_lens]).cpu().numpy()                  # the one host read
        src, lens = host[0].astype(np.int64), host[1].astype(np.int64)
    else:
        src, lens = starts.copy(), lengths.copy()
    F = mastering.fade_samples(sample_rate)
    table, N = plan_document(lens, sample_rate, pauses, F, starts=src, lead=lead, tail=tail)
    gain = None
    if mastering.level is not None or mastering.limiter is not None:
        sl = torch.from_numpy(np.concatenate([src, lens])).to(flat.device, non_blocking=True)
        S = src.size
        flat, gain = audio.master_source(flat, sl[:S], sl[S:], int(lens.max()), mastering, sample_rate)
    doc = audio.wave_master(flat, table["src"], table["len"], table["dst"], gain, table["flags"], N, F, mastering.dtype,
                            mastering.level == "reference", mastering.dither, mastering.seed)
    sr = float(sample_rate)
    spans = [(float(d) / sr, float(d + n) / sr) for d, n in zip(table["dst"], table["len"])]
    if return_plan:
        table = dict(table, N=N, starts=starts)
        return doc, spans, table
    return doc, spans


def tts_document(model, sentences, speaker_id=None, batch=64, timings=False, audio_cfg=None, timing_advance=1,
                 stall_limit=None, **join_options):
    """Speak a text longer than one utterance: sentences (a list of int id sequences, each within the model's
    max_positions) go through tts_batch in groups of at most `batch` (speaker_id: None or one id for the whole
    document), then through join_utterances(wavs, audio_cfg.sample_rate, **join_options) -- pauses, trim_db, mastering,
    lead, tail.  -> (document (N,), [(start, end) of every sentence in seconds]); timings=True: a third element, per
    sentence its timing dict (token_timings) with "start" and "end" moved onto the document's time axis: plus the
    sentence's first output sample minus the samples trimmed off its front, over the sample rate."""
    sentences = [list(s) for s in sentences]
    if len(sentences) == 0:
        raise ValueError("tts_document: no sentences")
    if int(batch) < 1:
        raise ValueError("tts_document: batch=%r must be positive" % (batch,))
    cfg = audio_cfg or audio.AudioConfig()
    wavs, spans = [], []
    for i in range(0, len(sentences), int(batch)):
        group = sentences[i:i + int(batch)]
        res = tts_batch(model, group, None if speaker_id is None else [speaker_id] * len(group), audio_cfg,
                        stall_limit=stall_limit, timings=timings, timing_advance=timing_advance)
        wavs += [r[3] for r in res]
        spans += [r[4] for r in res] if timings else []
    doc, where, plan = join_utterances(wavs, cfg.sample_rate, return_plan=True, **join_options)
    if not timings:
        return doc, where
    sr = float(cfg.sample_rate)
    out = []
    for k, span in enumerate(spans):
        shift = float(int(plan["dst"][k]) - (int(plan["src"][k]) - int(plan["starts"][k]))) / sr
        moved = dict(span)
        moved["start"], moved["end"] = span["start"] + shift, span["end"] + shift
        out.append(moved)
    return doc, where, out


# ----------------------------------------------------------------------------------------------------------------------
# free-running evaluation: mel-cepstral distortion along a DTW path, and the duration ratio
# ----------------------------------------------------------------------------------------------------------------------
SYNTH_EVAL_COLUMNS = ("mcd_sum", "path_len", "n_diag", "n_synth_only", "n_target_only", "frames_synth", "frames_target")


def mel_distortion(mel_a, len_a, mel_b, len_b, cfg=None, order=13, want_path=False):
    """Mel-cepstral distortion of two padded batches of normalised mel spectrograms along their DTW paths.
    mel_a (B, Ta, M), mel_b (B, Tb, M) fp32 on the device; len_a, len_b: each item's frames (ints or an int tensor;
    the frames past them are never read and may hold anything).  The features are audio.mel_cepstra -- cepstra of the
    mel spectrogram, c0 left out, scaled so that a frame pair's Euclidean distance is its distortion in dB --, ONE
    matmul over the frames of both batches (equal frames get equal features whichever batch holds them); the alignment is
    ops.dtw.  -> (B, 7) fp32 on the device, columns SYNTH_EVAL_COLUMNS: mcd_sum is the distortion summed over the
    path (dB), so mcd_sum / path_len is the utterance's MCD; with want_path also the (B, Ta + Tb - 1, 2) int32 paths,
    rows (frame of a, frame of b).  No host synchronisation."""
    from . import ops
    if mel_a.dim() != 3 or mel_b.dim() != 3 or mel_a.shape[0] != mel_b.shape[0] or mel_a.shape[2] != mel_b.shape[2]:
        raise ValueError("mel_distortion: (B, Ta, M) and (B, Tb, M), got %s and %s" % (tuple(mel_a.shape), tuple(mel_b.shape)))
    dev = mel_a.device
    (B, Ta, M), Tb = mel_a.shape, mel_b.shape[1]

    def lengths(v, T, name):
        v = torch.as_tensor(v).reshape(-1).to(device=dev, dtype=torch.int32)
        if v.numel() != B:
            raise ValueError("mel_distortion: %d %s for %d items" % (v.numel(), name, B))
        return v.clamp(0, T)

    la, lb = lengths(len_a, Ta, "len_a"), lengths(len_b, Tb, "len_b")
    rows = torch.cat([mel_a.reshape(B * Ta, M).to(torch.float32), mel_b.reshape(B * Tb, M).to(torch.float32)])
    feats = audio.mel_cepstra(rows, cfg, order)
    fa, fb = feats[:B * Ta].view(B, Ta, -1), feats[B * Ta:].view(B, Tb, -1)
    res = ops.dtw(fa, fb, la, lb, want_path=want_path)
    out = res[0] if want_path else res
    table = torch.cat([out, la.to(torch.float32)[:, None], lb.to(torch.float32)[:, None]], dim=1)
    return (table, res[1]) if want_path else table


def evaluate_synthesis(model, sequences, target_mels, speaker_ids=None, downsample_step=4, audio_cfg=None, order=13,
                       diagnostics=False, stall_limit=None):
    """How far is the model's own (free-running) synthesis of held-out sentences from their recordings?
    sequences: a list of int id sequences; target_mels: per utterance the recording's normalised mel (T_b, mel_dim) at
    the dataset's frame rate (tensor or array), downsampled here as the collate does it, mel[::downsample_step].
    Decodes with model.synthesize_batch (no Griffin-Lim: no waveform is needed) and runs mel_distortion(synthesised,
    target) on the device.  -> the (B, 7) table (SYNTH_EVAL_COLUMNS; feed it to SynthEvalTotals); with diagnostics
    (table, rows): per utterance the alignment statistics dict with its "flags", as tts_batch returns it.
    stall_limit: the end-of-text stop of synthesize_batch."""
    B = len(sequences)
    if B == 0 or len(target_mels) != B:
        raise ValueError("evaluate_synthesis: %d sequences and %d targets" % (B, len(target_mels)))
    dev = next(model.parameters()).device
    lengths = [len(s) for s in sequences]
    if min(lengths) < 1:
        raise ValueError("evaluate_synthesis: empty sequence")
    ds = int(downsample_step)
    if ds < 1:
        raise ValueError("evaluate_synthesis: downsample_step = %d < 1" % ds)
    pad = model.seq2seq.encoder.embed_tokens.padding_idx
    text = torch.full((B, max(lengths)), 0 if pad is None else pad, dtype=torch.long)
    for b, s in enumerate(sequences):
        text[b, :len(s)] = torch.as_tensor(s, dtype=torch.long)
    spk = None
    if speaker_ids is not None:
        spk = torch.as_tensor(speaker_ids, dtype=torch.long).reshape(-1).to(dev)
    targets = [torch.as_tensor(t)[::ds] for t in target_mels]
    for b, t in enumerate(targets):
        if t.dim() != 2 or t.shape[1] != model.mel_dim or t.shape[0] < 1:
            raise ValueError("evaluate_synthesis: target %d of shape %s, expected (T >= 1, %d)" % (
                b, tuple(torch.as_tensor(target_mels[b]).shape), model.mel_dim))
    frames_t = [int(t.shape[0]) for t in targets]
    tgt = torch.zeros(B, max(frames_t), model.mel_dim, dtype=torch.float32, device=dev)
    for b, t in enumerate(targets):
        tgt[b, :frames_t[b]] = t.to(device=dev, dtype=torch.float32)
    model.eval()
    mel, _, alignments, _, frames = model.synthesize_batch(text.to(dev), lengths, spk, stall_limit=stall_limit)
    with torch.no_grad():
        table = mel_distortion(mel, frames, tgt, frames_t, audio_cfg, order)
    if not diagnostics:
        return table
    r = mel.size(1) // alignments.size(1)
    rows = _diagnose(alignments, [int(n) // r for n in frames], lengths, [model.seq2seq.decoder.max_decoder_steps] * B)
    return table, rows


class SynthEvalTotals(object):
    """Accumulates evaluate_synthesis / mel_distortion tables over a held-out set (modelled on train_step.EvalTotals).
    add() keeps tensors and does not synchronise with the host; result() makes one transfer and sums in float64, in
    the order the rows were added.  The set-level figures are sums over sums, so they are the same however the set was
    cut into batches:
        mcd             sum mcd_sum / sum path_len           (dB per aligned frame pair)
        duration_ratio  sum frames_synth / sum frames_target
        n_items, and items: one dict per utterance in the order added -- its columns, "mcd" and "duration_ratio" of its
        own, and "id" when ids were given -- so utterances can be ranked."""

    def __init__(self):
        self._tables, self.ids = [], None

    def add(self, table, ids=None):
        table = table.detach()
        if table.dim() != 2 or table.shape[1] != len(SYNTH_EVAL_COLUMNS):
            raise ValueError("SynthEvalTotals.add: a table of shape %s, expected (B, %d)" % (
                tuple(table.shape), len(SYNTH_EVAL_COLUMNS)))
        n = int(table.shape[0])
        if (ids is not None) != (self.ids is not None) and self._tables:
            raise ValueError("SynthEvalTotals.add: ids for every batch or for none")
        if ids is not None:
            ids = list(ids)
            if len(ids) != n:
                raise ValueError("SynthEvalTotals.add: %d ids for %d items" % (len(ids), n))
            self.ids = (self.ids or []) + ids
        self._tables.append(table.to(torch.float32))

    def result(self):
        if not self._tables:
            raise ValueError("SynthEvalTotals.result: nothing was added")
        rows = torch.cat([t.cpu() for t in self._tables]).double()
        col = {name: rows[:, i] for i, name in enumerate(SYNTH_EVAL_COLUMNS)}
        tot = {name: float(sum(col[name].tolist())) for name in SYNTH_EVAL_COLUMNS}      # one order: the rows' own
        out = {"n_items": int(rows.shape[0])}
        out.update(tot)
        out["mcd"] = tot["mcd_sum"] / tot["path_len"] if tot["path_len"] > 0 else float("nan")
        out["duration_ratio"] = tot["frames_synth"] / tot["frames_target"] if tot["frames_target"] > 0 else float("nan")
        items = []
        for b, vals in enumerate(rows.tolist()):
            it = {k: (v if k == "mcd_sum" else int(v)) for k, v in zip(SYNTH_EVAL_COLUMNS, vals)}
            it["mcd"] = it["mcd_sum"] / it["path_len"] if it["path_len"] > 0 else float("nan")
            it["duration_ratio"] = it["frames_synth"] / it["frames_target"] if it["frames_target"] > 0 else float("nan")
            if self.ids is not None:
                it["id"] = self.ids[b]
            items.append(it)
        out["items"] = items
        return out


# ----------------------------------------------------------------------------------------------------------------------
# waveform-level evaluation: F0 and voicing error along the same DTW path as the distortion
# ----------------------------------------------------------------------------------------------------------------------
PITCH_EVAL_COLUMNS = ("f0_sqcents_sum", "n_both_voiced", "n_voicing_errors", "pitch_path_len", "n_voiced_a", "n_voiced_b")
WAVE_EVAL_COLUMNS = SYNTH_EVAL_COLUMNS + PITCH_EVAL_COLUMNS


def pitch_distortion(f0_a, voiced_a, f0_b, voiced_b, path):
    """F0 and voicing disagreement of two padded batches of pitch tracks along given alignment paths.
    f0_a (B, Ta), f0_b (B, Tb): Hz (audio.yin_items, padded); voiced_a, voiced_b: bool, same shapes (audio.voiced; False
    in the padding); path (B, Ta + Tb - 1, 2) int32 as ops.dtw / mel_distortion(want_path=True) return it: rows (frame
    of a, frame of b), rows of -1 past the path's end are skipped.  -> (B, 6) fp32, columns PITCH_EVAL_COLUMNS, over the
    path's pairs: f0_sqcents_sum = sum of (1200 log2(f0_a / f0_b))^2 over the pairs voiced on both sides and
    n_both_voiced their count (so sqrt of the ratio is the RMSE in cents); n_voicing_errors the pairs voiced on one side
    only; pitch_path_len the pairs; n_voiced_a / n_voiced_b each side's voiced frames inside its length (the path's last
    row + 1).  The squares are summed in float64 and rounded once.  Any device; no host synchronisation."""
    if f0_a.dim() != 2 or f0_b.dim() != 2 or f0_a.shape != voiced_a.shape or f0_b.shape != voiced_b.shape or \
            path.dim() != 3 or path.shape[0] != f0_a.shape[0] or f0_b.shape[0] != f0_a.shape[0] or path.shape[2] != 2:
        raise ValueError("pitch_distortion: (B, Ta), (B, Tb) tracks with flags of the same shapes and a (B, P, 2) path, got "
                         "%s / %s, %s / %s and %s" % (tuple(f0_a.shape), tuple(voiced_a.shape), tuple(f0_b.shape),
                                                      tuple(voiced_b.shape), tuple(path.shape)))
    (B, Ta), Tb = f0_a.shape, f0_b.shape[1]
    pi, pj = path[..., 0].long(), path[..., 1].long()
    on = (pi >= 0) & (pj >= 0)
    ia, ib = pi.clamp(0, Ta - 1), pj.clamp(0, Tb - 1)
    va, vb = voiced_a.bool().gather(1, ia) & on, voiced_b.bool().gather(1, ib) & on
    both = va & vb
    fa = torch.where(both, f0_a.gather(1, ia), torch.ones_like(ia, dtype=f0_a.dtype)).double()
    fb = torch.where(both, f0_b.gather(1, ib), torch.ones_like(ib, dtype=f0_b.dtype)).double()
    cents = 1200.0 * torch.log2(fa / fb)
    la, lb = pi.max(dim=1).values + 1, pj.max(dim=1).values + 1
    inside = lambda v, n: (v.bool() & (torch.arange(v.shape[1], device=v.device)[None, :] < n[:, None])).sum(1)
    cols = [(cents * cents).sum(1), both.sum(1), (va != vb).sum(1), on.sum(1), inside(voiced_a, la), inside(voiced_b, lb)]
    return torch.stack([c.double() for c in cols], dim=1).to(torch.float32)


def _pack_any(wavs, device, what):
    """a list of 1-D waveforms (host arrays, or tensors on any device) -> (flat float32 tensor on `device`, lengths)"""
    if len(wavs) == 0:
        raise ValueError("%s: no waveforms" % what)
    if all(isinstance(w, torch.Tensor) for w in wavs):
        lengths = np.array([int(w.numel()) for w in wavs], dtype=np.int64)
        return torch.cat([w.detach().reshape(-1).to(device=device, dtype=torch.float32) for w in wavs]), lengths
    flat, lengths = audio.pack_waveforms([np.asarray(w.detach().cpu() if isinstance(w, torch.Tensor) else w,
                                                     dtype=np.float32).reshape(-1) for w in wavs])
    return flat.to(device, non_blocking=True), lengths


def _pad_rows(rows, frames, fill=0):
    """packed rows (sum T_b, ...) -> (B, max T_b, ...), item b's rows first, `fill` behind them"""
    out = rows.new_full((len(frames), int(max(frames))) + tuple(rows.shape[1:]), fill)
    o = 0
    for b, n in enumerate(int(n) for n in frames):
        out[b, :n] = rows[o:o + n]
        o += n
    return out


def waveform_distortion(wavs_a, wavs_b, cfg=None, pitch=None, order=13, device="cuda:0", num_mels=80, fmin=125, fmax=7600):
    """Objective comparison of two lists of waveforms, utterance b of one against utterance b of the other (lists of 1-D
    host arrays or tensors): both sides go through audio.features_items -- the same analysis for both --, the mel rows
    through mel_distortion at the full frame rate, and audio.yin_items' pitch tracks through pitch_distortion along that
    same DTW path.  -> (B, 13) fp32 on the device, columns WAVE_EVAL_COLUMNS (feed it to WaveEvalTotals); "synth" in the
    column names is side a, "target" side b.  cfg: the AudioConfig of the analysis; pitch: an audio.PitchConfig; num_mels,
    fmin, fmax: the mel filterbank.  An item of more than DV3_DTW_MAX_T frames is refused."""
    from . import _lib
    cfg = cfg or audio.AudioConfig()
    pitch = pitch if pitch is not None else audio.PitchConfig()
    if len(wavs_a) != len(wavs_b) or len(wavs_a) == 0:
        raise ValueError("waveform_distortion: %d and %d waveforms" % (len(wavs_a), len(wavs_b)))
    top = _lib.CONSTS["DV3_DTW_MAX_T"]
    sides = []
    for name, wavs in (("a", wavs_a), ("b", wavs_b)):
        flat, lengths = _pack_any(wavs, device, "waveform_distortion")
        if int(lengths.min()) < 1:
            raise ValueError("waveform_distortion: side %s holds an empty waveform (lengths %s)" % (name, lengths.tolist()))
        frames = [audio.lws_num_frames(int(n), cfg.hop_size, cfg.fft_size) for n in lengths]
        if max(frames) > top:
            b = int(np.argmax(frames))
            raise ValueError("waveform_distortion: item %d of side %s has %d frames (%d samples at hop %d), at most %d "
                             "(DV3_DTW_MAX_T)" % (b, name, frames[b], int(lengths[b]), cfg.hop_size, top))
        with torch.no_grad():
            _, mel, frames = audio.features_items(flat, lengths, cfg, num_mels, fmin, fmax)
            f0, ap, power, _ = audio.yin_items(flat, lengths, cfg, pitch)
            sides.append((_pad_rows(mel, frames), _pad_rows(f0, frames, 1.0),
                          _pad_rows(audio.voiced(ap, power, pitch), frames, False), [int(n) for n in frames]))
    (mel_a, f0_a, v_a, n_a), (mel_b, f0_b, v_b, n_b) = sides
    with torch.no_grad():
        table, path = mel_distortion(mel_a, n_a, mel_b, n_b, cfg, order, want_path=True)
        return torch.cat([table, pitch_distortion(f0_a, v_a, f0_b, v_b, path)], dim=1)


def evaluate_synthesis_audio(model, sequences, target_wavs, speaker_ids=None, audio_cfg=None, pitch=None, order=13):
    """evaluate_synthesis at the waveform: synthesises `sequences` with tts_batch under audio_cfg -- so the vocoder options
    under test (iterations, momentum, starting phase) apply -- and compares each waveform with its recording in
    target_wavs (1-D arrays or tensors at audio_cfg.sample_rate) by waveform_distortion(synthesised, target).
    -> the (B, 13) table, columns WAVE_EVAL_COLUMNS."""
    B = len(sequences)
    if B == 0 or len(target_wavs) != B:
        raise ValueError("evaluate_synthesis_audio: %d sequences and %d targets" % (B, len(target_wavs)))
    dev = next(model.parameters()).device
    res = tts_batch(model, sequences, speaker_ids, audio_cfg)
    return waveform_distortion([r[3] for r in res], list(target_wavs), audio_cfg, pitch, order, device=dev)


class WaveEvalTotals(object):
    """Accumulates waveform_distortion / evaluate_synthesis_audio tables over a held-out set, as SynthEvalTotals does for
    the mel tables: add() keeps tensors and does not synchronise; result() makes one transfer and sums in float64 in the
    order the rows were added, so every figure is the same however the set was cut into batches:
        mcd             sum mcd_sum / sum path_len                        (dB per aligned frame pair)
        duration_ratio  sum frames_synth / sum frames_target
        f0_rmse_cents   sqrt(sum f0_sqcents_sum / sum n_both_voiced)      (NaN when no pair is voiced on both sides)
        vuv_error       sum n_voicing_errors / sum pitch_path_len
        n_items, and items: one dict per utterance in the order added -- its columns, the four figures of its own, and
        "id" when ids were given."""

    def __init__(self):
        self._tables, self.ids = [], None

    def add(self, table, ids=None):
        table = table.detach()
        if table.dim() != 2 or table.shape[1] != len(WAVE_EVAL_COLUMNS):
            raise ValueError("WaveEvalTotals.add: a table of shape %s, expected (B, %d)" % (
                tuple(table.shape), len(WAVE_EVAL_COLUMNS)))
        n = int(table.shape[0])
        if (ids is not None) != (self.ids is not None) and self._tables:
            raise ValueError("WaveEvalTotals.add: ids for every batch or for none")
        if ids is not None:
            ids = list(ids)
            if len(ids) != n:
                raise ValueError("WaveEvalTotals.add: %d ids for %d items" % (len(ids), n))
            self.ids = (self.ids or []) + ids
        self._tables.append(table.to(torch.float32))

    @staticmethod
    def _figures(v):
        ratio = lambda a, b: v[a] / v[b] if v[b] > 0 else float("nan")
        return {"mcd": ratio("mcd_sum", "path_len"), "duration_ratio": ratio("frames_synth", "frames_target"),
                "f0_rmse_cents": ratio("f0_sqcents_sum", "n_both_voiced") ** 0.5,
                "vuv_error": ratio("n_voicing_errors", "pitch_path_len")}

    def result(self):
        if not self._tables:
            raise ValueError("WaveEvalTotals.result: nothing was added")
        rows = torch.cat([t.cpu() for t in self._tables]).double()
        tot = {name: float(sum(rows[:, i].tolist())) for i, name in enumerate(WAVE_EVAL_COLUMNS)}   # the rows' own order
        out = {"n_items": int(rows.shape[0])}
        out.update(tot)
        out.update(self._figures(tot))
        items = []
        for b, vals in enumerate(rows.tolist()):
            it = {k: (v if k in ("mcd_sum", "f0_sqcents_sum") else int(v)) for k, v in zip(WAVE_EVAL_COLUMNS, vals)}
            it.update(self._figures(it))
            if self.ids is not None:
                it["id"] = self.ids[b]
            items.append(it)
        out["items"] = items
        return out
