# coding: utf-8
"""Batched synthesis of different utterances (the batched counterpart of the reference's synthesis.tts,
synthesis.py:42-73, without its text frontend): every utterance comes back as if it had been synthesised alone.

    from deepvoice3_pytorch_amd import synthesis
    for mel, linear, alignment, wav in synthesis.tts_batch(model, [seq0, seq1, ...]):
        ...

The model part is MultiSpeakerTTSModel.synthesize_batch (per-utterance attention, stop and zero tails on the HIP
kernels); the waveforms are ONE batched Griffin-Lim call with per-item frame counts (audio.inv_spectrogram_batch(...,
frame_lengths=)), each item equal to the inverse of its own trimmed spectrogram.
"""
import torch

from . import audio


def tts_batch(model, sequences, speaker_ids=None, audio_cfg=None):
    """sequences: a list of int id sequences (one per utterance); speaker_ids: None or one id per utterance.
    -> a list of (mel (T_b, mel_dim), linear (T_b * upsampling, linear_dim), alignment (steps_b, Tt_b), wav (L_b,)),
    device tensors, each trimmed to its own utterance."""
    if len(sequences) == 0:
        return []
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
    mel, linear, alignments, _, frames = model.synthesize_batch(text, lengths, spk)
    up = linear.size(1) // mel.size(1)
    steps_per_frame = mel.size(1) // alignments.size(1)        # r
    with torch.no_grad():
        wavs, samples = audio.inv_spectrogram_batch(linear, audio_cfg, frame_lengths=frames * up)
    out = []
    for b in range(B):
        n = int(frames[b])
        out.append((mel[b, :n], linear[b, :n * up], alignments[b, :n // steps_per_frame, :lengths[b]],
                    wavs[b, :int(samples[b])]))
    return out
