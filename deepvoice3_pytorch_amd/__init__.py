# coding: utf-8
"""deepvoice3_pytorch_amd -- the DeepVoice3 / Nyanko hot path on hand-written MI355X (gfx950) HIP
kernels, behind the module API of r9y9/deepvoice3_pytorch.

Drop-in surface (reference deepvoice3_pytorch/__init__.py:11-126, builder.py:7-258):
    from deepvoice3_pytorch_amd import builder
    model = builder.deepvoice3(n_vocab=..., ...)      # / nyanko / deepvoice3_multispeaker
    mel, linear, alignments, done = model(text, mel_targets, speaker_ids, text_positions,
                                          frame_positions, input_lengths)
    model.load_state_dict(reference_checkpoint["state_dict"])   # identical keys and shapes

Nothing here falls back to torch CPU/GPU ops for the conv stacks, attention, losses or the
optimiser tail: if libdv3hip.so is missing the first op raises.
"""
__version__ = "0.1.0"

import torch
from torch import nn

from .modules import Embedding
from . import conv as _conv


class MultiSpeakerTTSModel(nn.Module):
    """seq2seq (Encoder + attention Decoder) followed by the post-net ("Converter"), with an optional
    speaker-embedding table -- the object the reference's builders return
    (deepvoice3_pytorch/__init__.py:11-97): same constructor keywords, attributes and call signature."""

    def __init__(self, seq2seq, postnet, mel_dim=80, linear_dim=513, n_speakers=1, speaker_embed_dim=16,
                 padding_idx=None, trainable_positional_encodings=False,
                 use_decoder_state_for_postnet_input=False, speaker_embedding_weight_std=0.01,
                 freeze_embedding=False):
        nn.Module.__init__(self)
        self.seq2seq, self.postnet = seq2seq, postnet
        self.mel_dim, self.linear_dim = mel_dim, linear_dim
        self.n_speakers, self.speaker_embed_dim = n_speakers, speaker_embed_dim
        self.trainable_positional_encodings = trainable_positional_encodings
        self.use_decoder_state_for_postnet_input = use_decoder_state_for_postnet_input
        self.freeze_embedding = freeze_embedding
        if n_speakers > 1:     # state_dict key "embed_speakers.weight", N(0, std) init like the reference
            self.embed_speakers = Embedding(n_speakers, speaker_embed_dim, padding_idx=None,
                                            std=speaker_embedding_weight_std)
        from .deepvoice3 import _name_sites
        _name_sites(self, "model")     # stable dropout-site names for the Philox streams

    def make_generation_fast_(self):
        """Inference: replace every weight_g / weight_v pair by the plain weight (__init__.py:39-46)."""
        for layer in (m for m in self.modules() if isinstance(m, _conv._WNLayer)):
            try:
                layer.remove_weight_norm_()
            except ValueError:
                continue           # plain (never weight-normed) layer

    def get_trainable_parameters(self):
        """Everything except the frozen sinusoid tables (and the text embedding when
        freeze_embedding is set), as a generator -- reference __init__.py:48-63."""
        dec, enc = self.seq2seq.decoder, self.seq2seq.encoder
        frozen = [] if self.trainable_positional_encodings else [dec.embed_query_positions, dec.embed_keys_positions]
        if self.freeze_embedding:
            frozen.append(enc.embed_tokens)
        skip = {id(p) for mod in frozen for p in mod.parameters()}
        return (p for p in self.parameters() if id(p) not in skip)

    def forward(self, text_sequences, mel_targets=None, speaker_ids=None, text_positions=None,
                frame_positions=None, input_lengths=None):
        speaker_embed = None
        if speaker_ids is not None:
            assert self.n_speakers > 1
            speaker_embed = self.embed_speakers(speaker_ids)
        mel, alignments, done, states = self.seq2seq(text_sequences, mel_targets, speaker_embed,
                                                     text_positions, frame_positions, input_lengths)
        n = text_sequences.size(0)
        mel = mel.reshape(n, -1, self.mel_dim)            # (B, T//r, mel_dim*r) -> (B, T, mel_dim)
        if not self.use_decoder_state_for_postnet_input:
            post_in = mel
        else:
            post_in = states.view(n, mel.size(1), -1)
            bct = getattr(states, "_dv3_bct", None)
            if bct is not None and post_in.shape == states.shape:
                post_in._dv3_bct = bct                    # r == 1: reuse the decoder's BCT image
        linear = self.postnet(post_in, speaker_embed)
        assert linear.size(-1) == self.linear_dim
        return mel, linear, alignments, done


    def _guide_of(self, durations, tl, Tt, dev):
        """synthesize_batch(durations=...) -> (guide table, steps) on the device, or ValueError naming the item"""
        from . import ops
        B, T = tl.numel(), self.seq2seq.decoder.max_decoder_steps + 1
        if torch.is_tensor(durations):
            if durations.dtype != torch.int32 or not durations.is_cuda or tuple(durations.shape) != (B, Tt):
                raise ValueError("synthesize_batch: durations as a tensor are int32 (%d, %d) on the device (what "
                                 "ops.monotonic_path returns), got %s %s" % (B, Tt, durations.dtype, tuple(durations.shape)))
            dur = durations
        else:
            rows = [[int(v) for v in d] for d in durations]
            if len(rows) != B:
                raise ValueError("synthesize_batch: %d duration lists for %d utterances" % (len(rows), B))
            host = torch.zeros(B, Tt, dtype=torch.int32)
            for b, d in enumerate(rows):
                if len(d) != int(tl[b]):
                    raise ValueError("synthesize_batch: item %d has %d durations for its %d tokens" % (b, len(d), int(tl[b])))
                host[b, :len(d)] = torch.tensor(d, dtype=torch.int32)
            dur = host.to(dev)
        guide, steps, flags = ops.guide_from_durations(dur, tl.to(torch.int32).to(dev), T)
        for b, f in enumerate(flags.tolist()):
            if f:
                raise ValueError("synthesize_batch: durations of item %d are flagged %s (negative: a duration below 0; "
                                 "empty: they sum to 0; over: they sum to more than max_decoder_steps + 1 = %d)" % (
                                     b, "+".join(ops.guide_flag_names(f)), T))
        return guide, steps

    def synthesize_batch(self, text_sequences, text_lengths, speaker_ids=None, durations=None, guide_window=None,
                         stall_limit=None, postnet=True):
        """Per-utterance batched synthesis: every item of a ragged batch comes back as if it had been synthesised alone
        (the reference's synthesis.tts at B = 1, synthesis.py:42-73, model part).  text_sequences (B, Tt) int ids on
        the device, padded past each item's text_lengths[b]; positions are 1..text_lengths[b].  The encoder and the
        post-net zero each item's columns past its own length after every layer (ops.ItemLengths), the decoder runs in
        its per-utterance mode (Decoder.incremental_forward(text_lengths=...)).  Inference only.
        -> (mel (B, T, mel_dim), linear (B, T * upsampling, linear_dim), alignments, done, frame_lengths): frame_lengths
        (int64[B], host) are each item's mel frames (decoder steps x r); everything past them is zero.
        stall_limit (None: off): the opt-in end-of-text stop -- an item whose attention has reached its last key keeps
        decode_program.stall_stop(...) steps if its done flag has not fired by then.  Applied after the decode and before
        the post-net; the decode loop itself still runs until the slowest item's done flag (or the cap).
        postnet=False: the post-net is not run and linear comes back None (a model trained without its post-net has
        nothing to say there; synthesis.tts_batch(from_mel=...) vocodes the mel instead); nothing else differs.
        durations (None: off): decoder steps per token -- an int32 (B, Tt) device tensor, as
        ops.monotonic_path and train_step.align_batch return them, or one list of text_lengths[b] ints per utterance.
        The decode is guided: every attention layer's window of step t is centred on the token that owns step t
        (ops.guide_from_durations), a token of duration 0 is skipped, and item b stops after sum(durations[b]) steps:
        frame_lengths = that sum x r.  done is what the model computed; the stop is the guide's end.  guide_window
        (backward, ahead): the window around the guided token instead of the attention layers' own.  A negative
        duration, a sum of 0 or a sum above max_decoder_steps + 1 raises ValueError naming the item.  Not together with
        stall_limit.  Runs on the fused step kernels only."""
        from . import ops
        if self.training:
            raise RuntimeError("synthesize_batch: eval mode only")
        if durations is not None and stall_limit is not None:
            raise ValueError("synthesize_batch: durations prescribe every item's stop; stall_limit cannot be combined "
                             "with them")
        if durations is None and guide_window is not None:
            raise ValueError("synthesize_batch: guide_window is the window of a guided decode (durations=)")
        dev = text_sequences.device
        B, Tt = text_sequences.shape
        tl = torch.as_tensor(text_lengths).reshape(-1).to(torch.int64).cpu()
        if tl.numel() != B or int(tl.min()) < 1 or int(tl.max()) > Tt:
            raise ValueError("synthesize_batch: %d text lengths in [1, %d] expected, got %s" % (B, Tt, tl.tolist()))
        tl_dev = tl.to(torch.int32).to(dev)
        pos = torch.arange(1, Tt + 1, device=dev)[None, :].expand(B, Tt)
        text_positions = torch.where(pos <= tl_dev[:, None].long(), pos, torch.zeros_like(pos))
        speaker_embed = None
        if speaker_ids is not None:
            assert self.n_speakers > 1
            speaker_embed = self.embed_speakers(speaker_ids)
        enc, dec = self.seq2seq.encoder, self.seq2seq.decoder
        prev, vl = ops.valid, ops.ItemLengths(tl, Tt, dev)
        ops.valid = vl
        try:
            with torch.no_grad():
                memory = enc(text_sequences, lengths=None, speaker_embed=speaker_embed)
                dec.start_fresh_sequence()
                kw = dict(speaker_embed=speaker_embed) if speaker_embed is not None else {}
                if durations is not None:
                    kw.update(guide=self._guide_of(durations, tl, Tt, dev), guide_window=guide_window)
                mel, alignments, done, states, steps = dec.incremental_forward(memory, text_positions,
                                                                               text_lengths=tl, **kw)
                if stall_limit is not None:
                    # the end-of-text stop, after the fact: the loop above ran to the slowest item's
                    # done flag; an item whose attention reached its last key stall_limit steps earlier keeps only those
                    from .decode_program import end_of_text_stops, item_results
                    ran = [int(n) for n in steps]
                    stall = end_of_text_stops(alignments, "btk", ran, tl_dev, stall_limit, dec.min_decoder_steps)
                    kept = [s or n for n, s in zip(ran, stall)]
                    if kept != ran:
                        m = max(kept)
                        mel, alignments, done, states, steps = item_results(
                            kept, mel[:, :m], alignments[:, :m], list(done[:m]), states[:, :m])
                Td = mel.size(1)
                mel = mel.reshape(B, -1, self.mel_dim)
                post_in = states.view(B, mel.size(1), -1) if self.use_decoder_state_for_postnet_input else mel
                linear = None
                if postnet:
                    vl.set_dec(steps, Td)
                    linear = self.postnet(post_in, speaker_embed).contiguous()
                    ops.zero_frames(linear, vl.dec_len, int(steps.min()), linear.size(1) // Td)
        finally:
            ops.valid = prev
        assert linear is None or linear.size(-1) == self.linear_dim
        return mel, linear, alignments, done, steps * (mel.size(1) // Td)


class AttentionSeq2Seq(nn.Module):
    """Encoder -> attention Decoder pair (reference __init__.py:100-126)."""

    def __init__(self, encoder, decoder):
        nn.Module.__init__(self)
        self.encoder, self.decoder = encoder, decoder
        att = getattr(decoder, "attention", None)
        if isinstance(att, nn.ModuleList):
            encoder.num_attention_layers = sum(1 for layer in att if layer is not None)

    def forward(self, text_sequences, mel_targets=None, speaker_embed=None, text_positions=None,
                frame_positions=None, input_lengths=None):
        memory = self.encoder(text_sequences, lengths=input_lengths, speaker_embed=speaker_embed)
        return self.decoder(memory, mel_targets, text_positions=text_positions,
                            frame_positions=frame_positions, speaker_embed=speaker_embed,
                            lengths=input_lengths)
