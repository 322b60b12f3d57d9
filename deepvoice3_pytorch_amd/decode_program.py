# coding: utf-8
"""Per-step launch program of an autoregressive decoder on the fused step kernels (csrc/decode_step.hip).

A decoder step of the reference (deepvoice3.py:397-461, nyanko.py:283-321) is ~100 tiny module calls; here it is a
flat list of descriptors built ONCE per utterance batch -- one dv3_conv_step_f32 per conv / projection layer (ring
buffer on a device step counter, k-tap GEMV, the whole layer tail) and one dv3_attn_step_f32 per attention read --
that the host replays launch by launch (optionally as one hipGraph per step), or that ONE persistent launch walks for
the whole utterance (dv3_decode_program_run: the loop, the ring buffers, the stop rule and the layer-to-layer
hand-over all stay on the device; opt-in, see StepProgram.decode).  `StepProgram` owns the buffers the descriptors point
at, the stacked per-step outputs among them (`stack`, read back through `results` / `read_slot` / `read_slots`).

How a decoder builds its program: ONE walk over its layers, `Decoder._step_entries`, appends the entries; the walk over a
"Conv1d (+ReLU)" stack is modules.conv_relu_layers, shared with the module-by-module path.  `Decoder._slot_entries` runs
that walk on per-slot operand buffers; `Decoder._fast_decode_eligible(Tk)` is the same call against a DRY program
(StepProgram(1, "meta", ...): meta-device buffers, nothing packed, launched or allocated), which records why the step
kernels would not take an entry (`refuse`: a layer the walk has no entry for, a window `ops.conv_step_fits` rejects,
attention scores beyond the LDS) -- so the predicate can not drift from the builder.  `incremental_forward` does not
ask the predicate first: it builds its program once, and a build that was refused (nothing is packed or laid out for
a program from its first refusal on) hands the call to the module-by-module loop.  The frames around the walk, the
same for both decoder families, are `incremental_decode` and `slot_program_frame` below.

Slot mode (StepProgram(B, device, t_cap=...)): the program is built ONCE for B batch slots and lives
across utterances.  Every slot runs at its own step t - t_off[b] (the kernels' slot mode, include/dv3hip.h), so a slot
whose utterance has ended is handed to the next one (`admit`) while its neighbours keep decoding; `RollingSchedule` is
the host-side book of which ticket sits in which slot since which global step.
"""
import ctypes
import functools

import torch

from . import ops
from ._lib import STRUCTS, _env_flag, _env_int, _env_str

# which loop DecodeProgram.decode runs when its caller does not say (see its docstring)
persistent_default = _env_flag("DV3_DECODE_PERSISTENT", False)
launched_default = _env_str("DV3_DECODE_LAUNCHED", "1") != "0"      # (only "0" turns it off)
# developer knob of the persistent program: timing ablations of its barriers (scripts/decode_time.py sets the attribute)
ablate = _env_int("DV3_DECODE_ABLATE", 0)


def item_stops(done_rows, t0, min_steps, max_steps, stops):
    """The reference's B = 1 stop rule (deepvoice3.py:469-473) applied to every item of a per-utterance batch: item b
    stops after the first step n > min_steps whose done_b > 0.5, or after step max_steps + 1.  done_rows: the host
    rows (one per step, steps t0 + 1, t0 + 2, ...) of B booleans done > 0.5; stops: one entry per item, 0 while the
    item runs, updated in place to its number of steps.  -> True once every item has stopped (the batch then ends at
    max(stops) steps)."""
    for k, row in enumerate(done_rows):
        n = t0 + k + 1
        for b, d in enumerate(row):
            if stops[b] == 0 and ((n > min_steps and d) or n > max_steps):
                stops[b] = n
    return all(stops)


def stall_stop(end_step, stall_limit, min_steps):
    """The opt-in end-of-text stop: the number of steps after which an item stops once its attention
    has reached its last key.  end_step: the first step whose argmax sat on the last key (the alignment statistics'
    column, -1 if none yet) -> 0 while the end has not been reached (the item runs on), otherwise
    max(end_step + 1 + stall_limit, min_steps + 1): stall_limit more steps after the one that reached the end, and never
    fewer than the done flag's own rule allows (item_stops: n > min_steps).  The count depends only on rows before it,
    so it is the same whenever it is evaluated."""
    end_step, stall_limit, min_steps = int(end_step), int(stall_limit), int(min_steps)
    if stall_limit < 0:
        raise ValueError("stall_stop: stall_limit must be >= 0, got %d" % stall_limit)
    if end_step < 0:
        return 0
    return max(end_step + 1 + stall_limit, min_steps + 1)


# the columns of an alignment-statistics row (include/dv3hip.h: dv3_alignment_stats_f32), in order
ALIGNMENT_COLUMNS = ("steps", "keys", "focus_mean", "focus_min", "last_key", "furthest_key", "end_step", "tail_steps",
                     "covered_keys", "back_steps", "max_jump", "longest_stall", "bad_rows")


def end_of_text_stops(attn, layout, steps, key_len, stall_limit, min_steps):
    """stall_stop for every item of a batch or every slot of a slot program: attn / layout as ops.alignment_stats takes
    them (read in place), steps: the steps each item has run so far (host ints; 0: not looked at), key_len: device
    int32[B].  One kernel call and one device read.  -> per item the step count it stops after by the end-of-text rule
    if that many steps have run, else 0."""
    dev = attn.device
    run = torch.tensor([int(n) for n in steps], dtype=torch.int32).to(dev)
    stats = ops.alignment_stats(attn, run, key_len.to(device=dev, dtype=torch.int32), layout)
    end = stats[:, ALIGNMENT_COLUMNS.index("end_step")].tolist()
    out = []
    for n, e in zip(steps, end):
        s = stall_stop(e, stall_limit, min_steps) if n > 0 else 0
        out.append(s if 0 < s <= n else 0)
    return out


def item_results(stops, outputs, alignments, dones, states):
    """the per-utterance decode's results with every frame past item b's own step count stops[b] set to zero (in place
    where the tensor allows) -> (outputs, alignments, dones, states, frame_lengths int64[B] on the host)"""
    lengths = torch.tensor(stops, dtype=torch.int32)
    dev = outputs.device
    ld = lengths.to(dev)
    n = min(stops)
    outputs, alignments, states = (ops.zero_frames(x.contiguous(), ld, n) for x in (outputs, alignments, states))
    if dones:
        d = ops.zero_frames(torch.cat([x.reshape(x.size(0), 1, 1) for x in dones], dim=1), ld, n)
        dones = [d[:, i:i + 1] for i in range(d.size(1))]
    return outputs, alignments, dones, states, lengths.long()


def item_key_len(text_lengths, B, Tk, device):
    """Decoder.incremental_forward(text_lengths=...): each item's key count as a device int32[B] (None: reference mode)"""
    if text_lengths is None:
        return None
    tl = torch.as_tensor(text_lengths).reshape(-1).to(torch.int64).cpu()
    if tl.numel() != B or int(tl.min()) < 1 or int(tl.max()) > Tk:
        raise ValueError("text_lengths: %d lengths in [1, %d] expected for a batch of %d, got %s" % (
            B, Tk, B, tl.tolist()))
    return tl.to(torch.int32).to(device)


def incremental_decode(dec, encoder_out, text_lengths, *args, **guided):
    """The frame of Decoder.incremental_forward, both families: the per-utterance key lengths and stop list, the fused
    step program (dec._incremental_fast), the module-by-module loop (dec._incremental_modules) where the step kernels
    do not take the decoder or the key count, and the zero tails of a per-utterance result.  The program is built ONCE
    per call: _incremental_fast returns None if its own build was refused (StepProgram.refuse: nothing of a refused
    program is packed or launched), which is the answer _fast_decode_eligible gives from a dry build.  args: the
    family's own arguments, handed to either.
    guided: guide=(guide int32 (B, T) on the device, steps int32[B]) -- a guided decode: every
    attention layer centres item b's window of step t on guide[b, min(t, steps[b] - 1)] and item b stops after
    steps[b] steps -- and guide_window=(backward, ahead), the window used instead of the layers' own.  Guided decoding
    runs on the fused step kernels only: it needs text_lengths, and a decoder they do not take is refused."""
    keys = encoder_out[0]
    B = keys.size(0)
    key_len = item_key_len(text_lengths, B, keys.size(1), keys.device)
    stops = [0] * B if key_len is not None else None
    guide, guide_window = guided.pop("guide", None), guided.pop("guide_window", None)
    if guided:
        raise TypeError("incremental_forward: unexpected keyword(s) %s" % sorted(guided))
    if guide is not None:
        return guided_decode(dec, encoder_out, key_len, stops, args, guide, guide_window)
    if guide_window is not None:
        raise ValueError("incremental_forward: guide_window is the window of a guided decode (guide=)")
    res = None
    if getattr(dec, "fast_decode", False) and keys.is_cuda:
        res = dec._incremental_fast(encoder_out, *args, key_len=key_len, stops=stops)
    if res is None:
        res = dec._incremental_modules(encoder_out, *args, key_len=key_len, stops=stops)
    return res if stops is None else item_results(stops, *res)


def guide_window_of(guide_window):
    """the guide_window= keyword -> None or (backward >= 0, ahead >= 1) as ints"""
    if guide_window is None:
        return None
    try:
        back, ahead = (int(w) for w in guide_window)
    except (TypeError, ValueError):
        raise ValueError("guide_window: a pair (backward, ahead) expected, got %r" % (guide_window,))
    if back < 0 or ahead < 1:
        raise ValueError("guide_window: backward >= 0 and ahead >= 1 expected, got (%d, %d)" % (back, ahead))
    return back, ahead


def guided_decode(dec, encoder_out, key_len, stops, args, guide, guide_window):
    """incremental_decode under a guide: the checks, then the fused step program alone"""
    keys = encoder_out[0]
    if key_len is None:
        raise ValueError("incremental_forward: a guide needs text_lengths (guided decoding is per utterance)")
    try:
        table, steps = guide
    except (TypeError, ValueError):
        raise ValueError("incremental_forward: guide=(guide table, steps) expected")
    B = keys.size(0)
    for t, name in ((table, "guide table"), (steps, "steps")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32):
            raise ValueError("incremental_forward: the %s must be an int32 tensor on the device" % name)
    if table.dim() != 2 or table.size(0) != B or steps.numel() != B or (table.size(1) > 1 and table.stride(1) != 1):
        raise ValueError("incremental_forward: a guide table (B, T) with a dense step axis and B steps expected for a "
                         "batch of %d, got %s and %d steps" % (B, tuple(table.shape), steps.numel()))
    window = guide_window_of(guide_window)
    if not (getattr(dec, "fast_decode", False) and keys.is_cuda):
        raise RuntimeError("guided decode: runs on the fused decode-step kernels only (fast_decode on a GPU); there is "
                           "no module-by-module fallback under a guide")
    res = dec._incremental_fast(encoder_out, *args, key_len=key_len, stops=stops, guide=(table, steps),
                                guide_window=window)
    if res is None:
        raise RuntimeError("guided decode: runs on the fused decode-step kernels only, and this decoder (or %d keys) is "
                           "not eligible for them (_fast_decode_eligible); there is no module-by-module fallback under "
                           "a guide" % keys.size(1))
    return item_results(stops, *res)


def slot_program_frame(dec, slots, max_text_len, dev):
    """The frame of Decoder.slot_program, both families: the checks -> an empty slot-mode StepProgram of
    max_decoder_steps + 1 rows per slot"""
    if dec.training:
        raise RuntimeError("slot_program: eval mode only")
    if dev.type != "cuda" or not getattr(dec, "fast_decode", False) or not dec._fast_decode_eligible(int(max_text_len)):
        raise RuntimeError("slot_program: rolling admission runs on the fused decode-step kernels only, and this "
                           "decoder (or %d keys) is not eligible for them (_fast_decode_eligible); there is no "
                           "module-by-module fallback in slot mode" % int(max_text_len))
    t_cap = dec.max_decoder_steps + 1
    if t_cap >= dec.embed_query_positions.weight.size(0):
        raise RuntimeError("slot_program: decoder steps exceed max_positions")
    return StepProgram(int(slots), dev, t_cap=t_cap)


# ops.conv_step_fits (the library's own answer for a (taps, input channels) pair), asked once per pair
_conv_step_fits = functools.lru_cache(maxsize=None)(ops.conv_step_fits)
SLOT_IDLE = 2 ** 31 - 1         # t_off of a slot nobody sits in: its step t - t_off is negative for every t >= 0


class StepProgram(object):
    def __init__(self, B, device, t_cap=None):
        """t_cap: slot mode -- the rows every stacked output and step-indexed table holds per slot (the decoder's
        max_decoder_steps + 1); the program then owns t_off and key_len (int32[B] on the device).
        device "meta": a dry program -- the entries are recorded with every scalar field set and checked (`refused`),
        but its buffers are meta tensors and nothing is packed, launched or allocated"""
        self.B, self.dev = B, device
        self.dry = torch.device(device).type == "meta"
        self.refused = None           # why the step kernels do not take this program (the first reason), see refuse()
        self.f32 = dict(dtype=torch.float32, device=device)
        self.t_dev = torch.zeros(1, dtype=torch.int32, device=device)      # the step counter every launch reads
        self.keep, self.prog = [self.t_dev], []
        self.per_item = False         # an attention entry reads per-utterance key lengths (attn_step(key_len=...))
        self.n_attn, self.align_scale = 0, 1.0      # attention entries so far; what results() scales the alignments by
        self.t_cap = None if t_cap is None else int(t_cap)
        if self.t_cap is not None:
            if self.t_cap < 1:
                raise ValueError("decode program: slot mode needs t_cap >= 1")
            self.t_off = torch.full((B,), SLOT_IDLE, dtype=torch.int32, device=device)
            self.key_len = torch.ones(B, dtype=torch.int32, device=device)
            self.t = 0                # the global step (host): the next launch's t_value
            self.keep.extend([self.t_off, self.key_len])

    @property
    def slot_mode(self):
        return self.t_cap is not None

    @property
    def live(self):
        """weights are packed and operands laid out for the entries: not in a dry program, and no more once one was refused"""
        return not self.dry and self.refused is None

    def buffer(self, *shape):
        t = (torch.empty if self.dry else torch.zeros)(*shape, **self.f32)      # (zeros on "meta" is a slow Python path)
        self.keep.append(t)
        return t

    def stack(self, n, D, Cs, Tk):
        """the stacked per-step outputs, n rows each (slot mode: n = t_cap), for the entries' out_seq / attn_seq:
        outs (n, B, D), dones_seq (n, B, 1), states (n, B, Cs), aligns (n, B, Tk)"""
        self.outs, self.dones_seq = self.buffer(n, self.B, D), self.buffer(n, self.B, 1)
        self.states, self.aligns = self.buffer(n, self.B, Cs), self.buffer(n, self.B, Tk)

    def refuse(self, why):
        """the step kernels do not take what the builder was about to append: the decoder is not eligible"""
        self.refused = self.refused or why

    def _step_tiles(self, pk, K, M, Cg):
        """the weights of a packed image in step-tile order, built once per image"""
        tiles = getattr(pk, "step_tiles", None)
        if tiles is None:
            tiles = torch.empty(ops._lib.lib().dv3_conv_step_pack_floats(K, M, Cg), **self.f32)
            ops._lib.call("dv3_conv_step_pack_f32", pk.fwd.data_ptr(), pk.lda, pk.a_half, K, M, Cg, tiles.data_ptr(),
                          ops._stream())
            pk.step_tiles = tiles
        return tiles

    def conv_step(self, layer, x, mode, Cout, k=1, dil=1, gated=False, residual=False, spk=None, r=None, r2=None,
                  post_add=None, y=None, y_act=None, y_pre=None, out_seq=None):
        """one incremental conv layer (conv.py:17-46) with its tail; x (B, Cin) view (row stride free) -> y (B, Cout)"""
        B = self.B
        if y is None:
            y = torch.empty(B, Cout, **self.f32)
        Cin = x.size(1)
        if not _conv_step_fits(k, Cin):         # dv3_conv_step_f32 stages the k-tap window of a batch group in LDS
            self.refuse("a %d-tap layer of %d input channels does not fit the conv-step kernel's LDS" % (k, Cin))
        d = STRUCTS["dv3_conv_step_desc"]()
        d.x, d.x_bs = x.data_ptr(), x.stride(0)
        if k > 1:
            L = (k - 1) * dil + 1
            ring = self.buffer(L, B, Cin)
            d.ring, d.L = ring.data_ptr(), L
        d.t = self.t_dev.data_ptr()
        pk = None
        if self.live:
            pk = layer.packed(glu_cg=Cout if gated else 0)
            tiles = self._step_tiles(pk, k * Cin, 2 * Cout if gated else Cout, Cout if gated else 0)
            d.a, d.lda, d.a_half = tiles.data_ptr(), pk.lda, pk.a_half
        d.bias = layer.bias.data_ptr() if layer.bias is not None else None
        if spk is not None:
            d.spk, d.spk_bs = spk.data_ptr(), spk.stride(0)
        if r is not None:
            d.r, d.r_bs = r.data_ptr(), r.stride(0)
        if r2 is not None:
            d.r2, d.r2_bs = r2.data_ptr(), r2.stride(0)
        if post_add is not None:
            d.post_add, d.post_add_ts, d.post_add_bs = post_add.data_ptr(), post_add.stride(0), post_add.stride(1)
        d.y, d.y_bs = y.data_ptr(), y.stride(0)
        if y_act is not None:
            d.y_act, d.y_act_bs = y_act.data_ptr(), y_act.stride(0)
        if y_pre is not None:
            d.y_pre, d.y_pre_bs = y_pre.data_ptr(), y_pre.stride(0)
        if out_seq is not None:
            d.out_seq, d.out_seq_ts, d.out_seq_bs = out_seq.data_ptr(), out_seq.stride(0), out_seq.stride(1)
        d.B, d.Cin, d.M = B, Cin, (2 * Cout if gated else Cout)
        if self.slot_mode:
            d.t_off, d.t_cap = self.t_off.data_ptr(), self.t_cap
        d.Cg, d.J, d.dil, d.mode, d.residual = (Cout if gated else 0), k, dil, mode, int(residual)
        self.keep.extend([pk, x, y, spk, r, r2, post_add, y_act, y_pre, out_seq])
        self.prog.append(("dv3_conv_step_f32", d))
        return y

    def attn_step(self, q, k, v, window_backward, window_ahead, monotonic, attn_seq=None, key_len=None, rows=False,
                  guide_window=None):
        """one attention read over (B, E, Tk) keys / values (deepvoice3.py:143-171 at Tq = 1, no padding mask);
        key_len (device int32[B]): per-utterance mode -- item b reads its own keys n < key_len[b] with its own window.
        rows: k and v are already the contiguous-row (B, Tk, E) images the kernel reads (slot mode: the slots' rows,
        rewritten at every admission); guide_window (backward, ahead): the window of a guided decode, instead of the
        layer's own"""
        B = self.B
        if guide_window is not None:
            window_backward, window_ahead = guide_window
        if self.slot_mode:
            if not rows or key_len is not None:
                raise RuntimeError("decode program: slot mode reads per-slot key / value rows and its own key_len")
            key_len = self.key_len
        E, Tk = (k.size(2), k.size(1)) if rows else (k.size(1), k.size(2))
        if (E + Tk) * 4 > 64 * 1024:            # dv3_attn_step_f32 keeps the query and the scores of all keys in LDS
            self.refuse("the attention scores of %d keys do not fit the attention-step kernel's LDS" % Tk)
        # the stacked alignment is the FIRST attention layer's; over n layers the reference's running `ave + ave`
        # followed by / n (deepvoice3.py:449-461) makes of it that alignment * 2^(n-1) / n
        self.n_attn += 1
        self.align_scale = float(2 ** (self.n_attn - 1)) / self.n_attn
        ctx = torch.empty(B, E, **self.f32)
        la = self.buffer(2 * B if key_len is not None else 2).to(torch.int32) if monotonic else None
        if la is not None:
            self.keep.append(la)
        # one-frame reads want a key / value ROW contiguous: (B, Tk, E), transposed once per utterance batch
        if rows:
            if not (k.is_contiguous() and v.is_contiguous()):
                raise RuntimeError("decode program: key / value rows must be contiguous")
            kt, vt = k, v
        else:
            kt, vt = (ops.transpose(k.contiguous()), ops.transpose(v.contiguous())) if self.live else (k, v)
        self.keep.extend([kt, vt])
        a = STRUCTS["dv3_attn_step_desc"]()
        a.q, a.q_bs, a.k, a.v, a.kv_tke = q.data_ptr(), q.stride(0), kt.data_ptr(), vt.data_ptr(), 1
        a.last_attended = la.data_ptr() if la is not None else None
        a.win_back, a.win_ahead, a.t = window_backward, window_ahead, self.t_dev.data_ptr()
        a.ctx, a.ctx_bs = ctx.data_ptr(), ctx.stride(0)
        if attn_seq is not None:
            a.attn_seq, a.attn_seq_ts = attn_seq.data_ptr(), attn_seq.stride(0)
        a.B, a.E, a.Tk = B, E, Tk
        if key_len is not None:
            key_len = key_len.to(device=self.dev, dtype=torch.int32).contiguous()
            a.key_len = key_len.data_ptr()
            self.per_item = True
        if self.slot_mode:
            a.t_off, a.t_cap = self.t_off.data_ptr(), self.t_cap
        self.keep.extend([q, k, v, ctx, attn_seq, key_len])
        self.prog.append(("dv3_attn_step_f32", a))
        return ctx

    def run_step(self, guide=None):
        """guide (table, steps): the attention entries run the guided kernel on it"""
        s = ops._stream()
        for name, d in self.prog:
            if guide is not None and name == "dv3_attn_step_f32":
                ops._lib.call("dv3_attn_step_guided_f32", ctypes.byref(d), guide[0].data_ptr(), self._guide_bs(guide[0]),
                              guide[1].data_ptr(), s)
            else:
                ops._lib.call(name, ctypes.byref(d), s)
        self.t_dev.add_(1)

    def _guide_bs(self, table):
        return table.stride(0) if self.B > 1 else table.size(1)

    def _entries(self, cur_in, test_inputs):
        """the program as a host array of dv3_decode_entry (teacher forcing: the entries that read the decoder input
        buffer read frame t of test_inputs instead, deepvoice3.py:411-415)"""
        B = self.B
        Entry = STRUCTS["dv3_decode_entry"]
        arr = (Entry * len(self.prog))()
        ti = None
        if test_inputs is not None:
            ti = test_inputs.to(torch.float32).reshape(B, test_inputs.size(1), -1).contiguous()
            if ti.size(2) != cur_in.size(1):
                raise RuntimeError("decode program: test_inputs frames carry %d values, the decoder input %d" % (
                    ti.size(2), cur_in.size(1)))
            self.keep.append(ti)
        fed = 0
        for i, (name, d) in enumerate(self.prog):
            if name == "dv3_conv_step_f32":
                arr[i].kind = 0
                arr[i].conv = d
                if ti is not None and d.x == cur_in.data_ptr():
                    arr[i].conv.x, arr[i].conv.x_bs, arr[i].conv.x_ts = ti.data_ptr(), ti.stride(0), ti.stride(1)
                    fed += 1
            else:
                arr[i].kind = 1
                arr[i].attn = d
        if ti is not None and fed == 0:
            raise RuntimeError("decode program: no entry reads the decoder input buffer")
        return arr, ti

    # ---- slot mode -------------------------------------------------------------------------------------------------
    def seal(self, cur_in, write_operands):
        """slot mode: the program is complete.  cur_in: the decoder-input buffer (the x of entry 0);
        write_operands(slot_index int64[n] on the device, memory, text_positions, speaker_embed): the decoder family's
        writer of the per-slot operands (projected keys and values, position codes, speaker biases) for a group of
        admitted utterances."""
        if not self.slot_mode or self.dry or self.refused:
            raise RuntimeError("decode program: seal() is the slot mode's, of a program the step kernels take (%s)" %
                               self.refused)
        if not self.prog or self.prog[0][0] != "dv3_conv_step_f32" or self.prog[0][1].x != cur_in.data_ptr():
            raise RuntimeError("decode program: entry 0 must read the decoder input buffer")
        self._write_operands = write_operands
        self._arr, _ = self._entries(cur_in, None)
        p = STRUCTS["dv3_decode_program"]()
        p.entries_host = ctypes.addressof(self._arr)
        p.n_entries, p.B = len(self.prog), self.B
        p.n_steps = 1
        self._p = p
        return self

    def admit(self, slots, memory, text_positions, text_lengths, speaker_embed=None):
        """hand the batch slots `slots` (a list of n ints) to n new utterances at the current global step: memory = the
        encoder's (keys, values) (n, Tt, D) of the group, text_positions (n, Tt), text_lengths n ints (item i reads its
        keys < text_lengths[i]), speaker_embed (n, E) or None.  Writes the per-slot operands, key_len and
        t_off = the global step, and starts a fresh sequence in those slots (one dv3_decode_slots_reset launch)."""
        slots = [int(s) for s in slots]
        n = len(slots)
        keys = memory[0]
        tl = torch.as_tensor(text_lengths).reshape(-1).to(torch.int64).cpu()
        if n == 0 or len(set(slots)) != n or min(slots) < 0 or max(slots) >= self.B:
            raise ValueError("decode program: admit() takes distinct slot indices in [0, %d), got %s" % (self.B, slots))
        if keys.size(0) != n or tl.numel() != n or int(tl.min()) < 1 or int(tl.max()) > keys.size(1):
            raise ValueError("decode program: admit() of %d slots got %d utterances with text lengths %s over %d keys" % (
                n, keys.size(0), tl.tolist(), keys.size(1)))
        idx = torch.tensor(slots, dtype=torch.int64).to(self.dev)
        with torch.no_grad():
            self._write_operands(idx, memory, text_positions, speaker_embed)
            self.key_len[idx] = tl.to(torch.int32).to(self.dev)
            self.t_off[idx] = self.t
            self._idx32 = idx.to(torch.int32)
            ops._lib.call("dv3_decode_slots_reset", ctypes.byref(self._p), self._idx32.data_ptr(), n, ops._stream())

    def release(self, slots):
        """the slots are idle from the next step on (nothing of theirs is stored until they are admitted again)"""
        if len(slots):
            self.t_off[torch.tensor([int(s) for s in slots], dtype=torch.int64).to(self.dev)] = SLOT_IDLE

    def run_steps(self, n):
        """n steps of every slot, one library call (dv3_decode_program_launch); the global step advances by n"""
        if n > 0:
            self._p.t0, self._p.n_steps = self.t, int(n)
            ops._lib.call("dv3_decode_program_launch", ctypes.byref(self._p), ops._stream())
            self.t += int(n)

    def slot_step(self, slot_t_off):
        """the step a slot admitted at global step slot_t_off runs next"""
        return self.t - int(slot_t_off)

    def done_flags(self):
        """the stacked done flags > 0.5 as host rows [t_b][slot] (one device read per chunk of steps)"""
        return (self.dones_seq.reshape(self.t_cap, self.B) > 0.5).tolist()

    def _stacked(self, n, items=slice(None)):
        """the first n stacked rows of `items` (an index, a slice or an index tensor over the batch), the alignments
        scaled -> (outputs, alignments, states), each (n, items, .)"""
        outs, ali, states = (x[:n].index_select(1, items) if torch.is_tensor(items) else x[:n, items]
                             for x in (self.outs, self.aligns, self.states))
        if self.align_scale != 1.0:
            ali = ali * self.align_scale
        return outs, ali, states

    def results(self, t):
        """what Decoder.incremental_forward returns after t steps -> (outputs (B, t, D), alignments (B, t, Tk),
        dones: t tensors (B, 1, 1), decoder_states (B, t, Cs))"""
        outs, ali, states = self._stacked(t)
        return (outs.transpose(0, 1).contiguous(), ali.transpose(0, 1),
                [self.dones_seq[i].view(self.B, 1, 1) for i in range(t)], states.transpose(0, 1).contiguous())

    def decode_for(self, dec, cur_in, test_inputs, stops, guide=None):
        """decode() with the decoder's step limits and its choice of loop -> results() of the steps taken"""
        t = self.decode(cur_in, test_inputs, self.dones_seq, dec.min_decoder_steps, dec.max_decoder_steps,
                        getattr(dec, "use_step_graph", False), getattr(dec, "persistent_decode", None),
                        getattr(dec, "launched_decode", None), stops=stops, guide=guide)
        return self.results(t)

    def read_slot(self, slot, n):
        """copies of slot's first n stacked rows -> (outputs (n, D), alignments (n, Tk_cap), dones (n,), states (n, Cs))"""
        outs, ali, states = self._stacked(n, slot)
        return outs.clone(), ali.clone(), self.dones_seq[:n, slot, 0].clone(), states.clone()

    def read_slots(self, slots, steps):
        """the stacked results of several slots as one zero-tailed batch (item_results): slots[i] ran steps[i] steps
        -> (outputs (n, max steps, D), alignments (n, max steps, Tk_cap), states (n, max steps, Cs))"""
        idx = torch.tensor([int(s) for s in slots], dtype=torch.int64).to(self.dev)
        outputs, alignments, states = (x.transpose(0, 1) for x in self._stacked(max(steps), idx))
        outputs, alignments, _, states, _ = item_results(list(steps), outputs, alignments, [], states)
        return outputs, alignments, states

    def decode_persistent(self, cur_in, test_inputs, dones_seq, min_steps, max_steps):
        """the whole loop as one launch of the persistent program kernel (include/dv3hip.h: dv3_decode_program_run)
        -> number of steps taken"""
        B, dev = self.B, self.dev
        free_running = test_inputs is None
        Prog = STRUCTS["dv3_decode_program"]
        arr, ti = self._entries(cur_in, test_inputs)
        host = bytearray(bytes(arr))
        entries = torch.frombuffer(host, dtype=torch.uint8).to(dev)
        n_sync = ops._lib.lib().dv3_decode_program_sync_ints(B)
        sync = torch.empty(n_sync, dtype=torch.int32, device=dev)
        steps_out = torch.zeros(1, dtype=torch.int32, device=dev)
        p = Prog()
        p.entries = entries.data_ptr()
        p.entries_host = ctypes.addressof(arr)
        p.n_entries, p.B = len(self.prog), B
        p.t0 = 0
        p.n_steps = ti.size(1) if ti is not None else max_steps + 1
        if free_running:
            p.done_seq, p.done_ts = dones_seq.data_ptr(), dones_seq.stride(0)
        p.min_steps, p.max_steps = min_steps, max_steps
        p.reserved = ablate
        p.sync, p.steps_out = sync.data_ptr(), steps_out.data_ptr()
        ops._lib.call("dv3_decode_program_run", ctypes.byref(p), ops._stream())
        t = int(steps_out.item())
        if t < 0:
            raise RuntimeError("decode program: a device barrier timed out (the persistent grid was not co-resident?)")
        self.t_dev.fill_(t)
        return t

    def decode_launched(self, cur_in, test_inputs, dones_seq, min_steps, max_steps, chunk=8, stops=None):
        """the loop with the launches issued by the library (dv3_decode_program_launch: one call per chunk of steps, the
        step index in the descriptors).  Free running, the done flags are read once per chunk and the steps after the
        stopping one are dropped -- later steps never change earlier outputs.  stops (a list of B zeros): the
        per-utterance rule instead (item_stops), each item's step count stored there.  -> number of steps taken"""
        Prog = STRUCTS["dv3_decode_program"]
        arr, ti = self._entries(cur_in, test_inputs)
        p = Prog()
        p.entries_host = ctypes.addressof(arr)
        p.n_entries, p.B = len(self.prog), self.B
        stream = ops._stream()
        if ti is not None:
            p.t0, p.n_steps = 0, ti.size(1)
            if p.n_steps > 0:
                ops._lib.call("dv3_decode_program_launch", ctypes.byref(p), stream)
            if stops is not None:
                stops[:] = [int(ti.size(1))] * self.B
            return int(ti.size(1))
        limit, t = max_steps + 1, 0
        while True:
            n = min(min_steps + 1 if t == 0 else chunk, limit - t)
            p.t0, p.n_steps = t, n
            ops._lib.call("dv3_decode_program_launch", ctypes.byref(p), stream)
            if stops is not None:
                if item_stops((dones_seq[t:t + n].reshape(n, -1) > 0.5).tolist(), t, min_steps, max_steps, stops):
                    return max(stops)
                t += n
                continue
            done = (dones_seq[t:t + n].reshape(n, -1) > 0.5).all(dim=1).tolist()
            for k in range(n):
                if t + k + 1 > min_steps and done[k]:
                    return t + k + 1
            t += n
            if t >= limit:
                return t

    def decode_guided(self, cur_in, guide, stops, launched):
        """the loop under a guide: free running on the model's own outputs, item b's attention windows
        centred on guide[b, min(t, steps[b] - 1)], max(steps) steps -- one host read of steps, no done flag is read;
        stops[:] = steps.  launched: the whole utterance in ONE dv3_decode_program_launch_guided call; else one
        dv3_attn_step_guided_f32 / dv3_conv_step_f32 call per entry per step from here.  -> number of steps taken"""
        table, steps = guide
        counts = [int(n) for n in steps.tolist()]
        n = max(counts)
        if len(counts) != self.B or min(counts) < 1:
            raise ValueError("decode program: a guide gives every one of the %d items at least one step, got %s" % (
                self.B, counts))
        if n > table.size(1) or n > self.outs.size(0):
            raise ValueError("decode program: the guide asks for %d steps; its table holds %d rows and the program's "
                             "stacked outputs %d" % (n, table.size(1), self.outs.size(0)))
        steps = steps.contiguous()
        self.keep.extend([table, steps])
        if launched:
            arr, _ = self._entries(cur_in, None)
            p = STRUCTS["dv3_decode_program"]()
            p.entries_host = ctypes.addressof(arr)
            p.n_entries, p.B = len(self.prog), self.B
            p.t0, p.n_steps = 0, n
            ops._lib.call("dv3_decode_program_launch_guided", ctypes.byref(p), table.data_ptr(), self._guide_bs(table),
                          steps.data_ptr(), ops._stream())
            self.t_dev.fill_(n)
        else:
            for _ in range(n):
                self.run_step((table, steps))
        stops[:] = counts
        return n

    def decode(self, cur_in, test_inputs, dones_seq, min_steps, max_steps, use_graph, persistent=None, launched=None,
               stops=None, guide=None):
        """the decoder loop (deepvoice3.py:397-473 / nyanko.py:277-331): teacher-forced over test_inputs (B, n, D), or
        free running until every item's done flag passed 0.5 after min_steps, at most max_steps + 1 steps.
        -> number of steps taken.  Default (launched): one launch per program entry per step, issued by the library in
        chunks of steps (decode_launched: ~3 us of host time per launch).  launched=False: the same launches from
        Python + ctypes, optionally replayed as a per-step hipGraph (~100 us of host time per step either way: about
        what the GPU needs for the step, so the host is on the critical path).  persistent=True (or
        DV3_DECODE_PERSISTENT=1): ONE launch for the whole loop -- bit-identical, and the host drops out entirely,
        but on MI355X the device-wide barrier between layers (agent-scope release + acquire: L2 write-back /
        invalidate across the 8 XCDs, ~3.5 us) costs more than a kernel boundary does (scripts/decode_time.py), so
        it is opt-in.  Per-utterance mode (attention entries with key_len): pass stops = [0] * B; every item stops by
        its own done flag (item_stops), the loop runs until all have, and stops holds each item's step count; the
        persistent program does not take this mode.  guide=(table, steps): decode_guided (per-utterance mode only; not
        the persistent program, not a slot-mode program)."""
        if guide is not None and self.slot_mode:
            raise RuntimeError("decode program: a slot-mode program does not take a guide (a slot runs at its own step "
                               "t - t_off[b]; the guide table has one step axis for the batch)")
        if self.slot_mode:
            if persistent or (persistent is None and persistent_default):
                raise RuntimeError("decode program: the persistent program does not take slot mode (its loop is one "
                                   "step index for the batch); slots run through admit() / run_steps()")
            raise RuntimeError("decode program: a slot-mode program runs through admit() / run_steps(), not decode()")
        if self.dry or self.refused:
            raise RuntimeError("decode program: the step kernels do not take this program (%s)" % (self.refused or "dry"))
        if self.per_item and stops is None:
            raise RuntimeError("decode program: per-utterance attention entries need the per-item stop rule (stops=)")
        if persistent is None:
            persistent = persistent_default
        if guide is not None:
            if persistent:
                raise RuntimeError("decode program: persistent=True does not take a guide (dv3_decode_program_run has no "
                                   "guided form); use the launched or Python-driven loop")
            if test_inputs is not None:
                raise RuntimeError("decode program: a guide and test_inputs (teacher forcing) are not combined")
            if not self.per_item or stops is None:
                raise RuntimeError("decode program: a guide needs per-utterance attention entries (key_len) and stops=")
            return self.decode_guided(cur_in, guide, stops, launched_default if launched is None else launched)
        if persistent:
            if stops is not None:
                raise RuntimeError("decode program: the persistent program does not take per-utterance decoding "
                                   "(its stop rule is one flag per batch); use the launched or Python-driven loop")
            return self.decode_persistent(cur_in, test_inputs, dones_seq, min_steps, max_steps)
        if launched is None:
            launched = launched_default
        if launched:
            return self.decode_launched(cur_in, test_inputs, dones_seq, min_steps, max_steps, stops=stops)
        free_running = test_inputs is None
        B = self.B
        graphed = bool(use_graph) and free_running
        graph, t = None, 0
        while True:
            if not free_running:
                if t >= test_inputs.size(1):
                    break
                cur_in.copy_(test_inputs[:, t, :].reshape(B, -1))
            if graphed and t >= 1:
                if graph is None:
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        self.run_step()
                graph.replay()
            else:
                self.run_step()
            t += 1
            if free_running and stops is not None:
                if item_stops([(dones_seq[t - 1].reshape(-1) > 0.5).tolist()], t - 1, min_steps, max_steps, stops):
                    break
            elif free_running:
                if t > min_steps and bool((dones_seq[t - 1] > 0.5).all()):
                    break
                elif t > max_steps:
                    break
        if stops is not None and not free_running:
            stops[:] = [t] * B
        return t


class StepTrace(object):
    """Per-step results of the module-by-module decode loops (the configurations the step program does not take):
    each step's (B, 1, .) tensors are copied into stacked (B, capacity, .) buffers that double when full -- the host-side
    shape of what the step program writes on the device -- so the loops end with three slices instead of three lists of
    per-step tensors to squeeze, stack and transpose.  `stop` is the reference's rule (deepvoice3.py:469-473)."""

    def __init__(self, min_steps, max_steps, teacher_forced, stops=None):
        self.min_steps, self.max_steps, self.teacher_forced = min_steps, max_steps, teacher_forced
        self.stops = stops            # per-utterance mode: a list of B zeros, each item's step count once it stopped
        self.n = 0
        self.dones = []
        self._bufs = None

    def _room(self, parts):
        if self._bufs is None:
            cap = 64
            self._bufs = [p.new_empty((p.size(0), cap) + tuple(p.shape[2:])) for p in parts]
        elif self.n == self._bufs[0].size(1):
            self._bufs = [torch.cat((b, torch.empty_like(b)), dim=1) for b in self._bufs]

    def push(self, output, alignment, state, done):
        parts = (output, alignment, state)
        self._room(parts)
        for b, p in zip(self._bufs, parts):
            b[:, self.n:self.n + 1].copy_(p)
        self.dones.append(done)
        self.n += 1

    @property
    def last_output(self):
        return self._bufs[0][:, self.n - 1:self.n].contiguous()

    def stop(self, done):
        """after push: the free-running loop ends once every item signalled done past min_steps, or past max_steps"""
        if self.teacher_forced:
            if self.stops is not None:
                self.stops[:] = [self.n] * len(self.stops)
            return False
        if self.stops is not None:
            return item_stops([(done.reshape(-1) > 0.5).tolist()], self.n - 1, self.min_steps, self.max_steps,
                              self.stops)
        return bool((done > 0.5).all() and self.n > self.min_steps) or self.n > self.max_steps

    def result(self):
        out, ali, st = (b[:, :self.n] for b in self._bufs)
        return out.contiguous(), ali, self.dones, st.contiguous()


class RollingSchedule(object):
    """The host-side book of rolling admission: which ticket sits in which batch slot since which global step.  A pure
    host object (no GPU, no model).  One round (RollingSynthesizer.poll) is
        admit()          queued tickets, first in first out, into the free slots in ascending slot order; each gets
                         t_off = the current global step;
        advance(chunk)   every slot runs `chunk` decoder steps (idle ones included: a decode step costs the same at
                         any occupancy -- that is the point of refilling them);
        retire(slot)     for every slot whose utterance has stopped within the steps it has run.
    steps counts the decoder steps executed; log keeps (ticket, slot, t_off, retired_at) per retired ticket."""

    def __init__(self, slots, chunk=8):
        if slots < 1 or chunk < 1:
            raise ValueError("RollingSchedule: slots and chunk must be positive")
        self.n_slots, self.chunk = int(slots), int(chunk)
        self.t = 0                                   # global step
        self.steps = 0                               # decoder steps executed
        self.queue = []                              # tickets waiting, FIFO
        self.slot_ticket = [None] * self.n_slots
        self.slot_t_off = [0] * self.n_slots
        self.log = []

    def submit(self, ticket):
        self.queue.append(ticket)

    def busy(self):
        return [s for s in range(self.n_slots) if self.slot_ticket[s] is not None]

    def pending(self):
        return bool(self.queue) or any(t is not None for t in self.slot_ticket)

    def admit(self):
        """-> [(ticket, slot)] admitted now"""
        out = []
        for s in range(self.n_slots):
            if not self.queue:
                break
            if self.slot_ticket[s] is None:
                tk = self.queue.pop(0)
                self.slot_ticket[s], self.slot_t_off[s] = tk, self.t
                out.append((tk, s))
        return out

    def advance(self, n=None):
        n = self.chunk if n is None else int(n)
        self.t += n
        self.steps += n
        return n

    def steps_run(self, slot):
        """decoder steps the slot's utterance has run"""
        return self.t - self.slot_t_off[slot]

    def retire(self, slot):
        tk = self.slot_ticket[slot]
        if tk is None:
            raise RuntimeError("RollingSchedule: slot %d is free" % slot)
        self.slot_ticket[slot] = None
        self.log.append((tk, slot, self.slot_t_off[slot], self.t))
        return tk


def simulate_rolling(step_counts, slots, chunk=8):
    """decoder steps rolling admission executes for utterances that need step_counts[i] steps, submitted in that order
    before the first round -> (steps, the RollingSchedule with its log)"""
    sch = RollingSchedule(slots, chunk)
    for i, n in enumerate(step_counts):
        if n < 1:
            raise ValueError("simulate_rolling: every utterance needs at least one step")
        sch.submit(i)
    while sch.pending():
        sch.admit()
        sch.advance()
        for s in sch.busy():
            if sch.steps_run(s) >= step_counts[sch.slot_ticket[s]]:
                sch.retire(s)
    return sch.steps, sch


def simulate_waves(step_counts, slots, chunk=None):
    """decoder steps rigid waves of `slots` utterances execute: every wave runs until its slowest item has stopped
    (chunk: rounded up to whole chunks of steps, as a loop that reads the done flags once per chunk runs them;
    None: the exact maximum, the most favourable count for waves)"""
    total = 0
    for i in range(0, len(step_counts), slots):
        m = max(step_counts[i:i + slots])
        total += m if chunk is None else -(-m // chunk) * chunk
    return total


def cfg2_step_counts(n, seed, r=4, max_steps=None):
    """decoder steps of n utterances with LJSpeech-shaped lengths: mel frames ~ N(566, 180) clipped to
    [120, 870], steps = frames / r (optionally capped at max_steps)"""
    import numpy as np
    frames = np.clip(np.random.RandomState(seed).normal(566.0, 180.0, n), 120, 870)
    steps = np.maximum((frames / r).astype(np.int64), 1)
    if max_steps is not None:
        steps = np.minimum(steps, max_steps)
    return [int(v) for v in steps]
