# coding: utf-8
"""No GPU: every exported dv3_* entry point of include/dv3hip.h is exercised by the suite.  Each name must
  (1) appear in the text of some tests/*.py, or
  (2) stand in VIA = {symbol: (wrapper, ...)}: the wrapper's name appears in a test file and the wrapper's source in
      deepvoice3_pytorch_amd/ names the symbol -- where the public wrapper goes through an autograd Function or a
      private helper, the chain is spelled out: each link's source names the next link, the last one's the symbol, or
  (3) stand in EXEMPT = {symbol: reason}: entry points that launch no arithmetic or data-movement kernel of their own
      (graph and stream plumbing, size queries), or that nothing in the package calls.
An entry point added to the header without a test fails here."""
import glob
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIA = {
    "dv3_gather_spans_f32": ("audio.gather_spans",),
    "dv3_item_gain_f32": ("audio.item_gains",),
    "dv3_bce_loss_items_f32": ("ops.bce_loss_items",),
    "dv3_spec_loss_items_f32": ("ops.spec_loss_items",),
    "dv3_guided_attn_loss_items_f32": ("ops.guided_attention_loss_items",),
    "dv3_guided_attn_loss_f32": ("ops.guided_attention_loss", "ops.GuidedAttnLossFn"),
    "dv3_guided_attn_loss_valid_f32": ("ops.guided_attention_loss", "ops.GuidedAttnLossFn"),
    "dv3_conv_streamk_ws_bytes": ("ops._streamk_ws",),
    "dv3_embedding_bct_f32": ("ops.embedding_bct", "ops.EmbeddingBCTFn"),
    "dv3_embedding_bct_bwd_f32": ("ops.embedding_bct", "ops.EmbeddingBCTFn"),
    "dv3_to_c8_f32": ("ops.to_c8", "ops._ToC8Fn"),
    "dv3_from_c8_f32": ("ops.from_c8", "ops._FromC8Fn", "ops._from_c8_raw"),
    "dv3_grad_sqnorm_f32": ("ops.grad_sqnorm",),
    "dv3_mask_bits_to_c8": ("ops.mask_bits_to_c8",),
    "dv3_sincos_pos_bct_f32": ("ops.sincos_pos_bct",),
    "dv3_sincos_pos_bwd2_f32": ("ops.add_position_encoding", "ops._PosEncFn"),
    "dv3_sincos_pos_table_bwd_f32": ("ops.add_position_encoding", "ops._PosEncFn"),
}

EXEMPT = {
    "dv3_graph_side_begin": "graph capture plumbing: launches no kernel of its own",
    "dv3_graph_side_end": "graph capture plumbing: launches no kernel of its own",
    "dv3_graph_launch": "replays a captured graph: launches no kernel of its own",
    "dv3_graph_destroy": "frees a captured graph",
    "dv3_stream_fork": "event record / wait between two streams",
    "dv3_flag_signal": "a one-word flag ordering two streams inside captured segments: no arithmetic, no data movement",
    "dv3_flag_wait": "the wait on that flag: no arithmetic, no data movement",
    "dv3_ring_standin": "a measurement stand-in for a ring all-reduce: reduces nothing, not on the product path",
    "dv3_loss_items_scratch_floats": "a size query",
    "dv3_sincos_pos_bwd_f32": "nothing in the package calls it (superseded by dv3_sincos_pos_bwd2_f32)",
}


def _exported():
    from deepvoice3_pytorch_amd import _lib
    return sorted(_lib.FUNCS)


def _test_text():
    return "\n".join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")))
                     if os.path.basename(p) != os.path.basename(__file__))


def _wrapper_source(path):
    """the source of `module.attr[.attr]` under deepvoice3_pytorch_amd"""
    import importlib
    mod, _, rest = path.partition(".")
    obj = importlib.import_module("deepvoice3_pytorch_amd." + mod)
    for part in rest.split("."):
        obj = getattr(obj, part)
    return inspect.getsource(obj)


def test_every_entry_point_is_reached_by_a_test():
    text = _test_text()
    missing = []
    for sym in _exported():
        if re.search(r"\b%s\b" % sym, text):
            continue
        if sym in VIA:
            chain = VIA[sym]
            short = chain[0].split(".", 1)[1]
            assert re.search(r"\b%s\b" % re.escape(short), text), "%s: no test names its wrapper %s" % (sym, chain[0])
            for link, nxt in zip(chain, chain[1:] + (sym,)):
                assert re.search(r"\b%s\b" % re.escape(nxt.split(".")[-1]), _wrapper_source(link)), \
                    "%s: the source of %s does not name %s" % (sym, link, nxt)
            continue
        if sym in EXEMPT:
            continue
        missing.append(sym)
    assert not missing, "entry points no test reaches (add a test, or a VIA / EXEMPT line with its reason): %s" % missing


def test_the_tables_hold_nothing_stale():
    exported = set(_exported())
    text = _test_text()
    for table in (VIA, EXEMPT):
        for sym in table:
            assert sym in exported, "%s is no entry point of the header" % sym
            assert not re.search(r"\b%s\b" % sym, text), "%s is named by a test: drop its line" % sym
    assert not set(VIA) & set(EXEMPT)
