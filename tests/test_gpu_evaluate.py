# coding: utf-8
"""-m gpu: held-out evaluation (train_step.Trainer.evaluate) on the model fixtures of tests/golden with
their own inputs (plus linear targets, done flags and frame lengths made here):

  1. parity with the oracle's eval forward + train_losses, and of `items` with tests/item_losses_ref.py on the oracle's
     outputs (f32 and f16x3);
  2. no side effects: step, evaluate, step == step, step, bit for bit (Trainer and GraphedTrainer);
  3. after replayed steps evaluate sees the weights the replays wrote (bit-equal to a fresh model loaded from the
     trainer's checkpoint dict);
  4. a lattice-padded batch evaluates as the batch padded to its own maxima;
  5. in the bf16 mode and both split training modes evaluate runs and its rows recombine to its own scalars."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import dv3_oracle as O  # noqa: E402
from tests import item_losses_ref as R  # noqa: E402
from tests.util import load_golden, split_model_fixture  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = ["dv3_tiny", "nyanko_tiny", "dv3_multispeaker"]
# the eval-forward parity bar of tests/test_gpu_model.py for these fixtures (f32, f16x3 and bf16x3 alike): held here as
# |err| <= PARITY |want| on every scalar and every per-item sum (measured: test_evaluate_matches_the_oracle's docstring)
PARITY = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def gemm_mode(request):
    from deepvoice3_pytorch_amd import ops
    prev = ops.set_gemm_precision(request.param)
    yield request.param
    ops.set_gemm_precision(prev)


def _setup(name, dev, train_seq2seq=True, train_postnet=True, **cfg):
    """-> (trainer, batch, host dict): the fixture's model and inputs, targets of its shapes"""
    from deepvoice3_pytorch_amd import builder, train_step
    fx = load_golden("model_" + name)
    b, hp, sd, x = split_model_fixture(fx)
    model = getattr(builder, b)(**hp)
    model.load_state_dict(sd)
    model.to(dev)
    r, ds = hp["r"], hp.get("downsample_step", 1)
    rng = np.random.RandomState(17)
    B, Td = x["frame_positions"].shape
    T_lin = Td * r * ds
    tl = np.array([T_lin, T_lin - 2 * r * ds - 1, T_lin // 2])[:B]
    dl = tl // r // ds
    y = torch.from_numpy(rng.rand(B, T_lin, hp["linear_dim"]).astype(np.float32))
    done = torch.zeros(B, Td, 1)
    for i in range(B):
        done[i, max(int(dl[i]) - 1, 0):] = 1
    tc = train_step.TrainConfig(outputs_per_step=r, downsample_step=ds, max_positions=hp.get("max_positions", 512), **cfg)
    trainer = train_step.Trainer(model, tc, train_seq2seq=train_seq2seq, train_postnet=train_postnet)
    f = lambda t: t.to(dev) if t is not None else None
    batch = train_step.Batch(f(x["text"]), f(x["text_positions"]), f(x["frame_positions"]), f(x["mel"]), f(y), f(done),
                             x["input_lengths"].numpy(), tl, f(x.get("speaker_ids")), r, ds, dev)
    host = dict(b=b, hp=hp, sd=sd, x=x, y=y, done=done, tl=tl, dl=dl, r=r, ds=ds, fx=fx)
    return trainer, batch, host


def _floats(res):
    torch.cuda.synchronize()
    return {k: float(v) for k, v in res.items() if k != "items"}


def _bits(res):
    return {k: v.detach().cpu().numpy().copy() for k, v in res.items()}


def _same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, a[k], b[k])


# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gemm_mode", ["f32", "f16x3"], indirect=True)
@pytest.mark.parametrize("name", FIXTURES)
def test_evaluate_matches_the_oracle(dev, name, gemm_mode):
    """scalars against O.model_forward(drop=None) + O.train_losses, item rows against the restatement applied to the
    oracle's outputs; bound PARITY = 1e-4 relative per figure (the eval-forward bar of tests/test_gpu_model.py).
    Measured on an MI355X, worst over the three fixtures and both modes: 2.2e-7 (scalars), 2.5e-7 (item sums) -- the
    sums needed no wider bound than the forward's."""
    from deepvoice3_pytorch_amd import train_step
    trainer, batch, h = _setup(name, dev)
    try:
        res = trainer.evaluate(batch)
        assert all(v.is_cuda and not v.requires_grad for v in res.values())
        assert res["items"].shape == (batch.text.shape[0], len(train_step.EVAL_ITEM_COLUMNS))
        got = _floats(res)
        items = res["items"].cpu().numpy().astype(np.float64)
    finally:
        trainer.close()
    x, hp = h["x"], h["hp"]
    spec = O.build_spec(h["b"], **hp)
    il = x["input_lengths"].numpy()
    with torch.no_grad():
        out = O.model_forward(h["sd"], spec, x["text"], x["mel"], x.get("speaker_ids"), x["text_positions"],
                              x["frame_positions"], il, drop=None)
        c = trainer.cfg
        ohp = dict(outputs_per_step=h["r"], downsample_step=h["ds"], masked_loss_weight=c.masked_loss_weight,
                   binary_divergence_weight=c.binary_divergence_weight, use_guided_attention=True,
                   guided_attention_sigma=c.guided_attention_sigma)
        _, parts = O.train_losses(spec, ohp, out, x["mel"], h["y"], h["done"], il, h["tl"])
    names = dict(mel_l1_loss="mel_l1", mel_binary_div_loss="mel_bd", mel_loss="mel_loss", linear_l1_loss="lin_l1",
                 linear_binary_div_loss="lin_bd", linear_loss="lin_loss", done_loss="done_loss", attn_loss="attn_loss",
                 loss="loss")
    assert sorted(got) == sorted(names)
    worst = 0.0
    for k, ok in names.items():
        want = float(parts[ok])
        worst = max(worst, abs(got[k] - want) / abs(want))
    mel_out, lin_out, attn, done_hat = [t.numpy() for t in out]
    lin_len = h["tl"] if h["ds"] > 1 else h["dl"]
    want_items = np.concatenate([R.spec_items(mel_out, x["mel"].numpy(), h["dl"], h["r"]),
                                 R.spec_items(lin_out, h["y"].numpy(), lin_len, h["r"]),
                                 R.bce_items(done_hat, h["done"].numpy(), h["dl"]),
                                 R.guided_items(attn, il, h["dl"], c.guided_attention_sigma)], axis=1)
    cnt = [i for i, n in enumerate(train_step.EVAL_ITEM_COLUMNS) if n.endswith("cnt")]
    assert np.array_equal(items[:, cnt], want_items[:, cnt])
    nz = want_items != 0
    worst_items = float((np.abs(items - want_items)[nz] / np.abs(want_items)[nz]).max())
    print("evaluate vs oracle, %s %s: worst scalar %.3g, worst item sum %.3g" % (name, gemm_mode, worst, worst_items))
    assert np.array_equal(items[~nz], want_items[~nz])
    assert worst <= PARITY and worst_items <= PARITY, (worst, worst_items)


# ----------------------------------------------------------------------------------------------------------------
def _two_steps(dev, graphed, with_eval):
    from deepvoice3_pytorch_amd import ops, train_step
    ops.dropout_state.manual_seed(7)
    trainer, batch, _ = _setup("dv3_multispeaker", dev)
    runner = None
    try:
        if graphed:
            runner = train_step.GraphedTrainer(trainer, train_step.clone_batch(batch), warmup=1)
            stepper, step = runner, lambda: runner.step()
        else:
            stepper, step = trainer, lambda: trainer.step(batch)
        step()
        if with_eval:
            torch.cuda.synchronize()
            before = (trainer.global_step, trainer.adam_step, trainer._hyper_slot, ops.dropout_state.site,
                      ops.dropout_state.seed, ops.param_epoch, ops.mask_plan.plan, ops.mask_plan.last)
            grad = trainer.arena.grad.clone()
            assert trainer.model.training
            res = stepper.evaluate(batch)
            assert np.isfinite(float(res["loss"]))
            assert trainer.model.training and all(m.training for m in trainer.model.modules())
            assert before == (trainer.global_step, trainer.adam_step, trainer._hyper_slot, ops.dropout_state.site,
                              ops.dropout_state.seed, ops.param_epoch, ops.mask_plan.plan, ops.mask_plan.last)
            assert torch.equal(grad, trainer.arena.grad)
        scal = _bits(step())
        torch.cuda.synchronize()
        a = trainer.arena
        return scal, [t.detach().cpu().numpy().copy() for t in (a.flat, a.exp_avg, a.exp_avg_sq)]
    finally:
        if runner is not None:
            runner.close()
        trainer.close()


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_evaluate_between_two_steps_changes_nothing(dev, graphed):
    """from the same initial state and dropout seed (dropout 0.05 in the fixture): step, evaluate, step against step,
    step -- the second step's scalars, the parameters and both moments bit-equal"""
    s0, p0 = _two_steps(dev, graphed, with_eval=False)
    s1, p1 = _two_steps(dev, graphed, with_eval=True)
    _same_bits(s0, s1)
    for a, b in zip(p0, p1):
        assert np.array_equal(a, b)


def test_evaluate_raises_inside_a_capture(dev, monkeypatch):
    """evaluation is eager: asked for while the current stream is capturing, it refuses before it launches anything"""
    trainer, batch, _ = _setup("dv3_tiny", dev)
    try:
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="capture"):
            trainer.evaluate(batch)
        monkeypatch.undo()
        assert np.isfinite(float(trainer.evaluate(batch)["loss"]))
    finally:
        trainer.close()


# ----------------------------------------------------------------------------------------------------------------
def test_evaluate_after_replays_sees_the_replayed_weights(dev):
    from deepvoice3_pytorch_amd import builder, ops, train_step
    ops.dropout_state.manual_seed(3)
    trainer, batch, h = _setup("dv3_multispeaker", dev, lr_schedule=None, initial_learning_rate=1e-3)
    runner = train_step.GraphedTrainer(trainer, train_step.clone_batch(batch), warmup=1)
    try:
        first = _bits(runner.evaluate(batch))           # (fills the eval-mode packed-weight caches)
        for _ in range(3):
            runner.step()
        got = _bits(runner.evaluate(batch))
        ck = train_step.checkpoint_dict(trainer)
    finally:
        runner.close()
        trainer.close()
    assert not np.array_equal(first["loss"], got["loss"])
    model2 = getattr(builder, h["b"])(**h["hp"])
    model2.load_state_dict(ck["state_dict"])
    model2.to(dev)
    t2 = train_step.Trainer(model2, trainer.cfg)
    try:
        want = _bits(t2.evaluate(batch))
    finally:
        t2.close()
    _same_bits(got, want)


# ----------------------------------------------------------------------------------------------------------------
LHP = dict(n_vocab=30, embed_dim=32, mel_dim=16, linear_dim=17, r=1, downsample_step=4, padding_idx=0, dropout=0.0,
           kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32, use_memory_mask=False,
           force_monotonic_attention=False, use_decoder_state_for_postnet_input=True, key_projection=True,
           value_projection=True, max_positions=256)


@pytest.mark.parametrize("how", ["pad_to_shape", "device_collate_mask"])
def test_lattice_padded_batch_evaluates_as_the_batch_on_its_own_maxima(dev, how):
    """tolerance: that of tests/test_gpu_valid_lengths.py for the losses of a padded step in the f16x3 mode,
    2e-6 max(1, |figure|), on the scalars and on every entry of the item table"""
    from deepvoice3_pytorch_amd import builder, data, train_step
    hp = dict(LHP, use_memory_mask=(how == "device_collate_mask"))
    torch.manual_seed(0)
    model = builder.deepvoice3(**hp).to(dev)
    trainer = train_step.Trainer(model, train_step.TrainConfig(max_positions=256, outputs_per_step=1, downsample_step=4))
    rng = np.random.RandomState(11)
    items = []
    for tl, fl in ((20, 100), (25, 90), (13, 50), (22, 101)):
        text = np.concatenate([rng.randint(2, hp["n_vocab"], tl - 1), [1]]).astype(np.int32)
        items.append((text, rng.rand(fl, hp["mel_dim"]).astype(np.float32), rng.rand(fl, hp["linear_dim"]).astype(np.float32)))
    try:
        b0 = data.device_collate(data.pack_batch(items), dev, 1, 4)
        Tt, Td = b0.text.shape[1], b0.frame_positions.shape[1]
        if how == "pad_to_shape":
            t_in, t_dec = data.lattice_shape(Tt + 1, Td + 1, 16, 8)
            b1 = data.pad_to_shape(b0, t_in, t_dec, 15, 7)
        else:
            b1 = data.device_collate(data.pack_batch(items), dev, 1, 4, lattice=(16, 8))
        assert b1.valid is not None and b1.text.shape[1] > Tt and b1.frame_positions.shape[1] > Td
        r0, r1 = trainer.evaluate(b0), trainer.evaluate(b1)
        s0, s1 = _floats(r0), _floats(r1)
        i0, i1 = r0["items"].cpu().numpy().astype(np.float64), r1["items"].cpu().numpy().astype(np.float64)
        b1.valid = None
        s2 = _floats(trainer.evaluate(b1))
    finally:
        trainer.close()
    for k in s0:
        assert abs(s1[k] - s0[k]) <= 2e-6 * max(1.0, abs(s0[k])), (k, s0[k], s1[k])
    assert (np.abs(i1 - i0) <= 2e-6 * np.maximum(1.0, np.abs(i0))).all(), np.abs(i1 - i0).max()
    # ... and without the maxima the padded batch is another computation
    assert abs(s2["loss"] - s0["loss"]) > 1e-4 * abs(s0["loss"])


# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gemm_mode,name,part", [("bf16", "dv3_tiny", "both"), ("bf16", "dv3_multispeaker", "both"),
                                                 ("f16x3", "dv3_tiny", "seq2seq"), ("f16x3", "dv3_tiny", "postnet")],
                         indirect=["gemm_mode"])
def test_item_rows_recombine_to_the_batch_scalars(dev, gemm_mode, name, part):
    """with masked_loss_weight = 1 the trainer's own scalars ARE the batch kernels at w_masked = 1 on the outputs the
    item rows were taken from: sum S / sum cnt equals them within 1e-5 (tests/test_gpu_item_losses.py), whatever the
    GEMM mode and whichever part of the model ran.  (No parity across modes is claimed for bf16.)"""
    from deepvoice3_pytorch_amd import train_step
    trainer, batch, h = _setup(name, dev, train_seq2seq=part != "postnet", train_postnet=part != "seq2seq",
                               masked_loss_weight=1.0)
    try:
        res = trainer.evaluate(batch)
        got = _floats(res)
        items = res["items"].cpu().numpy().astype(np.float64)
    finally:
        trainer.close()
    col = {n: items[:, i] for i, n in enumerate(train_step.EVAL_ITEM_COLUMNS)}
    assert all(np.isfinite(v) for v in got.values()) and np.isfinite(items).all()
    close = lambda a, b: abs(a - b) <= 1e-5 * abs(b)
    s2s, pn = part != "postnet", part != "seq2seq"
    assert ("mel_loss" in got) == s2s and ("linear_loss" in got) == pn
    if s2s:
        assert close(col["mel_S1"].sum() / col["mel_cnt"].sum(), got["mel_l1_loss"])
        assert close(col["mel_Sz"].sum() / col["mel_cnt"].sum(), got["mel_binary_div_loss"])
        assert list(col["done_cnt"]) == list(h["dl"]) and (col["done_S"] > 0).all()
        L = h["fx"]["out/alignments"].shape[0]
        n_attn = L * batch.text.shape[0] * batch.frame_positions.shape[1] * batch.text.shape[1]
        assert close(col["attn_S"].sum() / n_attn, got["attn_loss"])
        assert list(col["attn_cnt"]) == [L * int(t) * int(n) for t, n in zip(h["dl"], batch.input_lengths_host)]
    else:
        assert not any(col[n].any() for n in ("mel_S1", "mel_Sz", "mel_cnt", "done_S", "done_cnt", "attn_S", "attn_cnt"))
    if pn:
        assert close(col["linear_S1"].sum() / col["linear_cnt"].sum(), got["linear_l1_loss"])
        assert close(col["linear_Sz"].sum() / col["linear_cnt"].sum(), got["linear_binary_div_loss"])
    else:
        assert not any(col[n].any() for n in ("linear_S1", "linear_Sz", "linear_cnt"))
