# coding: utf-8
"""Weight averaging without a GPU: the decay rule, the float64 reference of tests/ema_ref.py against
the closed form, and what a CPU Trainer does with the average around it -- the arena buffer, averaged(), the
checkpoint key and export_averaged.  (The update itself runs in the fused clip + Adam kernel: tests/test_gpu_ema.py.)"""
import numpy as np
import pytest
import torch

from tests import ema_ref as R

HP = dict(n_vocab=20, embed_dim=16, mel_dim=8, linear_dim=9, r=1, downsample_step=4, padding_idx=0, dropout=0.0,
          kernel_size=3, encoder_channels=16, decoder_channels=16, converter_channels=16, max_positions=32)


def _trainer(seed=0, **kw):
    from deepvoice3_pytorch_amd import builder, train_step
    split = {k: kw.pop(k) for k in ("train_seq2seq", "train_postnet") if k in kw}
    torch.manual_seed(seed)
    return train_step.Trainer(builder.deepvoice3(**HP), train_step.TrainConfig(max_positions=32, **kw), **split)


def _fill_average(tr, seed=5):
    g = torch.Generator().manual_seed(seed)
    tr.arena.ema.copy_(torch.randn(tr.arena.total, generator=g))


# ----------------------------------------------------------------------------------------------------------------
def test_decay_rule():
    from deepvoice3_pytorch_amd import train_step
    for fn in (R.decay_at, train_step.ema_decay_at):
        assert fn(1, 0.999) == 2.0 / 11.0
        d = [fn(t, 0.999) for t in range(1, 20001)]
        assert all(b >= a for a, b in zip(d, d[1:]))
        # (1 + t) / (10 + t) reaches 0.999 at t = 8990
        assert d[8988] < 0.999 and all(x == 0.999 for x in d[8989:])
        assert all(x == (1.0 + t) / (10.0 + t) for t, x in enumerate(d[:8989], 1))
        assert all(fn(t, 0.9, False) == 0.9 for t in (1, 2, 10, 10 ** 6))
        assert fn(8, 0.9) == 0.5 and fn(80, 0.9) == 0.9 and fn(81, 0.9) == 0.9
    for t in (1, 5, 79, 80, 81, 12345):
        for d in (0.5, 0.9, 0.9999):
            for w in (True, False):
                assert train_step.ema_decay_at(t, d, w) == R.decay_at(t, d, w)


def test_config_validates_the_decay():
    from deepvoice3_pytorch_amd import train_step
    c = train_step.TrainConfig()
    assert c.ema_decay == 0.0 and c.ema_warmup is True
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            train_step.TrainConfig(ema_decay=bad)
    assert train_step.TrainConfig(ema_decay=0.999, ema_warmup=False).ema_warmup is False


def test_reference_recursion_against_the_closed_form():
    """a constant parameter: e_n = p + (e_0 - p) prod d_t"""
    rng = np.random.RandomState(0)
    p, e0 = rng.randn(64), rng.randn(64)
    for decay, warm in ((0.9, True), (0.999, True), (0.9, False)):
        e, prod = e0.copy(), 1.0
        for t in range(1, 201):
            d = R.decay_at(t, decay, warm)
            e = R.update(e, p, 1.0 - d)
            prod *= d
            want = p + (e0 - p) * prod
            assert np.abs(e - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (decay, warm, t)
    # the end points of one update
    assert np.array_equal(R.update(e0, p, 0.0), e0)
    assert np.abs(R.update(e0, p, 1.0) - p).max() <= 1e-15
    assert np.array_equal(R.bound(np.float32([1.0, -4.0]), np.float32([-2.0, 0.5])), 4 * R.U * np.array([2.0, 4.0]))


# ----------------------------------------------------------------------------------------------------------------
def test_averaging_off_changes_nothing():
    from deepvoice3_pytorch_amd import train_step
    tr = _trainer()
    assert tr.arena.ema is None and not tr.ema_on
    assert sorted(train_step.checkpoint_dict(tr)) == ["global_epoch", "global_step", "optimizer", "state_dict"]
    with pytest.raises(ValueError):
        tr.evaluate(None, averaged=True)
    with pytest.raises(ValueError):
        with tr.averaged():
            pass
    with pytest.raises(ValueError):
        train_step.evaluate_loader(tr, [], averaged=True)
    with pytest.raises(ValueError):
        train_step.export_averaged(tr)
    # a file that carries an average loads into a trainer that keeps none: the key is ignored
    src = _trainer(seed=1, ema_decay=0.9)
    _fill_average(src)
    ck = train_step.checkpoint_dict(src)
    assert "ema_state_dict" in ck
    train_step.load_checkpoint(ck, tr)
    assert tr.arena.ema is None and torch.equal(tr.arena.flat, src.arena.flat)


def test_average_starts_as_the_weights_and_fourth_hyper_slot():
    tr = _trainer(ema_decay=0.9)
    a = tr.arena
    assert a.ema is not None and a.ema.data_ptr() != a.flat.data_ptr() and torch.equal(a.ema, a.flat)
    assert tr.hyper.numel() == 4 and all(h.numel() == 4 for h in tr._hyper_ring)
    for t in (1, 2, 3):
        tr._set_hyper()
        assert tr.adam_step == t
        assert float(tr.hyper[3]) == float(np.float32(1.0 - R.decay_at(t, 0.9)))
    off = _trainer()
    off._set_hyper()
    assert off.hyper.numel() == 4 and float(off.hyper[3]) == 0.0


def test_checkpoint_round_trip_reseed_and_mismatch(tmp_path):
    from deepvoice3_pytorch_amd import train_step
    tr = _trainer(ema_decay=0.9)
    _fill_average(tr)
    tr.adam_step = 3
    path = train_step.save_checkpoint(tr, str(tmp_path))
    ck = train_step._load_file(path)              # the restricted unpickler takes the extra key
    assert sorted(ck) == ["ema_state_dict", "global_epoch", "global_step", "optimizer", "state_dict"]
    names = [n for n, p in tr.model.named_parameters() if any(p is q for q in tr.arena.params)]
    assert list(ck["ema_state_dict"]) == names and set(names) <= set(ck["state_dict"])
    for n, p in tr.model.named_parameters():
        if n in ck["ema_state_dict"]:
            assert ck["ema_state_dict"][n].shape == p.shape
    t2 = _trainer(seed=1, ema_decay=0.9)
    train_step.load_checkpoint(path, t2)
    for o, n in zip(tr.arena.offsets, tr.arena.sizes):       # (the alignment pads are not state)
        assert torch.equal(t2.arena.ema[o:o + n], tr.arena.ema[o:o + n])
        assert torch.equal(t2.arena.flat[o:o + n], tr.arena.flat[o:o + n])
    # no key (the reference's file, a run without averaging): the average starts again from the loaded weights
    t3 = _trainer(seed=2, ema_decay=0.9)
    _fill_average(t3, seed=9)
    plain = {k: v for k, v in ck.items() if k != "ema_state_dict"}
    train_step.load_checkpoint(plain, t3)
    assert torch.equal(t3.arena.flat, tr.arena.flat)
    for o, n in zip(tr.arena.offsets, tr.arena.sizes):
        assert torch.equal(t3.arena.ema[o:o + n], tr.arena.flat[o:o + n])
    # names or shapes that do not fit: refused, the keys named
    k0 = names[0]
    bad = dict(ck, ema_state_dict={k: v for k, v in ck["ema_state_dict"].items() if k != k0})
    with pytest.raises(RuntimeError, match=k0.replace(".", r"\.")):
        train_step.load_checkpoint(bad, _trainer(seed=3, ema_decay=0.9))
    bad = dict(ck, ema_state_dict=dict(ck["ema_state_dict"], nonsense=torch.zeros(1)))
    with pytest.raises(RuntimeError, match="nonsense"):
        train_step.load_checkpoint(bad, _trainer(seed=3, ema_decay=0.9))
    bad = dict(ck, ema_state_dict=dict(ck["ema_state_dict"], **{k0: torch.zeros(3, 1, 1, 7)}))
    with pytest.raises(RuntimeError, match=k0.replace(".", r"\.")):
        train_step.load_checkpoint(bad, _trainer(seed=3, ema_decay=0.9))


def test_averaged_swaps_by_content_and_restores():
    from deepvoice3_pytorch_amd import ops, train_step
    tr = _trainer(ema_decay=0.9)
    _fill_average(tr)
    a = tr.arena
    raw, avg = a.flat.clone(), a.ema.clone()
    ptrs = (a.flat.data_ptr(), a.ema.data_ptr(), [p.data_ptr() for p in a.params])
    epoch = ops.param_epoch
    with tr.averaged() as same:
        assert same is tr and ops.param_epoch > epoch
        assert torch.equal(a.flat, avg) and torch.equal(a.ema, raw)
        for p, o, n in zip(a.params, a.offsets, a.sizes):           # the model's own parameters hold the average
            assert torch.equal(p.detach().reshape(-1), avg[o:o + n])
        assert ptrs == (a.flat.data_ptr(), a.ema.data_ptr(), [p.data_ptr() for p in a.params])
        with pytest.raises(RuntimeError, match="nest"):
            with tr.averaged():
                pass
        assert torch.equal(a.flat, avg)                  # the refused inner context exchanged nothing
        for call in (lambda: tr.step(None), tr.optimizer_step, lambda: train_step.checkpoint_dict(tr),
                     lambda: train_step.load_checkpoint({}, tr)):
            with pytest.raises(RuntimeError, match="averaged"):
                call()
        inside = ops.param_epoch
    assert ops.param_epoch > inside
    assert torch.equal(a.flat, raw) and torch.equal(a.ema, avg)
    # an exception inside still hands the raw weights back
    with pytest.raises(KeyError):
        with tr.averaged():
            raise KeyError("x")
    assert torch.equal(a.flat, raw) and torch.equal(a.ema, avg) and not tr._swapped


def test_export_averaged_loads_into_a_fresh_model(tmp_path):
    from deepvoice3_pytorch_amd import builder, train_step
    tr = _trainer(ema_decay=0.9)
    _fill_average(tr)
    tr.global_step = 17
    path = str(tmp_path / "averaged.pth")
    ck = train_step.export_averaged(tr, path, global_epoch=2)
    got = train_step._load_file(path)
    assert sorted(got) == ["global_epoch", "global_step", "optimizer", "state_dict"] and got["optimizer"] is None
    assert list(got["state_dict"]) == list(tr.model.state_dict()) and got["global_step"] == 17
    avg = tr.averaged_state()
    for k, v in tr.model.state_dict().items():
        assert torch.equal(got["state_dict"][k], avg[k] if k in avg else v), k
        assert torch.equal(ck["state_dict"][k], got["state_dict"][k])
    assert any(not torch.equal(got["state_dict"][k], tr.model.state_dict()[k]) for k in avg)
    # into a fresh trainer without its optimizer state ...
    t2 = _trainer(seed=4)
    assert train_step.load_checkpoint(path, t2, reset_optimizer=True) == 2
    assert t2.global_step == 17 and t2.adam_step == 0
    for p, o, n in zip(t2.arena.params, t2.arena.offsets, t2.arena.sizes):
        assert torch.equal(p.detach().reshape(-1), tr.arena.ema[o:o + n])
    # ... into a bare model (the reference's model.load_state_dict), and through restore_parts
    torch.manual_seed(6)
    m3 = builder.deepvoice3(**HP)
    m3.load_state_dict(got["state_dict"])
    m4 = builder.deepvoice3(**HP)
    restored, skipped = train_step.restore_parts(path, m4)
    assert not skipped and sorted(restored) == sorted(got["state_dict"])
    for m in (m3, m4):
        for k, v in m.state_dict().items():
            assert torch.equal(v, got["state_dict"][k]), k


def test_split_mode_average_covers_the_trained_part_only():
    from deepvoice3_pytorch_amd import train_step
    tr = _trainer(ema_decay=0.9, train_seq2seq=False)
    _fill_average(tr)
    s2s = [p.detach().clone() for p in tr.model.seq2seq.parameters()]
    assert tr.arena.total < sum(p.numel() for p in tr.model.parameters())
    ck = train_step.checkpoint_dict(tr)
    assert set(ck["ema_state_dict"]) <= set(tr.model.postnet.state_dict()) and set(ck["ema_state_dict"])
    with tr.averaged():
        for p, q in zip(tr.model.seq2seq.parameters(), s2s):
            assert torch.equal(p.detach(), q)
        for p, o, n in zip(tr.arena.params, tr.arena.offsets, tr.arena.sizes):
            assert torch.equal(p.detach().reshape(-1), tr.arena.flat[o:o + n])
    t2 = _trainer(seed=1, ema_decay=0.9, train_seq2seq=False)
    train_step.load_checkpoint(ck, t2)
    for o, n in zip(tr.arena.offsets, tr.arena.sizes):
        assert torch.equal(t2.arena.ema[o:o + n], tr.arena.ema[o:o + n])
