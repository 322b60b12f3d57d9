# coding: utf-8
"""Float64 restatement of the per-item loss reductions (ops.spec_loss_items, ops.bce_loss_items,
ops.guided_attention_loss_items), written from their definitions:

  spec    item b, n_b = max(lengths[b] - r, 0) frames: S1 = sum |y_hat[b, t, d] - y[b, t + r, d]|,
          Sz = sum z,  z = -y L + log1p(exp(L)),  L = log(y_hat + 1e-8) - log(1 - y_hat + 1e-8)  (train.py:537-556),
          cnt = n_b D;   over t < n_b and every d
  bce     S = sum_{t < lengths[b]} -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)),  cnt = lengths[b]
  guided  S = sum_{l, t < T_b, n < N_b} attn[l, b, t, n] W[t, n],  W = 1 - exp(-(n / N_b - t / T_b)^2 / (2 g^2)) stored
          as float32 (train.py:585-591),  cnt = L T_b N_b

Plain numpy on the fp32 inputs widened to float64.  tests/test_cpu_item_losses_ref.py pins these against the oracle's
batch losses; tests/test_gpu_item_losses.py and tests/test_gpu_evaluate.py hold the kernels to them."""
import numpy as np

EPS = 1e-8


def spec_items(y_hat, y, lengths, r):
    """y_hat, y (B, T, D); lengths (B,) ints -> (B, 3) float64 {S1, Sz, cnt}"""
    y_hat, y = np.asarray(y_hat, dtype=np.float64), np.asarray(y, dtype=np.float64)
    B, T, D = y_hat.shape
    out = np.zeros((B, 3))
    for b in range(B):
        n = max(min(int(lengths[b]), T) - r, 0)
        if n == 0:
            continue
        a, t = y_hat[b, :n], y[b, r:r + n]
        logit = np.log(a + EPS) - np.log(1.0 - a + EPS)
        z = -t * logit + np.log1p(np.exp(logit))
        out[b] = np.abs(a - t).sum(), z.sum(), n * D
    return out


def bce_items(p, t, lengths):
    """p, t (B, T) or (B, T, 1) -> (B, 2) float64 {S, cnt}"""
    p, t = np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.float64)
    B = p.shape[0]
    p, t = p.reshape(B, -1), t.reshape(B, -1)
    out = np.zeros((B, 2))
    for b in range(B):
        n = min(max(int(lengths[b]), 0), p.shape[1])
        x, y = p[b, :n], t[b, :n]
        with np.errstate(divide="ignore"):
            e = -(y * np.maximum(np.log(x), -100.0) + (1.0 - y) * np.maximum(np.log(1.0 - x), -100.0))
        out[b] = e.sum(), n
    return out


def guided_items(attn, in_len, out_len, g):
    """attn (L, B, Tq, Tk) -> (B, 2) float64 {S, cnt}"""
    attn = np.asarray(attn, dtype=np.float64)
    L, B, Tq, Tk = attn.shape
    out = np.zeros((B, 2))
    for b in range(B):
        N, T = int(in_len[b]), int(out_len[b])
        Nc, Tc = min(max(N, 0), Tk), min(max(T, 0), Tq)
        if Nc == 0 or Tc == 0:
            continue
        n = np.arange(Nc, dtype=np.float64)[None, :]
        t = np.arange(Tc, dtype=np.float64)[:, None]
        W = (1.0 - np.exp(-(n / N - t / T) ** 2 / (2.0 * g * g))).astype(np.float32).astype(np.float64)
        out[b] = (attn[:, b, :Tc, :Nc] * W[None]).sum(), L * Tc * Nc
    return out
