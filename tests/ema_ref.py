# coding: utf-8
"""float64 restatement of the weight averaging: the decay rule and one update of the average.  Written
from the definitions, not from the package's code; tests/test_cpu_ema_ref.py checks it against a closed form and
tests/test_gpu_ema.py checks the kernel and the trainer against it."""
import numpy as np

# one fp32 rounding, relative (round to nearest: half an ulp)
U = 2.0 ** -24


def decay_at(t, ema_decay, warmup=True):
    """d_t of optimiser step t = 1, 2, ...: min(ema_decay, (1 + t) / (10 + t)) with warm-up (the num_updates rule of
    tf.train.ExponentialMovingAverage), ema_decay without"""
    d = float(ema_decay)
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def update(e, p, one_minus_d):
    """e' = e + (1 - d) (p - e) in float64; e, p arrays of any float type"""
    e = np.asarray(e, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    return e + float(one_minus_d) * (p - e)


def bound(e, p):
    """element-wise bound on |fp32 update - float64 update| when both start from the same fp32 e, p and the same fp32
    1 - d: three roundings (the subtraction, the product with 1 - d <= 1, the sum), each at most U relative to a
    quantity no larger than 2 max(|e|, |p|) resp. max(|e|, |p|) -- 4 U max(|e|, |p|); an FMA drops one of them"""
    return 4.0 * U * np.maximum(np.abs(np.asarray(e, dtype=np.float64)), np.abs(np.asarray(p, dtype=np.float64)))
