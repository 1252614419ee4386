"""The target-duration rule of include/zerovox_amd.h ("target durations") restated with Python's unbounded integers, for
tests/test_fit_durations_cpu.py (against csrc/fit_durations.h) and tests/test_gpu_fit_durations.py (against the device)."""
import math

import numpy as np

WEIGHT_MAX = 1 << 40


def weight(dur):
    """q of one f32 duration: dur * 65536 truncated (the product of an f32 and 2^16 is exact in a double), capped at 2^40"""
    x = float(np.float32(dur))
    if not x > 0.0:                      # NaN, zero, negative
        return 0
    w = x * 65536.0
    return WEIGHT_MAX if w >= float(WEIGHT_MAX) else int(math.floor(w))


def scaled_dur(logdur, uscale=None, scale=None):
    """steps 1-3 of the header's per-phoneme duration rule, f32, every step rounded separately (restate_durations' arithmetic)"""
    with np.errstate(over="ignore", invalid="ignore"):
        dur = (np.exp(np.asarray(logdur, np.float32).astype(np.float64)) - 1.0).astype(np.float32)
        if uscale is not None:
            dur = (dur * np.float32(uscale)).astype(np.float32)
        if scale is not None:
            dur = (dur * np.asarray(scale, np.float32)).astype(np.float32)
    return dur


def fit(dur, forced, num_phonemes, T, target):
    """d[i] for the n = len(dur) tokens; forced: sequence of frame counts (-1 = free) or None"""
    n = len(dur)
    nw = max(0, min(int(num_phonemes), n))
    d = [0] * n
    free, Fs = [], 0
    for i in range(nw):
        if forced is not None and int(forced[i]) >= 0:
            d[i] = min(int(forced[i]), T)
            Fs += d[i]
        else:
            free.append(i)
    R = target - Fs
    if R <= 0 or not free:
        return np.array(d, np.int64)
    q = {i: weight(dur[i]) for i in free}
    Q = sum(q.values())
    if Q == 0:
        q = {i: 1 for i in free}
        Q = len(free)
    rem = {}
    for i in free:
        d[i], rem[i] = divmod(q[i] * R, Q)
    L = R - sum(d[i] for i in free)
    assert 0 <= L < len(free)
    for i in sorted(free, key=lambda i: (-rem[i], i))[:L]:
        d[i] += 1
    return np.array(d, np.int64)
