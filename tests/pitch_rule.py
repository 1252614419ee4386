"""The pitch track of include/zerovox_amd.h ("pitch track") restated: exact integers for every sum (numpy int64, far below 2^63), one
float64 operation per step, smallest lags for ties — what csrc/pitch.h and the two kernels must give bit for bit.  Independent of
pitch.h: nothing here is read from it but the frames kernel's chunk (chunk_frames, for the GPU tests' capacities)."""
import math

import numpy as np

F = np.float32
SILENT = 0x33800000


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def resolve(sr, hop, min_lag=0, max_lag=0, window=0, threshold=0.0):
    """the parameters with their defaults, or ValueError(field)"""
    lo = min_lag or sr // 441
    hi = max_lag or sr // 63
    W = window or 2 * hop
    thr = F(threshold) if F(threshold) != 0 else F(0.5)
    if not 8 <= lo < 512:
        raise ValueError("min_lag")
    if not (lo < hi <= 512 and hi <= 8 * lo):
        raise ValueError("max_lag")
    if not 64 <= W <= 1024:
        raise ValueError("window")
    if not (np.isfinite(thr) and 0 < thr <= 1):
        raise ValueError("voiced_threshold")
    return int(lo), int(hi), int(W), thr


def corr(c, E0, EL):
    if not (c > 0 and E0 > 0 and EL > 0):
        return 0.0
    r = float(c) / math.sqrt(float(E0 * EL))
    return r if r < 1.0 else 1.0


def frame(w, n, f, sr, hop, params):
    """((f0_hz, strength) as float32, Fq, voiced) of frame f of the waveform w[0 .. n)"""
    lo, hi, W, thr = params
    M = W + hi + 1
    s0 = f * hop + hop // 2 - M // 2
    y = np.zeros(M, F)
    a0, a1 = max(s0, 0), min(s0 + M, n)
    if a1 > a0:
        y[a0 - s0:a1 - s0] = w[a0:a1]
    y[~np.isfinite(y)] = 0
    ab = bits(y) & np.uint32(0x7fffffff)
    pk = int(ab.max())
    none = ((F(0), F(0)), 0, 0)
    if pk < SILENT:
        return none
    k = 9 - ((pk >> 23) - 127)
    mag = ab.view(F).astype(np.float64) * math.ldexp(1.0, k) + 0.5       # a product by a power of two, then one sum
    q = np.minimum(mag.astype(np.int64), 1023)                          # truncation
    a = np.where(bits(y) >> 31, -q, q).astype(np.int64)
    sq = np.concatenate([[0], np.cumsum(a * a)])
    E0 = int(sq[W])
    L = np.arange(lo - 1, hi + 2)
    E = sq[L + W] - sq[L]
    c = np.lib.stride_tricks.sliding_window_view(a, W)[lo - 1:hi + 2] @ a[:W]
    r = [corr(int(ci), E0, int(Ei)) for ci, Ei in zip(c, E)]
    at = lambda lag: r[lag - (lo - 1)]
    rmax = max(at(lag) for lag in range(lo, hi + 1))
    if rmax == 0.0:
        return none
    gate = 0.875 * rmax
    Ls = next(lag for lag in range(lo, hi + 1) if at(lag) >= gate)
    while Ls < hi and not at(Ls + 1) <= at(Ls):
        Ls += 1
    strength = at(Ls)
    p, nx = at(Ls - 1) - at(Ls), at(Ls + 1) - at(Ls)
    den = p + nx
    delta = 0.0
    if den < 0:
        delta = ((at(Ls - 1) - at(Ls + 1)) / den) * 0.5
        if not -0.5 <= delta <= 0.5:
            delta = 0.0
    f0 = float(sr) / (float(Ls) + delta)
    voiced = strength >= float(thr)
    return (F(f0) if voiced else F(0), F(strength)), (int(f0 * 256.0 + 0.5) if voiced else 0), int(voiced)


def phoneme_row(SF, nv, d):
    return (F(float(SF) / (float(nv) * 256.0)) if nv > 0 else F(0), F(float(nv) / float(d)) if d > 0 else F(0))


def rule(w, T, sr, hop, durations=None, min_lag=0, max_lag=0, window=0, threshold=0.0):
    """the whole rule for one utterance: dict(frames float32 [T, 2], phonemes float32 [n, 2] or None, Fq, voiced: per frame)"""
    params = resolve(sr, hop, min_lag, max_lag, window, threshold)
    w = np.asarray(w, F)
    assert w.shape == (T * hop,)
    frames = np.zeros((T, 2), F)
    Fq, V = [], []
    for f in range(T):
        frames[f], q, v = frame(w, T * hop, f, sr, hop, params)
        Fq.append(q)
        V.append(v)
    phonemes = None
    if durations is not None:
        phonemes = np.zeros((len(durations), 2), F)
        start = 0
        for i, d in enumerate(int(d) for d in durations):
            assert d >= 0 and start + d <= T
            phonemes[i] = phoneme_row(sum(Fq[start:start + d]), sum(V[start:start + d]), d)
            start += d
    return dict(frames=frames, phonemes=phonemes, Fq=Fq, voiced=V)


def chunk_frames(root):
    """PITCH_CHUNK_FRAMES of csrc/pitch.h: the frames one workgroup of the frames kernel covers"""
    import os
    import re
    m = re.search(r"constexpr int PITCH_CHUNK_FRAMES = (\d+);", open(os.path.join(root, "zerovox.cpp_amd", "csrc", "pitch.h")).read())
    return int(m.group(1))
