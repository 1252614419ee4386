"""Mel analysis of include/zerovox_amd.h ("mel analysis") restated: exact integers for every sum, one float64 operation per step —
what csrc/mel.h and the two kernels must give bit for bit.  Independent of mel.h: nothing here is read from it but the frames kernel's
tile (tile_frames, for the GPU tests' lengths).

The digit sums are products of integer matrices whose entries are at most 64 in magnitude, every partial sum below 2^23: float64 holds
each of them exactly, so the matrix products run in float64 (BLAS) and are converted to int64.  Behind them every step is one numpy
float64 operation over whole arrays, which rounds each element exactly as the scalar operation does."""
import math
import os
import re
import struct

import numpy as np

F = np.float32
N = 1024
BINS = N // 2 + 1
SCALE = 8188
Q_MAX = 8191
SILENT = 0x33800000              # 2^-24
FLOOR = np.array([0x2edbe6ff], np.uint32).view(F)[0]      # 1e-10f


def _f64(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


SQRT_HALF = _f64(0x3fe6a09e667f3bcd)
LN2 = _f64(0x3fe62e42fefa39ef)
LOG10E = _f64(0x3fdbcb7b1526e50e)
ODD = [1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0]      # (a correctly rounded quotient IS the nearest float64)

_tables = None


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def products():
    """the table entries before rounding: (8188 w cos, 8188 w sin), float64 [513, 1024] each"""
    kt = (np.arange(BINS, dtype=np.int64)[:, None] * np.arange(N, dtype=np.int64)[None, :]) % N
    ang = 2.0 * np.pi * kt / N
    w = SCALE * window()[None, :]
    return w * np.cos(ang), w * np.sin(ang)


def tables():
    """(C, S), int64 [513, 1024] each"""
    global _tables
    if _tables is None:
        pc, ps = products()
        _tables = (np.floor(pc + 0.5).astype(np.int64), np.floor(ps + 0.5).astype(np.int64))
    return _tables


def digits(a):
    """(hi, lo) of int64 values: a = 128 hi + lo, the shift a floor"""
    hi = (a + 64) >> 7
    return hi, a - 128 * hi


def spans(x, T, hop, centre, pad):
    """the T spans of x[0 .. T * hop), float32 [T, 1024]: zeros (pad 0) or the reflection (pad 1) outside, non-finite samples +0.0"""
    S = T * hop
    idx = (np.arange(T, dtype=np.int64) * hop + centre - N // 2)[:, None] + np.arange(N, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < S)
    if pad:
        assert S >= BINS
        idx = np.where(idx < 0, -idx, np.where(idx >= S, 2 * (S - 1) - idx, idx))
        assert ((idx >= 0) & (idx < S)).all()
        y = x[idx]
    else:
        y = np.where(inside, x[np.clip(idx, 0, S - 1)], F(0))
    return np.where(np.isfinite(y), y, F(0)).astype(F)


def quantise(y):
    """(a int64 [1024], k) of a span y float32 [1024] (finite), or (None, 0) for a silent one"""
    ab = bits(y) & np.uint32(0x7fffffff)
    pk = int(ab.max())
    if pk < SILENT:
        return None, 0
    k = 12 - ((pk >> 23) - 127)
    mag = ab.view(F).astype(np.float64) * math.ldexp(1.0, k) + 0.5       # a product by a power of two, then one sum
    q = np.minimum(mag.astype(np.int64), Q_MAX)                         # truncation
    return np.where(bits(y) >> 31, -q, q).astype(np.int64), k


def magnitudes(x, T, hop, centre=0, pad=0):
    """g float64 [T, 513] of the waveform x[0 .. T * hop)"""
    C, S = tables()
    planes = [[d.astype(np.float64) for d in digits(t)] for t in (C, S)]      # [cos, sin][hi, lo]
    Y = spans(np.asarray(x, F), T, hop, centre, pad)
    g = np.zeros((T, BINS), np.float64)
    for f in range(T):
        a, k = quantise(Y[f])
        if a is None:
            continue
        hi, lo = (d.astype(np.float64) for d in digits(a))
        tot = []
        for chi, clo in planes:
            a2 = (chi @ hi).astype(np.int64)
            a1 = (clo @ hi).astype(np.int64) + (chi @ lo).astype(np.int64)
            a0 = (clo @ lo).astype(np.int64)
            assert max(np.abs(a2).max(), np.abs(a1).max(), np.abs(a0).max()) <= 1 << 23
            tot.append(16384 * a2 + 128 * a1 + a0)
        assert max(np.abs(tot[0]).max(), np.abs(tot[1]).max()) < 1 << 37
        r, i = tot[0].astype(np.float64), tot[1].astype(np.float64)
        p = r * r
        q = i * i
        p = p + q
        m = np.sqrt(p)
        m = m * math.ldexp(1.0, -k)
        g[f] = m / float(SCALE)
    return g


def ln(v):
    """L of the header for positive normal float64 values: a fixed sequence of float64 steps, not libm's logarithm"""
    m, e = np.frexp(np.asarray(v, np.float64))
    low = m < SQRT_HALF
    m = np.where(low, m * 2.0, m)
    e = np.where(low, e - 1, e)
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    poly = np.full_like(z, ODD[0])
    for c in ODD[1:] + [1.0]:
        poly = poly * z
        poly = poly + c
    lnm = 2.0 * s
    lnm = lnm * poly
    r = e.astype(np.float64) * LN2
    return r + lnm


def level(acc, floor=0.0, log=0):
    fl = FLOOR if F(floor) == 0 else F(floor)
    v = np.maximum(acc, float(fl))
    with np.errstate(over="ignore"):
        if log == 2:
            return v.astype(F)
        r = ln(v)
        if log == 0:
            r = r * LOG10E
        return r.astype(F)


def channels(g, W):
    """acc float64 [T, M]: per channel +0.0, then the bins in ascending order, one multiply and one add each"""
    W = np.asarray(W, F).astype(np.float64)
    acc = np.zeros((g.shape[0], W.shape[0]), np.float64)
    for k in range(BINS):
        t = W[None, :, k] * g[:, k, None]
        acc = acc + t
    return acc


def rule(x, T, hop, W, centre=0, pad=0, log=0, floor=0.0):
    """the whole rule for one utterance: float32 [T, M]; W float32 [M, 513]"""
    x = np.asarray(x, F)
    assert x.shape == (T * hop,)
    return level(channels(magnitudes(x, T, hop, centre, pad), W), floor, log)


def tile_frames():
    """MEL_TILE_FRAMES of csrc/mel.h: the frames one workgroup of the frames kernel covers"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zerovox.cpp_amd", "csrc", "mel.h")
    with open(path) as f:
        return int(re.search(r"MEL_TILE_FRAMES\s*=\s*(\d+)", f.read()).group(1))
