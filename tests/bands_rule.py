"""The band levels of include/zerovox_amd.h ("band levels") restated: exact integers for every sum, one float64 operation per step —
what csrc/bands.h and the two kernels must give bit for bit.  Independent of bands.h: nothing here is read from it but the frames
kernel's tile (tile_frames, for the GPU tests' capacities).

Re(k) and Im(k) are products of integer matrices whose entries are at most 8 191 and 126 in magnitude, every partial sum below 2^29:
float64 holds each of them exactly, so the matrix product runs in float64 (BLAS) and is converted to int64.  Powers, shifts and band
sums are Python integers."""
import math
import os
import re

import numpy as np

F = np.float32
N = 1024
BINS = N // 2 + 1
SCALE = 126
Q_MAX = 8191
SILENT = 0x33800000
NORM = 48774928.0
EQ_ONE = 274877906944.0          # 2^38
EQ_MAX = 1 << 47
DEFAULT_EDGES = (1, 3, 5, 8, 12, 17, 24, 33, 45, 62, 84, 114, 155, 210, 285, 387, 513)

_tables = None


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def products():
    """the table entries before rounding: (126 wnd cos, 126 wnd sin), float64 [513, 1024] each"""
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


def resolve(n_bands=0, edges=None):
    """(n_bands, edges) with the defaults filled in, or ValueError(field)"""
    if n_bands > 64:
        raise ValueError("n_bands")
    if edges is None and n_bands not in (0, 16):
        raise ValueError("edges")
    nb = n_bands or 16
    e = [int(x) for x in (DEFAULT_EDGES if edges is None else edges)][:nb + 1]
    if len(e) != nb + 1 or any(not a < b for a, b in zip(e, e[1:])) or e[nb] > BINS:
        raise ValueError("edges")
    return nb, e


def quantise(y):
    """(a int64 [..., 1024], k) of a span y float32 [1024], or (None, None) for a silent one"""
    y = np.where(np.isfinite(y), y, F(0)).astype(F)
    ab = bits(y) & np.uint32(0x7fffffff)
    pk = int(ab.max())
    if pk < SILENT:
        return None, None
    k = 12 - ((pk >> 23) - 127)
    mag = ab.view(F).astype(np.float64) * math.ldexp(1.0, k) + 0.5       # a product by a power of two, then one sum
    q = np.minimum(mag.astype(np.int64), Q_MAX)                         # truncation
    return np.where(bits(y) >> 31, -q, q).astype(np.int64), k


def spans(w, T, hop):
    """the T spans of the waveform w[0 .. T * hop), float32 [T, 1024], zeros outside the utterance"""
    n = T * hop
    pad = np.zeros(n + 2 * N, F)
    pad[N:N + n] = w
    s0 = np.arange(T, dtype=np.int64) * hop + hop // 2 - N // 2 + N
    return pad[s0[:, None] + np.arange(N)[None, :]]


def band_row(S, k):
    """(the row entry float32, Eq) of a band sum S (a Python integer) at the exponent k"""
    pw = (float(S) / NORM) * math.ldexp(1.0, -2 * k)
    v = pw * EQ_ONE + 0.5
    with np.errstate(over="ignore"):                                # (a level past the f32 range reads inf)
        return F(math.sqrt(pw)), (EQ_MAX if v >= float(EQ_MAX) else int(v))


def sums(a):
    """(Re, Im), int64 [513] each, of a quantised span"""
    C, S = tables()
    re = (C.astype(np.float64) @ a.astype(np.float64)).astype(np.int64)
    im = (S.astype(np.float64) @ a.astype(np.float64)).astype(np.int64)
    return re, im


def rule(w, T, hop, durations=None, n_bands=0, edges=None):
    """the whole rule for one utterance: dict(frames float32 [T, n_bands], phonemes float32 [n, n_bands] or None, Eq [T][n_bands])"""
    nb, e = resolve(n_bands, edges)
    w = np.asarray(w, F)
    assert w.shape == (T * hop,)
    C, S = tables()
    Cf, Sf = C.astype(np.float64), S.astype(np.float64)
    frames = np.zeros((T, nb), F)
    Eq = [[0] * nb for _ in range(T)]
    Y = spans(w, T, hop)
    live, A, K = [], [], []
    for f in range(T):
        a, k = quantise(Y[f])
        if a is not None:
            live.append(f)
            A.append(a)
            K.append(k)
    if live:
        Af = np.asarray(A, np.float64)
        Re = (Af @ Cf.T).astype(np.int64)
        Im = (Af @ Sf.T).astype(np.int64)
        assert np.abs(Re).max() < 1 << 29 and np.abs(Im).max() < 1 << 29
        Q = (Re * Re + Im * Im) >> 6                                       # below 2^59 before the shift: int64 holds it
        for j, f in enumerate(live):
            q = [int(x) for x in Q[j]]
            for b in range(nb):
                frames[f, b], Eq[f][b] = band_row(sum(q[e[b]:e[b + 1]]), K[j])
    phonemes = None
    if durations is not None:
        phonemes = np.zeros((len(durations), nb), F)
        start = 0
        for i, d in enumerate(int(x) for x in durations):
            d = max(d, 0)
            for b in range(nb):
                tot = sum(Eq[f][b] for f in range(start, min(start + d, T)))
                phonemes[i, b] = F(math.sqrt(float(tot) / (float(d) * EQ_ONE))) if d > 0 else F(0)
            start += d
    return dict(frames=frames, phonemes=phonemes, Eq=Eq, n_bands=nb, edges=e)


def tile_frames():
    """BANDS_TILE_FRAMES of csrc/bands.h: the frames one workgroup of the frames kernel covers"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zerovox.cpp_amd", "csrc", "bands.h")
    with open(path) as f:
        return int(re.search(r"BANDS_TILE_FRAMES\s*=\s*(\d+)", f.read()).group(1))
