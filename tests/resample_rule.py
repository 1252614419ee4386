"""The resampling rule of include/zerovox_amd.h ("resampling") restated in numpy, and the design evaluated in float64.

rule(table, M, x, ...) is the whole rule for one utterance: count, span, the polyphase sums in ascending tap order (a product of two
float32 values is exact in float64, so a step is one IEEE addition), the PCM16 conversion with its hash, the report.  The table is data:
the GPU tests hand it what capi.resample_design returned or random entries.  design() is the header's formula in float64 with this
file's own I0 series — the only place libm stands between it and the library's table."""
from types import SimpleNamespace

import numpy as np

F = np.float32
ZEROS, BETA, CUTOFF = 32, 9.0, 0.91
MASK = np.uint64(0xFFFFFFFF)


def fbits(v):
    return int(np.asarray(v, F).view(np.uint32))


def count(S_in, L, M):
    return (int(S_in) * int(L) + int(M) - 1) // int(M)


def ratio(rate_in, rate_out):
    g = int(np.gcd(rate_in, rate_out))
    return rate_out // g, rate_in // g


def dither(seed, n):
    """d of the rule for the outputs n (an integer array) under a seed: float64, exact"""
    n = np.asarray(n).astype(np.uint64) & MASK
    r = (np.uint64(seed & 0xFFFFFFFF) + n * np.uint64(0x9E3779B9)) & MASK
    r ^= r >> np.uint64(16)
    r = (r * np.uint64(0x7feb352d)) & MASK
    r ^= r >> np.uint64(15)
    r = (r * np.uint64(0x846ca68b)) & MASK
    r ^= r >> np.uint64(16)
    s = (r & np.uint64(0xFFFF)) + (r >> np.uint64(16))
    return (s.astype(np.float64) - 65535.0) * 2.0 ** -16


def pcm16(y, dithered=False, seed=0):
    """(int16 samples, clipped) of float32 outputs y[0 .. n)"""
    with np.errstate(over="ignore", invalid="ignore"):
        z = y.astype(np.float64) * 32768.0
        if dithered:
            z = z + dither(seed, np.arange(y.size, dtype=np.int64))
        z = z + 0.5
        nan = np.isnan(z)
        q = np.floor(np.where(nan, 0.0, z))
        clip = nan | (q > 32767.0) | (q < -32768.0)
        q = np.clip(q, -32768.0, 32767.0)
    return q.astype(np.int16), int(clip.sum())


def sample_peak(y):
    a = y.view(np.uint32) & np.uint32(0x7fffffff)
    a = np.where(a < np.uint32(0x7f800000), a, np.uint32(0))
    return np.uint32(a.max() if a.size else 0).view(F)


def sums(table, M, x):
    """y[0 .. n_out) of the rule, float32, and the (i0, p) of every output"""
    table = np.asarray(table, F)
    x = np.asarray(x, F)
    L, P = table.shape
    half = P // 2
    n = np.arange(count(x.size, L, M), dtype=np.int64)
    t = n * M
    i0, p = t // L, t % L
    xs = np.where(np.isfinite(x), x, F(0)).astype(np.float64)
    xp = np.concatenate([np.zeros(half - 1), xs, np.zeros(half)])      # x'[j] at j + half - 1
    h = table.astype(np.float64)
    acc = np.zeros(n.size)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(P):
            acc = acc + h[p, k] * xp[i0 + k]
        y = acc.astype(F)
    return y, i0, p


def rule(table, M, x, dithered=False, seed=0, pcm=True):
    """-> (result: n_out, clipped, sample_peak; y float32; q int16 or None; intermediates: i0, p, L, M, P, half)"""
    y, i0, p = sums(table, M, x)
    q, clipped = pcm16(y, dithered, seed) if pcm else (None, 0)
    L, P = np.asarray(table).shape
    res = SimpleNamespace(n_out=int(y.size), clipped=clipped, sample_peak=sample_peak(y))
    return res, y, q, SimpleNamespace(i0=i0, p=p, L=L, M=M, P=P, half=P // 2)


def key(res):
    return int(res.n_out), int(res.clipped), fbits(res.sample_peak)


def i0(v):
    h, t, s = v / 2.0, 1.0, 1.0
    for j in range(1, 1000):
        t = t * (h / j)
        term = t * t
        s = s + term
        if term < 1e-17 * s:
            break
    return s


def sizes(rate_in, rate_out, zeros=0):
    L, M = ratio(rate_in, rate_out)
    zeros = zeros or ZEROS
    half = -(-zeros * M // L) if M > L else zeros
    return L, M, 2 * half


def design(rate_in, rate_out, zeros=0, beta=0.0, cutoff=0.0):
    """(L, M, the table float64 [L, P]): every row divided by its own sum, NOT yet rounded to float32"""
    L, M, P = sizes(rate_in, rate_out, zeros)
    half = P // 2
    beta, cutoff = beta or BETA, cutoff or CUTOFF
    sc = (L / M if M > L else 1.0) * cutoff
    k, p = np.meshgrid(np.arange(P, dtype=np.int64), np.arange(L, dtype=np.int64))
    d = ((k - half + 1) * L - p).astype(np.float64) / float(L)
    w = np.maximum(1.0 - (d / half) ** 2, 0.0)
    win = np.vectorize(i0)(beta * np.sqrt(w)) / i0(beta)
    g = np.where(np.abs(d) > half, 0.0, sc * np.sinc(sc * d) * win)
    return L, M, g / g.sum(axis=1, keepdims=True)


def prototype(table):
    """the rows of a table [L, P] as ONE filter at L times the input rate: entry h[p][k] sits at time (k - half + 1) L - p"""
    table = np.asarray(table, np.float64)
    L, P = table.shape
    half = P // 2
    g = np.zeros(L * P)
    k, p = np.meshgrid(np.arange(P), np.arange(L))
    g[((k - half + 1) * L - p + half * L - 1).ravel()] = table.ravel()      # times -(half L - 1) .. half L
    return g


def response_db(table, M, nfft):
    """(level in dB at every bin of an nfft-point FFT of the prototype, the bin of the narrower Nyquist frequency): the prototype runs at
    L * rate_in, the narrower of the two rates is min(1, L / M) * rate_in, and the rows' DC gain of 1 is a gain of L of the prototype"""
    L = np.asarray(table).shape[0]
    H = np.abs(np.fft.rfft(prototype(table), nfft)) / L
    return 20.0 * np.log10(np.maximum(H, 1e-30)), nfft * min(1.0, L / M) / (2.0 * L)
