"""Loudness of include/zerovox_amd.h ("loudness") restated from the header's text: one float64 operation per step, over whole arrays of
chunks where the rule allows it (the 256 positions of a chunk are a loop, the chunks are the array) — what csrc/loudness.h and the
kernels must give bit for bit.  Independent of loudness.h: nothing here is read from it.

The design is DATA to the rule: rule() takes any object with the fields of zv_loudness_filter (capi.loudness_design, or the native
check's own), so libm never stands between two sets of bits.  design() is this file's own evaluation of the header's formulas, for the
tests of the design itself."""
import math
import struct
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import mel_rule as MR

F = np.float32
CHUNK = 256
TARGET, CEILING = 1, 2


def _f64(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


GATE_ABS = _f64(0x3e7f791ec6e1d5aa)          # 10^((-70 + 0.691) / 10)
TENTH = 0.1
OFFSET = -0.691
MIN_NORMAL = _f64(0x0010000000000000)


def dbits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def fbits(v):
    return int(np.array([v], F).view(np.uint32)[0])


# ---- 1. the design ------------------------------------------------------------------------------------------------------------------

def biquads(rate):
    fs = float(rate)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    sb = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    sa = [2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return sb, sa, [1.0, -2.0, 1.0], [2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def transition(sa, ha):
    """A: the zero-input transition of the cascade on (p1, p2, q1, q2)"""
    a1, a2, h1, h2 = sa[0], sa[1], ha[0], ha[1]
    return np.array([[-a1, 1.0, 0.0, 0.0], [-a2, 0.0, 0.0, 0.0], [-2.0 - h1, 0.0, -h1, 1.0], [1.0 - h2, 0.0, -h2, 0.0]], np.float64)


def fma(a, b, c):
    """IEEE fusedMultiplyAdd of float64 values: the exact rational a * b + c, rounded once (to nearest, ties to even)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def square(P):
    """P P, every entry the chain acc <- fma(P[i][k], P[k][j], acc), k = 0 .. 3, from +0.0"""
    C = np.empty((4, 4), np.float64)
    for i in range(4):
        for j in range(4):
            acc = 0.0
            for k in range(4):
                acc = fma(P[i, k], P[k, j], acc)
            C[i, j] = acc
    return C


def interpolator():
    c = np.zeros(49, F)
    for j in range(49):
        t = (j - 24.0) / 4.0
        sinc = 1.0 if j == 24 else math.sin(math.pi * t) / (math.pi * t)
        v = F(sinc * (0.5 * (1.0 - math.cos(2.0 * math.pi * j / 48.0))))
        c[j] = v if abs(v) >= F(1e-6) else F(0)
    return c


def design(rate):
    sb, sa, hb, ha = biquads(rate)
    P = transition(sa, ha)
    for _ in range(8):
        P = square(P)
    return SimpleNamespace(shelf_b=sb, shelf_a=sa, highpass_b=hb, highpass_a=ha, M=[float(v) for v in P.reshape(16)], c=interpolator(),
                           step=(rate + 5) // 10)


# ---- 2. K-weighting in chunks -----------------------------------------------------------------------------------------------------------

def samples(x, N):
    """x'[0 .. N): float64, a sample that is not finite is +0.0"""
    v = np.asarray(x, F)[:N]
    return np.where(np.isfinite(v), v, F(0)).astype(np.float64)


def run_chunks(D, X, S):
    """every chunk (row of X, [n, 256]) through the cascade from its state (row of S, [n, 4]) -> (W [n, 256], the end states)"""
    b0, b1, b2 = (float(v) for v in D.shelf_b)
    a1, a2 = (float(v) for v in D.shelf_a)
    h1, h2 = (float(v) for v in D.highpass_a)
    p1, p2, q1, q2 = (S[:, r].copy() for r in range(4))
    W = np.empty_like(X)
    for i in range(CHUNK):
        x = X[:, i]
        y = b0 * x + p1
        n1 = (b1 * x + p2) - a1 * y
        p2 = b2 * x - a2 * y
        p1 = n1
        w = y + q1
        n1 = (q2 - 2.0 * y) - h1 * w
        q2 = y - h2 * w
        q1 = n1
        W[:, i] = w
    return W, np.stack([p1, p2, q1, q2], axis=1)


def entry_states(D, Z):
    """phase B: s_0 = 0, s_(k+1) = M s_k + z_k, rows ascending, each a left-to-right dot product, then + z"""
    M = [float(v) for v in D.M]
    S = np.zeros_like(Z)
    s = [0.0, 0.0, 0.0, 0.0]
    for k in range(Z.shape[0]):
        S[k] = s
        s = [(((M[4 * r] * s[0] + M[4 * r + 1] * s[1]) + M[4 * r + 2] * s[2]) + M[4 * r + 3] * s[3]) + float(Z[k, r]) for r in range(4)]
    return S


def step_energies(D, xs):
    """E[0 .. J) of the samples xs (float64 [N]) through phases A .. D"""
    N, step = xs.size, int(D.step)
    n = -(-N // CHUNK)
    J = N // step
    if n == 0:
        return np.zeros(0, np.float64)
    X = np.zeros(n * CHUNK, np.float64)
    X[:N] = xs
    X = X.reshape(n, CHUNK)
    _, Z = run_chunks(D, X, np.zeros((n, 4), np.float64))
    W, _ = run_chunks(D, X, entry_states(D, Z))
    first = CHUNK * np.arange(n, dtype=np.int64)
    edge = (first // step + 1) * step
    runs = np.zeros((n, 2), np.float64)
    for i in range(CHUNK):
        q = W[:, i] * W[:, i]
        second = first + i >= edge
        runs[:, 0] = np.where(second, runs[:, 0], runs[:, 0] + q)
        runs[:, 1] = np.where(second, runs[:, 1] + q, runs[:, 1])
    E = np.zeros(J, np.float64)
    for j in range(J):
        e = 0.0
        for c in range(j * step // CHUNK, ((j + 1) * step - 1) // CHUNK + 1):
            e = e + float(runs[c, j - CHUNK * c // step])
        E[j] = e
    return E


# ---- 3. gating ------------------------------------------------------------------------------------------------------------------------

def gate(E, step):
    """(integrated, momentary max, short-term max, blocks, past the absolute gate, past both) from the step energies"""
    J = E.size
    nb = max(J - 3, 0)
    z = (((E[0:nb] + E[1:nb + 1]) + E[2:nb + 2]) + E[3:nb + 3]) / float(4 * step) if nb else np.zeros(0)
    mom = float(z.max()) if nb else 0.0
    sht = 0.0
    if J >= 30:
        ns = J - 29
        acc = np.zeros(ns, np.float64)
        for k in range(30):
            acc = acc + E[k:k + ns]
        sht = float((acc / float(30 * step)).max())
    past = [float(v) for v in z if v > GATE_ABS]
    z_int, ng = 0.0, 0
    if past:
        s = 0.0
        for v in past:
            s = s + v
        gr = TENTH * (s / float(len(past)))
        s = 0.0
        for v in past:
            if v > gr:
                s = s + v
                ng += 1
        if ng:
            z_int = s / float(ng)
    return z_int, mom, sht, nb, len(past), ng


# ---- 4. true peak -----------------------------------------------------------------------------------------------------------------------

def true_peak(D, x, N):
    """(tp float64, sample peak float32) of x[0 .. N)"""
    xs = samples(x, N)
    c = np.asarray(D.c, F).astype(np.float64)
    P = np.concatenate([np.zeros(11), xs, np.zeros(11)])
    n = N + 11
    best = 0.0
    for f in (1, 2, 3):
        acc = np.zeros(n, np.float64)
        for k in range(12):
            acc = acc + c[f + 4 * k] * P[11 - k:11 - k + n]          # the product of two float32 values is exact
        best = max(best, float(np.abs(acc).max())) if n else best
    v = np.asarray(x, F)[:N]
    sp = F(np.abs(np.where(np.isfinite(v), v, F(0))).max()) if N else F(0)
    return max(best, float(sp)), sp


# ---- 5. gain, 6. report -------------------------------------------------------------------------------------------------------------------

def ask(gain=1.0, target_lufs=0.0, ceiling=0.0, flags=0):
    """the ask as the kernels read it: the target as a mean square (the host's pow, once)"""
    zt = 10.0 ** ((float(F(target_lufs)) + 0.691) / 10.0) if flags & TARGET else 0.0
    return SimpleNamespace(gain=F(gain), ceiling=F(ceiling), flags=int(flags), zt=zt)


def gain(q, z_int, tp):
    gd = float(q.gain)
    if q.flags & TARGET and z_int > 0.0:
        gd = math.sqrt(q.zt / z_int) * float(q.gain)
    ceiling = False
    if q.flags & CEILING and gd * tp > float(q.ceiling):
        gd = float(q.ceiling) / tp
        ceiling = True
    with np.errstate(over="ignore"):
        g = F(gd)
    for _ in range(4):
        if not ceiling or not F(float(g) * tp) > q.ceiling or g == 0:
            break
        g = np.array([fbits(g) - 1], np.uint32).view(F)[0]
    return g


def _log10(v):
    return float(MR.ln(np.array([v]))[0]) * MR.LOG10E


def lufs(z):
    if not z >= MIN_NORMAL:
        return F(-np.inf)
    return F(OFFSET + 10.0 * _log10(z))


def dbtp(tp):
    if not tp >= MIN_NORMAL:
        return F(-np.inf)
    return F(20.0 * _log10(tp))


def rule(D, x, N, q=None, out=True):
    """the whole rule for one utterance: x float32 [total], N <= total the samples measured -> (result, x * gain or None)"""
    x = np.asarray(x, F)
    q = q or ask()
    z_int, mom, sht, nb, na, ng = gate(step_energies(D, samples(x, N)), int(D.step))
    tp, sp = true_peak(D, x, N)
    g = gain(q, z_int, tp)
    res = SimpleNamespace(integrated_ms=z_int, momentary_max_ms=mom, short_term_max_ms=sht, true_peak=tp, blocks=nb, blocks_absolute=na,
                          blocks_gated=ng, sample_peak=sp, integrated_lufs=lufs(z_int), momentary_max_lufs=lufs(mom),
                          short_term_max_lufs=lufs(sht), true_peak_dbtp=dbtp(tp), gain=g)
    with np.errstate(over="ignore", invalid="ignore"):
        return res, (x * g if out else None)


FIELDS_F64 = ("integrated_ms", "momentary_max_ms", "short_term_max_ms", "true_peak")
FIELDS_U32 = ("blocks", "blocks_absolute", "blocks_gated")
FIELDS_F32 = ("sample_peak", "integrated_lufs", "momentary_max_lufs", "short_term_max_lufs", "true_peak_dbtp", "gain")


def key(res):
    """every field of a result as integers: two results are the same bits where their keys are equal"""
    return tuple(dbits(getattr(res, f)) for f in FIELDS_F64) + tuple(int(getattr(res, f)) for f in FIELDS_U32) + \
        tuple(fbits(getattr(res, f)) for f in FIELDS_F32)


# ---- the standard without the decomposition: one sequential pass, textbook gating ------------------------------------------------------------

def plain(D, x, N):
    """integrated mean square by ONE sequential float64 pass over the whole signal (direct form II transposed, sample by sample) and
    blocks summed straight from the squared samples: what the chunked rule must equal up to rounding"""
    xs = samples(x, N)
    b0, b1, b2 = (float(v) for v in D.shelf_b)
    a1, a2 = (float(v) for v in D.shelf_a)
    h1, h2 = (float(v) for v in D.highpass_a)
    p1 = p2 = q1 = q2 = 0.0
    sq = np.empty(N, np.float64)
    for i, v in enumerate(xs.tolist()):
        y = b0 * v + p1
        p1 = b1 * v + p2 - a1 * y
        p2 = b2 * v - a2 * y
        w = y + q1
        q1 = q2 - 2.0 * y - h1 * w
        q2 = y - h2 * w
        sq[i] = w * w
    step = int(D.step)
    J = N // step
    cum = np.concatenate([[0.0], np.cumsum(sq)])
    z = np.array([(cum[(i + 4) * step] - cum[i * step]) / (4 * step) for i in range(max(J - 3, 0))])
    past = z[z > GATE_ABS]
    if not past.size:
        return 0.0
    past = past[past > 0.1 * past.mean()]
    return float(past.mean()) if past.size else 0.0
