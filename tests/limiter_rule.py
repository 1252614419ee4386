"""The limiter of include/zerovox_amd.h ("limiter") restated from the header's text in numpy: one float64 operation per step up to the
required gain, integers behind it — what csrc/limiter.h and the kernels must give bit for bit.  Independent of limiter.h: nothing here
is read from it.  The interpolator is data (any object with the loudness design's field c); the logarithm of the report is
loudness_rule's.

rule() keeps its intermediates (p, q, m, s) so that a test can assert FROM THEM that an input reaches the branch it is there for.  The
windows are taken with numpy's sliding_window_view where they are short and by block prefix / suffix minima and a cumulative sum where
they are long: integers, so both give the same values (tests/test_limiter_cpu.py holds the two against each other)."""
from types import SimpleNamespace

import numpy as np

import loudness_rule as LR

F = np.float32
ONE = 1 << 30
DELAY = 6
MAX_ATTACK, MAX_RELEASE = 2047, 6144
ATTACK_MS, RELEASE_MS = 1.5, 60.0


def design(rate, attack_ms=0.0, release_ms=0.0):
    """zv_limit_design: floor(ms * rate / 1000 + 0.5) in float64, brought into [1, most]; 0 ms: the default"""
    def count(ms, most):
        v = (float(F(ms)) * float(rate)) / 1000.0 + 0.5
        return 1 if not v >= 1.0 else most if v >= most else int(v)
    return count(attack_ms or ATTACK_MS, MAX_ATTACK), count(release_ms or RELEASE_MS, MAX_RELEASE)


def ask(gain=1.0, ceiling=1.0, attack=1, release=1):
    return SimpleNamespace(gain=F(gain), ceiling=F(ceiling), attack=int(attack), release=int(release))


# ---- 1. peaks -------------------------------------------------------------------------------------------------------------------------

def peaks(D, x, N):
    """(p float64 [N + 11]: p_m at m + 6, m = -6 .. N + 4; true peak float64; sample peak float32) of x[0 .. N)"""
    xs = LR.samples(x, N)
    c = np.asarray(D.c, F).astype(np.float64)
    P = np.concatenate([np.zeros(11), xs, np.zeros(11)])
    n = N + 11
    p = np.zeros(n, np.float64)
    for f in (1, 2, 3):
        acc = np.zeros(n, np.float64)
        for k in range(12):
            acc = acc + c[f + 4 * k] * P[11 - k:11 - k + n]          # v_f(n'), n' = m + 6; the product of two float32 values is exact
        p = np.maximum(p, np.abs(acc))
    p[DELAY:DELAY + N] = np.maximum(p[DELAY:DELAY + N], np.abs(xs))
    sp = F(np.abs(xs).max()) if N else F(0)
    return p, (float(p.max()) if n else 0.0), sp


# ---- 2. required gain ---------------------------------------------------------------------------------------------------------------------

def required(q, p):
    """q_m (int64) of the peaks p"""
    a = float(q.gain) * p
    over = (p > 0.0) & ~(a <= float(q.ceiling))
    r = np.full(p.size, ONE, np.int64)
    r[over] = np.floor((float(q.ceiling) / a[over]) * 1073741824.0).astype(np.int64)
    return r


# ---- 3. sliding minimum, 4. sliding mean ------------------------------------------------------------------------------------------------------

def window_min(v, W):
    """min v[i .. i + W), i = 0 .. v.size - W, by prefix and suffix minima over blocks of W"""
    n = v.size
    nb = -(-n // W)
    pad = np.full(nb * W, np.iinfo(np.int64).max, np.int64)
    pad[:n] = v
    B = pad.reshape(nb, W)
    pre = np.minimum.accumulate(B, axis=1).reshape(-1)
    suf = np.minimum.accumulate(B[:, ::-1], axis=1)[:, ::-1].reshape(-1)
    i = np.arange(n - W + 1)
    return np.minimum(suf[i], pre[i + W - 1])


def window_sum(v, W):
    """sum v[i .. i + W), i = 0 .. v.size - W (int64: at most 8 192 values of at most 2^30)"""
    c = np.concatenate([[0], np.cumsum(v, dtype=np.int64)])
    return c[W:] - c[:-W]


def gains(q, p, N, span):
    """(qfull, m, s) over what the samples n in [0, span) need: qfull[j + H] = q_j, j in [-H, span + H); m[k + attack] = m_k, k in
    [-attack, span + release); s[n]"""
    H = q.attack + q.release
    W = H + 1
    qfull = np.full(span + 2 * H, ONE, np.int64)
    r = required(q, p)
    j = np.arange(-DELAY, N + 5)
    ok = (j + H >= 0) & (j + H < qfull.size)
    qfull[j[ok] + H] = r[ok]
    m = window_min(qfull, W)
    s = window_sum(m, W) // W
    assert m.size == span + H and s.size == span
    return qfull, m, s


# ---- 5. apply, 6. report ----------------------------------------------------------------------------------------------------------------------

def apply(x, gain, s):
    with np.errstate(over="ignore", invalid="ignore"):
        return ((x.astype(np.float64) * float(gain)) * (s.astype(np.float64) * 2.0 ** -30)).astype(F)


def rule(D, x, N, q=None, rate=22050):
    """the whole rule for one utterance: x float32 [total], N <= total the samples measured -> (result, out, intermediates).  Behind
    n = N + 4 + H no window meets a peak: s is ONE there and is not computed sample by sample."""
    x = np.asarray(x, F)
    total = x.size
    if q is None:
        q = ask(1.0, 1.0, *design(rate))
    H = q.attack + q.release
    p, tp, sp = peaks(D, x, N)
    span = min(total, N + 5 + H)
    qfull, m, s = gains(q, p, N, span)
    out = np.empty(total, F)
    out[:span] = apply(x[:span], q.gain, s)
    out[span:] = apply(x[span:], q.gain, np.full(total - span, ONE, np.int64))
    _, tpa, spa = peaks(D, out, N)
    min_s = int(s[:N].min()) if N else ONE
    g = float(min_s) * 2.0 ** -30
    res = SimpleNamespace(true_peak_before=tp, true_peak_after=tpa, limited_samples=int((s[:N] < ONE).sum()), sample_peak_before=sp,
                          sample_peak_after=spa, min_gain=F(g), true_peak_before_dbtp=LR.dbtp(tp), true_peak_after_dbtp=LR.dbtp(tpa),
                          reduction_db=LR.dbtp(g))
    return res, out, SimpleNamespace(p=p, q=qfull, m=m, s=s, H=H, W=H + 1, span=span, ask=q)


FIELDS_F64 = ("true_peak_before", "true_peak_after")
FIELDS_F32 = ("sample_peak_before", "sample_peak_after", "min_gain", "true_peak_before_dbtp", "true_peak_after_dbtp", "reduction_db")


def key(res):
    """every field of a result as integers: two results are the same bits where their keys are equal"""
    return tuple(LR.dbits(getattr(res, f)) for f in FIELDS_F64) + (int(res.limited_samples),) + tuple(LR.fbits(getattr(res, f)) for f in FIELDS_F32)


def brute(q, p, N, span):
    """steps 2 to 4 with the windows written out (slow: for short spans)"""
    H = q.attack + q.release
    r = required(q, p)
    qj = lambda j: int(r[j + DELAY]) if -DELAY <= j <= N + 4 else ONE
    mk = lambda k: min(qj(j) for j in range(k - q.release, k + q.attack + 1))
    return np.array([sum(mk(k) for k in range(n - q.attack, n + q.release + 1)) // (H + 1) for n in range(span)], np.int64)
