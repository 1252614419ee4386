"""The envelope rule of include/zerovox_amd.h ("amplitude envelope") restated with Python integers for the gains, the window sums and
the knots, and one float64 operation per step behind them — what csrc/envelope.h and the two kernels must give bit for bit."""
import numpy as np

ONE = 65536
IDENTITY = (None, 0, 0, 0)       # phoneme_gain, ramp_frames, fade_in_samples, fade_out_samples


def bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


def fixed_gain(g):
    """G_i of a linear gain: (int64)((double)g * 65536.0 + 0.5), truncating"""
    d = np.float64(np.float32(g)) * np.float64(65536.0)
    d = d + np.float64(0.5)
    return int(np.trunc(d))


def frame_gains(durations, gains, T):
    """F[0 .. nf) as Python integers from the phoneme timings (already clipped to the capacity T, as the library returns them) and
    the linear gains (None: all 1): phoneme i owns durations[i] frames from the sum of the durations before it"""
    F = []
    for i, d in enumerate(durations):
        G = ONE if gains is None else fixed_gain(gains[i])
        F += [G] * int(d)
    assert len(F) <= T
    return F


def knots(F, r):
    """B[0 .. nf] as Python integers: B[f] = A[f - 1] + A[f], A[f] = the sum of F over f - r .. f + r with F edge-replicated"""
    nf = len(F)
    if nf == 0:
        return []
    at = lambda j: F[min(max(j, 0), nf - 1)]
    A = lambda f: sum(at(j) for j in range(f - r, f + r + 1))
    return [A(f - 1) + A(f) for f in range(nf + 1)]


def sample_gains(B, nf, hop, total, r, Fi, Fo):
    """e[0 .. total) as float32: every step of the rule on whole arrays, one float64 operation each"""
    if nf == 0:
        return np.full(total, 0.0 if Fo > 0 else 1.0, np.float32)
    n = nf * hop
    s = np.arange(total, dtype=np.int64)
    f = np.minimum(s // hop, nf)
    j = s - (s // hop) * hop
    Bk = np.array(B, dtype=np.int64)
    num = np.where(s < n, Bk[f] * (hop - j) + Bk[np.minimum(f + 1, nf)] * j, Bk[nf] * hop)
    den = 2 * (2 * r + 1) * hop * 65536
    assert int(num.max()) < 1 << 38 and all(b < 1 << 29 for b in B)
    d = num.astype(np.float64) / np.float64(den)
    if Fi > 0:
        t = s.astype(np.float64) / np.float64(Fi)
        d = np.where(s < Fi, d * t, d)
    if Fo > 0:
        k = n - 1 - s
        t = np.maximum(k, 0).astype(np.float64) / np.float64(Fo)
        d = np.where(k < Fo, d * t, d)
    return d.astype(np.float32)


def rule(x, durations, T, hop, envelope=IDENTITY):
    """the whole rule over a waveform x of T * hop samples whose phoneme timings are durations: dict(B, e, out, nf)"""
    gains, r, Fi, Fo = envelope
    x = np.asarray(x, np.float32)
    assert x.shape == (T * hop,)
    F = frame_gains(durations, gains, T)
    nf = len(F)
    B = knots(F, r)
    e = sample_gains(B, nf, hop, T * hop, r, Fi, Fo)
    with np.errstate(all="ignore"):
        out = x * e
    return dict(B=B, e=e, out=out, nf=nf)


def as_tuple(env):
    """a capi.Envelope (or None: the identity) as the rule's tuple"""
    if env is None:
        return IDENTITY
    return (None if env.phoneme_gain is None else np.asarray(env.phoneme_gain, np.float32), int(env.ramp_frames), int(env.fade_in_samples),
            int(env.fade_out_samples))
