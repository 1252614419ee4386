"""The waveform filter's rule and design (include/zerovox_amd.h "waveform filter") restated in numpy: float64 steps, one IEEE operation
each.  tests/test_filter_cpu.py holds csrc/filter.h to it, tests/test_gpu_filter.py the device."""
import numpy as np

F = np.float32
MAX_TAPS = 511
TILE = 2048                      # outputs of one workgroup of filter_kernel (csrc/filter.h FILTER_TILE; filter_check compares)
DFT = 1024
DEFAULT_EDGES = (1, 3, 5, 8, 12, 17, 24, 33, 45, 62, 84, 114, 155, 210, 285, 387, 513)


def span(x):
    """x'[j]: float64, +0.0 where the sample is not finite"""
    x = np.asarray(x, F)
    return np.where(np.isfinite(x), x.astype(np.float64), 0.0)


def apply(x, taps, S=None):
    """y[0 .. len(x)): the rule over the span x[0 .. S) (S None: all of x), +0.0 behind it.  taps None: a copy, bit for bit."""
    x = np.ascontiguousarray(x, F)
    if taps is None:
        return x.copy()
    S = x.size if S is None else int(S)
    h = np.ascontiguousarray(taps, F).astype(np.float64)
    L = h.size
    assert L % 2 == 1 and 1 <= L <= MAX_TAPS and 0 <= S <= x.size
    c = (L - 1) // 2
    xp = np.concatenate([np.zeros(L), span(x[:S]), np.zeros(L)])
    acc = np.zeros(S)
    for k in range(L):                       # ascending k for every output sample; the product of two f32 values is exact in f64
        acc = acc + h[k] * xp[L + c - k: L + c - k + S]
    y = np.zeros(x.size, F)
    with np.errstate(over="ignore"):
        y[:S] = acc.astype(F)
    return y


def design(gains, edges=None, n_taps=255):
    """zv_filter_design: linear gains per band -> float32 taps"""
    g = np.asarray(gains, F).astype(np.float64)
    e = np.asarray(DEFAULT_EDGES if edges is None else edges, np.int64)
    assert e.size == g.size + 1 and n_taps % 2 == 1
    c = (n_taps - 1) // 2
    m = np.arange(-c, c + 1)
    w = 0.5 + 0.5 * np.cos(2.0 * np.pi * m / (n_taps + 1))

    def lp(f):
        out = np.full(m.size, 2.0 * f)
        nz = m != 0
        out[nz] = np.sin(2.0 * np.pi * f * m[nz]) / (np.pi * m[nz])
        return out

    h = (m == 0).astype(np.float64)
    for b in range(g.size):
        f_lo = max(e[b] - 0.5, 0.0) / DFT
        f_hi = min(e[b + 1] - 0.5, 512.0) / DFT
        h = h + (g[b] - 1.0) * (lp(f_hi) - lp(f_lo)) * w
    return h.astype(F)


def response(taps, n=4096):
    """|H| at the n/2 + 1 frequencies k / n cycles per sample (n = 4096: a quarter of a DFT bin apart)"""
    return np.abs(np.fft.rfft(np.asarray(taps, np.float64), n))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
