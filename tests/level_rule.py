"""The volume rule of include/zerovox_amd.h ("volume controls") restated with Python integers for the sum of squares, one float64
operation per step and np.nextafter — what csrc/level.h and the two kernels must give bit for bit."""
import numpy as np

Q_ONE = 524288.0                 # 2^19
S_ONE = 274877906944.0           # 2^38
IDENTITY = (1.0, 0.0, 0.0)       # gain, target_rms, peak_ceiling


def bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


def quant(x):
    """q_i of every sample, int64: min(|x|, 1) * 2^19 + 0.5 truncated, 0 for NaN and +-inf"""
    x = np.asarray(x, np.float32)
    finite = np.isfinite(x)
    a = np.where(finite, np.abs(x), np.float32(0)).astype(np.float32)
    a = np.minimum(a, np.float32(1.0))
    d = a.astype(np.float64) * Q_ONE
    d = d + 0.5
    return np.where(finite, np.trunc(d), 0.0).astype(np.int64)


def measure(speech):
    """(S as a Python integer, the peak's bit pattern) of the speech samples"""
    q = quant(speech)
    S = 0
    for i in range(0, len(q), 1 << 16):
        c = q[i:i + (1 << 16)]
        S += int(np.sum(c * c))           # <= 2^16 * 2^38: exact in int64; the total is a Python integer
    b = bits(speech) & np.uint32(0x7fffffff)
    b = b[b < np.uint32(0x7f800000)]
    return S, int(b.max()) if len(b) else 0


def rms_of(S, n):
    if S <= 0:
        return np.float64(0.0)
    den = np.float64(n) * np.float64(S_ONE)
    return np.sqrt(np.float64(S) / den)


def gain_of(S, rms, peak_bits, volume):
    gain, target, ceiling = (np.float32(v) for v in volume)
    peak = np.array([peak_bits], np.uint32).view(np.float32)[0]
    gd = np.float64(gain)
    if target > 0 and S > 0:
        gd = np.float64(target) / rms
        gd = gd * np.float64(gain)
    applied = False
    with np.errstate(all="ignore"):
        if ceiling > 0 and peak > 0 and gd * np.float64(peak) > np.float64(ceiling):
            gd = np.float64(ceiling) / np.float64(peak)
            applied = True
        g = np.float32(gd)
        for _ in range(4):
            if not (applied and np.float32(g * peak) > ceiling):
                break
            g = np.nextafter(g, np.float32(0))
    return np.float32(g)


def report(S, n, peak_bits, volume=IDENTITY):
    """(rms as float64, (rms, peak, gain) as float32) from the totals"""
    rms = rms_of(S, n)
    peak = np.array([peak_bits], np.uint32).view(np.float32)[0]
    return rms, (np.float32(rms), peak, gain_of(S, rms, peak_bits, volume))


def rule(x, n, volume=IDENTITY):
    """the whole rule over a waveform x of which the first n samples are speech: dict(S, peak_bits, rms, level, out)"""
    x = np.asarray(x, np.float32)
    S, pk = measure(x[:n])
    rms, level = report(S, n, pk, volume)
    with np.errstate(all="ignore"):
        out = x * level[2]
    return dict(S=S, peak_bits=pk, rms=rms, level=level, out=out)


def level_bits(level):
    """the three floats of a level as bit patterns (a capi.Level, or the tuple rule() gives)"""
    if hasattr(level, "rms"):
        level = (level.rms, level.peak, level.gain)
    return [int(b) for b in bits(np.array(level, np.float32))]


def chunk_samples(root):
    """LEVEL_CHUNK_SAMPLES of csrc/level.h"""
    import os
    import re
    m = re.search(r"constexpr int LEVEL_CHUNK_SAMPLES = (\d+);", open(os.path.join(root, "zerovox.cpp_amd", "csrc", "level.h")).read())
    return int(m.group(1))
