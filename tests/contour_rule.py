"""The level contour of include/zerovox_amd.h ("level contour") restated on top of tests/level_rule.py: Python integers for every sum of
squares, maxima of bit patterns, one float64 operation per step — what csrc/contour.h and the two kernels must give bit for bit."""
import numpy as np

import level_rule as LR

F = np.float32


def from_bits(b):
    return np.array([b], np.uint32).view(F)[0]


def row(S, samples, peak_bits):
    """(rms, peak) as float32 from the totals of `samples` samples"""
    return F(LR.rms_of(S, samples)), from_bits(peak_bits)


def frame_totals(w, T, hop):
    """([S_f] as Python integers, [P_f] as bit patterns) of the T frames of the capacity"""
    w = np.asarray(w, F)
    assert w.shape == (T * hop,)
    tot = [LR.measure(w[f * hop:(f + 1) * hop]) for f in range(T)]
    return [t[0] for t in tot], [t[1] for t in tot]


def rule(w, T, hop, durations):
    """the whole rule for one utterance: dict(S, P: the frames' totals; frames float32 [T, 2]; phonemes float32 [n, 2]; pS, pP: the
    phonemes' totals)"""
    S, P = frame_totals(w, T, hop)
    frames = np.zeros((T, 2), F)
    for f in range(T):
        frames[f] = row(S[f], hop, P[f])
    n = len(durations)
    phonemes = np.zeros((n, 2), F)
    pS, pP = [], []
    start = 0
    for i, d in enumerate(int(d) for d in durations):
        assert d >= 0 and start + d <= T
        s, p = sum(S[start:start + d]), max(P[start:start + d], default=0)
        phonemes[i] = row(s, d * hop, p)
        pS.append(s)
        pP.append(p)
        start += d
    return dict(S=S, P=P, frames=frames, phonemes=phonemes, pS=pS, pP=pP)


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def chunk_frames(root):
    """CONTOUR_CHUNK_FRAMES of csrc/contour.h: the frames one workgroup of the frames kernel covers"""
    import os
    import re
    m = re.search(r"constexpr int CONTOUR_CHUNK_FRAMES = (\d+);", open(os.path.join(root, "zerovox.cpp_amd", "csrc", "contour.h")).read())
    return int(m.group(1))
