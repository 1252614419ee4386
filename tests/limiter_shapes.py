"""Inputs that take the limiter (include/zerovox_amd.h "limiter") through every path of its kernels, and the proof that they get there:
every shape comes with an assertion computed from the restatement's own intermediate values (tests/limiter_rule.py), so a shape that
misses its branch fails on the CPU, before a device is asked.  Shared by tests/test_limiter_cpu.py (which runs every assertion here
without a device, and holds the restatement against csrc/limiter.h's reference) and tests/test_gpu_limiter.py.

The kernels' tiles (csrc/limiter.h): every pass covers TILE = 2 048 entries per workgroup — the peak pass entries of q, where q_j lies at
j + H + PAD (H = attack + release, PAD = 4); the minimum pass entries of m, where m_k lies at k + attack; the mean pass samples n."""
from types import SimpleNamespace

import numpy as np

import limiter_rule as LM
import loudness_shapes as LS

F = np.float32
SR, HOP = 22050, 300
TILE, PAD = 2048, 4
ATTACK, RELEASE = LM.design(SR)            # 33, 1323: W = 1 357
ONE = LM.ONE


def speech(seed, T, amp=0.1):
    return LS.speech(SR, seed, T * HOP, amp)


def _case(x, nf, ask, reach):
    return SimpleNamespace(x=np.asarray(x, F), nf=nf, N=min(nf, x.size // HOP) * HOP, ask=ask, reach=reach)


def _limited(I, res):
    assert 0 < res.limited_samples and int(I.s.min()) < ONE


def w3():
    """the smallest window: attack = release = 1"""
    def reach(I, res):
        assert I.W == 3
        _limited(I, res)
    return _case(speech(1, 8, 0.5), 8, LM.ask(4.0, 0.1, 1, 1), reach)


def w8192():
    """the largest window, a span of more than two of them"""
    def reach(I, res):
        assert I.W == 8192 and I.s.size > 2 * I.W
        _limited(I, res)
    return _case(speech(2, 60, 0.5), 58, LM.ask(2.0, 0.25, 2047, 6144), reach)


def span_below_window():
    """N < W"""
    def reach(I, res):
        assert 20 * HOP < I.W == 8192
        _limited(I, res)
    return _case(speech(3, 20, 0.5), 20, LM.ask(2.0, 0.25, 2047, 6144), reach)


def span_below_attack():
    """N < attack: the first sample's gain already looks past the whole span"""
    def reach(I, res):
        assert 5 * HOP < I.ask.attack
        _limited(I, res)
        assert int(I.s[0]) < ONE
    return _case(speech(4, 6, 0.5), 5, LM.ask(4.0, 0.25, 2047, 100), reach)


def zero_frames():
    """n_frames = 0: nothing is measured, the capacity is scaled by the gain alone"""
    def reach(I, res):
        assert res.limited_samples == 0 and res.true_peak_before == 0.0 and (I.s == ONE).all() and res.min_gain == F(1)
    return _case(speech(5, 4, 0.9), 0, LM.ask(3.0, 0.1, 10, 20), reach)


def loud_tail():
    """n_frames < T: the tail behind N is ten times louder, scaled and not measured"""
    x = speech(6, 20, 0.6)
    x[10 * HOP:] *= F(10)
    def reach(I, res):
        assert I.span < x.size and float(np.abs(x[I.span:]).max()) * 2.0 > 0.25      # the tail passes the ceiling and nobody minds
        _limited(I, res)
    return _case(x, 10, LM.ask(2.0, 0.25, ATTACK, RELEASE), reach)


def peaks_at_both_ends():
    """a peak in sample 0 and in sample N - 1: their pre- and post-ring lies outside the span and still asks for a gain"""
    x = speech(7, 12, 0.02)
    N = 10 * HOP
    x[0], x[N - 1] = F(0.9), F(-0.95)
    def reach(I, res):
        r = LM.required(I.ask, I.p)                                  # q_m at m + 6
        assert (r[:6] < ONE).any() and (r[N + 6:] < ONE).any()       # m < 0 and m >= N
        assert int(I.s[0]) <= int(r[6]) < ONE and int(I.s[N - 1]) <= int(r[N - 1 + 6]) < ONE
    return _case(x, 10, LM.ask(1.0, 0.1, ATTACK, RELEASE), reach)


def peak_pairs():
    """two peaks closer than W and two exactly W apart, the later the higher in one pair and the lower in the other"""
    x = speech(8, 40, 0.02)
    W = ATTACK + RELEASE + 1
    a, b = 700, 5000
    x[a], x[a + W - 10], x[b], x[b + W] = F(0.9), F(0.6), F(0.5), F(0.8)
    def reach(I, res):
        assert I.W == W
        s = I.s
        assert int(s[a]) < int(s[a + W - 10]) < ONE and int(s[b + W]) < int(s[b]) < ONE
        assert int(s[a:a + W].max()) < ONE                           # the gain does not recover between the close pair
    return _case(x, 40, LM.ask(1.0, 0.25, ATTACK, RELEASE), reach)


def tile_edges():
    """a span of three tiles with a peak on either side of a tile's end in every pass's own index: the mean pass's samples, the minimum
    pass's entries of m and the peak pass's entries of q"""
    x = speech(9, 20, 0.02)
    H = ATTACK + RELEASE
    at = {}
    for e in (TILE, 2 * TILE):
        at[("mean", e)] = (e - 1, e)
        at[("min", e)] = (e - 1 - ATTACK, e - ATTACK)
        at[("peak", e)] = (e - 1 - H - PAD, e - H - PAD)
    amp = 0.5
    for pair in at.values():
        for n in pair:
            x[n] = F(amp)
            amp += 0.03
    def reach(I, res):
        assert -(-x.size // TILE) == 3 and -(-(x.size + H) // TILE) == 4 and -(-(x.size + 2 * (H + PAD)) // TILE) == 5
        r = LM.required(I.ask, I.p)
        for (lo, hi) in at.values():
            assert 0 <= lo and hi < x.size and int(r[lo + 6]) < ONE and int(r[hi + 6]) < ONE
    return _case(x, 20, LM.ask(1.0, 0.25, ATTACK, RELEASE), reach)


def one_tile():
    """a span of one tile in every pass"""
    def reach(I, res):
        assert 6 * HOP + 2 * (I.H + PAD) <= TILE
        _limited(I, res)
    return _case(speech(10, 6, 0.5), 6, LM.ask(2.0, 0.25, 3, 40), reach)


def square():
    """a full-scale square wave: every sample is limited"""
    t = np.arange(12 * HOP)
    x = np.where((t // 37) % 2 == 0, 1.0, -1.0).astype(F)
    def reach(I, res):
        assert res.limited_samples == x.size and int(I.s.max()) < ONE
    return _case(x, 12, LM.ask(1.0, 0.5, ATTACK, RELEASE), reach)


def silent():
    def reach(I, res):
        assert res.limited_samples == 0 and res.true_peak_before == 0.0 and np.isneginf(res.true_peak_before_dbtp) and res.reduction_db == F(0)
    return _case(np.zeros(9 * HOP, F), 9, LM.ask(5.0, 0.1, ATTACK, RELEASE), reach)


def not_finite():
    """a NaN and two infinities: they count as +0.0 where peaks are measured and pass through the arithmetic of the apply step"""
    x = speech(11, 12, 0.5)
    x[1234], x[2000], x[2001] = np.nan, np.inf, -np.inf
    def reach(I, res):
        _limited(I, res)
        assert np.isfinite(res.true_peak_before) and np.isfinite(res.true_peak_after)
    return _case(x, 12, LM.ask(2.0, 0.25, ATTACK, RELEASE), reach)


def gain_zero():
    def reach(I, res):
        assert res.limited_samples == 0 and res.true_peak_after == 0.0 and res.true_peak_before > 0.0
    return _case(speech(12, 7, 0.5), 7, LM.ask(0.0, 0.25, ATTACK, RELEASE), reach)


def identity():
    """ask = None: gain 1, ceiling 1, the default windows; below full scale nothing happens"""
    def reach(I, res):
        assert I.ask.attack == ATTACK and I.ask.release == RELEASE and res.limited_samples == 0 and res.true_peak_before < 1.0
    return _case(speech(13, 9, 0.3), 9, None, reach)


CASES = {f.__name__: f for f in (w3, w8192, span_below_window, span_below_attack, zero_frames, loud_tail, peaks_at_both_ends, peak_pairs,
                                 tile_edges, one_tile, square, silent, not_finite, gain_zero, identity)}


def check(D, c):
    """the rule on a case, its reach asserted, and what holds on every case: s_n <= q_n and the promise -> (result, out, intermediates)"""
    res, out, I = LM.rule(D, c.x, c.N, c.ask, SR)
    c.reach(I, res)
    n = np.arange(I.span)
    assert (I.s <= I.q[n + I.H]).all()                               # s_n <= q_n
    head = out[:c.N]
    fin = np.isfinite(head)
    assert (np.abs(head[fin]) <= I.ask.ceiling).all()                # the promise
    return res, out, I


def ragged_batch():
    """five utterances under mixed asks: a short one, a silent one, one with a NaN and an infinity, a long one at the largest window,
    one at the smallest"""
    xs = [speech(31, 5, 0.5), np.zeros(9 * HOP, F), speech(33, 30, 0.5), speech(34, 64, 0.6), speech(35, 21, 0.4)]
    xs[2][1234], xs[2][7000], xs[2][7001] = np.nan, np.inf, -np.inf
    nfs = [5, 9, 27, 60, 21]
    asks = [LM.ask(6.0, 0.25, ATTACK, RELEASE), LM.ask(3.0, 0.5, 7, 9), LM.ask(1.5, 0.2, 100, 900), LM.ask(2.0, 0.25, 2047, 6144),
            LM.ask(4.0, 0.1, 1, 1)]
    return xs, nfs, asks
