"""Inputs that take loudness (include/zerovox_amd.h "loudness") where 22 050 Hz and three seconds never go, and the proof that they get
there: every shape comes with an assertion computed from the restatement's own intermediate values (tests/loudness_rule.py), so a
shape that misses its branch fails on the CPU, before a device is asked.  Shared by tests/test_loudness_cpu.py (which runs every
assertion here without a device) and tests/test_gpu_loudness_shapes.py (which runs them again in front of the device calls).
 * gate_wave / gate_reach: spans of more than 64 and more than 128 momentary blocks, short-term sums and true-peak tiles, shaped so
   that what the gate kernel carries from one round of 64 to the next decides the answer;
 * ROUND_DOWN_CEILINGS / round_down_split: ceilings at which (float)(ceiling / true peak) breaks the promise and loud_gain steps one
   bit pattern down;
 * group_ends: loud_group_end's rule (launch groups of at most 2^26 padded samples) restated."""
from types import SimpleNamespace

import numpy as np

import loudness_rule as LR

F = np.float32
HOP = 300
ROUND = 64                       # blocks, short-term sums and true-peak tiles one round of the gate kernel takes
TP_TILE, TP_TAIL = 2048, 11      # outputs of one true-peak tile; outputs behind the span
GROUP_SAMPLES = 1 << 26


def speech(rate, seed, n, amp=0.1):
    """n samples of harmonics and noise under a slow swell, so that blocks differ and the relative gate has something to drop"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    f0 = rng.uniform(90, 250) / rate
    x = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 6)) / h for h in range(1, 9))
    swell = 0.02 + np.abs(np.sin(2 * np.pi * t / rate * rng.uniform(0.4, 0.9)))
    return ((x * 0.4 + rng.standard_normal(n) * 0.05) * swell * amp).astype(F)


# ---- the gate's rounds --------------------------------------------------------------------------------------------------------------

GATE_CASES = ((4000, 90), (4000, 91), (4000, 175), (4000, 176), (22050, 436), (22050, 437), (22050, 1500))      # (rate, n_frames)
VARIANTS = ("early", "late")


def gate_counts(step, nf):
    """(N, steps, momentary blocks, short-term sums, true-peak tiles) of nf frames"""
    N = nf * HOP
    J = N // step
    return N, J, max(J - 3, 0), max(J - 29, 0), -(-(N + TP_TAIL) // TP_TILE)


def gate_wave(rate, step, nf, T, variant, seed=0):
    """T frames of a steady voice whose level follows the 100 ms steps of the first nf frames, in a pattern of 32 steps: seven silent
    steps (four whole blocks fail the absolute gate), eight at -26 dB (five whole blocks pass it and fall to the relative gate), the rest
    at full level.  "early": a loud stretch and a two-sample burst near the start hold every maximum, the last block is a quiet one.
    "late": the last four steps are loud and the burst is the last two samples of the span, so the momentary and the short-term
    maximum belong to the last block and the true peak to the interpolator's ringing BEHIND the span.  The frames behind nf are ten
    times louder than anything measured."""
    assert variant in VARIANTS
    N, J, *_ = gate_counts(step, nf)
    assert J >= 40 and N > 4 * TP_TILE and T > nf
    rng = np.random.default_rng(1000 * nf + seed)
    t = np.arange(T * HOP)
    f0 = rng.uniform(120, 200) / rate
    x = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 6)) / h for h in range(1, 6)) * 0.4 + rng.standard_normal(t.size) * 0.05
    j = np.arange(J)
    level = np.where((j % 32 >= 3) & (j % 32 < 10), 0.0, np.where((j % 32 >= 16) & (j % 32 < 24), 0.05, 1.0))
    if variant == "early":
        level[11:15] = 3.0
        level[J - 4:] = 0.05
    else:
        level[J - 4:] = 3.0
    env = np.full(t.size, 10.0)
    env[:N] = level[np.minimum(t[:N] // step, J - 1)]
    x = (x * env * 0.06).astype(F)
    at = 3 * TP_TILE + 100 if variant == "early" else N - 2
    x[at:at + 2] = F(0.9)
    return x


def peak_outputs(D, x, N):
    """the largest |v| of the three interpolated phases at every output n = 0 .. N + 11, in LR.true_peak's own steps"""
    c = np.asarray(D.c, F).astype(np.float64)
    P = np.concatenate([np.zeros(TP_TAIL), LR.samples(x, N), np.zeros(TP_TAIL)])
    n = N + TP_TAIL
    best = np.zeros(n, np.float64)
    for f in (1, 2, 3):
        acc = np.zeros(n, np.float64)
        for k in range(12):
            acc = acc + c[f + 4 * k] * P[11 - k:11 - k + n]
        best = np.maximum(best, np.abs(acc))
    return best


def gate_reach(D, x, nf, variant):
    """asserts, from the restatement alone, that gate_wave's span takes the gate through what it is there for; -> the counts"""
    step = int(D.step)
    N, J, nb, ns, tiles = gate_counts(step, nf)
    E = LR.step_energies(D, LR.samples(x, N))
    z_int, mom, sht, nb_, na, ng = LR.gate(E, step)
    assert E.size == J and nb_ == nb
    z = (((E[0:nb] + E[1:nb + 1]) + E[2:nb + 2]) + E[3:nb + 3]) / float(4 * step)
    assert float(z.max()) == mom
    passed = z > LR.GATE_ABS
    s = 0.0
    for v in z[passed]:
        s = s + float(v)
    gr = LR.TENTH * (s / float(na))
    dropped = passed & ~(z > gr)
    assert int(passed.sum()) == na and int((passed & ~dropped).sum()) == ng
    assert 0 < ng < na < nb, (ng, na, nb)                            # both gates drop blocks
    rounds = -(-nb // ROUND)
    if rounds > 1:
        assert (~passed[:ROUND]).any() and passed[ROUND:].any()      # blocks fail the absolute gate in round 0 and pass it later
        assert dropped[:ROUND].any()
        assert (int(z.argmax()) >= ROUND) == (variant == "late")     # the momentary maximum, behind the first round or inside it
        if variant == "early":
            assert all(dropped[r * ROUND:(r + 1) * ROUND].any() for r in range(rounds)), "the relative gate drops blocks in every round"
    if ns:
        acc = np.zeros(ns, np.float64)
        for k in range(30):
            acc = acc + E[k:k + ns]
        st = acc / float(30 * step)
        assert float(st.max()) == sht
        if ns > ROUND:
            assert (int(st.argmax()) >= ROUND) == (variant == "late")
    tp, sp = LR.true_peak(D, x, N)
    P = peak_outputs(D, x, N)
    assert max(float(P.max()), float(sp)) == tp
    at, at_sp = int(P.argmax()), int(np.abs(LR.samples(x, N)).argmax())
    if variant == "late":
        assert at >= N and float(P[:N].max()) < tp and float(sp) < tp, "the true peak lies in the ringing behind the span"
    if tiles > ROUND:
        assert (at // TP_TILE >= ROUND) == (variant == "late") and (at_sp // TP_TILE >= ROUND) == (variant == "late")
        assert (at_sp - TP_TAIL) // TP_TILE == at_sp // TP_TILE      # (one tile alone stages the loudest sample)
    return SimpleNamespace(N=N, steps=J, blocks=nb, short_terms=ns, tiles=tiles)


# ---- the ceiling's round-down step ----------------------------------------------------------------------------------------------------

ROUND_DOWN_RATE, ROUND_DOWN_FRAMES, ROUND_DOWN_GAIN = 22050, 40, 8.0
ROUND_DOWN_CEILINGS = tuple(F(0.04 + 0.0096 * k) for k in range(100))


def round_down_wave():
    return speech(ROUND_DOWN_RATE, 77, ROUND_DOWN_FRAMES * HOP, 0.6)


def round_down_split(tp):
    """(ceilings whose gain is NOT (float)(ceiling / tp): the loop stepped down; the others), every one with the ceiling applying"""
    needs, plain = [], []
    for c in ROUND_DOWN_CEILINGS:
        q = LR.ask(ROUND_DOWN_GAIN, 0.0, c, LR.CEILING)
        assert ROUND_DOWN_GAIN * tp > float(c)                       # the ceiling applies
        g = LR.gain(q, 0.0, tp)
        assert F(float(g) * tp) <= c
        (plain if g == F(float(c) / tp) else needs).append(c)
    return needs, plain


# ---- launch groups ----------------------------------------------------------------------------------------------------------------------

def group_ends(Ts, hop):
    """one past the last utterance of every launch group: consecutive utterances while their capacities, each rounded up to whole
    chunks of 256 samples, stay within 2^26 samples; a group holds one utterance at least"""
    ends, first = [], 0
    while first < len(Ts):
        total, u = 0, first
        while u < len(Ts):
            p = -(-(Ts[u] * hop) // LR.CHUNK) * LR.CHUNK
            if u > first and total + p > GROUP_SAMPLES:
                break
            total += p
            u += 1
        ends.append(u)
        first = u
    return ends
