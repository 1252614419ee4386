"""Inputs that take resampling (include/zerovox_amd.h "resampling") through every path of its kernel, and the proof that they get there:
every shape comes with an assertion computed from the restatement's own intermediate values (tests/resample_rule.py), so a shape that
misses its branch fails on the CPU, before a device is asked.  Shared by tests/test_resample_cpu.py (which runs every assertion here
without a device, and holds the restatement against csrc/resample.h's reference) and tests/test_gpu_resample.py.

The kernel's tile (csrc/resample.h resample_tile, restated in tile() below and held against the native plan by the CPU test): a workgroup
covers R * S consecutive outputs, S = L * max(1, 512 div L) slots of R outputs of one phase each, R the largest of 8, 4, 2, 1 whose tile
stages at most 8 000 input samples [i0(first) - half + 1, i0(last) + half]; the reduction is a wave per utterance over the tiles."""
from types import SimpleNamespace

import numpy as np

import loudness_shapes as LS
import resample_rule as RR

F = np.float32
SR = 22050
SLOTS, STAGE = 512, 8000
CHUNK, GROUP_SAMPLES = 256, 1 << 26
# (L, M, P) of the caller's tables; the last one is there for the tile of one output per slot (R = 1)
TABLES = ((1, 1, 2), (3, 2, 4), (2, 3, 6), (7, 1, 2), (1, 6, 16), (320, 147, 8), (160, 441, 24), (1280, 441, 2), (1, 1, 512), (1, 8, 4))


def tile_srd(L, M, P):
    """(S, D, R) of csrc/resample.h resample_tile"""
    k = SLOTS // L if L <= SLOTS else 1
    S, R = L * k, 8
    while R > 1 and (L - 1 + (R * S - 1) * M) // L + P > STAGE:
        R //= 2
    return S, M * k, R


def tile(L, M, P):
    """the outputs one workgroup covers"""
    S, _, R = tile_srd(L, M, P)
    return R * S


def targets(L, M, P):
    """the output counts on either side of the tile's end and of two tiles' end"""
    T = tile(L, M, P)
    return (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)


SEEDS = (0, 1, 0xFFFFFFFF)
DESIGNED = ((22050, 48000), (22050, 8000), (22050, 16000), (48000, 22050))
SPECIALS = (np.nan, np.inf, -np.inf, -0.0)


def table(L, M, P, seed=0):
    """random entries in (-1, 1), an eighth of them exactly zero: no low-pass, the rule takes any finite table"""
    rng = np.random.default_rng(1000 * L + 10 * P + M + seed)
    h = rng.uniform(-1.0, 1.0, (L, P)).astype(F)
    h[rng.random((L, P)) < 0.125] = F(0)
    h[0, 0], h[-1, -1] = -abs(h[0, 0]) - F(0.125), F(0)                # a negative and a zero entry in every table
    assert (h < 0).any() and (h == 0).any()
    return h


def noise(seed, n, amp=0.5):
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, n) * amp).astype(F)


def speech(seed, n, amp=0.3):
    return LS.speech(SR, seed, n, amp)


def first_length(t, L, M):
    """the shortest input with at least t outputs"""
    return (t - 1) * M // L + 1


def lengths(L, M, P):
    """the input lengths of a table's cases: 1, 2, half - 1, half, and for every target count the shortest input that reaches it"""
    half = P // 2
    S = {1, 2, max(half - 1, 1), half}
    for t in targets(L, M, P):
        s = first_length(t, L, M)
        assert RR.count(s, L, M) >= t and (s == 1 or RR.count(s - 1, L, M) < t)
        S.add(s)
    return sorted(S)


def check_targets():
    """every table has a count on either side of both ends of ITS tile, a table with L <= M reaches every target count exactly, and the
    tables take the kernel through R = 8, 4, 2 and 1 and through two and five passes of its 256 threads over the slots"""
    seen = set()
    for L, M, P in TABLES:
        counts = [RR.count(s, L, M) for s in lengths(L, M, P)]
        T = tile(L, M, P)
        for e in (T, 2 * T):
            assert any(c <= e for c in counts) and any(e < c <= e + max(L // M, 1) + 1 for c in counts), (L, M, counts)
        if L <= M:
            assert set(targets(L, M, P)) <= set(counts), (L, M, counts)
        S, D, R = tile_srd(L, M, P)
        seen.add(("R", R))
        seen.add(("passes", -(-S // 256)))
    assert {("R", 8), ("R", 4), ("R", 2), ("R", 1), ("passes", 2), ("passes", 5)} <= seen, seen


def last_base_lengths(L, M):
    """(a length whose last output has i0 == S_in - 1, one whose last output has not), for a table with M > L"""
    yes = no = None
    for S in range(40, 80):
        n = RR.count(S, L, M) - 1
        if (n * M) // L == S - 1:
            yes = yes or S
        else:
            no = no or S
    assert yes and no, (L, M)
    return yes, no


def special_positions(L, M, P, S, tile=1):
    """the first and the last sample, and the samples just either side of tile `tile`'s staged span, inside [0, S)"""
    half = P // 2
    n_out = RR.count(S, L, M)
    T = globals()["tile"](L, M, P)
    n0, n1 = tile * T, min((tile + 1) * T, n_out) - 1
    assert n0 < n_out
    lo, hi = (n0 * M) // L - half + 1, (n1 * M) // L + half
    edge = [g for g in (lo - 1, lo, hi, hi + 1) if 0 <= g < S]
    assert len(edge) >= 2, (L, M, P, S, lo, hi)
    return [0, S - 1] + edge


def special_cases():
    """(name, L, M, table, x): every special value at every special position, one value per position and rotated from case to case"""
    out = []
    for (L, M, P), S in (((3, 2, 4), 3500), ((160, 441, 24), 7000), ((320, 147, 8), 1500), ((1, 1, 512), 5000)):
        pos = special_positions(L, M, P, S)
        for rot in range(len(SPECIALS)):
            x = noise(7 + rot, S)
            for i, g in enumerate(pos):
                x[g] = SPECIALS[(i + rot) % len(SPECIALS)]
            out.append(("special %d/%d/%d rot %d" % (L, M, P, rot), L, M, table(L, M, P), x))
    return out


def square(n=3000, period=44):
    t = np.arange(n)
    return np.where((t // (period // 2)) % 2 == 0, 1.0, -1.0).astype(F)


def ragged_batch():
    """seven utterances: one sample, two, less than a tile of outputs, several tiles, silence, not finite, speech"""
    xs = [noise(41, 1), noise(42, 2), noise(43, 200), speech(44, 3000), np.zeros(777, F), noise(46, 1500, 1.5), speech(47, 513, 0.9)]
    xs[5][[0, 700, 701, 1499]] = SPECIALS
    return xs


def padded(n):
    return -(-n // CHUNK) * CHUNK


def group_ends(S, L, M):
    """one past the last utterance of every launch group: consecutive utterances while their input plus output samples, each rounded up
    to whole chunks of 256, stay within 2^26; a group holds one utterance at least and 65 535 at the most"""
    ends, first = [], 0
    while first < len(S):
        total, u = 0, first
        while u < len(S) and u - first < 65535:
            p = padded(S[u]) + padded(RR.count(S[u], L, M))
            if u > first and total + p > GROUP_SAMPLES:
                break
            total += p
            u += 1
        ends.append(u)
        first = u
    return ends


def group_batch(big):
    """(lengths, L, M, the table) of a batch that crosses a launch group's end: six utterances of `big` samples (zv_max_frames() * hop)
    fill the first group with their inputs and an eighth as many outputs, the seventh opens the second; a two-tap table at 1 : 8 keeps
    the rule cheap"""
    S = [big] * 7 + [5000, 300, 1, 1025]
    per = padded(big) + padded(RR.count(big, 1, 8))
    assert 6 * per <= GROUP_SAMPLES < 7 * per and group_ends(S, 1, 8) == [6, 11]
    return S, 1, 8, np.array([[0.75, -0.5]], F)


def case(name, L, M, h, x):
    return SimpleNamespace(name=name, L=L, M=M, table=h, x=np.asarray(x, F))


def cases():
    """every single-call case of the GPU tests with a caller's table"""
    out = []
    for L, M, P in TABLES:
        h = table(L, M, P)
        for S in lengths(L, M, P):
            out.append(case("table %d/%d/%d S %d" % (L, M, P, S), L, M, h, noise(S, S, 0.8)))
        if M > L:
            for S in last_base_lengths(L, M):
                out.append(case("table %d/%d/%d last base S %d" % (L, M, P, S), L, M, h, noise(S, S, 0.8)))
    for name, L, M, h, x in special_cases():
        out.append(case(name, L, M, h, x))
    out.append(case("silence", 3, 2, table(3, 2, 4), np.zeros(1000, F)))
    return out
