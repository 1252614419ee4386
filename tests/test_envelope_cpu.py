"""Amplitude envelope (include/zerovox_amd.h "amplitude envelope") on the CPU: csrc/envelope.h against its restatement in Python
integers and single float64 steps (tests/envelope_rule.py), bit for bit.
 * tests/native/envelope_check.cpp drives zv::envelope_reference (and zv::level_reference behind it, for the cases with a volume) over
   the named edge classes and a few thousand random cases: the knots, a hash of every scaled sample and the level must agree;
 * the same input through a build with -fsanitize=address,undefined;
 * the properties the header states, and a handful of results written out by hand;
 * the boundary: the three entry points are declared, exported and bound with their _volume counterpart's arguments plus one pointer,
   refuse a NULL model by name, the binding refuses bad envelopes before it touches a device, and the CLI knows its flags."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import envelope_rule as ER
import level_rule as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
CLI = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
NAMES = ("zv_synthesize_envelope", "zv_synthesize_batch_envelope", "zv_synthesize_batch_begin_envelope")
F = np.float32
SPECIALS = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x7f7fffff], np.uint32).view(F)


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "envelope_check.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("envelope_check")
    return _build(tmp, "envelope_check", []), _build(tmp, "envelope_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# ---- cases ------------------------------------------------------------------------------------------------------------------

def _wave(rng, total, specials=False):
    x = (rng.standard_normal(total) * 0.3).astype(F)
    if specials and total:
        at = rng.integers(0, total, size=min(total, 6))
        x[at] = SPECIALS[:len(at)]
    return x


def _case(name, rng, T, hop, raw, gains, r, Fi, Fo, volume=None, specials=False):
    """raw: the durations before the capacity cuts them (their scan is what the library keeps)"""
    raw = [int(d) for d in raw]
    cum = np.cumsum(raw).astype(np.int64)
    clipped = np.diff(np.minimum(np.concatenate([[0], cum]), T)).astype(int).tolist()
    return dict(name=name, T=T, hop=hop, cum=cum.tolist(), dur=clipped, gains=None if gains is None else np.asarray(gains, F), r=r, Fi=int(Fi),
                Fo=int(Fo), volume=volume, x=_wave(rng, T * hop, specials))


def _named(rng):
    c = []
    for Fo in (0, 3):
        c.append(_case(f"nf = 0, Fo = {Fo}", rng, 5, 4, [0, 0, 0], [2.0, 0.5, 1.0], 1, 2, Fo))
        c.append(_case(f"nf = 0, Fo = {Fo}, volume", rng, 5, 4, [0, 0], None, 0, 0, Fo, volume=(1.5, 0.1, 0.5)))
    c.append(_case("one frame", rng, 4, 5, [1], [3.0], 2, 0, 0))
    c.append(_case("one frame, fades", rng, 1, 7, [0, 1, 0], [3.0, 0.25, 9.0], 0, 3, 3))
    c.append(_case("one phoneme", rng, 12, 4, [9], [0.75], 3, 0, 0))
    c.append(_case("phonemes of 0 frames between others", rng, 20, 4, [3, 0, 0, 4, 0, 5, 0], [1, 16, 0, 2, 7, 0.5, 3], 1, 0, 0))
    c.append(_case("a phoneme cut off by T", rng, 10, 4, [4, 9, 5], [1.0, 2.0, 8.0], 1, 0, 0))
    c.append(_case("a phoneme cut off by T, fades and volume", rng, 10, 3, [4, 9, 5], [1.0, 2.0, 8.0], 2, 7, 9, volume=(1.0, 0.2, 0.0)))
    for r in (0, 64):
        c.append(_case(f"r = {r}", rng, 200, 2, [70, 3, 80, 1, 30], [1.0, 4.0, 0.5, 16.0, 2.0], r, 0, 0))
    c.append(_case("r larger than the utterance", rng, 9, 4, [2, 3, 1], [0.5, 2.0, 1.5], 40, 0, 0))
    c.append(_case("gains 0 and 16", rng, 16, 4, [5, 5, 5], [0.0, 16.0, 0.0], 1, 0, 0))
    c.append(_case("all gains 16, r = 64", rng, 140, 1, [140], [16.0], 64, 0, 0))
    n = 6 * 5
    for Fi, Fo in ((n, 0), (0, n), (n + 5, n + 5), (n, n), (1, 1), (4, 4), (20, 20), (25, 11), (2 ** 31 - 1, 2 ** 31 - 1)):
        c.append(_case(f"Fi = {Fi}, Fo = {Fo} of n = {n}", rng, 8, 5, [2, 4], [1.0, 2.0], 1, Fi, Fo))
    for hop in (1, 3, 5, 7, 10):
        c.append(_case(f"hop = {hop}", rng, 9, hop, [2, 0, 3, 2], [1.0, 5.0, 0.25, 3.0], 1, 2, 3, volume=(0.9, 0.0, 0.3)))
    c.append(_case("NaN, inf, -0.0 samples", rng, 8, 4, [3, 3], [0.0, 2.0], 0, 3, 3, specials=True))
    c.append(_case("NaN, inf, -0.0 samples, volume", rng, 8, 4, [3, 3], [1.0, 2.0], 1, 0, 0, volume=(1.0, 0.1, 0.5), specials=True))
    c.append(_case("-0.0 gains", rng, 8, 4, [3, 3], [-0.0, 1.0], 0, 0, 0))
    c.append(_case("no gains, r and fades", rng, 8, 4, [3, 3], None, 5, 6, 6))
    return c


def _random(rng, count):
    c = []
    for k in range(count):
        T, hop = int(rng.integers(1, 25)), int(rng.choice([1, 2, 3, 4, 5, 7, 12]))
        n = int(rng.integers(1, 9))
        raw = rng.integers(0, 7, size=n) * (rng.random(n) < 0.75)
        gains = None
        if rng.random() < 0.85:
            gains = np.where(rng.random(n) < 0.3, rng.choice([0.0, 1.0, 16.0], size=n), rng.random(n) * (16.0 if k % 2 else 2.0)).astype(F)
        r = int(rng.choice([0, 1, 2, 3, 7, 64, int(rng.integers(0, 65))]))
        ns = min(int(np.sum(raw)), T) * hop
        fade = lambda: int(rng.choice([0, 0, 1, max(hop - 1, 0), ns, ns + 5, int(rng.integers(0, ns + 8))]))
        vol = None
        if rng.random() < 0.35:
            vol = (float(F(rng.random() * 3)), float(F(rng.random() * 0.3)) if rng.random() < 0.6 else 0.0,
                   float(F(rng.random())) if rng.random() < 0.6 else 0.0)
        c.append(_case(f"random {k}", rng, T, hop, raw, gains, r, fade(), fade(), volume=vol, specials=rng.random() < 0.1))
    return c


def _hex(v):
    return " ".join("%x" % b for b in ER.bits(v))


def _stdin(cases):
    lines = []
    for c in cases:
        lines.append(f"{c['T']} {c['hop']} {len(c['cum'])} {c['r']} {c['Fi']} {c['Fo']} {int(c['gains'] is not None)} {int(c['volume'] is not None)}")
        lines.append(" ".join(map(str, c["cum"])))
        if c["gains"] is not None:
            lines.append(_hex(c["gains"]))
        if c["volume"] is not None:
            lines.append(_hex(np.array(c["volume"], F)))
        lines.append(_hex(c["x"]))
    return "\n".join(lines) + "\n"


def _hash(v):
    b = ER.bits(v).astype(object)
    return int(sum(int(x) * (i + 1) for i, x in enumerate(b)) % (1 << 64))


def _expect(c):
    r = ER.rule(c["x"], c["dur"], c["T"], c["hop"], (c["gains"], c["r"], c["Fi"], c["Fo"]))
    line = [str(r["nf"])] + [str(b) for b in r["B"]] + [str(_hash(r["out"]))]
    if c["volume"] is not None:
        v = LR.rule(r["out"], r["nf"] * c["hop"], c["volume"])
        line += [str(v["S"])] + ["%x" % b for b in LR.level_bits(v["level"])] + [str(_hash(v["out"]))]
    return " ".join(line)


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(20261020)
    return _named(rng) + _random(rng, 3000)


# ---- 1. header against restatement ------------------------------------------------------------------------------------------

def test_header_agrees_with_the_restatement_bit_for_bit(exes, cases):
    exe, _ = exes
    r = subprocess.run([exe], input=_stdin(cases), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.strip().split("\n")
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert g == _expect(c), (c["name"], c["T"], c["hop"], c["dur"], c["r"], c["Fi"], c["Fo"])
    names = " | ".join(c["name"] for c in cases[:60])
    for cls in ("nf = 0, Fo = 0", "nf = 0, Fo = 3", "one frame", "one phoneme", "0 frames between", "cut off by T", "r = 0", "r = 64",
                "r larger than", "gains 0 and 16", "Fi = 35, Fo = 35", "Fi = 25, Fo = 11", "hop = 7", "NaN, inf"):
        assert cls in names, cls


def test_header_under_address_and_undefined_sanitizers(exes, cases):
    """the stand-alone check program built with -fsanitize=address,undefined gives the same output and reports nothing"""
    exe, san = exes
    text = _stdin(cases[:60] + cases[60::10])
    a = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    b = subprocess.run([san], input=text, capture_output=True, text=True, timeout=600)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr[-1000:], b.stderr[-3000:])
    assert a.stdout == b.stdout and b.stderr == ""


# ---- 2. results written out by hand -----------------------------------------------------------------------------------------

def test_named_results():
    one = ER.ONE
    # gains [1, 2] over [3, 5] frames, r = 0: a knot is the sum of the two frame gains it sits between
    F_ = ER.frame_gains([3, 5], [1.0, 2.0], 8)
    assert F_ == [one] * 3 + [2 * one] * 5
    assert ER.knots(F_, 0) == [k * one for k in (2, 2, 2, 3, 4, 4, 4, 4, 4)]
    x = np.ones(16, F)
    r = ER.rule(x, [3, 5], 8, 2, ([1.0, 2.0], 0, 0, 0))
    assert r["out"].tolist() == [1, 1, 1, 1, 1, 1.25, 1.5, 1.75, 2, 2, 2, 2, 2, 2, 2, 2]
    # a fade-in over 4 samples: s / 4; a fade-out over 4: the last sample is 0, the one before it a quarter
    r = ER.rule(x, [3, 5], 8, 2, ([1.0, 2.0], 0, 4, 4))
    assert r["out"].tolist() == [0, 0.25, 0.5, 0.75, 1, 1.25, 1.5, 1.75, 2, 2, 2, 2, 1.5, 1.0, 0.5, 0]
    # gains [1, 3] over [4, 4] frames, r = 1: windows of 3, knots / 6 = 1, 1, 1, 4/3, 2, 8/3, 3, 3, 3 — four frames centred on frame 4
    assert ER.knots(ER.frame_gains([4, 4], [1.0, 3.0], 8), 1) == [k * one for k in (6, 6, 6, 8, 12, 16, 18, 18, 18)]
    r = ER.rule(np.ones(8, F), [4, 4], 8, 1, ([1.0, 3.0], 1, 0, 0))
    assert np.array_equal(r["out"], (np.array([6, 6, 6, 8, 12, 16, 18, 18], np.float64) / 6.0).astype(F))
    # a capacity of 10 behind 8 frames of speech: the tail keeps the last knot without a fade-out and is silent with one
    r = ER.rule(np.ones(10, F), [4, 4], 10, 1, ([1.0, 3.0], 1, 0, 0))
    assert r["out"][8:].tolist() == [3.0, 3.0]
    r = ER.rule(np.ones(10, F), [4, 4], 10, 1, ([1.0, 3.0], 1, 0, 2))
    assert r["out"][5:].tolist() == [F(16 / 6), 1.5, 0.0, 0.0, 0.0]
    # fixed-point gains: 0.5 ulp of 2^-16 rounds up, -0.0 is 0, 16 is 2^20
    assert [ER.fixed_gain(g) for g in (0.0, -0.0, 1.0, 16.0, 2.0 ** -17, 2.0 ** -18)] == [0, 0, one, 1 << 20, 1, 0]
    # nothing to fade: an utterance without speech keeps its bits, or is silenced by a fade-out
    assert ER.rule(x, [0, 0], 8, 2, ([4.0, 4.0], 3, 5, 0))["out"].tolist() == [1.0] * 16
    assert ER.rule(x, [0, 0], 8, 2, ([4.0, 4.0], 3, 5, 1))["out"].tolist() == [0.0] * 16
    # the largest knot and numerator stay inside their integers
    B = ER.knots([1 << 20] * 200, 64)
    assert max(B) == 2 * 129 * (1 << 20) < 1 << 29 and max(B) * 32768 < 1 << 53


def _native(exe, T, hop, raw, gains, r, Fi, Fo, x):
    """one case through the check program: (nf, the header's knots, the hash of the header's scaled samples)"""
    c = dict(T=T, hop=hop, cum=np.cumsum(raw).tolist(), gains=None if gains is None else np.asarray(gains, F), r=r, Fi=Fi, Fo=Fo, volume=None,
             x=np.asarray(x, F))
    p = subprocess.run([exe], input=_stdin([c]), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-1000:]
    f = [int(v) for v in p.stdout.split()]
    return f[0], f[1:-1], f[-1]


def test_named_results_through_the_header(exes):
    """the results written out by hand above, asked of csrc/envelope.h itself (zv::envelope_reference): literal knots, literal samples"""
    exe, _ = exes
    one = ER.ONE
    ones = lambda n: np.ones(n, F)
    lit = lambda v: _hash(np.array(v, F))
    assert _native(exe, 8, 2, [3, 5], [1.0, 2.0], 0, 0, 0, ones(16)) == \
        (8, [k * one for k in (2, 2, 2, 3, 4, 4, 4, 4, 4)], lit([1, 1, 1, 1, 1, 1.25, 1.5, 1.75, 2, 2, 2, 2, 2, 2, 2, 2]))
    assert _native(exe, 8, 2, [3, 5], [1.0, 2.0], 0, 4, 4, ones(16)) == \
        (8, [k * one for k in (2, 2, 2, 3, 4, 4, 4, 4, 4)], lit([0, 0.25, 0.5, 0.75, 1, 1.25, 1.5, 1.75, 2, 2, 2, 2, 1.5, 1.0, 0.5, 0]))
    k1 = [k * one for k in (6, 6, 6, 8, 12, 16, 18, 18, 18)]
    assert _native(exe, 8, 1, [4, 4], [1.0, 3.0], 1, 0, 0, ones(8)) == (8, k1, lit((np.array([6, 6, 6, 8, 12, 16, 18, 18], np.float64) / 6.0).astype(F)))
    third = (np.array([6, 6, 6, 8, 12, 16], np.float64) / 6.0).astype(F).tolist()
    assert _native(exe, 10, 1, [4, 4], [1.0, 3.0], 1, 0, 0, ones(10)) == (8, k1, lit(third + [3.0, 3.0, 3.0, 3.0]))      # the tail: the last knot
    assert _native(exe, 10, 1, [4, 4], [1.0, 3.0], 1, 0, 2, ones(10)) == (8, k1, lit(third[:5] + [F(16 / 6), 1.5, 0.0, 0.0, 0.0]))
    # a phoneme cut by the capacity: [4, 9] in 6 frames is [4, 2]
    assert _native(exe, 6, 1, [4, 9], [1.0, 2.0], 0, 0, 0, ones(6)) == (6, [k * one for k in (2, 2, 2, 2, 3, 4, 4)], lit([1, 1, 1, 1, 1.5, 2]))
    # no speech: no knots; the bits stay without a fade-out, silence with one
    assert _native(exe, 8, 2, [0, 0], [4.0, 4.0], 3, 5, 0, ones(16)) == (0, [], lit([1.0] * 16))
    assert _native(exe, 8, 2, [0, 0], [4.0, 4.0], 3, 5, 1, ones(16)) == (0, [], lit([0.0] * 16))
    # fixed-point gains: half an ulp of 2^-16 rounds up, -0.0 is 0, 16 is 2^20 (r = 0: a knot inside a phoneme is twice its G)
    nf, B, _h = _native(exe, 12, 1, [2] * 6, [0.0, -0.0, 1.0, 16.0, 2.0 ** -17, 2.0 ** -18], 0, 0, 0, ones(12))
    assert nf == 12 and B[1::2] == [0, 0, 2 * one, 2 << 20, 2, 0]
    # the identity keeps every bit, special values included (NaNs of the quiet kind: a multiply leaves their payload alone)
    x = np.concatenate([SPECIALS, np.array([0.1, -0.7], F)])
    nf, B, h = _native(exe, 4, 2, [1, 3], [1.0, 1.0], 64, 0, 0, x)
    assert nf == 4 and B == [2 * 129 * one] * 5 and h == _hash(x)


# ---- 3. what follows from the rule ------------------------------------------------------------------------------------------

def _curves(cases):
    """(case, rule result on a waveform of ones) for the cases without special samples"""
    for c in cases:
        x = np.ones(c["T"] * c["hop"], F)
        yield c, ER.rule(x, c["dur"], c["T"], c["hop"], (c["gains"], c["r"], c["Fi"], c["Fo"]))


def _owned_gains(c):
    return [ER.ONE if c["gains"] is None else ER.fixed_gain(g) for g, d in zip(c["gains"] if c["gains"] is not None else c["dur"], c["dur"]) if d > 0]


def test_curve_is_continuous_plateaus_are_exact_and_bounded(cases):
    plateaus = transitions = 0
    for c, r in _curves(cases):
        if r["nf"] == 0:
            continue
        hop, rr, W, nf = c["hop"], c["r"], 2 * c["r"] + 1, r["nf"]
        G = _owned_gains(c)
        lo, hi = F(np.float64(min(G)) / 65536.0), F(np.float64(max(G)) / 65536.0)
        B = r["B"]
        # continuity: a frame's line ends where the next begins (the knots are shared) and a sample's step is bounded by the largest
        # difference of two knots, 2 * (max G - min G), spread over a frame
        assert all(abs(B[f + 1] - B[f]) <= 2 * (max(G) - min(G)) for f in range(nf))
        if c["Fi"] == 0 and c["Fo"] == 0:
            e = r["e"].astype(np.float64)
            assert e.min() >= lo and e.max() <= hi, c["name"]                      # never leaves [min G, max G] / 65536
            step = (max(G) - min(G)) / (W * hop * 65536.0)
            assert np.abs(np.diff(e)).max(initial=0.0) <= step + 2.0 ** -23 * float(hi), c["name"]      # + two f32 roundings of 2^-24 * hi each
            assert np.all(r["e"][nf * hop:] == F(np.float64(B[nf] * hop) / np.float64(2 * W * hop * 65536))), c["name"]      # the tail: the last knot
            # inside a phoneme of more than 2r + 2 frames: exactly (float)(G_i / 65536) from r + 1 frames in to r + 1 frames before its end
            start = 0
            for i, d in enumerate(c["dur"]):
                if d > 2 * rr + 2:
                    Gi = ER.ONE if c["gains"] is None else ER.fixed_gain(c["gains"][i])
                    a, b = (start + rr + 1) * hop, (start + d - rr - 1) * hop
                    assert np.all(r["e"][a:b + 1] == F(np.float64(Gi) / 65536.0)), (c["name"], i)
                    assert b - a == (d - 2 * rr - 2) * hop >= hop          # one whole frame when the phoneme has exactly 2r + 3
                    plateaus += 1
                    if i + 1 < len(c["dur"]) and c["dur"][i + 1] > 2 * rr + 2:
                        # a transition spans 2r + 2 frames centred on the boundary: exact plateaus at both of its ends
                        bd = start + d
                        Gn = ER.ONE if c["gains"] is None else ER.fixed_gain(c["gains"][i + 1])
                        assert B[bd - rr - 1] == 2 * W * Gi and B[bd + rr + 1] == 2 * W * Gn
                        transitions += 1
                start += d
    assert plateaus > 50 and transitions > 10, (plateaus, transitions)          # the cases held enough of both


def test_identity_keeps_every_bit(cases):
    rng = np.random.default_rng(7)
    for c in cases[::7]:
        x = _wave(rng, c["T"] * c["hop"], specials=True)
        n = len(c["dur"])
        for env in (ER.IDENTITY, (np.ones(n, F), 0, 0, 0), (np.ones(n, F), 64, 0, 0), (None, c["r"], 0, 0), (np.ones(n, F), c["r"], 0, 0)):
            r = ER.rule(x, c["dur"], c["T"], c["hop"], env)
            assert np.all(r["e"] == F(1.0))
            nan = np.isnan(x)
            assert np.array_equal(ER.bits(r["out"])[~nan], ER.bits(x)[~nan]) and np.isnan(r["out"][nan]).all()
            W = 2 * env[1] + 1
            assert all(b * c["hop"] == 2 * W * c["hop"] * 65536 for b in r["B"])       # num == den


def test_fitted_zeros_stay_zero_and_a_fade_out_silences_the_tail(cases):
    rng = np.random.default_rng(8)
    for c in cases[::5]:
        x = _wave(rng, c["T"] * c["hop"])
        ns = sum(c["dur"]) * c["hop"]
        x[ns:] = 0.0
        r = ER.rule(x, c["dur"], c["T"], c["hop"], (c["gains"], c["r"], c["Fi"], c["Fo"]))
        assert not r["out"][ns:].any(), c["name"]
        x[ns:] = 0.25
        r = ER.rule(x, c["dur"], c["T"], c["hop"], (c["gains"], c["r"], c["Fi"], c["Fo"]))
        if c["Fo"] > 0:
            assert not r["out"][max(ns - 1, 0):].any(), c["name"]


# ---- 4. the boundary --------------------------------------------------------------------------------------------------------

def _declaration(header, name):
    m = re.search(r"zv_status\s+%s\s*\((.*?)\)\s*;" % name, header, flags=re.S)
    assert m, name
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    return [re.sub(r"\s*\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace(" *", "*") for p in params]


def test_entry_points_are_declared_exported_and_bound():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zerovox_amd.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in capi.SYMBOLS, name
    for name in ("zv_synthesize", "zv_synthesize_batch", "zv_synthesize_batch_begin"):
        assert _declaration(header, name + "_envelope") == _declaration(header, name + "_volume") + ["const zv_envelope*"], name
        assert getattr(lib, name + "_envelope").argtypes == getattr(lib, name + "_volume").argtypes + [C.POINTER(capi.EnvelopeC)]
    assert not re.search(r"\bzv_synthesize_batch_end_envelope\b", header)          # the existing _end finishes an envelope batch
    assert C.sizeof(capi.EnvelopeC) == 24 and bytes(capi.EnvelopeC()) == bytes(24)    # zero-initialised = identity
    assert re.search(r"typedef struct\s*\{\s*const float \*phoneme_gain;\s*uint32_t\s+ramp_frames;\s*uint32_t\s+fade_in_samples;\s*"
                     r"uint32_t\s+fade_out_samples;\s*\}\s*zv_envelope;", header)
    text = open(os.path.join(CSRC, "envelope.h")).read()
    assert "ENV_MAX_RAMP = 64" in text and "ENV_MAX_GAIN = 16.0f" in text
    assert (capi.ENVELOPE_MAX_GAIN, capi.ENVELOPE_MAX_RAMP, capi.ENVELOPE_MAX_FADE) == (16.0, 64, 0x7fffffff)


def test_null_model_is_refused_by_every_entry_point():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    n = C.c_uint32(0)
    env = capi.EnvelopeC()
    assert lib.zv_synthesize_envelope(None, None, None, None, 4, 8, None, C.byref(n), None, None, None, 0, 0, None, None, C.byref(env)) == 5
    assert b"zv_synthesize_envelope" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_envelope(None, 1, None, None, None, None, None, None, None, None, None, None, None, 0, None, None, env) == 5
    assert b"zv_synthesize_batch_envelope" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_begin_envelope(None, 0, 1, None, None, None, None, None, None, None, None, None, None, None, 0, None, None,
                                                  env) == 5
    assert b"zv_synthesize_batch_begin_envelope" in lib.zv_last_error()


class _NoDevice:
    """stands where a capi.Model would: any touch of the library or the handle fails the test"""
    hp = types.SimpleNamespace(audio_hop_size=300)

    def __getattr__(self, name):
        raise AssertionError(f"the binding touched .{name} before it had checked its arguments")


BAD = [(dict(phoneme_gain=[1, float("nan"), 1, 1]), r"phoneme_gain\[1\] = nan is not finite"),
       (dict(phoneme_gain=[1, 1, 1, float("inf")]), r"phoneme_gain\[3\] = inf is not finite"),
       (dict(phoneme_gain=[-0.5, 1, 1, 1]), r"phoneme_gain\[0\] = -0.5 is outside \[0, 16\]"),
       (dict(phoneme_gain=[1, 1, 16.5, 1]), r"phoneme_gain\[2\] = 16.5 is outside \[0, 16\]"),
       (dict(phoneme_gain=[1, 1, 1]), r"phoneme_gain has shape \(3,\), the utterance has 4 phonemes"),
       (dict(ramp_frames=65), r"ramp_frames = 65 is outside \[0, 64\]"), (dict(ramp_frames=-1), r"ramp_frames = -1 is outside \[0, 64\]"),
       (dict(fade_in_samples=1 << 31), r"fade_in_samples = 2147483648 is outside \[0, 2147483647\]"),
       (dict(fade_out_samples=-3), r"fade_out_samples = -3 is outside \[0, 2147483647\]")]


def test_binding_refuses_bad_envelopes_before_touching_a_device():
    from zerovox_cpp_amd import capi
    ids, puncts, style = np.ones(4, np.int32), np.zeros(4, np.int32), np.zeros(528, np.float32)
    fake = _NoDevice()
    two = [(ids, puncts, style, 64), (ids, puncts, style, 7)]
    for bad, msg in BAD:
        with pytest.raises(ValueError, match="envelope " + msg):
            capi.Model.synthesize(fake, ids, puncts, style, 64, envelope=bad)
        with pytest.raises(ValueError, match="utterance 1: envelope " + msg):
            capi.BatchCall(fake, two, envelope=[None, capi.Envelope(**bad)])
    for bad in (dict(ramp_frames=1.5), dict(ramp_frames=True), dict(fade_in_samples="3"), dict(fade_out_samples=None)):
        with pytest.raises(TypeError, match="must be an integer"):
            capi.Model.synthesize(fake, ids, puncts, style, 64, envelope=bad)
    with pytest.raises(ValueError, match="unknown envelope field"):
        capi.Model.synthesize(fake, ids, puncts, style, 64, envelope=dict(ramp=1))
    with pytest.raises(TypeError, match="an envelope is an Envelope"):
        capi.Model.synthesize(fake, ids, puncts, style, 64, envelope=(1, 2, 3))
    with pytest.raises(ValueError, match="envelope has 1 entries, the batch has 2"):
        capi.BatchCall(fake, two, envelope=[None])
    # a well-formed call is built without a device; None entries get the identity, set_envelope rewrites an entry and checks
    bc = capi.BatchCall(fake, two + [(ids, puncts, style, 9)], envelope=[dict(phoneme_gain=[1, 2, 3, 4], ramp_frames=2), None,
                                                                         capi.Envelope(fade_in_samples=5, fade_out_samples=6)])
    rows = lambda: [(bool(e.phoneme_gain), e.ramp_frames, e.fade_in_samples, e.fade_out_samples) for e in bc.envelope]
    assert rows() == [(True, 2, 0, 0), (False, 0, 0, 0), (False, 0, 5, 6)]
    assert bc.envelope[0].phoneme_gain == bc.ekeep[0].phoneme_gain.ctypes.data and bc.ekeep[0].phoneme_gain.tolist() == [1, 2, 3, 4]
    bc.set_envelope(1, capi.Envelope([0, 0, 16, 1], 64))
    bc.set_envelope(0, None)
    assert rows() == [(False, 0, 0, 0), (True, 64, 0, 0), (False, 0, 5, 6)]
    with pytest.raises(ValueError, match=r"utterance 2: envelope ramp_frames = 99 is outside \[0, 64\]"):
        bc.set_envelope(2, dict(ramp_frames=99))
    assert rows()[2] == (False, 0, 5, 6)
    plain = capi.BatchCall(fake, two)
    assert plain.envelope is None
    with pytest.raises(ValueError, match="built without envelopes"):
        plain.set_envelope(0, None)


def test_from_db():
    from zerovox_cpp_amd import capi
    e = capi.Envelope.from_db()
    assert e.phoneme_gain is None and (e.ramp_frames, e.fade_in_samples, e.fade_out_samples) == (0, 0, 0)
    e = capi.Envelope.from_db(phoneme_gain_db=[0, 6, -20], ramp_frames=3, fade_in_ms=20, fade_out_ms=12.5, rate=24000)
    assert e.phoneme_gain.dtype == F and e.phoneme_gain.tolist() == [1.0, F(10 ** 0.3), F(0.1)]
    assert (e.ramp_frames, e.fade_in_samples, e.fade_out_samples) == (3, 480, 300)
    assert capi.Envelope.from_db(fade_in_ms=0.03, rate=22050).fade_in_samples == 1          # floor(0.6615 + 0.5)
    with pytest.raises(ValueError, match="fade_out_ms needs rate"):
        capi.Envelope.from_db(fade_out_ms=5)


def test_call_variant_routes_an_envelope_to_the_envelope_symbol():
    from zerovox_cpp_amd import capi
    seen = []
    lib = types.SimpleNamespace(**{name: (lambda *a, _n=name: seen.append((_n, a)) or 0)
                                   for name in ("zv_synthesize", "zv_synthesize_target", "zv_synthesize_volume", "zv_synthesize_envelope")})
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev", "env")
    capi._call_variant(lib, "zv_synthesize", (1, 2), target=0, envelope="env")
    capi._call_variant(lib, "zv_synthesize", (1, 2), target=0, levels="lev")
    capi._call_variant(lib, "zv_synthesize", (1, 2))
    assert seen == [("zv_synthesize_envelope", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev", "env")),
                    ("zv_synthesize_envelope", (1, 2, None, None, None, 0, 0, None, None, "env")),
                    ("zv_synthesize_volume", (1, 2, None, None, None, 0, 0, None, "lev")), ("zv_synthesize", (1, 2))]


def test_cli_knows_the_flags(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(f in r.stdout for f in ("--phoneme-gain-db", "--ramp-frames", "--fade-in-ms", "--fade-out-ms"))
    utt = tmp_path / "utt.txt"
    utt.write_text("1 2 3\n0 0 0\n0\n")
    files = {"short": "0\n-6\n", "long": "0\n0\n0\n0\n", "word": "0\nloud\n0\n", "nan": "0\nnan\n0\n", "high": "0\n24.5\n0\n", "low": "0\n-201\n0\n",
             "two": "0 1\n0\n0\n"}
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    bad = [["--phoneme-gain-db", str(tmp_path / name)] for name in files] + [["--phoneme-gain-db", str(tmp_path / "missing")], ["--phoneme-gain-db"]]
    bad += [["--ramp-frames", v] for v in ("65", "-1", "1.5", "x")] + [["--ramp-frames"]]
    bad += [[f, v] for f in ("--fade-in-ms", "--fade-out-ms") for v in ("-1", "nan", "inf", "1e9", "5ms")] + [["--fade-in-ms"], ["--fade-out-ms"]]
    for args in bad:
        r = subprocess.run([CLI, "-m", "/nonexistent/model.gguf", "-u", str(utt)] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and args[0] in r.stderr, (args, r.returncode, r.stderr[-300:])
    # a well-formed file passes the usage checks: the run then fails at the missing checkpoint, which is no usage error
    (tmp_path / "good").write_text("0\n-6.5\n\n24.08\n")
    r = subprocess.run([CLI, "-m", "/nonexistent/model.gguf", "-u", str(utt), "--phoneme-gain-db", str(tmp_path / "good"), "--ramp-frames", "64",
                        "--fade-in-ms", "0", "--fade-out-ms", "12.5"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stderr[-300:])
