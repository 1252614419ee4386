"""Loudness (include/zerovox_amd.h "loudness") on the CPU: csrc/loudness.h against its restatement in single float64 steps
(tests/loudness_rule.py), bit for bit, and the rule against the standard.
 * tests/native/loudness_check.cpp drives zv::loud_reference at 22 050 Hz over N on both sides of four and of thirty steps, N a whole
   number of chunks and not, silence, a NaN and an infinity inside the span, leading silence (the absolute gate drops blocks) and a loud
   burst (the relative gate drops blocks), under asks of every kind: every field of the result and every output sample must agree;
 * the same comparison at 4 000 Hz (step 400: most chunks meet two steps), 5 120 Hz (step 512: no chunk holds an edge), 48 000 Hz and
   768 000 Hz (the highest rate the design takes): N = 0, N on both sides of four and of thirty steps of that rate, and N of 65 and 129
   blocks, more than one and more than two rounds of 64 of the gate kernel's loops;
 * the same inputs through a build with -fsanitize=address,undefined (a plain host program, nothing preloaded);
 * the ceiling's round-down step: a fixed waveform and a fixed list of ceilings of which some need it (tests/loudness_shapes.py);
 * the design: the standard's 48 kHz table within 1e-12, M against numpy's matrix power, the interpolator, the refused rates;
 * the decomposition is the standard: the chunked rule against one sequential pass over the whole signal with textbook gating;
 * conformance: EBU Tech 3341 cases 1, 3, 4 and 5 as mono at 22 050 Hz read -26.0 LUFS +- 0.1; EBU Tech 3341 true-peak tones of
   amplitude 0.5 read -6.0 dBTP +0.2 / -0.4;
 * the boundary: argument checks and messages without a device, the binding, an older library, the launch plan and the launch groups
   (loud_group_end, driven over lists of capacities: a sum of exactly 2^26 samples stays one group, one chunk more splits);
 * the shapes of tests/test_gpu_loudness_shapes.py reach what they are for (tests/loudness_shapes.py: asserted here, without a device)."""
import ctypes as C
import math
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

import loudness_rule as LR
import loudness_shapes as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
NAMES = ("zv_loudness_wave", "zv_loudness_wave_batch", "zv_loudness_design")
F = np.float32
SR, HOP = 22050, 300
STEP = 2205


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "loudness_check.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("loudness_check")
    return _build(tmp, "loudness_check", []), _build(tmp, "loudness_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _f64(word):
    return struct.unpack("<d", struct.pack("<Q", int(word, 16)))[0]


def native_design(exe, rate):
    t = subprocess.run([exe, "design", str(rate)], capture_output=True, text=True, timeout=60).stdout.split()
    if t[:1] == ["refused"]:
        return t[1]
    assert len(t) == 26 + 49 + 1, len(t)
    d = [_f64(v) for v in t[:26]]
    return types.SimpleNamespace(shelf_b=d[0:3], shelf_a=d[3:5], highpass_b=d[5:8], highpass_a=d[8:10], M=d[10:26],
                                 c=np.array([int(v, 16) for v in t[26:75]], np.uint32).view(F), step=int(t[75]))


OTHER_RATES = (4000, 5120, 48000, 768000)


@pytest.fixture(scope="module")
def designs(exes):
    return {rate: native_design(exes[0], rate) for rate in (SR,) + OTHER_RATES}


@pytest.fixture(scope="module")
def D(designs):
    return designs[SR]


# ---- cases --------------------------------------------------------------------------------------------------------------------------------

def noise(seed, n, amp=0.1):
    return (np.random.default_rng(seed).standard_normal(n) * amp).astype(F)


def _cases():
    """(name, x [total], N, (gain, target, ceiling, flags), rate)"""
    none, target, ceiling, both = (1.0, 0.0, 0.0, 0), (1.0, -16.0, 0.0, 1), (2.0, 0.0, 0.25, 2), (1.5, -9.0, 0.2, 3)
    out = []
    for k, N in enumerate((4 * STEP - 1, 4 * STEP, 4 * STEP + 1, 30 * STEP - 1, 30 * STEP, 30 * STEP + 1, 256 * 80, 256 * 80 + 255, 255, 1)):
        out.append(("N=%d" % N, noise(k, N + 300), N, (none, target, ceiling, both)[k % 4]))
    out.append(("silent", np.zeros(6 * STEP + 300, F), 6 * STEP, target))
    x = noise(20, 8 * STEP)
    x[1000], x[5 * STEP + 17], x[5 * STEP + 18] = np.nan, np.inf, -np.inf
    out.append(("nan and inf", x, x.size, both))
    x = noise(21, 25 * STEP)
    x[:10 * STEP] = 0
    out.append(("leading silence", x, x.size, target))
    x = noise(22, 40 * STEP, 0.003)
    x[28 * STEP:36 * STEP] *= F(100.0)
    out.append(("loud burst", x, x.size, both))
    out.append(("denormal", noise(23, 6 * STEP, 1e-40), 6 * STEP, target))
    out.append(("huge", noise(24, 6 * STEP, 1e30), 6 * STEP, ceiling))
    out.append(("zero gain", noise(25, 6 * STEP), 6 * STEP, (0.0, -20.0, 0.5, 3)))
    out = [c + (SR,) for c in out]
    for r, rate in enumerate(OTHER_RATES):
        step = (rate + 5) // 10
        for k, N in enumerate(rate_lengths(step)):
            out.append(("%d Hz N=%d" % (rate, N), noise(100 + 10 * r + k, N + 300), N, (none, target, ceiling, both)[(k + r) % 4], rate))
    return out


def rate_lengths(step):
    """N = 0, both sides of four and of thirty steps, 65 blocks (68 steps and a rest) and 129 blocks (132 steps and a rest)"""
    return (0, 4 * step - 1, 4 * step, 30 * step - 1, 30 * step, 68 * step + 5, 132 * step + 1)


@pytest.fixture(scope="module")
def cases():
    return _cases()


def _native(exe, tmp, x, N, q, meter=False, rate=SR):
    src, dst = str(tmp / "in.f32"), str(tmp / "out.f32")
    x.tofile(src)
    fb = lambda v: "%x" % LR.fbits(v)
    r = subprocess.run([exe, "run", str(rate), str(N), str(x.size), fb(q[0]), fb(q[1]), fb(q[2]), str(q[3]), src, "-" if meter else dst],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    t = r.stdout.split()
    key = tuple(int(v, 16) for v in t[:4]) + tuple(int(v) for v in t[4:7]) + tuple(int(v, 16) for v in t[7:])
    return key, None if meter else np.fromfile(dst, F)


@pytest.fixture(scope="module")
def outputs(exes, cases, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("loudness_io")
    return [[_native(e, tmp, x, N, q, rate=rate) for _, x, N, q, rate in cases] for e in exes]


@pytest.fixture(scope="module")
def restated(designs, cases):
    return [LR.rule(designs[rate], x, N, LR.ask(*q)) for _, x, N, q, rate in cases]


# ---- 1. bit for bit ---------------------------------------------------------------------------------------------------------------------------

def test_header_equals_restatement_bit_for_bit(cases, outputs, restated):
    for (name, x, N, q, rate), (key, y), (res, out) in zip(cases, outputs[0], restated):
        assert key == LR.key(res), (name, key, LR.key(res))
        assert y.size == x.size and (y.view(np.uint32) == out.view(np.uint32)).all(), name


def test_sanitized_build_agrees(cases, outputs):
    for (name, *_), (key, y), (skey, sy) in zip(cases, outputs[0], outputs[1]):
        assert key == skey and (y.view(np.uint32) == sy.view(np.uint32)).all(), name


def test_meter_only_gives_the_same_result(exes, cases, outputs, tmp_path):
    for k in (1, 13):
        _, x, N, q, rate = cases[k]
        assert _native(exes[0], tmp_path, x, N, q, meter=True, rate=rate)[0] == outputs[0][k][0]


def test_the_cases_reach_what_they_are_for(cases, restated):
    by = {c[0]: r[0] for c, r in zip(cases, restated)}
    assert by["N=%d" % (4 * STEP - 1)].blocks == 0 and by["N=%d" % (4 * STEP)].blocks == 1 and by["N=%d" % (4 * STEP + 1)].blocks == 1
    assert math.isinf(by["N=%d" % (4 * STEP - 1)].integrated_lufs) and by["N=%d" % (4 * STEP - 1)].gain == F(1.0)
    a, b = by["N=%d" % (30 * STEP - 1)], by["N=%d" % (30 * STEP)]
    assert a.short_term_max_ms == 0.0 and math.isinf(a.short_term_max_lufs) and b.short_term_max_ms > 0.0 and b.blocks == 27
    s = by["silent"]
    assert (s.blocks, s.blocks_absolute, s.blocks_gated) == (3, 0, 0) and s.integrated_ms == 0.0 and s.gain == F(1.0) and s.true_peak == 0.0
    assert math.isinf(s.integrated_lufs) and math.isinf(s.true_peak_dbtp)
    lead = by["leading silence"]
    assert lead.blocks == 22 and 0 < lead.blocks_absolute < lead.blocks                     # the absolute gate drops the silent blocks
    burst = by["loud burst"]
    assert 0 < burst.blocks_gated < burst.blocks_absolute <= burst.blocks == 37             # the relative gate drops the quiet ones
    assert by["denormal"].blocks_absolute == 0 and by["denormal"].momentary_max_ms > 0.0
    assert by["zero gain"].gain == F(0.0)
    n = by["nan and inf"]
    assert np.isfinite(n.true_peak) and np.isfinite(n.integrated_ms) and n.blocks_gated > 0
    # a ceiling that applied holds: (float)((double)g * tp) <= ceiling
    for (name, x, N, q, rate), (res, _) in zip(cases, restated):
        if q[3] & 2:
            assert F(float(res.gain) * res.true_peak) <= F(q[2]), name
    # the other rates: the block counts on both sides of four and thirty steps, one and two rounds of 64 blocks passed, N = 0
    for rate in OTHER_RATES:
        step = (rate + 5) // 10
        r = [by["%d Hz N=%d" % (rate, N)] for N in rate_lengths(step)]
        assert [v.blocks for v in r] == [0, 0, 1, 26, 27, 65, 129], rate
        assert [v.short_term_max_ms > 0.0 for v in r] == [False, False, False, False, True, True, True], rate
        assert all(v.blocks_gated == v.blocks for v in r), rate               # steady noise: every block counts, in every round
        z = r[0]
        assert z.true_peak == 0.0 and z.sample_peak == 0.0 and z.integrated_ms == 0.0 and math.isinf(z.true_peak_dbtp)
        assert math.isinf(z.integrated_lufs) and math.isinf(z.momentary_max_lufs) and math.isinf(z.short_term_max_lufs)
    assert [(rate + 5) // 10 for rate in OTHER_RATES] == [400, 512, 4800, 76800]


def test_a_non_finite_sample_counts_as_zero(D):
    x = noise(30, 8 * STEP)
    y = x.copy()
    x[3000], x[9000] = np.nan, -np.inf
    y[3000], y[9000] = 0.0, 0.0
    assert LR.key(LR.rule(D, x, x.size)[0]) == LR.key(LR.rule(D, y, y.size)[0])


def test_some_ceilings_need_the_round_down_step(exes, D, tmp_path):
    """loud_gain's loop: (float)(ceiling / tp) may have rounded up, and then (float)(g tp) > ceiling.  One fixed waveform, one hundred
    fixed ceilings (tests/loudness_shapes.py, run on the device by tests/test_gpu_loudness_shapes.py): the restatement says which of
    them need the step (about one in sixteen does), and the header must agree on every one, bit for bit."""
    x = LS.round_down_wave()
    tp, _ = LR.true_peak(D, x, x.size)
    needs, plain = LS.round_down_split(tp)
    print("true peak", tp, ":", len(needs), "of", len(LS.ROUND_DOWN_CEILINGS), "ceilings need the step:", [float(c) for c in needs])
    assert len(LS.ROUND_DOWN_CEILINGS) >= 64 and len(needs) >= 3 and len(plain) >= 3
    for c in needs:                                                             # exactly one step down, and the promise holds after it
        g = LR.gain(LR.ask(LS.ROUND_DOWN_GAIN, 0.0, c, LR.CEILING), 0.0, tp)
        assert LR.fbits(g) == LR.fbits(F(float(c) / tp)) - 1 and F(float(F(float(c) / tp)) * tp) > c and F(float(g) * tp) <= c
    base = LR.rule(D, x, x.size, out=False)[0]
    for c in needs + plain[:3]:
        q = (LS.ROUND_DOWN_GAIN, 0.0, float(c), LR.CEILING)
        key, y = _native(exes[0], tmp_path, x, x.size, q)
        want = types.SimpleNamespace(**{**vars(base), "gain": LR.gain(LR.ask(*q), base.integrated_ms, tp)})
        assert key == LR.key(want), (c, key, LR.key(want))
        assert (y.view(np.uint32) == (x * want.gain).view(np.uint32)).all(), c
    assert _native(exes[1], tmp_path, x, x.size, (LS.ROUND_DOWN_GAIN, 0.0, float(needs[0]), LR.CEILING))[0][-1] == LR.fbits(F(float(needs[0]) / tp)) - 1


@pytest.mark.parametrize("rate,nf", LS.GATE_CASES)
def test_the_gate_shapes_reach_their_rounds(designs, rate, nf):
    """the spans tests/test_gpu_loudness_shapes.py runs through the gate kernel's second and third rounds: their counts, and (asserted
    inside LS.gate_reach, from the restatement's step energies, blocks and peaks) that the maxima, the blocks the gates drop and the
    true peak lie where the case wants them"""
    Dr = designs[rate]
    want = {(4000, 90): (64, 38, 14), (4000, 91): (65, 39, 14), (4000, 175): (128, 102, 26), (4000, 176): (129, 103, 26),
            (22050, 436): (56, 30, 64), (22050, 437): (56, 30, 65), (22050, 1500): (201, 175, 220)}[(rate, nf)]
    for variant in LS.VARIANTS:
        x = LS.gate_wave(rate, Dr.step, nf, nf + 2, variant)
        r = LS.gate_reach(Dr, x, nf, variant)
        assert (r.blocks, r.short_terms, r.tiles) == want, (variant, vars(r))


# ---- 2. the design ------------------------------------------------------------------------------------------------------------------------------

TABLE_48K = dict(shelf_b=[1.53512485958697, -2.69169618940638, 1.19839281085285], shelf_a=[-1.69065929318241, 0.73248077421585],
                 highpass_b=[1.0, -2.0, 1.0], highpass_a=[-1.99004745483398, 0.99007225036621])


def test_design_reproduces_the_standards_table(exes):
    from zerovox_cpp_amd import capi
    for d in (native_design(exes[0], 48000), LR.design(48000), capi.loudness_design(48000)):
        worst = max(abs(a - b) for k, want in TABLE_48K.items() for a, b in zip(getattr(d, k), want))
        print("48 kHz table: max |difference|", worst)
        assert worst <= 1e-12
        assert d.step == 4800
    assert [LR.design(r).step for r in (22050, 44100, 8000, 11025)] == [2205, 4410, 800, 1103]


RATES = [8000, 16000, 22050, 44100, 48000, 192000]


def _exact_power(A):
    """A^256 in rational arithmetic (eight squarings of Fractions), rounded to float64 once"""
    from fractions import Fraction
    E = [[Fraction(float(v)) for v in row] for row in A]
    for _ in range(8):
        E = [[sum(E[i][k] * E[k][j] for k in range(4)) for j in range(4)] for i in range(4)]
    return np.array([[float(v) for v in row] for row in E])


@pytest.mark.parametrize("rate", RATES)
def test_matrix_is_numpys_matrix_power(exes, rate):
    """M within relative 1e-12 (of the largest entry) of numpy.linalg.matrix_power(A, 256).  The powers of A grow before they decay, so
    A^256 moves by 1e-11 of its largest entry with the ORDER of the squarings' sums (test_matrix_against_the_exact_power: numpy's own
    result lies that far from the exact power).  The rule's order, acc <- fma(P[i][k], P[k][j], acc) ascending in k from +0.0, is the
    one a fused dot-product kernel takes, which is what numpy's BLAS runs for a 4 x 4 product on a machine with fused multiply-adds:
    there the difference is 0.  A BLAS that sums otherwise would show as a difference of about 1e-11 here, not as a wrong M."""
    d, p = native_design(exes[0], rate), LR.design(rate)
    Mp = np.linalg.matrix_power(LR.transition(p.shelf_a, p.highpass_a), 256)
    for M in (np.array(d.M).reshape(4, 4), np.array(p.M).reshape(4, 4)):
        rel = np.abs(M - Mp).max() / np.abs(Mp).max()
        print(rate, "M: max |difference to numpy| / max |M|", rel)
        assert rel <= 1e-12


@pytest.mark.parametrize("rate", RATES)
def test_matrix_against_the_exact_power(exes, rate):
    """M against A^256 in rational arithmetic.  The bound: a squaring rounds every entry by at most 4 u sum |p| |q| (four fused steps,
    u = 2^-53), that is 16 u g^2 for powers whose entries reach g, and the seven squarings behind it can each double the relative
    error: 128 * 16 u g^2 / max|M| stays below 1e-9 for g <= 240, the growth at the highest rate, so 1e-9 of the largest entry is asked."""
    d, p = native_design(exes[0], rate), LR.design(rate)
    A = LR.transition(p.shelf_a, p.highpass_a)
    Ex = _exact_power(A)
    for M in (np.array(d.M).reshape(4, 4), np.array(p.M).reshape(4, 4)):
        rel = np.abs(M - Ex).max() / np.abs(Ex).max()
        print(rate, "M: max |difference to the exact power| / max |M|", rel)
        assert rel <= 1e-9
    assert (np.array(d.M).reshape(4, 4)[:2, 2:] == 0).all()                                 # the shelf's state never sees the high-pass's
    assert [LR.dbits(v) for v in d.M] == [LR.dbits(v) for v in p.M]                           # the header's squarings are the restatement's


@pytest.mark.parametrize("rate", RATES)
def test_interpolator(exes, rate):
    d, p = native_design(exes[0], rate), LR.design(rate)
    for c in (d.c, p.c):
        assert c.dtype == F and c.shape == (49,) and c[24] == 1 and (c[0:49:4][np.arange(13) != 6] == 0).all() and (c == c[::-1]).all()
        assert abs(float(c[1::4].sum()) - 1.0) < 0.01 and abs(float(c[2::4].sum()) - 1.0) < 0.01
    assert (d.c.view(np.uint32) == p.c.view(np.uint32)).all()


def test_design_refuses_rates_outside_its_range(exes):
    from zerovox_cpp_amd import capi
    for rate in (0, 3999, 768001):
        assert native_design(exes[0], rate) == "sampling_rate"
        with pytest.raises(capi.ZvError, match=r"zv_loudness_design: sampling_rate = %d must be in 4000 \.\. 768000" % rate):
            capi.loudness_design(rate)
    assert native_design(exes[0], 4000).step == 400 and capi.loudness_design(768000).step == 76800


# ---- 3. the decomposition is the standard ----------------------------------------------------------------------------------------------------------

def tone(level_db, seconds, freq=1000.0, rate=SR, fade=0.05, phase=0.0):
    """a sine of the peak level, with raised-cosine ends of `fade` seconds"""
    n = int(round(seconds * rate))
    x = 10.0 ** (level_db / 20.0) * np.sin(2.0 * np.pi * freq * np.arange(n) / rate + phase)
    k = int(round(fade * rate))
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(k) + 0.5) / k)
    x[:k] *= ramp
    x[n - k:] *= ramp[::-1]
    return x


def sequence(parts):
    return np.concatenate([tone(db, s) for db, s in parts]).astype(F)


EBU = {
    "case 1": [(-23.0, 20.0)],
    "case 3": [(-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0)],
    "case 4": [(-72.0, 10.0), (-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0), (-72.0, 10.0)],
    "case 5": [(-26.0, 20.0), (-20.0, 20.1), (-26.0, 20.0)],
}


@pytest.fixture(scope="module")
def ebu(D):
    return {name: LR.rule(D, sequence(parts), sum(int(round(s * SR)) for _, s in parts), out=False)[0] for name, parts in EBU.items()}


@pytest.mark.parametrize("name,x", [("noise", noise(40, 9 * SR + 123, 0.05)), ("swell", noise(41, 7 * SR) * np.linspace(0.001, 1, 7 * SR).astype(F)),
                                     ("tones", sequence([(-36.0, 2.0), (-23.0, 5.0), (-50.0, 2.0)]))])
def test_chunked_rule_equals_one_sequential_pass(D, name, x):
    z = LR.gate(LR.step_energies(D, LR.samples(x, x.size)), D.step)[0]
    want = LR.plain(D, x, x.size)
    rel = abs(z - want) / want
    print(name, "integrated mean square: chunked", z, "sequential", want, "relative difference", rel)
    assert want > 0 and rel <= 1e-9


def test_ebu_3341_sequences_read_minus_26(ebu):
    for name, res in ebu.items():
        print(name, res.integrated_lufs, res.blocks, res.blocks_absolute, res.blocks_gated)
    for name, res in ebu.items():
        assert abs(float(res.integrated_lufs) + 26.0) <= 0.1, (name, res.integrated_lufs)
    assert ebu["case 4"].blocks_absolute < ebu["case 4"].blocks and ebu["case 3"].blocks_gated < ebu["case 3"].blocks_absolute


@pytest.mark.parametrize("name,freq,phase", [("fs/4 45", SR / 4, 45.0), ("fs/4 0", SR / 4, 0.0), ("fs/6 60", SR / 6, 60.0), ("fs/8 67.5", SR / 8, 67.5)])
def test_true_peak_tones_read_minus_6(D, name, freq, phase):
    x = tone(20.0 * math.log10(0.5), 1.0, freq, phase=math.radians(phase)).astype(F)
    tp, sp = LR.true_peak(D, x, x.size)
    db = float(LR.dbtp(tp))
    print(name, "dBTP", db, "sample peak dBFS", 20.0 * math.log10(float(sp)))
    assert -6.0 - 0.4 <= db <= -6.0 + 0.2
    if name == "fs/4 45":
        assert abs(20.0 * math.log10(float(sp)) + 9.03) <= 0.01


# ---- 4. the boundary ----------------------------------------------------------------------------------------------------------------------------------

def test_check_names_the_field(exes):
    fb = lambda v: "%x" % LR.fbits(v)
    run = lambda *q: subprocess.run([exes[0], "check", fb(q[0]), fb(q[1]), fb(q[2]), str(q[3])], capture_output=True, text=True, timeout=60).stdout.strip()
    assert run(1.0, 0.0, 0.0, 0) == "ok" and run(0.0, -70.0, 1.0, 3) == "ok" and run(1000.0, 0.0, 1e-30, 3) == "ok"
    assert run(1.0, -99.0, 7.0, 0) == "ok"                                     # fields whose bit is off are finite, no more is asked
    for q, field in (((np.nan, 0, 0, 0), "gain"), ((-0.5, 0, 0, 0), "gain"), ((1000.5, 0, 0, 0), "gain"), ((1, np.inf, 0, 0), "target_lufs"),
                     ((1, 0, np.nan, 0), "true_peak_ceiling"), ((1, -70.5, 0, 1), "target_lufs"), ((1, 0.5, 0, 1), "target_lufs"),
                     ((1, 0, 0.0, 2), "true_peak_ceiling"), ((1, 0, 1.5, 2), "true_peak_ceiling"), ((1, 0, 0, 4), "flags")):
        assert run(*q) == field, (q, field)


def test_arguments_are_refused_by_name_without_a_device():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    x, res = np.zeros(3 * HOP, F), capi.LoudnessResultC()
    handle = C.c_void_p(x.ctypes.data)                        # never dereferenced: the argument checks come first
    q = capi.LoudnessC(1.0, 0.0, 0.0, 0)
    ok = [handle, x.ctypes.data, 0, 3, C.byref(q), C.byref(res), None]      # T = 0: refused last, before the model is looked at
    assert lib.zv_loudness_wave(*ok) == 5 and b"zv_loudness_wave: T must be > 0" in lib.zv_last_error(), lib.zv_last_error()
    for i, what in ((0, b"m is NULL"), (1, b"wav is NULL"), (5, b"res is NULL")):
        args = list(ok)
        args[i] = None
        assert lib.zv_loudness_wave(*args) == 5 and b"zv_loudness_wave: " + what in lib.zv_last_error(), lib.zv_last_error()
    bad = ((capi.LoudnessC(float("nan"), 0, 0, 0), b"loudness gain = nan is not finite"),
           (capi.LoudnessC(-1.0, 0, 0, 0), b"loudness gain = -1 is outside [0, 1000]"),
           (capi.LoudnessC(1001.0, 0, 0, 0), b"loudness gain = 1001 is outside [0, 1000]"),
           (capi.LoudnessC(1.0, float("inf"), 0, 0), b"loudness target_lufs = inf is not finite"),
           (capi.LoudnessC(1.0, -71.0, 0, 1), b"loudness target_lufs = -71 is outside [-70, 0]"),
           (capi.LoudnessC(1.0, 1.0, 0, 1), b"loudness target_lufs = 1 is outside [-70, 0]"),
           (capi.LoudnessC(1.0, 0, float("-inf"), 0), b"loudness true_peak_ceiling = -inf is not finite"),
           (capi.LoudnessC(1.0, 0, 0.0, 2), b"loudness true_peak_ceiling = 0 is outside (0, 1]"),
           (capi.LoudnessC(1.0, 0, 2.0, 2), b"loudness true_peak_ceiling = 2 is outside (0, 1]"),
           (capi.LoudnessC(1.0, 0, 0, 8), b"loudness flags = 8 holds bits other than 0 (target) and 1 (ceiling)"))
    for q2, what in bad:
        args = list(ok)
        args[4] = C.byref(q2)
        assert lib.zv_loudness_wave(*args) == 5 and b"zv_loudness_wave: " + what in lib.zv_last_error(), lib.zv_last_error()
    P, U = C.c_void_p * 2, C.c_uint32 * 2
    results = (capi.LoudnessResultC * 2)()
    okb = [handle, 2, P(x.ctypes.data, x.ctypes.data), U(3, 3), None, None, results, None]
    for i, v, what in ((0, None, b"m is NULL"), (6, None, b"res is NULL")):
        args = list(okb)
        args[i] = v
        assert lib.zv_loudness_wave_batch(*args) == 5 and b"zv_loudness_wave_batch: " + what in lib.zv_last_error(), lib.zv_last_error()
    for q2, what in bad:
        args = list(okb)
        args[5] = (capi.LoudnessC * 2)(capi.LoudnessC(1.0, 0, 0, 0), q2)
        assert lib.zv_loudness_wave_batch(*args) == 5 and b"zv_loudness_wave_batch: utterance 1: " + what in lib.zv_last_error(), lib.zv_last_error()
    assert lib.zv_loudness_design(48000, None) == 5 and b"zv_loudness_design: out is NULL" in lib.zv_last_error()


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
    assert _declaration(header, "zv_loudness_design") == ["uint32_t", "zv_loudness_filter*"]
    assert _declaration(header, "zv_loudness_wave") == ["zv_model*", "const float*", "uint32_t", "uint32_t", "const zv_loudness*", "zv_loudness_result*",
                                                       "float*"]
    assert _declaration(header, "zv_loudness_wave_batch") == ["zv_model*", "uint32_t", "const float*const*", "const uint32_t*", "const uint32_t*",
                                                             "const zv_loudness*", "zv_loudness_result*", "float*const*"]
    vp, u32, pvp, pu32 = C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)
    assert lib.zv_loudness_wave.argtypes == [vp, vp, u32, u32, C.POINTER(capi.LoudnessC), C.POINTER(capi.LoudnessResultC), vp]
    assert lib.zv_loudness_wave_batch.argtypes == [vp, u32, pvp, pu32, pu32, C.POINTER(capi.LoudnessC), C.POINTER(capi.LoudnessResultC), pvp]
    assert lib.zv_loudness_design.argtypes == [u32, C.POINTER(capi.LoudnessFilterC)]
    assert C.sizeof(capi.LoudnessC) == 16 and capi.LoudnessC.flags.offset == 12
    assert C.sizeof(capi.LoudnessResultC) == 72 and capi.LoudnessResultC.blocks.offset == 32 and capi.LoudnessResultC.gain.offset == 64
    assert C.sizeof(capi.LoudnessFilterC) == 408 and capi.LoudnessFilterC.M.offset == 80 and capi.LoudnessFilterC.interp.offset == 208
    assert re.search(r"typedef struct\s*\{\s*float\s+gain;\s*float\s+target_lufs;\s*float\s+true_peak_ceiling;\s*uint32_t\s+flags;\s*\}\s*zv_loudness;", header)
    # no new synthesize form, no new waveform stage
    assert not [s for s in capi.SYMBOLS if "loud" in s and (s.startswith("zv_synthesize") or s.startswith("zv_encode_taps"))]
    assert not any("loud" in f.suffix for f in capi.FORMS)
    # the kernels take every step of the rule from loudness.h, without atomics or anything to zero
    kernels = re.sub(r"//.*", "", open(os.path.join(CSRC, "loudness_kernels.hip")).read())
    for fn in ("loud_kweight", "loud_advance", "loud_run_add", "loud_edge", "loud_step_energy", "loud_momentary", "loud_short_term", "loud_gate_rel",
               "loud_tp_step", "loud_finish", "loud_plan"):
        assert fn + "(" in kernels, fn
    assert not re.search(r"\b(sqrt|log|log10|atomic\w+|hipMemset\w*|fma|__fma_rn)\s*\(", kernels)
    assert '#include "loudness_kernels.hip"' in open(os.path.join(CSRC, "misc_kernels.hip")).read()
    q = capi.Loudness.from_lufs(-16.0, true_peak_dbtp=-1.0).struct
    assert (q.gain, q.target_lufs, q.flags) == (1.0, -16.0, 3) and q.true_peak_ceiling == F(10.0 ** (-1.0 / 20.0))
    assert bytes(capi.Loudness().struct) == struct.pack("<fffI", 1.0, 0.0, 0.0, 0) and capi.Loudness(2.0, 0.0, None).struct.flags == 1
    for call in ("loudness_wave", "loudness_wave_batch"):
        assert callable(getattr(capi.Model, call))


def _stub_lib(symbols):
    lib = types.SimpleNamespace(calls=[])
    for name in symbols:
        setattr(lib, name, lambda *a, _n=name: lib.calls.append((_n, a)) or 0)
    return lib


def test_an_older_library_binds_and_fails_only_these_calls():
    from zerovox_cpp_amd import capi
    lib = _stub_lib([s for s in capi.SYMBOLS if s not in NAMES])
    capi._bind(lib)                                                  # binds what it has
    assert lib.zv_mel_wave.argtypes and lib.zv_vocode.argtypes
    model = types.SimpleNamespace(lib=lib, h="handle", hp=types.SimpleNamespace(audio_hop_size=HOP), _chk=lambda st: None)
    x = np.zeros(2 * HOP, F)
    for name, call in (("zv_loudness_wave", lambda: capi.Model.loudness_wave(model, x)),
                       ("zv_loudness_wave_batch", lambda: capi.Model.loudness_wave_batch(model, [x])),
                       ("zv_loudness_design", lambda: capi.loudness_design(SR, lib=lib))):
        with pytest.raises(AttributeError, match=name + r"\b"):
            call()
    assert not lib.calls
    # a library that has them receives the arrays in the header's order
    lib = _stub_lib(capi.SYMBOLS)
    capi._bind(lib)
    model.lib = lib
    capi.Model.loudness_wave(model, x, capi.Loudness(1.0, -16.0, None), n_frames=1)
    capi.Model.loudness_wave_batch(model, [x, x], None, [2, 1], apply=[True, False])
    (n1, a1), (n2, a2) = lib.calls
    assert n1 == "zv_loudness_wave" and a1[0] == "handle" and a1[2:4] == (2, 1) and a1[6] is not None
    assert n2 == "zv_loudness_wave_batch" and a2[1] == 2 and list(a2[3]) == [2, 2] and list(a2[4]) == [2, 1] and a2[5] is None
    assert [bool(p) for p in a2[7]] == [True, False]
    with pytest.raises(TypeError, match="ask must be a Loudness or None"):
        capi.Model.loudness_wave(model, x, (1.0, 0.0))
    with pytest.raises(ValueError, match="3 asks for 2 utterances"):
        capi.Model.loudness_wave_batch(model, [x, x], [None] * 3)


def test_plan_is_one_launch_per_kernel_and_groups_end_at_2_26_samples(exes):
    Ts = (1, 30, 1024, 32768)
    r = subprocess.run([exes[0], "plan", str(SR), str(HOP)] + [str(t) for t in Ts], capture_output=True, text=True, timeout=60)
    rows = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    for T, (ok, chunks, chunk_gx, tp_gx, steps, apply_gx, states_gx, gy) in zip(Ts, rows):
        n = T * HOP
        assert ok == 1 and chunks == -(-n // 256) and chunk_gx == -(-chunks // 64) and tp_gx == -(-(n + 11) // 2048) and steps == n // STEP
        assert apply_gx == -(-n // 4096) and states_gx == 1 and gy == 3
    src = open(os.path.join(CSRC, "loudness.h")).read()
    assert re.search(r"LOUD_GROUP_SAMPLES\s*=\s*1ull\s*<<\s*26", src) and "sum + p > LOUD_GROUP_SAMPLES" in src


GROUP_BATCH = (300, [32768] * 7 + [50, 50, 1])         # (hop, T): the batch tests/test_gpu_loudness_shapes.py sends across a group's end


def test_launch_groups_end_at_2_26_padded_samples(exes):
    """loud_group_end itself, walked as loud_run walks it, against the rule restated (LS.group_ends) and against the ends worked out
    by hand: capacities are rounded up to whole chunks first, a sum of exactly 2^26 samples stays one group, one chunk more splits, an
    utterance that alone exceeds the limit is a group of its own, and no group is empty."""
    def ends(hop, Ts):
        r = subprocess.run([exes[0], "groups", str(hop)] + [str(t) for t in Ts], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stderr)
        got = [int(v) for v in r.stdout.split()]
        assert got == LS.group_ends(Ts, hop), (hop, Ts, got)
        assert got[-1] == len(Ts) and all(b > a for a, b in zip([0] + got, got))       # every group holds an utterance; all are covered
        return got
    assert ends(256, [1 << 18]) == [1]                                         # exactly 2^26 samples
    assert ends(256, [1 << 17, 1 << 17]) == [2]                                # a sum that lands on 2^26 stays in one group
    assert ends(256, [1 << 17, (1 << 17) + 1]) == [1, 2]                       # one more chunk splits
    assert ends(256, [1 << 17, 1 << 17, 1]) == [2, 3]
    assert ends(255, [1 << 17, 1 << 17, 1]) == [3]                             # 2^26 - 2^18 samples and a chunk
    assert ends(257, [1 << 17, 1 << 17]) == [1, 2]
    assert ends(1, [(1 << 26) - 255, 1]) == [1, 2]                             # the padding counts: 2^26 - 255 samples are 2^26 padded
    assert ends(1, [(1 << 26) - 256, 1]) == [2] and ends(1, [(1 << 26) - 256, 257]) == [1, 2]
    assert ends(300, [(1 << 18) + 5] * 3 + [1]) == [1, 2, 3, 4]                # each alone exceeds the limit: a group of its own
    assert ends(300, [60000, 100000, 100000, 1]) == [2, 4]
    hop, Ts = GROUP_BATCH
    assert ends(hop, Ts) == [6, 10] and 6 * 32768 * 300 <= 1 << 26 < 7 * 32768 * 300
    assert ends(300, [1] * 200) == [200]


def test_cli_knows_its_flags_and_refuses_bad_values(tmp_path):
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    run = lambda *a: subprocess.run([cli, *a], capture_output=True, text=True, timeout=60)
    r = run("--help")
    assert r.returncode == 0 and all(w in r.stdout for w in ("--loudness IN.wav", "--lufs L", "--true-peak-dbtp P", "BS.1770"))
    for args, word in ((("--lufs", "1"), "--lufs 1 is outside [-70, 0]"), (("--lufs", "-71"), "--lufs -71 is outside [-70, 0]"),
                       (("--true-peak-dbtp", "0.5"), "--true-peak-dbtp 0.5 is outside [-200, 0]"), (("--lufs",), "--lufs needs a value"),
                       (("--loudness",), "--loudness needs a value"), (("--loudness", "a.wav", "--plan"), "exclude each other"),
                       (("--loudness", "a.wav", "--analyze", "b.wav", "--mel-out", "c"), "exclude each other")):
        r = run(*args)
        assert r.returncode == 2 and word in r.stderr, (args, r.stderr[:200])
    # the file is read ahead of the checkpoint: a missing or foreign file is an error by the flag's name
    r = run("-m", str(tmp_path / "missing.gguf"), "--loudness", str(tmp_path / "missing.wav"))
    assert r.returncode == 1 and "--loudness: cannot open" in r.stderr and r.stdout == ""
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"not a wave file at all")
    r = run("-m", str(tmp_path / "missing.gguf"), "--loudness", str(bad))
    assert r.returncode == 1 and "--loudness: '" in r.stderr and "is not a RIFF/WAVE file" in r.stderr
