"""Resampling (include/zerovox_amd.h "resampling") without a device.
 * tests/native/resample_check.cpp `self` holds csrc/resample.h's resample_reference against a restatement with every loop written out,
   on random and adversarial inputs, and the same program runs once more built with -fsanitize=address,undefined (a plain host program,
   nothing preloaded);
 * the numpy restatement (tests/resample_rule.py) against that reference, bit for bit: f32, int16 without and with dither and the
   report, on every shape of tests/resample_shapes.py, on the designed tables' signals and on the ragged batch's utterances;
 * the shapes' own reach assertions;
 * the design three ways: every entry within 2^-23 of the rule file's float64 evaluation and at most 1 in magnitude; every phase row's
   sum within P 2^-24 of 1; for six rate pairs the stop band, the pass band and the level at 0.91 of the narrower Nyquist frequency,
   with the measured values printed (profiles/resample_accuracy.txt);
 * a 1 kHz sine from 22 050 to 48 000 Hz against the analytic sine;
 * the argument checkers, the plan and the group cut."""
import os
import subprocess

import numpy as np
import pytest

import resample_rule as RR
import resample_shapes as RH

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
PAIRS = ((22050, 48000), (22050, 8000), (22050, 16000), (48000, 22050), (44100, 22050), (22050, 44100))


def fb(v):
    return "%x" % RR.fbits(v)


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "resample_check.cpp"), "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("resample_check")
    return _build(tmp, "resample_check", []), _build(tmp, "resample_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args[:6], r.returncode, r.stderr[-2000:])
    return r.stdout.split()


_TABLES = {}


def native_design(exe, tmp, rate_in, rate_out, zeros=0, beta=0.0, cutoff=0.0):
    k = (rate_in, rate_out, zeros, beta, cutoff)
    if k not in _TABLES:
        path = str(tmp / "design.f32")
        L, M, P = map(int, run(exe, "design", rate_in, rate_out, zeros, fb(beta), fb(cutoff), path))
        _TABLES[k] = (L, M, np.fromfile(path, F).reshape(L, P))
    return _TABLES[k]


@pytest.fixture(scope="module")
def designs(exes, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("resample_designs")
    return {pair: native_design(exes[0], tmp, *pair) for pair in PAIRS}


def native(exe, tmp, h, M, x, flags=0, seed=0):
    L, P = h.shape
    t, src, dst, pcm = (str(tmp / n) for n in ("table.f32", "in.f32", "out.f32", "out.i16"))
    np.asarray(h, F).tofile(t)
    np.asarray(x, F).tofile(src)
    o = run(exe, "run", L, M, P, flags, seed, t, x.size, src, dst, pcm)
    return (int(o[0]), int(o[1]), int(o[2], 16)), np.fromfile(dst, F), np.fromfile(pcm, np.int16)


def _same_as_native(exe, tmp, what, h, M, x, seeds=(0,)):
    for dithered in (False, True):
        for seed in (seeds if dithered else (0,)):
            res, y, q, _ = RR.rule(h, M, x, dithered, seed)
            key, ny, nq = native(exe, tmp, h, M, x, int(dithered), seed)
            assert RR.key(res) == key, (what, dithered, seed, res, key)
            assert y.size == ny.size and (y.view(np.uint32) == ny.view(np.uint32)).all(), (what, dithered, seed)
            assert (q == nq).all(), (what, dithered, seed, np.flatnonzero(q != nq)[:6])


def test_reference_against_written_out_loops(exes):
    for exe in exes:                                                            # the second one under the sanitizers
        r = subprocess.run([exe, "self"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) >= 200, (r.stdout[-2000:], r.stderr[-2000:])


def test_shapes_reach_their_branches():
    RH.check_targets()
    for L, M, P in RH.TABLES:
        if M > L:
            RH.last_base_lengths(L, M)
    names = [c.name for c in RH.cases()]
    assert len(set(names)) == len(names)
    for _, L, M, h, x in RH.special_cases():
        assert RR.count(x.size, L, M) > RH.tile(L, M, h.shape[1]) and not np.isfinite(x[[0, -1]]).all()
    assert RH.square().max() == 1.0


@pytest.mark.parametrize("shape", RH.TABLES, ids=lambda s: "%d_%d_%d" % s)
def test_restatement_equals_the_reference_on_every_shape(exes, tmp_path, shape):
    mine = [c for c in RH.cases() if (c.L, c.M, c.table.shape[1]) == shape]
    assert mine
    for i, c in enumerate(mine):
        _same_as_native(exes[0], tmp_path, c.name, c.table, c.M, c.x, RH.SEEDS if i % 4 == 0 else (1,))


def test_sanitized_reference_runs_a_shape(exes, tmp_path):
    c = [c for c in RH.cases() if c.name.startswith("special 160/441/24")][0]
    for flags in (0, 1):
        a = native(exes[0], tmp_path, c.table, c.M, c.x, flags, 5)
        b = native(exes[1], tmp_path, c.table, c.M, c.x, flags, 5)
        assert a[0] == b[0] and (a[1].view(np.uint32) == b[1].view(np.uint32)).all() and (a[2] == b[2]).all()


def test_designed_tables_signals_and_ragged_batch(exes, designs, tmp_path):
    x = RH.speech(70, 3000)
    for pair in RH.DESIGNED:
        L, M, h = designs[pair]
        _same_as_native(exes[0], tmp_path, pair, h, M, x, (3,))
    L, M, h = designs[(22050, 48000)]
    res, y, q, _ = RR.rule(h, M, RH.square(), False, 0)
    assert res.clipped > 0 and res.sample_peak > F(1)                           # the overshoot of a full-scale square wave clips
    _same_as_native(exes[0], tmp_path, "square", h, M, RH.square(), (0,))
    L, M, h = designs[(22050, 8000)]
    for u, xu in enumerate(RH.ragged_batch()):
        _same_as_native(exes[0], tmp_path, ("ragged", u), h, M, xu, (9 + u,))


def test_dither_is_tpdf():
    d = RR.dither(12345, np.arange(1 << 18))
    assert d.min() >= -65535.0 / 65536.0 and d.max() <= 65535.0 / 65536.0 and abs(d.mean()) < 0.005 and abs(d.var() - 1.0 / 6.0) < 0.005
    assert (RR.dither(1, np.arange(100)) != RR.dither(2, np.arange(100))).any()
    assert (RR.dither(7, np.array([1 << 32, (1 << 32) + 5])) == RR.dither(7, np.array([0, 5]))).all()      # n enters mod 2^32


# ---- the design ---------------------------------------------------------------------------------------------------------------------------

def test_design_sizes_and_refusals(exes):
    d = lambda *a: run(exes[0], "design", a[0], a[1], a[2], fb(a[3]), fb(a[4]))
    assert d(22050, 48000, 0, 0.0, 0.0) == ["320", "147", "64"] and d(22050, 8000, 0, 0.0, 0.0) == ["160", "441", "178"]
    assert d(22050, 22050, 0, 0.0, 0.0) == ["1", "1", "64"] and d(44100, 22050, 4, 5.0, 1.0) == ["1", "2", "16"]
    for pair in PAIRS + ((8000, 48000), (48000, 8000), (4000, 32000), (768000, 96000), (22050, 16000)):
        for zeros in (0, 4, 33, 64):
            L, M, P = RR.sizes(pair[0], pair[1], zeros)
            if P <= 512 and L * P <= 65536:
                assert d(pair[0], pair[1], zeros, 0.0, 0.0) == [str(L), str(M), str(P)], (pair, zeros)
    assert d(3999, 8000, 0, 0.0, 0.0) == ["refused", "rate_in"] and d(768001, 8000, 0, 0.0, 0.0) == ["refused", "rate_in"]
    assert d(8000, 3999, 0, 0.0, 0.0) == ["refused", "rate_out"] and d(8000, 768001, 0, 0.0, 0.0) == ["refused", "rate_out"]
    assert d(22050, 22051, 0, 0.0, 0.0) == ["refused", "L"] and d(5132, 4000, 0, 0.0, 0.0) == ["refused", "M"]
    assert d(4000, 36000, 0, 0.0, 0.0) == ["refused", "ratio"] and d(36000, 4000, 0, 0.0, 0.0) == ["refused", "ratio"]
    assert d(22050, 8000, 3, 0.0, 0.0) == ["refused", "zeros"] and d(22050, 8000, 65, 0.0, 0.0) == ["refused", "zeros"]
    for b in (-1.0, 20.5, np.nan, np.inf):
        assert d(22050, 8000, 0, b, 0.0) == ["refused", "beta"]
    for c in (-0.1, 1.01, np.nan, np.inf):
        assert d(22050, 8000, 0, 0.0, c) == ["refused", "cutoff"]
    assert d(48000, 8000, 64, 0.0, 0.0) == ["refused", "P"]                     # 2 * 64 * 6 = 768 taps
    assert d(22050, 48000, 64, 0.0, 0.0) == ["320", "147", "128"] and d(22050, 44099, 64, 0.0, 0.0)[0] == "refused"
    assert d(24000, 25600, 64, 0.0, 0.0) == ["16", "15", "128"]
    assert d(20000, 25600, 64, 0.0, 0.0) == ["32", "25", "128"] and d(4000, 5120, 64, 0.0, 0.0) == ["32", "25", "128"]
    assert d(6390, 6400, 64, 0.0, 0.0) == ["refused", "table", "size"]          # 640 rows of 128 taps
    assert d(6390, 6400, 0, 0.0, 0.0) == ["640", "639", "64"]


def test_design_entries_rows_and_defaults(exes, designs, tmp_path):
    for pair in PAIRS:
        L, M, h = designs[pair]
        rL, rM, g = RR.design(*pair)
        assert (L, M, h.shape) == (rL, rM, g.shape)
        err = float(np.abs(h.astype(np.float64) - g).max())
        print("design", pair, "entries within %.3e" % err)
        assert err <= 2.0 ** -23 and float(np.abs(h).max()) <= 1.0
        rows = h.astype(np.float64).sum(axis=1)
        assert float(np.abs(rows - 1.0).max()) <= h.shape[1] * 2.0 ** -24, pair
    # other parameters than the defaults, and the defaults spelt out (0.91 is no float32 value: the cutoff stays 0)
    L, M, h = native_design(exes[0], tmp_path, 16000, 44100, 12, 6.5, 0.8)
    assert float(np.abs(h.astype(np.float64) - RR.design(16000, 44100, 12, 6.5, 0.8)[2]).max()) <= 2.0 ** -23
    L, M, h = native_design(exes[0], tmp_path, 22050, 8000, 32, 9.0, 0.0)
    assert (h.view(np.uint32) == designs[(22050, 8000)][2].view(np.uint32)).all()
    # a constant stays constant (every phase has DC gain 1): away from the ends, within the rows' rounding
    L, M, h = designs[(22050, 48000)]
    y = RR.sums(h, M, np.full(400, 0.25, F))[0]
    assert float(np.abs(y[200:600] - 0.25).max()) <= 64 * 2.0 ** -24


def measured_response(designs):
    """{pair: (stop band max dB, pass band min dB, pass band max dB, level at 0.91 dB)} of the prototype assembled from the f32 rows"""
    out = {}
    for pair in PAIRS:
        L, M, h = designs[pair]
        nfft = 1 << 22
        db, nyq = RR.response_db(h, M, nfft)
        stop = float(db[int(np.ceil(nyq)):].max())
        band = db[:int(np.floor(0.82 * nyq)) + 1]
        b = 0.91 * nyq
        lo = int(np.floor(b))
        at = float(db[lo] + (db[lo + 1] - db[lo]) * (b - lo))
        out[pair] = (stop, float(band.min()), float(band.max()), at)
    return out


def test_design_spectrum_of_six_rate_pairs(designs):
    for pair, (stop, pmin, pmax, at) in measured_response(designs).items():
        print("response %d -> %d: stop band %.2f dB, pass band %+.5f .. %+.5f dB, at 0.91 %.3f dB" % (pair + (stop, pmin, pmax, at)))
        assert stop <= -88.0, (pair, stop)
        assert -0.001 <= pmin and pmax <= 0.001, (pair, pmin, pmax)
        assert abs(at + 6.0) <= 0.1, (pair, at)


def test_sine_against_the_analytic_sine(designs):
    L, M, h = designs[(22050, 48000)]
    t = np.arange(4000)
    x = (0.5 * np.sin(2.0 * np.pi * 1000.0 * t / 22050.0)).astype(F)
    y = RR.sums(h, M, x)[0]
    n = np.arange(y.size)
    want = 0.5 * np.sin(2.0 * np.pi * 1000.0 * n / 48000.0)
    err = float(np.abs(y.astype(np.float64) - want)[401:-401].max())
    print("sine 22050 -> 48000: max error %.3e over %d outputs" % (err, y.size - 802))
    assert y.size == RR.count(4000, L, M) == 8708 and err <= 1e-4


# ---- checkers, plan, groups -----------------------------------------------------------------------------------------------------------------

def test_argument_checker(exes, tmp_path):
    chk = lambda *a: run(exes[0], "check", *a)[0:2]
    for L, M, P in RH.TABLES + ((8, 1, 2), (1, 8, 512), (128, 127, 512), (1280, 1279, 50)):
        assert chk(L, M, P) == ["ok"], (L, M, P)
    assert chk(0, 1, 2) == ["L"] and chk(1281, 1280, 2) == ["L"] and chk(1, 0, 2) == ["M"] and chk(1280, 1281, 2) == ["M"]
    assert chk(9, 1, 2) == ["ratio"] and chk(1, 9, 2) == ["ratio"] and chk(17, 2, 2) == ["ratio"]
    assert chk(1, 1, 0) == ["P"] and chk(1, 1, 3) == ["P"] and chk(1, 1, 514) == ["P"]
    assert chk(129, 128, 512) == ["table", "size"] and chk(1280, 441, 52) == ["table", "size"]
    assert chk(0, 0, 0) == ["L"]                                                # in the order L, M, ratio, P, table size
    path = str(tmp_path / "t.f32")
    h = RH.table(3, 2, 4)
    h.tofile(path)
    assert chk(3, 2, 4, path) == ["ok"]
    np.tile(h, (2, 1)).tofile(path)
    assert chk(6, 4, 4, path) == ["gcd"]
    for bad in (np.nan, np.inf, -np.inf):
        g = h.copy()
        g[2, 3] = bad
        g.tofile(path)
        assert chk(3, 2, 4, path) == ["table"]


def test_plan_and_group_cut(exes):
    plan = lambda *a: tuple(map(int, run(exes[0], "plan", *a)))
    for n in (1, 2559, 2560, 2561, 5120, 5121, 78643200):
        assert plan(n, 5, 320, 147, 64) == (1, -(-n // 2560), 5, 320, 147, 8), n
    # the tile of every table of the shapes, of the designed pairs and of the corners: the restatement is the plan's, the staged span fits
    shapes = RH.TABLES + tuple(RR.sizes(*p) for p in PAIRS) + ((1, 8, 512), (8, 1, 512), (159, 1270, 412), (1280, 1279, 50), (1279, 1280, 50), (513, 512, 126),
                                                              (512, 513, 128), (127, 16, 512), (1, 1, 2), (257, 256, 254))
    for L, M, P in shapes:
        S, D, R = RH.tile_srd(L, M, P)
        assert plan(R * S + 1, 1, L, M, P) == (1, 2, 1, S, D, R), (L, M, P)
        assert S % L == 0 and D * L == S * M and R in (1, 2, 4, 8) and chk_stage(L, M, P) <= RH.STAGE, (L, M, P)
        assert R == 8 or chk_stage(L, M, P, 2 * R) > RH.STAGE, (L, M, P)        # R is the largest that fits
    assert [RH.tile_srd(*RR.sizes(*p)) for p in PAIRS[:2]] == [(320, 147, 8), (480, 1323, 4)]
    ok = lambda *a: plan(*a)[0]
    assert ok(1, 1, 1, 1, 2) and not ok(0, 1, 1, 1, 2) and not ok(1, 0, 1, 1, 2) and not ok(1, 65536, 1, 1, 2) and ok(1, 65535, 1, 1, 2)
    assert not ok(1, 1, 9, 1, 2) and not ok(1, 1, 1, 1, 3) and not ok(1, 1, 1281, 1280, 2) and not ok(1, 1, 129, 128, 512)
    cnt = lambda S, L, M: RR.count(S, L, M)
    assert run(exes[0], "plan", 1, 1, 1, 1, 2)[0] == "1" and cnt(1, 1, 1) == 1 and cnt(1, 7, 1) == 7 and cnt(1, 1, 6) == 1 and cnt(7, 1, 6) == 2 and cnt(3000, 320, 147) == 6531
    big = 32768 * 300
    for L, M, S in ((1, 1, [big] * 4 + [5000, 300, 1]), (1, 8, RH.group_batch(big)[0]), (1, 1, [1, 2, 3]), (8, 1, [big, big, 7]), (1, 8, [big] * 8), (320, 147, [big] * 5),
                    (3, 2, [100] * 70000)):
        got = list(map(int, run(exes[0], "groups", L, M, *S)))
        assert got == RH.group_ends(S, L, M), (L, M, got[:8])
    assert RH.group_batch(big)[0][:7] == [big] * 7 and RH.group_ends([big] * 4 + [5000, 300, 1], 1, 1) == [3, 7] and RH.group_ends([100] * 70000, 3, 2) == [65535, 70000]


def chk_stage(L, M, P, R=None):
    """the most input samples a tile of outputs reaches: over every first remainder, the bases' reach plus the taps"""
    S, _, R0 = RH.tile_srd(L, M, P)
    return max((r + ((R or R0) * S - 1) * M) // L for r in range(L)) + P
