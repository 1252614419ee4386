"""Pitch track (include/zerovox_amd.h "pitch track") on the CPU: csrc/pitch.h against its restatement in exact integers and single
float64 steps (tests/pitch_rule.py), bit for bit.
 * tests/native/pitch_check.cpp drives zv::pitch_params_resolve and zv::pitch_reference over the named edge classes and random small
   cases: the resolved parameters, every frame's row, Fq and flag and every phoneme's row must agree;
 * the same input through a build with -fsanitize=address,undefined (a plain host program, nothing preloaded);
 * the properties the header states: power-of-two invariance, known periods, noise, the phoneme mean;
 * the boundary: the four entry points are declared, exported and bound, refuse a NULL model by name, zv_pitch_track refuses a phoneme
   table, the binding refuses a bad return_pitch before it touches a device, _call_variant routes a pitch request and nothing else to
   the _pitch symbol, and the CLI knows its flags."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import pitch_rule as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
CLI = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
NAMES = ("zv_synthesize_pitch", "zv_synthesize_batch_pitch", "zv_synthesize_batch_begin_pitch", "zv_pitch_track")
F = np.float32
SR = 22050
SPECIALS = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x7f7fffff], np.uint32).view(F)


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "pitch_check.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pitch_check")
    return _build(tmp, "pitch_check", []), _build(tmp, "pitch_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# ---- cases ------------------------------------------------------------------------------------------------------------------

def _tone(total, P, amp=0.4):
    return (np.sin(2 * np.pi * np.arange(total) / P) * amp).astype(F)


def _case(name, T, hop, x, dur=(), sr=8000, lo=0, hi=0, W=0, thr=0.0):
    x = np.asarray(x, F)
    assert x.shape == (T * hop,), name
    return dict(name=name, T=T, sr=sr, hop=hop, dur=[int(d) for d in dur], x=x, lo=lo, hi=hi, W=W, thr=float(F(thr)))


def _named(rng):
    small = dict(sr=8000, lo=8, hi=40, W=64, thr=0.3)         # spans of 105 samples: short cases stay quick
    noise = lambda n, s=0.3: (rng.standard_normal(n) * s).astype(F)
    c = [_case("T = 1", 1, 40, _tone(40, 13), [1], **small),
         _case("window and lags at their lower bounds", 6, 40, _tone(240, 9), [6], sr=8000, lo=8, hi=9, W=64, thr=0.5),
         _case("window and lags at their upper bounds", 3, 700, _tone(2100, 300) + noise(2100, 0.01), [1, 2], sr=48000, lo=511, hi=512, W=1024, thr=0.5),
         _case("max_lag = 8 * min_lag", 3, 700, _tone(2100, 77), [3], sr=48000, lo=64, hi=512, W=1024, thr=0.5),
         _case("max_lag = 8 * min_lag, short", 8, 40, _tone(320, 21), [8], sr=8000, lo=8, hi=64, W=64, thr=0.5),
         _case("a span wholly outside the speech (fitted zeros)", 12, 40, np.concatenate([_tone(120, 11), np.zeros(360, F)]), [3], **small),
         _case("a span half in zeros", 4, 40, np.concatenate([np.zeros(80, F), _tone(80, 11)]), [2, 2], **small),
         _case("an all-zero waveform", 5, 40, np.zeros(200, F), [2, 3], **small),
         _case("all -0.0", 3, 40, np.full(120, -0.0, F), [3], **small),
         _case("a peak just below 2^-24", 3, 40, _tone(120, 12, 1.0) * F(2.0 ** -25) * F(1.9999), [3], **small),
         _case("a peak just at 2^-24", 3, 40, np.where(np.arange(120) % 12 == 0, F(2.0 ** -24), F(2.0 ** -26)), [3], **small),
         _case("NaN, inf and -0.0 samples", 6, 40, np.where(rng.random(240) < 0.1, rng.choice(SPECIALS[:4], 240), _tone(240, 14)), [6], **small),
         _case("only NaN and inf", 2, 40, rng.choice(SPECIALS[:3], 80), [2], **small),
         _case("samples above 1.0", 4, 40, _tone(160, 15, 7.5), [4], **small),
         _case("samples at 1e30", 4, 40, np.where(np.arange(160) % 15 == 0, F(1e30), _tone(160, 15)), [4], **small),
         _case("a waveform scaled to 1e30", 4, 40, _tone(160, 15) * F(1e30), [4], **small),
         _case("subnormal samples next to large ones", 4, 40, np.where(np.arange(160) % 2 == 0, F(1e-42), _tone(160, 15)), [4], **small),
         _case("a constant (DC) waveform", 6, 40, np.full(240, 0.25, F), [6], **small),
         _case("alternating signs: c(L) < 0 at every odd lag", 4, 40, np.tile(np.array([0.5, -0.5], F), 80), [4], sr=8000, lo=9, hi=10, W=64, thr=0.5),
         _case("rmax == 0: one pulse", 4, 40, (np.arange(160) == 70) * F(0.9), [4], **small),
         _case("a plateau r(L+1) == r(L) (DC: r = 1 at every lag)", 8, 40, np.full(320, -0.75, F), [8], sr=8000, lo=8, hi=64, W=64, thr=1.0),
         _case("L* == Lmax: a ramp of correlation", 5, 40, _tone(200, 21), [5], sr=8000, lo=8, hi=20, W=64, thr=0.1),
         _case("L0 == Lmin: the period is the shortest lag", 5, 40, _tone(200, 8), [5], **small),
         _case("den == 0: three equal correlations (DC)", 3, 40, np.full(120, 0.5, F), [3], sr=8000, lo=10, hi=12, W=64, thr=0.5),
         _case("phonemes of 0 frames between others", 10, 40, _tone(400, 16), [3, 0, 0, 4, 0, 3, 0], **small),
         _case("a phoneme cut off by T", 10, 40, _tone(400, 16), [4, 6, 0, 0], **small),
         _case("a phoneme with no voiced frame", 10, 40, np.concatenate([_tone(200, 16), noise(200, 0.1)]), [5, 5], sr=8000, lo=8, hi=40, W=64, thr=0.95),
         _case("no phonemes", 3, 40, _tone(120, 16), [], **small),
         _case("threshold 1.0", 4, 40, _tone(160, 16), [4], sr=8000, lo=8, hi=40, W=64, thr=1.0),
         _case("the smallest threshold", 4, 40, noise(160), [4], sr=8000, lo=8, hi=40, W=64, thr=1e-45),
         _case("defaults at 22 050 Hz and hop 300", 4, 300, _tone(1200, 100), [1, 3], sr=SR)]
    for hop in (1, 3, 4, 7, 300):
        T = 200 if hop == 1 else 3 if hop == 300 else 40
        c.append(_case(f"hop = {hop}", T, hop, _tone(T * hop, 17) + noise(T * hop, 0.05), [T // 2, 0, T - T // 2], **small))
    return c


REFUSED = [("min_lag below 8", dict(lo=7, hi=40, W=64), "min_lag", 0), ("min_lag == max_lag", dict(lo=20, hi=20, W=64), "max_lag", 0),
           ("max_lag above 512", dict(lo=100, hi=513, W=64), "max_lag", 0), ("max_lag above 8 * min_lag", dict(lo=8, hi=65, W=64), "max_lag", 0),
           ("window below 64", dict(lo=8, hi=40, W=63), "window", 0), ("window above 1024", dict(lo=8, hi=40, W=1025), "window", 0),
           ("threshold above 1", dict(lo=8, hi=40, W=64, thr=1.5), "voiced_threshold", 0),
           ("threshold negative", dict(lo=8, hi=40, W=64, thr=-0.5), "voiced_threshold", 0),
           ("threshold NaN", dict(lo=8, hi=40, W=64, thr=float("nan")), "voiced_threshold", 0),
           ("threshold inf", dict(lo=8, hi=40, W=64, thr=float("inf")), "voiced_threshold", 0),
           ("default min_lag at 3 000 Hz", dict(sr=3000, hi=40, W=64), "min_lag", 1), ("default max_lag at 48 kHz", dict(sr=48000, lo=100, W=64), "max_lag", 1),
           ("default window at hop 16", dict(sr=SR, hop=16), "window", 1), ("default window at hop 600", dict(sr=SR, hop=600), "window", 1)]


def _random(rng, count):
    c = []
    for k in range(count):
        hop = int(rng.choice([1, 3, 4, 7, 30]))
        T = int(rng.integers(1, 120 // hop + 2))
        lo = int(rng.integers(8, 24))
        hi = int(rng.integers(lo + 1, min(8 * lo, 90) + 1))
        W = int(rng.integers(64, 110))
        n = int(rng.integers(0, 6))
        cuts = np.sort(rng.integers(0, T + 1, size=n))
        dur = np.diff(np.concatenate([[0], cuts])).tolist()
        total = T * hop
        kind = k % 5
        if kind == 0:
            x = rng.standard_normal(total) * 10.0 ** int(rng.integers(-9, 3))
        elif kind == 1:
            x = np.sin(2 * np.pi * np.arange(total) / rng.uniform(lo, hi)) * rng.uniform(0.01, 2) + rng.standard_normal(total) * 0.05
        elif kind == 2:
            x = (np.arange(total) % int(rng.integers(lo, hi + 1)) == 0) * rng.uniform(0.1, 1.0)
        elif kind == 3:
            x = np.round(rng.standard_normal(total) * 2) / 4           # few distinct values: ties and plateaus
        else:
            x = rng.standard_normal(total) * 0.2
            x[rng.random(total) < 0.05] = 0
        x = np.asarray(x, F)
        if rng.random() < 0.15 and total:
            at = rng.integers(0, total, size=min(total, 6))
            x[at] = SPECIALS[:len(at)]
        c.append(_case(f"random {k}", T, hop, x, dur, sr=int(rng.choice([8000, 16000, SR])), lo=lo, hi=hi, W=W, thr=float(rng.choice([0.0, 0.2, 0.5, 0.9]))))
    return c


def _stdin(cases):
    lines = []
    for c in cases:
        lines.append(f"{c['T']} {c['sr']} {c['hop']} {len(c['dur'])} {c['lo']} {c['hi']} {c['W']} {PR.bits(F(c['thr']))[()]:x}")
        lines.append(" ".join(map(str, c["dur"])))
        lines.append(" ".join("%x" % b for b in PR.bits(c["x"])))
    return "\n".join(lines) + "\n"


def _rule(c):
    return PR.rule(c["x"], c["T"], c["sr"], c["hop"], c["dur"], c["lo"], c["hi"], c["W"], c["thr"])


def _expect(c):
    lo, hi, W, thr = PR.resolve(c["sr"], c["hop"], c["lo"], c["hi"], c["W"], c["thr"])
    r = _rule(c)
    fb, pb = PR.bits(r["frames"]), PR.bits(r["phonemes"])
    line = f"{lo} {hi} {W} {PR.bits(thr)[()]:x} |"
    line += "".join(f" {fb[f, 0]:x}:{fb[f, 1]:x}:{r['Fq'][f]}:{r['voiced'][f]}" for f in range(c["T"])) + " |"
    return line + "".join(f" {pb[i, 0]:x}:{pb[i, 1]:x}" for i in range(len(c["dur"])))


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(20261020)
    return _named(rng) + _random(rng, 1200)


@pytest.fixture(scope="module")
def refused():
    return [_case(name, 1, kw.get("hop", 40), np.zeros(kw.get("hop", 40), F), [], **{k: v for k, v in kw.items() if k != "hop"}) for name, kw, _, _ in REFUSED]


@pytest.fixture(scope="module")
def outputs(exes, cases, refused):
    text = _stdin(cases + refused)
    return [subprocess.run([e], input=text, capture_output=True, text=True, timeout=600) for e in exes]


# ---- 1. header against restatement --------------------------------------------------------------------------------------------

def test_header_equals_restatement_bit_for_bit(cases, refused, outputs):
    r = outputs[0]
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(cases) + len(refused)
    for c, line in zip(cases, got):
        assert line == _expect(c), c["name"]
    for (name, kw, field, defaulted), c, line in zip(REFUSED, refused, got[len(cases):]):
        assert line == f"refused {field} {defaulted}", name
        with pytest.raises(ValueError, match=field):
            PR.resolve(c["sr"], c["hop"], c["lo"], c["hi"], c["W"], c["thr"])


def test_sanitized_build_agrees_and_is_silent(outputs):
    plain, san = outputs
    assert san.returncode == 0 and san.stderr == "", san.stderr[-3000:]
    assert san.stdout == plain.stdout


def test_the_named_cases_reach_what_they_name(cases):
    by = {c["name"]: c for c in cases}
    rows = lambda name: _rule(by[name])
    zero = lambda a: not PR.bits(a).any()
    assert zero(rows("an all-zero waveform")["frames"]) and zero(rows("all -0.0")["frames"]) and zero(rows("only NaN and inf")["frames"])
    assert zero(rows("a peak just below 2^-24")["frames"]) and rows("a peak just at 2^-24")["frames"][1, 1] > 0
    r = rows("a span wholly outside the speech (fitted zeros)")
    assert r["frames"][0, 1] > 0 and zero(r["frames"][5:]) and r["phonemes"][0, 1] > 0
    assert rows("a span half in zeros")["frames"][2:, 1].all()          # (frame 1: its window lies in the zeros, E0 = 0)
    assert zero(rows("rmax == 0: one pulse")["frames"])
    r = rows("a plateau r(L+1) == r(L) (DC: r = 1 at every lag)")
    assert r["frames"][4].tolist() == [1000.0, 1.0]                      # frame 4's span lies inside: L* = L0 = Lmin = 8, the plateau ends the search at once
    assert rows("den == 0: three equal correlations (DC)")["frames"][1].tolist() == [800.0, 1.0]      # delta = 0: exactly sr / 10
    r = rows("L* == Lmax: a ramp of correlation")
    assert F(8000.0 / 20.5) <= r["frames"][2, 0] <= F(8000.0 / 19.5)
    r = rows("L0 == Lmin: the period is the shortest lag")
    assert abs(8000.0 / r["frames"][2, 0] - 8) <= 0.5
    r = rows("a phoneme with no voiced frame")
    assert r["phonemes"][0].tolist()[1] > 0 and r["phonemes"][1].tolist() == [0.0, 0.0] and not any(r["voiced"][7:])
    r = rows("phonemes of 0 frames between others")
    assert zero(r["phonemes"][[1, 2, 4, 6]]) and r["phonemes"][[0, 3, 5], 1].all()
    assert rows("no phonemes")["phonemes"].shape == (0, 2)
    assert rows("samples at 1e30")["frames"][:, 1].any() and rows("a waveform scaled to 1e30")["frames"][:, 0].all()


# ---- 2. the properties the header states ------------------------------------------------------------------------------------------

def test_power_of_two_scaling_changes_no_row(cases):
    n = 0
    for c in cases[::9]:
        x = c["x"]
        if not np.isfinite(x).all():
            continue
        base = _rule(c)
        for s in (0.25, 64.0, 2.0 ** -12):
            y = x * F(s)
            ay = np.abs(y[y != 0])
            if ay.size and (ay.min() < 2.0 ** -126 or not np.isfinite(y).all()):
                continue                                            # a sample became subnormal or infinite: outside the promise
            r = PR.rule(y, c["T"], c["sr"], c["hop"], c["dur"], c["lo"], c["hi"], c["W"], c["thr"])
            # the promise holds while the span's peak stays at or above 2^-24 on both sides: a frame that is silent on the smaller side
            # alone fell below it; every other frame keeps its bits, and with all frames the phonemes do
            small, large = (r, base) if s < 1 else (base, r)
            fell = [f for f in range(c["T"]) if not PR.bits(small["frames"][f]).any() and PR.bits(large["frames"][f]).any()]
            for f in range(c["T"]):
                assert f in fell or np.array_equal(PR.bits(r["frames"][f]), PR.bits(base["frames"][f])), (c["name"], s, f)
            if not fell:
                assert np.array_equal(PR.bits(r["phonemes"]), PR.bits(base["phonemes"])), (c["name"], s)
            n += not fell
    assert n > 200


@pytest.fixture(scope="module")
def known():
    """frame 3 (its span [575, 1526) lies inside the waveform) of the three signals at every integer period 50 .. 350"""
    T, hop = 8, 300
    t = np.arange(T * hop)
    params = PR.resolve(SR, hop)
    out = {}
    for P in range(50, 351):
        sig = dict(pulses=((t % P) == 0) * 0.7, sine=np.sin(2 * np.pi * t / P) * 0.4,
                   harmonics=sum(np.sin(2 * np.pi * h * t / P) / h for h in range(1, 9)) * 0.1)
        for name, x in sig.items():
            out[name, P] = PR.frame(x.astype(F), T * hop, 3, SR, hop, params)[0]
    return out


def test_known_periods(known):
    assert PR.resolve(SR, 300)[:3] == (50, 350, 600)
    for (name, P), (f0, strength) in known.items():
        assert abs(SR / float(f0) - P) <= 0.5 and strength >= 0.9, (name, P, f0, strength)


def test_white_noise_is_unvoiced():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(16 * 300) * 0.1).astype(F)
    r = PR.rule(x, 16, SR, 300)
    assert not r["frames"][:, 0].any() and 0.0 < r["frames"][2:-2, 1].max() < 0.5


def test_a_phonemes_mean_lies_between_its_voiced_frames(cases):
    n = 0
    for c in cases:
        if not c["dur"]:
            continue
        r = _rule(c)
        start = 0
        for i, d in enumerate(c["dur"]):
            f0 = [float(r["frames"][f, 0]) for f in range(start, start + d) if r["voiced"][f]]
            if f0:
                ulp = 2.0 ** -9                                       # Fq rounds f0 to 1/256 Hz: half a step on each side
                assert min(f0) - ulp <= float(r["phonemes"][i, 0]) <= max(f0) + ulp, (c["name"], i)
                assert r["phonemes"][i, 1] == F(len(f0) / d)
                n += 1
            else:
                assert r["phonemes"][i, 0] == 0 and r["phonemes"][i, 1] == 0
            start += d
    assert n > 300


# ---- 3. the boundary --------------------------------------------------------------------------------------------------------------

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
        assert _declaration(header, name + "_pitch") == _declaration(header, name + "_contour") + ["const zv_pitch*"], name
        assert getattr(lib, name + "_pitch").argtypes == getattr(lib, name + "_contour").argtypes + [C.POINTER(capi.PitchC)]
    assert _declaration(header, "zv_pitch_track") == ["zv_model*", "const float*", "uint32_t", "const zv_pitch*"]
    assert not re.search(r"\bzv_synthesize_batch_end_pitch\b", header)             # the existing _end finishes a pitch batch
    assert C.sizeof(capi.PitchC) == 32 and bytes(capi.PitchC()) == bytes(32)        # zero-initialised = none
    assert re.search(r"typedef struct\s*\{\s*float f0_hz, strength;\s*\}\s*zv_pitch_frame;", header)
    assert re.search(r"typedef struct\s*\{\s*float f0_hz, voiced;\s*\}\s*zv_pitch_phoneme;", header)
    assert re.search(r"typedef struct\s*\{\s*zv_pitch_frame\s*\*frames;\s*zv_pitch_phoneme \*phonemes;\s*uint32_t min_lag, max_lag, window;\s*"
                     r"float\s+voiced_threshold;\s*\}\s*zv_pitch;", header)
    # the kernels take every non-integer step from pitch.h
    kernels = re.sub(r"//.*", "", open(os.path.join(CSRC, "pitch_kernels.hip")).read())
    for fn in ("pitch_span", "pitch_scale", "pitch_quant", "pitch_corr", "pitch_refine", "pitch_frame_row", "pitch_phoneme_row", "contour_extent"):
        assert fn + "(" in kernels, fn
    assert "sqrt" not in kernels and "atomic" not in kernels.lower().replace("__atomic_release", "").replace("__atomic_acquire", "")


def test_null_model_is_refused_by_every_entry_point():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    n = C.c_uint32(0)
    pit = capi.PitchC()
    assert lib.zv_synthesize_pitch(None, None, None, None, 4, 8, None, C.byref(n), None, None, None, 0, 0, None, None, None, None, C.byref(pit)) == 5
    assert b"zv_synthesize_pitch" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_pitch(None, 1, None, None, None, None, None, None, None, None, None, None, None, 0, None, None, None, None, pit) == 5
    assert b"zv_synthesize_batch_pitch" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_begin_pitch(None, 0, 1, None, None, None, None, None, None, None, None, None, None, None, 0, None, None,
                                               None, None, pit) == 5
    assert b"zv_synthesize_batch_begin_pitch" in lib.zv_last_error()
    assert lib.zv_pitch_track(None, None, 8, C.byref(pit)) == 5
    assert b"zv_pitch_track" in lib.zv_last_error()


def test_pitch_track_refuses_a_phoneme_table_and_a_missing_frame_table():
    """both are refused ahead of everything that needs the model: a handle that is not null but never dereferenced shows it"""
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    rows, wav = np.zeros((8, 2), F), np.zeros(8 * 300, F)
    handle = C.c_void_p(wav.ctypes.data)                      # never dereferenced: the argument checks come first
    pit = capi.PitchC(rows.ctypes.data, rows.ctypes.data)
    assert lib.zv_pitch_track(handle, wav.ctypes.data, 8, C.byref(pit)) == 5
    assert b"zv_pitch_track" in lib.zv_last_error() and b"phonemes must be NULL" in lib.zv_last_error()
    pit = capi.PitchC(None, None)
    assert lib.zv_pitch_track(handle, wav.ctypes.data, 8, C.byref(pit)) == 5
    assert b"zv_pitch_track" in lib.zv_last_error() and b"frames is required" in lib.zv_last_error()


class _NoDevice:
    """stands where a capi.Model would: any touch of the library or the handle fails the test"""
    hp = types.SimpleNamespace(audio_hop_size=300)

    def __getattr__(self, name):
        raise AssertionError(f"the binding touched .{name} before it had checked its arguments")


def test_binding_refuses_a_bad_return_pitch_before_touching_a_device():
    from zerovox_cpp_amd import capi
    ids, puncts, style = np.ones(4, np.int32), np.zeros(4, np.int32), np.zeros(528, np.float32)
    fake = _NoDevice()
    two = [(ids, puncts, style, 64), (ids, puncts, style, 7)]
    for bad in ("frame", "both", ""):
        with pytest.raises(ValueError, match="return_pitch = %r: expected False, True, 'frames', 'phonemes' or a PitchTrack" % bad):
            capi.Model.synthesize(fake, ids, puncts, style, 64, return_pitch=bad)
        with pytest.raises(ValueError, match="utterance 1: return_pitch = %r" % bad):
            capi.BatchCall(fake, two, return_pitch=[True, bad])
    for bad in (1, None, 2.0, b"frames", {}):
        with pytest.raises(TypeError, match="return_pitch must be a bool, 'frames', 'phonemes' or a PitchTrack"):
            capi.Model.synthesize(fake, ids, puncts, style, 64, return_pitch=bad)
        with pytest.raises(TypeError, match="return_pitch must be a bool, 'frames', 'phonemes' or a PitchTrack"):
            capi.BatchCall(fake, two, return_pitch=bad)
    with pytest.raises(ValueError, match="return_pitch has 1 entries, the batch has 2"):
        capi.BatchCall(fake, two, return_pitch=["frames"])
    for kw in (dict(min_lag=-1), dict(window=1 << 32)):
        with pytest.raises(ValueError, match="PitchTrack"):
            capi.PitchTrack(**kw)
    for kw in (dict(min_lag=1.5), dict(max_lag=True), dict(voiced_threshold="0.5"), dict(frames=1)):
        with pytest.raises(TypeError, match="PitchTrack"):
            capi.PitchTrack(**kw)
    with pytest.raises(TypeError, match="pitch_track: params must be a PitchTrack or None"):
        capi.Model.pitch_track(fake, np.zeros(300, F), params=True)
    with pytest.raises(ValueError, match="pitch_track: the waveform must be"):
        capi.Model.pitch_track(fake, np.zeros(301, F))
    # a well-formed call is built without a device: one wish for the batch, or one per utterance
    t = capi.PitchTrack(40, 300, 512, 0.25, phonemes=False)
    bc = capi.BatchCall(fake, two + [(ids, puncts, style, 9)] * 3, return_pitch=["frames", "phonemes", True, False, t])
    shape = lambda a: None if a is None else a.shape
    assert [None if p is None else (shape(p.frames), shape(p.phonemes)) for p in bc.pitches] == \
        [((64, 2), None), (None, (4, 2)), ((9, 2), (4, 2)), None, ((9, 2), None)]
    assert [(bool(s.frames), bool(s.phonemes)) for s in bc.pitch] == [(True, False), (False, True), (True, True), (False, False), (True, False)]
    s = bc.pitch[4]
    assert (s.min_lag, s.max_lag, s.window, s.voiced_threshold) == (40, 300, 512, 0.25) and bc.pitch[0].window == 0
    assert bc.pitch[0].frames == bc.pitches[0].frames.ctypes.data and bc.pitch[2].phonemes == bc.pitches[2].phonemes.ctypes.data
    for none in (False, [False] * 5, capi.PitchTrack(frames=False, phonemes=False)):
        plain = capi.BatchCall(fake, two + [(ids, puncts, style, 9)] * 3, return_pitch=none)
        assert plain.pitch is None and plain.pitches is None
    t = capi.PitchTrack.from_hz(SR, 80, 500)
    assert (t.min_lag, t.max_lag) == (44, 275) and capi.PitchTrack.from_hz(SR).min_lag == 0


def test_call_variant_routes_only_a_pitch_request_to_the_pitch_symbol():
    from zerovox_cpp_amd import capi
    seen = []
    lib = types.SimpleNamespace(**{name: (lambda *a, _n=name: seen.append((_n, a)) or 0)
                                   for name in ("zv_synthesize", "zv_synthesize_volume", "zv_synthesize_contour", "zv_synthesize_pitch")})
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev", "env", "ctr", "pit")
    capi._call_variant(lib, "zv_synthesize", (1, 2), target=0, pitch="pit")
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev", "env", "ctr")
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev", "env", "ctr", None)
    capi._call_variant(lib, "zv_synthesize", (1, 2), target=0, levels="lev", pitch=None)
    capi._call_variant(lib, "zv_synthesize", (1, 2))
    assert seen == [("zv_synthesize_pitch", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev", "env", "ctr", "pit")),
                    ("zv_synthesize_pitch", (1, 2, None, None, None, 0, 0, None, None, None, None, "pit")),
                    ("zv_synthesize_contour", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev", "env", "ctr")),
                    ("zv_synthesize_contour", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev", "env", "ctr")),
                    ("zv_synthesize_volume", (1, 2, None, None, None, 0, 0, None, "lev")), ("zv_synthesize", (1, 2))]


def test_cli_knows_the_flags(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert all(f in r.stdout for f in ("--pitch FILE", "--phoneme-pitch FILE", "--pitch-min-hz F", "--pitch-max-hz F", "--pitch-threshold X"))
    utt = tmp_path / "utt.txt"
    utt.write_text("1 2 3\n0 0 0\n0\n")
    base = [CLI, "-m", "/nonexistent/model.gguf", "-u", str(utt)]
    for args in (["--pitch"], ["--phoneme-pitch"], ["--pitch", str(tmp_path / "f.tsv"), "--pitch-min-hz"], ["--pitch-threshold"]):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and args[-1] + " needs a value" in r.stderr, (args, r.returncode, r.stderr[-300:])
    for args in (["--pitch-min-hz", "0"], ["--pitch-max-hz", "nan"], ["--pitch-threshold", "1.5"], ["--pitch-max-hz", "12x"]):
        r = subprocess.run(base + ["--pitch", str(tmp_path / "f.tsv")] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and args[0] + " needs a number" in r.stderr, (args, r.returncode, r.stderr[-300:])
    r = subprocess.run(base + ["--pitch-min-hz", "80"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "need --pitch FILE or --phoneme-pitch FILE" in r.stderr
    # well-formed flags pass the usage checks: the run then fails at the missing checkpoint, which is no usage error
    r = subprocess.run(base + ["--pitch", str(tmp_path / "f.tsv"), "--phoneme-pitch", str(tmp_path / "p.tsv"), "--pitch-min-hz", "80",
                               "--pitch-max-hz", "500", "--pitch-threshold", "0.3"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stderr[-300:])
