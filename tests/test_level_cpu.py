"""CPU: volume controls (include/zerovox_amd.h "volume controls").

1. The rule's source (csrc/level.h, shared with level_measure_kernel / level_apply_kernel) against the restatement in Python integers
   and single float64 steps (tests/level_rule.py), driven through tests/native/level_check.cpp: the edge classes and a few thousand
   random cases, bit equality of S, peak, rms and the gain (and of every scaled sample, through a hash); the same cases once more
   through a build with -fsanitize=address,undefined.
2. Two properties of the rule on speech-like input: no finite sample leaves above the ceiling, and without a ceiling the level lands
   on the target within a bound derived from the quantisation step and the two f32 roundings.
3. The boundary: the three entry points are declared, exported and bound; each refuses a NULL model; the Python binding checks a
   volume before it touches a device; the CLI lists its three flags and refuses a bad value."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import level_rule as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
CLI = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
NAMES = ("zv_synthesize_volume", "zv_synthesize_batch_volume", "zv_synthesize_batch_begin_volume")
F = np.float32


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "level_check.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("level")
    return _build(tmp, "level_check", []), _build(tmp, "level_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _speech(rng, cap, scale):
    """speech-like: an enveloped noise through tanh, like the vocoder's output"""
    env = 0.2 + np.abs(np.sin(np.arange(cap) * rng.uniform(0.001, 0.05) + rng.uniform(0, 6)))
    return np.tanh(rng.standard_normal(cap) * env * scale).astype(F)


def _case(x, n, volume=LR.IDENTITY):
    x = np.asarray(x, F)
    return ("w", x, int(n), tuple(float(F(v)) for v in volume))


def _ulp_cases(rng):
    """a ceiling one ulp under, on and one ulp above the scaled peak, with and without a target"""
    out = []
    for k in range(40):
        x = _speech(rng, 257, 0.7)
        n = 200
        gain = F(rng.uniform(0.3, 3.0))
        for target in (0.0, float(F(rng.uniform(0.02, 0.3)))):
            free = LR.rule(x, n, (gain, target, 0.0))
            peak = np.array([free["peak_bits"]], np.uint32).view(F)[0]
            scaled = F(np.float64(free["level"][2]) * np.float64(peak))
            for name, c in (("below", np.nextafter(scaled, F(0))), ("on", scaled), ("above", np.nextafter(scaled, F(2)))):
                if 0 < c <= 1:
                    out.append((f"ceiling one ulp {name} the scaled peak {k} target {target}", _case(x, n, (gain, target, c))))
    return out


def _cases():
    """(name, case) pairs: the classes the rule distinguishes, then random ones"""
    rng = np.random.default_rng(20261019)
    inf, nan = F(np.inf), F(np.nan)
    sp = _speech(rng, 600, 0.8)
    out = [
        ("nf = 0", _case(sp[:64], 0, (2.0, 0.1, 0.5))),
        ("nf = 0, identity", _case(sp[:64], 0)),
        ("all zeros", _case(np.zeros(300, F), 300, (1.5, 0.1, 0.5))),
        ("all -0.0", _case(np.full(300, -0.0, F), 300, (1.0, 0.1, 0.5))),
        ("one sample", _case([0.25], 1, (1.0, 0.1, 0.0))),
        ("one sample, ceiling", _case([-0.25], 1, (4.0, 0.0, 0.5))),
        ("one sample of capacity, none of speech", _case([0.25], 0, (4.0, 0.0, 0.5))),
        ("NaN and +-inf among speech", _case(np.concatenate([sp[:100], [nan, inf, -inf, -nan], sp[100:200]]), 204, (1.0, 0.1, 0.9))),
        ("only NaN and inf", _case([nan, inf, -inf, nan], 4, (1.0, 0.1, 0.9))),
        ("|x| > 1", _case(sp[:300] * F(3.0), 300, (1.0, 0.2, 0.0))),
        ("|x| > 1, ceiling", _case(sp[:300] * F(3.0), 300, (1.0, 0.0, 0.5))),
        ("huge finite", _case([3.0e38, -1.0e30, 0.5], 3, (1000.0, 1.0, 1.0))),
        ("-0.0 among speech", _case(np.concatenate([[-0.0, 0.0], sp[:50]]), 52, (0.5, 0.0, 0.0))),
        ("subnormals", _case([1e-45, -1e-40, 1e-38, 0.0], 4, (1000.0, 1.0, 1.0))),
        ("one subnormal, ceiling", _case([1e-45], 1, (1000.0, 1.0, 1e-45))),
        ("below the quantisation step", _case(np.full(100, 2.0 ** -21, F), 100, (1.0, 0.5, 0.0))),
        ("ceiling binds without a target", _case(sp, 500, (4.0, 0.0, 0.25))),
        ("ceiling binds with a target", _case(sp, 500, (1.0, 0.9, 0.25))),
        ("ceiling does not bind", _case(sp, 500, (0.5, 0.0, 1.0))),
        ("gain = 0", _case(sp, 500, (0.0, 0.0, 0.0))),
        ("gain = 0 with target and ceiling", _case(sp, 500, (0.0, 0.1, 0.5))),
        ("gain = 1000", _case(sp, 500, (1000.0, 0.0, 0.0))),
        ("target = 1, ceiling = 1", _case(sp, 500, (1.0, 1.0, 1.0))),
        ("tail past the speech is scaled, not measured", _case(np.concatenate([sp[:100] * F(0.1), np.full(50, 0.99, F)]), 100, (1.0, 0.2, 0.3))),
        # totals alone: S = 1 with a target, and the largest utterance — 32 768 frames of 300 samples, every one at full scale
        ("target_rms with S = 1", ("t", 1, 300, int(LR.bits(F(2.0 ** -19))[0]), (1.0, 0.1, 0.0))),
        ("target_rms with S = 1, ceiling", ("t", 1, 32768 * 300, int(LR.bits(F(2.0 ** -19))[0]), (1000.0, 1.0, 0.5))),
        ("the largest utterance at full scale", ("t", (1 << 38) * 32768 * 300, 32768 * 300, int(LR.bits(F(1.0))[0]), (1.0, 0.1, 0.5))),
        ("the largest utterance, one step under full scale", ("t", (1 << 38) * 32768 * 300 - 1, 32768 * 300, int(LR.bits(F(0.999))[0]), (2.0, 0.7, 0.0))),
    ]
    out += _ulp_cases(rng)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, 1.0000001, 1e-45, 2.0 ** -20, 3e38], F)
    for k in range(3000):
        cap = int(rng.integers(1, 40)) if k % 3 == 0 else (int(rng.integers(40, 700)) if k % 40 else int(rng.integers(9000, 30000)))
        x = _speech(rng, cap, float(rng.choice([0.01, 0.1, 0.5, 1.0, 3.0])))
        if rng.random() < 0.25:
            at = rng.random(cap) < rng.uniform(0.01, 0.5)
            x[at] = rng.choice(special, int(at.sum()))
        n = cap if rng.random() < 0.5 else int(rng.integers(0, cap + 1))
        gain = float(rng.choice([1.0, 0.0, 1000.0, rng.uniform(0.05, 20.0)]))
        target = float(rng.choice([0.0, 1.0, rng.uniform(0.001, 1.0)]))
        ceiling = float(rng.choice([0.0, 1.0, rng.uniform(0.001, 1.0)]))
        out.append((f"random {k}", _case(x, n, (gain, target, ceiling))))
    return out


def _hex(v):
    return "%x" % int(LR.bits(F(v))[0])


def _stdin(cases):
    lines = []
    for _, c in cases:
        if c[0] == "w":
            _, x, n, vol = c
            lines.append(f"0 {n} {len(x)} " + " ".join(_hex(v) for v in vol))
            lines.append(" ".join("%x" % b for b in LR.bits(x)))
        else:
            _, S, n, pk, vol = c
            lines.append(f"1 {S} {n} {pk:x} " + " ".join(_hex(v) for v in vol))
    return "\n".join(lines) + "\n"


def _expect(c):
    """what the check program must print for a case, from the restatement"""
    if c[0] == "w":
        _, x, n, vol = c
        r = LR.rule(x, n, vol)
        S, pk, rms, level = r["S"], r["peak_bits"], r["rms"], r["level"]
        idx = np.arange(1, len(x) + 1, dtype=np.uint64)
        with np.errstate(over="ignore"):
            h = int(np.sum(LR.bits(r["out"]).astype(np.uint64) * idx, dtype=np.uint64))
    else:
        _, S, n, pk, vol = c
        rms, level = LR.report(S, n, pk, vol)
        h = 0
    lb = LR.level_bits(level)
    return f"{S} {pk:x} {int(np.array([rms], np.float64).view(np.uint64)[0]):x} {lb[0]:x} {lb[1]:x} {lb[2]:x} 0 {h}"


@pytest.fixture(scope="module")
def cases():
    return _cases()


def test_header_agrees_with_the_restatement_bit_for_bit(exes, cases):
    exe, _ = exes
    r = subprocess.run([exe], input=_stdin(cases), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = r.stdout.split("\n")
    assert len(rows) == len(cases) + 1 and rows[-1] == ""
    bound = stepped = 0
    for (name, c), row in zip(cases, rows):
        want = _expect(c)
        assert row == want, (name, row, want)
        if c[0] == "w" and c[3][2] > 0:
            _, x, n, vol = c
            free = LR.rule(x, n, (vol[0], vol[1], 0.0))["level"][2]
            got = LR.rule(x, n, vol)["level"][2]
            bound += got != free
            pk = np.array([LR.measure(x[:n])[1]], np.uint32).view(F)[0]
            stepped += got != free and pk > 0 and F(np.float64(vol[2]) / np.float64(pk)) != got
    assert bound > 300 and stepped > 3, (bound, stepped)        # the ceiling binds often, and the step down is taken


def test_named_results(cases):
    """a few results written out by hand, so that the two restatements cannot be wrong together"""
    by = dict(cases)
    rule = lambda name: LR.rule(*by[name][1:])
    assert LR.quant(F([0.0, -0.0, 1.0, -1.0, 5.0, 0.5, np.nan, np.inf, -np.inf, 2.0 ** -20, 2.0 ** -21, 1e-45])).tolist() == \
        [0, 0, 524288, 524288, 524288, 262144, 0, 0, 0, 1, 0, 0]              # 2^-20 * 2^19 + 0.5 = 1.0; 2^-21: 0.75 -> 0
    r = rule("one sample")                                                        # q = 2^17, rms = 0.25 exactly, g = 0.1f / 0.25
    assert r["S"] == 1 << 34 and r["rms"] == 0.25 and r["level"][2] == F(np.float64(F(0.1)) / 0.25)
    r = rule("one sample, ceiling")                                               # 4 * 0.25 = 1 > 0.5: g = 0.5 / 0.25
    assert r["level"][2] == F(2.0) and r["out"].tolist() == [-0.5]
    for name in ("nf = 0", "one sample of capacity, none of speech"):
        r = rule(name)                                                            # nothing measured: the plain gain, the capacity scaled
        assert r["S"] == 0 and r["peak_bits"] == 0 and r["rms"] == 0 and r["level"][2] == F(by[name][3][0])
        assert np.array_equal(r["out"], by[name][1] * F(by[name][3][0]))
    r = rule("only NaN and inf")
    assert r["S"] == 0 and r["peak_bits"] == 0 and r["level"][2] == F(1.0)
    r = rule("NaN and +-inf among speech")
    assert np.isfinite(np.array([r["peak_bits"]], np.uint32).view(F)[0]) and r["S"] > 0
    r = rule("|x| > 1")                                                           # clamped in S, not in the peak
    assert np.array([r["peak_bits"]], np.uint32).view(F)[0] > 1 and r["rms"] <= 1.0
    r = rule("all -0.0")
    assert r["S"] == 0 and r["peak_bits"] == 0 and LR.bits(r["out"]).tolist() == [0x80000000] * 300
    assert rule("gain = 0 with target and ceiling")["level"][2] == 0 and rule("gain = 0")["level"][2] == 0
    assert rule("below the quantisation step")["S"] == 0
    t = by["tail past the speech is scaled, not measured"]
    r = LR.rule(*t[1:])
    assert np.abs(r["out"][100:]).max() > 0.3                                     # the ceiling looks at the speech alone
    rms, level = LR.report(*by["target_rms with S = 1"][1:])
    assert rms == np.sqrt(1.0 / (300 * 2.0 ** 38)) and level[2] == F(np.float64(F(0.1)) / rms)
    rms, level = LR.report(*by["the largest utterance at full scale"][1:])
    assert rms == 1.0 and level[0] == 1 and level[2] == F(0.1)


def test_sum_of_squares_stays_inside_64_bits():
    """the largest utterance, computed and not allocated: zv_max_frames() <= 32 768 frames of at most 300 samples, every q = 2^19"""
    S_max = (1 << 38) * 32768 * 300
    assert S_max < 1 << 62 and int(LR.quant(F([7.0]))[0]) ** 2 == 1 << 38
    assert float(S_max) == S_max                       # and it converts to f64 exactly: the level of full scale is exactly 1


def test_header_under_address_and_undefined_sanitizers(exes, cases):
    """the stand-alone check program built with -fsanitize=address,undefined gives the same output and reports nothing"""
    exe, san = exes
    text = _stdin(cases[:700])
    a = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    b = subprocess.run([san], input=text, capture_output=True, text=True, timeout=600)
    assert a.returncode == 0 and b.returncode == 0, b.stderr[-3000:]
    assert b.stdout == a.stdout and "runtime error" not in b.stderr and "Sanitizer" not in b.stderr, b.stderr[-3000:]


# ---- 2. two properties ------------------------------------------------------------------------------------------------------

def _speech_with_level(rng):
    while True:
        cap = int(rng.integers(300, 20000))
        x = _speech(rng, cap, float(rng.uniform(0.05, 2.0)))
        n = int(rng.integers(cap // 2, cap + 1))
        rms_in = float(np.sqrt(np.mean(x[:n].astype(np.float64) ** 2)))
        if rms_in >= 0.01:
            return x, n, rms_in


def test_no_finite_sample_leaves_above_the_ceiling():
    rng = np.random.default_rng(5)
    binds = 0
    for _ in range(400):
        x, n, _ = _speech_with_level(rng)
        vol = (float(rng.uniform(0.0, 30.0)), float(rng.choice([0.0, rng.uniform(0.01, 1.0)])), float(F(rng.uniform(0.001, 1.0))))
        r = LR.rule(x, n, vol)
        out = r["out"][:n]
        assert not (np.abs(out[np.isfinite(out)]) > F(vol[2])).any(), vol
        binds += r["level"][2] != LR.rule(x, n, (vol[0], vol[1], 0.0))["level"][2]
    assert binds > 100, binds


def test_level_lands_on_the_target_when_the_ceiling_does_not_bind():
    """|rms(out) - target| <= target * (2^-20 / rms_in + 2^-22): quantisation moves the measured rms by at most 2^-20 absolute (half a
    step of 2^-19 per sample, the triangle inequality), so the gain is off by at most 2^-20 / rms_in relative; rounding the gain to
    f32 and each product to f32 adds 2^-24 each.  The restatement alone is checked against it here; the GPU is held to the
    restatement's bits."""
    rng = np.random.default_rng(6)
    worst = 0.0
    for _ in range(300):
        x, n, rms_in = _speech_with_level(rng)
        target = float(F(rng.uniform(0.005, 0.5)))
        ceiling = float(rng.choice([0.0, 1.0]))
        r = LR.rule(x, n, (1.0, target, ceiling))
        if ceiling and r["level"][2] != LR.rule(x, n, (1.0, target, 0.0))["level"][2]:
            continue                                   # the ceiling bound: the other property
        rms_out = float(np.sqrt(np.mean(r["out"][:n].astype(np.float64) ** 2)))
        bound = target * (2.0 ** -20 / rms_in + 2.0 ** -22)
        assert abs(rms_out - target) <= bound, (rms_in, target, rms_out, bound)
        worst = max(worst, abs(rms_out - target) / bound)
    assert 0 < worst <= 1.0


# ---- 3. the boundary --------------------------------------------------------------------------------------------------------

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
    # each is its _target counterpart's argument list, then the volumes and the levels
    for name in ("zv_synthesize", "zv_synthesize_batch", "zv_synthesize_batch_begin"):
        assert _declaration(header, name + "_volume") == _declaration(header, name + "_target") + ["const zv_volume*", "zv_level*"], name
        assert getattr(lib, name + "_volume").argtypes == getattr(lib, name + "_target").argtypes + [C.POINTER(capi.Volume), C.POINTER(capi.Level)]
    assert not re.search(r"\bzv_synthesize_batch_end_volume\b", header)          # the existing _end finishes a volume batch
    assert C.sizeof(capi.Volume) == 12 and C.sizeof(capi.Level) == 16
    v = capi.Volume()
    assert (v.gain, v.target_rms, v.peak_ceiling) == (1.0, 0.0, 0.0)
    assert re.search(r"typedef struct\s*\{\s*float gain;\s*float target_rms;\s*float peak_ceiling;\s*\}\s*zv_volume;", header)
    assert re.search(r"typedef struct\s*\{\s*float\s+rms, peak;\s*float\s+gain;\s*uint32_t reserved;\s*\}\s*zv_level;", header)
    assert LR.chunk_samples(ROOT) % 4 == 0


def test_null_model_is_refused_by_every_entry_point():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    n = C.c_uint32(0)
    vol, lev = capi.Volume(), capi.Level()
    assert lib.zv_synthesize_volume(None, None, None, None, 4, 8, None, C.byref(n), None, None, None, 0, 0, C.byref(vol), C.byref(lev)) == 5
    assert b"zv_synthesize_volume" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_volume(None, 1, None, None, None, None, None, None, None, None, None, None, None, 0, vol, lev) == 5
    assert b"zv_synthesize_batch_volume" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_begin_volume(None, 0, 1, None, None, None, None, None, None, None, None, None, None, None, 0, vol, lev) == 5
    assert b"zv_synthesize_batch_begin_volume" in lib.zv_last_error()


class _NoDevice:
    """stands where a capi.Model would: any touch of the library or the handle fails the test"""
    hp = types.SimpleNamespace(audio_hop_size=300)

    def __getattr__(self, name):
        raise AssertionError(f"the binding touched .{name} before it had checked its arguments")


BAD = [((float("nan"), 0, 0), "gain = nan is not finite"), ((float("inf"), 0, 0), "gain = inf is not finite"),
       ((-0.5, 0, 0), r"gain = -0.5 is outside \[0, 1000\]"), ((1000.5, 0, 0), r"gain = 1000.5 is outside \[0, 1000\]"),
       ((1, float("nan"), 0), "target_rms = nan is not finite"), ((1, -0.1, 0), r"target_rms = .* is outside \[0, 1\]"),
       ((1, 1.5, 0), r"target_rms = 1.5 is outside \[0, 1\]"), ((1, 0, float("-inf")), "peak_ceiling = -inf is not finite"),
       ((1, 0, -1e-3), r"peak_ceiling = .* is outside \[0, 1\]"), ((1, 0, 2), r"peak_ceiling = 2.0 is outside \[0, 1\]")]


def test_binding_refuses_bad_volumes_before_touching_a_device():
    from zerovox_cpp_amd import capi
    ids, puncts, style = np.ones(4, np.int32), np.zeros(4, np.int32), np.zeros(528, np.float32)
    fake = _NoDevice()
    for bad, msg in BAD:
        with pytest.raises(ValueError, match=msg):
            capi.Model.synthesize(fake, ids, puncts, style, 64, volume=bad)
        with pytest.raises(ValueError, match="utterance 1: volume " + msg):
            capi.BatchCall(fake, [(ids, puncts, style, 64), (ids, puncts, style, 7)], volume=[None, capi.Volume(*bad)])
    for bad in (("1", 0, 0), (True, 0, 0), (1, None, 0), (1, 0, [0.5])):
        with pytest.raises(TypeError, match="must be a number"):
            capi.Model.synthesize(fake, ids, puncts, style, 64, volume=bad)
    with pytest.raises(ValueError, match="got 2 values"):
        capi.Model.synthesize(fake, ids, puncts, style, 64, volume=(1, 0))
    with pytest.raises(ValueError, match="unknown volume field"):
        capi.Model.synthesize(fake, ids, puncts, style, 64, volume=dict(gain=1, loudness=0.1))
    with pytest.raises(TypeError, match="return_levels must be a bool"):
        capi.Model.synthesize(fake, ids, puncts, style, 64, return_levels=1)
    with pytest.raises(ValueError, match="volume has 1 entries, the batch has 2"):
        capi.BatchCall(fake, [(ids, puncts, style, 64), (ids, puncts, style, 7)], volume=[None])
    # a well-formed call is built without a device; None entries get the identity, set_volume rewrites in place and checks
    bc = capi.BatchCall(fake, [(ids, puncts, style, 64), (ids, puncts, style, 7), (ids, puncts, style, 9)],
                        volume=[dict(target_rms=0.1), None, (2.0, 0.0, 0.5)])
    as_tuples = lambda: [(v.gain, v.target_rms, v.peak_ceiling) for v in bc.volume]
    assert as_tuples() == [(1.0, float(F(0.1)), 0.0), (1.0, 0.0, 0.0), (2.0, 0.0, 0.5)] and len(bc.levels) == 3
    bc.set_volume(1, capi.Volume(0.5, 0.25, 1.0))
    bc.set_volume(0, None)
    assert as_tuples() == [(1.0, 0.0, 0.0), (0.5, 0.25, 1.0), (2.0, 0.0, 0.5)]
    with pytest.raises(ValueError, match=r"utterance 2: volume gain = -1.0 is outside \[0, 1000\]"):
        bc.set_volume(2, (-1, 0, 0))
    assert as_tuples()[2] == (2.0, 0.0, 0.5)
    plain = capi.BatchCall(fake, [(ids, puncts, style, 64)])
    assert plain.volume is None and plain.levels is None
    with pytest.raises(ValueError, match="built without volume"):
        plain.set_volume(0, (1, 0, 0))
    meter = capi.BatchCall(fake, [(ids, puncts, style, 64)], return_levels=True)
    assert meter.volume is None and len(meter.levels) == 1


def test_from_db():
    from zerovox_cpp_amd import capi
    v = capi.Volume.from_db()
    assert (v.gain, v.target_rms, v.peak_ceiling) == (1.0, 0.0, 0.0)
    v = capi.Volume.from_db(gain_db=6, target_dbfs=-20, peak_dbfs=-1)
    assert v.gain == F(10 ** 0.3) and v.target_rms == F(0.1) and v.peak_ceiling == F(10 ** -0.05)
    assert capi.Volume.from_db(gain_db=60).gain == 1000.0 and capi.Volume.from_db(target_dbfs=0).target_rms == 1.0


def test_call_variant_routes_volume_to_the_volume_symbol():
    from zerovox_cpp_amd import capi
    seen = []
    lib = types.SimpleNamespace(**{name: (lambda *a, _n=name: seen.append((_n, a)) or 0)
                                   for name in ("zv_synthesize", "zv_synthesize_target", "zv_synthesize_volume")})
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev")
    capi._call_variant(lib, "zv_synthesize", (1, 2), target=0, levels="lev")
    capi._call_variant(lib, "zv_synthesize", (1, 2), target=0)
    capi._call_variant(lib, "zv_synthesize", (1, 2))
    assert seen == [("zv_synthesize_volume", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev")),
                    ("zv_synthesize_volume", (1, 2, None, None, None, 0, 0, None, "lev")),
                    ("zv_synthesize_target", (1, 2, None, None, None, 0, 0)), ("zv_synthesize", (1, 2))]


def test_cli_knows_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(f in r.stdout for f in ("--gain-db", "--loudness-dbfs", "--peak-dbfs"))
    for args in (["--gain-db", "abc"], ["--gain-db", "61"], ["--gain-db", "nan"], ["--gain-db", "-300"], ["--gain-db"],
                 ["--loudness-dbfs", "1"], ["--loudness-dbfs", "x"], ["--loudness-dbfs", "inf"], ["--loudness-dbfs"],
                 ["--peak-dbfs", "0.5"], ["--peak-dbfs", "-1dB"], ["--peak-dbfs", "-1e9"], ["--peak-dbfs"]):
        r = subprocess.run([CLI, "-m", "/nonexistent/model.gguf"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and args[0] in r.stderr, (args, r.returncode, r.stderr[-300:])
