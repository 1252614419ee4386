"""CPU: target durations (include/zerovox_amd.h "target durations").

1. The rule's source (csrc/fit_durations.h, shared with fit_durations_kernel) against a big-integer restatement
   (tests/fit_durations_rule.py), driven through tests/native/fit_durations_check.cpp: a few thousand random cases and the edge
   classes, with the sum property and 0 <= d_i <= T; the same cases once more through a build with -fsanitize=address,undefined.
2. The boundary: the four entry points are declared, exported and bound; each refuses a NULL model; the Python binding checks a
   target before it touches a device; the CLI lists its two flags and refuses a bad value."""
import ctypes as C
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

from fit_durations_rule import WEIGHT_MAX, fit, weight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
CLI = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
NAMES = ("zv_encode_taps_target", "zv_synthesize_target", "zv_synthesize_batch_target", "zv_synthesize_batch_begin_target")


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "fit_durations_check.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fit_durations")
    return _build(tmp, "fit_durations_check", []), _build(tmp, "fit_durations_check_san", ["-fsanitize=address,undefined",
                                                                                          "-fno-sanitize-recover=all"])


def _case(dur, forced, num_phonemes, T, target):
    return (np.asarray(dur, np.float32), None if forced is None else np.asarray(forced, np.int32), int(num_phonemes), int(T),
            int(target))


def _cases():
    """(name, case) pairs: the classes the rule distinguishes, then random ones"""
    rng = np.random.default_rng(20261018)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    out = [
        ("n = 1", _case([3.2], None, 1, 50, 17)),
        ("n = 1, weight 0", _case([0.0], None, 1, 50, 17)),
        ("num_phonemes = 0", _case([1.0, 2.0, 3.0], None, 0, 40, 9)),
        ("num_phonemes < n", _case([1.0, 2.0, 3.0, 4.0, 5.0], [-1, -1, -1, 7, -1], 3, 40, 11)),
        ("all forced", _case([1.0, 2.0, 3.0], [4, 0, 50], 3, 40, 30)),
        ("Fs > target", _case([1.0, 2.0, 3.0, 4.0], [9, -1, 8, -1], 4, 40, 12)),
        ("Fs == target", _case([1.0, 2.0, 3.0, 4.0], [9, -1, 3, -1], 4, 40, 12)),
        ("all weights 0", _case([0.0, -1.5, nan, 0.0, -0.0, 0.0, 0.0], None, 7, 100, 10)),
        ("all weights 0, forced between", _case([0.0, 0.0, 0.0, 0.0, 0.0], [-1, 2, -1, -1, -1], 5, 100, 9)),
        ("+inf and NaN", _case([1.0, inf, nan, 2.5, inf, -inf], None, 6, 1000, 999)),
        ("only +inf", _case([inf, inf, inf], None, 3, 1000, 1000)),
        ("target = 1", _case(rng.uniform(0.1, 9.0, 37), None, 37, 500, 1)),
        ("target = T", _case(rng.uniform(0.1, 9.0, 37), np.where(rng.random(37) < 0.3, 2, -1), 37, 500, 500)),
        ("equal weights, index tie-break", _case(np.full(9, 2.0), None, 9, 100, 13)),
        ("tiny weights", _case(np.full(5, 1e-30), None, 5, 100, 8)),
        ("sub-unit weights", _case([1.6e-5, 3.1e-5, 1.0e-5], None, 3, 100, 50)),
        ("huge weights", _case([3.0e38, 1.7e7, 1.6e7, 1.0], None, 4, 32768, 32768)),
        ("n = 1501, target 32768", _case(rng.lognormal(1.0, 1.0, 1501), None, 1501, 32768, 32768)),
        ("n = 1501, target 32768, all +inf", _case(np.full(1501, inf), None, 1501, 32768, 32768)),
        ("n = 1501, target 32768, forced among", _case(rng.lognormal(1.0, 1.0, 1501), np.where(rng.random(1501) < 0.2, 5, -1), 1501,
                                                       32768, 32768)),
    ]
    special = np.array([0.0, -0.0, -2.0, np.nan, np.inf, 1e-30, 1e-6, 3e38], np.float32)
    for k in range(4000):
        n = int(rng.integers(1, 48)) if k % 50 else int(rng.integers(200, 700))
        dur = rng.lognormal(rng.uniform(-2.0, 3.0), rng.uniform(0.1, 2.0), n).astype(np.float32)
        if rng.random() < 0.3:
            at = rng.random(n) < rng.uniform(0.05, 1.0)
            dur[at] = rng.choice(special, int(at.sum()))
        forced = None
        if rng.random() < 0.6:
            forced = np.where(rng.random(n) < rng.uniform(0.0, 1.0), rng.integers(0, 40, n), -1)
        T = int(rng.choice([1, 2, 7, 64, 1024, 1500, 32768]))
        target = int(rng.choice([1, min(T, max(1, n - 1)), min(T, n + 3), max(1, T // 2), max(1, T - 1), T, int(rng.integers(1, T + 1))]))
        num = n if rng.random() < 0.7 else int(rng.integers(0, n + 1))
        out.append((f"random {k}", _case(dur, forced, num, T, target)))
    return out


def _stdin(cases):
    lines = []
    for _, (dur, forced, num, T, target) in cases:
        lines.append(f"{len(dur)} {num} {T} {target} {int(forced is not None)}")
        lines.append(" ".join("%x" % struct.unpack("<I", struct.pack("<f", float(x)))[0] for x in dur))
        lines.append("" if forced is None else " ".join(str(int(f)) for f in forced))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def cases():
    return _cases()


def test_weight_classes():
    assert weight(np.nan) == 0 and weight(0.0) == 0 and weight(-3.0) == 0 and weight(-np.inf) == 0
    assert weight(np.inf) == WEIGHT_MAX == weight(3e38) == weight(2.0 ** 24) and weight(2.0 ** 24 - 1) == (2 ** 24 - 1) << 16
    assert weight(1.0) == 65536 and weight(1.5) == 98304 and weight(1e-30) == 0 and weight(2.0 ** -16) == 1


def test_header_agrees_with_big_integers(exes, cases):
    exe, _ = exes
    r = subprocess.run([exe], input=_stdin(cases), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = r.stdout.split("\n")
    assert len(rows) == len(cases) + 1 and rows[-1] == ""
    reached = over = equal = 0
    for (name, (dur, forced, num, T, target)), row in zip(cases, rows):
        got = np.array([int(v) for v in row.split()], np.int64)
        want = fit(dur, forced, num, T, target)
        assert np.array_equal(got, want), (name, got, want)
        assert len(got) == len(dur) and (got >= 0).all() and (got <= T).all(), name
        assert not got[num:].any(), name
        nw = min(num, len(dur))
        is_forced = np.zeros(len(dur), bool) if forced is None else np.asarray(forced) >= 0
        is_forced[nw:] = False
        Fs = int(got[is_forced].sum())
        n_free = nw - int(is_forced[:nw].sum())
        if n_free and Fs <= target:
            assert int(got.sum()) == target, name
            reached += 1
        else:
            assert int(got.sum()) == Fs, name
            over += Fs > target
        equal += n_free > 1 and all(weight(dur[i]) == 0 for i in range(nw) if not is_forced[i])
    assert reached > 2000 and over > 100 and equal > 20, (reached, over, equal)


def test_named_results(exes, cases):
    """a few results written out by hand, so that the two restatements cannot be wrong together"""
    by = dict(cases)
    assert fit(*by["all weights 0"]).tolist() == [2, 2, 2, 1, 1, 1, 1]                      # 10 = 7 * 1 + 3: the first three
    assert fit(*by["all weights 0, forced between"]).tolist() == [2, 2, 2, 2, 1]            # R = 7 over four free: 2 2 2 1 around the forced 2
    assert fit(*by["equal weights, index tie-break"]).tolist() == [2, 2, 2, 2, 1, 1, 1, 1, 1]
    assert fit(*by["+inf and NaN"]).tolist() == [0, 500, 0, 0, 499, 0]                      # 2^40 each dwarfs 1.0 and 2.5; the tie goes to index 1
    assert fit(*by["Fs > target"]).tolist() == [9, 0, 8, 0] and fit(*by["Fs == target"]).tolist() == [9, 0, 3, 0]
    assert fit(*by["num_phonemes < n"]).tolist() == [2, 4, 5, 0, 0]                         # 11 over 1 : 2 : 3 = 1.83, 3.67, 5.5 -> 1 + 3 + 5, L = 2
    assert fit(*by["all forced"]).tolist() == [4, 0, 40]
    assert fit(*by["n = 1"]).tolist() == [17] and fit(*by["n = 1, weight 0"]).tolist() == [17]
    assert fit(*by["num_phonemes = 0"]).tolist() == [0, 0, 0]


def test_header_under_address_and_undefined_sanitizers(exes, cases):
    """the stand-alone check program built with -fsanitize=address,undefined gives the same output and reports nothing"""
    exe, san = exes
    text = _stdin(cases[:600])
    a = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    b = subprocess.run([san], input=text, capture_output=True, text=True, timeout=600)
    assert a.returncode == 0 and b.returncode == 0, b.stderr[-3000:]
    assert b.stdout == a.stdout and "runtime error" not in b.stderr and "Sanitizer" not in b.stderr, b.stderr[-3000:]


def test_products_stay_inside_64_bits():
    """q * R < 2^55 and Q < 2^51 at the limits the header states: 1 501 phonemes of the largest weight, 32 768 frames"""
    assert WEIGHT_MAX * 32768 <= 2 ** 55 < 2 ** 63 and 1501 * WEIGHT_MAX < 2 ** 51
    assert 3584 * WEIGHT_MAX < 2 ** 52                     # the kernel's own token limit (kernels.h FIT_MAX_TOKENS)


# ---- 2. the boundary --------------------------------------------------------------------------------------------------------

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
    # each is its _phonemes counterpart's argument list, the target and (synthesize forms) the fitted flag
    assert _declaration(header, "zv_encode_taps_target") == _declaration(header, "zv_encode_taps_phonemes") + ["uint32_t"]
    assert _declaration(header, "zv_synthesize_target") == _declaration(header, "zv_synthesize_phonemes") + ["uint32_t", "int"]
    for name in ("zv_synthesize_batch", "zv_synthesize_batch_begin"):
        assert _declaration(header, name + "_target") == _declaration(header, name + "_phonemes") + ["const uint32_t*", "int"], name
    assert lib.zv_encode_taps_target.argtypes == lib.zv_encode_taps_phonemes.argtypes + [C.c_uint32]
    assert lib.zv_synthesize_target.argtypes == lib.zv_synthesize_phonemes.argtypes + [C.c_uint32, C.c_int]
    assert lib.zv_synthesize_batch_target.argtypes == lib.zv_synthesize_batch_phonemes.argtypes + [C.POINTER(C.c_uint32), C.c_int]
    assert lib.zv_synthesize_batch_begin_target.argtypes == lib.zv_synthesize_batch_begin_phonemes.argtypes + [C.POINTER(C.c_uint32), C.c_int]
    assert not re.search(r"\bzv_synthesize_batch_end_target\b", header)          # the existing _end finishes a target batch


def test_null_model_is_refused_by_every_entry_point():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    n = C.c_uint32(0)
    assert lib.zv_encode_taps_target(None, None, None, None, 4, 4, 8, None, C.byref(n), None, None, None, None, None, None, None, None,
                                     None, 6) == 5
    assert b"zv_encode_taps_target" in lib.zv_last_error()
    assert lib.zv_synthesize_target(None, None, None, None, 4, 8, None, C.byref(n), None, None, None, 6, 1) == 5
    assert b"zv_synthesize_target" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_target(None, 1, None, None, None, None, None, None, None, None, None, None, None, 0) == 5
    assert b"zv_synthesize_batch_target" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_begin_target(None, 0, 1, None, None, None, None, None, None, None, None, None, None, None, 0) == 5
    assert b"zv_synthesize_batch_begin_target" in lib.zv_last_error()


class _NoDevice:
    """stands where a capi.Model would: any touch of the library or the handle fails the test"""
    hp = types.SimpleNamespace(audio_hop_size=300)

    def __getattr__(self, name):
        raise AssertionError(f"the binding touched .{name} before it had checked its arguments")


def test_binding_refuses_bad_targets_before_touching_a_device():
    from zerovox_cpp_amd import capi
    ids, puncts, style = np.ones(4, np.int32), np.zeros(4, np.int32), np.zeros(528, np.float32)
    fake = _NoDevice()
    for call in (capi.Model.synthesize, capi.Model.encode):
        for bad in (2.0, "12", True, [3]):
            with pytest.raises(TypeError, match="target_frames must be an integer"):
                call(fake, ids, puncts, style, 64, target_frames=bad)
        with pytest.raises(ValueError, match="cannot be negative"):
            call(fake, ids, puncts, style, 64, target_frames=-1)
        with pytest.raises(ValueError, match="exceeds the frame capacity T = 64"):
            call(fake, ids, puncts, style, 64, target_frames=65)
    with pytest.raises(ValueError, match="exceeds the frame capacity T = 7"):
        capi.BatchCall(fake, [(ids, puncts, style, 64, None, None, 64), (ids, puncts, style, 7, None, None, 8)])
    with pytest.raises(TypeError, match="target_frames must be an integer"):
        capi.BatchCall(fake, [(ids, puncts, style, 64, None, None, 1.0)])
    # a well-formed call is built without a device; set_target_frames checks against that utterance's capacity
    bc = capi.BatchCall(fake, [(ids, puncts, style, 64, None, None, np.int64(40)), (ids, puncts, style, 7), (ids, puncts, style, 9, None, None, None)])
    assert list(bc.targets) == [40, 0, 0]
    bc.set_target_frames(1, 7)
    bc.set_target_frames(0, None)
    assert list(bc.targets) == [0, 7, 0]
    with pytest.raises(ValueError, match="exceeds the frame capacity T = 7"):
        bc.set_target_frames(1, 8)
    with pytest.raises(TypeError):
        bc.set_target_frames(2, 1.5)
    assert list(bc.targets) == [0, 7, 0]
    plain = capi.BatchCall(fake, [(ids, puncts, style, 64), (ids, puncts, style, 7, None, None, None)])
    assert plain.targets is None
    with pytest.raises(ValueError, match="built without target"):
        plain.set_target_frames(0, 3)


def test_call_variant_routes_targets_to_the_target_symbol():
    from zerovox_cpp_amd import capi
    seen = []
    lib = types.SimpleNamespace(**{name: (lambda *a, _n=name: seen.append((_n, a)) or 0)
                                   for name in ("zv_synthesize", "zv_synthesize_phonemes", "zv_synthesize_fitted", "zv_synthesize_target")})
    capi._call_variant(lib, "zv_synthesize", (1, 2), target=0)
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99)
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True)
    capi._call_variant(lib, "zv_synthesize", (1, 2))
    assert seen == [("zv_synthesize_target", (1, 2, None, None, None, 0, 0)), ("zv_synthesize_target", (1, 2, "pr", "pc", "dur", 99, 1)),
                    ("zv_synthesize_fitted", (1, 2, "pr", "pc", "dur")), ("zv_synthesize", (1, 2))]


def test_cli_knows_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--target-frames" in r.stdout and "--target-seconds" in r.stdout
    for args in (["--target-frames", "abc"], ["--target-frames", "-3"], ["--target-frames", "0"], ["--target-frames", "1.5"],
                 ["--target-frames", "40000"], ["--target-frames"], ["--target-seconds", "x"], ["--target-seconds", "-1"],
                 ["--target-seconds", "0"], ["--target-seconds", "nan"], ["--target-seconds"]):
        r = subprocess.run([CLI, "-m", "/nonexistent/model.gguf"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and args[0] in r.stderr, (args, r.returncode, r.stderr[-300:])
