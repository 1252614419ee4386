"""Level contour (include/zerovox_amd.h "level contour") on the CPU: csrc/contour.h against its restatement in Python integers and
single float64 steps (tests/contour_rule.py on top of tests/level_rule.py), bit for bit.
 * tests/native/contour_check.cpp drives zv::contour_extent and zv::contour_reference over the named edge classes and about 3 000
   random small cases: the clipped durations, every frame's totals and row and every phoneme's row must agree;
 * the same input through a build with -fsanitize=address,undefined;
 * the properties the header states, and a handful of results written out by hand;
 * the boundary: the three entry points are declared, exported and bound with their _envelope counterpart's arguments plus one pointer,
   refuse a NULL model by name, the binding refuses a bad return_contour before it touches a device, _call_variant routes a contour
   and nothing else to the _contour symbol, and the CLI knows its flags."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import contour_rule as CR
import level_rule as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
CLI = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
NAMES = ("zv_synthesize_contour", "zv_synthesize_batch_contour", "zv_synthesize_batch_begin_contour")
F = np.float32
SPECIALS = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x7f7fffff], np.uint32).view(F)


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "contour_check.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("contour_check")
    return _build(tmp, "contour_check", []), _build(tmp, "contour_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# ---- cases ------------------------------------------------------------------------------------------------------------------

def _wave(rng, total, specials=False):
    x = (rng.standard_normal(total) * 0.3).astype(F)
    if specials and total:
        at = rng.integers(0, total, size=min(total, 6))
        x[at] = SPECIALS[:len(at)]
    return x


def _case(name, rng, T, hop, raw, x=None, tail=None, specials=False):
    """raw: the durations before the capacity cuts them (their scan is what the library keeps).  tail: what the samples behind the
    speech hold (None: like the speech)"""
    cum = np.cumsum([int(d) for d in raw]).astype(np.int64)
    clipped = np.diff(np.minimum(np.concatenate([[0], cum]), T)).astype(int).tolist()
    x = _wave(rng, T * hop, specials) if x is None else np.asarray(x, F)
    assert x.shape == (T * hop,)
    if tail is not None:
        x[sum(clipped) * hop:] = tail
    return dict(name=name, T=T, hop=hop, cum=cum.tolist(), dur=clipped, x=x)


def _named(rng):
    c = [_case("nf = 0", rng, 5, 4, [0, 0, 0]),
         _case("nf = 0, a zero waveform", rng, 5, 4, [0], tail=0.0),
         _case("one frame", rng, 1, 5, [1]),
         _case("one frame of many", rng, 6, 4, [0, 1, 0]),
         _case("one phoneme", rng, 12, 4, [9]),
         _case("phonemes of 0 frames between others", rng, 20, 4, [3, 0, 0, 4, 0, 5, 0]),
         _case("a phoneme cut off by T", rng, 10, 4, [4, 9, 5]),
         _case("a phoneme that starts at T", rng, 10, 4, [4, 6, 5, 1]),
         _case("T = nf", rng, 9, 4, [2, 3, 4]),
         _case("a zero tail behind nf", rng, 12, 4, [2, 3, 1], tail=0.0),
         _case("a tail behind nf that is not zero", rng, 12, 4, [2, 3, 1], tail=0.25),
         _case("NaN, inf, -0.0 samples", rng, 8, 4, [3, 3], specials=True),
         _case("NaN, inf, -0.0 samples, hop 1", rng, 24, 1, [7, 0, 9, 8], specials=True),
         _case("only NaN and inf", rng, 3, 2, [1, 2], x=np.array([0x7fc00000, 0x7f800000, 0xff800000, 0xffc00000, 0x7f800001, 0x7f800000], np.uint32).view(F)),
         _case("samples at and above 1.0", rng, 4, 4, [2, 2], x=np.array([1.0, -1.0, 1.0000001, 0.99999994, 2.0, -3.5, 1e30, 1.0] + [1.0] * 4 + [-7.0] * 4, F)),
         _case("a frame of all zeros", rng, 6, 4, [2, 1, 3], x=np.concatenate([_wave(rng, 8), np.zeros(4, F), _wave(rng, 12)])),
         _case("a phoneme of all -0.0", rng, 4, 3, [1, 2, 1], x=np.concatenate([_wave(rng, 3), np.full(6, -0.0, F), _wave(rng, 3)]))]
    for hop in (1, 3, 4, 5, 7, 12):
        c.append(_case(f"hop = {hop}", rng, 9, hop, [2, 0, 3, 2]))
        c.append(_case(f"hop = {hop}, specials, cut off", rng, 7, hop, [2, 0, 3, 9], specials=True))
    return c


def _random(rng, count):
    c = []
    for k in range(count):
        T, hop = int(rng.integers(1, 25)), int(rng.choice([1, 2, 3, 4, 5, 7, 12]))
        n = int(rng.integers(1, 9))
        raw = rng.integers(0, 7, size=n) * (rng.random(n) < 0.75)
        tail = [None, 0.0, 0.25][int(rng.integers(0, 3))]
        c.append(_case(f"random {k}", rng, T, hop, raw, tail=tail, specials=rng.random() < 0.15))
        if k % 7 == 0:
            with np.errstate(over="ignore"):
                c[-1]["x"] *= F(6.0)         # many samples above 1.0
    return c


def _stdin(cases):
    lines = []
    for c in cases:
        lines.append(f"{c['T']} {c['hop']} {len(c['cum'])}")
        lines.append(" ".join(map(str, c["cum"])))
        lines.append(" ".join("%x" % b for b in CR.bits(c["x"])))
    return "\n".join(lines) + "\n"


def _expect(c):
    r = CR.rule(c["x"], c["T"], c["hop"], c["dur"])
    fb, pb = CR.bits(r["frames"]), CR.bits(r["phonemes"])
    line = "".join(f"{d} " for d in c["dur"]) + "|"
    line += "".join(f" {r['S'][f]}:{r['P'][f]:x}:{fb[f, 0]:x}:{fb[f, 1]:x}" for f in range(c["T"])) + " |"
    return line + "".join(f" {pb[i, 0]:x}:{pb[i, 1]:x}" for i in range(len(c["dur"])))


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(20261020)
    return _named(rng) + _random(rng, 3000)


@pytest.fixture(scope="module")
def outputs(exes, cases):
    text = _stdin(cases)
    runs = [subprocess.run([e], input=text, capture_output=True, text=True, timeout=600) for e in exes]
    return runs


# ---- 1. header against restatement --------------------------------------------------------------------------------------------

def test_header_equals_restatement_bit_for_bit(cases, outputs):
    r = outputs[0]
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    for c, line in zip(cases, got):
        assert line == _expect(c), c["name"]


def test_sanitized_build_agrees_and_is_silent(outputs):
    plain, san = outputs
    assert san.returncode == 0 and san.stderr == "", san.stderr[-3000:]
    assert san.stdout == plain.stdout


# ---- 2. the properties the header states ------------------------------------------------------------------------------------------

def test_frame_totals_add_up_to_the_level_meters(cases):
    """up to nf the frames' sums and peaks are level_rule.measure's S and peak; the phonemes' sums partition them"""
    for c in cases:
        r = CR.rule(c["x"], c["T"], c["hop"], c["dur"])
        nf = sum(c["dur"])
        S, pk = LR.measure(c["x"][:nf * c["hop"]]) if nf else (0, 0)
        assert sum(r["S"][:nf]) == S and max(r["P"][:nf], default=0) == pk, c["name"]
        assert sum(r["pS"]) == S and max(r["pP"], default=0) == pk, c["name"]
        assert S < 1 << 62
        # the frame peaks as floats: their maximum is the zv_level peak of a meter-only call
        level = LR.report(S, nf * c["hop"], pk)[1]
        assert CR.bits(np.max(r["frames"][:nf, 1], initial=F(0)))[()] == LR.bits(level[1])[0], c["name"]
        # a phoneme of no frames has the row {0, 0}
        for i, d in enumerate(c["dur"]):
            if d == 0:
                assert CR.bits(r["phonemes"][i]).tolist() == [0, 0], c["name"]


def test_zero_frames_give_zero_rows_and_other_tails_do_not(cases):
    for c in cases:
        if c["name"] in ("a zero tail behind nf", "a tail behind nf that is not zero"):
            r = CR.rule(c["x"], c["T"], c["hop"], c["dur"])
            nf = sum(c["dur"])
            if "not" in c["name"]:
                assert np.all(CR.bits(r["frames"][nf:]) == CR.bits(F(0.25))[()])
            else:
                assert not CR.bits(r["frames"][nf:]).any()


# ---- 3. results written out by hand -------------------------------------------------------------------------------------------------

def test_results_by_hand(exes):
    nan, inf = F("nan"), F("inf")
    x = np.array([0.5, -0.5, 0.5, 0.5,        # q = 2^18 each: S = 2^38, rms = sqrt(2^38 / (4 * 2^38)) = 0.5
                  1.0, 0.0, 0.0, 0.0,         # S = 2^38: rms 0.5, peak 1
                  2.0, -2.0, 2.0, -4.0,       # clamped in the sum (S = 4 * 2^38: rms 1), not in the peak: 4
                  nan, inf, -0.0, 0.25,       # only 0.25 counts: S = 2^34, rms = sqrt(2^-6) = 0.125, peak 0.25
                  0.0, -0.0, 0.0, 0.0], F)    # {0, 0}
    dur = [2, 0, 1, 2, 0]
    r = CR.rule(x, 5, 4, dur)
    assert r["S"] == [1 << 38, 1 << 38, 1 << 40, 1 << 34, 0]
    assert r["frames"].tolist() == [[0.5, 0.5], [0.5, 1.0], [1.0, 4.0], [0.125, 0.25], [0.0, 0.0]]
    # phoneme 0: S = 2^39 over 8 samples: 0.5, peak 1.  phoneme 3: S = 2^34 over 8 samples: sqrt(2^-7)
    want = [[0.5, 1.0], [0.0, 0.0], [1.0, 4.0], [F(np.sqrt(2.0 ** -7)), 0.25], [0.0, 0.0]]
    assert r["phonemes"].tolist() == [[float(F(a)), float(F(b))] for a, b in want]
    c = dict(T=5, hop=4, cum=np.cumsum(dur).tolist(), dur=dur, x=x)
    out = subprocess.run([exes[0]], input=_stdin([c]), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.splitlines() == [_expect(c)]
    assert " 274877906944:3f800000:3f000000:3f800000 " in out.stdout           # frame 1, spelled out


# ---- 4. the boundary --------------------------------------------------------------------------------------------------------------

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
        assert _declaration(header, name + "_contour") == _declaration(header, name + "_envelope") + ["const zv_contour*"], name
        assert getattr(lib, name + "_contour").argtypes == getattr(lib, name + "_envelope").argtypes + [C.POINTER(capi.ContourC)]
    assert not re.search(r"\bzv_synthesize_batch_end_contour\b", header)           # the existing _end finishes a contour batch
    assert C.sizeof(capi.ContourC) == 16 and bytes(capi.ContourC()) == bytes(16)      # zero-initialised = none
    assert re.search(r"typedef struct\s*\{\s*float rms, peak;\s*\}\s*zv_frame_level;", header)
    assert re.search(r"typedef struct\s*\{\s*zv_frame_level \*frames;\s*zv_frame_level \*phonemes;\s*\}\s*zv_contour;", header)
    # the header reuses level.h's arithmetic and does not copy it
    text = open(os.path.join(CSRC, "contour.h")).read()
    assert '#include "level.h"' in text and not re.search(r"524288|274877906944|0x7f800000", text)
    assert CR.chunk_frames(ROOT) * 300 == LR.chunk_samples(ROOT)


def test_null_model_is_refused_by_every_entry_point():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    n = C.c_uint32(0)
    ctr = capi.ContourC()
    assert lib.zv_synthesize_contour(None, None, None, None, 4, 8, None, C.byref(n), None, None, None, 0, 0, None, None, None, C.byref(ctr)) == 5
    assert b"zv_synthesize_contour" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_contour(None, 1, None, None, None, None, None, None, None, None, None, None, None, 0, None, None, None, ctr) == 5
    assert b"zv_synthesize_batch_contour" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_begin_contour(None, 0, 1, None, None, None, None, None, None, None, None, None, None, None, 0, None, None,
                                                 None, ctr) == 5
    assert b"zv_synthesize_batch_begin_contour" in lib.zv_last_error()


class _NoDevice:
    """stands where a capi.Model would: any touch of the library or the handle fails the test"""
    hp = types.SimpleNamespace(audio_hop_size=300)

    def __getattr__(self, name):
        raise AssertionError(f"the binding touched .{name} before it had checked its arguments")


def test_binding_refuses_a_bad_return_contour_before_touching_a_device():
    from zerovox_cpp_amd import capi
    ids, puncts, style = np.ones(4, np.int32), np.zeros(4, np.int32), np.zeros(528, np.float32)
    fake = _NoDevice()
    two = [(ids, puncts, style, 64), (ids, puncts, style, 7)]
    for bad in ("frame", "both", ""):
        with pytest.raises(ValueError, match="return_contour = %r: expected False, True, 'frames' or 'phonemes'" % bad):
            capi.Model.synthesize(fake, ids, puncts, style, 64, return_contour=bad)
        with pytest.raises(ValueError, match="utterance 1: return_contour = %r" % bad):
            capi.BatchCall(fake, two, return_contour=[True, bad])
    for bad in (1, None, 2.0, b"frames"):
        with pytest.raises(TypeError, match="return_contour must be a bool, 'frames' or 'phonemes'"):
            capi.Model.synthesize(fake, ids, puncts, style, 64, return_contour=bad)
        with pytest.raises(TypeError, match="return_contour must be a bool, 'frames' or 'phonemes'"):
            capi.BatchCall(fake, two, return_contour=bad)
    with pytest.raises(ValueError, match="return_contour has 1 entries, the batch has 2"):
        capi.BatchCall(fake, two, return_contour=["frames"])
    # a well-formed call is built without a device: one wish for the batch, or one per utterance
    bc = capi.BatchCall(fake, two + [(ids, puncts, style, 9)] * 2, return_contour=["frames", "phonemes", True, False])
    shape = lambda a: None if a is None else a.shape
    assert [None if c is None else (shape(c.frames), shape(c.phonemes)) for c in bc.contours] == \
        [((64, 2), None), (None, (4, 2)), ((9, 2), (4, 2)), None]
    assert [(bool(s.frames), bool(s.phonemes)) for s in bc.contour] == [(True, False), (False, True), (True, True), (False, False)]
    assert bc.contour[0].frames == bc.contours[0].frames.ctypes.data and bc.contour[2].phonemes == bc.contours[2].phonemes.ctypes.data
    assert all(c.frames.dtype == F for c in capi.BatchCall(fake, two, return_contour=True).contours)
    for none in (False, [False, False]):
        plain = capi.BatchCall(fake, two, return_contour=none)
        assert plain.contour is None and plain.contours is None


def test_dbfs_helper():
    from zerovox_cpp_amd import capi
    db = capi.Contour.dbfs(np.array([[1.0, 0.5], [0.1, 0.0]], F))
    assert db.shape == (2, 2) and db[0, 0] == 0.0 and abs(db[0, 1] + 6.0206) < 1e-4 and abs(db[1, 0] + 20.0) < 1e-5 and db[1, 1] == -np.inf
    c = capi.Contour(3, 2, frames=True, phonemes=False)
    assert c.frames.shape == (3, 2) and c.phonemes is None and not c.struct.phonemes and c.struct.frames == c.frames.ctypes.data


def test_call_variant_routes_only_a_contour_to_the_contour_symbol():
    from zerovox_cpp_amd import capi
    seen = []
    lib = types.SimpleNamespace(**{name: (lambda *a, _n=name: seen.append((_n, a)) or 0)
                                   for name in ("zv_synthesize", "zv_synthesize_volume", "zv_synthesize_envelope", "zv_synthesize_contour")})
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev", "env", "ctr")
    capi._call_variant(lib, "zv_synthesize", (1, 2), target=0, contour="ctr")
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev", "env")
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev", "env", None)
    capi._call_variant(lib, "zv_synthesize", (1, 2), target=0, levels="lev", contour=None)
    capi._call_variant(lib, "zv_synthesize", (1, 2))
    assert seen == [("zv_synthesize_contour", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev", "env", "ctr")),
                    ("zv_synthesize_contour", (1, 2, None, None, None, 0, 0, None, None, None, "ctr")),
                    ("zv_synthesize_envelope", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev", "env")),
                    ("zv_synthesize_envelope", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev", "env")),
                    ("zv_synthesize_volume", (1, 2, None, None, None, 0, 0, None, "lev")), ("zv_synthesize", (1, 2))]


def test_cli_knows_the_flags(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(f in r.stdout for f in ("--contour FILE", "--phoneme-levels FILE"))
    utt = tmp_path / "utt.txt"
    utt.write_text("1 2 3\n0 0 0\n0\n")
    for args in (["--contour"], ["--phoneme-levels"], ["--contour", str(tmp_path / "c.tsv"), "--phoneme-levels"]):
        r = subprocess.run([CLI, "-m", "/nonexistent/model.gguf", "-u", str(utt)] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and args[-1] + " needs a value" in r.stderr, (args, r.returncode, r.stderr[-300:])
    # well-formed flags pass the usage checks: the run then fails at the missing checkpoint, which is no usage error
    r = subprocess.run([CLI, "-m", "/nonexistent/model.gguf", "-u", str(utt), "--contour", str(tmp_path / "c.tsv"), "--phoneme-levels",
                        str(tmp_path / "p.tsv")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stderr[-300:])
