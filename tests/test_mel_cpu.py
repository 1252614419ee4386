"""Mel analysis (include/zerovox_amd.h "mel analysis") on the CPU: csrc/mel.h against its restatement in exact integers and single
float64 steps (tests/mel_rule.py), bit for bit.
 * tests/native/mel_check.cpp drives zv::mel_resolve and zv::mel_reference over hop 256 and 300, both pads, centre 0 and hop / 2, the
   three log modes, caller weights and the design, non-finite samples, a silent frame and a +-1.5 overload: every row entry must agree;
 * the same input through a build with -fsanitize=address,undefined (a plain host program, nothing preloaded);
 * the table: no product within 1e-6 of a half-integer, the C++ table equal to the Python one entry for entry, the kernel's image of
   it the two digit planes (checked inside mel_check);
 * L, the rule's own logarithm, against math.log over a sweep, and mel.h's against the restatement bit for bit;
 * zv_mel_design against the formulas written out here, and its refusals by name;
 * the boundary: the three entry points are declared, exported and bound, and refuse NULL arguments by name; the batch plan;
 * the accuracy of the rule against the textbook (reflect-padded Hann STFT magnitude . Slaney weights in float64)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import mel_rule as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
NAMES = ("zv_mel_wave", "zv_mel_wave_batch", "zv_mel_design")
F = np.float32
SR = 22050
SPECIALS = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000], np.uint32).view(F)


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "mel_check.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mel_check")
    return _build(tmp, "mel_check", []), _build(tmp, "mel_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _fbits(x):
    return "%x" % int(np.array([x], F).view(np.uint32)[0])


# ---- the design, written out ------------------------------------------------------------------------------------------------------

def _hz_to_mel(f):
    return 3.0 * f / 200.0 if f < 1000.0 else 15.0 + 27.0 * math.log(f / 1000.0) / math.log(6.4)


def _mel_to_hz(m):
    return 200.0 * m / 3.0 if m < 15.0 else 1000.0 * math.exp(math.log(6.4) * (m - 15.0) / 27.0)


def _design(rate, M, fmin=0.0, fmax=0.0):
    """Slaney-scale triangles with Slaney area normalisation on the 513 bin centres, float64 [M, 513] (librosa.filters.mel's defaults)"""
    fmax = fmax or rate / 2.0
    m0, m1 = _hz_to_mel(fmin), _hz_to_mel(fmax)
    p = [_mel_to_hz(m0 + i * (m1 - m0) / (M + 1)) for i in range(M + 2)]
    f = np.arange(MR.BINS) * rate / MR.N
    W = np.zeros((M, MR.BINS))
    for c in range(M):
        up, down = (f - p[c]) / (p[c + 1] - p[c]), (p[c + 2] - f) / (p[c + 2] - p[c + 1])
        W[c] = np.maximum(0.0, np.minimum(up, down)) * (2.0 / (p[c + 2] - p[c]))
    return W


def _c_design(exe, rate, M, fmin=0.0, fmax=0.0):
    r = subprocess.run([exe, "design", str(rate), str(M), _fbits(fmin), _fbits(fmax)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    if r.stdout.startswith("refused"):
        return r.stdout.strip()
    return np.array([int(t, 16) for t in r.stdout.split()], np.uint32).view(F).reshape(M, MR.BINS)


# ---- cases ------------------------------------------------------------------------------------------------------------------------

def _speech(rng, total, amp=0.3):
    t = np.arange(total)
    f0 = rng.uniform(80, 300) / SR
    x = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 6)) / h for h in range(1, 12))
    return ((x * 0.3 + rng.standard_normal(total) * 0.05) * amp).astype(F)


def _weights(rng, M):
    """caller weights: sparse rows with negative entries, -0.0 and an all-zero row"""
    W = np.zeros((M, MR.BINS), F)
    for c in range(M):
        lo = int(rng.integers(0, MR.BINS - 1))
        hi = int(rng.integers(lo + 1, min(lo + 60, MR.BINS) + 1))
        W[c, lo:hi] = rng.standard_normal(hi - lo).astype(F)
        W[c, lo + (hi - lo) // 2] = 0.0
    W[0, 0], W[0, 512] = 1.0, 0.5
    W[1] = -0.0
    return W


def _case(name, T, hop, x, M=6, W=None, centre=0, pad=0, log=0, floor=0.0, fmin=0.0, fmax=0.0, rate=SR):
    x = np.asarray(x, F)
    assert x.shape == (T * hop,), name
    return dict(name=name, T=T, hop=hop, x=x, M=M, W=W, centre=centre, pad=pad, log=log, floor=floor, fmin=fmin, fmax=fmax, rate=rate)


def _cases(rng):
    c, i = [], 0
    for hop in (256, 300):
        for pad in (0, 1):
            for centre in (0, hop // 2):
                for log in (0, 1, 2):
                    W = _weights(rng, 6) if i % 2 else None
                    c.append(_case(f"hop {hop} pad {pad} centre {centre} log {log} {'caller' if i % 2 else 'design'}", 4, hop,
                                   _speech(rng, 4 * hop), W=W, centre=centre, pad=pad, log=log, fmin=(0.0, 60.0)[i % 3 == 0],
                                   fmax=(0.0, 8000.0)[i % 4 < 2], floor=(0.0, 1e-5, 3.0)[i % 3]))
                    i += 1
    for hop in (256, 300):
        x = _speech(rng, 5 * hop)
        x[rng.integers(0, x.size, 40)] = rng.choice(SPECIALS, 40)
        c.append(_case(f"hop {hop}: NaN, inf and -0.0 samples", 5, hop, x, pad=1, log=1))
        x = np.concatenate([_speech(rng, 2 * hop), np.zeros(1024 + 3 * hop, F), _speech(rng, 2 * hop)])
        T = x.size // hop
        c.append(_case(f"hop {hop}: silent frames between loud ones", T, hop, x[:T * hop], W=_weights(rng, 6)))
        c.append(_case(f"hop {hop}: silent frames, linear, a floor", T, hop, x[:T * hop], log=2, floor=0.25))
        x = _speech(rng, 4 * hop)
        x[hop + 7], x[2 * hop + 11] = 1.5, -1.5
        c.append(_case(f"hop {hop}: a +-1.5 overload", 4, hop, x, centre=hop // 2, pad=1))
        c.append(_case(f"hop {hop}: T = 1", 1, hop, _speech(rng, hop), centre=hop - 1))
    c += [_case("an all-zero waveform", 3, 300, np.zeros(900, F), log=0),
          _case("only NaN and inf", 2, 300, rng.choice(SPECIALS[:3], 600), log=1),
          _case("80 channels of the design", 3, 300, _speech(rng, 900), M=80, pad=1),
          _case("256 channels of the design", 2, 300, _speech(rng, 600), M=256),
          _case("a tiny signal: 1e-6", 3, 256, _speech(rng, 768, 1e-6), log=1),
          _case("a huge signal: 1e30", 3, 256, _speech(rng, 768, 1e30), log=2, W=_weights(rng, 6) * F(1e30))]
    return c


def _bad_weights():
    W = np.zeros((6, MR.BINS), F)
    W[3, 77] = np.inf
    return W


REFUSED = [("centre at the hop", dict(centre=300), "centre"), ("pad 2", dict(pad=2), "pad"), ("log 3", dict(log=3), "log"),
           ("reflect with fewer than 513 samples", dict(pad=1, T=1), "pad (T)"), ("a negative floor", dict(floor=-1.0), "floor"),
           ("a NaN floor", dict(floor=float("nan")), "floor"), ("a weight that is not finite", dict(W=_bad_weights()), "weights"),
           ("no channels", dict(M=0), "num_mels"), ("257 channels", dict(M=257), "num_mels"),
           ("fmin = fmax", dict(fmin=4000.0, fmax=4000.0), "fmin_hz"), ("fmin above Nyquist", dict(fmin=12000.0), "fmin_hz"),
           ("fmax above Nyquist", dict(fmax=11026.0), "fmax_hz"), ("fmin infinite", dict(fmin=float("inf")), "fmin_hz"),
           ("fmax NaN", dict(fmax=float("nan")), "fmax_hz"), ("fmin negative", dict(fmin=-1.0), "fmin_hz")]


def _stdin(cases):
    lines = []
    for c in cases:
        W = c["W"]
        lines.append(f"{c['T']} {c['hop']} {c['M']} {c['rate']} {c['centre']} {c['pad']} {c['log']} {_fbits(c['floor'])} {_fbits(c['fmin'])} "
                     f"{_fbits(c['fmax'])} {0 if W is None else W.size}")
        lines.append("" if W is None else " ".join("%x" % b for b in MR.bits(W).reshape(-1)))
        lines.append(" ".join("%x" % b for b in MR.bits(c["x"])))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def cases():
    return _cases(np.random.default_rng(20261021))


@pytest.fixture(scope="module")
def refused():
    out = []
    for name, kw, _ in REFUSED:
        kw = dict(kw)
        T = kw.pop("T", 2)
        out.append(_case(name, T, 300, np.zeros(T * 300, F), **kw))
    return out


@pytest.fixture(scope="module")
def outputs(exes, cases, refused):
    text = _stdin(cases + refused)
    return [subprocess.run([e], input=text, capture_output=True, text=True, timeout=900) for e in exes]


# ---- 1. header against restatement ------------------------------------------------------------------------------------------------

def test_header_equals_restatement_bit_for_bit(exes, cases, refused, outputs):
    r = outputs[0]
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(cases) + len(refused)
    designs = {}
    for c, line in zip(cases, got):
        W = c["W"]
        if W is None:                     # the design's own weights: test_design_equals_the_formulas holds them to the formulas
            key = (c["rate"], c["M"], c["fmin"], c["fmax"])
            if key not in designs:
                designs[key] = _c_design(exes[0], *key)
            W = designs[key]
        want = MR.rule(c["x"], c["T"], c["hop"], W, c["centre"], c["pad"], c["log"], c["floor"])
        have = np.array([int(t, 16) for t in line.split()], np.uint32).reshape(c["T"], c["M"])
        bad = np.argwhere(have != MR.bits(want))
        assert bad.size == 0, (c["name"], len(bad), bad[:4], have.view(F)[tuple(bad[0])], want[tuple(bad[0])])
    for (name, kw, field), line in zip(REFUSED, got[len(cases):]):
        assert line == f"refused {field}", name


def test_sanitized_build_agrees(outputs):
    assert outputs[1].returncode == 0 and outputs[1].stderr == "", outputs[1].stderr[-3000:]
    assert outputs[1].stdout == outputs[0].stdout


def test_silent_frames_read_the_floor(cases):
    c = next(c for c in cases if c["name"] == "hop 300: silent frames, linear, a floor")
    W = _design(SR, 6).astype(F)
    out = MR.rule(c["x"], c["T"], 300, W, log=2, floor=0.25)
    silent = [f for f in range(c["T"]) if not np.any(MR.spans(c["x"], c["T"], 300, 0, 0)[f])]
    assert silent and all((out[f] == F(0.25)).all() for f in silent)
    assert (MR.rule(np.zeros(900, F), 3, 300, W) == F(-10.0)).all() and MR.level(np.zeros(1), 0.0, 0)[0] == F(-10.0)


# ---- 2. the table -----------------------------------------------------------------------------------------------------------------

def test_table_has_no_ties_and_equals_the_c_table(exes, tmp_path):
    pc, ps = MR.products()
    for p in (pc, ps):
        frac = np.abs(p + 0.5 - np.round(p + 0.5))       # the distance of p from the nearest half-integer
        assert frac.min() >= 1e-6, frac.min()
    C_, S_ = MR.tables()
    assert max(np.abs(C_).max(), np.abs(S_).max()) <= MR.SCALE
    for t in (C_, S_):
        hi, lo = MR.digits(t)
        assert (128 * hi + lo == t).all() and np.abs(hi).max() <= 64 and np.abs(lo).max() <= 64
    path = str(tmp_path / "tables.i16")
    for exe in exes:
        r = subprocess.run([exe, "table", path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        tab = np.fromfile(path, "<i2").reshape(2, MR.BINS, MR.N)
        assert np.array_equal(tab[0], C_) and np.array_equal(tab[1], S_)


# ---- 3. the logarithm -------------------------------------------------------------------------------------------------------------

def _sweep():
    rng = np.random.default_rng(5)
    v = np.concatenate([10.0 ** rng.uniform(-300, 300, 4000), 10.0 ** rng.uniform(-12, 3, 4000), 1.0 + rng.uniform(-1e-3, 1e-3, 500),
                        np.sqrt(0.5) * 2.0 ** rng.integers(-40, 40, 500) * (1.0 + rng.uniform(-1e-9, 1e-9, 500)),
                        [1.0, 2.0, 0.5, 1e-10, float(MR.FLOOR), np.nextafter(1.0, 0), np.nextafter(1.0, 2), 2.2250738585072014e-308,
                         1.7976931348623157e308, MR.SQRT_HALF, np.nextafter(MR.SQRT_HALF, 0)]])
    return v.astype(np.float64)


def test_the_rules_logarithm_is_within_1e_11_of_libm():
    v = _sweep()
    got = MR.ln(v)
    want = np.array([math.log(x) for x in v])
    assert np.abs(got - want).max() <= 1e-11, np.abs(got - want).max()
    assert MR.ln(np.array([1.0]))[0] == 0.0


def test_header_logarithm_equals_restatement(exes):
    v = _sweep()
    text = "\n".join("%x" % b for b in v.view(np.uint64)) + "\n"
    for exe in exes:
        r = subprocess.run([exe, "ln"], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        have = np.array([int(t, 16) for t in r.stdout.split()], np.uint64)
        assert np.array_equal(have, MR.ln(v).view(np.uint64))


# ---- 4. the design ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate,M,fmin,fmax", [(22050, 80, 0.0, 0.0), (22050, 80, 0.0, 8000.0), (24000, 100, 55.0, 7600.0), (16000, 1, 0.0, 0.0),
                                               (44100, 256, 20.0, 0.0), (22050, 6, 60.0, 8000.0)])
def test_design_equals_the_formulas(exes, rate, M, fmin, fmax):
    """The filter points come from libm's log and exp, which differ between libraries by an ulp or two of f64: about 1e-11 Hz at the
    top of the band.  A ramp divides that by at least the narrowest filter's width (10 Hz or more here) and multiplies by the
    normalisation (below 0.1): 1e-13 absolute; the rounding to f32 then moves a weight by at most one ulp of f32."""
    have, want = _c_design(exes[0], rate, M, fmin, fmax), _design(rate, M, fmin, fmax)
    assert have.shape == want.shape and have.dtype == F
    assert (np.abs(have.astype(np.float64) - want) <= np.abs(want) * 2.0 ** -23 + 1e-13).all()
    assert ((have == 0) == (want.astype(F) == 0)).mean() > 0.999
    if M > 1 and not fmin and not fmax:
        assert (have.sum(axis=1) > 0).all()


def test_design_through_the_library_and_its_refusals(exes):
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    W = capi.mel_design(22050, 80, 0.0, 8000.0, lib=lib)
    assert W.shape == (80, 513) and np.array_equal(MR.bits(W), MR.bits(_c_design(exes[0], 22050, 80, 0.0, 8000.0)))
    assert np.array_equal(MR.bits(capi.mel_design(22050, 80)), MR.bits(capi.mel_design(22050, 80, 0.0, 11025.0)))
    for args, word in (((22050, 0), "num_mels"), ((22050, 257), "num_mels"), ((22050, 80, 4000.0, 4000.0), "fmin_hz"),
                       ((22050, 80, 5000.0, 4000.0), "fmin_hz"), ((22050, 80, 0.0, 11026.0), "fmax_hz"), ((22050, 80, float("nan")), "fmin_hz"),
                       ((22050, 80, 0.0, float("inf")), "fmax_hz"), ((0, 80), "sampling_rate")):
        with pytest.raises(capi.ZvError) as e:
            capi.mel_design(*args, lib=lib)
        assert e.value.status == 5 and "zv_mel_design" in str(e.value) and word in str(e.value), (args, str(e.value))
    assert lib.zv_mel_design(22050, 80, 0.0, 0.0, None) == 5 and b"zv_mel_design: weights is NULL" in lib.zv_last_error()


# ---- 5. the boundary --------------------------------------------------------------------------------------------------------------

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
    assert _declaration(header, "zv_mel_wave") == ["zv_model*", "const float*", "uint32_t", "const zv_mel*", "float*"]
    assert _declaration(header, "zv_mel_wave_batch") == ["zv_model*", "uint32_t", "const float*const*", "const uint32_t*", "const zv_mel*", "float*const*"]
    assert _declaration(header, "zv_mel_design") == ["uint32_t", "uint32_t", "float", "float", "float*"]
    vp, u32 = C.c_void_p, C.c_uint32
    assert lib.zv_mel_wave.argtypes == [vp, vp, u32, C.POINTER(capi.MelC), vp]
    assert lib.zv_mel_wave_batch.argtypes == [vp, u32, C.POINTER(vp), C.POINTER(u32), C.POINTER(capi.MelC), C.POINTER(vp)]
    assert lib.zv_mel_design.argtypes == [u32, u32, C.c_float, C.c_float, vp]
    assert C.sizeof(capi.MelC) == 32 and bytes(capi.MelC()) == bytes(32)          # zero-initialised = the defaults
    assert re.search(r"typedef struct\s*\{\s*const float \*weights;\s*float\s+fmin_hz, fmax_hz;\s*uint32_t\s+centre, pad, log;\s*float\s+floor;\s*\}\s*zv_mel;", header)
    # the kernels take every non-integer step from mel.h and bands.h and sum the matrix products on the i8 MFMA
    kernels = re.sub(r"//.*", "", open(os.path.join(CSRC, "mel_kernels.hip")).read())
    for fn in ("mel_span", "mel_sample_index", "bands_exponent", "bands_quant", "bands_digits", "mel_combine", "mel_magnitude", "mel_channel",
               "mel_level", "mel_plan", "__builtin_amdgcn_mfma_i32_16x16x64_i8"):
        assert fn + "(" in kernels, fn
    assert not re.search(r"\b(sqrt|sqrtf|log|logf|log10|log10f|log2|exp)\s*\(", kernels)
    header_h = open(os.path.join(CSRC, "mel.h")).read()
    assert "bands_quant(" in header_h and not re.search(r"\bmel_quant\b", header_h)      # the quantiser is the band levels', not a copy
    s = capi.MelAnalysis(np.zeros((80, 513), F), 50.0, 7000.0, 150, "reflect", "ln", 1e-5).struct
    assert (s.fmin_hz, s.fmax_hz, s.centre, s.pad, s.log) == (50.0, 7000.0, 150, 1, 1) and s.weights
    for bad in (dict(pad="mirror"), dict(log="db"), dict(weights=np.zeros((80, 512), F))):
        with pytest.raises(ValueError):
            capi.MelAnalysis(**bad)


def test_null_arguments_are_refused_by_name():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    wav, out, mel = np.zeros(8 * 300, F), np.zeros((8, 80), F), capi.MelC()
    handle = C.c_void_p(wav.ctypes.data)                      # never dereferenced: the argument checks come first
    assert lib.zv_mel_wave(None, wav.ctypes.data, 8, C.byref(mel), out.ctypes.data) == 5
    assert b"zv_mel_wave: m is NULL" in lib.zv_last_error()
    assert lib.zv_mel_wave(handle, None, 8, C.byref(mel), out.ctypes.data) == 5 and b"zv_mel_wave: wav is NULL" in lib.zv_last_error()
    assert lib.zv_mel_wave(handle, wav.ctypes.data, 8, C.byref(mel), None) == 5 and b"zv_mel_wave: out is NULL" in lib.zv_last_error()
    P, Ts = C.c_void_p * 1, (C.c_uint32 * 1)(8)
    assert lib.zv_mel_wave_batch(None, 1, P(wav.ctypes.data), Ts, C.byref(mel), P(out.ctypes.data)) == 5
    assert b"zv_mel_wave_batch: m is NULL" in lib.zv_last_error()
    for args, what in (((handle, 1, None, Ts, C.byref(mel), P(out.ctypes.data)), b"wav is NULL"),
                       ((handle, 1, P(wav.ctypes.data), Ts, C.byref(mel), None), b"out is NULL"),
                       ((handle, 1, P(wav.ctypes.data), None, C.byref(mel), P(out.ctypes.data)), b"T is NULL"),
                       ((handle, 0, P(wav.ctypes.data), Ts, C.byref(mel), P(out.ctypes.data)), b"n_utt must be > 0")):
        assert lib.zv_mel_wave_batch(*args) == 5
        assert b"zv_mel_wave_batch: " + what in lib.zv_last_error(), lib.zv_last_error()


def test_batch_plan_is_one_launch_per_kernel(exes):
    """stage_plan.h mel_plan: grid (tiles, segments) for both kernels whatever the batch; hops that are no multiple of 4 and channel
    counts outside 1 .. 256 are refused"""
    tile = MR.tile_frames()
    assert tile == 32
    rows = [(1, 1, 300, 80), (tile, 1, 300, 80), (tile + 1, 1, 256, 80), (1024, 32, 300, 80), (2 * tile + 3, 3, 300, 256), (5, 2, 4, 1),
            (8, 1, 302, 80), (8, 1, 2, 80), (8, 1, 300, 0), (8, 1, 300, 257), (0, 1, 300, 80), (8, 0, 300, 80)]
    text = "".join("%d %d %d %d\n" % r for r in rows)
    r = subprocess.run([exes[0], "plan"], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = [tuple(map(int, line.split())) for line in r.stdout.splitlines()]
    want = [(int(i < 6), -(-t // tile), -(-t // 4), n) for i, (t, n, _, _) in enumerate(rows)]
    assert got == want


def test_cli_knows_its_flags_and_refuses_bad_files(tmp_path):
    """usage errors exit 2 before anything is loaded; a file that is not mono PCM16 is refused by name ahead of the checkpoint"""
    import wave
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    run = lambda *a: subprocess.run([cli, *a], capture_output=True, text=True, timeout=60)
    for flag in ("--analyze", "--mel-out", "--resynth", "--mel-fmin", "--mel-fmax", "--mel-centre", "--mel-pad"):
        assert flag in run("--help").stdout, flag
    for args, word in ((("--analyze", "a.wav", "--mel-out", "r.f32", "--mel-pad", "mirror"), "--mel-pad"), (("--mel-out", "r.f32"), "need --analyze"),
                       (("--mel-fmin", "50"), "need --analyze"), (("--analyze", "a.wav"), "--analyze needs"),
                       (("--analyze", "a.wav", "--mel-out", "r.f32", "--mel-centre", "-3"), "--mel-centre"),
                       (("--analyze", "a.wav", "--mel-out", "r.f32", "--mel-fmax", "x"), "--mel-fmax")):
        r = run(*args)
        assert r.returncode == 2 and word in r.stderr, (args, r.stderr[:300])
    stereo, text = str(tmp_path / "stereo.wav"), str(tmp_path / "text.wav")
    with wave.open(stereo, "wb") as w:
        w.setnchannels(2), w.setsampwidth(2), w.setframerate(SR)
        w.writeframes(bytes(4 * 600))
    open(text, "w").write("not a wave file at all")
    for path, word in ((stereo, "2 channels"), (text, "not a RIFF/WAVE file"), (str(tmp_path / "missing.wav"), "cannot open")):
        r = run("--analyze", path, "--mel-out", str(tmp_path / "rows.f32"))
        assert r.returncode == 1 and "--analyze" in r.stderr and word in r.stderr, (path, r.stderr[:300])


# ---- 6. the accuracy of the rule --------------------------------------------------------------------------------------------------

ACC_HOP, ACC_T, ACC_M = 256, 48, 80
# measured with this file (both sides are deterministic), rounded up to the next dB and the next 1e-3; profiles/mel_accuracy.txt
ACC_BOUNDS = {"speech": (-81.0, 3e-3), "tones": (-94.0, 4e-3)}      # measured: -81.35 dB, 2.146e-3; -94.86 dB, 3.320e-3


def _acc_signals():
    rng = np.random.default_rng(20261021)
    n = ACC_T * ACC_HOP
    t = np.arange(n)
    f0 = 137.0 / SR
    x = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 6)) / h ** 1.2 for h in range(1, 60)) * 0.08 + rng.standard_normal(n) * 0.003
    x[n // 3:n // 3 + 6 * ACC_HOP] *= 0.01                          # a passage 40 dB down
    x[2 * n // 3:2 * n // 3 + 7 * ACC_HOP] = 0.0                     # a run of zeros: two silent frames and the edges around them
    tones = sum(a * np.sin(2 * np.pi * f / SR * t + p) for a, f, p in ((0.5, 440.0, 0.3), (0.5 * 10 ** (-54 / 20), 2793.0, 1.1),
                                                                       (0.5 * 10 ** (-108 / 20), 6271.0, 2.0)))
    return dict(speech=x.astype(F), tones=tones.astype(F))


def _textbook(x, W):
    """reflect-padded Hann STFT magnitude . Slaney weights, float64 (librosa's center=True, window 'hann' periodic, power 1)"""
    xp = np.pad(x.astype(np.float64), MR.N // 2, mode="reflect")
    frames = np.stack([xp[f * ACC_HOP:f * ACC_HOP + MR.N] for f in range(ACC_T)]) * MR.window()[None, :]
    return np.abs(np.fft.rfft(frames, axis=1)) @ W.T


def accuracy():
    """{signal: (the largest error relative to the frame's strongest channel in dB, the largest |delta log10| within 60 dB of it)}"""
    W = _design(SR, ACC_M)
    out = {}
    for name, x in _acc_signals().items():
        want = _textbook(x, W)
        lin = MR.rule(x, ACC_T, ACC_HOP, W.astype(F), 0, 1, 2, 0.0).astype(np.float64)
        lg = MR.rule(x, ACC_T, ACC_HOP, W.astype(F), 0, 1, 0, 0.0).astype(np.float64)
        top = want.max(axis=1)
        live = top > 1e-9
        assert live.sum() >= ACC_T - 8
        rel = np.abs(np.where(want > 1e-10, lin, want) - want)[live] / top[live, None]      # (below the floor the rule reads the floor)
        near = want[live] >= top[live, None] * 1e-3
        dlog = np.abs(lg[live] - np.log10(np.maximum(want[live], 1e-10)))[near]
        out[name] = (20.0 * math.log10(rel.max()), float(dlog.max()))
    return out


def test_accuracy_against_the_textbook():
    """The measured figures (profiles/mel_accuracy.txt): see ACC_BOUNDS; the speech-like signal must stay below -75 dB."""
    got = accuracy()
    for name, (db, dlog) in got.items():
        print(f"mel accuracy, {name}: {db:.2f} dB re the frame's strongest channel, |delta log10| <= {dlog:.3e} within 60 dB")
    for name, (db, dlog) in got.items():
        assert db <= ACC_BOUNDS[name][0] and dlog <= ACC_BOUNDS[name][1], (name, db, dlog)
    assert ACC_BOUNDS["speech"][0] <= -75


if __name__ == "__main__":
    for k, (db, dlog) in accuracy().items():
        print(f"{k}: {db:.2f} dB re the frame's strongest channel; |delta log10| <= {dlog:.3e} within 60 dB of it")
