"""Band levels (include/zerovox_amd.h "band levels") on the CPU: csrc/bands.h against its restatement in exact integers and single
float64 steps (tests/bands_rule.py), bit for bit.
 * tests/native/bands_check.cpp drives zv::bands_resolve and zv::bands_reference over the named edge classes and random small cases:
   the resolved edges, every frame's row and kept powers and every phoneme's row must agree;
 * the same input through a build with -fsanitize=address,undefined (a plain host program, nothing preloaded);
 * the table: no product within 1e-6 of a half-integer, the C++ table equal to the Python one entry for entry, the kernel's image of
   it a permutation (checked inside bands_check);
 * the fidelity of the rule itself: sines read A / sqrt(2), far bands stay 48 dB below, white noise agrees with a float64 Hann FFT;
 * the bounds: |Re|, |Im| < 2^29 and S_b < 2^63 for the full-scale square waves that maximise every bin;
 * the boundary: the four entry points are declared, exported and bound, refuse a NULL model by name, zv_band_levels refuses a phoneme
   table, the binding refuses a bad return_bands before it touches a device, _call_variant routes a bands request and nothing else to
   the _bands symbol, and the CLI knows its flags and refuses bad edges."""
import ctypes as C
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

import bands_rule as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
CLI = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
NAMES = ("zv_synthesize_bands", "zv_synthesize_batch_bands", "zv_synthesize_batch_begin_bands", "zv_band_levels")
F = np.float32
SR = 22050
SPECIALS = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x7f7fffff], np.uint32).view(F)
SINGLE = list(range(100, 165))                   # 64 bands of one bin each


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "bands_check.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bands_check")
    return _build(tmp, "bands_check", []), _build(tmp, "bands_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# ---- cases ------------------------------------------------------------------------------------------------------------------

def _speech(rng, total, amp=0.3):
    """speech-like: a few harmonics of a drifting fundamental under an envelope, and some noise"""
    t = np.arange(total)
    f0 = rng.uniform(80, 300) / SR
    x = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 6)) / h for h in range(1, 12))
    env = 0.5 + 0.5 * np.sin(2 * np.pi * t / max(total, 1) * rng.uniform(0.5, 3))
    return ((x * env * 0.3 + rng.standard_normal(total) * 0.05) * amp).astype(F)


def _case(name, T, hop, x, dur=(), n_bands=0, edges=None):
    x = np.asarray(x, F)
    assert x.shape == (T * hop,), name
    return dict(name=name, T=T, hop=hop, dur=[int(d) for d in dur], x=x, n_bands=n_bands, edges=None if edges is None else [int(e) for e in edges])


def _named(rng):
    sp = lambda T, hop, amp=0.3: _speech(rng, T * hop, amp)
    tone = lambda total, P, amp=0.4: (np.sin(2 * np.pi * np.arange(total) / P) * amp).astype(F)
    c = [_case(f"T = {T}: shorter than the window", T, 300, sp(T, 300), [T]) for T in (1, 2, 3, 4)]
    c += [_case("defaults at hop 300", 6, 300, sp(6, 300), [1, 0, 3, 2]),
          _case("n_bands = 16 with the default edges", 3, 300, sp(3, 300), [3], n_bands=16),
          _case("64 bands of one bin", 4, 300, sp(4, 300), [2, 2], edges=SINGLE),
          _case("one band [0, 513)", 4, 300, sp(4, 300), [4], edges=[0, 513]),
          _case("one band of one bin at 0", 3, 300, sp(3, 300) + F(0.2), [3], edges=[0, 1]),
          _case("one band of one bin at 512", 6, 300, np.tile(np.array([0.5, -0.5], F), 900), [6], edges=[512, 513]),
          _case("64 bands over everything", 3, 300, sp(3, 300), [1, 2], edges=list(range(0, 512, 8)) + [513]),
          _case("an all-zero waveform", 3, 300, np.zeros(900, F), [1, 2]),
          _case("all -0.0", 2, 300, np.full(600, -0.0, F), [2]),
          _case("a peak just below 2^-24", 4, 300, tone(1200, 12, 1.0) * F(2.0 ** -25) * F(1.9999), [4]),
          _case("a peak just at 2^-24", 4, 300, np.where(np.arange(1200) % 12 == 0, F(2.0 ** -24), F(2.0 ** -26)), [4]),
          _case("NaN, inf and -0.0 samples", 4, 300, np.where(rng.random(1200) < 0.1, rng.choice(SPECIALS[:4], 1200), tone(1200, 14)), [4]),
          _case("only NaN and inf", 2, 300, rng.choice(SPECIALS[:3], 600), [2]),
          _case("subnormal samples next to large ones", 3, 300, np.where(np.arange(900) % 2 == 0, F(1e-42), tone(900, 15)), [3]),
          _case("only subnormal samples", 2, 300, np.full(600, 1e-40, F), [2]),
          _case("samples at 1e30", 3, 300, np.where(np.arange(900) % 15 == 0, F(1e30), tone(900, 15)), [3]),
          _case("the largest finite samples", 2, 300, np.where(np.arange(600) % 2 == 0, SPECIALS[5], -SPECIALS[5]), [2]),
          _case("a constant at the quantiser's ceiling: hi = 64", 6, 300, np.full(1800, F(8191.0 / 8192.0), F), [6], edges=[0, 1, 2, 513]),
          _case("negative samples: the floor split", 4, 300, -np.abs(sp(4, 300)), [4]),
          _case("fitted zeros behind the speech", 8, 300, np.concatenate([sp(3, 300), np.zeros(1500, F)]), [3]),
          _case("phonemes of 0 frames between others", 8, 300, sp(8, 300), [3, 0, 0, 2, 0, 3, 0]),
          _case("a phoneme cut off by T", 6, 300, sp(6, 300), [2, 7, 0]),
          _case("no phonemes", 2, 300, sp(2, 300), []),
          _case("loud: the kept power saturates", 3, 300, sp(3, 300, 3000.0), [3], edges=[1, 513])]
    for hop in (4, 7, 64, 1024, 1500):
        T = 40 if hop <= 7 else 4 if hop <= 64 else 2
        c.append(_case(f"hop = {hop}", T, hop, sp(T, hop), [T // 2, 0, T - T // 2]))
    return c


REFUSED = [("n_bands above 64", dict(n_bands=65, edges=list(range(66))), "n_bands"),
           ("edges not ascending", dict(edges=[1, 5, 5, 9]), "edges"), ("edges descending", dict(edges=[9, 5]), "edges"),
           ("the last edge above 513", dict(edges=[1, 100, 514]), "edges"),
           ("NULL edges with n_bands 5", dict(n_bands=5), "edges"), ("NULL edges with n_bands 64", dict(n_bands=64), "edges")]


def _random(rng, count):
    c = []
    for k in range(count):
        hop = int(rng.choice([4, 40, 300]))
        T = int(rng.integers(1, 5))
        n = int(rng.integers(0, 4))
        cuts = np.sort(rng.integers(0, T + 1, size=n))
        dur = np.diff(np.concatenate([[0], cuts])).tolist()
        total = T * hop
        kind = k % 4
        if kind == 0:
            x = rng.standard_normal(total) * 10.0 ** int(rng.integers(-9, 3))
        elif kind == 1:
            x = _speech(rng, total, rng.uniform(0.01, 2))
        elif kind == 2:
            x = np.round(rng.standard_normal(total) * 2) / 4
        else:
            x = rng.standard_normal(total) * 0.2
            x[rng.random(total) < 0.3] = 0
        x = np.asarray(x, F)
        if rng.random() < 0.2:
            at = rng.integers(0, total, size=min(total, 6))
            x[at] = SPECIALS[:len(at)]
        edges = None
        if k % 3:
            nb = int(rng.integers(1, 9))
            edges = np.sort(rng.choice(BR.BINS + 1, size=nb + 1, replace=False)).tolist()
        c.append(_case(f"random {k}", T, hop, x, dur, edges=edges))
    return c


def _stdin(cases):
    lines = []
    for c in cases:
        e = c["edges"] or []
        lines.append(f"{c['T']} {c['hop']} {len(c['dur'])} {c['n_bands']} {len(e)}")
        lines.append(" ".join(map(str, e)))
        lines.append(" ".join(map(str, c["dur"])))
        lines.append(" ".join("%x" % b for b in BR.bits(c["x"])))
    return "\n".join(lines) + "\n"


def _n_bands(c):
    return c["n_bands"] or (len(c["edges"]) - 1 if c["edges"] else 0)


def _rule(c):
    return BR.rule(c["x"], c["T"], c["hop"], c["dur"], _n_bands(c), c["edges"])


def _expect(c):
    r = _rule(c)
    fb, pb = BR.bits(r["frames"]), BR.bits(r["phonemes"])
    line = " ".join(map(str, [r["n_bands"]] + r["edges"])) + " |"
    line += "".join(f" {fb[f, b]:x}:{r['Eq'][f][b]}" for f in range(c["T"]) for b in range(r["n_bands"])) + " |"
    return line + "".join(f" {v:x}" for v in pb.reshape(-1))


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(20261021)
    return _named(rng) + _random(rng, 60)


@pytest.fixture(scope="module")
def refused():
    return [_case(name, 1, 40, np.zeros(40, F), [], **kw) for name, kw, _ in REFUSED]


def _send(c):
    """what bands_check receives: n_bands as the caller would set it, with explicit edges the count they imply"""
    return dict(c, n_bands=c["n_bands"] or (len(c["edges"]) - 1 if c["edges"] else 0))


@pytest.fixture(scope="module")
def outputs(exes, cases, refused):
    text = _stdin([_send(c) for c in cases + refused])
    return [subprocess.run([e], input=text, capture_output=True, text=True, timeout=900) for e in exes]


# ---- 1. header against restatement --------------------------------------------------------------------------------------------

def test_header_equals_restatement_bit_for_bit(cases, refused, outputs):
    r = outputs[0]
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(cases) + len(refused)
    for c, line in zip(cases, got):
        assert line == _expect(c), c["name"]
    for (name, kw, field), c, line in zip(REFUSED, refused, got[len(cases):]):
        assert line == f"refused {field}", name
        with pytest.raises(ValueError, match=field):
            BR.resolve(c["n_bands"], c["edges"])


def test_sanitized_build_agrees_and_is_silent(outputs):
    plain, san = outputs
    assert san.returncode == 0 and san.stderr == "", san.stderr[-3000:]
    assert san.stdout == plain.stdout


def test_the_named_cases_reach_what_they_name(cases):
    by = {c["name"]: c for c in cases}
    rows = lambda name: _rule(by[name])
    zero = lambda a: not BR.bits(a).any()
    for name in ("an all-zero waveform", "all -0.0", "only NaN and inf", "a peak just below 2^-24", "only subnormal samples"):
        assert zero(rows(name)["frames"]) and zero(rows(name)["phonemes"]), name
    assert rows("a peak just at 2^-24")["frames"][1].any()
    r = rows("fitted zeros behind the speech")
    assert r["frames"][0].all() and zero(r["frames"][6:]) and r["phonemes"][0].all()
    r = rows("phonemes of 0 frames between others")
    assert zero(r["phonemes"][[1, 2, 4, 6]]) and r["phonemes"][[0, 3, 5]].all()
    assert rows("no phonemes")["phonemes"].shape == (0, 16)
    r = rows("loud: the kept power saturates")
    assert max(max(e) for e in r["Eq"]) == BR.EQ_MAX and r["frames"].max() > 22
    # the ceiling: every sample quantises to 8 191, whose digits are hi = 64, lo = -1.  Bin 0 alone holds 512^2 / (512 * 384) = 4/3 of
    # the constant's square (the window's sum squared over N / 2 times its sum of squares), and the window's side lobes fall off
    c = by["a constant at the quantiser's ceiling: hi = 64"]
    a, k = BR.quantise(BR.spans(c["x"], 6, 300)[2])                  # (frame 2's span [238, 1262) lies inside the waveform)
    assert k == 13 and (a == 8191).all()
    r = rows(c["name"])
    assert abs(float(r["frames"][2, 0]) / (math.sqrt(4 / 3) * 8191.0 / 8192.0) - 1) < 2e-3 and r["frames"][2, 2] < 1e-2 * r["frames"][2, 0]
    assert (BR.quantise(BR.spans(by["negative samples: the floor split"]["x"], 4, 300)[2])[0] <= 0).all()
    r = rows("one band of one bin at 512")
    assert abs(float(r["frames"][2, 0]) / (math.sqrt(4 / 3) * 0.5) - 1) < 2e-3      # the Nyquist bin is counted like bin 0
    for T in (1, 2, 3, 4):
        assert rows(f"T = {T}: shorter than the window")["frames"].all()


# ---- 2. the table -----------------------------------------------------------------------------------------------------------------

def test_no_table_product_is_near_a_tie():
    worst = min(float(np.abs(p - np.floor(p) - 0.5).min()) for p in BR.products())
    print(f"closest product to a half-integer: {worst:.3e}")
    assert worst > 1e-6
    C_, S_ = BR.tables()
    assert max(np.abs(C_).max(), np.abs(S_).max()) <= 126
    assert max(int(np.abs(C_).sum(axis=1).max()), int(np.abs(S_).sum(axis=1).max())) <= 64512
    assert int((np.floor(BR.SCALE * BR.window() + 0.5).astype(np.int64) ** 2).sum()) * 8 == int(BR.NORM) == 8 * 6096866


def test_cpp_table_equals_python_table(exes, tmp_path):
    out = tmp_path / "table.bin"
    for exe in exes:
        r = subprocess.run([exe, "table", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        got = np.fromfile(out, np.int8).reshape(2, BR.BINS, BR.N)
        C_, S_ = BR.tables()
        assert np.array_equal(got[0], C_) and np.array_equal(got[1], S_)
        # the margins the rule relies on, on the C++ table itself: entries fit i8 with room, rows of |C| and |S| sum to at most 64 512
        # (so |Re|, |Im| <= 8191 * 64512 < 2^29), and row 0 of C is the rounded window, whose squares give the norm 8 * W2
        g64 = got.astype(np.int64)
        assert int(np.abs(g64).max()) <= 126 and int(np.abs(g64).sum(axis=2).max()) <= 64512 and 8191 * 64512 < 1 << 29
        assert 8 * int((g64[0, 0] ** 2).sum()) == int(BR.NORM) and not g64[1, 0].any()


# ---- 3. the fidelity of the rule ----------------------------------------------------------------------------------------------------

AMPS = (0.01, 0.5, 0.9)
TONES = (70, 100, 150, 333.3, 1000, 2500, 5000, 9000, 10500)


@pytest.fixture(scope="module")
def sines():
    """frame 4 (its span [838, 1862) lies inside the waveform) of every sine, as the single band [1, 513) and as the default bands"""
    T, hop = 8, 300
    t = np.arange(T * hop)
    out = {}
    for A in AMPS:
        for hz in TONES:
            x = (A * np.sin(2 * np.pi * hz * t / SR + 0.3)).astype(F)
            a, k = BR.quantise(BR.spans(x, T, hop)[4])
            re, im = BR.sums(a)
            q = [(int(r) * int(r) + int(i) * int(i)) >> 6 for r, i in zip(re, im)]
            one = float(BR.band_row(sum(q[1:513]), k)[0])
            e = BR.DEFAULT_EDGES
            out[A, hz] = one, [float(BR.band_row(sum(q[e[b]:e[b + 1]]), k)[0]) for b in range(16)]
    return out


def test_a_sine_reads_its_rms(sines):
    worst = 0.0
    for (A, hz), (one, _) in sines.items():
        err = abs(one / (A / math.sqrt(2)) - 1)
        worst = max(worst, err)
        assert err < 1e-3, (A, hz, one)
    print(f"single band [1, 513): worst relative error to A / sqrt(2): {worst:.3e}")


def test_bands_far_from_a_tone_stay_48_db_below_it(sines):
    worst = -1e9
    for (A, hz), (_, bands) in sines.items():
        k0 = hz * BR.N / SR
        for b in range(16):
            lo, hi = BR.DEFAULT_EDGES[b], BR.DEFAULT_EDGES[b + 1] - 1
            if lo - k0 > 8 or k0 - hi > 8:
                db = 20 * math.log10(max(bands[b], 1e-30) / (A / math.sqrt(2)))
                worst = max(worst, db)
                assert db <= -48.0, (A, hz, b, db)
    print(f"bands wholly more than 8 bins from the tone: at most {worst:.1f} dB re A / sqrt(2)")


def test_white_noise_agrees_with_a_float64_hann_fft():
    rng = np.random.default_rng(11)
    T, hop = 12, 300
    x = (rng.standard_normal(T * hop) * 0.3).astype(F)
    r = BR.rule(x, T, hop)
    wnd = BR.window()
    worst = 0.0
    for f in range(3, 9):                                             # spans inside the waveform
        X = np.fft.rfft(BR.spans(x, T, hop)[f].astype(np.float64) * wnd)
        p = np.abs(X) ** 2
        for b in range(16):
            ref = math.sqrt(p[BR.DEFAULT_EDGES[b]:BR.DEFAULT_EDGES[b + 1]].sum() / (512.0 * (wnd ** 2).sum()))
            err = abs(float(r["frames"][f, b]) / ref - 1)
            worst = max(worst, err)
            assert err < 1e-2, (f, b, float(r["frames"][f, b]), ref)
    print(f"white noise, 16 default bands: worst relative error to the float64 FFT: {worst:.3e}")


def test_power_of_two_scaling_scales_every_row_exactly(cases):
    n = 0
    for c in cases[::5]:
        x = c["x"]
        if not np.isfinite(x).all() or c["name"].startswith("loud"):
            continue
        base = _rule(c)
        for s in (0.25, 64.0):
            with np.errstate(over="ignore"):
                y = x * F(s)
            ay = np.abs(y[y != 0])
            if ay.size and (ay.min() < 2.0 ** -126 or not np.isfinite(y).all()):
                continue
            r = BR.rule(y, c["T"], c["hop"], c["dur"], _n_bands(c), c["edges"])
            small, large = (r, base) if s < 1 else (base, r)
            fell = [f for f in range(c["T"]) if not BR.bits(small["frames"][f]).any() and BR.bits(large["frames"][f]).any()]
            for f in range(c["T"]):
                want = base["frames"][f].astype(np.float64) * s
                if (want > 3e38).any() or ((want != 0) & (want < 2.0 ** -126)).any():
                    continue                                        # a row left the f32 range: outside the promise
                assert f in fell or np.array_equal(BR.bits(r["frames"][f]), BR.bits(base["frames"][f] * F(s))), (c["name"], s, f)
            n += not fell
    assert n > 10


# ---- 4. the bounds ------------------------------------------------------------------------------------------------------------------

def test_sums_stay_inside_their_bounds_for_the_worst_square_waves():
    """a[t] = 8191 * sign(C[k][t]) maximises Re(k), likewise S and Im(k): full-scale square waves at every bin's frequency (times the
    window's sign, which is +).  One band [0, 513) takes every bin's power."""
    C_, S_ = BR.tables()
    worst_r = worst_s = 0
    for tab in (C_, S_):
        A = np.where(tab >= 0, 8191, -8191).astype(np.float64)           # [513 square waves, 1024]
        Re = (A @ C_.T.astype(np.float64)).astype(np.int64)
        Im = (A @ S_.T.astype(np.float64)).astype(np.int64)
        worst_r = max(worst_r, int(np.abs(Re).max()), int(np.abs(Im).max()))
        for j in range(BR.BINS):
            Sb = sum((int(r) * int(r) + int(i) * int(i)) >> 6 for r, i in zip(Re[j], Im[j]))
            worst_s = max(worst_s, Sb)
    print(f"largest |Re|, |Im|: {worst_r} = 2^{math.log2(worst_r):.2f}; largest S_b: 2^{math.log2(worst_s):.2f}")
    assert worst_r < 1 << 29 and worst_s < 1 << 63
    assert worst_r == 8191 * max(int(np.abs(C_).sum(axis=1).max()), int(np.abs(S_).sum(axis=1).max()))


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
    for name in ("zv_synthesize", "zv_synthesize_batch", "zv_synthesize_batch_begin"):
        assert _declaration(header, name + "_bands") == _declaration(header, name + "_pitch") + ["const zv_bands*"], name
        assert getattr(lib, name + "_bands").argtypes == getattr(lib, name + "_pitch").argtypes + [C.POINTER(capi.BandsC)]
    assert _declaration(header, "zv_band_levels") == ["zv_model*", "const float*", "uint32_t", "const zv_bands*"]
    assert not re.search(r"\bzv_synthesize_batch_end_bands\b", header)             # the existing _end finishes a bands batch
    assert C.sizeof(capi.BandsC) == 32 and bytes(capi.BandsC()) == bytes(32)        # zero-initialised = none
    assert re.search(r"typedef struct\s*\{\s*float\s*\*frames;\s*float\s*\*phonemes;\s*uint32_t\s+n_bands;\s*const uint32_t \*edges;\s*\}\s*zv_bands;", header)
    # the kernels take every non-integer step from bands.h and sum the matrix products on the i8 MFMA
    kernels = re.sub(r"//.*", "", open(os.path.join(CSRC, "bands_kernels.hip")).read())
    for fn in ("bands_span", "bands_exponent", "bands_quant", "bands_digits", "bands_power", "bands_row", "bands_phoneme_row", "contour_extent",
               "__builtin_amdgcn_mfma_i32_16x16x64_i8"):
        assert fn + "(" in kernels, fn
    assert "sqrt" not in kernels
    assert capi.BandLevels.DEFAULT_EDGES == BR.DEFAULT_EDGES


def test_null_model_is_refused_by_every_entry_point():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    n = C.c_uint32(0)
    bnd = capi.BandsC()
    assert lib.zv_synthesize_bands(None, None, None, None, 4, 8, None, C.byref(n), None, None, None, 0, 0, None, None, None, None, None,
                                   C.byref(bnd)) == 5
    assert b"zv_synthesize_bands" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_bands(None, 1, None, None, None, None, None, None, None, None, None, None, None, 0, None, None, None, None,
                                         None, bnd) == 5
    assert b"zv_synthesize_batch_bands" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_begin_bands(None, 0, 1, None, None, None, None, None, None, None, None, None, None, None, 0, None, None,
                                               None, None, None, bnd) == 5
    assert b"zv_synthesize_batch_begin_bands" in lib.zv_last_error()
    assert lib.zv_band_levels(None, None, 8, C.byref(bnd)) == 5
    assert b"zv_band_levels" in lib.zv_last_error()


def test_band_levels_refuses_a_phoneme_table_and_a_missing_frame_table():
    """both are refused ahead of everything that needs the model: a handle that is not null but never dereferenced shows it"""
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    rows, wav = np.zeros((8, 16), F), np.zeros(8 * 300, F)
    handle = C.c_void_p(wav.ctypes.data)                      # never dereferenced: the argument checks come first
    bnd = capi.BandsC(rows.ctypes.data, rows.ctypes.data, 0, None)
    assert lib.zv_band_levels(handle, wav.ctypes.data, 8, C.byref(bnd)) == 5
    assert b"zv_band_levels" in lib.zv_last_error() and b"phonemes must be NULL" in lib.zv_last_error()
    bnd = capi.BandsC(None, None, 0, None)
    assert lib.zv_band_levels(handle, wav.ctypes.data, 8, C.byref(bnd)) == 5
    assert b"zv_band_levels" in lib.zv_last_error() and b"frames is required" in lib.zv_last_error()


class _NoDevice:
    """stands where a capi.Model would: any touch of the library or the handle fails the test"""
    hp = types.SimpleNamespace(audio_hop_size=300)

    def __getattr__(self, name):
        raise AssertionError(f"the binding touched .{name} before it had checked its arguments")


def test_binding_refuses_a_bad_return_bands_before_touching_a_device():
    from zerovox_cpp_amd import capi
    ids, puncts, style = np.ones(4, np.int32), np.zeros(4, np.int32), np.zeros(528, np.float32)
    fake = _NoDevice()
    two = [(ids, puncts, style, 64), (ids, puncts, style, 7)]
    for bad in ("frame", "both", ""):
        with pytest.raises(ValueError, match="return_bands = %r: expected False, True, 'frames', 'phonemes' or a BandLevels" % bad):
            capi.Model.synthesize(fake, ids, puncts, style, 64, return_bands=bad)
        with pytest.raises(ValueError, match="utterance 1: return_bands = %r" % bad):
            capi.BatchCall(fake, two, return_bands=[True, bad])
    for bad in (1, None, 2.0, b"frames", {}):
        with pytest.raises(TypeError, match="return_bands must be a bool, 'frames', 'phonemes' or a BandLevels"):
            capi.Model.synthesize(fake, ids, puncts, style, 64, return_bands=bad)
        with pytest.raises(TypeError, match="return_bands must be a bool, 'frames', 'phonemes' or a BandLevels"):
            capi.BatchCall(fake, two, return_bands=bad)
    with pytest.raises(ValueError, match="return_bands has 1 entries, the batch has 2"):
        capi.BatchCall(fake, two, return_bands=["frames"])
    for kw in (dict(n_bands=-1), dict(n_bands=1 << 32), dict(edges=[1]), dict(edges=[1.5, 2.5]), dict(edges=[-1, 4]), dict(n_bands=3, edges=[1, 2, 3])):
        with pytest.raises(ValueError, match="BandLevels"):
            capi.BandLevels(**kw)
    for kw in (dict(n_bands=1.5), dict(n_bands=True), dict(frames=1)):
        with pytest.raises(TypeError, match="BandLevels"):
            capi.BandLevels(**kw)
    with pytest.raises(TypeError, match="band_levels: params must be a BandLevels or None"):
        capi.Model.band_levels(fake, np.zeros(300, F), params=True)
    with pytest.raises(ValueError, match="band_levels: the waveform must be"):
        capi.Model.band_levels(fake, np.zeros(301, F))
    # a well-formed call is built without a device: one wish for the batch, or one per utterance
    t = capi.BandLevels(edges=[2, 10, 100, 513], phonemes=False)
    bc = capi.BatchCall(fake, two + [(ids, puncts, style, 9)] * 3, return_bands=["frames", "phonemes", True, False, t])
    shape = lambda a: None if a is None else a.shape
    assert [None if p is None else (shape(p.frames), shape(p.phonemes)) for p in bc.bands] == \
        [((64, 16), None), (None, (4, 16)), ((9, 16), (4, 16)), None, ((9, 3), None)]
    assert [(bool(s.frames), bool(s.phonemes)) for s in bc.band] == [(True, False), (False, True), (True, True), (False, False), (True, False)]
    s = bc.band[4]
    assert s.n_bands == 3 and s.edges == t.edges.ctypes.data and bc.band[0].n_bands == 0 and not bc.band[0].edges
    assert bc.band[0].frames == bc.bands[0].frames.ctypes.data and bc.band[2].phonemes == bc.bands[2].phonemes.ctypes.data
    for none in (False, [False] * 5, capi.BandLevels(frames=False, phonemes=False)):
        plain = capi.BatchCall(fake, two + [(ids, puncts, style, 9)] * 3, return_bands=none)
        assert plain.band is None and plain.bands is None
    t = capi.BandLevels.from_hz(SR, [100, 1000, 8000])
    assert t.edges.tolist() == [5, 46, 372] and t.n_bands == 2
    with pytest.raises(ValueError, match="do not ascend strictly"):
        capi.BandLevels.from_hz(SR, [100, 105, 1000])
    assert capi.Bands.dbfs([1.0, 0.1, 0.0]).tolist() == [0.0, -20.0, -np.inf]


def test_call_variant_routes_only_a_bands_request_to_the_bands_symbol():
    from zerovox_cpp_amd import capi
    seen = []
    lib = types.SimpleNamespace(**{name: (lambda *a, _n=name: seen.append((_n, a)) or 0)
                                   for name in ("zv_synthesize", "zv_synthesize_pitch", "zv_synthesize_bands")})
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev", "env", "ctr", "pit", "bnd")
    capi._call_variant(lib, "zv_synthesize", (1, 2), target=0, bands="bnd")
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev", "env", "ctr", "pit", None)
    capi._call_variant(lib, "zv_synthesize", (1, 2))
    assert seen == [("zv_synthesize_bands", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev", "env", "ctr", "pit", "bnd")),
                    ("zv_synthesize_bands", (1, 2, None, None, None, 0, 0, None, None, None, None, None, "bnd")),
                    ("zv_synthesize_pitch", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev", "env", "ctr", "pit")), ("zv_synthesize", (1, 2))]


def test_cli_knows_the_flags_and_refuses_bad_edges(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert all(f in r.stdout for f in ("--bands FILE", "--phoneme-bands FILE", "--band-edges-hz a,b,c,..."))
    utt = tmp_path / "utt.txt"
    utt.write_text("1 2 3\n0 0 0\n0\n")
    base = [CLI, "-m", "/nonexistent/model.gguf", "-u", str(utt)]
    for args in (["--bands"], ["--phoneme-bands"], ["--bands", str(tmp_path / "f.tsv"), "--band-edges-hz"]):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and args[-1] + " needs a value" in r.stderr, (args, r.returncode, r.stderr[-300:])
    for bad in ("100", "100,100", "200,100", "0,100", "100,,200", "100,abc", "100,200,", "nan,100", "-5,100", ",".join(str(100 + i) for i in range(66))):
        r = subprocess.run(base + ["--bands", str(tmp_path / "f.tsv"), "--band-edges-hz", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--band-edges-hz needs 2 to 65 ascending numbers" in r.stderr, (bad, r.returncode, r.stderr[-300:])
    r = subprocess.run(base + ["--band-edges-hz", "100,200"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "needs --bands FILE or --phoneme-bands FILE" in r.stderr
    # well-formed flags pass the usage checks: the run then fails at the missing checkpoint, which is no usage error
    r = subprocess.run(base + ["--bands", str(tmp_path / "f.tsv"), "--phoneme-bands", str(tmp_path / "p.tsv"), "--band-edges-hz", "100,1000,8000"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode not in (0, 2) and "usage" not in r.stderr.lower()
