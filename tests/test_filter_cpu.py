"""The waveform filter (include/zerovox_amd.h "waveform filter") on the CPU: csrc/filter.h against its numpy restatement
(tests/filter_rule.py).
 * tests/native/filter_check.cpp drives zv::filter_reference over random waveforms with non-symmetric taps of every length class,
   lengths around one frame and around the kernel's tile, special values and sums that overflow f32: bit for bit;
 * zv::filter_design against the numpy design within one f32 ulp of the largest tap, all-ones gains exactly the delta filter, and its
   refusals by field;
 * the same input through a build with -fsanitize=address,undefined (a plain host program, nothing preloaded);
 * the design's frequency response against the gains asked for, away from the edges;
 * the boundary: the entry points are declared, exported and bound, refuse a NULL model by name, zv_filter_design answers through the
   library with the messages of the header, the binding builds its structs without a device, _call_variant routes a filter and
   nothing else to the _filter symbol, and the CLI knows its flags."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import filter_rule as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
CLI = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
NAMES = ("zv_synthesize_filter", "zv_synthesize_batch_filter", "zv_synthesize_batch_begin_filter", "zv_filter_wave", "zv_filter_design")
F = np.float32
HOP = 300
LENGTHS = (1, 3, 33, 255, 511)
SPECIALS = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x7f7fffff, 0xffc12345], np.uint32).view(F)


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "filter_check.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("filter_check")
    return _build(tmp, "filter_check", []), _build(tmp, "filter_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _hex(a):
    return " ".join("%x" % b for b in FR.bits(a))


def _taps(rng, L):
    """non-symmetric, a few of them zero or negative zero"""
    h = (rng.standard_normal(L) / np.sqrt(L)).astype(F)
    if L > 3:
        h[rng.integers(0, L, 2)] = [0.0, -0.0]
    return h


def _apply_cases():
    rng = np.random.default_rng(20261020)
    cases = []
    for L in LENGTHS:
        for total in (HOP, 2 * HOP, FR.TILE - HOP, FR.TILE - 1, FR.TILE, FR.TILE + 1, FR.TILE + HOP):
            x = (rng.standard_normal(total) * 0.3).astype(F)
            cases.append(("random L=%d total=%d" % (L, total), x, total, _taps(rng, L)))
    # a span shorter than the capacity (fitted), the empty span, and no filter at all (a copy, specials included)
    x = (rng.standard_normal(3 * HOP) * 0.3).astype(F)
    cases.append(("fitted", x, 2 * HOP, _taps(rng, 33)))
    cases.append(("fitted empty", x, 0, _taps(rng, 33)))
    y = x.copy()
    y[:SPECIALS.size] = SPECIALS
    cases.append(("copy", y, y.size, None))
    # special values: a NaN or an infinity is +0.0 to its neighbours, -0.0 and subnormals are themselves
    for L in (1, 3, 255):
        z = (rng.standard_normal(HOP + 77) * 0.3).astype(F)
        z[rng.choice(z.size, 4 * SPECIALS.size, replace=False)] = np.tile(SPECIALS, 4)
        cases.append(("specials L=%d" % L, z, z.size, _taps(rng, L)))
    cases.append(("identity specials", y, y.size, np.ones(1, F)))
    # sums beyond f32: large samples under large taps of one sign
    big = np.full(HOP, 3.0e38, F)
    big[::7] = -3.0e38
    cases.append(("overflow", big, big.size, np.full(33, 1.5, F)))
    cases.append(("overflow products", np.full(HOP, 1.0e30, F), HOP, np.array([1.0e30, -1.0e30, 1.0e20], F)))
    cases.append(("subnormal results", np.full(HOP, 1.0e-30, F), HOP, np.array([1.0e-10, 3.0e-12, -1.0e-10], F)))
    return cases


@pytest.fixture(scope="module")
def apply_cases():
    return _apply_cases()


REFUSED = [("n_taps", 2, None), ("n_taps", 512, None), ("n_taps", 513, None), ("taps", 3, np.inf), ("taps", 255, np.nan)]


def _design_cases():
    rng = np.random.default_rng(7)
    cases = []
    for L in (1, 3, 127, 255, 511):
        cases.append((0, None, np.power(10.0, rng.uniform(-12, 12, 16) / 20).astype(F), L))
        cases.append((16, None, np.ones(16, F), L))
    cases.append((3, [2, 10, 100, 513], np.array([0.0, 2.0, 0.5], F), 255))
    cases.append((1, [0, 513], np.array([0.25], F), 33))
    cases.append((64, list(range(100, 165)), rng.uniform(0, 4, 64).astype(F), 511))
    return cases


DESIGN_REFUSED = [("n_bands", 65, list(range(1, 67)), np.ones(65, F), 255), ("edges", 3, None, np.ones(3, F), 255),
                  ("edges", 2, [5, 5, 9], np.ones(2, F), 255), ("edges", 2, [5, 9, 514], np.ones(2, F), 255),
                  ("n_taps", 0, None, np.ones(16, F), 0), ("n_taps", 0, None, np.ones(16, F), 254), ("n_taps", 0, None, np.ones(16, F), 513),
                  ("gains", 0, None, np.r_[np.ones(15, F), F(-0.5)], 255), ("gains", 0, None, np.r_[np.ones(15, F), F(np.inf)], 255),
                  ("gains", 2, [5, 9, 20], np.array([1.0, np.nan], F), 255)]


def _stdin(apply_cases):
    lines = ["constants"]
    for _, x, S, h in apply_cases:
        lines += ["apply %d %d %d" % (S, x.size, 0 if h is None else h.size), "" if h is None else _hex(h), _hex(x)]
    for _, L, bad in REFUSED:
        h = np.full(L, 0.5, F)
        if bad is not None:
            h[L // 2] = bad
        lines += ["apply 4 4 %d" % L, _hex(h), _hex(np.ones(4, F))]
    for nb, e, g, L in _design_cases() + [r[1:] for r in DESIGN_REFUSED]:
        lines += ["design %d %d %d" % (nb, 0 if e is None else len(e), L), "" if e is None else " ".join(map(str, e)), _hex(g)]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def outputs(exes, apply_cases):
    text = _stdin(apply_cases)
    return [subprocess.run([e], input=text, capture_output=True, text=True, timeout=900) for e in exes]


def _floats(line):
    return np.array([int(t, 16) for t in line.split()], np.uint32).view(F)


def test_header_equals_restatement(apply_cases, outputs):
    r = outputs[0]
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0].split() == [str(FR.TILE), str(FR.MAX_TAPS), str(1 + FR.MAX_TAPS)] + [str(e) for e in FR.DEFAULT_EDGES]
    at = 1
    for name, x, S, h in apply_cases:
        got, want = _floats(lines[at]), FR.apply(x, h, S)
        assert np.array_equal(FR.bits(got), FR.bits(want)), name
        at += 1
    for field, L, _ in REFUSED:
        assert lines[at] == "refused " + field, (field, L, lines[at])
        at += 1
    for nb, e, g, L in _design_cases():
        got, want = _floats(lines[at]), FR.design(g, e, L)
        # two libms differ by about an f64 ulp: after the rounding to f32 at most one ulp of the tap, and no tap's ulp exceeds the largest's
        assert got.size == L and np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23 * np.abs(want).max(), (nb, L)
        if np.all(g == 1):
            delta = np.zeros(L, F)
            delta[(L - 1) // 2] = 1
            assert np.array_equal(FR.bits(got), FR.bits(delta)) and np.array_equal(FR.bits(want), FR.bits(delta)), L
        at += 1
    for field, nb, e, g, L in DESIGN_REFUSED:
        assert lines[at] == "refused " + field, (field, nb, L, lines[at])
        at += 1
    assert at == len(lines)


def test_sanitized_build_agrees_and_is_silent(outputs):
    plain, san = outputs
    assert san.returncode == 0, san.stderr[-2000:]
    assert san.stdout == plain.stdout and san.stderr == ""


def test_the_named_cases_reach_what_they_name(apply_cases):
    by = {name: (x, S, h) for name, x, S, h in apply_cases}
    x, S, h = by["overflow"]
    assert np.isinf(FR.apply(x, h, S)).any()
    x, S, h = by["subnormal results"]
    y = FR.apply(x, h, S)
    assert ((np.abs(y) < np.finfo(F).tiny) & (y != 0)).any()
    x, S, h = by["identity specials"]
    y = FR.apply(x, h, S)
    k = SPECIALS.size
    assert np.array_equal(FR.bits(y[:k]), FR.bits(np.where(np.isfinite(SPECIALS), SPECIALS, 0) + F(0)))      # -0.0 -> +0.0, NaN and inf -> +0.0
    assert FR.bits(y[3]) == 0 and y[4] == SPECIALS[4]
    x, S, h = by["copy"]
    assert np.array_equal(FR.bits(FR.apply(x, None, S)), FR.bits(x))
    x, S, h = by["fitted"]
    y = FR.apply(x, h, S)
    assert not y[S:].any() and np.array_equal(FR.bits(y[:S]), FR.bits(FR.apply(x[:S], h)))
    # an impulse reads the taps back at the right offset and orientation
    h = np.arange(1, 8, dtype=F)
    for at in (0, 1, 2, 3, 40, 99):
        d = np.zeros(100, F)
        d[at] = 1
        want = np.zeros(100, F)
        lo, hi = max(at - 3, 0), min(at + 4, 100)
        want[lo:hi] = h[lo - at + 3: hi - at + 3]
        assert np.array_equal(FR.apply(d, h), want), at


def test_the_design_meets_the_gains_away_from_the_edges():
    """at every frequency at least 4096 / (L + 1) bins from every edge: ||H| - gain| <= 0.0063 * the sum of the gain steps at all edges
    (the Hann window's -44 dB approximation error per step, added at worst)"""
    rng = np.random.default_rng(11)
    edges = np.array(FR.DEFAULT_EDGES, np.float64) - 0.5
    edges[0], edges[-1] = max(edges[0], 0.0), 512.0
    k = np.arange(2049) / 4.0                                       # frequencies of response(): a quarter of a bin apart
    worst = 0.0
    for L in (127, 255, 511):
        clear = np.abs(k[:, None] - edges[None, :]).min(axis=1) >= 4096.0 / (L + 1)
        for _ in range(20):
            g = np.power(10.0, rng.uniform(-12, 12, 16) / 20).astype(F)
            full = np.r_[1.0, g.astype(np.float64), 1.0]           # gain 1 outside every band
            steps = np.abs(np.diff(full)).sum()
            want = full[np.searchsorted(edges, k, side="right")]
            dev = np.abs(FR.response(FR.design(g, None, L)) - want)[clear]
            assert clear.any() and dev.max() <= 0.0063 * steps, (L, dev.max(), steps)
            worst = max(worst, dev.max() / steps)
    print("largest deviation / sum of steps: %.5f" % worst)


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
        assert _declaration(header, name + "_filter") == _declaration(header, name + "_bands") + ["const zv_filter*"], name
        assert getattr(lib, name + "_filter").argtypes == getattr(lib, name + "_bands").argtypes + [C.POINTER(capi.FilterC)]
    assert _declaration(header, "zv_filter_wave") == ["zv_model*", "const float*", "uint32_t", "const zv_filter*", "float*"]
    assert _declaration(header, "zv_filter_design") == ["uint32_t", "const uint32_t*", "const float*", "uint32_t", "float*"]
    assert not re.search(r"\bzv_synthesize_batch_end_filter\b", header)            # the existing _end finishes a filter batch
    assert C.sizeof(capi.FilterC) == 16 and bytes(capi.FilterC()) == bytes(16)      # zero-initialised = none
    assert re.search(r"typedef struct\s*\{\s*const float \*taps;\s*uint32_t\s+n_taps;\s*\}\s*zv_filter;", header)
    # the kernel takes its sample test from filter.h and walks the taps in f64 fused multiply-adds, with no matrix instruction
    kernel = re.sub(r"//.*", "", open(os.path.join(CSRC, "filter_kernels.hip")).read())
    assert "filter_sample(" in kernel and "__builtin_fma(" in kernel and "mfma" not in kernel
    assert "FILTER_TILE = 256 * FILTER_LANE_OUTPUTS" in open(os.path.join(CSRC, "filter.h")).read()


def test_null_model_is_refused_by_every_entry_point():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    n = C.c_uint32(0)
    flt = capi.FilterC()
    assert lib.zv_synthesize_filter(None, None, None, None, 4, 8, None, C.byref(n), None, None, None, 0, 0, None, None, None, None, None,
                                    None, C.byref(flt)) == 5
    assert b"zv_synthesize_filter" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_filter(None, 1, None, None, None, None, None, None, None, None, None, None, None, 0, None, None, None, None,
                                          None, None, flt) == 5
    assert b"zv_synthesize_batch_filter" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_begin_filter(None, 0, 1, None, None, None, None, None, None, None, None, None, None, None, 0, None, None,
                                                None, None, None, None, flt) == 5
    assert b"zv_synthesize_batch_begin_filter" in lib.zv_last_error()
    assert lib.zv_filter_wave(None, None, 8, C.byref(flt), None) == 5
    assert b"zv_filter_wave" in lib.zv_last_error()


def test_the_design_through_the_library_and_its_messages():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    for nb, e, g, L in _design_cases():
        got, want = capi.filter_design(g, e, L), FR.design(g, e, L)
        assert got.dtype == F and got.size == L
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23 * np.abs(want).max(), (nb, L)
    delta = capi.filter_design(np.ones(16, F))
    assert delta.size == 255 and delta[127] == 1 and np.count_nonzero(delta) == 1
    f = capi.Filter.from_band_gains_db([0.0] * 8 + [-12.0] * 8)
    assert f.n_taps == 255 and np.array_equal(f.taps, capi.filter_design(np.r_[np.ones(8), np.full(8, 10 ** -0.6)].astype(F)))
    messages = {"n_bands": "zv_filter_design: n_bands = 65 exceeds 64", "n_taps": "zv_filter_design: n_taps = %u must be odd and in 1 .. 511",
                "gains": "zv_filter_design: gains holds a value that is negative or not finite"}
    for field, nb, e, g, L in DESIGN_REFUSED:
        taps = np.zeros(600, F)
        ee = None if e is None else np.asarray(e, np.uint32)
        st = lib.zv_filter_design(nb, None if ee is None else ee.ctypes.data, g.ctypes.data, L, taps.ctypes.data)
        msg = lib.zv_last_error().decode()
        assert st == 5 and not taps.any(), (field, nb, L)
        if field == "edges":
            assert msg.startswith("zv_filter_design: edges"), msg
        else:
            assert msg == messages[field].replace("%u", str(L)), msg
    assert lib.zv_filter_design(0, None, None, 255, np.zeros(255, F).ctypes.data) == 5 and b"zv_filter_design: null argument" in lib.zv_last_error()
    with pytest.raises(capi.ZvError, match="gains holds a value"):
        capi.filter_design([1.0, -1.0], [3, 9, 20])
    with pytest.raises(ValueError, match="edges has 2 entries, 2 gains need 3"):
        capi.filter_design([1.0, 1.0], [3, 9])


class _NoDevice:
    """stands where a capi.Model would: any touch of the library or the handle fails the test"""
    hp = types.SimpleNamespace(audio_hop_size=300)

    def __getattr__(self, name):
        raise AssertionError(f"the binding touched .{name} before it had checked its arguments")


def test_binding_builds_its_structs_without_a_device():
    from zerovox_cpp_amd import capi
    ids, puncts, style = np.ones(4, np.int32), np.zeros(4, np.int32), np.zeros(528, np.float32)
    fake = _NoDevice()
    two = [(ids, puncts, style, 64), (ids, puncts, style, 7)]
    h = np.arange(5, dtype=np.float64)
    bc = capi.BatchCall(fake, two + [(ids, puncts, style, 9)], filter=[capi.Filter(h), None, [1.0, 2.0, 3.0]])
    assert [s.n_taps for s in bc.filter] == [5, 0, 3] and not bc.filter[1].taps
    assert bc.filter[0].taps == bc.fkeep[0].taps.ctypes.data and bc.fkeep[0].taps.dtype == F
    bc.set_filter(1, capi.Filter(None, n_taps=77))
    bc.set_filter(0, None)
    assert [s.n_taps for s in bc.filter] == [0, 77, 3] and not bc.filter[0].taps and not bc.filter[1].taps
    assert capi.BatchCall(fake, two).filter is None
    with pytest.raises(ValueError, match="filter has 1 entries, the batch has 2"):
        capi.BatchCall(fake, two, filter=[None])
    with pytest.raises(ValueError, match="built without filters"):
        capi.BatchCall(fake, two).set_filter(0, None)
    with pytest.raises(TypeError, match="utterance 1: filter must be a Filter"):
        capi.BatchCall(fake, two, filter=[None, "taps"])
    with pytest.raises(TypeError, match="filter must be a Filter"):
        capi.Model.synthesize(fake, ids, puncts, style, 64, filter={"taps": 1})
    with pytest.raises(ValueError, match="Filter taps must be a 1-D sequence"):
        capi.Filter(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="filter_wave: the waveform must be"):
        capi.Model.filter_wave(fake, np.zeros(301, F), [1.0])
    with pytest.raises(TypeError, match="filter_wave: filter must be"):
        capi.Model.filter_wave(fake, np.zeros(300, F), None)


def test_call_variant_routes_only_a_filter_to_the_filter_symbol():
    from zerovox_cpp_amd import capi
    seen = []
    lib = types.SimpleNamespace(**{name: (lambda *a, _n=name: seen.append((_n, a)) or 0)
                                   for name in ("zv_synthesize", "zv_synthesize_bands", "zv_synthesize_filter")})
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev", "env", "ctr", "pit", "bnd", "flt")
    capi._call_variant(lib, "zv_synthesize", (1, 2), target=0, filter="flt")
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", True, 99, "vol", "lev", "env", "ctr", "pit", "bnd", None)
    capi._call_variant(lib, "zv_synthesize", (1, 2))
    assert seen == [("zv_synthesize_filter", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev", "env", "ctr", "pit", "bnd", "flt")),
                    ("zv_synthesize_filter", (1, 2, None, None, None, 0, 0, None, None, None, None, None, None, "flt")),
                    ("zv_synthesize_bands", (1, 2, "pr", "pc", "dur", 99, 1, "vol", "lev", "env", "ctr", "pit", "bnd")), ("zv_synthesize", (1, 2))]


def test_cli_knows_the_flags_and_refuses_bad_values(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert all(f in r.stdout for f in ("--eq-gain-db g0,g1,...", "--eq-edges-hz a,b,c,...", "--eq-taps L", "--filter-taps FILE"))
    utt = tmp_path / "utt.txt"
    utt.write_text("1 2 3\n0 0 0\n0\n")
    base = [CLI, "-m", "/nonexistent/model.gguf", "-u", str(utt)]
    for flag in ("--eq-gain-db", "--eq-edges-hz", "--eq-taps", "--filter-taps"):
        r = subprocess.run(base + [flag], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and flag + " needs a value" in r.stderr, (flag, r.returncode, r.stderr[-300:])
    for bad in ("", "1,,2", "abc", "1,nan", "3,inf"):
        r = subprocess.run(base + ["--eq-gain-db", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--eq-gain-db needs 1 to 64 finite numbers" in r.stderr, (bad, r.returncode, r.stderr[-300:])
    for bad in ("0", "abc", "254", "513", "-3"):
        r = subprocess.run(base + ["--eq-gain-db", "0,0", "--eq-edges-hz", "100,1000,8000", "--eq-taps", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--eq-taps needs an odd number in 1 .. 511" in r.stderr, (bad, r.returncode, r.stderr[-300:])
    r = subprocess.run(base + ["--eq-edges-hz", "100,200"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--eq-edges-hz and --eq-taps need --eq-gain-db" in r.stderr
    r = subprocess.run(base + ["--eq-gain-db", "0,0,0", "--eq-edges-hz", "100,1000,8000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--eq-gain-db has 3 gains, --eq-edges-hz gives 2 bands" in r.stderr
    taps = tmp_path / "taps.txt"
    taps.write_text("0.25\n0.5\n0.25\n")
    r = subprocess.run(base + ["--filter-taps", str(taps), "--eq-gain-db", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--filter-taps and --eq-gain-db exclude each other" in r.stderr
    r = subprocess.run(base + ["--filter-taps", str(tmp_path / "missing.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--filter-taps: cannot read" in r.stderr
    # well-formed flags pass the usage checks: the run then fails at the missing checkpoint, which is no usage error
    for args in (["--filter-taps", str(taps)], ["--eq-gain-db", "0,-12", "--eq-edges-hz", "100,1000,8000", "--eq-taps", "127"],
                 ["--eq-gain-db", ",".join(["-3"] * 16)]):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode not in (0, 2) and "usage" not in r.stderr.lower(), (args, r.returncode, r.stderr[-300:])
