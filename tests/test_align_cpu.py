"""Mel alignment (include/zerovox_amd.h "mel alignment") on the CPU: csrc/align.h against its restatement in exact integers and single
float64 steps (tests/align_rule.py), bit for bit.
 * the two forms of the restatement (plain loops, anti-diagonals) are held equal at small sizes;
 * tests/native/align_check.cpp drives zv::align_reference over the shapes (1,1) .. (300,41), M of 1, 80 and 256, with and without
   normalise, on random rows, rows holding NaN and +-inf, rows beyond the clamp and tie-rich rows: total, maps, path length and the
   distance's bit pattern must agree;
 * the same input through a build with -fsanitize=address,undefined (a plain host program, nothing preloaded);
 * the known answers: A against A, A against A with repeated rows (both roles), A against A + k/64 with normalise;
 * zv_align_durations against the formulas, its refusals by name, without a device;
 * the boundary: the three entry points are declared, exported and bound, and refuse NULL arguments by name; the launch plan and the
   launch groups; the CLI's flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import align_rule as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
NAMES = ("zv_mel_align", "zv_mel_align_batch", "zv_align_durations")
F = np.float32
SHAPES = [(1, 1), (1, 7), (7, 1), (16, 16), (17, 33), (64, 65), (300, 41)]
WIDTHS = (1, 80, 256)


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "align_check.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("align_check")
    return _build(tmp, "align_check", []), _build(tmp, "align_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _fbits(x):
    return "%x" % int(np.array([x], F).view(np.uint32)[0])


# ---- cases ------------------------------------------------------------------------------------------------------------------------

def mel_like(rng, T, M):
    """rows in the range of natural-log mels: a slow drift plus noise"""
    return (rng.standard_normal((T, M)) * 1.5 - 4.0 + np.cumsum(rng.standard_normal((T, 1)) * 0.3, axis=0)).astype(F)


def tie_rich(rng, T, M):
    """rows drawn from an alphabet of three rows on the 1/64 grid: equal costs everywhere, so the tie order decides the path"""
    alphabet = (rng.integers(-200, 200, (3, M)) / 64.0).astype(F)
    return alphabet[rng.integers(0, 3, T)]


def _inputs(rng, kind, T, M):
    if kind == "random":
        return mel_like(rng, T, M)
    if kind == "specials":
        x = mel_like(rng, T, M)
        idx = rng.integers(0, x.size, max(1, x.size // 7))
        x.reshape(-1)[idx] = rng.choice(np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0xffc00001], np.uint32).view(F), idx.size)
        return x
    if kind == "clamp":
        x = mel_like(rng, T, M) * F(6.0)                   # +-16 at scale 64 is the clamp's +-1023: many entries lie beyond it
        x.reshape(-1)[rng.integers(0, x.size, max(1, x.size // 9))] = F(1e30)
        x.reshape(-1)[rng.integers(0, x.size, max(1, x.size // 9))] = F(-3e38)
        return x
    return tie_rich(rng, T, M)


def _cases(rng):
    c = []
    for Ta, Tb in SHAPES:
        for M in WIDTHS:
            for normalise in (0, 1):
                for kind in ("random", "specials", "clamp", "ties"):
                    scale = 0.0 if kind != "random" or M != 80 else (10.0, 100.5)[normalise]
                    if kind == "ties":                     # both sides from ONE alphabet
                        both = tie_rich(rng, Ta + Tb, M)
                        a, b = both[:Ta], both[Ta:]
                    else:
                        a, b = _inputs(rng, kind, Ta, M), _inputs(rng, kind, Tb, M)
                    c.append(dict(name=f"{Ta}x{Tb}x{M} {kind} normalise {normalise}", a=a, b=b, scale=scale, normalise=normalise))
    return c


REFUSED = [("a negative scale", -1.0, 0, "scale"), ("a NaN scale", float("nan"), 0, "scale"), ("an infinite scale", float("inf"), 1, "scale"),
           ("normalise 2", 0.0, 2, "normalise")]


def _stdin(cases):
    lines = []
    for c in cases:
        a, b = c["a"], c["b"]
        lines.append(f"{a.shape[0]} {b.shape[0]} {a.shape[1]} {_fbits(c['scale'])} {c['normalise']}")
        lines.append(" ".join(map("%x".__mod__, AR.bits(a).reshape(-1).tolist())))
        lines.append(" ".join(map("%x".__mod__, AR.bits(b).reshape(-1).tolist())))
    return "\n".join(lines) + "\n"


def parse(line):
    """a result line of align_check -> (total, distance bits, path_len, map_a, map_b)"""
    head, ma, mb = line.split("|")
    total, dist, L = head.split()
    return int(total), int(dist, 16), int(L), np.array(ma.split(), np.int32), np.array(mb.split(), np.int32)


def same(have, want):
    """have: parse()'s tuple; want: the restatement's (total, distance, path_len, map_a, map_b)"""
    total, dist, L, ma, mb = want
    return (have[0] == total and have[1] == int(np.array([dist], np.float64).view(np.uint64)[0]) and have[2] == L and
            np.array_equal(have[3], ma) and np.array_equal(have[4], mb))


@pytest.fixture(scope="module")
def cases():
    return _cases(np.random.default_rng(20261021))


@pytest.fixture(scope="module")
def refused():
    z = np.zeros((2, 3), F)
    return [dict(name=name, a=z, b=z, scale=scale, normalise=normalise) for name, scale, normalise, _ in REFUSED]


@pytest.fixture(scope="module")
def outputs(exes, cases, refused):
    text = _stdin(cases + refused)
    return [subprocess.run([e], input=text, capture_output=True, text=True, timeout=900) for e in exes]


def _run(exe, cases):
    r = subprocess.run([exe], input=_stdin(cases), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    return [parse(line) for line in r.stdout.splitlines()]


# ---- 1. the restatement's two forms, the header against them ----------------------------------------------------------------------

def test_the_two_forms_of_the_restatement_agree():
    rng = np.random.default_rng(7)
    for Ta, Tb, M in ((1, 1, 1), (1, 7, 3), (7, 1, 3), (9, 14, 5), (16, 16, 80), (17, 33, 2), (23, 8, 256)):
        for normalise in (0, 1):
            for a, b in ((mel_like(rng, Ta, M), mel_like(rng, Tb, M)), (lambda x: (x[:Ta], x[Ta:]))(tie_rich(rng, Ta + Tb, M)),
                         (_inputs(rng, "specials", Ta, M), _inputs(rng, "clamp", Tb, M))):
                one, two = AR.align_loops(a, b, 0.0, normalise), AR.align(a, b, 0.0, normalise)
                assert one[:3] == two[:3] and np.array_equal(one[3], two[3]) and np.array_equal(one[4], two[4]), (Ta, Tb, M, normalise)
                assert np.array([one[1]]).view(np.uint64)[0] == np.array([two[1]]).view(np.uint64)[0]


def test_ties_are_exercised(cases):
    """the tie-rich cases hold cells whose predecessors are equal: another tie order gives another path"""
    c = next(c for c in cases if c["name"] == "17x33x80 ties normalise 0")
    cost = AR.costs(c["a"], c["b"])
    assert (cost == 0).sum() > 17 and len(np.unique(cost)) <= 6


def test_header_equals_restatement_bit_for_bit(cases, refused, outputs):
    r = outputs[0]
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(cases) + len(refused)
    for c, line in zip(cases, got):
        want = AR.align(c["a"], c["b"], c["scale"], c["normalise"])
        assert same(parse(line), want), (c["name"], line[:80], want[:3])
    for (name, _, _, field), line in zip(REFUSED, got[len(cases):]):
        assert line == f"refused {field}", name


def test_sanitized_build_agrees(outputs):
    assert outputs[1].returncode == 0 and outputs[1].stderr == "", outputs[1].stderr[-3000:]
    assert outputs[1].stdout == outputs[0].stdout


# ---- 2. known answers -------------------------------------------------------------------------------------------------------------

def distinct_rows(rng, T, M):
    """rows on the 1/64 grid inside the clamp whose neighbours differ"""
    A = (rng.integers(-500, 500, (T, M)) / 64.0).astype(F)
    A[:, 0] = (np.arange(T) % 7 - 3) / 64.0 * 5              # adjacent rows differ in channel 0 whatever the draw
    return A


def test_known_answers(exes):
    rng = np.random.default_rng(11)
    A = distinct_rows(rng, 37, 80)
    reps = rng.integers(1, 5, 37)
    B, starts, index = AR.repeated(A, reps)
    Tb = len(B)
    shifted = (A.astype(np.float64) + 5 / 64.0).astype(F)
    assert np.array_equal(shifted.astype(np.float64), A.astype(np.float64) + 5 / 64.0)       # still on the grid
    cases = [dict(a=A, b=A, scale=0.0, normalise=0), dict(a=A, b=B, scale=0.0, normalise=0), dict(a=B, b=A, scale=0.0, normalise=0),
             dict(a=A, b=shifted, scale=0.0, normalise=1), dict(a=A, b=shifted, scale=0.0, normalise=0)]
    for exe in exes:
        same_, rep, swapped, norm, plain = _run(exe, cases)
        ident = np.arange(37, dtype=np.int32)
        assert same_[0] == 0 and same_[1] == 0 and same_[2] == 37 and np.array_equal(same_[3], ident) and np.array_equal(same_[4], ident)
        assert rep[0] == 0 and rep[1] == 0 and rep[2] == Tb and np.array_equal(rep[3], starts) and np.array_equal(rep[4], index)
        assert swapped[0] == 0 and swapped[2] == Tb and np.array_equal(swapped[4], starts) and np.array_equal(swapped[3], index)
        assert norm[0] == 0 and norm[1] == 0 and norm[2] == 37 and np.array_equal(norm[3], ident)
        assert plain[0] == 37 * 80 * 25 and plain[2] == 37                                    # 5 steps in every channel of every row
        assert abs(float(np.array([plain[1]], np.uint64).view(np.float64)[0]) - np.sqrt(80 * 25.0) / 64.0) < 1e-12
    for c, want in zip(cases, (same_, rep, swapped, norm, plain)):
        assert same(want, AR.align(c["a"], c["b"], c["scale"], c["normalise"]))


# ---- 3. the timing transfer -------------------------------------------------------------------------------------------------------

def _repeated_map():
    reps = np.random.default_rng(11).integers(1, 5, 37)
    return (np.cumsum(reps) - reps).astype(np.int32), int(reps.sum()), reps


def test_align_durations_formulas_and_refusals(exes):
    from zerovox_cpp_amd import capi
    lib = capi.load_library()                             # no model, no device
    map_a, Tb, reps = _repeated_map()
    da = np.array([5, 0, 7, 10, 15], np.int32)
    db = capi.align_durations(da, map_a, Tb, lib=lib)
    want = np.array([reps[:5].sum(), 0, reps[5:12].sum(), reps[12:22].sum(), reps[22:].sum()], np.int32)
    assert db.dtype == np.int32 and np.array_equal(db, want) and db.sum() == Tb and (db >= 0).all()
    assert np.array_equal(db, AR.durations(da, map_a, Tb))
    rng = np.random.default_rng(3)
    text, wants = "", []
    for _ in range(40):
        Ta, Tb2 = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        n = int(rng.integers(1, 9))
        cuts = np.sort(rng.integers(0, Ta + 1, n - 1))
        d = np.diff(np.concatenate([[0], cuts, [Ta]])).astype(np.int32)       # zero-length phonemes included, at either end too
        m = np.sort(rng.integers(0, Tb2, Ta)).astype(np.int32)
        assert np.array_equal(capi.align_durations(d, m, Tb2, lib=lib), AR.durations(d, m, Tb2))
        text += f"{n} {Ta} {Tb2}\n{' '.join(map(str, d))}\n{' '.join(map(str, m))}\n"
        wants.append(" ".join(map(str, AR.durations(d, m, Tb2))))
    bad = [((np.array([5, -1, 33], np.int32), map_a, Tb), "negative duration", "durations_a"),
           ((np.array([5, 0, 7, 10, 14], np.int32), map_a, Tb), "the sum of durations_a must be Ta = 37", "sum"),
           ((da, map_a[::-1].copy(), Tb), "map_a must be non-decreasing inside [0, Tb", "map_a"),
           ((da, map_a, int(map_a[-1])), "map_a must be non-decreasing inside [0, Tb", "map_a"),
           ((da, np.where(np.arange(37) == 3, -1, map_a).astype(np.int32), Tb), "map_a must be non-decreasing inside [0, Tb", "map_a")]
    for args, word, field in bad:
        with pytest.raises(capi.ZvError) as e:
            capi.align_durations(*args, lib=lib)
        assert e.value.status == 5 and "zv_align_durations" in str(e.value) and word in str(e.value), str(e.value)
        text += f"{len(args[0])} 37 {args[2]}\n{' '.join(map(str, args[0]))}\n{' '.join(map(str, args[1]))}\n"
        wants.append(f"refused {field}")
    for exe in exes:
        r = subprocess.run([exe, "durations"], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        assert [line.strip() for line in r.stdout.splitlines()] == wants
    i32 = np.zeros(4, np.int32).ctypes.data
    for args, what in (((1, None, 4, i32, 4, i32), b"durations_a is NULL"), ((1, i32, 4, None, 4, i32), b"map_a is NULL"),
                       ((1, i32, 4, i32, 4, None), b"durations_b is NULL"), ((0, i32, 4, i32, 4, i32), b"n must be > 0"),
                       ((1, i32, 0, i32, 4, i32), b"Ta = 0 and Tb = 4 must be > 0")):
        assert lib.zv_align_durations(*args) == 5 and b"zv_align_durations: " + what in lib.zv_last_error(), lib.zv_last_error()


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
    assert _declaration(header, "zv_mel_align") == ["zv_model*", "const float*", "uint32_t", "const float*", "uint32_t", "uint32_t", "const zv_align*",
                                                   "zv_alignment*", "int32_t*", "int32_t*"]
    assert _declaration(header, "zv_mel_align_batch") == ["zv_model*", "uint32_t", "const float*const*", "const uint32_t*", "const float*const*",
                                                         "const uint32_t*", "uint32_t", "const zv_align*", "zv_alignment*", "int32_t*const*",
                                                         "int32_t*const*"]
    assert _declaration(header, "zv_align_durations") == ["uint32_t", "const int32_t*", "uint32_t", "const int32_t*", "uint32_t", "int32_t*"]
    vp, u32, pvp, pu32 = C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)
    assert lib.zv_mel_align.argtypes == [vp, vp, u32, vp, u32, u32, C.POINTER(capi.AlignC), C.POINTER(capi.AlignmentC), vp, vp]
    assert lib.zv_mel_align_batch.argtypes == [vp, u32, pvp, pu32, pvp, pu32, u32, C.POINTER(capi.AlignC), C.POINTER(capi.AlignmentC), pvp, pvp]
    assert lib.zv_align_durations.argtypes == [u32, vp, u32, vp, u32, vp]
    assert C.sizeof(capi.AlignC) == 8 and bytes(capi.AlignC()) == bytes(8)              # zero-initialised = scale 64, no normalisation
    assert C.sizeof(capi.AlignmentC) == 24 and capi.AlignmentC.distance.offset == 8 and capi.AlignmentC.path_len.offset == 16
    assert re.search(r"typedef struct\s*\{\s*float\s+scale;\s*uint32_t\s+normalise;\s*\}\s*zv_align;", header)
    assert re.search(r"typedef struct\s*\{\s*uint64_t\s+total;\s*double\s+distance;\s*uint32_t\s+path_len;\s*uint32_t\s+reserved;\s*\}\s*zv_alignment;", header)
    assert re.search(r"#define\s+ZV_ALIGN_MAX_FRAMES\s+4096\b", header) and AR.constant("ALIGN_MAX_FRAMES") == 4096
    # no new synthesize form, no new waveform stage
    assert not [s for s in capi.SYMBOLS if "align" in s and (s.startswith("zv_synthesize") or s.startswith("zv_encode_taps"))]
    assert not any("align" in f.suffix for f in capi.FORMS)
    # the kernels take every step of the rule from align.h and sum the dot products on the i8 MFMA
    kernels = re.sub(r"//.*", "", open(os.path.join(CSRC, "align_kernels.hip")).read())
    for fn in ("align_quant", "align_mean", "bands_digits", "align_combine", "align_choose", "align_step", "align_distance", "align_plan",
               "align_dp_steps", "__builtin_amdgcn_mfma_i32_16x16x64_i8"):
        assert fn + "(" in kernels, fn
    assert not re.search(r"\b(sqrt|sqrtf|atomicAdd|atomicMin|hipMemset\w*)\s*\(", kernels)
    assert '#include "align_kernels.hip"' in open(os.path.join(CSRC, "misc_kernels.hip")).read()
    p = capi.AlignParams(32.0, True).struct
    assert (p.scale, p.normalise) == (32.0, 1)
    for call in ("mel_align", "mel_align_batch", "synthesize_like"):
        assert callable(getattr(capi.Model, call))


def test_null_arguments_are_refused_by_name():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    a, b, q, out = np.zeros((8, 80), F), np.zeros((9, 80), F), capi.AlignC(), capi.AlignmentC()
    handle = C.c_void_p(a.ctypes.data)                        # never dereferenced: the argument checks come first
    ok = [handle, a.ctypes.data, 8, b.ctypes.data, 9, 80, C.byref(q), C.byref(out), None, None]
    for i, what in ((0, b"m is NULL"), (1, b"a is NULL"), (3, b"b is NULL"), (6, b"params is NULL"), (7, b"out is NULL")):
        args = list(ok)
        args[i] = None
        assert lib.zv_mel_align(*args) == 5 and b"zv_mel_align: " + what in lib.zv_last_error(), lib.zv_last_error()
    for i, v, what in ((2, 0, b"Ta = 0"), (2, 4097, b"Ta = 4097"), (4, 0, b"Tb = 0"), (4, 4097, b"Tb = 4097"), (5, 0, b"M = 0"), (5, 257, b"M = 257")):
        args = list(ok)
        args[i] = v
        assert lib.zv_mel_align(*args) == 5 and b"zv_mel_align: " + what in lib.zv_last_error(), lib.zv_last_error()
    for q2, what in ((capi.AlignC(-2.0, 0), b"align scale"), (capi.AlignC(float("nan"), 0), b"align scale"), (capi.AlignC(0.0, 2), b"align normalise = 2")):
        args = list(ok)
        args[6] = C.byref(q2)
        assert lib.zv_mel_align(*args) == 5 and b"zv_mel_align: " + what in lib.zv_last_error(), lib.zv_last_error()
    P, U = C.c_void_p * 2, C.c_uint32 * 2
    outs = (capi.AlignmentC * 2)()
    okb = [handle, 2, P(a.ctypes.data, a.ctypes.data), U(8, 8), P(b.ctypes.data, b.ctypes.data), U(9, 9), 80, C.byref(q), outs, None, None]
    for i, v, what in ((0, None, b"m is NULL"), (2, None, b"a is NULL"), (3, None, b"Ta is NULL"), (4, None, b"b is NULL"), (5, None, b"Tb is NULL"),
                       (7, None, b"params is NULL"), (8, None, b"out is NULL"), (1, 0, b"n_pairs must be > 0"),
                       (2, P(a.ctypes.data, None), b"pair 1: a is NULL"), (4, P(None, b.ctypes.data), b"pair 0: b is NULL"),
                       (3, U(8, 4097), b"pair 1: Ta = 4097"), (5, U(0, 9), b"pair 0: Tb = 0"), (6, 257, b"M = 257")):
        args = list(okb)
        args[i] = v
        assert lib.zv_mel_align_batch(*args) == 5 and b"zv_mel_align_batch: " + what in lib.zv_last_error(), lib.zv_last_error()


def test_plan_is_one_launch_per_kernel_and_groups_end_at_2_27_cells(exes):
    R, tile, qrows, chans = AR.constant("ALIGN_DP_ROWS"), AR.constant("ALIGN_TILE"), AR.constant("ALIGN_QUANT_ROWS"), AR.constant("ALIGN_SUM_CHANNELS")
    assert R >= 64 and R % 64 == 0 and tile % 16 == 0
    rows = [(1, 1, 1, 1), (1, 300, 41, 80), (32, 1024, 1024, 80), (5, 4096, 4096, 256), (3, 17, 4096, 65), (7, 4096, 1, 64),
            (0, 8, 8, 80), (1, 0, 8, 80), (1, 8, 0, 80), (1, 4097, 8, 80), (1, 8, 4097, 80), (1, 8, 8, 0), (1, 8, 8, 257)]
    r = subprocess.run([exes[0], "plan"], input="".join("%d %d %d %d\n" % x for x in rows), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = [tuple(map(int, line.split())) for line in r.stdout.splitlines()]
    up = lambda x, y: -(-x // y)
    for i, ((n, ta, tb, M), g) in enumerate(zip(rows, got)):
        assert g[0] == int(i < 6), (rows[i], g)
        if g[0]:        # ONE grid per kernel: the pairs (or the sequences, two per pair) are a grid dimension
            assert g[1:] == (up(M, chans), 2 * n, up(max(ta, tb), qrows), 2 * n, up(tb, tile), up(ta, tile), n, n, n), (rows[i], g)
    # launch groups: consecutive pairs while the cells stay within 2^27
    big = 4096 * 4096
    batches = [[(4096, 4096)] * 5, [(4096, 4096)] * 8, [(4096, 4096)] * 9, [(1, 1)] * 50, [(4096, 4096)] * 7 + [(4096, 4095), (1, 1), (4096, 1)],
               [(300, 41), (4096, 4096)] * 9, [(4096, 4096)] * 17]
    for batch in batches:
        text = f"{len(batch)}\n" + "".join("%d %d\n" % p for p in batch)
        r = subprocess.run([exes[0], "groups"], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        ends = list(map(int, r.stdout.split()))
        assert ends == AR.group_ends(*zip(*batch)), (batch[:3], ends)
        first = 0
        for e in ends:
            cells = sum(x * y for x, y in batch[first:e])
            assert e > first and cells <= AR.GROUP_CELLS and (e == len(batch) or cells + batch[e][0] * batch[e][1] > AR.GROUP_CELLS)
            first = e
    assert AR.GROUP_CELLS == 8 * big and AR.group_ends([4096] * 5, [4096] * 5) == [5] and AR.group_ends([4096] * 9, [4096] * 9) == [8, 9]
    # the dp pass: Tb + rows - 1 steps inside one pass, a pass every max(Tb, ALIGN_DP_ROWS) steps
    shapes = [(1, 1), (7, 300), (R, 5), (R + 1, 5), (R + 1, 4096), (2 * R + 1, R - 1), (4096, 4096)]
    r = subprocess.run([exes[0], "steps"], input="".join("%d %d\n" % s for s in shapes), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == ""
    want = [(up(ta, R) - 1) * max(tb, R) + tb + (ta - (up(ta, R) - 1) * R) - 1 for ta, tb in shapes]
    assert list(map(int, r.stdout.split())) == want


def test_cli_knows_its_flags_and_refuses_bad_files(tmp_path):
    """usage errors exit 2 before anything is loaded; a file that does not hold whole rows is refused by name ahead of the checkpoint"""
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    run = lambda *a: subprocess.run([cli, *a], capture_output=True, text=True, timeout=60)
    for flag in ("--align", "--mel-width", "--align-scale", "--align-normalise", "--map-out", "--time-like"):
        assert flag in run("--help").stdout, flag
    for args, word in ((("--align", "a.f32"), "--align"), (("--align", "a.f32", "b.f32"), "--mel-width"),
                       (("--align", "a.f32", "b.f32", "--mel-width", "0"), "--mel-width"), (("--align", "a.f32", "b.f32", "--mel-width", "257"), "--mel-width"),
                       (("--align", "a.f32", "b.f32", "--mel-width", "80", "--align-scale", "-1"), "--align-scale"),
                       (("--align", "a.f32", "b.f32", "--mel-width", "80", "--align-scale", "x"), "--align-scale"),
                       (("--mel-width", "80"), "need --align"), (("--align-normalise",), "need --align"), (("--map-out", "m.tsv"), "need --align"),
                       (("--align", "a.f32", "b.f32", "--mel-width", "80", "--time-like", "r.wav"), "exclude")):
        r = run(*args)
        assert r.returncode == 2 and word in r.stderr, (args, r.stderr[:300])
    good, ragged, empty = str(tmp_path / "good.f32"), str(tmp_path / "ragged.f32"), str(tmp_path / "empty.f32")
    np.zeros((5, 80), F).tofile(good)
    np.zeros(5 * 80 + 3, F).tofile(ragged)
    open(empty, "wb").close()
    for pa, pb, word in ((str(tmp_path / "missing.f32"), good, "cannot open"), (good, ragged, "whole rows"), (empty, good, "whole rows")):
        r = run("--align", pa, pb, "--mel-width", "80")
        assert r.returncode == 1 and "--align" in r.stderr and word in r.stderr, (pa, r.stderr[:300])
    long = str(tmp_path / "long.f32")
    np.zeros((4097, 2), F).tofile(long)
    r = run("--align", long, long, "--mel-width", "2")
    assert r.returncode == 1 and "--align" in r.stderr and "4097" in r.stderr, r.stderr[:300]
