"""-m gpu: mel alignment (include/zerovox_amd.h "mel alignment") on the device.  The five kernels depend on the rows, the sizes and the
call's parameters alone, so the smallest synthetic checkpoint ("tiny") serves every test.

Every expectation is the rule restated in Python (tests/align_rule.py): there is no tolerance anywhere, total, maps, path length and the
distance's bit pattern must match.
  * the shapes of the CPU test, sizes around the dp pass's ALIGN_DP_ROWS rows on either side and beyond it on both, sizes around the
    16 x 16 matrix tile, M of 1, 63, 64, 65, 80 and 256, one 1 024 x 1 024 x 80 pair;
  * the limits: one 4 096 x 4 096 x 80 pair with a known answer, and the refusals at 0 / 4 097 rows and 0 / 257 channels;
  * a ragged batch with NULL map entries whatever the neighbours hold, and a batch that crosses a launch group's 2^27 cells;
  * history independence: lane poisons and synthesize_batch calls around the call, graph mode on and off;
  * synthesize_like on the tiny model;
  * the command line: --align on two files of rows, --time-like on a reference file.

The known answer at the limits.  X holds 1 024 rows whose neighbours differ; A repeats row k of X r_k times, B repeats it s_k times, both
to 4 096 rows.  Row block k of A against column block k of B is an r_k x s_k block of zero cost and every other cell near the path costs
more, so total = 0 and distance = 0.  Each block is the repeated-rows case of tests/test_align_cpu.py in one or the other role (a
diagonal run of min(r_k, s_k) cells from the block's end, then the remaining rows in its first column or the remaining columns in its
first row, because (i-1, j-1) is examined first and wins ties): path_len = sum of max(r_k, s_k), and inside block k, with d = r_k - s_k,
map_a of row u is max(u - d, 0) for d >= 0 and u - d for u > 0 (0 for u = 0) otherwise; map_b is the same with the roles swapped.
test_known_answer_formula_at_a_small_size holds the formula to the restatement on the CPU side of this file's helpers."""
import ctypes as C

import numpy as np
import pytest

import align_rule as AR
from test_align_cpu import distinct_rows, mel_like, tie_rich, _inputs

pytestmark = pytest.mark.gpu

_M = {}
F = np.float32
R = AR.constant("ALIGN_DP_ROWS")


@pytest.fixture(scope="module")
def env(ckpt):
    from zerovox_cpp_amd import capi
    if "m" not in _M:
        path, g, tensors = ckpt("tiny")
        _M.update(m=capi.Model(path, 0), g=g, path=path)
    _M["m"].set_graph_mode(False)
    yield _M["m"]


def teardown_module(module):
    if "m" in _M:
        _M["m"].close()
    _M.clear()


def _dbits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def _same(what, have, want):
    """have: an Alignment; want: the restatement's tuple or another Alignment"""
    if not isinstance(want, tuple):
        want = (want.total, want.distance, want.path_len, want.map_a, want.map_b)
    total, dist, L, ma, mb = want
    assert have.total == total and have.path_len == L, (what, have, want[:3])
    assert _dbits(have.distance) == _dbits(dist), (what, have.distance, dist)
    for name, h, w in (("map_a", have.map_a, ma), ("map_b", have.map_b, mb)):
        if h is not None:
            bad = np.argwhere(np.asarray(h) != np.asarray(w))
            assert h.shape == w.shape and bad.size == 0, (what, name, len(bad), bad[:4])


def _pair(seed, Ta, Tb, M, kind):
    rng = np.random.default_rng(seed)
    if kind == "ties":
        both = tie_rich(rng, Ta + Tb, M)
        return both[:Ta], both[Ta:]
    return _inputs(rng, kind, Ta, M), _inputs(rng, kind, Tb, M)


KINDS = ("random", "ties", "specials", "clamp")


# ---- 1. bit for bit against the restatement ---------------------------------------------------------------------------------------

BASIC = [(1, 1), (1, 7), (7, 1), (16, 16), (17, 33), (64, 65), (300, 41)]
TILE = [(15, 17), (16, 15), (17, 16), (15, 15), (17, 17)]
BLOCK = [(R - 1, 33), (R, 33), (R + 1, 33), (2 * R + 1, 33), (33, R - 1), (33, R), (33, R + 1), (33, 2 * R + 1), (R + 1, R + 6), (2 * R + 1, R + 1)]


@pytest.mark.parametrize("M", [1, 63, 64, 65, 80, 256])
def test_shapes_and_widths(env, M):
    from zerovox_cpp_amd import capi
    for k, (Ta, Tb) in enumerate(BASIC + TILE):
        for normalise in (0, 1):
            kind = KINDS[(k + normalise) % 4]
            a, b = _pair(1000 * M + 2 * k + normalise, Ta, Tb, M, kind)
            scale = (0.0, 25.0)[k % 2]
            _same((Ta, Tb, M, kind, normalise), env.mel_align(a, b, capi.AlignParams(scale, normalise)), AR.align(a, b, scale, normalise))


@pytest.mark.parametrize("Ta,Tb", BLOCK)
def test_sizes_around_the_dp_pass(env, Ta, Tb):
    from zerovox_cpp_amd import capi
    for normalise, kind in ((0, "ties"), (1, "random")):
        a, b = _pair(Ta * 7 + Tb + normalise, Ta, Tb, 80, kind)
        _same((Ta, Tb, kind), env.mel_align(a, b, capi.AlignParams(0.0, normalise)), AR.align(a, b, 0.0, normalise))


def test_a_1024_x_1024_x_80_pair(env):
    from zerovox_cpp_amd import capi
    rng = np.random.default_rng(1024)
    a = mel_like(rng, 1024, 80)
    b = a[np.sort(rng.integers(0, 1024, 1024))] + (rng.standard_normal((1024, 80)) * 0.2).astype(F)      # a re-timed, noisy take of a
    _same("1024", env.mel_align(a, b, capi.AlignParams(normalise=True)), AR.align(a, b, 0.0, 1))


# ---- 2. the limits ----------------------------------------------------------------------------------------------------------------

def block_answer(r, s):
    """the known answer of rep(X, r) against rep(X, s) (the module's docstring) -> (path_len, map_a, map_b)"""
    def side(r, s):
        out, col0 = [], 0
        for rk, sk in zip(r, s):
            d = rk - sk
            u = np.arange(rk)
            out.append(col0 + (np.maximum(u - d, 0) if d >= 0 else np.where(u > 0, u - d, 0)))
            col0 += sk
        return np.concatenate(out).astype(np.int32)
    return int(np.maximum(r, s).sum()), side(r, s), side(s, r)


def _limits_pair():
    if "limits" not in _M:
        rng = np.random.default_rng(4096)
        X = distinct_rows(rng, 1024, 80)
        r = np.tile([3, 5, 4, 4, 1, 7, 6, 2], 128)
        s = np.tile([5, 3, 4, 4, 7, 1, 2, 6], 128)
        assert r.sum() == 4096 and s.sum() == 4096
        _M["limits"] = (AR.repeated(X, r)[0], AR.repeated(X, s)[0], block_answer(r, s))
    return _M["limits"]


def test_known_answer_formula_at_a_small_size():
    rng = np.random.default_rng(5)
    X = distinct_rows(rng, 24, 7)
    r, s = rng.integers(1, 6, 24), rng.integers(1, 6, 24)
    total, dist, L, ma, mb = AR.align(AR.repeated(X, r)[0], AR.repeated(X, s)[0])
    wl, wa, wb = block_answer(r, s)
    assert (total, dist, L) == (0, 0.0, wl) and np.array_equal(ma, wa) and np.array_equal(mb, wb)


def test_a_4096_x_4096_x_80_pair_with_the_known_answer(env):
    a, b, (L, ma, mb) = _limits_pair()
    assert a.shape == b.shape == (AR.MAX_FRAMES, 80)
    got = env.mel_align(a, b)
    _same("limits", got, (0, 0.0, L, ma, mb))
    _M["limits_got"] = got


def test_sizes_beyond_the_limits_are_refused(env):
    from zerovox_cpp_amd import capi
    ok = np.zeros((5, 80), F)
    for a, b, word in ((np.zeros((0, 80), F), ok, "Ta = 0"), (np.zeros((4097, 80), F), ok, "Ta = 4097"), (ok, np.zeros((0, 80), F), "Tb = 0"),
                       (ok, np.zeros((4097, 80), F), "Tb = 4097"), (np.zeros((5, 0), F), np.zeros((5, 0), F), "M = 0"),
                       (np.zeros((5, 257), F), np.zeros((5, 257), F), "M = 257")):
        for call, name in ((lambda: env.mel_align(a, b), "zv_mel_align:"), (lambda: env.mel_align_batch([(ok, ok), (a, b)]) if a.shape[1] == 80 else
                                                                             env.mel_align_batch([(a, b)]), "zv_mel_align_batch:")):
            with pytest.raises(capi.ZvError) as e:
                call()
            assert e.value.status == 5 and name in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(capi.ZvError) as e:
        env.mel_align_batch([(ok, ok), (ok, np.zeros((4097, 80), F))])
    assert "zv_mel_align_batch: pair 1: Tb = 4097" in str(e.value)
    for p, word in ((capi.AlignParams(-1.0), "align scale"), (capi.AlignParams(float("inf")), "align scale"), (capi.AlignParams(0.0, 2), "align normalise = 2")):
        with pytest.raises(capi.ZvError) as e:
            env.mel_align(ok, ok, p)
        assert e.value.status == 5 and word in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        env.mel_align(ok, np.zeros((5, 79), F))
    with pytest.raises(TypeError):
        env.mel_align(ok, ok, dict(scale=1.0))
    _same("a call after the refusals", env.mel_align(ok, ok), (0, 0.0, 5, np.arange(5), np.arange(5)))


# ---- 3. batches -------------------------------------------------------------------------------------------------------------------

def _raw_batch(m, pairs, params, no_map_a=(), no_map_b=()):
    """zv_mel_align_batch through ctypes, with NULL entries in the map arrays -> Alignments whose missing maps are None"""
    from zerovox_cpp_amd import capi
    n = len(pairs)
    rows = [(np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)) for a, b in pairs]
    mas = [None if k in no_map_a else np.full(a.shape[0], -7, np.int32) for k, (a, _) in enumerate(rows)]
    mbs = [None if k in no_map_b else np.full(b.shape[0], -7, np.int32) for k, (_, b) in enumerate(rows)]
    P, U = C.c_void_p * n, C.c_uint32 * n
    st, out = params.struct, (capi.AlignmentC * n)()
    ptr = lambda x: None if x is None else x.ctypes.data
    m._chk(m.lib.zv_mel_align_batch(m.h, n, P(*[a.ctypes.data for a, _ in rows]), U(*[a.shape[0] for a, _ in rows]), P(*[b.ctypes.data for _, b in rows]),
                                    U(*[b.shape[0] for _, b in rows]), rows[0][0].shape[1], C.byref(st), out, P(*map(ptr, mas)), P(*map(ptr, mbs))))
    return [capi.Alignment(o.total, o.distance, o.path_len, ma, mb) for o, ma, mb in zip(out, mas, mbs)]


RAGGED = [(1, 1), (300, 41), (7, 1), (17, 33), (1, 7), (64, 65), (16, 16), (41, 300)]


@pytest.mark.parametrize("normalise", [0, 1])
def test_ragged_batch_equals_single_calls_whatever_the_neighbours_hold(env, normalise):
    from zerovox_cpp_amd import capi
    p = capi.AlignParams(0.0, normalise)
    pairs = [_pair(50 + k, Ta, Tb, 80, KINDS[k % 4]) for k, (Ta, Tb) in enumerate(RAGGED)]
    single = [env.mel_align(a, b, p) for a, b in pairs]
    for k, (a, b) in enumerate(pairs):
        _same(("single", k), single[k], AR.align(a, b, 0.0, normalise))
    for k, got in enumerate(env.mel_align_batch(pairs, p)):
        _same(("batch", k), got, single[k])
    got = _raw_batch(env, pairs, p, no_map_a=(0, 3, 4), no_map_b=(1, 3, 7))
    for k, g in enumerate(got):
        assert (g.map_a is None) == (k in (0, 3, 4)) and (g.map_b is None) == (k in (1, 3, 7))
        _same(("NULL entries", k), g, single[k])
    # a pair's result does not move when its neighbours' rows do
    rng = np.random.default_rng(8)
    for k in range(len(pairs)):
        other = [(a, b) if v == k else (mel_like(rng, *a.shape) * F(3.0), np.full_like(b, 9.0)) for v, (a, b) in enumerate(pairs)]
        _same(("neighbours", k), env.mel_align_batch(other, p)[k], single[k])
    # the whole arrays may be NULL as well
    m = env
    n = len(pairs)
    P, U = C.c_void_p * n, C.c_uint32 * n
    st, out = p.struct, (capi.AlignmentC * n)()
    m._chk(m.lib.zv_mel_align_batch(m.h, n, P(*[a.ctypes.data for a, _ in pairs]), U(*[a.shape[0] for a, _ in pairs]), P(*[b.ctypes.data for _, b in pairs]),
                                    U(*[b.shape[0] for _, b in pairs]), 80, C.byref(st), out, None, None))
    assert [(o.total, _dbits(o.distance), o.path_len) for o in out] == [(s.total, _dbits(s.distance), s.path_len) for s in single]


def test_a_batch_across_a_launch_group_boundary(env):
    """nine pairs of 4 096 x 4 096 hold 9 * 2^24 cells, more than a group's 2^27: eight run as one group, then the small pair and the
    ninth as another; every pair has the bits of its single call"""
    from zerovox_cpp_amd import capi
    a, b, (L, ma, mb) = _limits_pair()
    big = _M.get("limits_got") or env.mel_align(a, b)
    sa, sb = _pair(99, 300, 41, 80, "random")
    small = env.mel_align(sa, sb)
    _same("small", small, AR.align(sa, sb))
    pairs = [(a, b)] * 8 + [(sa, sb), (a, b)]
    assert AR.group_ends([x.shape[0] for x, _ in pairs], [y.shape[0] for _, y in pairs]) == [8, 10]
    got = env.mel_align_batch(pairs)
    for k, g in enumerate(got):
        _same(("across groups", k), g, small if k == 8 else big)
    assert got[9].path_len == L and np.array_equal(got[9].map_a, ma)


# ---- 4. history independence ------------------------------------------------------------------------------------------------------

def _utterances(g):
    from zerovox_cpp_amd import synth
    return [(*synth.encoder_inputs(g, 8100 + i, N), T) for i, (N, T) in enumerate(((6, 40), (3, 17), (9, 64)))]


def test_poisoned_lane_and_calls_around_it_leave_the_bits_unchanged(env):
    from zerovox_cpp_amd import capi
    m, g = env, _M["g"]
    p = capi.AlignParams(0.0, 1)
    pairs = [_pair(70 + k, Ta, Tb, 80, KINDS[k % 4]) for k, (Ta, Tb) in enumerate(((300, 41), (R + 1, 33), (17, 16)))]
    want = [AR.align(a, b, 0.0, 1) for a, b in pairs]
    first = m.mel_align_batch(pairs, p)
    for k in range(3):
        _same(("first", k), first[k], want[k])
    for byte in (0x00, 0xFF):
        m.poison(byte, 0)
        for k, got in enumerate(m.mel_align_batch(pairs, p)):
            _same(("poison", byte, k), got, want[k])
        m.poison(byte, 0)
        _same(("poison, single", byte), m.mel_align(*pairs[1], p), want[1])
    utts = _utterances(g)
    for graph in (False, True):
        m.set_graph_mode(graph)
        before = m.synthesize_batch(utts)
        for k, got in enumerate(m.mel_align_batch(pairs, p)):
            _same(("between batches", graph, k), got, want[k])
        after = m.synthesize_batch(utts)
        _same(("after a batch", graph), m.mel_align(*pairs[0], p), want[0])
        again = m.synthesize_batch(utts)
        for (w0, n0), (w1, n1), (w2, n2) in zip(before, after, again):
            assert n0 == n1 == n2 and np.array_equal(AR.bits(w0), AR.bits(w1)) and np.array_equal(AR.bits(w0), AR.bits(w2)), graph
    m.set_graph_mode(False)
    eager = m.synthesize_batch(utts)
    for (w0, n0), (w1, n1) in zip(eager, again):
        assert n0 == n1 and np.array_equal(AR.bits(w0), AR.bits(w1))


# ---- 5. the timing transfer, end to end -------------------------------------------------------------------------------------------

def test_synthesize_like(env):
    from zerovox_cpp_amd import capi, synth
    m, g = env, _M["g"]
    hop, T = g.hop_size, g.max_seq_len
    ids, puncts, style = synth.encoder_inputs(g, 8200, 6)
    forced = np.array([4, 9, 0, 12, 7, 5], np.int32)                     # D*: the reference's timing, a zero-length phoneme included
    Tb = int(forced.sum())
    ref, nf_ref = m.synthesize(ids, puncts, style, Tb, phonemes=dict(duration_frames=forced), fitted=True)
    assert nf_ref == Tb
    ref = np.concatenate([ref[:Tb * hop], np.zeros(hop // 2, F)])         # samples behind the last whole hop are dropped
    wav, nf, dur_b, al = m.synthesize_like(ids, puncts, style, T, ref)
    assert nf == Tb and wav.shape == (Tb * hop,) and dur_b.dtype == np.int32 and dur_b.sum() == Tb and (dur_b >= 0).all()
    # its own intermediate results, made again call by call
    own, nf_a, dur_a = m.synthesize(ids, puncts, style, T, fitted=True, return_durations=True)
    mel = capi.MelAnalysis(log="ln")
    rows_a, rows_b = m.mel_wave_batch([own[:nf_a * hop], ref[:Tb * hop]], mel)
    al2 = m.mel_align(rows_a, rows_b, capi.AlignParams(normalise=True))
    _same("the call's alignment", al, al2)
    _same("against the restatement", al, AR.align(rows_a, rows_b, 0.0, 1))
    assert np.array_equal(dur_b, capi.align_durations(dur_a, al.map_a, Tb)) and np.array_equal(dur_b, AR.durations(dur_a, al.map_a, Tb))
    plain, nf_p = m.synthesize(ids, puncts, style, Tb, phonemes=dict(duration_frames=dur_b), fitted=True)
    assert nf_p == Tb and np.array_equal(AR.bits(wav), AR.bits(plain))
    print("synthesize_like on the tiny model: sum |d_b - D*| = %d over %d frames, distance %.6f" % (int(np.abs(dur_b - forced).sum()), Tb, al.distance))
    # the reference against itself
    self_ = m.mel_align(rows_b, rows_b, capi.AlignParams(normalise=True))
    assert self_.total == 0 and self_.distance == 0.0 and self_.path_len == Tb and np.array_equal(self_.map_a, np.arange(Tb))
    # controls pass through; a duration among them is refused
    wav_c, nf_c, _, _ = m.synthesize_like(ids, puncts, style, T, ref, volume=(0.5, 0.0, 0.0))
    assert nf_c == Tb and not np.array_equal(AR.bits(wav_c), AR.bits(wav))
    with pytest.raises(ValueError):
        m.synthesize_like(ids, puncts, style, T, ref, phonemes=dict(duration_frames=forced))
    with pytest.raises(TypeError):
        m.synthesize_like(ids, puncts, style, T, ref, target_frames=20)


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------

def test_cli_aligns_files_and_follows_a_reference(env, tmp_path):
    """zerovox --align on two files of raw rows prints what mel_align returns and writes the maps; --time-like follows a reference the
    model made itself, written as the PCM16 file zv_write_wav writes"""
    import os
    import re
    import subprocess
    import wave
    from zerovox_cpp_amd import capi, synth
    m, g = env, _M["g"]
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zerovox.cpp_amd", "zerovox")
    a, b = _pair(123, 57, 41, 80, "random")
    pa, pb, pm = str(tmp_path / "a.f32"), str(tmp_path / "b.f32"), str(tmp_path / "map.tsv")
    a.tofile(pa), b.tofile(pb)
    r = subprocess.run([cli, "-m", _M["path"], "--align", pa, pb, "--mel-width", "80", "--align-normalise", "--align-scale", "32", "--map-out", pm],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    want = m.mel_align(a, b, capi.AlignParams(32.0, True))
    _same("the library against the restatement", want, AR.align(a, b, 32.0, 1))
    got = re.search(r"total (\d+) path_len (\d+) distance (\S+)", r.stdout)
    assert got and (int(got.group(1)), int(got.group(2))) == (want.total, want.path_len) and float(got.group(3)) == want.distance, r.stdout
    rows = [line.split("\t") for line in open(pm).read().splitlines()[1:]]
    assert [int(x[2]) for x in rows if x[0] == "a"] == want.map_a.tolist() and [int(x[2]) for x in rows if x[0] == "b"] == want.map_b.tolist()
    # --time-like
    hop, T = g.hop_size, g.max_seq_len
    ids, puncts, _ = synth.encoder_inputs(g, 8300, 6)
    style = np.zeros(g.E, F)
    forced = np.array([6, 3, 10, 0, 8, 4], np.int32)
    Tb = int(forced.sum())
    ref, _ = m.synthesize(ids, puncts, style, Tb, phonemes=dict(duration_frames=forced), fitted=True)
    src, out, utt = str(tmp_path / "ref.wav"), str(tmp_path / "out.wav"), str(tmp_path / "utt.txt")
    assert m.lib.zv_write_wav(src.encode(), ref.ctypes.data, Tb * hop, g.sampling_rate) == 0
    with wave.open(src, "rb") as w:
        pcm = np.frombuffer(w.readframes(Tb * hop), "<i2").astype(F) / F(32768.0)
    open(utt, "w").write(" ".join(map(str, ids)) + "\n" + " ".join(map(str, puncts)) + "\n0\n")
    r = subprocess.run([cli, "-m", _M["path"], "-u", utt, "-o", out, "--time-like", src], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    _, nf, dur_b, al = m.synthesize_like(ids, puncts, style, T, pcm)
    got = re.search(r"time-like: (\d+) frames, alignment total (\d+) path_len (\d+)", r.stdout)
    assert got and tuple(map(int, got.groups())) == (Tb, al.total, al.path_len) and nf == Tb, (r.stdout, al)
    with wave.open(out, "rb") as w:
        assert w.getnchannels() == 1 and w.getframerate() == g.sampling_rate and w.getnframes() == Tb * hop
    r = subprocess.run([cli, "-m", _M["path"], "-u", utt, "-o", out, "--time-like", str(tmp_path / "missing.wav")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--time-like" in r.stderr and "cannot open" in r.stderr, r.stderr[-500:]
