"""-m gpu: fitted synthesis (include/zerovox_amd.h zv_synthesize_fitted): the decoder and the vocoder run over the n_frames the length
regulator fills instead of the capacity T.

The contract is bit equality with the existing unfitted entry points at T = n_frames, so every comparison below is
np.array_equal; no tolerance appears anywhere.  For an utterance with frame count nf under capacity T:
    fitted wav[: nf * hop] == unfitted call of the same kind at T = nf,   wav[nf * hop :] == 0,   n_frames == nf,
    durations equal (they sum to nf).
Lengths are made deterministic with duration_frames (forced frames per phoneme) where a case needs a particular nf.  A lane's
buffers keep the previous call's waveform, live table and zeroed tail at offsets that depend on the shapes alone, so the lane is
poisoned (zv_debug_poison, _poison below) before every fitted call of sections 1 to 7.  Checked:
  * single calls, eager and graph: nf at and around the 32-row statistics blocks and the 64 / 256-row tiles, capacities 64-aligned
    and not;
  * predicted durations under duration_scale 0.5 / 1 / 2: fitted call first, then the unfitted call at the n_frames it returned;
  * nf == T (forced total above the capacity, duration_scale = 16) and nf == 0 (alone and between neighbours in a batch);
  * ragged batches with and without prosody / per-phoneme controls / timings == stand-alone fitted == unfitted at n_frames[u];
    under graph replay a second set of controls changes every length under the same capacities;
  * a batch split into tail groups, and a fitted and an unfitted batch in flight on two lanes;
  * the fitted batch under every kernel-regime switch of tests/test_gpu_batch_edges.py;
  * two other geometries (residual-block taps; encoder / decoder widths and mel count);
  * the CLI's --fit against the unfitted run of a checkpoint whose max_seq_len is n_frames; --trim keeps its bits."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_M = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def env(ckpt):
    from zerovox_cpp_amd import capi
    if "m" not in _M:
        path, g, tensors = ckpt("medium")
        _M.update(m=capi.Model(path, 0), g=g, t=tensors, path=path)
    _M["m"].set_graph_mode(False)
    yield _M["m"], _M["g"], _M["t"]
    _M["m"].set_graph_mode(False)


def teardown_module(module):
    if "m" in _M:
        _M["m"].close()
    _M.clear()


def _utt(g, seed, N):
    from zerovox_cpp_amd import synth
    return synth.encoder_inputs(g, seed, N)


def _forced(N, total):
    """duration_frames [N] that sum to `total`, as even as integers allow (some are 0 when total < N)"""
    return (total // N + (np.arange(N) < total % N)).astype(np.int32)


def _poison(m, lane=0):
    """fills what the lane keeps between calls, 0xFF and 0x3C bytes in turn (tests/test_gpu_poison.py says why these two)"""
    _M["fill"] = 0xFF ^ 0x3C ^ _M.get("fill", 0x3C)
    m.poison(_M["fill"], lane)


def _check_fitted(hop, got, ref, T, what):
    """got: (wav, n_frames, durations) of a fitted call under capacity T; ref: the unfitted call at T = n_frames, or None when
    n_frames == 0"""
    w, nf, d = got
    assert w.shape == (T * hop,), what
    assert int(d.sum()) == nf, (what, "durations sum")
    if ref is None:
        assert nf == 0 and not w.any(), (what, "empty utterance")
        return
    wr, nfr, dr = ref
    assert nf == nfr and wr.shape == (nf * hop,), (what, nf, nfr)
    assert np.array_equal(w[: nf * hop], wr), (what, "live samples")
    assert not np.isnan(w[nf * hop:]).any() and not w[nf * hop:].any(), (what, "tail is not zero")
    assert np.array_equal(d, dr), (what, "durations")


# ---- 1. single calls at forced lengths --------------------------------------------------------------------------------------

FORCED_NF = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_single_forced_lengths(env, graph):
    m, g, _ = env
    hop, N = g.hop_size, 24
    ids, puncts, style = _utt(g, 901, N)
    refs = {}
    for nf in FORCED_NF:
        refs[nf] = m.synthesize(ids, puncts, style, nf, phonemes=dict(duration_frames=_forced(N, nf)), return_durations=True)
        assert refs[nf][1] == nf
    m.set_graph_mode(graph)
    for nf in FORCED_NF:
        pc = dict(duration_frames=_forced(N, nf))
        for T in (nf + 1, 2 * nf + 7, 1024, (nf + 64) // 64 * 64):
            for rep in range(2 if graph else 1):            # graph: capture, then replay
                _poison(m)
                got = m.synthesize(ids, puncts, style, T, phonemes=pc, return_durations=True, fitted=True)
                _check_fitted(hop, got, refs[nf], T, (nf, T, graph, rep))


# ---- 2. predicted durations -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_single_predicted_durations(env, graph):
    m, g, _ = env
    hop, skipped, cases = g.hop_size, 0, 0
    for seed, N, T in ((21, 40, 1500), (22, 7, 300), (23, 200, 1500), (24, 1100, 1437), (25, 1, 64)):
        ids, puncts, style = _utt(g, seed, N)
        for ds in (0.5, 1.0, 2.0):
            pr = dict(duration_scale=ds)
            m.set_graph_mode(graph)
            _poison(m)
            w, nf = m.synthesize(ids, puncts, style, T, prosody=pr, fitted=True)          # no per-phoneme arguments at all
            _poison(m)
            got = m.synthesize(ids, puncts, style, T, prosody=pr, return_durations=True, fitted=True)
            assert got[1] == nf and np.array_equal(got[0], w)
            m.set_graph_mode(False)
            cases += 1
            if nf == 0:
                skipped += 1
                continue
            ref = m.synthesize(ids, puncts, style, nf, prosody=pr, return_durations=True)
            _check_fitted(hop, got, ref, T, (seed, N, T, ds))
            if ds == 1.0:                                   # the plain form, too
                wp, nfp = m.synthesize(ids, puncts, style, nf)
                assert nfp == nf and np.array_equal(w[: nf * hop], wp)
    assert skipped <= 1 and cases == 15, (skipped, cases)


# ---- 3. nf == T -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_full_capacity_gives_the_unfitted_bits(env, graph):
    m, g, _ = env
    N = 30
    ids, puncts, style = _utt(g, 31, N)
    for T, kw in ((200, dict(phonemes=dict(duration_frames=_forced(N, 333)))),          # forced total above the capacity
                  (96, dict(prosody=dict(duration_scale=16.0))),
                  (257, dict(phonemes=dict(duration_frames=_forced(N, 257))))):         # exactly the capacity
        m.set_graph_mode(False)
        ref = m.synthesize(ids, puncts, style, T, return_durations=True, **kw)
        assert ref[1] == T, (T, ref[1])
        m.set_graph_mode(graph)
        for rep in range(2 if graph else 1):
            _poison(m)
            got = m.synthesize(ids, puncts, style, T, return_durations=True, fitted=True, **kw)
            assert got[1] == T and np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]), (T, rep)


# ---- 4. nf == 0 -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_empty_utterance_alone_and_between_neighbours(env, graph):
    m, g, _ = env
    hop, N, T = g.hop_size, 12, 130
    ids, puncts, style = _utt(g, 41, N)
    zero = dict(duration_frames=np.zeros(N, np.int32))
    before = m.synthesize(ids, puncts, style, T, return_durations=True)
    m.set_graph_mode(graph)
    for rep in range(2):
        _poison(m)
        got = m.synthesize(ids, puncts, style, T, phonemes=zero, return_durations=True, fitted=True)
        _check_fitted(hop, got, None, T, ("alone", rep))
        # the model still gives correct bits on the next call, fitted (same capacity: the same graph, another table) and unfitted
        _poison(m)
        nxt = m.synthesize(ids, puncts, style, T, phonemes=dict(duration_frames=_forced(N, 77)), return_durations=True, fitted=True)
        assert nxt[1] == 77
        after = m.synthesize(ids, puncts, style, T, return_durations=True)
        assert after[1] == before[1] and np.array_equal(after[0], before[0])
    m.set_graph_mode(False)
    ref77 = m.synthesize(ids, puncts, style, 77, phonemes=dict(duration_frames=_forced(N, 77)), return_durations=True)
    _check_fitted(hop, nxt, ref77, T, "after the empty call")
    # in a batch: the empty utterance first, in the middle and last
    nbrs = [(*_utt(g, 42 + i, n), t) for i, (n, t) in enumerate(((20, 300), (5, 64), (64, 700)))]
    alone = [(_poison(m), m.synthesize(*u, return_durations=True, fitted=True))[1] for u in nbrs]
    empty = (ids, puncts, style, T, None, zero)
    for pos in (0, 1, 3):
        utts = [u + (None, None) for u in nbrs]
        utts.insert(pos, empty)
        m.set_graph_mode(graph)
        bc = m.prepare_batch(utts, durations=True, fitted=True)
        for rep in range(2):
            for w in bc.wavs:
                w[:] = NAN
            _poison(m)
            bc.run()
            res = [r + (d,) for r, d in zip(bc.results(), bc.durations)]
            _check_fitted(hop, res.pop(pos), None, T, ("batch", pos, rep))
            for i, (r, a) in enumerate(zip(res, alone)):
                assert r[1] == a[1] and np.array_equal(r[0], a[0]) and np.array_equal(r[2], a[2]), ("neighbour", pos, i, rep)
        m.set_graph_mode(False)


# ---- 5. ragged batches ------------------------------------------------------------------------------------------------------

PROSODIES = [None, dict(duration_scale=1.3, pitch_scale=0.9, pitch_shift=0.05, energy_scale=1.1, energy_shift=-0.03)]
RAGGED_NT = [(200, 1500), (7, 60), (300, 1200), (1, 11), (40, 1), (64, 257), (1100, 1437), (33, 640)]


def _controls(rng, n, total):
    """per-phoneme controls of an utterance: forced frames that sum to `total` (None: predicted durations, some of them scaled),
    local pitch / energy shifts"""
    c = dict(pitch_shift=rng.uniform(-0.2, 0.2, n).astype(np.float32), energy_shift=rng.uniform(-0.2, 0.2, n).astype(np.float32))
    if total is None:
        c["duration_scale"] = np.where(rng.random(n) < 0.5, rng.uniform(0.3, 3.0, n), 1.0).astype(np.float32)
    else:
        c["duration_frames"] = _forced(n, total)
    return c


def _ragged_sets(g):
    base = [(*_utt(g, 300 + i, N), T) for i, (N, T) in enumerate(RAGGED_NT)]
    rng = np.random.default_rng(17)
    prs = [PROSODIES[i % 2] for i in range(len(base))]
    # forced totals from one frame to the full capacity (and beyond it), predicted lengths, and utterances without controls
    tot1 = [1, 60, None, 11, 1, 130, None, "none"]
    tot2 = [1499, 1, 777, 3, 0, 257, 1100, 100]
    mk = lambda tot: [None if t == "none" else _controls(rng, len(u[0]), t) for u, t in zip(base, tot)]
    return base, prs, mk(tot1), mk(tot2)


def _alone_fitted(m, base, prs, pcs):
    return [(_poison(m), m.synthesize(*u, prosody=p, phonemes=c, return_durations=True, fitted=True))[1] for u, p, c in zip(base, prs, pcs)]


def _alone_unfitted(m, base, prs, pcs, fitted):
    return [None if f[1] == 0 else m.synthesize(*u[:3], f[1], prosody=p, phonemes=c, return_durations=True)
            for u, p, c, f in zip(base, prs, pcs, fitted)]


def _batch_results(bc):
    for w in bc.wavs:
        w[:] = NAN
    _poison(bc.model)
    bc.run()
    return [r + (d,) for r, d in zip(bc.results(), bc.durations)]


def _same_as(hop, res, base, fitted, unfitted, what):
    for i, (r, u, f, rf) in enumerate(zip(res, base, fitted, unfitted)):
        assert r[1] == f[1] and np.array_equal(r[0], f[0]) and np.array_equal(r[2], f[2]), (what, i, "stand-alone fitted")
        _check_fitted(hop, r, rf, u[3], (what, i))


def test_ragged_batch_eager_graph_and_replay_with_new_lengths(env):
    m, g, _ = env
    hop = g.hop_size
    base, prs, pc1, pc2 = _ragged_sets(g)
    f1, f2 = _alone_fitted(m, base, prs, pc1), _alone_fitted(m, base, prs, pc2)
    u1, u2 = _alone_unfitted(m, base, prs, pc1, f1), _alone_unfitted(m, base, prs, pc2, f2)
    nf1, nf2 = [f[1] for f in f1], [f[1] for f in f2]
    assert nf1[0] == 1 and nf1[1] == 60 and nf1[4] == 1 and nf2[0] == 1499 and nf2[4] == 0 and nf2[5] == 257, (nf1, nf2)
    assert all(a != b for a, b in zip(nf1, nf2)), ("the second set must change every length", nf1, nf2)
    bc = m.prepare_batch([u + (p, c) for u, p, c in zip(base, prs, pc1)], durations=True, fitted=True)
    _same_as(hop, _batch_results(bc), base, f1, u1, "eager")
    m.set_graph_mode(True)
    _same_as(hop, _batch_results(bc), base, f1, u1, "graph capture")
    _same_as(hop, _batch_results(bc), base, f1, u1, "graph replay")
    for i, c in enumerate(pc2):
        bc.set_phoneme_controls(i, c)
    _same_as(hop, _batch_results(bc), base, f2, u2, "graph replay, new lengths under the same capacities")
    for i, c in enumerate(pc1):
        bc.set_phoneme_controls(i, c)
    _same_as(hop, _batch_results(bc), base, f1, u1, "graph replay, back to the first lengths")
    for w in bc.wavs:
        w[:] = NAN
    _poison(m, 2)
    bc.begin(2)
    bc.end(2)
    _same_as(hop, [r + (d,) for r, d in zip(bc.results(), bc.durations)], base, f1, u1, "begin / end, graph")
    m.set_graph_mode(False)
    # without prosody, controls or timings: the NULL arguments of the fitted entry point
    _poison(m)
    plain = m.synthesize_batch([u for u in base], fitted=True)
    for i, (u, (w, nf)) in enumerate(zip(base, plain)):
        _poison(m)
        wa, nfa = m.synthesize(*u, fitted=True)
        assert nf == nfa and np.array_equal(w, wa), ("plain", i)
        if nf:
            wr, nfr = m.synthesize(*u[:3], nf)
            assert nfr == nf and np.array_equal(w[: nf * hop], wr) and not w[nf * hop:].any(), ("plain", i)


# ---- 6. tail groups and lanes -----------------------------------------------------------------------------------------------

def _big(g, seed0):
    """16 utterances of up to 1 500 frames of capacity (>= 16 MB of waveform: the last vocoder stage runs in utterance groups);
    lengths from a frame to the capacity"""
    utts = [(*_utt(g, seed0 + i, N), T) for i, (N, T) in enumerate([(150 + 13 * i, 1500 - 7 * i) for i in range(16)])]
    rng = np.random.default_rng(seed0)
    totals = [None, 1, 700, None, 1500, 64, None, 333, 0, None, 1024, 31, None, 257, 900, 2000]
    pcs = [_controls(rng, len(u[0]), t) for u, t in zip(utts, totals)]
    return utts, pcs


def test_batch_split_into_tail_groups(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop = g.hop_size
    utts, pcs = _big(g, 500)
    assert sum(u[3] for u in utts) * hop * 4 >= 16 << 20 and capi.debug_get("ZV_TAIL_GROUPS") > 1
    prs = [None] * 16
    fit = _alone_fitted(m, utts, prs, pcs)
    unf = _alone_unfitted(m, utts, prs, pcs, fit)
    assert fit[8][1] == 0 and fit[4][1] == utts[4][3] and fit[15][1] == utts[15][3]
    for graph in (False, True):
        m.set_graph_mode(graph)
        bc = m.prepare_batch([u + (None, c) for u, c in zip(utts, pcs)], durations=True, fitted=True)
        for rep in range(2 if graph else 1):
            _same_as(hop, _batch_results(bc), utts, fit, unf, f"tail groups, graph={graph}, rep={rep}")
    m.set_graph_mode(False)


def test_fitted_and_unfitted_lanes_in_flight(env):
    m, g, _ = env
    hop = g.hop_size
    utts, pcs = _big(g, 700)
    prs = [None] * 16
    fit = _alone_fitted(m, utts, prs, pcs)
    unf = _alone_unfitted(m, utts, prs, pcs, fit)
    cap = [m.synthesize(*u, phonemes=c, return_durations=True) for u, c in zip(utts, pcs)]       # the unfitted batch's references
    for graph in (False, True):
        m.set_graph_mode(graph)
        bf = [m.prepare_batch([u + (None, c) for u, c in zip(utts, pcs)], durations=True, fitted=True) for _ in range(2)]
        bu = [m.prepare_batch([u + (None, c) for u, c in zip(utts, pcs)], durations=True) for _ in range(2)]
        order = [bf[0], bu[0], bf[1], bu[1]]                # lanes 0, 1, 0, 1: _begin k, _end k - 1
        for bc in order:
            for w in bc.wavs:
                w[:] = NAN
        for k, bc in enumerate(order):
            _poison(m, k % 2)                               # idle: the lane's previous batch has ended
            bc.begin(k % 2)
            if k:
                order[k - 1].end((k - 1) % 2)
        order[-1].end((len(order) - 1) % 2)
        for k, bc in enumerate(bf):
            _same_as(hop, [r + (d,) for r, d in zip(bc.results(), bc.durations)], utts, fit, unf, f"fitted lane batch {k}, graph={graph}")
        for k, bc in enumerate(bu):
            for i, ((w, nf), d, (wr, nfr, dr)) in enumerate(zip(bc.results(), bc.durations, cap)):
                assert nf == nfr and np.array_equal(w, wr) and np.array_equal(d, dr), ("unfitted lane batch", k, i, graph)
    m.set_graph_mode(False)


# ---- 7. kernel regimes ------------------------------------------------------------------------------------------------------

def _regimes():
    from test_gpu_batch_edges import _regimes as batch_regimes
    return batch_regimes()


def _regime_utterances(g):
    """the compositions of tests/test_gpu_batch_edges.py, (a): 18 utterances, capacities 1 .. 1 500; predicted durations (their
    stand-alone calls fill from under a quarter of T to all of it)"""
    from test_gpu_batch_edges import BASE
    from zerovox_cpp_amd import synth
    return [(*synth.encoder_inputs(g, 5000 + 37 * i + N, N), T) for i, (N, T) in enumerate(BASE)]


@pytest.fixture(scope="module")
def regime_refs(ckpt):
    """default regime, once: the fitted batch's frame counts, and the unfitted stand-alone call of every utterance at its own"""
    from zerovox_cpp_amd import capi
    path, g, _ = ckpt("medium")
    utts = _regime_utterances(g)
    m = capi.Model(path, 0)
    try:
        nfs = [nf for _, nf in m.synthesize_batch(utts, fitted=True)]
        refs = [None if nf == 0 else m.synthesize(*u[:3], nf) for u, nf in zip(utts, nfs)]
    finally:
        m.close()
    assert any(nf == u[3] for u, nf in zip(utts, nfs)) and any(0 < nf < u[3] // 4 for u, nf in zip(utts, nfs)), nfs
    return path, g, utts, nfs, refs


@pytest.mark.parametrize("regime", _regimes(), ids=lambda r: r[0])
def test_fitted_batch_in_every_kernel_regime(regime_refs, regime):
    from zerovox_cpp_amd import capi
    path, g, utts, nfs, refs = regime_refs
    hop = g.hop_size
    name, sw = regime

    def check(res, what):
        for i, ((w, nf), u, nfr, ref) in enumerate(zip(res, utts, nfs, refs)):
            assert nf == nfr, (name, what, i, nf, nfr)
            if ref is not None:
                assert np.array_equal(w[: nf * hop], ref[0]), (name, what, i)
            assert not np.isnan(w[nf * hop:]).any() and not w[nf * hop:].any(), (name, what, i, "tail")

    with capi.switches(**sw):
        m = capi.Model(path, 0)
        try:
            bc = m.prepare_batch(utts, fitted=True)
            for mode in ("eager", "capture", "replay"):
                m.set_graph_mode(mode != "eager")
                for w in bc.wavs:
                    w[:] = NAN
                _poison(m)
                bc.run()
                check(bc.results(), mode)
            m.set_graph_mode(False)
            # a single fitted call goes through a one-entry table: the same regimes
            i = max(range(len(utts)), key=lambda k: nfs[k] if nfs[k] < utts[k][3] else 0)
            _poison(m)
            w, nf = m.synthesize(*utts[i], fitted=True)
            assert nf == nfs[i] and np.array_equal(w[: nf * hop], refs[i][0]) and not w[nf * hop:].any(), (name, "single", i)
        finally:
            m.close()


# ---- 8. other geometries ----------------------------------------------------------------------------------------------------

def test_geometry_choice_is_from_the_lists():
    from zerovox_cpp_amd import synth
    assert OTHER_GEOMETRIES[0] in synth.RESBLOCK_GEOMETRIES and OTHER_GEOMETRIES[1] in synth.ENCDEC_GEOMETRIES


OTHER_GEOMETRIES = ("medium_rb_wide", "medium_e720")


@pytest.mark.parametrize("geom", OTHER_GEOMETRIES)
def test_other_geometries(ckpt, geom):
    from zerovox_cpp_amd import capi
    path, g, _ = ckpt(geom)
    hop = g.hop_size
    m = capi.Model(path, 0)
    try:
        rng = np.random.default_rng(3)
        utts = [(*_utt(g, 800 + i, N), T) for i, (N, T) in enumerate(((50, 400), (9, 65), (120, 900), (3, 256)))]
        pcs = [_controls(rng, len(u[0]), t) for u, t in zip(utts, (None, 33, 257, 256))]
        prs = [None, PROSODIES[1], None, None]
        fit = _alone_fitted(m, utts, prs, pcs)
        unf = _alone_unfitted(m, utts, prs, pcs, fit)
        assert [f[1] for f in fit[1:]] == [33, 257, 256]
        for i, (f, u, rf) in enumerate(zip(fit, utts, unf)):
            _check_fitted(hop, f, rf, u[3], (geom, "single", i))
        for graph in (False, True):
            m.set_graph_mode(graph)
            bc = m.prepare_batch([u + (p, c) for u, p, c in zip(utts, prs, pcs)], durations=True, fitted=True)
            for rep in range(2 if graph else 1):
                _same_as(hop, _batch_results(bc), utts, fit, unf, (geom, graph, rep))
        m.set_graph_mode(False)
    finally:
        m.close()


# ---- 9. CLI -----------------------------------------------------------------------------------------------------------------

def _cli(model, args):
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    r = subprocess.run([cli, "-m", model] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_fit_equals_the_run_at_its_own_length_and_trim_is_unchanged(env, tmp_path):
    from zerovox_cpp_amd import synth
    m, g, _ = env
    hop, N, nf = g.hop_size, 40, 137
    ids, puncts, style = _utt(g, 71, N)
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(map(str, ids.tolist())) + "\n" + " ".join(map(str, puncts.tolist())) + "\n" +
                   " ".join(repr(float(x)) for x in style.tolist()) + "\n")
    frames = _forced(N, nf)
    pcf = tmp_path / "forced.txt"
    pcf.write_text("".join(f"{f} 1 0.05 -0.05\n" for f in frames))
    ctl = ["-u", str(utt), "--phoneme-controls", str(pcf)]
    fit, trim, full, tsv = tmp_path / "fit.wav", tmp_path / "trim.wav", tmp_path / "full.wav", tmp_path / "align.tsv"
    r = _cli(_M["path"], ctl + ["-o", str(fit), "--fit", "--alignment", str(tsv)])
    assert f"{nf * hop} samples ({nf} frames)" in r.stdout, r.stdout
    _cli(_M["path"], ctl + ["-o", str(trim), "--trim"])
    _cli(_M["path"], ctl + ["-o", str(full)])
    assert os.path.getsize(fit) == 44 + 2 * nf * hop and os.path.getsize(trim) == 44 + 2 * nf * hop
    # --trim: the first n_frames * hop samples of the max_seq_len-frame run, as before
    assert trim.read_bytes()[44:] == full.read_bytes()[44: 44 + 2 * nf * hop]
    # --fit: the file of the unfitted run whose capacity is n_frames (the same weights in a checkpoint with max_seq_len = nf)
    g_nf = dataclasses.replace(g, name="medium_fit_cli", max_seq_len=nf)
    short = tmp_path / "short.gguf"
    synth.write_checkpoint(str(short), g_nf, 1234)
    own = tmp_path / "own.wav"
    _cli(str(short), ctl + ["-o", str(own)])
    assert fit.read_bytes() == own.read_bytes()
    assert fit.read_bytes() != trim.read_bytes()            # the padded run's statistics include the zero tail
    # the alignment of the fitted run: the forced frames
    rows = [line.split("\t") for line in tsv.read_text().splitlines()][1:]
    assert [int(r[3]) for r in rows] == frames.tolist()
    # and the library agrees with the file (PCM16 of the fitted call's live samples)
    w, n, d = m.synthesize(ids, puncts, style, g.max_seq_len, return_durations=True, fitted=True,
                           phonemes=dict(duration_frames=frames, pitch_shift=np.full(N, 0.05, np.float32),
                                         energy_shift=np.full(N, -0.05, np.float32)))
    assert n == nf and np.array_equal(d, frames)
    # --fit alone (no controls) and with a prosody flag: n_frames * hop samples, reported frames = the library's
    for extra, pr in (([], None), (["--duration-scale", "0.5"], dict(duration_scale=0.5))):
        out = tmp_path / "plain_fit.wav"
        r = _cli(_M["path"], ["-u", str(utt), "-o", str(out), "--fit"] + extra)
        _, n2 = m.synthesize(ids, puncts, style, g.max_seq_len, prosody=pr, fitted=True)
        assert os.path.getsize(out) == 44 + 2 * n2 * hop and f"({n2} frames)" in r.stdout
