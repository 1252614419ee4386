"""-m gpu: the six waveform stages (filter, envelope, volume, contour, pitch track, band levels) in ONE call with mixed asks, at the
production geometry (the "medium" synthetic checkpoint).  The per-stage tests hold each stage to its rule; this one holds the plumbing
they share (csrc/wave_stages.h, capi.cpp) to the one property it owes: a batch gives every utterance what the utterance gets alone
with the same asks, bit for bit — waveform, level and every table — whichever utterances ask for what.
  * a ragged batch of three (capacities 40, 64, 96; 9, 33, 70 phonemes): utterance 0 asks for everything, utterance 1 for nothing (no
    tables, no taps, no volume: the identity row), utterance 2 for contour frames only, pitch phonemes only, bands with its own edges
    and a one-tap filter; eagerly and under a graph replayed twice, the lane poisoned between runs and every output prefilled with a
    sentinel; then two such batches in flight on lanes 0 and 1;
  * the smallest batch that splits into tail groups (16 utterances at T = 900: 16 MiB of waveform), the asks cycled over the
    utterances: under ZV_TAIL_GROUPS = 2 and 8 everything is bit-equal to the one-group run."""
import numpy as np
import pytest

import filter_rule as FR
import level_rule as LR

pytestmark = pytest.mark.gpu

_M = {}
F = np.float32


@pytest.fixture(scope="module")
def env(ckpt):
    from zerovox_cpp_amd import capi
    if "m" not in _M:
        path, g, tensors = ckpt("medium")
        _M.update(m=capi.Model(path, 0), g=g)
    _M["m"].set_graph_mode(False)
    yield _M["m"], _M["g"]
    _M["m"].set_graph_mode(False)


def teardown_module(module):
    if "m" in _M:
        _M["m"].close()
    _M.clear()


def _utt(g, seed, N):
    from zerovox_cpp_amd import synth
    return synth.encoder_inputs(g, seed, N)


def _taps(seed, L):
    return (np.random.default_rng(1000 + seed).standard_normal(L) / np.sqrt(L)).astype(F)


def _gains(N, seed):
    g = np.random.default_rng(seed).random(N) * 4.0
    g[::5] = 0.0
    return g.astype(F)


def _asks(kind, N, seed):
    """the keyword arguments of one utterance's asks: 0 everything, 1 nothing, 2 the mixed ones"""
    from zerovox_cpp_amd import capi
    if kind == 0:
        return dict(volume=capi.Volume(0.8, 0.07, 0.5), envelope=capi.Envelope(_gains(N, seed), 2, 450, 1000), return_contour=True,
                    return_pitch=True, return_bands=True, filter=_taps(seed, 33))
    if kind == 1:
        return dict(volume=None, envelope=None, return_contour=False, return_pitch=False, return_bands=False, filter=None)
    return dict(volume=None, envelope=None, return_contour="frames", return_pitch=capi.PitchTrack(frames=False),
                return_bands=capi.BandLevels(edges=[2, 9, 40, 200, 500]), filter=np.array([0.5], F))


def _tables(c, p, b):
    return dict(cf=None if c is None else c.frames, cp=None if c is None else c.phonemes, pf=None if p is None else p.frames,
                pp=None if p is None else p.phonemes, bf=None if b is None else b.frames, bp=None if b is None else b.phonemes)


def _alone(m, u, a, fitted):
    """utterance u = (ids, puncts, style, T, None, None, target) synthesized alone with the asks a: (wav, n_frames, level bits, tables)"""
    out = m.synthesize(*u[:4], fitted=fitted, target_frames=u[6], return_levels=True, **a)
    w, n, lv = out[:3]
    rest = list(out[3:])
    c = rest.pop(0) if a["return_contour"] else None
    p = rest.pop(0) if a["return_pitch"] else None
    b = rest.pop(0) if a["return_bands"] else None
    assert not rest
    return w.copy(), n, LR.level_bits(lv), {k: None if t is None else t.copy() for k, t in _tables(c, p, b).items()}


def _prepare(m, utts, asks, fitted):
    col = lambda k: [a[k] for a in asks]
    return m.prepare_batch(utts, fitted=fitted, volume=col("volume"), return_levels=True, envelope=col("envelope"),
                           return_contour=col("return_contour"), return_pitch=col("return_pitch"), return_bands=col("return_bands"),
                           filter=col("filter"))


def _snapshot(bc):
    """what a finished batch handed out, per utterance, copied: (wav, n_frames, level bits, tables)"""
    out = []
    for i, (w, n) in enumerate(bc.results()):
        t = _tables(bc.contours[i], bc.pitches[i], bc.bands[i])
        out.append((w.copy(), n, LR.level_bits(bc.levels[i]), {k: None if a is None else a.copy() for k, a in t.items()}))
    return out


def _prefill(bc):
    for i, w in enumerate(bc.wavs):
        w.fill(7.0)
        bc.levels[i].rms = bc.levels[i].peak = bc.levels[i].gain = 7.0
        for a in _tables(bc.contours[i], bc.pitches[i], bc.bands[i]).values():
            if a is not None:
                a.fill(7.0)


def _same(what, got, want):
    """bit for bit, the comparison of the per-stage tests"""
    assert len(got) == len(want)
    for i, ((w, n, lv, t), (w0, n0, lv0, t0)) in enumerate(zip(got, want)):
        assert n == n0, (what, i, n, n0)
        bad = np.flatnonzero(FR.bits(w) != FR.bits(w0))
        assert bad.size == 0, (what, i, "wave", bad.size, bad[:8])
        assert lv == lv0, (what, i, "level", lv, lv0)
        for k in t0:
            assert (t[k] is None) == (t0[k] is None), (what, i, k)
            if t0[k] is not None:
                assert t[k].shape == t0[k].shape and np.array_equal(FR.bits(t[k]), FR.bits(t0[k])), (what, i, k)


def _ragged(g, seed, rot):
    """three utterances of capacities 40, 64, 96 with 9, 33, 70 phonemes and the three asks, rotated by rot"""
    nt = [(9, 40, 31), (33, 64, 64), (70, 96, 77)]
    utts = [(*_utt(g, seed + i, N), T, None, None, tf) for i, (N, T, tf) in enumerate(nt)]
    return utts, [_asks((i + rot) % 3, nt[i][0], seed + i) for i in range(3)]


def test_ragged_batch_with_mixed_asks_equals_the_utterances_alone(env):
    m, g = env
    utts, asks = _ragged(g, 900, 0)
    m.set_graph_mode(False)
    alone = [_alone(m, u, a, False) for u, a in zip(utts, asks)]
    plain = m.synthesize(*utts[1][:4], target_frames=utts[1][6])[0]
    assert np.array_equal(FR.bits(alone[1][0]), FR.bits(plain))                  # an utterance that asks for nothing: the plain call's bits
    assert [t is None for t in alone[1][3].values()] == [True] * 6
    assert alone[2][3]["cp"] is None and alone[2][3]["pf"] is None and alone[2][3]["bf"].shape == (96, 4) and alone[2][3]["bp"].shape == (70, 4)
    bc = _prepare(m, utts, asks, False)
    assert bc.contours[1] is None and bc.pitches[1] is None and bc.bands[1] is None
    for what, graph, poison in [("eager", False, 0xFF), ("graph capture", True, 0x00), ("graph replay", True, 0xFF), ("second replay", True, 0x00)]:
        m.set_graph_mode(graph)
        m.poison(poison)
        _prefill(bc)
        bc.run()
        _same(what, _snapshot(bc), alone)
    m.set_graph_mode(False)


def test_two_batches_in_flight_on_lanes_0_and_1(env):
    m, g = env
    sets = [_ragged(g, 900, 0), _ragged(g, 950, 1)]
    m.set_graph_mode(False)
    alone = [[_alone(m, u, a, False) for u, a in zip(utts, asks)] for utts, asks in sets]
    batches = [_prepare(m, utts, asks, False) for utts, asks in sets]
    for graph in (False, True, True):
        m.set_graph_mode(graph)
        for lane, bc in enumerate(batches):
            m.poison(0xFF, lane)
            _prefill(bc)
        batches[0].begin(0)
        batches[1].begin(1)
        batches[0].end(0)
        batches[1].end(1)
        for k, bc in enumerate(batches):
            _same((graph, k), _snapshot(bc), alone[k])
    m.set_graph_mode(False)


def test_batch_split_into_tail_groups(env):
    from zerovox_cpp_amd import capi
    m, g = env
    hop, T = g.hop_size, 900                                  # 16 utterances: 2 and 8 groups are different schedules (two utterances per group at least)
    tfs = [900, 500, 250, 37, 899, 1, 640, 333, 65, 700, 31, 32, 33, 450, 820, 128]
    utts = [(*_utt(g, 700 + i, 40 + 9 * i), T, None, None, tf) for i, tf in enumerate(tfs)]
    assert len(utts) * T * hop * 4 >= 16 << 20 and len(utts) // 2 >= 8
    asks = [_asks(i % 3, 40 + 9 * i, 700 + i) for i in range(len(utts))]
    m.set_graph_mode(False)
    with capi.switches(ZV_TAIL_GROUPS=1):
        bc = _prepare(m, utts, asks, True)
        _prefill(bc)
        bc.run()
        one = _snapshot(bc)
        assert [n for _, n, _, _ in one] == tfs
        for i in (3, 4, 5):                                   # one utterance of each ask of the one-group run against itself alone
            _same(("one group", i), [one[i]], [_alone(m, utts[i], asks[i], True)])
    for groups in (2, 8):
        with capi.switches(ZV_TAIL_GROUPS=groups):
            for graph in (False, True):
                m.set_graph_mode(graph)
                bc = _prepare(m, utts, asks, True)
                for rep in range(2 if graph else 1):
                    m.poison(0x00 if rep else 0xFF)
                    _prefill(bc)
                    bc.run()
                    _same((groups, graph, rep), _snapshot(bc), one)
            m.set_graph_mode(False)
