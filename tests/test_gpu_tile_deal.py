"""-m gpu: the ResBlock kernels' deal of a batch's tiles over the XCDs (csrc/tile_deal.h) changes no bit.

Launches with one segment keep the map they always had, so every utterance of a ragged batch is compared, bitwise (uint32 views), with
the same utterance synthesized alone with ZV_VOC_RUNS = 0.  The batches have 2, 3, 5 and 9 utterances of 8 to 40 phonemes under
one capacity T <= 200 frames; frame counts are forced (duration_frames) so that every batch holds utterances far shorter than T, one
that overfills it, and several in between.  T is computed from the last stage's tile height and the chunk length c the library
ships for that stage, so that the tiles per segment are 8c - 1, 0 and 1 modulo 8c (a full last round of chunks, none, one tile);
a fourth capacity, with 128-row tiles forced (ZV_PAIR_MT = 4), leaves the 256-channel stage fewer than 8 tiles per segment.  Each
batch runs run-shortened (ZV_VOC_RUNS = 2) and through zv_synthesize_batch_fitted, eager and under graph capture plus one replay, and
once more in the kernel regime of large batches (512-row tiles of the 32-channel whole-block kernel, the 64-channel ring kernels).
The lane is poisoned before every call under test: a tile no workgroup covers cannot pass on the previous call's samples.  After
the run-shortened call the run table must show fewer than T rows for at least one utterance, and the fitted batch must be ragged."""
import numpy as np
import pytest

from test_tile_deal_cpu import shipped_chunks

pytestmark = pytest.mark.gpu

_M = {}
T_MAX = 200
NS = (8, 40, 13, 29, 21, 35, 10, 17, 26)              # phonemes per utterance
BATCH_REGIME = dict(ZV_TRIPLE_V2=3, ZV_PAIR64_RING=2, ZV_BLOCK64=-3)


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


def _bits(w):
    return np.ascontiguousarray(w, dtype=np.float32).view(np.uint32)


def _poison(m):
    _M["fill"] = 0xFF ^ 0x3C ^ _M.get("fill", 0x3C)
    m.poison(_M["fill"])


def _last_stage_tm(g):
    """tile height of the 3-tap branch in the last stage's whole-block kernels on 256-row tiles: 256 - (K - 1) (sum(dil) + n_dil)"""
    assert tuple(g.resblock_dilations) == (1, 3, 5)
    return 256 - 2 * (sum(g.resblock_dilations) + len(g.resblock_dilations))


def _capacity(g, c, residue):
    """the largest T <= T_MAX whose tiles per segment at the last stage are `residue` modulo 8c"""
    TM, hop = _last_stage_tm(g), g.hop_size
    for T in range(T_MAX, 100, -1):
        if -(-T * hop // TM) % (8 * c) == residue:
            return T
    raise AssertionError("no capacity for residue %d" % residue)


def _forced(N, total):
    return (total // N + (np.arange(N) < total % N)).astype(np.int32)


def _batch(g, nseg, T):
    """(ids, puncts, style, T, None, controls) per utterance and the frame counts they must come out with"""
    from zerovox_cpp_amd import synth
    totals = [12, T + 20, T // 3, T - 87, 40, T // 2, 25, T - 60, 70][:nseg]
    utts = []
    for i, (N, tot) in enumerate(zip(NS, totals)):
        ids, puncts, style = synth.encoder_inputs(g, 4200 + 10 * nseg + i, N)
        utts.append((ids, puncts, style, T, None, dict(duration_frames=_forced(N, tot))))
    return utts, [min(t, T) for t in totals]


def _same(res, ref, what):
    for i, ((w, nf), (wr, nfr)) in enumerate(zip(res, ref)):
        assert nf == nfr and np.array_equal(_bits(w), _bits(wr)), (what, i, nf, nfr, int((_bits(w) != _bits(wr)).sum()))


def _run_batch(m, utts, T, fitted, what):
    """eager, then capture and one replay; the results of each run"""
    out = []
    for graph in (False, True):
        m.set_graph_mode(graph)
        bc = m.prepare_batch(utts, fitted=fitted)
        for rep in range(2 if graph else 1):
            for w in bc.wavs:
                w[:] = np.nan
            _poison(m)
            bc.run()
            if not fitted:
                tab = m.voc_runs()
                assert tab.shape == (len(utts), 4) and (tab[:, 1] < T).any(), (what, graph, rep, tab.tolist())
            out.append(((graph, rep), [(w.copy(), nf) for w, nf in bc.results()]))
    m.set_graph_mode(False)
    return out


def _check(m, g, nseg, T, extra, what):
    from zerovox_cpp_amd import capi
    utts, want_nf = _batch(g, nseg, T)
    assert min(want_nf) + 87 <= T and max(want_nf) == T
    with capi.switches(ZV_VOC_RUNS=0):
        ref = [m.synthesize(u[0], u[1], u[2], T, phonemes=u[5]) for u in utts]
        ref_fit = [m.synthesize(u[0], u[1], u[2], T, phonemes=u[5], fitted=True) for u in utts]
        assert m.voc_runs().shape[0] == 0
    assert [nf for _, nf in ref] == want_nf and [nf for _, nf in ref_fit] == want_nf
    regimes = [("default", extra), ("batch regime", dict(BATCH_REGIME, **extra))]
    for name, sw in regimes:
        with capi.switches(ZV_VOC_RUNS=2, **sw):
            for tag, res in _run_batch(m, utts, T, False, (what, name)):
                _same(res, ref, (what, name, "runs", tag))
            for tag, res in _run_batch(m, utts, T, True, (what, name)):
                _same(res, ref_fit, (what, name, "fitted", tag))


@pytest.mark.parametrize("kind", ["full_last_round", "no_remainder", "one_tile_over"])
def test_ragged_batches_at_chunk_edges(env, kind):
    m, g = env
    c = shipped_chunks()[32]
    residue = {"full_last_round": 8 * c - 1, "no_remainder": 0, "one_tile_over": 1}[kind]
    T = _capacity(g, c, residue)
    tps = -(-T * g.hop_size // _last_stage_tm(g))
    print("T", T, "tiles per segment", tps, "mod 8c", tps % (8 * c), "c", c)
    assert tps % (8 * c) == residue and 100 < T <= T_MAX
    for nseg in (2, 3, 5, 9):
        _check(m, g, nseg, T, {}, (kind, nseg, T))


def test_fewer_than_eight_tiles_per_segment_at_256_channels(env):
    """128-row tiles (ZV_PAIR_MT = 4): 118 to 126 output rows each, 5 rows per frame at the 256-channel stage -> 6 or 7 tiles per
    segment at T = 150, fewer than one per XCD; nine utterances give the stage enough rows to run on the fused kernel"""
    m, g = env
    T, rate = 150, g.upsample_scales[0]
    assert m.voc_channels(0) == 256 and m.voc_rate(0) == rate
    for K in (3, 7, 11):
        assert -(-T * rate // (128 - (K - 1))) < 8
    n_cu = 256
    assert (T * rate * 9 // 54) * 3 >= n_cu                   # voc_plan.h: enough_rows
    _check(m, g, 9, T, dict(ZV_PAIR_MT=4), ("tps < 8", 9, T))
