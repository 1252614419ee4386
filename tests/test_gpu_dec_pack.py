"""-m gpu: densely packed decoding (csrc/dec_runs.h "densely packed decoding"; switch ZV_DEC_PACK: 1 packs wherever the decoder
runs run-shortened, 0 keeps every utterance a segment of its own).

The contract is that nothing changes: every comparison is between ZV_DEC_PACK = 1 and ZV_DEC_PACK = 0 and is bitwise (uint32
views) — waveforms, frame counts and the vocoder's run table (ZV_VOC_RUNS = 2 in both arms), which is found from the rows of the
expanded mel that are bitwise equal.  (The batch entry points return no mel; the waveform is the vocoder's function of it.)
ZV_DEC_RUNS = 2, ZV_CONV_GEMM = 2 and ZV_DEC_PREPASS = 1 put a batch of six short utterances on the batch kernels: on the small
geometry every wide conv is whole groups of conv_gemm_kernel, on small_e304 two or three output tiles are left to
conv1d_mfma_kernel from nt_begin on, over the same packed segment.

One batch, capacities (96, 128, 64, 100, 160, 352), three sets of frame counts set exactly with target durations; the packed layout
of each is restated here and test_the_cases_sit_where_they_are_meant_to pins what each set is for.  The lane is poisoned
(zv_debug_poison, NaN patterns) before every call, so a guard row that is not written, or a read of a guard row's output, cannot
pass as a stale right value; one pass also runs with ZV_ARENA_FILL = 255.  No test passes because nothing was packed: the event
profile has the pack pass in one arm and not in the other."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 14                      # the shipped decoder's reach (tests/test_gpu_dec_runs.py)
CAPS = (96, 128, 64, 100, 160, 352)
PHONEMES = (5, 7, 4, 9, 6, 8)
# set 0: a live end exactly on the 256-row tile edge (its guard opens the next tile), a slot end on 512, runs taken and not (n = T;
#        T = 64 and 96 are too short for one), rows_c = 100 is no multiple of 32 (the last statistics block holds guard rows).
# set 1: tile [256, 512) holds rows of three utterances and the 512 edge falls inside an utterance.
# set 2: every utterance fills its capacity: no run is taken, the packed rows are more than the capacity rows.
LENGTHS = ((96, 128, 10, 100, 12, 40), (10, 9, 10, 30, 12, 40), CAPS)
REGIME = dict(ZV_DEC_RUNS=2, ZV_CONV_GEMM=2, ZV_DEC_PREPASS=1, ZV_VOC_RUNS=2)
_M = {}


def dec_run(n, T, r=R):
    """(rows the decoder computes, blocks dropped) — csrc/dec_runs.h dec_run restated"""
    a = (n + r + 32 + 31) // 32 * 32
    b = (T - r - 1) // 32 * 32 if T - r - 1 >= 0 else 0
    G = (b - a) // 32
    return (T, 0) if G < 1 else (a + T - b, G)


def layout(lengths):
    """[(row0_p, rows_c, slot, blocks dropped)] and L_p — csrc/dec_runs.h dec_pack_slot restated"""
    out, at = [], 0
    for n, T in zip(lengths, CAPS):
        rows_c, G = dec_run(n, T)
        slot = (rows_c + 1 + 31) // 32 * 32
        out.append((at, rows_c, slot, G))
        at += slot
    return out, at


def test_the_cases_sit_where_they_are_meant_to():
    l0, L0 = layout(LENGTHS[0])
    assert [G > 0 for _, _, _, G in l0] == [False, False, False, False, True, True]
    assert l0[1][0] + l0[1][1] == 256 and l0[1][2] - l0[1][1] == 32          # the live rows end on the tile edge, a whole guard block behind it
    assert l0[3][0] + l0[3][2] == 512 and l0[3][1] == 100                       # a slot ends on a tile edge; rows_c no multiple of 32
    assert any(rc % 32 == 0 for _, rc, _, _ in l0) and L0 == 800
    l1, L1 = layout(LENGTHS[1])
    live = [(r0, r0 + rc) for r0, rc, _, _ in l1]
    assert sum(1 for a, b in live if a < 512 and b > 256) == 3                  # three utterances have live rows in tile [256, 512)
    assert any(a < 512 < b for a, b in live)                                    # and the 512 edge falls inside one of them
    l2, L2 = layout(LENGTHS[2])
    assert all(G == 0 for _, _, _, G in l2) and L2 > sum(CAPS) and L2 <= sum(CAPS) + 32 * len(CAPS)
    assert all(r0 % 32 == 0 and 1 <= slot - rc <= 32 for lay in (l0, l1, l2) for r0, rc, slot, _ in lay)


def _model(ckpt, name):
    from zerovox_cpp_amd import capi
    if name not in _M:
        path, g, tensors = ckpt(name)
        _M[name] = (capi.Model(path, 0), g)
    _M[name][0].set_graph_mode(False)
    return _M[name]


def teardown_module(module):
    for m, _ in _M.values():
        m.close()
    _M.clear()


def _bits(w):
    return np.ascontiguousarray(w, dtype=np.float32).view(np.uint32)


def _batch(g, lengths):
    from zerovox_cpp_amd import synth
    return [(*synth.encoder_inputs(g, 1200 + i, N), T, None, None, n) for i, (N, T, n) in enumerate(zip(PHONEMES, CAPS, lengths))]


def _set(bc, lengths):
    for i, n in enumerate(lengths):
        bc.set_target_frames(i, n)


def _run(m, bc, poison=0xFF):
    for w in bc.wavs:
        w[:] = np.nan
    m.poison(poison)
    bc.run()
    return [(w.copy(), nf) for w, nf in bc.results()], m.voc_runs().copy()


def _same(got, ref, what):
    (res, tab), (res0, tab0) = got, ref
    assert tab.shape == tab0.shape and np.array_equal(tab, tab0), (what, tab.tolist(), tab0.tolist())
    for i, ((w, nf), (w0, nf0)) in enumerate(zip(res, res0)):
        assert np.isfinite(w0).all(), (what, i)
        assert nf == nf0 and np.array_equal(_bits(w), _bits(w0)), (what, i, nf, nf0, int((_bits(w) != _bits(w0)).sum()))


_REFS = {}


def _refs(m, g, name):
    """ZV_DEC_PACK = 0, eager, once per geometry: [(results, vocoder run table)] per length set"""
    from zerovox_cpp_amd import capi
    if name not in _REFS:
        with capi.switches(ZV_DEC_PACK=0, **REGIME):
            out = []
            for lengths in LENGTHS:
                out.append(_run(m, m.prepare_batch(_batch(g, lengths))))
                assert [nf for _, nf in out[-1][0]] == list(lengths)          # the targets set the frame counts exactly
                assert out[-1][1].shape == (len(CAPS), 4)
        _REFS[name] = out
    return _REFS[name]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["small", "small_e304"])
def test_packed_batch_has_the_bits_of_the_unpacked_one(ckpt, name, graph):
    """eager, and under graph replay with the lengths changed between replays: one graph, a new table each time"""
    from zerovox_cpp_amd import capi
    m, g = _model(ckpt, name)
    refs = _refs(m, g, name)
    with capi.switches(ZV_DEC_PACK=1, **REGIME):
        m.set_graph_mode(graph)
        bc = m.prepare_batch(_batch(g, LENGTHS[0]))
        for rep in range(2 if graph else 1):                                  # graph: capture, then replays
            for k, lengths in enumerate(LENGTHS):
                _set(bc, lengths)
                _same(_run(m, bc, 0x3C if (rep + k) & 1 else 0xFF), refs[k], (name, graph, rep, k))
        m.set_graph_mode(False)


def test_two_lanes_in_flight(ckpt):
    """two batches with different lengths enqueued on two lanes before either is waited for"""
    from zerovox_cpp_amd import capi
    m, g = _model(ckpt, "small")
    refs = _refs(m, g, "small")
    with capi.switches(ZV_DEC_PACK=1, **REGIME):
        for graph in (False, True):
            m.set_graph_mode(graph)
            bcs = [m.prepare_batch(_batch(g, LENGTHS[k])) for k in (0, 1)]
            for rep in range(2):
                for lane, bc in enumerate(bcs):
                    for w in bc.wavs:
                        w[:] = np.nan
                    m.poison(0xFF, lane)
                for lane, bc in enumerate(bcs):
                    bc.begin(lane)
                for lane, bc in enumerate(bcs):
                    bc.end(lane)
                for lane, bc in enumerate(bcs):
                    got = [(w.copy(), nf) for w, nf in bc.results()], m.voc_runs(lane).copy()
                    _same(got, refs[lane], ("lanes", graph, rep, lane))
        m.set_graph_mode(False)


def test_fresh_arenas_filled_with_nan_patterns(ckpt):
    """ZV_ARENA_FILL = 255 on a model of its own, so that its arenas are allocated under the fill: a guard left unwritten is a NaN"""
    from zerovox_cpp_amd import capi
    path, g, _ = ckpt("small")
    refs = _refs(*_model(ckpt, "small"), "small")
    with capi.switches(ZV_DEC_PACK=1, ZV_ARENA_FILL=255, **REGIME):
        m = capi.Model(path, 0)
        try:
            m.set_graph_mode(False)
            for k, lengths in enumerate(LENGTHS):
                bc = m.prepare_batch(_batch(g, lengths))
                for w in bc.wavs:
                    w[:] = np.nan
                bc.run()
                _same(([(w.copy(), nf) for w, nf in bc.results()], m.voc_runs().copy()), refs[k], ("arena fill", k))
        finally:
            m.close()


def test_the_pack_pass_runs_in_one_arm_only_and_the_profile_prices_the_table_rows(ckpt):
    from zerovox_cpp_amd import capi
    m, g = _model(ckpt, "small")
    utts = _batch(g, LENGTHS[0])

    def prof(**sw):
        with capi.switches(**sw):
            m.profile_begin()
            m.synthesize_batch(utts)
            st = m.profile_end()
        return [s["name"] for s in st], sum(s["algo_flops"] for s in st if s["name"] == "dec_conv")

    n1, f1 = prof(ZV_DEC_PACK=1, **REGIME)
    n0, f0 = prof(ZV_DEC_PACK=0, **REGIME)
    assert "dec_pack_rows" in n1 and "dec_run_expand" in n1 and "dec_pack_rows" not in n0 and "dec_run_expand" in n0
    assert f1 == f0 > 0                                                        # priced by the rows the table holds, in both layouts
    # packing follows the run table: none in fitted mode, with the pre-pass off, or with ZV_DEC_RUNS at its default on a small batch
    assert capi.debug_get("ZV_DEC_PACK") in (0, 1)
    with capi.switches(ZV_DEC_PACK=1):
        m.profile_begin()
        m.synthesize_batch(utts)
        assert "dec_pack_rows" not in [s["name"] for s in m.profile_end()]
    with capi.switches(ZV_DEC_PACK=1, **dict(REGIME, ZV_DEC_PREPASS=0)):
        m.profile_begin()
        m.synthesize_batch(utts)
        assert "dec_pack_rows" not in [s["name"] for s in m.profile_end()]
    with capi.switches(ZV_DEC_PACK=1, **REGIME):
        m.profile_begin()
        m.synthesize_batch([u[:4] for u in utts], fitted=True)
        assert "dec_pack_rows" not in [s["name"] for s in m.profile_end()]
