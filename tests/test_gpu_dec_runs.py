"""-m gpu: run-shortened decoding (csrc/dec_runs.h; switch ZV_DEC_RUNS: 0 never, 1 batches, 2 always).

The contract is that nothing changes: every comparison is between the switch at 0 and at 2 (or at its default) and is bitwise
(uint32 views) — waveforms, frame counts, and the vocoder's run table (ZV_VOC_RUNS = 2 in both arms of the small cases), which
shows that the expanded mel carries the same run of equal rows.  Frame counts are set exactly with target durations, so that a case
sits where it is meant to: an utterance that takes its run, one that misses it by one block, one that fills its capacity.  The lane
is poisoned (zv_debug_poison) before every call, so that an expanded mel row that is not written, or a read of a dropped block,
cannot pass as the stale right value.  No test passes because nothing was skipped: the event profile prices the decoder's convs by
the rows its table holds, and test_profile_counts_the_rows_the_table_holds compares that with the restated rule."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 14                      # the shipped decoder's reach: two 3-tap convs in each of its 7 residual blocks, every other conv 1-tap
_M = {}


def dec_run(n, T, r=R):
    """(rows the decoder computes, blocks dropped) — csrc/dec_runs.h dec_run restated"""
    a = (n + r + 32 + 31) // 32 * 32
    b = (T - r - 1) // 32 * 32 if T - r - 1 >= 0 else 0
    G = (b - a) // 32
    return (T, 0) if G < 1 else (a + T - b, G)


T_MIN = 111                 # the smallest capacity at which a run can be taken: a = 64 (n <= 18), b = 96 <= T - R - 1


def test_the_cases_sit_where_they_are_meant_to():
    assert dec_run(12, 130) == (64 + 34, 1) and dec_run(18, 130)[1] == 1 and dec_run(19, 130) == (130, 0)
    assert dec_run(10, 100) == (100, 0) and dec_run(10, 100 + 11)[1] == 1          # misses it by one block
    assert dec_run(96, 96) == (96, 0)
    assert dec_run(1, T_MIN) == (79, 1) and all(dec_run(n, T_MIN - 1) == (T_MIN - 1, 0) for n in range(1, T_MIN))
    assert all(dec_run(n, T)[1] == 0 for T in range(1, T_MIN) for n in range(1, T + 1))


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


CAPS = (96, 100, 130)       # 100: not a multiple of the 32-row statistics block
# frame counts per capacity.  Set 0: fills its capacity / misses its run by one block (b = 64, it needs 96) / takes it.  Set 1: too
# long for a run / fills its capacity / misses by one block (19 frames put a at 96).  Set 2: too long / misses by one block / takes
# it with the most frames that still do
LENGTHS = ((96, 10, 12), (20, 100, 19), (33, 18, 18))


def _small_batch(g, lengths):
    from zerovox_cpp_amd import synth
    return [(*synth.encoder_inputs(g, 900 + i, N), T, None, None, n) for i, (N, T, n) in enumerate(zip((5, 7, 9), CAPS, lengths))]


def _run_batch(m, bc, poison):
    for w in bc.wavs:
        w[:] = np.nan
    m.poison(poison)
    bc.run()
    return [(w.copy(), nf) for w, nf in bc.results()], m.voc_runs().copy()


def _same(got, ref, what):
    (res, tab), (res0, tab0) = got, ref
    assert tab.shape == tab0.shape and np.array_equal(tab, tab0), (what, tab.tolist(), tab0.tolist())
    for i, ((w, nf), (w0, nf0)) in enumerate(zip(res, res0)):
        assert nf == nf0 and np.array_equal(_bits(w), _bits(w0)), (what, i, nf, nf0, int((_bits(w) != _bits(w0)).sum()))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_small_batch_of_three_capacities(ckpt, graph):
    """three utterances of 96, 100 and 130 frames of capacity; under graph capture the three length sets replay one graph"""
    from zerovox_cpp_amd import capi
    m, g = _model(ckpt, "small")
    with capi.switches(ZV_VOC_RUNS=2):
        refs = []
        with capi.switches(ZV_DEC_RUNS=0):
            for k, lengths in enumerate(LENGTHS):
                refs.append(_run_batch(m, m.prepare_batch(_small_batch(g, lengths)), 0xFF))
                assert [nf for _, nf in refs[-1][0]] == list(lengths)            # the targets set the frame counts exactly
                assert refs[-1][1].shape == (3, 4)
        with capi.switches(ZV_DEC_RUNS=2):
            m.set_graph_mode(graph)
            bc = m.prepare_batch(_small_batch(g, LENGTHS[0]))
            for rep in range(2):                                                 # graph: capture, then replays
                for k, lengths in enumerate(LENGTHS):
                    for i, n in enumerate(lengths):
                        bc.set_target_frames(i, n)
                    _same(_run_batch(m, bc, 0x3C if (rep + k) & 1 else 0xFF), refs[k], (graph, rep, lengths))
            m.set_graph_mode(False)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("T", [T_MIN, T_MIN - 1, 300])
def test_single_utterance_through_synthesize(ckpt, T, graph):
    """ZV_DEC_RUNS = 2 on one utterance through synthesize (a one-entry table): at the smallest T with a run and one below — with
    the operand pre-pass forced on, which a single utterance has from 256 frames on and without which no run is taken — and at 300"""
    from zerovox_cpp_amd import capi, synth
    m, g = _model(ckpt, "small")
    ids, puncts, style = synth.encoder_inputs(g, 950, 6)
    with capi.switches(ZV_VOC_RUNS=2, **({"ZV_DEC_PREPASS": 1} if T < 256 else {})):
        with capi.switches(ZV_DEC_RUNS=0):
            ref = {n: m.synthesize(ids, puncts, style, T, target_frames=n) + (m.voc_runs().copy(),) for n in (9, 18)}
        with capi.switches(ZV_DEC_RUNS=2):
            m.set_graph_mode(graph)
            for rep in range(2 if graph else 1):
                for n in (9, 18):
                    m.poison(0x3C if rep else 0xFF)
                    w, nf = m.synthesize(ids, puncts, style, T, target_frames=n)
                    w0, nf0, tab0 = ref[n]
                    assert nf == nf0 == n and np.array_equal(_bits(w), _bits(w0)), (T, n, rep, int((_bits(w) != _bits(w0)).sum()))
                    assert np.array_equal(m.voc_runs(), tab0), (T, n, rep)
            m.set_graph_mode(False)


def _dec_conv(stats):
    return sum(s["algo_flops"] for s in stats if s["name"] == "dec_conv"), [s["name"] for s in stats]


def test_profile_counts_the_rows_the_table_holds(ckpt):
    """the event profile prices the decoder's convs by the rows decoded: the ratio between the switch at 2 and at 0 is the restated
    rule's, so the runs the other tests count on are really taken (and the library's reach is R)"""
    from zerovox_cpp_amd import capi, synth
    m, g = _model(ckpt, "small")

    def flops(call):
        m.profile_begin()
        call()
        return _dec_conv(m.profile_end())

    for lengths in LENGTHS:
        utts = _small_batch(g, lengths)
        t_rows = len(utts) * ((max(CAPS) + 63) // 64 * 64)           # a batch's launches are priced by its capacity rows
        with capi.switches(ZV_DEC_RUNS=0):
            f0, names0 = flops(lambda: m.synthesize_batch(utts))
        with capi.switches(ZV_DEC_RUNS=2):
            f2, names2 = flops(lambda: m.synthesize_batch(utts))
        rows = sum(dec_run(n, T)[0] for n, T in zip(lengths, CAPS))
        assert "dec_run_expand" in names2 and "enc_dec_runs" in names2 and "dec_run_expand" not in names0
        assert f0 > 0 and abs(f2 / f0 - rows / t_rows) < 1e-9, (lengths, f2 / f0, rows, t_rows)
    ids, puncts, style = synth.encoder_inputs(g, 950, 6)
    for T in (T_MIN, T_MIN - 1, 300):
        with capi.switches(**({"ZV_DEC_PREPASS": 1} if T < 256 else {})):
            with capi.switches(ZV_DEC_RUNS=0):
                f0, _ = flops(lambda: m.synthesize(ids, puncts, style, T, target_frames=18))
            with capi.switches(ZV_DEC_RUNS=2):
                f2, _ = flops(lambda: m.synthesize(ids, puncts, style, T, target_frames=18))
        assert abs(f2 / f0 - dec_run(18, T)[0] / T) < 1e-9, (T, f2 / f0)
    # the default leaves a small batch and a single utterance on the schedule they had; fitted mode and a stand-alone decode take no table
    assert capi.debug_get("ZV_DEC_RUNS") == 1
    _, names = flops(lambda: m.synthesize_batch(_small_batch(g, LENGTHS[0])))
    assert "dec_run_expand" not in names and "enc_dec_runs" not in names
    with capi.switches(ZV_DEC_RUNS=2):
        _, names = flops(lambda: m.synthesize(ids, puncts, style, T_MIN, fitted=True))
        assert "dec_run_expand" not in names and "enc_dec_runs" not in names
        _, names = flops(lambda: m.decode(synth.decoder_hidden(g, 11, T_MIN), style))
        assert "dec_run_expand" not in names
        with capi.switches(ZV_DEC_PREPASS=0):
            _, names = flops(lambda: m.synthesize(ids, puncts, style, 300))
            assert "dec_run_expand" not in names and "enc_dec_runs" not in names


def test_medium_batch_just_over_the_threshold_with_the_default_switch(ckpt):
    """33 utterances of up to 512 frames of capacity: 16 896 capacity rows, so the default (1) takes it and the decoder's wide convs run
    on conv_gemm_kernel with the 33rd output tile on the generic kernel; compared with the switch at 0"""
    from zerovox_cpp_amd import capi, synth
    m, g = _model(ckpt, "medium")
    caps = [512, 500, 449, 512, 384, 511, 480, 417]
    utts = [(*synth.encoder_inputs(g, 700 + i, 4 + (29 * i) % 120), caps[i % len(caps)]) for i in range(33)]
    assert len(utts) * 512 >= 16384 > (len(utts) - 2) * 512 and capi.debug_get("ZV_DEC_RUNS") == 1
    with capi.switches(ZV_DEC_RUNS=0):
        ref = _run_batch(m, m.prepare_batch(utts), 0xFF)
    took = [dec_run(nf, u[3])[1] > 0 for (_, nf), u in zip(ref[0], utts)]
    print("utterances that take their run:", sum(took), "of", len(utts))
    assert 8 <= sum(took) < len(utts) and ref[1].shape == (33, 4)
    for graph in (False, True):
        m.set_graph_mode(graph)
        _same(_run_batch(m, m.prepare_batch(utts), 0x3C if graph else 0xFF), ref, ("default", graph))
    m.set_graph_mode(False)
    m.profile_begin()
    m.synthesize_batch(utts)
    assert "dec_run_expand" in [s["name"] for s in m.profile_end()]
