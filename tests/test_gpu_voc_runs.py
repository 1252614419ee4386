"""-m gpu: run-shortened vocoding (include/zerovox_amd.h zv_vocode; switch ZV_VOC_RUNS: 0 never, 1 batches, 2 always).

The contract is that nothing changes: every comparison is between the switch at 0 and at 2 and is bitwise (uint32 views, so NaN
patterns and the sign of zero count).  No test passes because nothing was skipped: after every call at 2 the device's run table
(zv_debug_voc_runs) is compared, utterance by utterance, with the model of tests/test_voc_runs_cpu.py — rows = T - (b - a) + 2H + 1
for the expected run [a, b), rows = T where no run qualifies — and at 0 the table must be absent.  The two calls of a comparison
run on one lane, whose buffers keep the first call's waveform at the same offsets: the lane is poisoned (zv_debug_poison) before every
call at 1 or 2, so that a sample the shortened schedule does not write cannot pass as the stale right one."""
import numpy as np
import pytest

from test_voc_runs_cpu import MARGIN, halo_frames, longest_run, run_entry

pytestmark = pytest.mark.gpu

_M = {}


@pytest.fixture(scope="module")
def env(ckpt):
    from zerovox_cpp_amd import capi
    if "m" not in _M:
        path, g, tensors = ckpt("medium")
        _M.update(m=capi.Model(path, 0), g=g, t=tensors)
    _M["m"].set_graph_mode(False)
    yield _M["m"], _M["g"], _M["t"]
    _M["m"].set_graph_mode(False)


def teardown_module(module):
    if "m" in _M:
        _M["m"].close()
    _M.clear()


def _bits(w):
    return np.ascontiguousarray(w, dtype=np.float32).view(np.uint32)


def test_halo_formula_is_the_librarys(env):
    m, g, _ = env
    assert halo_frames(g) == m.vocoder_halo_frames()


# ---- 1. zv_vocode on hand-made mels ---------------------------------------------------------------------------------------------

def _cases(g, tensors, H):
    """name -> (mel, expected run [a, b) or None when none qualifies)"""
    from zerovox_cpp_amd import synth
    thr = 2 * H + 1 + MARGIN                     # the shortest run that is taken
    T = 3 * thr + 40

    def base(seed, rows=T):
        mel = synth.vocoder_mel(g, tensors, seed, rows)
        assert longest_run(mel) == (0, 1)        # no two neighbouring rows are equal to begin with
        return mel

    def const(mel, a, b):
        mel[a:b] = mel[a]
        return mel

    out = {"no equal rows": (base(31), None)}
    for d, name in ((-1, "one below the threshold"), (0, "at the threshold"), (1, "one above the threshold")):
        out[name] = (const(base(32 + d), 50, 50 + thr + d), (50, 50 + thr + d) if d >= 0 else None)
    out["touches row 0"] = (const(base(35), 0, thr + 9), (0, thr + 9))
    out["touches row T"] = (const(base(36), T - thr - 5, T), (T - thr - 5, T))
    out["whole mel"] = (const(base(37), 0, T), (0, T))
    out["two runs, the longer is the second"] = (const(const(base(38), 7, 7 + thr), 30 + thr, 30 + 2 * thr + 3), (30 + thr, 30 + 2 * thr + 3))
    out["two equal runs, the first"] = (const(const(base(39), 7, 7 + thr), 30 + thr, 30 + 2 * thr), (7, 7 + thr))
    out["run, then a non-constant end"] = (const(base(40), 20, 20 + 2 * thr), (20, 20 + 2 * thr))
    z = const(base(41), 10, 10 + 2 * thr)
    z[10:10 + 2 * thr] = 0.0
    z[11:10 + 2 * thr:2, 5] = -0.0               # rows equal as floats, no two neighbours equal as bits
    out["+0 / -0 rows"] = (z, None)
    n = base(42)
    n[40:40 + thr + 30] = np.nan
    out["identical NaN rows"] = (n, (40, 40 + thr + 30))
    short = const(base(43, 2 * H + 1), 0, 2 * H + 1)         # the whole mel one run, shorter than the threshold
    out["short whole-mel run"] = (short, None)
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_vocode_hand_made_mels(env, graph):
    from zerovox_cpp_amd import capi
    m, g, tensors = env
    H = m.vocoder_halo_frames()
    taken = 0
    for name, (mel, run) in _cases(g, tensors, H).items():
        T = mel.shape[0]
        want = (T, T, 0) if run is None else (T - (run[1] - run[0]) + 2 * H + 1, run[0] + H, run[1] - run[0] - (2 * H + 1))
        assert run_entry(mel, H) == want, name                      # the model agrees with the case's intent
        m.set_graph_mode(graph)
        with capi.switches(ZV_VOC_RUNS=0):
            ref = m.vocode(mel)
            assert m.voc_runs().shape[0] == 0, name
        with capi.switches(ZV_VOC_RUNS=2):
            for rep in range(2 if graph else 1):                    # graph: capture, then replay
                m.poison(0x3C if rep else 0xFF)
                got = m.vocode(mel)
                tab = m.voc_runs()
                assert tab.shape == (1, 4) and tuple(tab[0]) == (0,) + want, (name, rep, tab, want)
                assert np.array_equal(_bits(got), _bits(ref)), (name, rep, int((_bits(got) != _bits(ref)).sum()))
        taken += run is not None
        m.set_graph_mode(False)
    assert taken >= 8


def test_default_switch_leaves_single_utterances_alone_and_stream_and_fitted_have_no_table(env):
    from zerovox_cpp_amd import capi, synth
    m, g, tensors = env
    assert capi.debug_get("ZV_VOC_RUNS") == 1
    mel = synth.vocoder_mel(g, tensors, 50, 400)
    mel[100:350] = mel[100]
    ref = m.vocode(mel)
    assert m.voc_runs().shape[0] == 0                               # 400 rows: not a batch
    with capi.switches(ZV_VOC_RUNS=2):
        m.poison()
        assert np.array_equal(_bits(m.vocode(mel)), _bits(ref)) and m.voc_runs()[0, 3] > 0
        m.poison(0x3C)
        chunks = m.vocode_stream(mel, 128)
        assert m.voc_runs().shape[0] == 0                           # the chunks are the schedule
        assert np.array_equal(_bits(np.concatenate([c for _, c in chunks])), _bits(ref))
        ids, puncts, style = synth.encoder_inputs(g, 51, 30)
        m.synthesize(ids, puncts, style, 400, fitted=True)
        assert m.voc_runs().shape[0] == 0
        m.poison()
        w2, nf2 = m.synthesize(ids, puncts, style, 400)
        assert m.voc_runs()[0, 3] > 0
    w0, nf0 = m.synthesize(ids, puncts, style, 400)
    assert nf0 == nf2 and np.array_equal(_bits(w0), _bits(w2))


# ---- 2. a batch large enough for the grouped last stage -----------------------------------------------------------------------

T_BATCH = 512


def _batch(g):
    """32 utterances x 512 frames of capacity (19.7 MB of waveform: the last vocoder stage runs in utterance groups), from a few
    phonemes to more than fill the capacity"""
    from zerovox_cpp_amd import synth
    Ns = [4 + (37 * i) % 150 for i in range(30)] + [400, 700]
    return [(*synth.encoder_inputs(g, 800 + i, N), T_BATCH) for i, N in enumerate(Ns)]


def _expected_table(m, utts, H):
    """per utterance (row0, rows, split, shift) from the mel the stand-alone entry points give"""
    want, row0 = [], 0
    for ids, puncts, style, T in utts:
        mel = m.decode(m.encode(ids, puncts, style, T)["hidden"], style)
        want.append((row0,) + run_entry(mel, H))
        row0 += T
    return np.array(want, np.int32)


def _check_table(tab, want, what):
    assert tab.shape == want.shape and np.array_equal(tab, want), (what, tab.tolist(), want.tolist())


def test_batch_switch_0_and_2_eager_graph_and_lanes(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop, H = g.hop_size, m.vocoder_halo_frames()
    utts = _batch(g)
    assert len(utts) * T_BATCH * hop * 4 >= 16 << 20 and capi.debug_get("ZV_TAIL_GROUPS") > 1
    with capi.switches(ZV_VOC_RUNS=0):
        want = _expected_table(m, utts, H)
        ref = m.synthesize_batch(utts)
        assert m.voc_runs().shape[0] == 0
    # every utterance is one of the two kinds, and both kinds are there
    for (row0, rows, split, shift), (w, nf) in zip(want, ref):
        assert (rows == T_BATCH and shift == 0) or (rows == T_BATCH - shift and shift >= MARGIN and split >= H)
    n_taken = int((want[:, 3] > 0).sum())
    print("utterances shortened:", n_taken, "of", len(utts), "rows vocoded:", int(want[:, 1].sum()), "of", len(utts) * T_BATCH)
    assert n_taken >= 16 and n_taken < len(utts)

    def same(res, what):
        for i, ((w, nf), (wr, nfr)) in enumerate(zip(res, ref)):
            assert nf == nfr and np.array_equal(_bits(w), _bits(wr)), (what, i, nf, nfr, int((_bits(w) != _bits(wr)).sum()))

    for sw in (2, 1):                      # 1: the default takes a batch of this size too
        with capi.switches(ZV_VOC_RUNS=sw):
            for graph in (False, True):
                m.set_graph_mode(graph)
                bc = m.prepare_batch(utts)
                for rep in range(2 if graph else 1):
                    for w in bc.wavs:
                        w[:] = np.nan
                    m.poison(0x3C if rep else 0xFF)
                    bc.run()
                    _check_table(m.voc_runs(0), want, (sw, graph, rep))
                    same(bc.results(), (sw, graph, rep))
                # two lanes in flight: begin k, end k - 1
                calls = [m.prepare_batch(utts) for _ in range(3)]
                for k, c in enumerate(calls):
                    for w in c.wavs:
                        w[:] = np.nan
                    m.poison(0x3C if k & 2 else 0xFF, k % 2)       # the lane is idle: its previous batch has ended
                    c.begin(k % 2)
                    if k:
                        calls[k - 1].end((k - 1) % 2)
                calls[-1].end((len(calls) - 1) % 2)
                for lane in (0, 1):
                    _check_table(m.voc_runs(lane), want, (sw, graph, "lane", lane))
                for k, c in enumerate(calls):
                    same(c.results(), (sw, graph, "lane batch", k))
            m.set_graph_mode(False)
    # lanes with the switch at 0, for the record: the references themselves do not depend on the lane
    with capi.switches(ZV_VOC_RUNS=0):
        c = m.prepare_batch(utts)
        c.begin(1)
        c.end(1)
        same(c.results(), "switch 0, lane 1")
        assert m.voc_runs(1).shape[0] == 0


def test_table_is_gone_once_the_arena_it_lay_in_is_reallocated(ckpt):
    """zv_debug_voc_runs must not read a table out of a freed arena: a lane whose arena grows forgets its table"""
    from zerovox_cpp_amd import capi, synth
    path, g, tensors = ckpt("medium")
    m = capi.Model(path, 0)
    try:
        mel = synth.vocoder_mel(g, tensors, 60, 400)
        mel[100:350] = mel[100]
        with capi.switches(ZV_VOC_RUNS=2):
            m.vocode(mel)
            assert m.voc_runs().shape == (1, 4) and m.voc_runs(1).shape[0] == 0      # asking about lane 1 leaves lane 0 selected ...
            assert m.voc_runs().shape == (1, 4)
            ref = m.vocode(mel)                                                      # ... and the next call runs on it as before
            m.reserve(1, 8192)                                                       # the arena grows: a new allocation
            assert m.voc_runs().shape[0] == 0
            m.poison()
            assert np.array_equal(_bits(m.vocode(mel)), _bits(ref)) and m.voc_runs().shape == (1, 4)
    finally:
        m.close()
