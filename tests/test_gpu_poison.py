"""-m gpu: no call may read what it did not write (include/zerovox_amd.h zv_debug_poison).

A lane keeps its activation arena, its device I/O block and its pinned staging block between calls, and the layout of each is a
function of the shapes alone: the second of two equal calls finds the first one's data at the same offsets, so a write that does
not happen (a fill kernel that is not launched, a copy that is not enqueued, a zeroed tail that is skipped) leaves the right values
behind and no bitwise A/B on one lane can see it.  Every case here runs as

    poison, call (allocates, captures in graph mode; compared);  for fill in (0xFF, 0x3C): poison(lane) -> call -> compare

against a second model that is never poisoned and sees each distinct call once, stand-alone and eagerly, with run-shortened
vocoding off.  Comparisons are of uint32 views.  0xFF bytes read as NaN in f32 and f16 and as -1 in an int32; 0x3C bytes as 0.0115
in f32 and 1.06 in f16, finite, so that a stale read shows where fmaxf / fminf, a clamp or an (int) cast swallows a NaN; 0x00 is
what a fresh arena holds and proves nothing.  After every poison the bytes it reports must cover what the call before it used (at
least the waveform and the mel in the I/O block, the waveforms in the pinned block of a batch): a hook that did nothing fails."""
import numpy as np
import pytest

from parity_helpers import BATCH_REGIME
from test_gpu_fitted import _forced
from test_gpu_voc_runs import _batch, _cases
from test_voc_runs_cpu import MARGIN, run_entry

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0x3C)
REGIMES = {"default": {}, "batch_regime": BATCH_REGIME}
_M = {}


@pytest.fixture(scope="module")
def ref(ckpt):
    """the reference model (never poisoned) and the cache of what it gave: get(key, fn) runs fn(model) once per key, with the
    switches at their defaults but for run-shortened vocoding, which is off"""
    from zerovox_cpp_amd import capi
    path, g, tensors = ckpt("medium")
    if "ref" not in _M:
        _M.update(ref=capi.Model(path, 0), cache={}, path=path, g=g, t=tensors)

    def get(key, fn):
        if key not in _M["cache"]:
            assert capi.debug_get("ZV_CONV_GEMM") == 1 and capi.debug_get("ZV_VOC_RUNS") == 1      # no regime is in force
            with capi.switches(ZV_VOC_RUNS=0):
                _M["cache"][key] = fn(_M["ref"])
        return _M["cache"][key]

    return get


@pytest.fixture(scope="module")
def under_test(ckpt):
    """name -> the model under test of that regime: a model of its own per regime (and per `extra`), so that no regime finds another's
    buffers.  Every switch is read at the call: the tests make their calls inside capi.switches(**REGIMES[name], **extra)"""
    from zerovox_cpp_amd import capi
    path, _, _ = ckpt("medium")

    def get(name, **extra):
        key = (name,) + tuple(sorted(extra.items()))
        if key not in _M:
            _M[key] = capi.Model(path, 0)
        _M[key].set_graph_mode(False)
        return _M[key]

    return get


def teardown_module(module):
    for v in _M.values():
        if hasattr(v, "close"):
            v.close()
    _M.clear()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype.itemsize == 4 else x


def _same(got, want, what):
    """tuples / lists / dicts of arrays and integers, compared as bits"""
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), what
        for k in want:
            _same(got[k], want[k], (what, k))
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want), what
        for i, (a, b) in enumerate(zip(got, want)):
            _same(a, b, (what, i))
    elif isinstance(want, np.ndarray):
        a, b = _bits(got), _bits(want)
        assert a.shape == b.shape and np.array_equal(a, b), (what, int((a != b).sum()) if a.shape == b.shape else (a.shape, b.shape))
    else:
        assert got == want, (what, got, want)


def _poisoned(m, call, check, need, lanes=(0,), what=None, prime=True):
    """the module's protocol.  need = (arena, io, pinned) bytes the call is known to use at the least: what every poison after a
    call must report for each of its lanes"""
    if prime:
        for lane in lanes:
            m.poison(FILLS[-1], lane)
        check(call(), (what, "first call"))
    for fill in FILLS:
        for lane in lanes:
            filled = m.poison(fill, lane)
            assert all(f >= n for f, n in zip(filled, need)) and filled[0] > 0, (what, "poison reports", filled, "the call needs", need)
        check(call(), (what, hex(fill)))


# ---- 1. single entry points -----------------------------------------------------------------------------------------------------

SINGLE_T, SINGLE_N, CHUNK = (1, 33, 255, 256, 257, 400), 24, 64


def _single_ops(g, tensors, T):
    """name -> (call(model), bytes of the I/O block the call needs at the least)"""
    from zerovox_cpp_amd import synth
    hop, M, E, N = g.hop_size, g.num_mels, g.E, SINGLE_N
    ids, puncts, style = synth.encoder_inputs(g, 7000 + T, N)
    mel = synth.vocoder_mel(g, tensors, 7100 + T, T)
    hid = synth.decoder_hidden(g, 7200 + T, T)
    half = dict(duration_frames=_forced(N, (T + 1) // 2))         # fitted: half of the capacity stays silent
    io_chain = T * (hop + M + E) * 4
    return {
        "vocode": (lambda m: m.vocode(mel), T * (hop + M) * 4),
        "decode": (lambda m: m.decode(hid, style), T * (E + M) * 4),
        "encode": (lambda m: m.encode(ids, puncts, style, T, return_durations=True), T * E * 4),
        "synthesize": (lambda m: m.synthesize(ids, puncts, style, T, return_durations=True), io_chain),
        "synthesize_fitted": (lambda m: m.synthesize(ids, puncts, style, T, phonemes=half, return_durations=True, fitted=True), io_chain),
        "vocode_stream": (lambda m: m.vocode_stream(mel, CHUNK), (T * M + min(T, CHUNK) * hop) * 4),
    }


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_single_entry_points(ref, under_test, regime, graph):
    from zerovox_cpp_amd import capi
    g, tensors = _M["g"], _M["t"]
    ops = {T: _single_ops(g, tensors, T) for T in SINGLE_T}
    want = {(T, name): ref(("single", T, name), fn) for T in SINGLE_T for name, (fn, _) in ops[T].items()}
    assert want[(400, "synthesize_fitted")][1] == 200 and want[(400, "synthesize")][1] < 400
    m = under_test(regime)
    with capi.switches(**REGIMES[regime]):
        m.set_graph_mode(graph)                  # graph: capture, poison, replay, poison, replay
        for T in SINGLE_T:
            for name, (fn, need_io) in ops[T].items():
                _poisoned(m, lambda: fn(m), lambda got, what: _same(got, want[(T, name)], what), (0, need_io, 0), what=(regime, graph, T, name))
        m.set_graph_mode(False)


# ---- 2. ragged batch ------------------------------------------------------------------------------------------------------------

RAGGED_NT = ((1, 1), (340, 2), (5, 11), (60, 54), (1, 55), (64, 255), (33, 256), (97, 257))
# forced frame counts: four utterances fill their capacity (no run behind them), two leave T - n_frames >= 29 + 2H + 1 + 16 + 8
# frames (the constant run starts within 14 frames of n_frames and ends within 15 of T, tests/test_voc_runs_cpu.py: it qualifies)
RAGGED_NF = (1, 2, 7, 30, 55, 100, 138, 257)
PROSODY = dict(duration_scale=1.3, pitch_scale=0.9, pitch_shift=0.05, energy_scale=1.1, energy_shift=-0.03)


def _ragged(g, controls):
    """utterances (ids, puncts, style, T, prosody, phonemes)"""
    from zerovox_cpp_amd import synth
    rng = np.random.default_rng(23)
    out = []
    for i, ((N, T), nf) in enumerate(zip(RAGGED_NT, RAGGED_NF)):
        pc = dict(duration_frames=_forced(N, nf), pitch_shift=rng.uniform(-0.2, 0.2, N).astype(np.float32),
                  energy_shift=rng.uniform(-0.2, 0.2, N).astype(np.float32))
        out.append((*synth.encoder_inputs(g, 7300 + i, N), T) + ((PROSODY if i % 2 else None, pc) if controls else (None, None)))
    return out


def _alone(ref, tag, utts, fitted, H):
    """per utterance, from the reference model: (wav, n_frames, durations) of the stand-alone call, and the run-table entry the
    unfitted schedule owes for the mel of the stand-alone stages (H None: not asked for)"""
    res, runs = [], []
    for i, (ids, puncts, style, T, pr, pc) in enumerate(utts):
        res.append(ref((tag, i, fitted), lambda r: r.synthesize(ids, puncts, style, T, prosody=pr, phonemes=pc, return_durations=True, fitted=fitted)))
        if H is not None:
            runs.append(ref((tag, i, "run"), lambda r: run_entry(r.decode(r.encode(ids, puncts, style, T, prosody=pr, phonemes=pc)["hidden"], style), H)))
    return res, runs


def _batch_call(bc, lane=None):
    for w in bc.wavs:
        w[:] = np.nan
    if lane is None:
        bc.run()
    else:
        bc.begin(lane)
        bc.end(lane)
    return [r + ((d,) if bc.durations is not None else ()) for r, d in zip(bc.results(), bc.durations or [None] * bc.n)]


def _table(utts, runs):
    rows, row0 = [], 0
    for u, e in zip(utts, runs):
        rows.append((row0,) + e)
        row0 += u[3]
    return np.array(rows, np.int32)


def _need(g, utts):
    """(arena, io, pinned) bytes a batch of these utterances needs at the least"""
    rows = sum(u[3] for u in utts)
    return 0, rows * (g.hop_size + g.num_mels) * 4, rows * g.hop_size * 4


@pytest.mark.parametrize("fitted", [False, True], ids=["unfitted", "fitted"])
@pytest.mark.parametrize("controls", [True, False], ids=["controls", "plain"])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_ragged_batch(ref, under_test, regime, controls, fitted):
    from zerovox_cpp_amd import capi
    g = _M["g"]
    m = under_test(regime)
    H = m.vocoder_halo_frames()
    utts = _ragged(g, controls)
    want, runs = _alone(ref, ("ragged", controls), utts, fitted, H)
    if controls:
        nfs = [w[1] for w in want]
        assert nfs == list(RAGGED_NF), nfs
        assert sum(nf == u[3] for nf, u in zip(nfs, utts)) >= 2
        assert sum(u[3] - nf >= 29 + 2 * H + 1 + MARGIN + 8 for nf, u in zip(nfs, utts)) >= 2
        assert sum(e[2] > 0 for e in runs) >= 2 and sum(e[2] == 0 for e in runs) >= 2, runs      # runs taken and not taken
    else:
        # the duration predictor's own lengths (the CPU oracle gives 1, 2, 11, 54, 4, 234, 94, 257 frames): only the (33, 256)
        # utterance leaves the 118 frames a run needs behind it, the (1, 55) one has too little capacity for any run
        assert sum(e[2] > 0 for e in runs) >= 1 and sum(e[2] == 0 for e in runs) >= 2, runs
    sw = dict(REGIMES[regime], **({"ZV_VOC_RUNS": 2} if regime != "default" else {}))
    with capi.switches(**sw):
        # else no table: the default switch takes a batch from 16 384 rows of capacity on, and this one has t_rows = 8 utterances x 320
        # (the longest T, 257, rounded up to 64) = 2 560
        table = sw.get("ZV_VOC_RUNS") == 2 and not fitted

        def check_for(order):
            us, ws = [utts[i] for i in order], [want[i] if controls else want[i][:2] for i in order]
            tab = _table(us, [runs[i] for i in order])

            def check(got, what):
                _same(got, ws, what)
                t = m.voc_runs()
                assert (t.shape == tab.shape and np.array_equal(t, tab)) if table else t.shape[0] == 0, (what, t.tolist(), tab.tolist())
            return us, check

        ident, rot = list(range(len(utts))), list(range(1, len(utts))) + [0]
        for graph in (False, True):
            # graph: capture, two replays, then two more replays of that same graph by a batch of the utterances rotated by one.  A
            # chain graph is keyed by the batch's capacities (count, longest N and T rounded up, rows) and its buffers
            # (Batch::same_schedule), which the rotation keeps; every utterance's own (N, T) is in the device tables, which the
            # kernels read when they run: another slot for every utterance, other offsets, no new capture
            m.set_graph_mode(graph)
            us, check = check_for(ident)
            bc = m.prepare_batch(us, durations=controls, fitted=fitted)
            _poisoned(m, lambda: _batch_call(bc), check, _need(g, us), what=(regime, controls, fitted, graph))
            if graph:
                us, check = check_for(rot)
                bc = m.prepare_batch(us, durations=controls, fitted=fitted)
                _poisoned(m, lambda: _batch_call(bc), check, _need(g, us), what=(regime, controls, fitted, "rotated"), prime=False)
        m.set_graph_mode(False)


@pytest.mark.parametrize("regime", list(REGIMES))
def test_fitted_batch_with_an_empty_utterance_between_neighbours(ref, under_test, regime):
    from zerovox_cpp_amd import capi, synth
    g = _M["g"]
    m = under_test(regime)
    base = _ragged(g, True)
    N, T = 12, 130
    empty = (*synth.encoder_inputs(g, 7400, N), T, None, dict(duration_frames=np.zeros(N, np.int32)))
    utts = [base[3], empty, base[5]]
    want, _ = _alone(ref, "empty", utts, True, m.vocoder_halo_frames())
    assert [w[1] for w in want] == [30, 0, 100] and not want[1][0].any()
    with capi.switches(**REGIMES[regime]):
        for graph in (False, True):
            m.set_graph_mode(graph)
            bc = m.prepare_batch(utts, durations=True, fitted=True)
            _poisoned(m, lambda: _batch_call(bc), lambda got, what: _same(got, want, what), _need(g, utts), what=(regime, graph))
        m.set_graph_mode(False)


# ---- 3. run-shortened zv_vocode -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_run_shortened_vocode_of_hand_made_mels(ref, under_test, graph):
    from zerovox_cpp_amd import capi
    g, tensors = _M["g"], _M["t"]
    m = under_test("default")
    H, hop, M = m.vocoder_halo_frames(), g.hop_size, g.num_mels
    cases = _cases(g, tensors, H)
    want = {name: ref(("hand-made", name), lambda r: r.vocode(mel)) for name, (mel, _) in cases.items()}      # the switch at 0
    taken = 0
    with capi.switches(ZV_VOC_RUNS=2):
        for name, (mel, run) in cases.items():
            T = mel.shape[0]
            tab = np.array([(0,) + run_entry(mel, H)], np.int32)
            taken += int(tab[0, 3] > 0)
            assert (tab[0, 3] > 0) == (run is not None), name

            def check(got, what):
                _same(got, want[name], what)
                t = m.voc_runs()
                assert t.shape == tab.shape and np.array_equal(t, tab), (what, t.tolist(), tab.tolist())

            m.set_graph_mode(graph)
            _poisoned(m, lambda: m.vocode(mel), check, (0, T * (hop + M) * 4, 0), what=(name, graph))
            # device-resident: the waveform lands in a buffer of the caller's, which is no lane block: the test fills it
            d_mel, d_wav = m.device_alloc(mel.nbytes), m.device_alloc(T * hop * 4)
            try:
                m.h2d(d_mel, mel)

                def device_call():
                    m.h2d(d_wav, np.full(T * hop, np.nan, np.float32))
                    m.vocode_device(d_mel, T, d_wav)
                    m.synchronize()
                    out = np.empty(T * hop, np.float32)
                    m.d2h(out, d_wav)
                    return out

                _poisoned(m, device_call, check, (0, T * (hop + M) * 4, 0), what=(name, graph, "device"))
            finally:
                m.device_free(d_mel)
                m.device_free(d_wav)
            m.set_graph_mode(False)
    assert taken >= 8


# ---- 4. tail groups -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fitted", [False, True], ids=["unfitted", "fitted"])
@pytest.mark.parametrize("groups", [8, 5])
def test_tail_groups(ref, under_test, groups, fitted):
    """32 utterances x 512 frames, 19.7 MB of waveform: the last vocoder stage runs in utterance groups, each group's waveforms
    travel to the pinned block on the copy stream"""
    from zerovox_cpp_amd import capi
    g = _M["g"]
    utts = [u + (None, None) for u in _batch(g)]
    assert sum(u[3] for u in utts) * g.hop_size * 4 >= 16 << 20
    want = [w[:2] for w in _alone(ref, "tail", utts, fitted, None)[0]]
    assert any(nf == u[3] for (_, nf), u in zip(want, utts)) and sum(nf < u[3] // 2 for (_, nf), u in zip(want, utts)) >= 8
    m = under_test("default", ZV_TAIL_GROUPS=groups)
    need = _need(g, utts)

    def check(lane):
        def f(got, what):
            _same(got, want, what)
            t = m.voc_runs(lane)                 # 16 Ki frames of capacity: the default switch shortens the unfitted batch
            assert t.shape[0] == 0 if fitted else (t.shape == (len(utts), 4) and int((t[:, 3] > 0).sum()) >= 8), (what, t.tolist())
        return f

    with capi.switches(ZV_TAIL_GROUPS=groups):       # read when a batch is enqueued: every batch call of the test sits in here
        bc = m.prepare_batch(utts, fitted=fitted)
        _poisoned(m, lambda: _batch_call(bc), check(0), need, what=(groups, fitted, "lane 0"))
        # two batches in flight on lanes 0 and 1, each lane poisoned while it is idle (the other one is not), before its begin
        calls = [m.prepare_batch(utts, fitted=fitted) for _ in range(2)]
        for k in range(4):
            lane = k % 2
            if k >= 2:
                calls[lane].end(lane)
                check(lane)(calls[lane].results(), (groups, fitted, "in flight", k - 2))
                assert all(f >= n for f, n in zip(m.poison(FILLS[k % 2 ^ 1], lane), need)), (groups, fitted, k)
            else:
                m.poison(FILLS[k], lane)
            for w in calls[lane].wavs:
                w[:] = np.nan
            calls[lane].begin(lane)
        for lane in (0, 1):
            calls[lane].end(lane)
            check(lane)(calls[lane].results(), (groups, fitted, "in flight", 2 + lane))


# ---- 5. the hook's own contract -------------------------------------------------------------------------------------------------

def test_the_hooks_contract(ref, ckpt):
    from zerovox_cpp_amd import capi, synth
    path, g, tensors = ckpt("medium")
    hop, M = g.hop_size, g.num_mels
    m = capi.Model(path, 0)
    try:
        for lane in range(capi.BATCH_LANES):
            assert m.poison(0xFF, lane) == (0, 0, 0), lane                        # a fresh model: nothing to fill, nothing allocated
        assert m.poison(0xFF, 0) == (0, 0, 0)
        T = 400
        mel = synth.vocoder_mel(g, tensors, 60, T)
        mel[100:350] = mel[100]
        want = ref(("contract", "vocode"), lambda r: r.vocode(mel))
        with capi.switches(ZV_VOC_RUNS=2):
            _same(m.vocode(mel), want, "vocode")
            assert m.voc_runs().shape == (1, 4)
            arena, io, pinned = m.poison(0x3C, 0)
            assert arena > 0 and io >= T * (hop + M) * 4 and pinned == 0          # zv_vocode stages nothing in pinned memory
            assert m.voc_runs().shape[0] == 0                                     # the table lay in the arena
            _same(m.vocode(mel), want, "vocode after the poison")
            assert m.voc_runs().shape == (1, 4) and m.voc_runs()[0, 3] > 0        # and the next call gives it again
        for byte in (-1, 256, 1 << 20):
            with pytest.raises(capi.ZvError) as e:
                m.poison(byte, 0)
            assert e.value.status == 5, byte
        for lane in (capi.BATCH_LANES, 1 << 20):
            with pytest.raises(capi.ZvError) as e:
                m.poison(0xFF, lane)
            assert e.value.status == 5, lane
        _same(m.vocode(mel), want, "vocode after the refused calls")
        # a lane with a batch in flight is refused and left alone
        utts = [(*synth.encoder_inputs(g, 7500 + i, N), t) for i, (N, t) in enumerate(((20, 96), (7, 33), (40, 200)))]
        alone = [ref(("contract", i), lambda r: r.synthesize(*u)) for i, u in enumerate(utts)]
        bc = m.prepare_batch(utts)
        for rep in range(2):                     # the second time the lane's blocks exist and hold the batch's data
            for w in bc.wavs:
                w[:] = np.nan
            bc.begin(1)
            with pytest.raises(capi.ZvError) as e:
                m.poison(0xFF, 1)
            assert e.value.status == 5 and "in flight" in str(e.value)
            assert m.poison(0xFF, 0)[0] > 0 and m.poison(0xFF, 2) == (0, 0, 0)    # the other lanes are idle
            bc.end(1)
            _same(bc.results(), alone, ("the batch in flight", rep))
        assert all(f >= n for f, n in zip(m.poison(0xFF, 1), _need(g, [u + (None, None) for u in utts])))
        # poisoning lane 1 leaves lane 0 selected: zv_model_reserve grows the selected lane's arena
        m.vocode(mel)
        a0, a1 = m.poison(0xFF, 0)[0], m.poison(0xFF, 1)[0]
        m.reserve(1, 8192)
        assert m.poison(0xFF, 0)[0] > a0 and m.poison(0xFF, 1)[0] == a1
    finally:
        m.close()
