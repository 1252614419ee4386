"""-m gpu: loudness (include/zerovox_amd.h "loudness") where tests/test_gpu_loudness.py does not go: other sampling rates, spans of
more than one round of the gate kernel's loops, more utterances than one workgroup of phase B, n_frames = 0, a batch across a launch
group's end, the ceiling's round-down step, and calls around it.

As there, every expectation is the rule restated in numpy (tests/loudness_rule.py) on the design the library returns, and the bits
must match: every field of the result and every sample, no tolerance anywhere.  Every case first asserts, FROM THE RESTATEMENT (its
step energies, blocks, gates and peaks; tests/loudness_shapes.py), that it reaches what it is there for; tests/test_loudness_cpu.py
runs the same assertions without a device.
  * the gate's rounds (loud_gate_kernel walks steps, blocks, short-term sums and peak tiles 64 to a round and carries the gated sums
    and counts between rounds): 64 / 65 and 128 / 129 blocks at 4 000 Hz, 64 / 65 true-peak tiles and the production length of 1 500
    frames (201 blocks, 220 tiles) at 22 050 Hz, each with its maxima inside the first round and behind it, blocks that fail the
    absolute gate in the first round and pass it later, blocks the relative gate drops in every round, and the true peak in the 11
    outputs BEHIND the span;
  * 4 000 Hz (step 400: most chunks meet two steps), 5 120 Hz (step 512: no chunk holds a step edge) and 48 000 Hz (step 4 800) on
    checkpoints that are `tiny` at that rate: single calls on both sides of four and thirty steps, and a ragged batch of five;
  * 130 utterances in one call: three workgroups of phase B, every remainder of the chunk count by its prefetch depth of 8;
  * n_frames = 0: alone, a whole batch of them (phases A, B, C and the peak pass are not launched) and mixed, on a poisoned lane;
  * one batch in two launch groups (2^26 padded samples), every utterance with the bits of its single call;
  * ceilings that need loud_gain's step one bit pattern down, and their neighbours that do not;
  * history: beside a batch in flight on lane 1 (eager and graph), after a much longer and a much shorter call, after lane poisons;
  * a checkpoint at 3 999 Hz: refused by name, and the model synthesizes on."""
import math
import types

import numpy as np
import pytest

import loudness_rule as LR
import loudness_shapes as LS

pytestmark = pytest.mark.gpu

_M = {}
F = np.float32
HOP = LS.HOP


def _model(ckpt, name):
    from zerovox_cpp_amd import capi
    if name not in _M:
        path, g, _ = ckpt(name)
        assert g.hop_size == HOP
        _M[name] = types.SimpleNamespace(m=capi.Model(path, 0), g=g, path=path,
                                         D=capi.loudness_design(g.sampling_rate) if g.sampling_rate >= 4000 else None)
    e = _M[name]
    e.m.set_graph_mode(False)
    return e


@pytest.fixture
def tiny(ckpt):
    e = _model(ckpt, "tiny")
    assert e.g.sampling_rate == 22050 and e.D.step == 2205
    return e


def teardown_module(module):
    for e in _M.values():
        e.m.close()
    _M.clear()


def _ask(q):
    """a capi.Loudness (or None) as the rule's ask"""
    if q is None:
        return LR.ask()
    s = q.struct
    return LR.ask(s.gain, s.target_lufs, s.true_peak_ceiling, s.flags)


def _same(what, got, want):
    (res, out), (wres, wout) = got, want
    assert LR.key(res) == LR.key(wres), (what, res, wres)
    if wout is None:
        assert out is None, what
    else:
        assert out.shape == wout.shape and out.dtype == F, what
        bad = np.flatnonzero(out.view(np.uint32) != wout.view(np.uint32))
        assert bad.size == 0, (what, bad.size, bad[:6], out[bad[0]], wout[bad[0]])


def _asks():
    from zerovox_cpp_amd import capi
    return (None, capi.Loudness(1.0, -16.0, None), capi.Loudness(2.0, None, 0.25), capi.Loudness.from_lufs(-19.0, true_peak_dbtp=-1.0))


# ---- 1. the gate's rounds -----------------------------------------------------------------------------------------------------------------

GATE_COUNTS = {(4000, 90): (64, 14), (4000, 91): (65, 14), (4000, 175): (128, 26), (4000, 176): (129, 26),
               (22050, 436): (56, 64), (22050, 437): (56, 65), (22050, 1500): (201, 220)}          # (blocks, true-peak tiles)


@pytest.mark.parametrize("rate,nf", LS.GATE_CASES)
def test_spans_of_more_than_one_round_of_the_gate(ckpt, rate, nf):
    """A gate kernel that drops the carry of `sum`, `na` or `ng` between rounds fails the 65-, 129- and 201-block cases (both gates keep
    and drop blocks on both sides of block 64); one that reads `peaks` for t < 64 only fails 437 and 1 500 frames, "late" (the true
    peak and the sample peak lie in tile 64 or behind); one that loses a later round's maximum fails every "late" case."""
    from zerovox_cpp_amd import capi
    e = _model(ckpt, "tiny" if rate == 22050 else "tiny_sr%d" % rate)
    m, D = e.m, e.D
    assert e.g.sampling_rate == rate and D.step == (rate + 5) // 10
    N = nf * HOP
    assert (max(N // D.step - 3, 0), (N + 11 + 2047) // 2048) == GATE_COUNTS[(rate, nf)]
    for variant in LS.VARIANTS:
        x = LS.gate_wave(rate, D.step, nf, nf + 2, variant)
        r = LS.gate_reach(D, x, nf, variant)                                  # the reach, from the restatement
        assert (r.blocks, r.tiles) == GATE_COUNTS[(rate, nf)]
        for q in (None, capi.Loudness.from_lufs(-16.0, true_peak_dbtp=-1.0)):
            want = LR.rule(D, x, N, _ask(q))
            assert 0 < want[0].blocks_gated < want[0].blocks_absolute < want[0].blocks == r.blocks
            _same((rate, nf, variant, q), m.loudness_wave(x, q, n_frames=nf), want)


# ---- 2. other rates -------------------------------------------------------------------------------------------------------------------------

RATE_EDGES = {4000: ((5, 6), (39, 40)), 5120: ((6, 7), (51, 52)), 48000: ((63, 64), (479, 480))}      # n_frames on both sides of 4 and 30 steps


def _two_step_chunks(step, nch):
    """how many of the chunks 0 .. nch hold a step edge (loud_edge: their second run is not empty)"""
    k = np.arange(nch, dtype=np.int64)
    return int((((256 * k) // step + 1) * step < 256 * (k + 1)).sum())


@pytest.mark.parametrize("rate", sorted(RATE_EDGES))
def test_other_rates_single_calls_around_the_block_edges(ckpt, rate):
    """Where a chunk meets a step.  At 4 000 Hz more than half of the chunks hold a step edge, at 48 000 Hz about one in nineteen, and a
    phase C that puts the edge's own sample into the wrong run fails both.  At 5 120 Hz the step is two whole chunks and NO chunk holds
    an edge (asserted below from loud_edge's formula): a phase C that sends every sample to run 0 whenever step % 256 == 0 computes the
    rule there, so that is no error a test could see; what this rate pins is phase D adding run 0 of exactly two chunks per step."""
    from zerovox_cpp_amd import capi
    e = _model(ckpt, "tiny_sr%d" % rate)
    m, D = e.m, e.D
    step = D.step
    assert e.g.sampling_rate == rate and step == (rate + 5) // 10 == {4000: 400, 5120: 512, 48000: 4800}[rate]
    (a4, b4), (a30, b30) = RATE_EDGES[rate]
    assert a4 * HOP // step == 3 and b4 * HOP // step == 4 and a30 * HOP // step == 29 and b30 * HOP // step == 30
    if rate == 48000:
        assert b4 * HOP == 4 * step and b30 * HOP == 30 * step                  # exactly four and exactly thirty steps
    if rate == 4000:
        assert b30 * HOP == 30 * step
    nch = -(-b30 * HOP // 256)
    two = _two_step_chunks(step, nch)
    assert {4000: two > nch // 2, 5120: two == 0, 48000: 0 < two < nch // 8}[rate], (two, nch)
    for nf in (a4, b4, a30, b30):
        T, N = nf + 3, nf * HOP
        x = LS.speech(rate, 200 + nf, T * HOP)
        for q in (None, capi.Loudness(1.0, -16.0, None), capi.Loudness.from_lufs(-16.0, true_peak_dbtp=-1.0)):
            want = LR.rule(D, x, N, _ask(q))
            assert want[0].blocks == max(N // step - 3, 0) == {a4: 0, b4: 1, a30: 26, b30: 27}[nf]
            assert (want[0].short_term_max_ms > 0.0) == (nf == b30)
            if q is not None and want[0].blocks:
                assert want[0].blocks_gated > 0 and want[0].gain != F(1.0)     # the target moved the gain
            _same((rate, nf, q), m.loudness_wave(x, q, n_frames=nf), want)


@pytest.mark.parametrize("rate", sorted(RATE_EDGES))
def test_other_rates_ragged_batch_equals_single_calls_and_the_rule(ckpt, rate):
    from zerovox_cpp_amd import capi
    e = _model(ckpt, "tiny_sr%d" % rate)
    m, D = e.m, e.D
    (a4, b4), (a30, b30) = RATE_EDGES[rate]
    nfs = [a4, b30 + 7, b4 + 9, b30, a30]
    Ts = [a4 + 1, b30 + 8, b4 + 12, b30 + 2, a30]
    xs = [LS.speech(rate, 300 + u, T * HOP, (0.1, 0.1, 0.1, 0.5, 0.2)[u]) for u, T in enumerate(Ts)]
    xs[1][:] = 0                                                                # silent
    N2 = nfs[2] * HOP
    xs[2][N2 // 3] = np.nan
    xs[2][N2 // 2], xs[2][N2 // 2 + 1] = np.inf, -np.inf
    xs[4][:nfs[4] * HOP // 2] *= F(0.03)                                        # a quiet half: the relative gate drops its blocks
    asks = [None, capi.Loudness(1.0, -16.0, None), capi.Loudness(2.0, None, 0.25), capi.Loudness(1.0, -6.0, 0.125), capi.Loudness(1.0, -20.0, 1.0)]
    want = [LR.rule(D, x, nf * HOP, _ask(q)) for x, nf, q in zip(xs, nfs, asks)]
    assert want[0][0].blocks == 0 and want[1][0].blocks > 0 and want[1][0].blocks_absolute == 0 and math.isinf(want[1][0].integrated_lufs)
    assert np.isfinite(want[2][0].true_peak) and want[2][0].blocks_gated > 0
    assert 0 < want[4][0].blocks_gated < want[4][0].blocks_absolute <= want[4][0].blocks
    assert want[3][0].gain < F(math.sqrt(_ask(asks[3]).zt / want[3][0].integrated_ms))      # the ceiling won
    single = [m.loudness_wave(x, q, n_frames=nf) for x, nf, q in zip(xs, nfs, asks)]
    for u in range(5):
        _same(("single", rate, u), single[u], want[u])
    for u, got in enumerate(m.loudness_wave_batch(xs, asks, nfs)):
        _same(("batch", rate, u), got, single[u])


# ---- 3. a wide batch ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("base", [0, 30])
def test_130_utterances_in_one_call(tiny, base):
    """n_frames = base + u % 17.  From 0 the spans stay below four steps (8 820 samples): the chunk counts take every remainder by
    the prefetch depth, but no block exists, so no result depends on phase B.  From 30 every utterance has blocks and the remainders are
    all there again: a phase B that runs for the first 64 utterances only fails utterances 64 .. 129 (their phase C would start from
    the z_k phase A left)."""
    m, D = tiny.m, tiny.D
    n = 130
    nfs = [base + u % 17 for u in range(n)]
    Ts = [nf + 1 + u % 3 for u, nf in enumerate(nfs)]
    assert -(-n // 64) == 3                                                     # three workgroups of phase B
    for part in (nfs[:64], nfs[64:]):                                           # every remainder of nch by LOUD_B_AHEAD, behind the first workgroup too
        assert {-(-nf * HOP // 256) % 8 for nf in part} == set(range(8))
    xs = [LS.speech(22050, 400 + u, T * HOP, 0.05 + 0.01 * (u % 7)) for u, T in enumerate(Ts)]
    asks = [_asks()[u % 4] for u in range(n)]
    apply = [u % 5 != 2 for u in range(n)]
    want = [LR.rule(D, x, nf * HOP, _ask(q), out=a) for x, nf, q, a in zip(xs, nfs, asks, apply)]
    if base:
        assert all(w[0].blocks_gated > 0 for w in want)
        assert all(w[0].gain != F(q.gain) for w, q in zip(want, asks) if q is not None and q.target_lufs is not None)
    else:
        assert not any(w[0].blocks for w in want) and want[0][0].true_peak == 0.0 and all(w[0].true_peak > 0.0 for w, nf in zip(want, nfs) if nf)
    batch = m.loudness_wave_batch(xs, asks, nfs, apply=apply)
    for u in range(n):
        _same(("batch", u), batch[u], want[u])
    for u in range(n):
        _same(("single", u), m.loudness_wave(xs[u], asks[u], n_frames=nfs[u], apply=apply[u]), want[u])


# ---- 4. n_frames = 0 ------------------------------------------------------------------------------------------------------------------------

def _nothing_measured(res):
    assert (res.blocks, res.blocks_absolute, res.blocks_gated) == (0, 0, 0)
    assert res.integrated_ms == 0.0 and res.momentary_max_ms == 0.0 and res.short_term_max_ms == 0.0
    assert res.true_peak == 0.0 and res.sample_peak == 0.0 and LR.dbits(res.true_peak) == 0 and LR.fbits(res.sample_peak) == 0
    for v in (res.integrated_lufs, res.momentary_max_lufs, res.short_term_max_lufs, res.true_peak_dbtp):
        assert v == F(-np.inf)


def test_zero_frames_measure_nothing_and_scale_the_capacity(tiny):
    """n_frames = 0: no chunk, no step, no block; in a group of such utterances phases A, B, C and the peak pass are not launched, so
    the gate must not read peaks nobody wrote (the lane is poisoned with 0xFF first: stale peaks would be NaN bit patterns, the largest)."""
    from zerovox_cpp_amd import capi
    m, D = tiny.m, tiny.D
    xs = [LS.speech(22050, 500 + u, T * HOP, 0.3) for u, T in enumerate((3, 1, 40, 8))]
    asks = [capi.Loudness(0.5, None, None), capi.Loudness(2.0, -16.0, None), capi.Loudness(3.0, -16.0, 0.25), None]
    want = [LR.rule(D, x, 0, _ask(q)) for x, q in zip(xs, asks)]
    for (res, out), x, q in zip(want, xs, asks):                                # what the rule says of an empty span
        _nothing_measured(res)
        assert res.gain == F(q.gain if q else 1.0) and (out.view(np.uint32) == (x * res.gain).view(np.uint32)).all()
    # a long measured call first, so that the peak slab holds values of another call
    m.loudness_wave(LS.speech(22050, 510, 100 * HOP, 0.9), None, apply=False)
    for byte in (None, 0xFF, 0x00):
        if byte is not None:
            m.poison(byte, 0)
        for u in range(4):
            got = m.loudness_wave(xs[u], asks[u], n_frames=0)
            _nothing_measured(got[0])
            _same(("single", byte, u), got, want[u])
        if byte is not None:
            m.poison(byte, 0)
        for u, got in enumerate(m.loudness_wave_batch(xs, asks, [0, 0, 0, 0])):     # nothing but the gate and the apply pass runs
            _same(("all zero", byte, u), got, want[u])
        if byte is not None:
            m.poison(byte, 0)
        _same(("meter", byte), m.loudness_wave(xs[2], asks[2], n_frames=0, apply=False), (want[2][0], None))
    # mixed with measured spans: the peak pass runs over the 11-sample tail of the empty ones
    ys = [xs[0], LS.speech(22050, 520, 45 * HOP, 0.2), xs[2], LS.speech(22050, 521, 9 * HOP, 0.4), xs[1]]
    nfs = [0, 44, 0, 9, 0]
    qs = [asks[0], asks[2], asks[2], asks[1], asks[1]]
    mixed = [LR.rule(D, y, nf * HOP, _ask(q)) for y, nf, q in zip(ys, nfs, qs)]
    assert mixed[1][0].blocks > 0 and mixed[1][0].gain != F(3.0) and mixed[3][0].true_peak > 0.0
    for byte in (0xFF, 0x00):
        m.poison(byte, 0)
        for u, got in enumerate(m.loudness_wave_batch(ys, qs, nfs)):
            _same(("mixed", byte, u), got, mixed[u])


# ---- 5. one batch, two launch groups ---------------------------------------------------------------------------------------------------------

def test_a_batch_across_a_launch_groups_end(tiny):
    """Capacities that cross 2^26 padded samples: utterances 0 .. 5 are one launch group, 6 .. 9 the next, whose segment offsets
    (x0, chunk0, step0, tile0) start at 0 again in an I/O block that is reused.  Utterance 0 has many rounds at the head of the first
    group; utterance 6, the head of the second at offset 0, measures nothing.  A kernel that ignores chunk0, step0 or tile0 fails
    utterances 1, 4 and 8, which lie behind measured spans in their group."""
    from zerovox_cpp_amd import capi
    m, D = tiny.m, tiny.D
    tmax = m.max_frames()
    Ts = [32768] * 7 + [50, 50, 1]
    assert tmax >= max(Ts), tmax                                                # (zv_max_frames() caps an utterance at 32 768 frames)
    assert LS.group_ends(Ts, HOP) == [6, 10]                                    # the rule of loud_group_end, restated
    assert sum(-(-T * HOP // 256) * 256 for T in Ts[:6]) <= LS.GROUP_SAMPLES < sum(-(-T * HOP // 256) * 256 for T in Ts[:7])
    nfs = [5000, 40, 0, 7, 300, 1, 0, 50, 45, 1]
    block = LS.speech(22050, 600, 1 << 20, 0.3)
    xs = [np.resize(np.roll(block, 4099 * u), T * HOP) * F(0.5 + 0.1 * u) for u, T in enumerate(Ts)]
    assert all(x.dtype == F for x in xs)
    a = _asks()
    asks = [a[3], a[1], None, a[2], a[1], a[3], a[2], a[1], a[3], a[2]]
    apply = [True, False, False, False, False, False, True, True, True, True]
    keep = [xs[0][:HOP * 64].copy(), xs[1].copy()]
    want = [LR.rule(D, x, nf * HOP, _ask(q), out=ap) for x, nf, q, ap in zip(xs, nfs, asks, apply)]
    assert want[0][0].blocks == 5000 * HOP // 2205 - 3 > 10 * LS.ROUND and want[4][0].blocks == 37 and want[7][0].blocks == want[8][0].blocks == 3
    assert want[0][0].gain != F(1.0) and want[1][0].gain != F(1.0) and want[8][0].gain != F(1.0) and want[6][0].gain == F(2.0)
    batch = m.loudness_wave_batch(xs, asks, nfs, apply=apply)
    for u in range(len(Ts)):
        _same(("batch", u), batch[u], want[u])
    assert np.array_equal(xs[0][:HOP * 64].view(np.uint32), keep[0].view(np.uint32)) and np.array_equal(xs[1].view(np.uint32), keep[1].view(np.uint32))
    del batch, want
    for u in (0, 1, 6, 8, 9):                                                    # the single calls, metering (the outputs were compared above)
        res, out = m.loudness_wave(xs[u], asks[u], n_frames=nfs[u], apply=False)
        assert out is None and LR.key(res) == LR.key(LR.rule(D, xs[u], nfs[u] * HOP, _ask(asks[u]), out=False)[0]), u


# ---- 6. the ceiling's round-down step -----------------------------------------------------------------------------------------------------------

def test_ceilings_that_need_the_round_down_step(tiny):
    """A loud_gain without its loop returns (float)(ceiling / tp) and fails every ceiling of `needs`."""
    from zerovox_cpp_amd import capi
    m, D = tiny.m, tiny.D
    x = LS.round_down_wave()
    base = LR.rule(D, x, x.size, out=False)[0]
    tp = base.true_peak
    needs, plain = LS.round_down_split(tp)
    assert len(needs) >= 3 and all(LR.gain(LR.ask(LS.ROUND_DOWN_GAIN, 0.0, c, LR.CEILING), 0.0, tp) != F(float(c) / tp) for c in needs)
    near = [LS.ROUND_DOWN_CEILINGS[k + d] for k, c in enumerate(LS.ROUND_DOWN_CEILINGS) if c in needs for d in (-1, 1)
            if 0 <= k + d < len(LS.ROUND_DOWN_CEILINGS) and LS.ROUND_DOWN_CEILINGS[k + d] in plain]
    assert len(near) >= 3
    for c in needs + near:
        q = capi.Loudness(LS.ROUND_DOWN_GAIN, None, float(c))
        g = LR.gain(_ask(q), base.integrated_ms, tp)
        assert (g != F(float(c) / tp)) == (c in needs)
        res, out = m.loudness_wave(x, q)
        _same(("ceiling", c), (res, out), (types.SimpleNamespace(**{**vars(base), "gain": g}), x * g))
        assert F(float(res.gain) * res.true_peak) <= c, (c, res)
    # the same ceilings as one batch
    qs = [capi.Loudness(LS.ROUND_DOWN_GAIN, None, float(c)) for c in needs + near]
    for c, (res, out) in zip(needs + near, m.loudness_wave_batch([x] * len(qs), qs)):
        assert LR.fbits(res.gain) == LR.fbits(LR.gain(LR.ask(LS.ROUND_DOWN_GAIN, 0.0, c, LR.CEILING), 0.0, tp)), c


# ---- 7. history -------------------------------------------------------------------------------------------------------------------------------

def _utterances(g):
    from zerovox_cpp_amd import synth
    return [(*synth.encoder_inputs(g, 8300 + i, N), T) for i, (N, T) in enumerate(((6, 40), (3, 17), (9, 64)))]


def test_calls_around_it_leave_the_bits_unchanged(tiny):
    from zerovox_cpp_amd import capi
    m, D, g = tiny.m, tiny.D, tiny.g
    Ts, nfs = [20, 40, 75, 230], [20, 40, 71, 226]
    xs = [LS.speech(22050, 700 + u, T * HOP, (0.1, 0.1, 0.2, 0.5)[u]) for u, T in enumerate(Ts)]
    xs[1][:] = 0
    xs[2][:35 * HOP] *= F(0.05)
    asks = [None, capi.Loudness(1.0, -16.0, None), capi.Loudness(1.0, -20.0, 1.0), capi.Loudness(1.0, -6.0, 0.125)]
    want = [LR.rule(D, x, nf * HOP, _ask(q)) for x, nf, q in zip(xs, nfs, asks)]
    assert 0 < want[2][0].blocks_gated < want[2][0].blocks_absolute and want[3][0].short_term_max_ms > 0.0

    def check(what):
        for u, got in enumerate(m.loudness_wave_batch(xs, asks, nfs)):
            _same((what, "batch", u), got, want[u])
        _same((what, "single"), m.loudness_wave(xs[3], asks[3], n_frames=nfs[3]), want[3])

    check("quiescent")
    utts = _utterances(g)
    plain = m.synthesize_batch(utts)
    for graph in (False, True, True):                                          # eager, graph capture, graph replay
        m.set_graph_mode(graph)
        bc = m.prepare_batch(utts)
        bc.begin(1)
        check(("beside a batch in flight on lane 1", graph))
        bc.end(1)
        for (w0, n0), (w1, n1) in zip(plain, bc.results()):                     # and the batch beside it is what it is alone
            assert n0 == n1 and np.array_equal(w0.view(np.uint32), w1.view(np.uint32)), graph
        check(("after the batch", graph))
    m.set_graph_mode(False)
    long = LS.speech(22050, 710, 3000 * HOP, 0.4)                               # the I/O block grows ...
    first = m.loudness_wave(long, asks[3], n_frames=2990)
    check("after a much longer call")
    m.loudness_wave(xs[0][:HOP], None)                                          # ... and is reused by a call of one frame
    check("after a much shorter call")
    _same("the long call again", m.loudness_wave(long, asks[3], n_frames=2990), first)
    for byte in (0x00, 0xFF):
        m.poison(byte, 0)
        check(("poison", byte))
        m.poison(byte, 1)
        m.poison(byte, 0)
        _same(("poison, single", byte), m.loudness_wave(xs[2], asks[2], n_frames=nfs[2]), want[2])


# ---- 8. the rate loudness refuses -------------------------------------------------------------------------------------------------------------

def test_a_checkpoint_at_3999_hz_is_refused_by_name(ckpt):
    from zerovox_cpp_amd import capi, synth
    e = _model(ckpt, "tiny_sr3999")
    m, g = e.m, e.g
    assert g.sampling_rate == 3999
    x = LS.speech(4000, 800, 12 * HOP)
    ids, puncts, style = synth.encoder_inputs(g, 9, 12)
    before = m.synthesize(ids, puncts, style, 64)[:2]
    for call in (lambda: m.loudness_wave(x), lambda: m.loudness_wave(x, capi.Loudness(1.0, -16.0, None), n_frames=0),
                 lambda: m.loudness_wave_batch([x, x])):
        with pytest.raises(capi.ZvError, match=r"audio_sampling_rate = 3999 must be in 4000 \.\. 768000") as err:
            call()
        assert err.value.status == 5
    after = m.synthesize(ids, puncts, style, 64)[:2]
    assert before[1] == after[1] > 0 and np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32))
