"""-m gpu: history independence across every entry point, every per-utterance ask and the cached graphs, on the "small" synthetic
checkpoint.  tests/test_gpu_state_machine.py walks the six oldest kinds of call; this file walks all of them on ONE model (tests/
call_history.py: the synthesize forms with a menu of nine asks, batches on lanes 0 and 1 and in pairs, the stage batches, the
stand-alone waveform calls, the device-resident calls) between graph mode changes, cache capacities 1, 2 and 16, reserves and lane
poisons.  The expectation needs no reference of its own: every call must give the bits of the same call made once, eagerly, on a
second model that is never poisoned (a batch on a lane: its synthesize_batch; a pair: its two batches).  No tolerance anywhere.

The walk makes the collisions a graph key, a regrown I/O block or a stale per-lane parameter block would show in (the counts are
asserted on the CPU, tests/test_call_history_cpu.py); three directed tests state one interleaving each:
  * asks alternating at ONE shape under graph mode, stand-alone and as batches on lanes 0 and 1, at cache capacities 16 and 1;
  * stand-alone analysis calls that regrow lane 0's I/O block between two replays of a synth graph and a batch graph;
  * the lane-0 calls beside a batch in flight on lane 1, and refused (status 5, "lane 0 has a batch in flight") beside one on lane 0."""
import os

import numpy as np
import pytest

import call_history as CH

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("ZV_SM_SEED", "2024"))
ERR_ARG = 5
_M = {}


class _Reference:
    """the second model: graph mode off, the default cache, never poisoned; every canonical key is run once and kept"""

    def __init__(self, model, ctx):
        self.model, self.ctx, self.kept = model, ctx, {}

    def __call__(self, key, make=None):
        if key not in self.kept:
            self.kept[key] = make(self.model, self.ctx) if make else CH.run_parts(self.model, key, self.ctx)[0]
        return self.kept[key]


@pytest.fixture(scope="module")
def env(ckpt):
    """(fresh, ref): fresh() loads the model under test with its Context (one per test, closed behind it); ref the shared reference"""
    from zerovox_cpp_amd import capi
    path, g, tensors = ckpt("small")
    if "ref" not in _M:
        b = capi.Model(path, 0)
        _M["ref"] = _Reference(b, CH.Context(b, g, tensors))
    opened = []

    def fresh():
        done()                                     # two models at a time: this one and the reference
        m = capi.Model(path, 0)
        opened.append((m, CH.Context(m, g, tensors)))
        return opened[-1]

    def done():
        while opened:
            m, ctx = opened.pop()
            ctx.close()
            m.close()
    yield fresh, _M["ref"], done
    done()


def teardown_module(module):
    if "ref" in _M:
        _M["ref"].ctx.close()
        _M["ref"].model.close()
    _M.clear()


def _invariants(s):
    """the cache's counters add up (tests/test_gpu_graph_cache.py)"""
    assert s["lookups"] == s["hits"] + s["captures"], s
    assert s["captures"] == s["entries"] + s["evictions"] + s["stale_evictions"] + s["lane_drops"] + s["full_drops"], s
    assert s["entries"] <= s["capacity"] and s["retired"] <= s["capacity"], s


def _check(model, ctx, ref, key, what):
    """makes the call of `key` and compares every part with the reference"""
    for part, got in zip(CH.parts(key), CH.run_parts(model, key, ctx)):
        CH.same(got, ref(part), (what, key))


# ---- the walk -------------------------------------------------------------------------------------------------------------------------

def test_every_entry_point_in_one_history(env):
    """A repeat's promise: an identical call made back to back under graph mode costs no capture (test_a_repeated_shape_costs_no_capture,
    here for every form).  An LRU cache of capacity c keeps the c graphs used last, so the promise can hold only for a call that
    looks up at most c graphs; a call that needs more (a pair of batches at capacity 1) is exempt, and counted."""
    fresh, ref, done = env
    a, ctx = fresh()
    steps = CH.history(SEED, CH.STEPS)
    want = CH.coverage(steps)
    repeat_at = set(CH.repeats(steps))
    filed = {}
    cost = {}
    counts = dict(calls=0, poisons=0, pairs=0, repeats=0, repeats_exempt=0)
    for i, s, graph, cache in CH.walk(steps):
        if s[0] in CH.STATE_OPS:
            CH.apply_state(a, s)
            counts["poisons"] += s[0] == "poison"
            continue
        s0 = a.graph_cache_stats().as_dict()
        outs = CH.run_parts(a, s, ctx)
        s1 = a.graph_cache_stats().as_dict()
        assert s0["capacity"] == cache, (i, s0, cache)
        cost[i] = (s1["lookups"] - s0["lookups"], s1["captures"] - s0["captures"])
        assert graph or cost[i] == (0, 0), (i, s, cost[i])                 # graph mode off goes past the cache
        for part, out in zip(CH.parts(s), outs):
            filed.setdefault(part, []).append((i, out))
        counts["calls"] += len(CH.calls_of(s))
        counts["pairs"] += s[0] == "pair"
        if i in repeat_at:
            counts["repeats"] += 1
            if cost[i - 1][0] <= cache:
                assert cost[i] == (cost[i - 1][0], 0), ("a repeat cost a capture", i, s, "capacity", cache, "first", cost[i - 1], "again", cost[i])
            else:
                counts["repeats_exempt"] += 1
    a.set_graph_mode(False)
    stats = a.graph_cache_stats().as_dict()
    _invariants(stats)
    assert stats["hits"] > 0 and stats["captures"] > 0, stats
    # the second model: every distinct call once, eagerly, in sorted order (a different history)
    for part in sorted(filed, key=repr):
        expect = ref(part)
        for i, got in filed[part]:
            CH.same(got, expect, ("step", i, steps[i], "after", steps[i - 1]))
    counts["distinct"] = len(filed)
    print(f"{counts['calls']} calls, {counts['distinct']} distinct, {counts['poisons']} poisons, {counts['pairs']} pairs in flight, "
          f"{counts['repeats']} repeats under graph mode ({counts['repeats_exempt']} need more graphs than the cache holds), "
          f"{want['successions']} same-shape successions ({want['successions_lane1']} on lane 1), {want['sandwiches']} analysis sandwiches; {stats}")
    assert [counts[k] for k in ("calls", "distinct", "poisons", "pairs", "repeats")] == [want[k] for k in ("calls", "distinct", "poisons", "pairs", "repeats")]
    assert counts["repeats"] - counts["repeats_exempt"] >= 8, counts
    done()


# ---- directed: asks alternating at one shape --------------------------------------------------------------------------------------------

NOTHING, EVERYTHING, MIXED = (CH.MENU.index(k) for k in ("nothing", "everything", "mixed"))


def test_alternating_asks_at_one_shape_under_graph_mode(env):
    """N = 24, T = 64, stand-alone and as a batch of three on lane 0 and on lane 1; the asks go nothing, everything, mixed, nothing,
    everything, mixed, nothing with both lanes poisoned between the runs; once with the Level asked for throughout (a call that asks
    for nothing then gets the identity row) and once as the menu has the asks (nothing: the plain form)"""
    from zerovox_cpp_amd import synth
    fresh, ref, done = env
    a, ctx = fresh()
    N, T = 24, 64
    plain = [ref(("plain", N, T, s), lambda m, c, s=s: [m.synthesize(*synth.encoder_inputs(c.g, s, N), T)[0].copy()])[0] for s in range(3)]
    one = np.array([1.0], np.float32).view(np.uint32)[0]

    def nothing_asked(out, seed, levels, what):
        """an utterance's ten outputs of a run that asked for nothing: the plain call's bits, no table, the identity row"""
        assert np.array_equal(CH.bits(out[0]), CH.bits(plain[seed])), what
        assert all(t.shape == (0,) for t in out[4:]) and out[2].shape == (0,), what
        assert (out[3].shape == (3,) and out[3][2] == one) if levels else out[3].shape == (0,), (what, out[3])

    a.set_graph_mode(True)
    for capacity in (16, 1):
        a.set_graph_cache(capacity)
        for levels in (True, None):
            for run, entry in enumerate((NOTHING, EVERYTHING, MIXED, NOTHING, EVERYTHING, MIXED, NOTHING)):
                what = ("capacity", capacity, "levels", levels, "run", run, CH.MENU[entry])
                utts = tuple((N, T, s, entry) for s in range(3))
                alone = ref(("synth", N, T, 0, entry, False, levels), lambda m, c: CH.run_synth(m, c, N, T, 0, entry, False, levels))
                batch = ref(("batch", utts, levels), lambda m, c: CH.run_batch_sync(m, c, False, utts, levels))
                for lane in (0, 1):
                    a.poison(0x3C if run % 2 else 0xFF, lane)
                got = CH.run_synth(a, ctx, N, T, 0, entry, False, levels)
                CH.same(got, alone, what + ("alone",))
                if entry == NOTHING:
                    nothing_asked(got, 0, levels, what + ("alone",))
                for lane in (0, 1):
                    bc, rows = CH.prepare(a, ctx, False, utts, levels)
                    bc.begin(lane)
                    bc.end(lane)
                    got = CH._snapshot(bc, rows)
                    CH.same(got, batch, what + ("lane", lane))
                    if entry == NOTHING:
                        for s in range(3):
                            nothing_asked(got[10 * s:10 * s + 10], s, levels, what + ("lane", lane, s))
    a.set_graph_mode(False)
    stats = a.graph_cache_stats().as_dict()
    _invariants(stats)
    assert stats["hits"] > 0 and stats["captures"] > 0 and stats["full_drops"] == 0, stats
    done()


# ---- directed: analysis calls between replays -------------------------------------------------------------------------------------------

def test_analysis_calls_between_replays(env):
    fresh, ref, done = env
    a, ctx = fresh()
    synth_key = ("synth", 5, 7, 0, EVERYTHING, False)
    batch_key = ("batch", "lane", 0, False, ((5, 7, 0, EVERYTHING), (24, 33, 1, MIXED), (5, 33, 2, NOTHING)))
    a.set_graph_mode(True)
    for what in ("capture", "again", "replay"):      # (the batch's first run grows lane 0's blocks, which drops the synth graph once)
        _check(a, ctx, ref, synth_key, what)
        _check(a, ctx, ref, batch_key, what)
    s0 = a.graph_cache_stats().as_dict()
    assert s0["captures"] >= 2 and s0["hits"] >= 2 and s0["full_drops"] == 0, s0
    io0 = a.poison(0xFF, 0)[1]
    # four waveforms of 250 frames: the call's layout (waveforms, rows, slabs) is far larger than anything lane 0 has held
    _check(a, ctx, ref, ("mel_wave_batch", ((250, 0), (250, 1), (250, 2), (250, 0)), False), "mel_wave_batch")
    io1 = a.poison(0x3C, 0)[1]
    assert io1 > io0 >= 1 and io1 >= 4 * 250 * (CH.HOP + CH.NUM_MELS) * 4, (io0, io1)      # lane 0's I/O block has been freed and regrown
    for key in (("filter_wave", 33, 0, 33), ("band_levels", 33, 1, True), ("pitch_track", 33, 2, False), ("mel_wave", 33, 0, True)):
        _check(a, ctx, ref, key, "analysis")
    for what in ("after the regrow", "once more"):
        _check(a, ctx, ref, synth_key, what)
        _check(a, ctx, ref, batch_key, what)
    a.set_graph_mode(False)
    s1 = a.graph_cache_stats().as_dict()
    _invariants(s1)
    assert s1["full_drops"] == 0 and s1["lane_drops"] >= s0["lane_drops"] and s1["hits"] > s0["hits"], (s0, s1)
    done()


# ---- directed: lane 0 beside a batch in flight -------------------------------------------------------------------------------------------

LANE0_CALLS = (("filter_wave", 33, 0, 33), ("band_levels", 33, 1, True), ("pitch_track", 33, 2, False), ("mel_wave", 33, 0, True),
               ("vocode_batch", ((7, 0), (33, 1))), ("vocode_device", 33, 2))


def test_lane0_calls_beside_a_batch_in_flight(env):
    from zerovox_cpp_amd import capi
    fresh, ref, done = env
    a, ctx = fresh()
    utts = ((5, 7, 0, EVERYTHING), (24, 33, 1, MIXED), (40, 64, 2, NOTHING))
    batch = ref(("batch", "sync", 0, False, utts))
    mels = ((33, 0), (7, 1), (64, 2))
    wavs = ref(("vocode_batch", mels))
    for graph in (False, True):
        a.set_graph_mode(graph)
        # a synthesize batch in flight on lane 1, then a vocode batch
        bc, rows = CH.prepare(a, ctx, False, utts)
        a.poison(0xFF, 1)
        bc.begin(1)
        for key in LANE0_CALLS:
            _check(a, ctx, ref, key, ("beside a synthesize batch on lane 1", graph))
        bc.end(1)
        CH.same(CH._snapshot(bc, rows), batch, ("the synthesize batch on lane 1", graph))
        a.poison(0x3C, 1)
        a.vocode_batch_begin(1, CH._mels(ctx, mels))
        for key in LANE0_CALLS:
            _check(a, ctx, ref, key, ("beside a vocode batch on lane 1", graph))
        CH.same(a.vocode_batch_end(1), wavs, ("the vocode batch on lane 1", graph))
        # a batch in flight on lane 0: every one of the calls is refused in the same words, and the batch is left alone
        bc, rows = CH.prepare(a, ctx, False, utts)
        a.poison(0xFF, 0)
        bc.begin(0)
        for key in LANE0_CALLS:
            with pytest.raises(capi.ZvError, match="lane 0 has a batch in flight") as e:
                CH.run_parts(a, key, ctx)
            assert e.value.status == ERR_ARG, (key, str(e.value))
        bc.end(0)
        CH.same(CH._snapshot(bc, rows), batch, ("the batch on lane 0 after the refusals", graph))
        for key in LANE0_CALLS:
            _check(a, ctx, ref, key, ("after the refusal", graph))
    a.set_graph_mode(False)
    _invariants(a.graph_cache_stats().as_dict())
    done()
