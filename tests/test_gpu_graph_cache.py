"""-m gpu: the captured-graph cache under changing batch shapes (include/zerovox_amd.h zv_set_graph_cache / zv_graph_cache_stats,
csrc/graph_cache.h): a repeated shape costs no capture, a full cache gives up one graph, the least recently used, graphs of an
older switch epoch first, lanes evict each other's graphs while both have work queued, a lane that regrows its blocks loses its own
graphs alone, and a smaller capacity keeps the most recent.  Graph mode is on throughout, and every waveform is compared bit for
bit with the same call made once with graph mode off.

A shape is (utterances, phoneme class, frame class): the batch's key rounds the longest phoneme count up to 32 and the longest
frame capacity up to 64, so 1-3 utterances x {32, 64} phonemes x {64, 128, 192, 256} frames are 24 distinct keys on the small
checkpoint, the largest (3, 64, 256).  A lane's blocks only grow, and every one of them grows with each of the three numbers, so a
lane that has run the largest shape once regrows nothing afterwards."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LARGEST = (3, 64, 256)
SHAPES = [(s, n, t) for t in (64, 128, 192, 256) for n in (32, 64) for s in (1, 2, 3)]      # 24, the largest last
_REF = {}


def _utterances(g, shape):
    from zerovox_cpp_amd import synth
    nseg, ncls, tcls = shape
    seed = 4000 + 100 * nseg + ncls + 7 * tcls
    # the first utterance reaches into the class's top 32 phonemes / 64 frames, the others are shorter and ragged
    return [(*synth.encoder_inputs(g, seed + u, ncls - 3 - 9 * u), tcls - 5 - 21 * u) for u in range(nseg)]


@pytest.fixture(scope="module")
def small(ckpt):
    """(path, geometry, ref): ref(shape) = the shape's waveforms and frame counts with graph mode off, computed once per shape"""
    from zerovox_cpp_amd import capi
    path, g, _ = ckpt("small")
    eager = capi.Model(path, 0)

    def ref(shape):
        if shape not in _REF:
            _REF[shape] = [(w.copy(), nf) for w, nf in eager.synthesize_batch(_utterances(g, shape))]
        return _REF[shape]
    yield path, g, ref
    eager.close()
    _REF.clear()


@pytest.fixture
def model(small):
    """a fresh model per test: its counters start at zero and no earlier test has captured anything"""
    from zerovox_cpp_amd import capi
    m = capi.Model(small[0], 0)
    yield m
    m.close()


def _grow(model, g, lanes=(0,)):
    """runs the largest shape once per lane with graph mode off: no block of these lanes regrows afterwards"""
    model.set_graph_mode(False)
    for lane in lanes:
        c = model.prepare_batch(_utterances(g, LARGEST))
        c.begin(lane)
        c.end(lane)
    model.set_graph_mode(True)


def _run(model, small, shape, lane=0):
    """the shape through begin / end on `lane`, compared with its eager twin; the stats before and after"""
    _, g, ref = small
    before = model.graph_cache_stats().as_dict()
    c = model.prepare_batch(_utterances(g, shape))
    c.begin(lane)
    c.end(lane)
    _same(c, ref(shape), shape)
    return before, model.graph_cache_stats().as_dict()


def _same(call, want, what):
    for (w, nf), (rw, rnf) in zip(call.results(), want):
        assert nf == rnf and np.array_equal(w, rw), what


def _invariants(s):
    assert s["lookups"] == s["hits"] + s["captures"], s
    assert s["captures"] == s["entries"] + s["evictions"] + s["stale_evictions"] + s["lane_drops"] + s["full_drops"], s
    assert s["entries"] <= s["capacity"] and s["retired"] <= s["capacity"], s


def _delta(pair, name):
    return pair[1][name] - pair[0][name]


def test_a_repeated_shape_costs_no_capture(model, small):
    model.set_graph_mode(True)
    s0 = model.graph_cache_stats().as_dict()
    assert s0["capacity"] == 16 and all(v == 0 for k, v in s0.items() if k != "capacity"), s0
    first = _run(model, small, (2, 32, 128))
    c = _delta(first, "captures")
    assert c >= 1 and _delta(first, "hits") == 0 and _delta(first, "entries") == c, first
    again = _run(model, small, (2, 32, 128))
    assert _delta(again, "captures") == 0 and _delta(again, "hits") == c and _delta(again, "entries") == 0, again
    _invariants(again[1])
    # graph mode off goes past the cache: no lookup
    model.set_graph_mode(False)
    eager = _run(model, small, (2, 32, 128))
    assert eager[0] == eager[1]


def test_a_full_cache_gives_up_one_graph_the_least_recently_used(model, small):
    """capacity 8, 20 distinct shapes: never more than 8 held, nothing dropped wholesale; the newest shapes that fit in 8 are all still
    held, the very first is not.  (Without the stats call there is nothing to read; counters alone on the earlier cache, which
    dropped all sixteen graphs when the seventeenth arrived, would fail the re-runs.)"""
    _grow(model, small[1])
    model.set_graph_cache(8)
    shapes = SHAPES[:20]
    cost = []
    for sh in shapes:
        pair = _run(model, small, sh)
        cost.append(_delta(pair, "captures"))
        assert cost[-1] >= 1 and _delta(pair, "hits") == 0, (sh, pair)
        assert pair[1]["entries"] <= 8 and pair[1]["full_drops"] == 0 and pair[1]["lane_drops"] == 0, (sh, pair)
        # one graph goes for each that comes once the cache is full, never more
        assert _delta(pair, "evictions") == max(0, pair[0]["entries"] + cost[-1] - 8) and pair[1]["stale_evictions"] == 0, (sh, pair)
    _invariants(model.graph_cache_stats().as_dict())
    held, room = [], 8
    for i in reversed(range(len(shapes))):
        if cost[i] > room:
            break
        room -= cost[i]
        held.append(i)
    assert len(held) >= 2
    for i in held:                                    # newest first
        pair = _run(model, small, shapes[i])
        assert _delta(pair, "captures") == 0 and _delta(pair, "hits") == cost[i], (shapes[i], pair)
    pair = _run(model, small, shapes[0])
    assert _delta(pair, "captures") == cost[0], pair
    _invariants(pair[1])


def test_two_lanes_evict_each_others_graphs_with_work_queued(model, small):
    """capacity 4, different shapes alternating on lanes 0 and 1 with two batches in flight: every capture past the fourth retires a
    graph, often the other lane's, while that lane has a batch queued.  Every waveform equals its eager twin; after zv_synchronize
    one more capture finds every retired graph finished."""
    _, g, ref = small
    _grow(model, g, lanes=(0, 1))
    model.set_graph_cache(4)
    shapes = SHAPES[:16]
    calls = [model.prepare_batch(_utterances(g, sh)) for sh in shapes]
    for k, c in enumerate(calls):
        c.begin(k % 2)                                # the other lane's batch k - 1 is still in flight
        if k >= 1:
            calls[k - 1].end((k - 1) % 2)
            _same(calls[k - 1], ref(shapes[k - 1]), shapes[k - 1])
        s = model.graph_cache_stats().as_dict()
        assert s["entries"] <= 4 and s["retired"] <= 4 and s["full_drops"] == 0 and s["lane_drops"] == 0, (k, s)
    calls[-1].end((len(calls) - 1) % 2)
    _same(calls[-1], ref(shapes[-1]), shapes[-1])
    # once more, now every one a miss again but for the last four: the graphs were evicted while in use and captured anew
    for k, c in enumerate(calls[:6]):
        c.begin(k % 2)
        if k >= 1:
            calls[k - 1].end((k - 1) % 2)
            _same(calls[k - 1], ref(shapes[k - 1]), shapes[k - 1])
    calls[5].end(1)
    _same(calls[5], ref(shapes[5]), shapes[5])
    s = model.graph_cache_stats().as_dict()
    _invariants(s)
    assert s["evictions"] >= len(shapes) + 6 - 4 and s["stale_evictions"] == 0, s
    model.synchronize()
    pair = _run(model, small, SHAPES[20])
    assert _delta(pair, "captures") >= 1 and pair[1]["retired"] == 0, pair
    _invariants(pair[1])


def test_graphs_of_an_older_switch_epoch_go_first(model, small):
    from zerovox_cpp_amd import capi
    _grow(model, small[1])
    model.set_graph_cache(4)
    k = 0
    while model.graph_cache_stats().entries < 4:
        _run(model, small, SHAPES[k])
        k += 1
    filled = model.graph_cache_stats().as_dict()
    assert filled["entries"] == 4 and filled["evictions"] == 0, filled
    with capi.switches(ZV_PAIR_MT=4):                 # set and set back: the same switches, a later epoch
        pass
    stale_left = 4
    for sh in SHAPES[k:k + 7]:
        pair = _run(model, small, sh)
        c = _delta(pair, "captures")
        assert c >= 1 and pair[1]["entries"] <= 4, (sh, pair)
        went_stale = min(c, stale_left)
        assert _delta(pair, "stale_evictions") == went_stale and _delta(pair, "evictions") == c - went_stale, (sh, stale_left, pair)
        stale_left -= went_stale
    final = model.graph_cache_stats().as_dict()
    assert stale_left == 0 and final["stale_evictions"] == 4 and final["evictions"] >= 1, final
    _invariants(final)


def test_a_lanes_regrow_spares_the_other_lanes_graphs(model, small):
    model.set_graph_mode(True)
    on0 = _run(model, small, (1, 32, 64), lane=0)
    c0 = _delta(on0, "captures")
    on1 = _run(model, small, (1, 32, 128), lane=1)
    c1 = _delta(on1, "captures")
    assert c0 >= 1 and c1 >= 1 and on1[1]["lane_drops"] == 0 and on1[1]["entries"] == c0 + c1, (on0, on1)
    grown = _run(model, small, LARGEST, lane=1)       # lane 1's arena and blocks grow: its graphs name the old ones
    assert _delta(grown, "lane_drops") == c1 and grown[1]["full_drops"] == 0, grown
    assert grown[1]["entries"] == c0 + _delta(grown, "captures"), grown
    still = _run(model, small, (1, 32, 64), lane=0)
    assert _delta(still, "captures") == 0 and _delta(still, "hits") == c0, still
    _invariants(still[1])


def test_a_smaller_capacity_keeps_the_most_recently_used(model, small):
    from zerovox_cpp_amd import capi
    _grow(model, small[1])
    model.set_graph_cache(8)
    shapes = SHAPES[:5]
    cost = [_delta(_run(model, small, sh), "captures") for sh in shapes]
    _run(model, small, shapes[1])                     # a hit: shape 1 is now the most recent, ahead of shape 4
    order = [0, 2, 3, 4, 1]                           # least to most recently used
    assert sum(cost) <= 8
    model.set_graph_cache(2)
    s = model.graph_cache_stats().as_dict()
    assert s["capacity"] == 2 and s["entries"] == 2 and s["evictions"] == sum(cost) - 2, s
    _invariants(s)
    for status_of in (0, 1025):
        with pytest.raises(capi.ZvError) as e:
            model.set_graph_cache(status_of)
        assert e.value.status == 5 and "graph cache capacity" in str(e.value)
        assert model.graph_cache_stats().as_dict() == s
    kept, room = [], 2
    for i in reversed(order):
        if cost[i] > room:
            break
        room -= cost[i]
        kept.append(i)
    assert kept and kept[0] == 1
    for i in kept:
        pair = _run(model, small, shapes[i])
        assert _delta(pair, "captures") == 0 and _delta(pair, "hits") == cost[i], (shapes[i], pair)
    gone = order[len(order) - len(kept) - 1]
    pair = _run(model, small, shapes[gone])
    assert _delta(pair, "captures") == cost[gone], pair
    _invariants(pair[1])
