"""No GPU: the call history of tests/test_gpu_call_history.py holds what that test is there to cross.  These are conditions on the
test's INPUT (tests/call_history.py history(), for the default seed and the step count the GPU test walks), not measurements: a
history that misses one tests less than it claims, and the remedy is the generator's probabilities or more steps, never a lower
minimum."""
import os

import call_history as CH

SEED = int(os.environ.get("ZV_SM_SEED", "2024"))
STEPS = CH.STEPS                                    # the step count of test_every_entry_point_in_one_history


def _history():
    return CH.history(SEED, STEPS)


def test_the_history_is_a_pure_function_of_seed_and_steps():
    a, b = CH.history(SEED, STEPS), CH.history(SEED, STEPS)
    assert a == b and len(a) == STEPS
    assert CH.history(SEED + 1, STEPS) != a
    for s in a:
        hash(s)                                    # every step is hashable: a call key files its outputs


def test_the_history_holds_only_legal_calls():
    for seed in (SEED, 7):
        steps = CH.history(seed, STEPS)
        assert CH.legal(steps) is None, CH.legal(steps)
        for s in steps:
            if s[0] == "poison":
                assert s[2] in (0, 1) and 0 <= s[1] <= 255
            elif s[0] == "cache":
                assert s[1] in CH.CACHES
            elif s[0] == "reserve":
                assert s[1:] in CH.RESERVES
            elif s[0] not in CH.STATE_OPS:
                assert all(CH.op_of(k) in CH.OPS for k in CH.calls_of(s)), s
                # the call beside a vocode batch on lane 1 is a synchronous lane-0 call
                if s[0] == "vocode_batch_lane":
                    assert all(not (k[0] in ("pair", "vocode_batch_lane") or (k[0] == "batch" and k[1] == "lane")) for k in CH.calls_of(s)[1:]), s


def test_the_default_history_meets_every_condition():
    c = CH.coverage(_history())
    print(c)
    assert len(CH.MENU) >= 8
    for op, n in c["ops"].items():
        assert n >= 5, (op, n)
    for e, name in enumerate(CH.MENU):
        assert c["synth_entries"][e] >= 5, ("synth", name, c["synth_entries"][e])
        assert c["batch_entries"][e] >= 5, ("batch", name, c["batch_entries"][e])
        assert c["fitted_entries"][e] >= 1, ("fitted", name)
    assert c["successions"] >= 15 and c["successions_lane1"] >= 5, (c["successions"], c["successions_lane1"])
    assert c["repeats"] >= 8, c["repeats"]
    assert c["sandwiches"] >= 8, c["sandwiches"]
    for cap, n in c["cache_steps"].items():
        assert n >= 20, (cap, n)
    assert c["pairs"] >= 5, c["pairs"]
    assert c["growing_reserves"] >= 3, c["growing_reserves"]
    assert c["poisons"] >= 10, c["poisons"]


def test_the_counts_see_what_they_are_meant_to_see():
    """coverage() on a history written out by hand: one of each thing it counts"""
    u, v = ((5, 7, 0, 0),), ((5, 7, 0, 1),)
    steps = [("graph", True), ("reserve", 5, 7), ("synth", 5, 7, 0, 0, False), ("synth", 5, 7, 0, 1, False), ("synth", 5, 7, 0, 1, False),
             ("mel_wave", 7, 0, False), ("synth", 5, 7, 0, 1, False), ("reserve", 5, 7), ("reserve", 256, 512), ("cache", 2),
             ("batch", "lane", 1, False, u), ("batch", "lane", 1, False, v), ("pair", (1, 0), False, u, True, v), ("poison", 255, 1),
             ("graph", False), ("synth", 5, 7, 0, 0, True), ("synth", 5, 7, 0, 2, True), ("synth", 5, 7, 0, 2, True),
             ("vocode_batch_lane", ((7, 0),), ("vocode", 7, 1))]
    c = CH.coverage(steps)
    assert c["successions"] == 2 and c["successions_lane1"] == 1 and c["repeats"] == 1 and c["sandwiches"] == 1
    assert c["cache_steps"] == {1: 0, 2: 7, 16: 5} and c["pairs"] == 1 and c["poisons"] == 1
    assert c["reserves"] == 3 and c["growing_reserves"] == 2
    assert c["ops"]["synth"] == 7 and c["ops"]["batch_lane"] == 2 and c["ops"]["vocode_batch_lane"] == 1 and c["ops"]["vocode"] == 1
    assert c["synth_entries"][:3] == [2, 3, 2] and c["batch_entries"][:2] == [2, 2] and c["fitted_entries"][:3] == [1, 1, 2]
    assert CH.repeats(steps) == [4]
    # a pair is compared with its two batches, a lane batch with its synthesize_batch
    assert CH.parts(steps[12]) == [("batch", "sync", 0, False, u), ("batch", "sync", 0, True, v)]
    assert CH.parts(steps[10]) == [("batch", "sync", 0, False, u)]
    assert CH.parts(steps[-1]) == [("vocode_batch", ((7, 0),)), ("vocode", 7, 1)]


def test_same_sees_every_kind_of_difference():
    """same() compares bits, not values: a NaN equals itself, -0.0 differs from 0.0, and a table where the reference has none (or none
    where it has one), another shape or another dtype is a difference; the message names the key, the output and the first element"""
    import numpy as np
    import pytest
    f = lambda *v: np.array(v, np.float32)
    ok = [f(1.0, np.nan, -0.0), np.array([3], np.uint32), CH.ABSENT, np.zeros((2, 2), np.float32), np.array([1, -1], np.int32)]
    CH.same([x.copy() for x in ok], ok, "key")
    for i, other in ((0, f(1.0, np.nan, 0.0)), (0, f(1.0, np.nan)), (1, np.array([3], np.int32)), (2, np.zeros((1, 2), np.float32)),
                     (3, CH.ABSENT), (3, np.zeros(4, np.float32)), (4, np.array([1, -2], np.int32))):
        got = [x.copy() for x in ok]
        got[i] = other
        with pytest.raises(AssertionError) as e:
            CH.same(got, ok, "the key")
        assert "the key" in str(e.value) and f"'output', {i}" in str(e.value), str(e.value)
    with pytest.raises(AssertionError, match="'element', 2"):
        CH.same([f(1.0, np.nan, 0.0)], [f(1.0, np.nan, -0.0)], "k")
    with pytest.raises(AssertionError, match="outputs"):
        CH.same(ok[:4], ok, "k")
