"""The limiter (include/zerovox_amd.h "limiter") without a device.
 * tests/native/limiter_check.cpp `self` holds csrc/limiter.h's limit_reference against a restatement with every window loop written
   out, on random and adversarial inputs, and the same program runs once more built with -fsanitize=address,undefined (a plain host
   program, nothing preloaded);
 * the numpy restatement (tests/limiter_rule.py) against that reference, bit for bit: every field of the result, every sample of the
   output and every s_n, on every shape of tests/limiter_shapes.py and on the ragged batch's utterances;
 * on every shape: its own reach assertion, s_n <= q_n everywhere and the promise (limiter_shapes.check);
 * true_peak_before and sample_peak_before equal to loudness_rule's of the same span; the restatement's block minima and cumulative
   sums against windows written out;
 * the identity: gain 1 and a ceiling above the true peak give out == wav bit for bit on finite samples and limited_samples == 0;
 * limit_design, limit_check, limit_plan and the group cut;
 * how far true_peak_after passes the ceiling: the table of profiles/limiter_accuracy.txt recomputed, its default-window column asserted
   as a regression guard."""
import os
import subprocess

import numpy as np
import pytest

import limiter_rule as LM
import limiter_shapes as LH
import loudness_rule as LR
import loudness_shapes as LS

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
SR, HOP = LH.SR, LH.HOP


def fb(v):
    return "%x" % LR.fbits(v)


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "limiter_check.cpp"), "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("limiter_check")
    return _build(tmp, "limiter_check", []), _build(tmp, "limiter_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def D(exes):
    """the interpolator the native reference uses, as data"""
    t = subprocess.run([exes[0], "taps", str(SR)], capture_output=True, text=True, timeout=60).stdout.split()
    assert len(t) == 49
    return type("Design", (), {"c": np.array([int(v, 16) for v in t], np.uint32).view(F)})


def native(exe, tmp, x, N, q):
    src, dst, sdst = (str(tmp / n) for n in ("in.f32", "out.f32", "s.u32"))
    np.asarray(x, F).tofile(src)
    r = subprocess.run([exe, "run", str(SR), str(N), str(x.size), fb(q.gain), fb(q.ceiling), str(q.attack), str(q.release), src, dst, sdst],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    t = r.stdout.split()
    key = (int(t[0], 16), int(t[1], 16), int(t[2])) + tuple(int(v, 16) for v in t[3:])
    return key, np.fromfile(dst, F), np.fromfile(sdst, np.uint32)


def _same_as_native(exe, tmp, D, what, x, N, q):
    res, out, I = LM.rule(D, x, N, q, SR)
    key, nout, ns = native(exe, tmp, x, N, I.ask)
    assert LM.key(res) == key, (what, res, key)
    bad = np.flatnonzero(out.view(np.uint32) != nout.view(np.uint32))
    assert bad.size == 0, (what, bad[:6])
    assert (ns[:I.span] == I.s).all() and (ns[I.span:] == LM.ONE).all(), what
    return res, out, I


def test_reference_against_written_out_windows(exes):
    for exe in exes:                                                            # the second one under the sanitizers
        r = subprocess.run([exe, "self"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.split() == ["ok", "40"], (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("name", sorted(LH.CASES))
def test_restatement_equals_the_reference_on_every_shape(exes, D, tmp_path, name):
    c = LH.CASES[name]()
    res, out, I = LH.check(D, c)
    got = _same_as_native(exes[0], tmp_path, D, name, c.x, c.N, c.ask)
    assert LM.key(got[0]) == LM.key(res)
    tp, sp = LR.true_peak(D, c.x, c.N)
    assert LR.dbits(tp) == LR.dbits(res.true_peak_before) and LR.fbits(sp) == LR.fbits(res.sample_peak_before)
    tpa, spa = LR.true_peak(D, out, c.N)
    assert LR.dbits(tpa) == LR.dbits(res.true_peak_after) and LR.fbits(spa) == LR.fbits(res.sample_peak_after)


def test_sanitized_reference_runs_a_shape(exes, D, tmp_path):
    c = LH.CASES["not_finite"]()
    a = native(exes[0], tmp_path, c.x, c.N, c.ask)
    b = native(exes[1], tmp_path, c.x, c.N, c.ask)
    assert a[0] == b[0] and (a[1].view(np.uint32) == b[1].view(np.uint32)).all() and (a[2] == b[2]).all()


def test_ragged_batch_utterances(exes, D, tmp_path):
    xs, nfs, asks = LH.ragged_batch()
    for u, (x, nf, q) in enumerate(zip(xs, nfs, asks)):
        _same_as_native(exes[0], tmp_path, D, u, x, nf * HOP, q)


def test_block_minima_and_cumulative_sums_equal_written_out_windows(D):
    rng = np.random.default_rng(5)
    for attack, release in ((1, 1), (2, 7), (9, 3), (33, 40)):
        x = (rng.standard_normal(400) * 0.3).astype(F)
        x[[0, 17, 18, 399]] = F(0.99)
        q = LM.ask(2.0, 0.3, attack, release)
        for N in (0, 5, 250, 400):
            p, _, _ = LM.peaks(D, x, N)
            _, _, s = LM.gains(q, p, N, 400)
            assert (s == LM.brute(q, p, N, 400)).all(), (attack, release, N)


def test_identity_leaves_the_waveform_alone(D):
    x = LH.speech(40, 10, 0.4)
    x[77] = np.nan
    tp = LR.true_peak(D, x, x.size)[0]
    assert tp < 0.9
    for q in (None, LM.ask(1.0, 0.9, 1, 1), LM.ask(1.0, 1.0, 2047, 6144)):
        res, out, I = LM.rule(D, x, x.size, q, SR)
        fin = np.isfinite(x)
        assert res.limited_samples == 0 and (out[fin].view(np.uint32) == x[fin].view(np.uint32)).all() and np.isnan(out[77])
        assert res.min_gain == F(1) and res.reduction_db == F(0)


def test_design_counts(exes):
    run = lambda rate, a, r: subprocess.run([exes[0], "design", str(rate), fb(a), fb(r)], capture_output=True, text=True, timeout=60).stdout.split()
    assert LM.design(22050) == (33, 1323) and LM.design(48000) == (72, 2880)
    for rate in (4000, 8000, 22050, 44100, 48000, 96000, 768000):
        for a, r in ((0.0, 0.0), (1.5, 60.0), (0.01, 0.01), (5.0, 200.0), (0.3, 17.7), (1000.0, 1000.0)):
            assert tuple(map(int, run(rate, a, r))) == LM.design(rate, a, r), (rate, a, r)
    assert LM.design(768000) == (1152, 6144) and LM.design(4000, 0.01, 0.01) == (1, 1)       # brought into [1, most]
    assert run(3999, 0.0, 0.0) == ["refused", "sampling_rate"] and run(768001, 0.0, 0.0) == ["refused", "sampling_rate"]
    assert run(22050, -1.0, 0.0) == ["refused", "attack_ms"] and run(22050, np.nan, 0.0) == ["refused", "attack_ms"]
    assert run(22050, 1.0, np.inf) == ["refused", "release_ms"] and run(22050, 1.0, -0.5) == ["refused", "release_ms"]


def test_argument_checker(exes):
    run = lambda g, c, a, r, f=0: subprocess.run([exes[0], "check", fb(g), fb(c), str(a), str(r), str(f)], capture_output=True, text=True,
                                                 timeout=60).stdout.strip()
    assert run(1.0, 1.0, 1, 1) == "ok" and run(0.0, 1e-30, 2047, 6144) == "ok" and run(1000.0, 0.5, 33, 1323) == "ok"
    for g in (-0.001, 1000.5, np.nan, np.inf):
        assert run(g, 0.5, 1, 1) == "gain"
    for c in (0.0, -0.5, 1.0000001, np.nan, np.inf):
        assert run(1.0, c, 1, 1) == "ceiling"
    assert run(1.0, 0.5, 0, 1) == "attack" and run(1.0, 0.5, 2048, 1) == "attack"
    assert run(1.0, 0.5, 1, 0) == "release" and run(1.0, 0.5, 1, 6145) == "release"
    assert run(1.0, 0.5, 1, 1, 1) == "flags"
    assert run(np.nan, np.nan, 0, 0, 9) == "gain"                               # in the order of the struct


def test_plan_and_group_cut(exes):
    plan = lambda nseg, halo, total, qlen: tuple(map(int, subprocess.run([exes[0], "plan", str(nseg), str(halo), str(total), str(qlen)],
                                                                        capture_output=True, text=True, timeout=60).stdout.split()))
    up = lambda n: -(-n // LH.TILE)
    for total in (1, 300, 2047, 2048, 2049, 6000, 9830400):
        for halo in (2, 1356, 8191):
            qlen = total + 2 * (halo + LH.PAD)
            stage = -(-(LH.TILE + halo) // 4) * 4
            assert plan(5, halo, total, qlen) == (1, up(qlen), up(total + halo), up(total), 5, stage, (stage + LH.TILE) * 4 + 64, (stage + 4) * 6 + 64)
    ok = lambda *a: plan(*a)[0]
    assert ok(1, 2, 1, 13) and not ok(0, 2, 1, 13) and not ok(65536, 2, 1, 13) and not ok(1, 1, 1, 13) and not ok(1, 8192, 1, 13)
    assert not ok(1, 2, 0, 12) and not ok(1, 2, 1, 12) and not ok(1, 2, 1, 14)
    big = plan(1, 8191, 9830400, 9830400 + 2 * 8195)
    assert 3 * big[6] <= 160 * 1024 and 2 * big[7] <= 160 * 1024 < 3 * big[7]   # workgroups of the minimum / mean pass a CU's LDS holds
    for hop, Ts in ((300, [32768] * 7 + [50, 50, 1]), (300, [1, 2, 3]), (256, [32768] * 20), (512, [32768] * 9)):
        r = subprocess.run([exes[0], "groups", str(hop)] + [str(t) for t in Ts], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and list(map(int, r.stdout.split())) == LS.group_ends(Ts, hop), (hop, r.stdout)


# ---- how far true_peak_after passes the ceiling -------------------------------------------------------------------------------------------------

OVERSHOOT_DRIVES = (6.0, 12.0, 20.0)
OVERSHOOT_SEEDS = (400, 401, 402, 403)
# the largest true_peak_after / ceiling measured at the default windows over those drives and seeds (profiles/limiter_accuracy.txt)
OVERSHOOT_DEFAULT_MEASURED = 1.135e-05


def overshoot_table(D):
    """{(window, drive dB): the largest true_peak_after / ceiling - 1 over the seeds}: speech-like signals of the loudness tests, 40
    frames, driven `drive` dB over a ceiling of -1 dBTP relative to their own true peak"""
    ceiling = F(10.0 ** (-1.0 / 20.0))
    table = {}
    for name, (a, r) in (("default", LM.design(SR)), ("W = 3", (1, 1))):
        for drive in OVERSHOOT_DRIVES:
            worst = 0.0
            for seed in OVERSHOOT_SEEDS:
                x = LS.speech(SR, seed, 40 * HOP, 0.3)
                tp = LR.true_peak(D, x, x.size)[0]
                gain = F(float(ceiling) / tp * 10.0 ** (drive / 20.0))
                res, out, _ = LM.rule(D, x, x.size, LM.ask(gain, ceiling, a, r), SR)
                assert res.limited_samples > 0
                worst = max(worst, res.true_peak_after / float(ceiling) - 1.0)
            table[(name, drive)] = worst
    return table


def test_true_peak_after_overshoot_is_guarded(D):
    table = overshoot_table(D)
    for k, v in sorted(table.items()):
        print("overshoot", k, "%.3e" % v)
    worst = max(v for (name, _), v in table.items() if name == "default")
    assert worst < 2.0 * OVERSHOOT_DEFAULT_MEASURED, (worst, OVERSHOOT_DEFAULT_MEASURED)      # W = 3 is recorded, not asserted
