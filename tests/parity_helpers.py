"""shared parity gates of the GPU tests (no test in here)"""
import numpy as np


def encoder_decisions_vs_reference(e, z, nb, T):
    """Integer decisions of the encoder against a reference fixture, gated on the reference semantics' OWN re-association noise
    (tests/golden/make_golden.py add_encoder_margins: our oracle in sequential-f32 order against the reference, stored per
    fixture) — no hand-written tolerance:
      * float predictions within 2 x their floor (energy away from pitch flips: the energy predictor reads x + pitch embedding
        through two k = 3 convs, reference src/fs2encoder.cpp:569-572);
      * every flipped decision moved by ONE step and sat, in the reference, no further from its rounding boundary than 2 x the
        floor of the value it rounds (a flip elsewhere is an error, not noise); an energy flip may instead sit within two rows of
        a pitch flip;
      * no more flips than 2 x the floor's own count + 2."""
    N = len(z["logdur"])
    f_ld, f_p, f_e = float(z["floor_logdur_max"]), float(z["floor_pitch_max"]), float(z["floor_energy_max"])
    ld_err = float(np.max(np.abs(e["logdur"] - z["logdur"])))
    p_err = float(np.max(np.abs(e["pitch"] - z["pitch"])))
    dur_x = np.exp(z["logdur"].astype(np.float64)) - 1 + 0.5                     # the reference's value before (int)
    dur_g = (np.exp(e["logdur"].astype(np.float64)) - 1 + 0.5).astype(np.int64)
    dur_r = dur_x.astype(np.int64)
    dflip = dur_g != dur_r
    pflip = e["pitch_bucket"] != z["pitch_bucket"]
    eflip = e["energy_bucket"] != z["energy_bucket"]
    near = np.convolve(pflip.astype(np.int32), np.ones(5, np.int32), mode="same") > 0
    e_err = float(np.max(np.abs(e["energy"][~near] - z["energy"][~near]))) if (~near).any() else 0.0
    print(f"   N={N}: logdur err {ld_err:.2e} (floor {f_ld:.2e}), pitch err {p_err:.2e} ({f_p:.2e}), energy err away from pitch flips "
          f"{e_err:.2e} ({f_e:.2e}); flips dur {int(dflip.sum())} (floor {int(z['floor_dur_flips'])}) pitch {int(pflip.sum())} "
          f"({int(z['floor_pitch_flips'])}) energy {int(eflip.sum())} ({int(z['floor_energy_flips'])}); frames {e['n_frames']} vs {int(z['n_frames'])}")
    assert ld_err <= 2.0 * f_ld + 1e-5 and p_err <= 2.0 * f_p + 1e-5 and e_err <= 2.0 * f_e + 1e-5
    # distance of the reference's pre-rounding value from the boundary a flip crossed
    dist = lambda x: np.abs(x - np.round(x))
    d_dur = dist(dur_x)                                    # frames; d(dur)/d(logdur) = exp(logdur)
    band_dur = 2.0 * f_ld * np.exp(z["logdur"].astype(np.float64)) + 1e-6
    assert np.all(np.abs(dur_g - dur_r) <= 1) and np.all(d_dur[dflip] <= band_dur[dflip]), "a duration flipped away from a rounding boundary"
    xp = z["pitch"].astype(np.float64) * nb + 0.5
    assert np.all(np.abs(e["pitch_bucket"].astype(np.int64) - z["pitch_bucket"])[pflip] <= 1)
    assert np.all(dist(xp)[pflip] <= 2.0 * f_p * nb + 1e-6), "a pitch bucket flipped away from a boundary"
    xe = z["energy"].astype(np.float64) * nb + 0.5
    tie = dist(xe) <= 2.0 * f_e * nb + 1e-6
    assert np.all(tie[eflip] | near[eflip]), "an energy bucket flipped away from a boundary and away from any pitch flip"
    assert int(dflip.sum()) <= 2 * int(z["floor_dur_flips"]) + 2
    assert int(pflip.sum()) <= 2 * int(z["floor_pitch_flips"]) + 2
    assert int(eflip.sum()) <= 2 * int(z["floor_energy_flips"]) + 2
    assert min(e["n_frames"], int(z["n_frames"])) == T or abs(e["n_frames"] - int(z["n_frames"])) <= int(dflip.sum())
    return int(dflip.sum()), int(pflip.sum()), int(eflip.sum())


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def layer_gate(name, got, ref, alt, rel_gate, floor_mult=2.0):
    """got: GPU, ref: oracle (ggml AVX2 order), alt: oracle (sequential f32).  rel = rms(err) / rms(signal)."""
    sig = _rms(ref)
    err, floor = _rms(got - ref) / sig, _rms(alt - ref) / sig
    mx = float(np.max(np.abs(got - ref))) / sig
    print(f"{name:28s} rel rms err {err:.2e} (oracle self-noise {floor:.2e}), max {mx:.2e}, signal rms {sig:.3f}")
    assert np.isfinite(got).all()
    assert err <= max(floor_mult * floor, 3e-7), name          # no worse than the reference's own re-association noise
    assert err <= rel_gate, name


def oracle_pair(o, fn, *args, **kw):
    """fn(*args, **kw) of the oracle o in the reference's summation order (ggml AVX2) and in sequential f32 order"""
    from oracle import zvoracle
    o.set_order(zvoracle.ORDER_GGML_AVX2)
    ref = getattr(o, fn)(*args, **kw)
    o.set_order(zvoracle.ORDER_SEQ_F32)
    alt = getattr(o, fn)(*args, **kw)
    o.set_order(zvoracle.ORDER_GGML_AVX2)
    return ref, alt


# the kernels only batches pick by themselves, forced on for one utterance (some are sampled when a model is built: build it
# inside capi.switches(**BATCH_REGIME))
BATCH_REGIME = dict(ZV_BLOCK64=-11, ZV_CONV_STREAM=2, ZV_CONV_GEMM=2, ZV_UP_GEMM=2, ZV_PAIR64_RING=2, ZV_TRIPLE_V2=3, ZV_FUSE256=1,
                    ZV_PAIR_MT=0, ZV_DEC_PREPASS=1)

# every kernel regime of the vocoder (tests/test_gpu_full_size.py::test_kernel_regimes_give_the_same_bits): each sums every
# output element in the same order, so none may change a bit
VOCODER_REGIMES = (
    ("default", {}), ("fuse256", {"ZV_FUSE256": 1}), ("no_triple", {"ZV_NO_TRIPLE": 1}), ("no_fuse", {"ZV_NO_FUSE": 1}),
    ("no_merge", {"ZV_NO_MERGE": 1}), ("fuse256_no_merge", {"ZV_FUSE256": 1, "ZV_NO_MERGE": 1}),
    ("merge", {"ZV_MERGE_ALWAYS": 1}), ("fuse256_merge", {"ZV_FUSE256": 1, "ZV_MERGE_ALWAYS": 1}),
    ("merge_in_one_workgroup", {"ZV_MERGE_ALWAYS": 1, "ZV_MERGE_SEQ": 0}),
    ("fuse256_merge_in_one_workgroup", {"ZV_FUSE256": 1, "ZV_MERGE_ALWAYS": 1, "ZV_MERGE_SEQ": 0}),
    ("fuse256_merge_mt3", {"ZV_FUSE256": 1, "ZV_MERGE_ALWAYS": 1, "ZV_PAIR_MT": 3}),
    ("pair64_ring_merge", {"ZV_PAIR64_RING": 2, "ZV_MERGE_ALWAYS": 1}),
    ("single_loop_everywhere", {"ZV_CONV_SINGLE": 2}), ("no_single_loop", {"ZV_CONV_SINGLE": 0}),
    ("block_v1", {"ZV_TRIPLE_V2": 0}), ("block_v2", {"ZV_TRIPLE_V2": 2}),
    ("block_v2_512", {"ZV_TRIPLE_V2": 3}), ("block_v2_512_one_weight_buffer", {"ZV_TRIPLE_V2": 3, "ZV_TRIPLE_DB": 0}),
    ("block_v2_not_interleaved", {"ZV_TRIPLE_V2": 2, "ZV_TRIPLE_INTERLEAVE": 0}),
    ("pair64_ring", {"ZV_PAIR64_RING": 2}), ("pair64_ring_no_merge", {"ZV_PAIR64_RING": 2, "ZV_NO_MERGE": 1}),
    ("pair64_no_ring", {"ZV_PAIR64_RING": 0}),
    ("upsample_gemm", {"ZV_UP_GEMM": 2, "ZV_CONV_GEMM": 2}), ("upsample_no_gemm", {"ZV_UP_GEMM": 0}),
    ("block64_3_merge", {"ZV_BLOCK64": -3, "ZV_PAIR64_RING": 2, "ZV_MERGE_ALWAYS": 1}),
    ("block64_3_no_merge", {"ZV_BLOCK64": -3, "ZV_PAIR64_RING": 2}), ("block64_11", {"ZV_BLOCK64": -11, "ZV_PAIR64_RING": 2}),
    ("no_block64", {"ZV_BLOCK64": 0, "ZV_PAIR64_RING": 2}),
    ("upsample_stream", {"ZV_CONV_STREAM": 2}), ("upsample_no_stream", {"ZV_CONV_STREAM": 0}),
    # the fused batch kernels run on v_mfma_f32_16x16x32_f16, the generic conv kernel ("no_fuse") and the single-utterance
    # whole-block kernel on 32x32x16: one k-ordered chain, two instruction shapes, the same bits
    ("pair_mt4", {"ZV_PAIR_MT": 4, "ZV_FUSE256": 1}),
    ("pair_no_ring_no_triple", {"ZV_PAIR64_RING": 0, "ZV_NO_TRIPLE": 1, "ZV_MERGE_ALWAYS": 1}),
    # the single-utterance conv form (loader waves, two LDS tiles) with its channel groups dealt / not dealt over the XCDs
    ("single_loop_everywhere_plain_grid", {"ZV_CONV_SINGLE": 2, "ZV_CONV_XCD": 0}), ("plain_grid", {"ZV_CONV_XCD": 0}),
)
