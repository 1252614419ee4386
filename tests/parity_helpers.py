"""shared parity gates of the GPU tests (no test in here)"""
import numpy as np


def near_flips(flip):
    """tokens within two rows of a flipped pitch bucket (the energy predictor sees two k = 3 convs of x + pitch embedding).  Also
    for fewer than 5 tokens, where np.convolve(mode="same") returns the longer operand's length"""
    n = len(flip)
    return np.convolve(flip.astype(np.int32), np.ones(5, np.int32), mode="full")[2:2 + n] > 0


def encoder_decisions_vs_reference(e, z, nb, T, count_energy_near_pitch=True):
    """Integer decisions of the encoder against a reference fixture, gated on the reference semantics' OWN re-association noise
    (tests/golden/make_golden.py add_encoder_margins: our oracle in sequential-f32 order against the reference, stored per
    fixture) — no hand-written tolerance:
      * float predictions within 2 x their floor (energy away from pitch flips: the energy predictor reads x + pitch embedding
        through two k = 3 convs, reference src/fs2encoder.cpp:569-572);
      * every flipped decision moved by ONE step and sat, in the reference, no further from its rounding boundary than 2 x the
        floor of the value it rounds (a flip elsewhere is an error, not noise); an energy flip may instead sit within two rows of
        a pitch flip;
      * no more flips than 2 x the floor's own count + 2 (count_energy_near_pitch=False: energy flips within two rows of a pitch
        flip, which the pitch flip explains, are not counted — for short runs of a wide energy embedding, where one pitch flip
        moves up to five energy buckets)."""
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
    near = near_flips(pflip)
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
    assert int((eflip if count_energy_near_pitch else eflip & ~near).sum()) <= 2 * int(z["floor_energy_flips"]) + 2
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


# the kernels only batches pick by themselves, forced on for one utterance (every switch is read at every call: make the calls
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


# ---- value-range families (tests/test_gpu_value_ranges.py, tests/test_oracle_golden.py::test_oracle_value_ranges_*) --------
# Every generator is seeded and returns (x, regions): regions = [(label, index)], index a numpy index into the layer's OUTPUT
# (rows for time-preserving layers; columns where the layer keeps channels apart) that is gated on its own.

F16_MAX = 65504.0
EPS = 1e-5          # the eps of every InstanceNorm / LayerNorm of the model

# band scales: 2^-22 (every f16 operand of the band subnormal: |x| < 2^-14 up to 2^8 sigma) to 2^12 (tails near 2^14)
BAND_EXPONENTS = (-22, -16, -10, -4, 0, 6, 12)


def resblock_halo(k, dilations=(1, 3, 5)):
    """rows per side that one output row of a HiFi-GAN residual block reads: each of its pairs is a conv of dilation d
    then one of dilation 1, both 'same' with k taps, so a pair reaches d (k - 1) / 2 + (k - 1) / 2 rows: k = 11 ->
    5 (1 + 3 + 5) + 3 * 5 = 60, k = 7 -> 36, k = 3 -> 12 (rows at the stage's rate)"""
    return sum(d * (k - 1) // 2 + (k - 1) // 2 for d in dilations)


def upsample_halo(k_up, s):
    """input rows per side that one output row of a transposed conv (kernel k_up = 2 s, stride s, pad s / 2) reads:
    ceil(k_up / s) = 2 -> 2 (one spare)"""
    return -(-k_up // s)


def banded(seed, cols, halo, out_rate=1, interior=64, exponents=BAND_EXPONENTS, scale=1.0):
    """magnitude bands along time: band i is scale * 2^exponents[i] * N(0, 1), interior + 2 halo rows long; only the
    interior (halo rows away from the neighbouring bands, so the layer's output there reads one band only) is gated.
    out_rate: output rows per input row (transposed conv)."""
    rng = np.random.default_rng(seed)
    n = interior + 2 * halo
    x = np.concatenate([scale * 2.0 ** e * rng.standard_normal((n, cols)) for e in exponents]).astype(np.float32)
    regions = [(f"2^{e:+d}", slice((i * n + halo) * out_rate, (i * n + halo + interior) * out_rate)) for i, e in enumerate(exponents)]
    return x, regions


def offset(seed, rows, cols, common_ratio=None, n_special=4):
    """per channel mu_c + sigma_c z (statistics along time).  Columns, in order:
      * n_special exactly constant channels (sigma = 0; one of them all zeros);
      * n_special channels with sigma^2 ~ eps (0.5 .. 2 eps) and mu_c up to 2;
      * n_special channels with sigma^2 << eps (1e-10 .. 1e-8) and mu_c up to 2;
      * the rest: magnitude m_c in [0.5, 2], |mu_c| / sigma_c from 0 to 1e3 log-spaced (or all common_ratio), so a
        conv over them keeps the offset (a conv's output then has |mu| / sigma ~ common_ratio)."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((rows, cols))
    mu, sd = np.zeros(cols), np.ones(cols)
    s = n_special
    mu[:s] = [0.0, 1.5, -0.75, 3.0][:s]
    sd[:s] = 0.0
    mu[s:2 * s], sd[s:2 * s] = [0.0, 0.5, -1.0, 2.0][:s], np.sqrt(EPS * np.array([0.5, 1.0, 2.0, 1.0][:s]))
    mu[2 * s:3 * s], sd[2 * s:3 * s] = [0.0, 1.0, -0.3, 2.0][:s], np.sqrt(np.array([1e-10, 1e-9, 1e-8, 1e-10][:s]))
    n = cols - 3 * s
    r = np.full(n, float(common_ratio)) if common_ratio is not None else np.concatenate([[0.0], np.logspace(-1, 3, n - 1)])
    m = rng.uniform(0.5, 2.0, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    mu[3 * s:], sd[3 * s:] = sign * m * r / np.sqrt(1 + r * r), m / np.sqrt(1 + r * r)
    x = (mu + sd * z).astype(np.float32)
    rest = np.arange(3 * s, cols)
    lo = rest[r < 10] if common_ratio is None else rest[:0]
    hi = rest[r >= 10]
    regions = [("constant", np.arange(0, s)), ("var~eps", np.arange(s, 2 * s)), ("var<<eps", np.arange(2 * s, 3 * s))]
    regions += [(lbl, idx) for lbl, idx in (("mu/sd<10", lo), ("mu/sd>=10", hi)) if len(idx)]
    return x, [(lbl, (slice(None), idx)) for lbl, idx in regions]


def sparse(seed, rows, cols, zero_frac=0.9):
    """~zero_frac exact zeros, +0 and -0 mixed; the rest heavy-tailed (Student t, 2 degrees of freedom, clipped to
    +-2^12 so no f16 operand overflows)"""
    rng = np.random.default_rng(seed)
    v = np.clip(0.3 * rng.standard_t(2, (rows, cols)), -4096.0, 4096.0)
    zero = rng.random((rows, cols)) < zero_frac
    neg = rng.random((rows, cols)) < 0.5
    x = np.where(zero, np.where(neg, -0.0, 0.0), v).astype(np.float32)
    return x, [("all", slice(None))]


def near_saturation(seed, rows, cols, peak=30000.0):
    """N(0, 1) scaled so the largest |x| is `peak` (between 2^14 and 65504): the layer's first f16 operand nears the top of
    the f16 range"""
    z = np.random.default_rng(seed).standard_normal((rows, cols))
    return (z * (peak / np.max(np.abs(z)))).astype(np.float32), [("all", slice(None))]


CROSS_VALUES = (65520.0, -65520.0, 1e5, -1e5, 65504.0)
def resblock_cross_margin(dilations=(1, 3, 5)):
    """rows beyond a residual block's reach that a kernel may still make NaN where an operand is inf (inf x 0 with a zero
    weight the reference never forms): the last stage's whole-block kernel pads k = 11 to 12 taps, one more row per conv on
    one side, (1 + 1) + (3 + 1) + (5 + 1) = 12 rows for the three pairs (measured: NaN up to 72 = 60 + 12 rows before a +inf
    operand).  The transposed convs need no margin: their polyphase form's zero tap reaches one input row further than the
    reference, which upsample_halo's spare row already covers."""
    return sum(d + 1 for d in dilations)


def crossing(seed, cols, halo, margin, out_rate=1, interior=48, std=0.5):
    """N(0, std) with a few single elements at +-65520 (rounds to +-inf in f16: halfway, even is 2^16), +-1e5 and 65504
    (the largest finite f16), each alone in its row, the rows 2 halo + interior apart: the output rows that read none of
    them (the rows between two, less a margin) are gated as usual, the rest must be non-finite exactly where the oracle's are"""
    rng = np.random.default_rng(seed)
    step = interior + 2 * halo
    rows = step * (len(CROSS_VALUES) + 1)
    x = (std * rng.standard_normal((rows, cols))).astype(np.float32)
    for i, v in enumerate(CROSS_VALUES):
        x[step * (i + 1), rng.integers(cols)] = v
    # gated: the rows further than halo + margin from every crossing input (margin: resblock_cross_margin)
    regions = [(f"clean {i}", slice((step * i + halo + 1 + margin) * out_rate, (step * (i + 1) - halo - margin) * out_rate))
               for i in range(len(CROSS_VALUES) + 1)]
    return x, regions


def ln_rows(seed, rows, cols):
    """LayerNorm rows (statistics along channels): row classes in blocks of rows // 4 — normal N(0, 1); exactly constant rows;
    rows mu_r + sigma_r z with sigma_r in [0.5, 2] and |mu_r| / sigma_r log-spaced from 1 to 1e3; rows with sigma_r^2 from 1e-4 eps
    to 2 eps"""
    rng = np.random.default_rng(seed)
    q = rows // 4
    x = rng.standard_normal((rows, cols))
    x[q:2 * q] = rng.uniform(-2, 2, (q, 1))                                 # constant rows
    r = np.logspace(0, 3, q)
    m = rng.uniform(0.5, 2.0, q) * np.where(rng.random(q) < 0.5, -1, 1)
    x[2 * q:3 * q] = (m * r)[:, None] + np.abs(m)[:, None] * x[2 * q:3 * q]
    sd = np.sqrt(EPS * np.logspace(-4, 0.3, rows - 3 * q))
    x[3 * q:] = rng.uniform(-1, 1, (rows - 3 * q, 1)) + sd[:, None] * x[3 * q:]
    regions = [("normal rows", slice(0, q)), ("constant rows", slice(q, 2 * q)), ("offset rows", slice(2 * q, 3 * q)),
               ("var<=2eps rows", slice(3 * q, rows))]
    return x.astype(np.float32), regions


def ln_rows_reached(x, regions):
    """the rows of ln_rows have the statistics their labels claim (in f64, of the f32 values handed to the layer)"""
    x = x.astype(np.float64)
    mu, var = x.mean(axis=1), x.var(axis=1)
    r = dict(regions)
    assert np.all(var[r["constant rows"]] == 0.0)
    assert np.max(np.abs(mu[r["offset rows"]]) / np.sqrt(var[r["offset rows"]])) >= 5e2
    assert np.all(var[r["var<=2eps rows"]] <= 2.1 * EPS) and np.min(var[r["var<=2eps rows"]]) <= 1e-3 * EPS


def ln_scales_reached(name, y, w, b, regions):
    """what the LayerNorm made of those rows, recovered from the oracle's output: the row scale sqrt(var / (var + eps)) is 0 on
    constant rows, ~1 on the offset rows, and spans 1e-2 .. 0.82 on the rows of variance <= 2 eps"""
    t = (y.astype(np.float64) - b) / w
    s = np.sqrt(np.mean(t * t, axis=1))
    r = dict(regions)
    print(f"{name:28s} row scale: constant rows max {np.max(s[r['constant rows']]):.1e}, offset rows min "
          f"{np.min(s[r['offset rows']]):.4f}, var<=2eps rows {np.min(s[r['var<=2eps rows']]):.1e} .. {np.max(s[r['var<=2eps rows']]):.3f}")
    assert np.max(s[r["constant rows"]]) < 1e-6
    assert np.min(s[r["offset rows"]]) > 0.9
    assert np.min(s[r["var<=2eps rows"]]) < 2e-2 and np.max(s[r["var<=2eps rows"]]) < 0.83


def attention_extremes(seed, rows, cols, scale=24.0, group=4):
    """scale * N(0, 1) rows in groups of `group` exactly identical rows: logits q.k / sqrt(dk) reach far beyond 88 (exp
    overflows f32 without the max subtraction) and every key is tied exactly with the others of its group"""
    z = np.random.default_rng(seed).standard_normal(((rows + group - 1) // group, cols))
    return (scale * np.repeat(z, group, axis=0)[:rows]).astype(np.float32), [("all", slice(None))]


def oracle_triple(o, fn, *args, **kw):
    """oracle_pair + the oracle in ORDER_SEQ_F64 (the same f16 operand points, one f64 accumulator per dot product)"""
    from oracle import zvoracle
    ref, alt = oracle_pair(o, fn, *args, **kw)
    o.set_order(zvoracle.ORDER_SEQ_F64)
    hi = getattr(o, fn)(*args, **kw)
    o.set_order(zvoracle.ORDER_GGML_AVX2)
    return ref, alt, hi


# the f64 judge: rms(GPU - f64 oracle) <= JUDGE_MULT x the farther of the two f32 orders of the oracle (AVX2 lanes, sequential)
# from the f64 oracle + JUDGE_ABS rms(signal), per region.  Measured on the MI355X the GPU's long k-ordered f32 chains sit 1-5x
# further from the f64 result than the AVX2 order's 32 short chains and at or below the sequential order's distance (the GPU
# and the sequential order both accumulate in long f32 chains), so the envelope is the farther of the two f32 orders.
JUDGE_MULT, JUDGE_ABS = 2.0, 3e-7


def region_gates(name, got, ref, alt, hi, regions, rel_gate, floor_mult=2.0, resolution=None):
    """layer_gate on every region alone, its floor from that same region: the farther of the oracle's two other summation
    orders (sequential f32 `alt`, and f64 `hi` where given) from its AVX2 order `ref` (a region of a few hundred values may
    hold one f16 re-rounding flip in one order and none in another); where hi is given, the f64 judge on it.  A region whose
    oracle output is all zeros must be all zeros on the GPU too.  resolution (same shape as got): the f32 spacing the values
    were measured through (a response f(x) - f(0) is resolved only to the spacing of f(x)); half of it, in rms, joins the floor."""
    worst = []
    for label, idx in regions:
        g, r, a = got[idx], ref[idx], alt[idx]
        assert np.isfinite(r).all() and np.isfinite(a).all(), f"{name} [{label}]: the oracle is not finite"
        if _rms(r) == 0.0:
            assert np.array_equal(g, r), f"{name} [{label}]"
            continue
        sig = _rms(r)
        if hi is not None and _rms(hi[idx] - r) > _rms(a - r):
            a = hi[idx]
        if resolution is not None:
            res = 0.5 * _rms(resolution[idx])
            err = _rms(g - r)
            print(f"{name + ' [' + label + ']':28s} rel rms err {err / sig:.2e} (oracle self-noise {_rms(a - r) / sig:.2e}, "
                  f"f32 resolution {res / sig:.2e}), signal rms {sig:.3e}")
            assert np.isfinite(g).all()
            assert err <= max(floor_mult * _rms(a - r), res, 3e-7 * sig) and err <= rel_gate * sig, f"{name} [{label}]"
        else:
            layer_gate(f"{name} [{label}]", g, r, a, rel_gate, floor_mult)
        if hi is not None:
            h = hi[idx]
            e_g, e_r, e_s = _rms(g - h), _rms(r - h), _rms(alt[idx] - h)
            print(f"{'':28s} vs f64 oracle: gpu {e_g / sig:.2e}, avx2 oracle {e_r / sig:.2e}, sequential-f32 oracle {e_s / sig:.2e}")
            assert e_g <= JUDGE_MULT * max(e_r, e_s) + JUDGE_ABS * sig, f"{name} [{label}] vs the f64 oracle"
        worst.append((label, _rms(g - r) / sig, _rms(a - r) / sig))
    return worst


def nonfinite_masks_equal(name, got, ref):
    """the same NaN positions and the same signed-inf positions (two orders of the oracle)"""
    for what, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        mg, mr = f(got), f(ref)
        assert np.array_equal(mg, mr), f"{name}: {what} at {int(mg.sum())} positions in one, {int(mr.sum())} in the other " \
                                       f"({int((mg != mr).sum())} differ)"
    print(f"{name:28s} non-finite: {int(np.isnan(ref).sum())} NaN, {int(np.isinf(ref).sum())} inf, masks equal")


def nonfinite_footprint(name, got, ref, clean_rows):
    """what the GPU's conv kernels do where an f16 operand is +-inf (gate 7): every position the oracle makes
    non-finite is non-finite on the GPU; every +-inf the GPU gives is the oracle's inf of the same sign at that position (an
    oracle inf may be NaN on the GPU); the GPU's non-finite values stay inside the rows that read a crossing input (clean_rows:
    boolean per output row, True where no crossing input is read) — the matrix-core tiles also multiply the inf operand by
    zero weights (padded taps / channels, the transposed convs' structural zero taps) that the reference never forms"""
    nf_g, nf_r = ~np.isfinite(got), ~np.isfinite(ref)
    assert nf_g[nf_r].all(), f"{name}: {int((nf_r & ~nf_g).sum())} oracle non-finite positions are finite on the GPU"
    gi = np.isinf(got)
    assert np.array_equal(got[gi], ref[gi]), f"{name}: a GPU inf is not the oracle's inf of the same sign"
    bad = np.flatnonzero(clean_rows & np.any(nf_g, axis=tuple(range(1, got.ndim))))
    assert not len(bad), f"{name}: non-finite values outside the rows that read a crossing input: rows {bad[:8]} .. {bad[-8:]} " \
                         f"({len(bad)} rows; rows with oracle non-finite {np.flatnonzero(np.any(nf_r, axis=tuple(range(1, got.ndim))))[[0, -1]]})"
    print(f"{name:28s} non-finite: oracle {int(np.isnan(ref).sum())} NaN / {int(np.isinf(ref).sum())} inf, GPU "
          f"{int(np.isnan(got).sum())} NaN / {int(gi.sum())} inf")


def ln_row_scale_gate(name, got, ref, alt, w, b, mult=2.0, floor_abs=1e-7):
    """LayerNorm output rows y = w t + b with t = (u - mean) rstd: the scale of each row, sqrt(mean t^2) = sqrt(var / (var + eps)),
    is a per-row factor common to all C values, so a wrong variance shows in it ~sqrt(C) more clearly than in the per-value rms
    gate.  max over rows |s_gpu / s_oracle - 1| <= mult x the same for the oracle's sequential-f32 order + floor_abs"""
    def scale(y):
        t = (y.astype(np.float64) - b) / w
        return np.sqrt(np.mean(t * t, axis=1))
    s_r = scale(ref)
    z = s_r == 0.0                                         # constant rows: the output is b itself, on the GPU too
    assert np.array_equal(got[z], ref[z]), name
    d_g, d_a = (float(np.max(np.abs(scale(a)[~z] / s_r[~z] - 1))) for a in (got, alt))
    print(f"{name:28s} LayerNorm row scale: max rel dev {d_g:.2e} (oracle self-noise {d_a:.2e})")
    assert d_g <= mult * d_a + floor_abs, name


# ---- stage inputs of tests/golden/value_ranges_small.npz (make_golden.py value_ranges) --------------------------------------
VR_DEC_T, VR_ZERO_ROWS = 96, slice(40, 56)
# vocoder mel: four bands of VR_BAND frames along time, the normalised input (mel - mean) / scale at 0 exactly (mel ==
# hifigan.mean), 1e-3, 1 and 8 times N(0, 1); a band's middle VR_GATED frames lie further than the vocoder's reach from the
# next band: input conv k7 (3 frames), each transposed conv (2 input rows) and each stage's k = 11 residual block (60 rows at
# rates 5, 25, 100, 300): 3 + 2 + 12 + 1 + 3 + 1 + 1 + 1 + 1 + 1 (output conv) = 26 frames < (64 - 8) / 2
VR_BAND, VR_GATED, VR_MEL_SCALES = 64, 8, (0.0, 1e-3, 1.0, 8.0)


def value_range_stage_inputs(g, tensors, seed=31):
    """(hidden [T, E], style [E], mel [T, num_mels], decoder regions (mel rows), vocoder regions (wav samples))"""
    hidden, _ = offset(seed, VR_DEC_T, g.E)
    hidden[VR_ZERO_ROWS] = 0.0
    style = (0.05 * np.random.default_rng(seed + 1).standard_normal(g.E)).astype(np.float32)
    mean, scale = tensors["hifigan.mean"].astype(np.float32), tensors["hifigan.scale"].astype(np.float32)
    z = np.random.default_rng(seed + 2).standard_normal((VR_BAND * len(VR_MEL_SCALES), g.num_mels))
    n = np.repeat(np.array(VR_MEL_SCALES), VR_BAND)[:, None] * z
    mel = (mean + scale * n).astype(np.float32)
    mel[:VR_BAND] = mean                                       # exactly at the mean: (mel - mean) / scale == 0
    dec_regions = [("all frames", slice(None)), ("zero-hidden frames", VR_ZERO_ROWS)]
    lo = (VR_BAND - VR_GATED) // 2
    voc_regions = [(f"mel band n x {s:g}", slice((i * VR_BAND + lo) * g.hop_size, (i * VR_BAND + lo + VR_GATED) * g.hop_size))
                   for i, s in enumerate(VR_MEL_SCALES)]
    return hidden, style, mel, dec_regions, voc_regions


# ---- vocoder receptive field (tests/test_gpu_vocoder_geometries.py, tests/test_boundary_cpu.py) ----------------------------

def upsample_window(K, s):
    """input rows relative to floor(t / s) that output row t of the reference's transposed conv reads (kernel K, stride s,
    padding s / 2 + s % 2, output padding s % 2, src/hifigan.cpp:22-71): (lowest, highest)"""
    p = s // 2 + s % 2
    off = K - 1 - p
    ds = [(k - off + r) // s for r in range(s) for k in range(K) if (k - off + r) % s == 0]
    return min(ds), max(ds)


def receptive_radius(g, tensors):
    """exact receptive radius of one output sample in mel frames, from the checkpoint's tensors: the input rows each output sample
    of one frame reads, walked back through output conv, 4 x (residual blocks, transposed conv) and input conv.  A stage's residual
    blocks reach the widest branch's sum over its pairs of (K1 - 1) / 2 d + (K2 - 1) / 2 rows."""
    k_in = tensors["_meldec.input_conv.w"].shape[2]
    k_out = tensors["_meldec.output_conv.1.w"].shape[2]
    stages = []
    for i in range(len(g.upsample_kernels)):
        K = tensors[f"_meldec.upsamples.{i}.1.w"].shape[2]
        reach = 0
        for j in range(len(g.resblock_kernels)):
            n = i * len(g.resblock_kernels) + j
            reach = max(reach, sum((tensors[f"_meldec.blocks.{n}.convs1.{d}.1.w"].shape[2] - 1) // 2 * dil +
                                   (tensors[f"_meldec.blocks.{n}.convs2.{d}.1.w"].shape[2] - 1) // 2
                                   for d, dil in enumerate(g.resblock_dilations)))
        stages.append((K, K // 2, reach))
    worst = 0
    for t in range(g.hop_size):             # the samples of frame 0: every frame's samples read the same offsets
        a, b = t - (k_out - 1) // 2, t + (k_out - 1) // 2
        for K, s, reach in reversed(stages):
            a, b = a - reach, b + reach
            lo, hi = upsample_window(K, s)
            a, b = a // s + lo, b // s + hi
        a, b = a - (k_in - 1) // 2, b + (k_in - 1) // 2
        worst = max(worst, -a, b)
    return worst


# ---- the merged MRF sum as the output conv's input (tests/test_gpu_vocoder_widths.py, tests/test_voc_plan_cpu.py) -----------
# (geometry, switches, plan of one utterance of WIDTH_MERGE_T frames as tests/native/voc_plan_check.cpp prints it, whether the last
# stage stores the merged sum: the output conv then reads one tensor).  The GPU test runs these switches at this length; the CPU test
# holds csrc/voc_plan.h to the plans, so the GPU test knows which form ran without a profile (the merged launch and the three
# branches side by side are both one launch).  The 32-channel last stage of small_v496 runs the whole-block kernel, which never
# merges: its merged sum (31 real channels) reaches the output conv only with that kernel off.
WIDTH_MERGE_T = 40
WIDTH_MERGE_CASES = (
    ("small_v1024", {"ZV_MERGE_ALWAYS": 1}, "r0 h0 -N000- -N000- -F0001 -F0001", True),
    ("small_v1024", {"ZV_MERGE_ALWAYS": 1, "ZV_MERGE_SEQ": 0}, "r0 h0 -N000- -N000- -F0001 -F0001", True),
    ("small_v1024", {"ZV_MERGE_ALWAYS": 1, "ZV_FUSE256": 1}, "r0 h0 -N000- -F0003 -F0001 -F0001", True),
    ("small_v496", {"ZV_MERGE_ALWAYS": 1}, "r0 h0 -N000- -F0001 -F0001 -W000-", False),
    ("small_v496", {"ZV_MERGE_ALWAYS": 1, "ZV_MERGE_SEQ": 0}, "r0 h0 -N000- -F0001 -F0001 -W000-", False),
    ("small_v496", {"ZV_MERGE_ALWAYS": 1, "ZV_NO_TRIPLE": 1}, "r0 h0 -N000- -F0001 -F0001 -F0001", True),
    ("small_v496", {"ZV_MERGE_ALWAYS": 1, "ZV_MERGE_SEQ": 0, "ZV_NO_TRIPLE": 1, "ZV_FUSE256": 1}, "r0 h0 -F0001 -F0001 -F0001 -F0001", True),
)


# ---- decoder conv tile split (tests/test_gpu_encdec_geometries.py, tests/test_boundary_cpu.py) ------------------------------
# restated from zerovox.cpp_amd/csrc/conv_gemm.hip (conv_gemm_groups / conv_gemm_tiles): a wide conv of a batch runs whole groups
# of 8 32-channel output tiles on conv_gemm_kernel, which also takes ONE leftover tile; two or more leftovers run on
# conv1d_mfma_kernel from tile nt_begin = conv_gemm_tiles on (conv.hip launch_conv)

def conv_gemm_groups(cout_p):
    return ((cout_p + 31) // 32) // 8


def conv_gemm_tiles(cout_p):
    nt = (cout_p + 31) // 32
    ng = nt // 8
    return ng * 8 + (1 if nt - ng * 8 == 1 and ng >= 1 else 0)


def conv_tile_split(cout):
    """(tiles, tiles on conv_gemm_kernel, tiles left to the generic kernel) of a decoder conv of cout channels"""
    cout_p = (cout + 15) // 16 * 16
    nt = (cout_p + 31) // 32
    done = conv_gemm_tiles(cout_p)
    return nt, done, nt - done


# ---- attention and LayerNorm-tail limits (tests/test_gpu_attention_heads.py, tests/test_boundary_cpu.py) --------------------
# restated from zerovox.cpp_amd/csrc/stage_plan.h (att_plan, layernorm_tail_ok); tests/test_stage_plan_cpu.py compares them with
# what the header gives

ATT_NS_MAX, ATT_LDS_MAX, LN_TAIL_MAX = 144, 160 * 1024 - 4096, 64 * 12


def mfma_max_tokens(dk):
    """largest n the matrix-core attention kernel takes at head dim dk (0: never)"""
    if dk % 4 or dk > 2 * ATT_NS_MAX:
        return 0
    n = 0
    while ((64 * (dk | 1) + 1 + 64 * ((n + 1 + 31) // 32 * 32)) * 4) <= ATT_LDS_MAX:
        n += 1
    return n


def encoder_margins(ex, alt):
    """the reference semantics' own re-association noise on one encoder run, in the form encoder_decisions_vs_reference reads:
    ex = the oracle in the reference's summation order (bit-exact to it: tests/test_oracle_golden.py), alt = the oracle in
    sequential f32 order (as tests/golden/make_golden.py _encoder_margins, computed live)"""
    dur_r = np.exp(ex["logdur"].astype(np.float64)) - 1 + 0.5
    dur_a = np.exp(alt["logdur"].astype(np.float64)) - 1 + 0.5
    pflip = alt["pitch_bucket"] != ex["pitch_bucket"]
    clean = ~near_flips(pflip)
    return dict(logdur=ex["logdur"], pitch=ex["pitch"], energy=ex["energy"], pitch_bucket=ex["pitch_bucket"],
                energy_bucket=ex["energy_bucket"], n_frames=ex["n_frames"],
                floor_logdur_max=float(np.max(np.abs(alt["logdur"] - ex["logdur"]))),
                floor_pitch_max=float(np.max(np.abs(alt["pitch"] - ex["pitch"]))),
                floor_energy_max=float(np.max(np.abs(alt["energy"][clean] - ex["energy"][clean]))) if clean.any() else 0.0,
                floor_dur_flips=int(np.sum(dur_r.astype(np.int64) != dur_a.astype(np.int64))),
                floor_pitch_flips=int(pflip.sum()), floor_energy_flips=int(np.sum(alt["energy_bucket"] != ex["energy_bucket"])))


# ---- sizes at the limits (tests/test_gpu_long.py, tests/test_long_cpu.py) ---------------------------------------------------
# restated from zerovox.cpp_amd/csrc/capi.cpp (batch_group_end): a launch group takes utterances while it holds at most 64 of
# them and (count) x (the longest T so far rounded up to 64) stays <= 64 Ki frames of capacity; the first always fits

GROUP_MAX_UTTERANCES, GROUP_MAX_FRAMES = 64, 65536


def launch_group_end(a, Ts):
    b, tmax = a, 0
    while b < len(Ts) and b - a < GROUP_MAX_UTTERANCES:
        tm = max(tmax, Ts[b])
        if b > a and (b - a + 1) * ((tm + 63) // 64 * 64) > GROUP_MAX_FRAMES:
            break
        tmax = tm
        b += 1
    return b


def launch_groups(Ts):
    """sizes of the launch groups zv_synthesize_batch splits utterances of capacities Ts into"""
    sizes, a = [], 0
    while a < len(Ts):
        b = launch_group_end(a, Ts)
        sizes.append(b - a)
        a = b
    return sizes


def voc_stage_bytes_per_frame(scales, voc_channels):
    """bytes of one mel frame's rows in the f32 tensor of each vocoder stage: rate x channels (padded to 16) x 4"""
    out, rate = [], 1
    for i, s in enumerate(scales):
        rate *= s
        out.append(rate * (((voc_channels >> (i + 1)) + 15) // 16 * 16) * 4)
    return out


def offset_crossing_frames(bytes_per_frame, T, lowest=27):
    """{frame: [(stage, k)]}: the frames of a T-frame utterance whose rows hold byte 2^k (k >= lowest) of a stage's tensor"""
    frames = {}
    for i, bpf in enumerate(bytes_per_frame):
        k = lowest
        while (1 << k) < bpf * T:
            frames.setdefault((1 << k) // bpf, []).append((i, k))
            k += 1
    return frames


WINDOW_FRAMES = 64


def oracle_windows(crossings, T):
    """[(a, b)]: 64-frame windows at the start, around every crossing frame (the frame in the middle) and at the end"""
    w = [(0, WINDOW_FRAMES)] + [(f - WINDOW_FRAMES // 2, f + WINDOW_FRAMES // 2) for f in sorted(crossings)] + [(T - WINDOW_FRAMES, T)]
    assert all(0 <= a < b <= T for a, b in w)
    return w


def window_of_oracle(o_vocoder, mel, a, b, H, hop):
    """samples [a hop, b hop) of the vocoder of `mel`, computed from frames [a - H, b + H) alone (clipped to the utterance)"""
    lo, hi = max(0, a - H), min(len(mel), b + H)
    w = o_vocoder(mel[lo:hi])
    return w[(a - lo) * hop:(b - lo) * hop]


def block_gates(name, got, ref, alt, block=256, rms_mult=2.0, max_mult=1.5):
    """rows in blocks of `block`: every block's rms error <= rms_mult x max(its own floor, the median block floor), its max-abs
    error likewise with max_mult; the floors are the oracle's alone (alt vs ref).  Returns the worst ratios against the block's
    own floor: (rms ratio, block, max ratio, block)"""
    n = got.shape[0] // block
    assert n * block == got.shape[0]
    e, f = (got - ref).astype(np.float64).reshape(n, -1), (alt - ref).astype(np.float64).reshape(n, -1)
    e_rms, f_rms = np.sqrt(np.mean(e * e, axis=1)), np.sqrt(np.mean(f * f, axis=1))
    e_max, f_max = np.max(np.abs(e), axis=1), np.max(np.abs(f), axis=1)
    assert np.all(f_rms > 0) and np.all(f_max > 0), f"{name}: a block with a zero floor"
    r_rms, r_max = e_rms / f_rms, e_max / f_max
    i, j = int(np.argmax(r_rms)), int(np.argmax(r_max))
    print(f"{name}: {n} blocks of {block} rows; floors rms min {f_rms.min():.2e} median {np.median(f_rms):.2e} max {f_rms.max():.2e}, "
          f"max-abs {f_max.min():.2e} / {np.median(f_max):.2e} / {f_max.max():.2e}; worst rms ratio to the block's own floor "
          f"{r_rms[i]:.3f} (block {i}), worst max-abs ratio {r_max[j]:.3f} (block {j})")
    bad = np.flatnonzero((e_rms > rms_mult * np.maximum(f_rms, np.median(f_rms))) | (e_max > max_mult * np.maximum(f_max, np.median(f_max))))
    assert not len(bad), f"{name}: blocks {bad[:16]} ({len(bad)}) beyond the gate"
    return float(r_rms[i]), i, float(r_max[j]), j
