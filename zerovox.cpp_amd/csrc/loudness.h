// loudness.h — loudness (include/zerovox_amd.h "loudness"): ITU-R BS.1770 K-weighted, gated loudness, the true peak of the 4x
// oversampled signal and the gain that brings an utterance to a LUFS target under a dBTP ceiling.  Plain arithmetic shared by the
// kernels (loudness_kernels.hip), the C-ABI (capi.cpp) and the host-side test (tests/native/loudness_check.cpp): nothing here needs HIP.
//
// K-weighting is a recursive filter, and a caller must be able to restate every result bit for bit.  So the RULE fixes the split: the
// signal is cut into chunks of 256 samples, every chunk is filtered from the zero state (phase A), the true entry states follow from
// a 4 x 4 matrix recurrence over the chunks (phase B), and every chunk is filtered again from its entry state (phase C).  Whoever runs
// the chunks, in whatever order or tiling, gets the same bits; the host reference below runs them one after the other.
// Every f64 step is ONE IEEE operation (+, -, *, /, sqrt or a conversion), written as a statement or a parenthesis of its own, never a
// CONTRACTED multiply-add: the library and the checks build with -ffp-contract=off and the kernels carry the contraction pragma.  Two
// places write a fused multiply-add out, as the one IEEE operation it is: loud_tp_step, whose product of two f32 values is exact in f64, so
// the fused and the unfused form round alike (filter.h), and the host-only loud_square of the design.
// Denormals are kept.  A sample that is not finite counts as +0.0.  The logarithm of the report is mel.h's mel_ln, not libm's.
//
// The design (loud_design: both biquads, the step, M = A^256 and the interpolator) is computed on the host and travels as DATA, so
// libm's tan, pow and cos never reach a comparison of bits between a device and a host.
#pragma once

#include <math.h>
#include <stdint.h>

#include "mel.h"          // mel_ln, mel_from_bits, level_bits (level.h): the fixed logarithm of the report

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

namespace zv
{

constexpr int      LOUD_CHUNK = 256;                          // samples per chunk
constexpr int      LOUD_TAPS = 49;                            // interpolator c[0 .. 48]
constexpr int      LOUD_PHASE_TAPS = 12;                      // taps of one phase: c[f + 4 k], k = 0 .. 11
constexpr int      LOUD_TP_TAIL = 11;                         // the interpolator rings for 11 samples behind the span
constexpr int      LOUD_TP_TILE = 2048;                       // outputs one workgroup of the true-peak kernel covers: 256 lanes, 8 each
constexpr int      LOUD_WG_CHUNKS = 64;                       // chunks one workgroup of the two chunk kernels owns: one per lane
constexpr int      LOUD_SLICE = 64;                           // samples of every chunk a workgroup stages through LDS at a time
constexpr uint32_t LOUD_MIN_RATE = 4000, LOUD_MAX_RATE = 768000;      // step >= 256 (a chunk meets at most two steps) and f0 < fs / 2
constexpr uint32_t LOUD_FLAG_TARGET = 1u, LOUD_FLAG_CEILING = 2u;
constexpr uint64_t LOUD_GATE_ABS_BITS = 0x3e7f791ec6e1d5aaull;   // the f64 nearest to 10^((-70 + 0.691) / 10) = 1.17246530458229639...e-7
constexpr uint64_t LOUD_TENTH_BITS = 0x3fb999999999999aull;      // 0.1
constexpr uint64_t LOUD_OFFSET_BITS = 0xbfe61cac083126e9ull;     // -0.691
constexpr uint64_t LOUD_LOG10E_BITS = 0x3fdbcb7b1526e50eull;     // log10 e (mel.h)

// The design; the layout of include/zerovox_amd.h zv_loudness_filter.
struct LoudFilter
{
    double   shelf_b[3], shelf_a[2];      // stage 1: b0 b1 b2, a1 a2 (a0 = 1)
    double   highpass_b[3], highpass_a[2];      // stage 2: (1, -2, 1), a1 a2
    double   M[16];                       // A^256, row major, on the state (p1, p2, q1, q2)
    float    c[LOUD_TAPS];                // the interpolator
    uint32_t step;                        // samples per 100 ms gating step: (fs + 5) / 10
};

// What one utterance asks for, as the kernels read it (capi.cpp packs it from a zv_loudness): zt is the target as a mean square.
struct LoudAsk
{
    double   zt;
    float    gain, ceiling;
    uint32_t flags, reserved;
};

// What one utterance gets; the layout of include/zerovox_amd.h zv_loudness_result.
struct LoudRow
{
    double   integrated_ms, momentary_max_ms, short_term_max_ms, true_peak;
    uint32_t blocks, blocks_absolute, blocks_gated;
    float    sample_peak;
    float    integrated_lufs, momentary_max_lufs, short_term_max_lufs, true_peak_dbtp;
    float    gain;
    uint32_t reserved;
};

// One utterance of a launch group, as the kernels find it: offsets into the group's arrays.
struct LoudSeg
{
    int64_t x0;            // first sample in the waveform array (a multiple of LOUD_CHUNK)
    int64_t N;             // samples measured: min(n_frames, T) * hop
    int64_t total;         // samples scaled: T * hop
    int32_t chunk0;        // first entry of the state and run arrays
    int32_t step0;         // first entry of the step-energy and block arrays
    int32_t tile0;         // first entry of the true-peak slab
    int32_t reserved;
};

ZV_LV_FN uint64_t loud_dbits(double d)
{
    uint64_t b;
    __builtin_memcpy(&b, &d, 8);
    return b;
}
ZV_LV_FN int64_t loud_chunks(int64_t N) { return (N + LOUD_CHUNK - 1) / LOUD_CHUNK; }
ZV_LV_FN int64_t loud_tp_tiles(int64_t N) { return (N + LOUD_TP_TAIL + LOUD_TP_TILE - 1) / LOUD_TP_TILE; }
ZV_LV_FN bool loud_finite(float x) { return (level_bits(x) & 0x7fffffffu) < 0x7f800000u; }
ZV_LV_FN double loud_sample(float x) { return loud_finite(x) ? (double)x : 0.0; }

// ---- K-weighting: one sample through the cascade, transposed direct form II, state s = (p1, p2, q1, q2) ----
//   y   = b0 x + p1          w   = y + q1                       (the high-pass has b = (1, -2, 1): its products are exact)
//   p1' = (b1 x + p2) - a1 y      q1' = (q2 - 2 y) - a1' w
//   p2' = b2 x - a2 y             q2' = y - a2' w
// The chain from sample to sample is p1 -> y -> a1 y -> p1' (three operations) and likewise q1 -> w -> a1' w -> q1'.
ZV_LV_FN double loud_kweight(const LoudFilter &F, double s[4], double x)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double t0 = F.shelf_b[0] * x;
    const double y = t0 + s[0];
    const double t1 = F.shelf_b[1] * x;
    const double t2 = t1 + s[1];
    const double t3 = F.shelf_a[0] * y;
    const double t4 = F.shelf_b[2] * x;
    const double t5 = F.shelf_a[1] * y;
    s[0] = t2 - t3;
    s[1] = t4 - t5;
    const double w = y + s[2];
    const double u0 = 2.0 * y;
    const double u1 = s[3] - u0;
    const double u2 = F.highpass_a[0] * w;
    const double u3 = F.highpass_a[1] * w;
    s[2] = u1 - u2;
    s[3] = y - u3;
    return w;
}

// phase B, one step: s' = M s + z; rows in ascending order, each a left-to-right dot product, then + z
ZV_LV_FN void loud_advance(const double *M, double s[4], const double z[4])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double n[4];
    for (int r = 0; r < 4; r++)
    {
        double acc = M[4 * r] * s[0];
        double t = M[4 * r + 1] * s[1];
        acc = acc + t;
        t = M[4 * r + 2] * s[2];
        acc = acc + t;
        t = M[4 * r + 3] * s[3];
        acc = acc + t;
        n[r] = acc + z[r];
    }
    for (int r = 0; r < 4; r++) s[r] = n[r];
}

// phase C, one sample: w^2 into the run of its step (run 0 before the chunk's step boundary `edge`, run 1 from it on)
ZV_LV_FN void loud_run_add(double run[2], double w, bool second)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double q = w * w;
    if (second) run[1] = run[1] + q;
    else run[0] = run[0] + q;
}
// the first sample of chunk k that belongs to the chunk's second step (>= 256 (k + 1): the chunk has one run)
ZV_LV_FN int64_t loud_edge(int64_t k, uint32_t step) { return ((int64_t)LOUD_CHUNK * k / step + 1) * step; }

// phase D: the energy of step j from the run sums, runs[2 * chunk + r], the chunks in ascending order
ZV_LV_FN double loud_step_energy(const double *runs, int64_t j, uint32_t step)
{
    const int64_t c0 = j * step / LOUD_CHUNK, c1 = ((j + 1) * step - 1) / LOUD_CHUNK;
    double E = 0.0;
    for (int64_t c = c0; c <= c1; c++) E = E + runs[2 * c + (j - (int64_t)LOUD_CHUNK * c / step)];
    return E;
}

// ---- gating ----
ZV_LV_FN double loud_gate_abs() { return mel_from_bits(LOUD_GATE_ABS_BITS); }
// momentary block i from the step energies
ZV_LV_FN double loud_momentary(const double *E, int64_t i, uint32_t step)
{
    double z = E[i] + E[i + 1];
    z = z + E[i + 2];
    z = z + E[i + 3];
    const double den = (double)(4 * (uint64_t)step);
    return z / den;
}
// short-term block i: steps i .. i + 29
ZV_LV_FN double loud_short_term(const double *E, int64_t i, uint32_t step)
{
    double z = 0.0;
    for (int k = 0; k < 30; k++) z = z + E[i + k];
    const double den = (double)(30 * (uint64_t)step);
    return z / den;
}
// Γr from the sum and the count of the blocks past the absolute gate (count > 0)
ZV_LV_FN double loud_gate_rel(double sum, uint32_t count)
{
    const double mean = sum / (double)count;
    return mel_from_bits(LOUD_TENTH_BITS) * mean;
}

// ---- true peak: one output of one phase; xs[k] = x'[n - k], k = 0 .. 11 ----
ZV_LV_FN double loud_tp_step(double acc, float c, double xs) { return __builtin_fma((double)c, xs, acc); }
ZV_LV_FN double loud_tp_phase(const float *c, int f, const double *xs)
{
    double acc = 0.0;
    for (int k = 0; k < LOUD_PHASE_TAPS; k++) acc = loud_tp_step(acc, c[f + 4 * k], xs[k]);
    return acc;
}

// ---- report and gain ----
// LUFS of a mean square: -0.691 + 10 log10 z; -inf for z below the smallest normal f64 (mel_ln takes normal values)
ZV_LV_FN float loud_lufs(double z)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(z >= mel_from_bits(0x0010000000000000ull))) return -INFINITY;
    double r = mel_ln(z);
    r = r * mel_from_bits(LOUD_LOG10E_BITS);
    r = 10.0 * r;
    r = mel_from_bits(LOUD_OFFSET_BITS) + r;
    return (float)r;
}
ZV_LV_FN float loud_dbtp(double tp)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(tp >= mel_from_bits(0x0010000000000000ull))) return -INFINITY;
    double r = mel_ln(tp);
    r = r * mel_from_bits(LOUD_LOG10E_BITS);
    r = 20.0 * r;
    return (float)r;
}
ZV_LV_FN float loud_gain(const LoudAsk &q, double z_int, double tp)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double gd = (double)q.gain;
    if ((q.flags & LOUD_FLAG_TARGET) && z_int > 0.0)
    {
        double r = q.zt / z_int;
        r = sqrt(r);
        gd = r * (double)q.gain;
    }
    bool ceiling = false;
    if (q.flags & LOUD_FLAG_CEILING)
    {
        const double scaled = gd * tp;
        if (scaled > (double)q.ceiling)
        {
            gd = (double)q.ceiling / tp;
            ceiling = true;
        }
    }
    float g = (float)gd;
    // the promise: (float)((double)g * tp) <= ceiling.  (float)gd may have rounded up: one bit pattern down is nextafterf(g, 0)
    for (int k = 0; ceiling && k < 4; k++)
    {
        const double p = (double)g * tp;
        if (!((float)p > q.ceiling) || g == 0.0f) break;
        g = level_from_bits(level_bits(g) - 1u);
    }
    return g;
}

// the result row from the gated values and the peaks: report and gain
ZV_LV_FN LoudRow loud_finish(double z_int, double mom, double sht, uint32_t nb, uint32_t na, uint32_t ng, double tp, float sample_peak,
                             const LoudAsk &q)
{
    LoudRow r;
    r.integrated_ms = z_int;
    r.momentary_max_ms = mom;
    r.short_term_max_ms = sht;
    r.true_peak = tp;
    r.blocks = nb;
    r.blocks_absolute = na;
    r.blocks_gated = ng;
    r.sample_peak = sample_peak;
    r.integrated_lufs = loud_lufs(z_int);
    r.momentary_max_lufs = loud_lufs(mom);
    r.short_term_max_lufs = loud_lufs(sht);
    r.true_peak_dbtp = loud_dbtp(tp);
    r.gain = loud_gain(q, z_int, tp);
    r.reserved = 0;
    return r;
}

// Everything behind the step energies and the peaks, for one utterance: E[0 .. J) the step energies, z[] room for J - 3 momentary
// blocks (J >= 4), tp and sample_peak the maxima.  Sequential; the gate kernel computes the same values with the independent ones
// (blocks, short-term sums, maxima) shared over lanes and the two gated sums as this chain.
ZV_LV_FN LoudRow loud_gate(const double *E, int64_t J, double *z, uint32_t step, double tp, float sample_peak, const LoudAsk &q)
{
    const int64_t nb = J >= 4 ? J - 3 : 0;
    double mom = 0.0, sht = 0.0;
    for (int64_t i = 0; i < nb; i++)
    {
        z[i] = loud_momentary(E, i, step);
        mom = z[i] > mom ? z[i] : mom;
    }
    for (int64_t i = 0; i + 30 <= J; i++)
    {
        const double v = loud_short_term(E, i, step);
        sht = v > sht ? v : sht;
    }
    const double ga = loud_gate_abs();
    double sum = 0.0;
    uint32_t na = 0, ng = 0;
    for (int64_t i = 0; i < nb; i++)
        if (z[i] > ga)
        {
            sum = sum + z[i];
            na++;
        }
    double z_int = 0.0;
    if (na)
    {
        const double gr = loud_gate_rel(sum, na);
        sum = 0.0;
        for (int64_t i = 0; i < nb; i++)
            if (z[i] > ga && z[i] > gr)
            {
                sum = sum + z[i];
                ng++;
            }
        if (ng) z_int = sum / (double)ng;
    }
    return loud_finish(z_int, mom, sht, (uint32_t)nb, na, ng, tp, sample_peak, q);
}

// validation of a zv_loudness {gain, target_lufs, true_peak_ceiling, flags}: null, else the name of the field that is wrong
ZV_LV_FN const char *loud_check(float gain, float target_lufs, float ceiling, uint32_t flags)
{
    if (!loud_finite(gain) || !(gain >= 0.0f && gain <= 1000.0f)) return "gain";
    if (!loud_finite(target_lufs)) return "target_lufs";
    if (!loud_finite(ceiling)) return "true_peak_ceiling";
    if (flags & ~(LOUD_FLAG_TARGET | LOUD_FLAG_CEILING)) return "flags";
    if ((flags & LOUD_FLAG_TARGET) && !(target_lufs >= -70.0f && target_lufs <= 0.0f)) return "target_lufs";
    if ((flags & LOUD_FLAG_CEILING) && !(ceiling > 0.0f && ceiling <= 1.0f)) return "true_peak_ceiling";
    return nullptr;
}

// One launch group as the kernels take it (kernels.h launch_loud_*): every array holds the group's utterances one behind the other, at
// the offsets of their LoudSeg.
struct LoudJob
{
    float *wav;                    // the samples, utterance u at segs[u].x0; the apply pass scales them in place
    double *state;                 // [chunk][4]: phase A stores z_k, phase B replaces it by the entry state s_k
    double *runs;                  // [chunk][2]: phase C's run sums
    double *energy, *blocks;       // [step]: E_j and the momentary blocks z_i
    uint64_t *peaks;               // [tile][2]: the true-peak pass's maxima per workgroup: f64 bits of |v|, f32 bits of the sample peak
    LoudRow *rows;                 // [utterance]
    const LoudSeg *segs;
    const LoudAsk *asks;
    const LoudFilter *filter;      // the model's design, in device memory
    int nseg;
    int64_t max_N, max_total;      // the longest measured span and the longest capacity of the group, in samples
    uint32_t step;
};

// launch groups: consecutive utterances whose padded capacities stay within LOUD_GROUP_SAMPLES (every utterance fits: zv_max_frames()
// frames of a hop are fewer); `padded` holds the capacities rounded up to whole chunks
constexpr uint64_t LOUD_GROUP_SAMPLES = 1ull << 26;
ZV_LV_FN uint64_t loud_padded(uint64_t total) { return (total + LOUD_CHUNK - 1) / LOUD_CHUNK * LOUD_CHUNK; }
inline uint32_t loud_group_end(uint32_t first, uint32_t n_utt, const uint32_t *T, uint32_t hop)
{
    uint64_t sum = 0;
    uint32_t u = first;
    for (; u < n_utt; u++)
    {
        const uint64_t p = loud_padded((uint64_t)T[u] * hop);
        if (u > first && sum + p > LOUD_GROUP_SAMPLES) break;
        sum += p;
    }
    return u;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host side only: the design, the ask and the reference; a device pass sees none of it ----

// the target as a mean square, zt = 10^((target + 0.691) / 10): libm's pow, on the host, once
inline LoudAsk loud_ask(float gain, float target_lufs, float ceiling, uint32_t flags)
{
    double e = (double)target_lufs + 0.691;
    e = e / 10.0;
    return LoudAsk{(flags & LOUD_FLAG_TARGET) ? pow(10.0, e) : 0.0, gain, ceiling, flags, 0u};
}

// C = P P, every entry the chain acc <- fma(P[i][k], P[k][j], acc) over k = 0 .. 3 from +0.0: four IEEE fusedMultiplyAdd operations,
// written out (nothing is left to contraction).  The powers of A grow before they decay, so A^256 is sensitive to the order of these
// sums at 1e-11 of its largest entry; this order is the one an FMA dot-product kernel takes, ascending in k.
inline void loud_square(double *P)
{
    double C[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
        {
            double acc = 0.0;
            for (int k = 0; k < 4; k++) acc = __builtin_fma(P[4 * i + k], P[4 * k + j], acc);
            C[4 * i + j] = acc;
        }
    for (int i = 0; i < 16; i++) P[i] = C[i];
}

// The design for a sampling rate (include/zerovox_amd.h zv_loudness_design).  Returns null, else "sampling_rate".
inline const char *loud_design(uint32_t rate, LoudFilter *out)
{
    if (rate < LOUD_MIN_RATE || rate > LOUD_MAX_RATE) return "sampling_rate";
    const double fs = (double)rate;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(M_PI * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        out->shelf_b[0] = (Vh + Vb * K / Q + K * K) / a0;
        out->shelf_b[1] = 2.0 * (K * K - Vh) / a0;
        out->shelf_b[2] = (Vh - Vb * K / Q + K * K) / a0;
        out->shelf_a[0] = 2.0 * (K * K - 1.0) / a0;
        out->shelf_a[1] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(M_PI * f0 / fs);
        const double a0 = 1.0 + K / Q + K * K;
        out->highpass_b[0] = 1.0;
        out->highpass_b[1] = -2.0;
        out->highpass_b[2] = 1.0;
        out->highpass_a[0] = 2.0 * (K * K - 1.0) / a0;
        out->highpass_a[1] = (1.0 - K / Q + K * K) / a0;
    }
    out->step = (rate + 5u) / 10u;
    // A, the zero-input transition of loud_kweight on (p1, p2, q1, q2), then M = A^256: P <- P P eight times
    const double a1 = out->shelf_a[0], a2 = out->shelf_a[1], h1 = out->highpass_a[0], h2 = out->highpass_a[1];
    const double A[16] = {-a1, 1.0, 0.0, 0.0, -a2, 0.0, 0.0, 0.0, -2.0 - h1, 0.0, -h1, 1.0, 1.0 - h2, 0.0, -h2, 0.0};
    for (int i = 0; i < 16; i++) out->M[i] = A[i];
    for (int k = 0; k < 8; k++) loud_square(out->M);
    for (int j = 0; j < LOUD_TAPS; j++)
    {
        const double t = ((double)j - 24.0) / 4.0;
        const double sinc = j == 24 ? 1.0 : sin(M_PI * t) / (M_PI * t);
        const double w = 0.5 * (1.0 - cos(2.0 * M_PI * (double)j / 48.0));
        const float c = (float)(sinc * w);
        out->c[j] = fabsf(c) < 1e-6f ? 0.0f : c;
    }
    return nullptr;
}

// Host reference of the whole rule for one utterance: x[0 .. total) the waveform, N <= total the samples measured.  out (may be null:
// meter only) receives x[i] * gain for all total samples.
inline LoudRow loud_reference(const LoudFilter &F, const float *x, uint64_t N, uint64_t total, const LoudAsk &q, float *out)
{
    const int64_t nch = loud_chunks((int64_t)N), J = (int64_t)(N / F.step);
    auto xs = [&](int64_t n) { return n >= 0 && (uint64_t)n < N ? loud_sample(x[n]) : 0.0; };
    std::vector<double> st((size_t)nch * 4), runs((size_t)nch * 2 + 2, 0.0);
    for (int64_t k = 0; k < nch; k++)            // phase A
    {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < LOUD_CHUNK; i++) loud_kweight(F, s, xs(LOUD_CHUNK * k + i));
        for (int r = 0; r < 4; r++) st[4 * k + r] = s[r];
    }
    {
        double s[4] = {0.0, 0.0, 0.0, 0.0};      // phase B: st[k] becomes the entry state of chunk k
        for (int64_t k = 0; k < nch; k++)
        {
            double z[4];
            for (int r = 0; r < 4; r++) z[r] = st[4 * k + r], st[4 * k + r] = s[r];
            loud_advance(F.M, s, z);
        }
    }
    for (int64_t k = 0; k < nch; k++)            // phase C
    {
        double s[4], run[2] = {0.0, 0.0};
        for (int r = 0; r < 4; r++) s[r] = st[4 * k + r];
        const int64_t edge = loud_edge(k, F.step);
        for (int i = 0; i < LOUD_CHUNK; i++)
        {
            const int64_t n = LOUD_CHUNK * k + i;
            loud_run_add(run, loud_kweight(F, s, xs(n)), n >= edge);
        }
        runs[2 * k] = run[0];
        runs[2 * k + 1] = run[1];
    }
    std::vector<double> E((size_t)J + 1), z((size_t)J + 1);
    for (int64_t j = 0; j < J; j++) E[j] = loud_step_energy(runs.data(), j, F.step);      // phase D
    uint64_t tpb = 0;
    uint32_t spb = 0;
    for (int64_t n = 0; n < (int64_t)N + LOUD_TP_TAIL; n++)
    {
        double w[LOUD_PHASE_TAPS];
        for (int k = 0; k < LOUD_PHASE_TAPS; k++) w[k] = xs(n - k);
        for (int f = 1; f < 4; f++)
        {
            const uint64_t b = loud_dbits(fabs(loud_tp_phase(F.c, f, w)));
            tpb = b > tpb ? b : tpb;
        }
        if ((uint64_t)n < N)
        {
            const uint32_t a = level_abs_bits(x[n]);
            spb = a > spb ? a : spb;
        }
    }
    const float sp = level_from_bits(spb);
    const uint64_t sb = loud_dbits((double)sp);
    tpb = sb > tpb ? sb : tpb;
    const LoudRow r = loud_gate(E.data(), J, z.data(), F.step, mel_from_bits(tpb), sp, q);
    for (uint64_t i = 0; out && i < total; i++) out[i] = x[i] * r.gain;
    return r;
}
#endif

}  // namespace zv
