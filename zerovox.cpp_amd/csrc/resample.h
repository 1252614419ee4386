// resample.h — sample-rate conversion and PCM16 delivery (include/zerovox_amd.h "resampling"): the step behind the limiter in a delivery
// chain, and the way in for a recording at another rate.  Plain arithmetic shared by the kernels (resample_kernels.hip), the C-ABI
// (capi.cpp) and the host-side test (tests/native/resample_check.cpp): nothing here needs HIP.
//
// THE RULE is a rational polyphase FIR; nothing in it is recursive along time, so no result depends on how the work is split.
//   g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g; the table h[L][P] is f32, P even, half = P / 2; x[0 .. S_in) the input
//   count    n_out = floor((S_in L + M - 1) / M) in 64-bit integers: the outputs whose time n M / L lies inside [0, S_in)
//   span     x'[j] = x[j] where 0 <= j < S_in and the sample is finite, else +0.0 (the waveform filter's span rule)
//   sample   t = n M (64 bit), i0 = t div L, p = t mod L; acc = +0.0 (f64); for k = 0 .. P - 1 ascending:
//            acc = acc + (double)h[p][k] * (double)x'[i0 - half + 1 + k]; y[n] = (float)acc.  The product of two f32 values is exact in
//            f64, so a step is ONE IEEE addition whether or not it is fused.  Output n sits at input time n M / L: no delay.
//   PCM16    z = (double)y[n] * 32768; with dither (flag bit 0) z = z + d, d = ((double)((r & 0xFFFF) + (r >> 16)) - 65535) * 2^-16 for
//            the hash r of seed and n below (TPDF, zero mean, +-1 LSB); z = z + 0.5; q = floor(z) clamped to [-32768, 32767]; a NaN
//            gives 0; `clipped` counts the clamped and the NaN samples
//   report   n_out; clipped (0 where no PCM16 is asked for); sample_peak: the largest finite |y[n]| as a maximum of bit patterns
// The design (resample_design, host only) is data to the rule: a Kaiser-windowed sinc, every phase row divided by its own sum.
#pragma once

#include "loudness.h"     // loud_padded, LOUD_GROUP_SAMPLES, loud_finite, loud_sample; level.h's bit patterns

#if !defined(__HIP_DEVICE_COMPILE__)
#include <cmath>
#include <vector>
#endif

namespace zv
{

constexpr uint32_t RESAMPLE_MIN_RATE = 4000, RESAMPLE_MAX_RATE = 768000;
constexpr uint32_t RESAMPLE_MAX_L = 1280;                      // L and M alike
constexpr uint32_t RESAMPLE_MAX_RATIO = 8;                     // max(L / M, M / L)
constexpr uint32_t RESAMPLE_MAX_P = 512, RESAMPLE_MAX_TABLE = 65536;      // taps per phase; L * P
constexpr uint32_t RESAMPLE_MIN_ZEROS = 4, RESAMPLE_MAX_ZEROS = 64, RESAMPLE_ZEROS = 32;
constexpr double   RESAMPLE_BETA = 9.0, RESAMPLE_MAX_BETA = 20.0, RESAMPLE_CUTOFF = 0.91;
constexpr uint32_t RESAMPLE_FLAG_DITHER = 1u;
constexpr int      RESAMPLE_THREADS = 256;
constexpr int      RESAMPLE_SLOTS = 512;                       // a tile's slots: the largest multiple of L up to here (L itself beyond)
constexpr int      RESAMPLE_MAX_R = 8;                         // outputs of one phase a slot owns at the most
constexpr int      RESAMPLE_STAGE = 8000;                      // input samples a workgroup stages at the most (f64: 64 000 bytes of LDS)

// The deal (resample_kernels.hip).  A tile is R * S consecutive outputs, S = L * max(1, 512 div L) slots.  Slot s owns the R outputs
// n0 + s + r S: S is a multiple of L, so they share ONE phase and their input bases lie D = S M / L = M * max(1, 512 div L) apart.  R is
// the largest of 8, 4, 2, 1 whose tile stages at most RESAMPLE_STAGE samples at the worst first remainder; R = 1 always fits
// (S M / L <= 4 096 for L <= 512, <= 1 280 beyond).
struct ResampleTile
{
    int S, D, R;
};
ZV_LV_FN int resample_tile_outputs(const ResampleTile &t) { return t.R * t.S; }
ZV_LV_FN int resample_tile_stage(uint32_t L, uint32_t M, uint32_t P, int S, int R)
{
    return (int)((L - 1u + (uint32_t)(R * S - 1) * M) / L) + (int)P;
}
ZV_LV_FN ResampleTile resample_tile(uint32_t L, uint32_t M, uint32_t P)
{
    const int k = (int)L <= RESAMPLE_SLOTS ? RESAMPLE_SLOTS / (int)L : 1;
    ResampleTile t{(int)L * k, (int)M * k, RESAMPLE_MAX_R};
    while (t.R > 1 && resample_tile_stage(L, M, P, t.S, t.R) > RESAMPLE_STAGE) t.R >>= 1;
    return t;
}

// What one utterance gets; the layout of include/zerovox_amd.h zv_resample_result.
struct ResampleRow
{
    uint64_t n_out, clipped;
    float    sample_peak;
};

// One utterance of a launch group, as the kernels find it.
struct ResampleSeg
{
    int64_t  x0, S_in;      // first sample in the wav array (a multiple of 4) and the samples there
    int64_t  y0, n_out;     // first sample in the out and pcm arrays (a multiple of 8) and the samples there
    int32_t  tile0;         // first entry of the statistics: tiles of resample_tile_outputs(resample_tile(L, M, P)) outputs
    uint32_t seed;          // the dither's seed for this utterance: the ask's + u
};

// One launch group as the kernels take it (kernels.h launch_resample*).
struct ResampleJob
{
    const float *wav;              // the inputs, utterance u at segs[u].x0
    float *out;                    // the f32 outputs at segs[u].y0, or null
    int16_t *pcm;                  // the PCM16 outputs at segs[u].y0, or null
    const float *table;            // h[L][P], 8-byte aligned
    uint32_t *stats;               // [tile][2]: a tile's sample peak (bits) and its clip count
    ResampleRow *rows;             // [utterance]
    const ResampleSeg *segs;
    int nseg;
    uint32_t L, M, P, flags;
    int64_t max_n_out;             // the longest output of the group
};

// 0 where M is 0; saturates at 2^64 - 1 where S_in L + M - 1 does not fit 64 bits (S_in above about 2^64 / L)
ZV_LV_FN uint64_t resample_count(uint64_t S_in, uint32_t L, uint32_t M)
{
    if (!M) return 0;
    if (L && S_in > (~(uint64_t)0 - (M - 1u)) / L) return ~(uint64_t)0;
    return (S_in * L + M - 1) / M;
}
ZV_LV_FN int64_t resample_tiles(int64_t n, int tile) { return (n + tile - 1) / tile; }
ZV_LV_FN uint32_t resample_gcd(uint32_t a, uint32_t b)
{
    while (b)
    {
        const uint32_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// the limits of a table's shape: null, else the name of what is wrong
ZV_LV_FN const char *resample_check_shape(uint32_t L, uint32_t M, uint32_t P)
{
    if (L < 1u || L > RESAMPLE_MAX_L) return "L";
    if (M < 1u || M > RESAMPLE_MAX_L) return "M";
    if (L > RESAMPLE_MAX_RATIO * M || M > RESAMPLE_MAX_RATIO * L) return "ratio";
    if (P < 2u || P > RESAMPLE_MAX_P || (P & 1u)) return "P";
    if (L * P > RESAMPLE_MAX_TABLE) return "table size";
    return nullptr;
}
// a caller's table: the shape, gcd(L, M) = 1, finite entries
ZV_LV_FN const char *resample_check_table(const float *table, uint32_t L, uint32_t M, uint32_t P)
{
    if (const char *f = resample_check_shape(L, M, P)) return f;
    if (resample_gcd(L, M) != 1u) return "gcd";
    for (uint32_t i = 0; i < L * P; i++)
        if (!loud_finite(table[i])) return "table";
    return nullptr;
}

// PCM16: the dither of output n under a seed
ZV_LV_FN double resample_dither(uint32_t seed, uint64_t n)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    uint32_t r = seed + (uint32_t)n * 0x9E3779B9u;
    r ^= r >> 16;
    r *= 0x7feb352du;
    r ^= r >> 15;
    r *= 0x846ca68bu;
    r ^= r >> 16;
    double d = (double)((r & 0xFFFFu) + (r >> 16));
    d = d - 65535.0;
    return d * 0.0000152587890625;      // 2^-16
}
// PCM16 of one output; *clip is raised where the sample is clamped or a NaN
ZV_LV_FN int16_t resample_pcm(float y, uint32_t flags, uint32_t seed, uint64_t n, uint32_t *clip)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double z = (double)y * 32768.0;
    if (flags & RESAMPLE_FLAG_DITHER)
    {
        const double d = resample_dither(seed, n);
        z = z + d;
    }
    z = z + 0.5;
    if (z != z)
    {
        *clip += 1u;
        return 0;
    }
    const double q = __builtin_floor(z);
    if (q > 32767.0)
    {
        *clip += 1u;
        return 32767;
    }
    if (q < -32768.0)
    {
        *clip += 1u;
        return -32768;
    }
    return (int16_t)(int32_t)q;
}

// launch groups: consecutive utterances whose padded input plus output samples stay within LOUD_GROUP_SAMPLES, 65 535 at the most (an
// utterance alone is a group whatever its size)
ZV_LV_FN uint64_t resample_padded(uint64_t S_in, uint32_t L, uint32_t M) { return loud_padded(S_in) + loud_padded(resample_count(S_in, L, M)); }
inline uint32_t resample_group_end(uint32_t first, uint32_t n_utt, const uint64_t *S_in, uint32_t L, uint32_t M)
{
    uint64_t sum = 0;
    uint32_t u = first;
    for (; u < n_utt && u - first < 65535u; u++)
    {
        const uint64_t p = resample_padded(S_in[u], L, M);
        if (u > first && sum + p > LOUD_GROUP_SAMPLES) break;
        sum += p;
    }
    return u;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host side only: the design and the reference ----

// the modified Bessel function I0 as its power series, summed until a term falls below 1e-17 of the sum
inline double resample_i0(double v)
{
    const double h = v / 2.0;
    double t = 1.0, sum = 1.0;
    for (int j = 1; j < 1000; j++)
    {
        t = t * (h / (double)j);
        const double term = t * t;
        sum = sum + term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

// zv_resample_design: 0 means the default (zeros 32, beta 9, cutoff 0.91).  Returns null, else the name of what is wrong.  table == null:
// the sizes only.
inline const char *resample_design(uint32_t rate_in, uint32_t rate_out, uint32_t zeros, float beta_, float cutoff_, uint32_t *L_, uint32_t *M_,
                                   uint32_t *P_, float *table)
{
    if (rate_in < RESAMPLE_MIN_RATE || rate_in > RESAMPLE_MAX_RATE) return "rate_in";
    if (rate_out < RESAMPLE_MIN_RATE || rate_out > RESAMPLE_MAX_RATE) return "rate_out";
    const uint32_t g = resample_gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g;
    if (L > RESAMPLE_MAX_L) return "L";
    if (M > RESAMPLE_MAX_L) return "M";
    if (L > RESAMPLE_MAX_RATIO * M || M > RESAMPLE_MAX_RATIO * L) return "ratio";
    if (zeros == 0u) zeros = RESAMPLE_ZEROS;
    if (zeros < RESAMPLE_MIN_ZEROS || zeros > RESAMPLE_MAX_ZEROS) return "zeros";
    if (!loud_finite(beta_) || !(beta_ >= 0.0f && beta_ <= (float)RESAMPLE_MAX_BETA)) return "beta";
    if (!loud_finite(cutoff_) || !(cutoff_ >= 0.0f && cutoff_ <= 1.0f)) return "cutoff";
    const double beta = beta_ == 0.0f ? RESAMPLE_BETA : (double)beta_, cutoff = cutoff_ == 0.0f ? RESAMPLE_CUTOFF : (double)cutoff_;
    const uint32_t half = M > L ? (zeros * M + L - 1) / L : zeros, P = 2 * half;
    if (P > RESAMPLE_MAX_P) return "P";
    if (L * P > RESAMPLE_MAX_TABLE) return "table size";
    *L_ = L;
    *M_ = M;
    *P_ = P;
    if (!table) return nullptr;
    const double sc = (M > L ? (double)L / (double)M : 1.0) * cutoff, i0b = resample_i0(beta);
    std::vector<double> row(P);
    for (uint32_t p = 0; p < L; p++)
    {
        double sum = 0.0;
        for (uint32_t k = 0; k < P; k++)
        {
            const double d = (double)(((int64_t)k - (int64_t)half + 1) * (int64_t)L - (int64_t)p) / (double)L;
            const double r = d / (double)half, v = sc * d;
            double w = 1.0 - r * r;
            w = w > 0.0 ? w : 0.0;
            const double sinc = v == 0.0 ? 1.0 : sin(M_PI * v) / (M_PI * v);
            row[k] = fabs(d) > (double)half ? 0.0 : sc * sinc * (resample_i0(beta * sqrt(w)) / i0b);
            sum = sum + row[k];
        }
        for (uint32_t k = 0; k < P; k++) table[(size_t)p * P + k] = (float)(row[k] / sum);
    }
    return nullptr;
}

// Host reference of the whole rule for one utterance: out and pcm hold n_out samples each, either may be null.
inline ResampleRow resample_reference(const float *table, uint32_t L, uint32_t M, uint32_t P, const float *x, uint64_t S_in, uint32_t flags,
                                      uint32_t seed, float *out, int16_t *pcm)
{
    const int64_t S = (int64_t)S_in, half = P / 2;
    ResampleRow r{resample_count(S_in, L, M), 0, 0.0f};
    uint32_t peak = 0;
    for (uint64_t n = 0; n < r.n_out; n++)
    {
        const uint64_t t = n * M;
        const int64_t i0 = (int64_t)(t / L);
        const float *row = table + (size_t)(t % L) * P;
        double acc = 0.0;
        for (int64_t k = 0; k < (int64_t)P; k++)
        {
            const int64_t j = i0 - half + 1 + k;
            acc = __builtin_fma((double)row[k], j >= 0 && j < S ? loud_sample(x[j]) : 0.0, acc);
        }
        const float y = (float)acc;
        const uint32_t a = level_abs_bits(y);
        peak = a > peak ? a : peak;
        if (out) out[n] = y;
        if (pcm)
        {
            uint32_t clip = 0;
            pcm[n] = resample_pcm(y, flags, seed, n, &clip);
            r.clipped += clip;
        }
    }
    r.sample_peak = level_from_bits(peak);
    return r;
}
#endif

}  // namespace zv
