// filter.h — waveform filter (include/zerovox_amd.h "waveform filter"): a linear-phase FIR equaliser per utterance, applied to the
// vocoder's waveform ahead of the envelope, the volume controls and every meter.  Plain arithmetic shared by filter_kernel
// (filter_kernels.hip) and the host-side test (tests/native/filter_check.cpp): nothing here needs HIP.
//
// An output sample is ONE chain of f64 additions over the taps in ascending order, acc = acc + (double)h[k] * (double)x'[n + c - k].
// The product of two f32 values is exact in f64 (48 bits of significand, exponents inside the range), so every step is one IEEE
// addition whether it is written as a product and a sum or as a fused multiply-add: filter_step is the one place that writes it.  A
// chain starts at +0.0 and a product of finite factors is finite, so a chain is never -0.0, and a step whose tap is +0.0 leaves it as
// it is: the kernel pads a tap count to a multiple of its unroll with such steps.
#pragma once

#include <math.h>
#include <stdint.h>

#include "level.h"        // ZV_LV_FN, level_bits

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

namespace zv
{

constexpr uint32_t FILTER_MAX_TAPS = 511;                          // n_taps is odd, 1 .. 511
// a parameter row in HBM, uint32 [segment][FILTER_PARAM_STRIDE]: n_taps (0: this segment is copied, bit for bit), then the taps' f32 bits
constexpr int FILTER_PARAM_STRIDE = 1 + (int)FILTER_MAX_TAPS;
// outputs one workgroup of filter_kernel owns: 256 lanes, FILTER_LANE_OUTPUTS consecutive outputs each
constexpr int FILTER_LANE_OUTPUTS = 8;
constexpr int FILTER_TILE = 256 * FILTER_LANE_OUTPUTS;
// the 1 024-point DFT the design's edges are bins of (bands.h BANDS_N), and the default edges (bands.h BANDS_DEFAULT_EDGES)
constexpr int      FILTER_DFT = 1024;
constexpr uint32_t FILTER_BANDS_MAX = 64, FILTER_BANDS_DEFAULT = 16;
constexpr uint32_t FILTER_DEFAULT_EDGES[FILTER_BANDS_DEFAULT + 1] = {1, 3, 5, 8, 12, 17, 24, 33, 45, 62, 84, 114, 155, 210, 285, 387, 513};

// x'[j]: the sample where it is finite, else +0.0
ZV_LV_FN bool filter_finite(float x) { return (level_bits(x) & 0x7fffffffu) < 0x7f800000u; }
ZV_LV_FN double filter_sample(float x) { return filter_finite(x) ? (double)x : 0.0; }

// one step of a chain; the product is exact, so the fused form rounds once, where the sum of the unfused form rounds
ZV_LV_FN double filter_step(double acc, float h, double xs) { return __builtin_fma((double)h, xs, acc); }

// validation of a zv_filter: null, else the name of the field that is wrong.  taps == NULL is "no filter" whatever n_taps says.
ZV_LV_FN const char *filter_check(const float *taps, uint32_t n_taps)
{
    if (!taps) return nullptr;
    if (n_taps == 0 || n_taps > FILTER_MAX_TAPS || (n_taps & 1u) == 0) return "n_taps";
    for (uint32_t k = 0; k < n_taps; k++)
        if (!filter_finite(taps[k])) return "taps";
    return nullptr;
}

// the parameter row of a checked zv_filter (taps == NULL: the row of "no filter")
ZV_LV_FN void filter_pack(const float *taps, uint32_t n_taps, uint32_t *row)
{
    for (int i = 0; i < FILTER_PARAM_STRIDE; i++) row[i] = 0;
    if (!taps) return;
    row[0] = n_taps;
    for (uint32_t k = 0; k < n_taps; k++) row[1 + k] = level_bits(taps[k]);
}

// grid of filter_kernel over segments of at most max_rows frames: (tiles, segments)
struct FilterPlan
{
    int tiles;
};
inline FilterPlan filter_plan(int max_rows, int hop) { return FilterPlan{(int)(((long)max_rows * hop + FILTER_TILE - 1) / FILTER_TILE)}; }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host side only: the reference and the design; a device pass sees none of it ----

// Host reference of the rule for one utterance: x[0 .. S) is the span (the utterance's own samples), y[0 .. cap) receives the filtered
// span and zeros behind it (S <= cap).  taps == NULL: y = x over the whole capacity, bit for bit (x then holds cap samples).
inline void filter_reference(const float *x, uint64_t S, uint64_t cap, const float *taps, uint32_t n_taps, float *y)
{
    if (!taps)
    {
        for (uint64_t n = 0; n < cap; n++) __builtin_memcpy(&y[n], &x[n], 4);
        return;
    }
    const int64_t c = ((int64_t)n_taps - 1) / 2;
    std::vector<double> xs(S);
    for (uint64_t j = 0; j < S; j++) xs[j] = filter_sample(x[j]);
    for (uint64_t n = 0; n < S; n++)
    {
        double acc = 0.0;
        for (uint32_t k = 0; k < n_taps; k++)
        {
            const int64_t j = (int64_t)n + c - (int64_t)k;
            acc = filter_step(acc, taps[k], j >= 0 && (uint64_t)j < S ? xs[j] : 0.0);
        }
        y[n] = (float)acc;
    }
    for (uint64_t n = S; n < cap; n++) y[n] = 0.0f;
}

// The design (include/zerovox_amd.h zv_filter_design): band gains on DFT-bin edges to n_taps Hann-windowed taps, in f64, each tap
// rounded to f32 once.  Returns null, else the name of the field that is wrong ("n_bands", "edges", "gains", "n_taps").
inline const char *filter_design(uint32_t n_bands, const uint32_t *edges, const float *gains, uint32_t n_taps, float *taps)
{
    if (n_bands > FILTER_BANDS_MAX) return "n_bands";
    if (!edges && n_bands != 0 && n_bands != FILTER_BANDS_DEFAULT) return "edges";
    const uint32_t nb = n_bands ? n_bands : FILTER_BANDS_DEFAULT;
    const uint32_t *e = edges ? edges : FILTER_DEFAULT_EDGES;
    for (uint32_t b = 0; b < nb; b++)
        if (!(e[b] < e[b + 1])) return "edges";
    if (e[nb] > (uint32_t)(FILTER_DFT / 2 + 1)) return "edges";
    if (n_taps == 0 || n_taps > FILTER_MAX_TAPS || (n_taps & 1u) == 0) return "n_taps";
    for (uint32_t b = 0; b < nb; b++)
        if (!(gains[b] >= 0.0f && filter_finite(gains[b]))) return "gains";
    const int c = ((int)n_taps - 1) / 2;
    auto lp = [](double f, int m) { return m == 0 ? 2.0 * f : sin(2.0 * M_PI * f * (double)m) / (M_PI * (double)m); };
    for (int m = -c; m <= c; m++)
    {
        const double w = 0.5 + 0.5 * cos(2.0 * M_PI * (double)m / (double)(n_taps + 1));
        double h = m == 0 ? 1.0 : 0.0;
        for (uint32_t b = 0; b < nb; b++)
        {
            const double lo = (double)e[b] - 0.5, hi = (double)e[b + 1] - 0.5;
            const double f_lo = (lo > 0.0 ? lo : 0.0) / (double)FILTER_DFT, f_hi = (hi < 512.0 ? hi : 512.0) / (double)FILTER_DFT;
            h += ((double)gains[b] - 1.0) * (lp(f_hi, m) - lp(f_lo, m)) * w;
        }
        taps[m + c] = (float)h;
    }
    return nullptr;
}
#endif

}  // namespace zv
