// level.h — volume controls (include/zerovox_amd.h "volume controls"): how an utterance's level is measured, how the gain follows
// from it and from a zv_volume, and what the zv_level reports.  Plain arithmetic shared by level_measure_kernel / level_apply_kernel
// (level_kernels.hip) and the host-side test (tests/native/level_check.cpp): nothing here needs HIP.
//
// Why integers: the sum of squares is taken over 16-byte loads, lanes, waves and workgroups, and a caller must be able to restate
// the gain bit for bit.  So every sample is turned into a 1.19 fixed-point magnitude ONCE (level_quant: one exactly rounded double
// product, one exactly rounded double sum, a truncation) and the squares are added as unsigned 64-bit integers: associative, the
// same on the host, on the device and in a big-integer restatement, whatever the tiling.  The peak is a maximum of bit patterns,
// which no order changes either.  Behind the two totals every f64 step is ONE IEEE operation (a conversion, *, / or sqrt), written
// as a statement of its own; the library builds with -ffp-contract=off.
//
// dB: a caller converts, gain = 10^(dB / 20); a level in dBFS the same way (target_rms = 10^(dBFS / 20), full scale = 1.0).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZV_LV_FN __host__ __device__ static inline
#else
#define ZV_LV_FN static inline
#endif

namespace zv
{

// samples one workgroup of the two kernels covers: a multiple of 4 (16-byte loads stay aligned from chunk to chunk) and of the
// 300-sample hop of the shipped checkpoints (a chunk is 32 of their frames)
constexpr int LEVEL_CHUNK_SAMPLES = 9600;
// S = sum of q^2 with q <= 2^19: 2^38 * 32768 frames * 300 samples < 2^62 (zv_max_frames() <= 32768)
constexpr double LEVEL_Q_ONE = 524288.0;              // 2^19: q of |x| >= 1
constexpr double LEVEL_S_ONE = 274877906944.0;        // 2^38: q^2 of |x| >= 1
// a volume row in HBM, f32 [segment][LEVEL_VOL_STRIDE]: gain, target_rms, peak_ceiling, unused
constexpr int LEVEL_VOL_STRIDE = 4;

// what the apply step stores per utterance; the layout of include/zerovox_amd.h zv_level
struct LevelRow
{
    float    rms, peak, gain;
    uint32_t reserved;
};

ZV_LV_FN uint32_t level_bits(float x)
{
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    return b;
}
ZV_LV_FN float level_from_bits(uint32_t b)
{
    float x;
    __builtin_memcpy(&x, &b, 4);
    return x;
}

// |x| as its bit pattern when x is finite, else 0: the peak is the largest of these (bit patterns of non-negative floats order as
// the floats do), so NaN and +-inf are left out and -0.0 counts as 0
ZV_LV_FN uint32_t level_abs_bits(float x)
{
    const uint32_t a = level_bits(x) & 0x7fffffffu;
    return a < 0x7f800000u ? a : 0u;
}

// 1.19 fixed-point magnitude of a sample: min(|x|, 1) * 2^19 + 0.5 truncated, 0 for NaN and +-inf; 0 <= q <= 2^19
ZV_LV_FN uint32_t level_quant(float x)
{
    const uint32_t ab = level_bits(x) & 0x7fffffffu;
    if (ab >= 0x7f800000u) return 0u;
    float a = level_from_bits(ab);
    a = a < 1.0f ? a : 1.0f;
    double d = (double)a * LEVEL_Q_ONE;
    d = d + 0.5;
    return (uint32_t)d;               // d < 2^20: the truncation of the (int64) conversion
}

// the level of n samples whose squares sum to S: sqrt(S / (n * 2^38)), 0 when S == 0
ZV_LV_FN double level_rms(uint64_t S, uint64_t n)
{
    if (S == 0) return 0.0;
    double den = (double)n;
    den = den * LEVEL_S_ONE;
    double r = (double)S;
    r = r / den;
    return sqrt(r);
}

// the gain of an utterance from its totals and its zv_volume {gain, target_rms, peak_ceiling}
ZV_LV_FN float level_gain(uint64_t S, double rms, uint32_t peak_bits, float gain, float target_rms, float peak_ceiling)
{
    const float peak = level_from_bits(peak_bits);
    double gd = (double)gain;
    if (target_rms > 0.0f && S > 0)
    {
        gd = (double)target_rms / rms;
        gd = gd * (double)gain;
    }
    bool ceiling = false;
    if (peak_ceiling > 0.0f && peak > 0.0f)
    {
        const double scaled = gd * (double)peak;
        if (scaled > (double)peak_ceiling)
        {
            gd = (double)peak_ceiling / (double)peak;
            ceiling = true;
        }
    }
    float g = (float)gd;
    // the promise: no finite sample leaves above the ceiling.  (float)gd may have rounded up and g * peak rounds once more, so step
    // g towards 0 while the scaled peak still exceeds the ceiling (g > 0 here: one bit pattern down is nextafterf(g, 0))
    for (int k = 0; ceiling && k < 4; k++)
    {
        const float p = g * peak;
        if (!(p > peak_ceiling)) break;
        g = level_from_bits(level_bits(g) - 1u);
    }
    return g;
}

// the report of an utterance: level and peak before the gain, and the gain
ZV_LV_FN LevelRow level_report(uint64_t S, uint64_t n, uint32_t peak_bits, float gain, float target_rms, float peak_ceiling)
{
    const double rms = level_rms(S, n);
    LevelRow r;
    r.rms = (float)rms;
    r.peak = level_from_bits(peak_bits);
    r.gain = level_gain(S, rms, peak_bits, gain, target_rms, peak_ceiling);
    r.reserved = 0;
    return r;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// Host reference of the whole rule for one utterance: x[0 .. cap) is the waveform of its capacity, n <= cap the samples of its
// speech (nf * hop).  Measures x[0 .. n), scales all cap samples in place (out may be x, or null: measure only) and returns the
// report; S_out (may be null) receives the sum of squares.
inline LevelRow level_reference(const float *x, uint64_t n, uint64_t cap, float gain, float target_rms, float peak_ceiling, float *out,
                                uint64_t *S_out)
{
    uint64_t S = 0;
    uint32_t peak = 0;
    for (uint64_t i = 0; i < n; i++)
    {
        const uint64_t q = level_quant(x[i]);
        S += q * q;
        const uint32_t a = level_abs_bits(x[i]);
        peak = a > peak ? a : peak;
    }
    const LevelRow r = level_report(S, n, peak, gain, target_rms, peak_ceiling);
    for (uint64_t i = 0; out && i < cap; i++) out[i] = x[i] * r.gain;
    if (S_out) *S_out = S;
    return r;
}
#endif

}  // namespace zv
