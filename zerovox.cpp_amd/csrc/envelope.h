// envelope.h — amplitude envelope (include/zerovox_amd.h "amplitude envelope"): how the per-phoneme gains, the cross-fade half-width and
// the two fades of a zv_envelope become one gain per sample.  Plain arithmetic shared by env_knots_kernel / env_apply_kernel
// (envelope_kernels.hip) and the host-side test (tests/native/envelope_check.cpp): nothing here needs HIP.
//
// Why integers: a frame's gain is a 16.16 fixed-point number, a window sum adds 2r + 1 of them and a knot adds two window sums, so the
// table the apply pass interpolates in is the same however the knots pass splits its work, on the host, on the device and in a
// big-integer restatement.  Behind the knots every f64 step is ONE IEEE operation (a conversion, * or /), written as a statement of its
// own; the library builds with -ffp-contract=off.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZV_ENV_FN __host__ __device__ static inline
#else
#define ZV_ENV_FN static inline
#endif

namespace zv
{

constexpr uint32_t ENV_ONE = 65536;              // the fixed-point gain 1
constexpr int      ENV_MAX_RAMP = 64;            // ramp_frames <= 64: a knot is at most 2 * 129 * 2^20 < 2^29
constexpr float    ENV_MAX_GAIN = 16.0f;
// an envelope row in HBM, int32 [segment][ENV_CTL_STRIDE]: ramp_frames, fade_in_samples, fade_out_samples, unused
constexpr int ENV_CTL_STRIDE = 4;

// 16.16 fixed-point gain of a phoneme: gain * 65536 + 0.5 truncated; 0 <= G <= 2^20 for 0 <= gain <= 16
ZV_ENV_FN uint32_t env_fixed_gain(float gain)
{
    double d = (double)gain * 65536.0;
    d = d + 0.5;
    return (uint32_t)(int64_t)d;
}

// the phoneme that owns frame f: the first token i of n with cum[i] > f (cum: the length regulator's inclusive scan); n when there is none
ZV_ENV_FN int env_owner(const int32_t *cum, int n, int f)
{
    int lo = 0, hi = n;
    while (lo < hi)
    {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > f) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// F[f] of an utterance with nf > 0 speech frames, edge-replicated outside [0, nf); gain: f32 [n] or null (all 1)
ZV_ENV_FN uint32_t env_frame_gain(const int32_t *cum, const float *gain, int n, int nf, int f)
{
    f = f < 0 ? 0 : (f < nf ? f : nf - 1);
    const int i = env_owner(cum, n, f);
    return gain && i < n ? env_fixed_gain(gain[i]) : ENV_ONE;
}

// den = 2 * W * hop * 65536 with W = 2r + 1
ZV_ENV_FN int64_t env_den(int r, int hop) { return (int64_t)2 * (2 * r + 1) * hop * 65536; }

// The gain of sample s = f * hop + j of an utterance of n = nf * hop speech samples, nf > 0, from the knots at the frame's two ends
// (b0 = B[min(f, nf)], b1 = B[min(f + 1, nf)]: behind the speech both are the last knot) and the fades.
ZV_ENV_FN float env_sample_gain(uint32_t b0, uint32_t b1, int hop, int j, int64_t den, int64_t s, int64_t n, uint32_t Fi, uint32_t Fo)
{
    const int64_t num = (int64_t)b0 * (hop - j) + (int64_t)b1 * j;
    const double dn = (double)num, dd = (double)den;
    double d = dn / dd;
    if (Fi > 0 && s < (int64_t)Fi)
    {
        const double ts = (double)s, tf = (double)Fi;
        const double t = ts / tf;
        d = d * t;
    }
    if (Fo > 0 && n - 1 - s < (int64_t)Fo)
    {
        const int64_t k = n - 1 - s;
        const double tk = (double)(k > 0 ? k : 0), tf = (double)Fo;
        const double t = tk / tf;
        d = d * t;
    }
    return (float)d;
}

// an utterance without speech (nf == 0) has no knots: every sample keeps its bits without a fade-out and is silenced with one
ZV_ENV_FN float env_empty_gain(uint32_t Fo) { return Fo > 0 ? 0.0f : 1.0f; }

#if !defined(__HIP_DEVICE_COMPILE__)
// Host reference, the knots of one utterance: B[0 .. nf] from the scan cum [n], the gains (f32 [n] or null) and r; nf > 0
inline void envelope_knots_reference(const int32_t *cum, const float *gain, int n, int nf, int r, uint32_t *B)
{
    for (int f = 0; f <= nf; f++)
    {
        uint32_t b = 0;
        for (int j = f - 1 - r; j <= f - 1 + r; j++) b += env_frame_gain(cum, gain, n, nf, j);
        for (int j = f - r; j <= f + r; j++) b += env_frame_gain(cum, gain, n, nf, j);
        B[f] = b;
    }
}

// Host reference of the whole rule for one utterance: x[0 .. T * hop) is the waveform of its capacity, cum [n] the regulator's scan
// (the timings are min(cum_i, T) - min(cum_{i-1}, T)), nf = min(n_frames, T).  Scales all T * hop samples (out may be x) and stores the
// knots into B (nf + 1 entries, may be null).
inline void envelope_reference(const float *x, int T, int hop, const int32_t *cum, int n, int nf, const float *gain, int r, uint32_t Fi,
                               uint32_t Fo, float *out, uint32_t *B)
{
    const int64_t total = (int64_t)T * hop, ns = (int64_t)nf * hop, den = env_den(r, hop);
    uint32_t *knots = nf > 0 ? new uint32_t[(size_t)nf + 1] : nullptr;
    if (nf > 0) envelope_knots_reference(cum, gain, n, nf, r, knots);
    for (int64_t s = 0; s < total; s++)
    {
        float e = env_empty_gain(Fo);
        if (nf > 0)
        {
            const int64_t f = s / hop;
            const int j = (int)(s - f * hop);
            e = env_sample_gain(knots[f < nf ? f : nf], knots[f + 1 < nf ? f + 1 : nf], hop, j, den, s, ns, Fi, Fo);
        }
        out[s] = x[s] * e;
    }
    for (int f = 0; B && f <= nf && nf > 0; f++) B[f] = knots[f];
    delete[] knots;
}
#endif

}  // namespace zv
