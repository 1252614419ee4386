// fit_durations.h — target durations (include/zerovox_amd.h "target durations"): the integer rule that turns an utterance's predicted
// durations and a target frame count into per-phoneme frame counts that sum to the target exactly.  Plain arithmetic shared by
// fit_durations_kernel (regulator_kernels.hip) and the host-side test (tests/native/fit_durations_check.cpp): nothing here needs HIP.
//
// Why integers: the shares must sum to the target whatever order a workgroup adds them in, and a caller must be able to restate
// them bit for bit.  So the f32 duration is turned into a 16.16 fixed-point weight ONCE (fit_weight, one exactly rounded double
// product and a truncation) and everything behind it — the weights' sum, the shares, the remainders, the ranks — is 64-bit
// integer arithmetic: associative, and the same on the host, on the device and in a big-integer restatement.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define ZV_FD_FN __host__ __device__ static inline
#else
#define ZV_FD_FN static inline
#endif

namespace zv
{

// the largest weight, 2^40: q * R < 2^55 for R <= 32768 frames and the sum of 1 501 weights stays below 2^51
constexpr int64_t FIT_WEIGHT_MAX = (int64_t)1 << 40;

// weight of a free phoneme from its (scaled) f32 duration: dur * 65536 truncated, capped at 2^40; NaN and dur <= 0 give 0, +inf 2^40
ZV_FD_FN int64_t fit_weight(float dur)
{
    if (!(dur > 0.0f)) return 0;
    const double w = (double)dur * 65536.0;
    return w >= (double)FIT_WEIGHT_MAX ? FIT_WEIGHT_MAX : (int64_t)w;
}

// a free phoneme's share of the R frames the forced phonemes leave: floor(q * R / Q), and what the floor dropped (0 <= rem < Q)
ZV_FD_FN int64_t fit_share(int64_t q, int64_t R, int64_t Q) { return q * R / Q; }
ZV_FD_FN int64_t fit_remainder(int64_t q, int64_t R, int64_t Q) { return q * R % Q; }

// largest remainder first, ties to the lower index: does free phoneme j come before free phoneme i?  The L = R - sum of shares
// free phonemes that fewer than L others come before get one frame more.
ZV_FD_FN bool fit_before(int64_t rem_j, int j, int64_t rem_i, int i) { return rem_j > rem_i || (rem_j == rem_i && j < i); }

#if !defined(__HIP_DEVICE_COMPILE__)
// Host reference of the whole rule for one utterance of n tokens whose first num_phonemes the length regulator walks:
//   dur[i]     the f32 duration after the utterance's and the phoneme's scale (steps 1-3 of the header's duration rule)
//   forced[i]  duration_frames[i] (>= 0: forced, < 0: free), or forced == NULL: every phoneme is free
//   T          the frame capacity, target the frames to hit (0 < target <= T; target <= 0 leaves nothing for the free phonemes)
//   d[i]       out: the frames of every token; tokens at or past num_phonemes get 0
inline void fit_durations(const float *dur, const int32_t *forced, int n, int num_phonemes, int T, int target, int32_t *d)
{
    const int nw = num_phonemes < n ? (num_phonemes < 0 ? 0 : num_phonemes) : n;
    int64_t Fs = 0, Q = 0;
    int n_free = 0;
    for (int i = 0; i < n; i++) d[i] = 0;
    for (int i = 0; i < nw; i++)
    {
        if (forced && forced[i] >= 0)
        {
            d[i] = forced[i] < T ? forced[i] : T;
            Fs += d[i];
            continue;
        }
        Q += fit_weight(dur[i]);
        n_free++;
    }
    const int64_t R = (int64_t)target - Fs;
    if (R <= 0 || n_free == 0) return;              // forced durations win: every free phoneme keeps 0
    const bool equal = Q == 0;                      // no weight at all: equal shares
    if (equal) Q = n_free;
    auto free_at = [&](int i) { return !(forced && forced[i] >= 0); };
    auto weight = [&](int i) { return equal ? (int64_t)1 : fit_weight(dur[i]); };
    int64_t L = R;
    for (int i = 0; i < nw; i++)
        if (free_at(i))
        {
            d[i] = (int32_t)fit_share(weight(i), R, Q);
            L -= d[i];
        }
    for (int i = 0; i < nw && L > 0; i++)
    {
        if (!free_at(i)) continue;
        const int64_t rem_i = fit_remainder(weight(i), R, Q);
        int64_t before = 0;
        for (int j = 0; j < nw; j++)
            if (free_at(j) && fit_before(fit_remainder(weight(j), R, Q), j, rem_i, i)) before++;
        if (before < L) d[i]++;
    }
}
#endif

}  // namespace zv
