// limiter.h — the look-ahead peak limiter (include/zerovox_amd.h "limiter"): the stage behind loudness in a delivery chain.  One gain
// meets a LUFS target OR a dBTP ceiling; the limiter takes the gain the target asked for and pulls down only the samples around a peak.
// Plain arithmetic shared by the kernels (limiter_kernels.hip), the C-ABI (capi.cpp) and the host-side test
// (tests/native/limiter_check.cpp): nothing here needs HIP.
//
// THE RULE has nothing recursive along time, and everything behind the required gain is integer:
//   1. p_m   the peak of the interval [m, m + 1) on the 4x grid: max(|x'_m|, |v_1(m + 6)|, |v_2(m + 6)|, |v_3(m + 6)|), v_f loudness.h's
//            interpolated phases (loud_tp_phase), whose delay is 6 samples; 0 outside m in [-6, N + 4]
//   2. q_m   the gain sample m needs, 2.30 fixed point: ONE where gain * p_m <= ceiling, else floor((ceiling / (gain * p_m)) * 2^30)
//   3. m_k   min q_j, j in [k - release, k + attack]
//   4. s_n   floor((sum of m_k, k in [n - attack, n + release]) / W), W = attack + release + 1, in 64-bit integers
//   5. out_n = (float)(((double)wav_n * (double)gain) * ((double)s_n * 2^-30))
// Every window of step 3 that enters the sum of step 4 contains n, so every m_k of the sum is <= q_n and so is their mean: s_n <= q_n.
// The sum of W values changes by one entering and one leaving value per sample, and m_k is constant for W samples around an isolated
// peak, so s_n falls to the peak's q over `attack` samples and rises over `release` samples in straight ramps.
//
// THE PROMISE: every finite |out_n|, n in [0, N), is at most `ceiling`.  Let y = fl(|wav_n| * gain) and a = fl(gain * p_n); p_n >= |x'_n|
// = |wav_n| and rounding is monotonic, so y <= a.  Where a <= ceiling, s_n <= ONE gives |product| <= y <= ceiling.  Otherwise
// s_n 2^-30 <= q_n 2^-30 <= fl(ceiling / a) <= (ceiling / a)(1 + 2^-53) (the scalings by 2^30 and 2^-30 are exact, s_n 2^-30 has at most
// 31 bits), so fl(y * s_n 2^-30) <= ceiling (1 + 2^-53)^2: the f64 product passes the ceiling by at most a unit or so of 2^-52
// relative.  `ceiling` is an f32 value and its upper neighbour lies 2^-23 relative above it, so the rounding to f32 returns at most
// `ceiling`.  true_peak_after <= ceiling is NOT promised: a gain that varies in time moves the peaks between the samples a little.
//
// Every f64 step is ONE IEEE operation; the library and the checks build with -ffp-contract=off and the functions carry the pragma.
#pragma once

#include "loudness.h"     // LoudFilter (the interpolator), loud_tp_phase, loud_sample, loud_dbtp, loud_group_end

#if !defined(__HIP_DEVICE_COMPILE__)
#include <deque>
#include <vector>
#endif

namespace zv
{

constexpr uint32_t LIMIT_ONE = 1u << 30;                       // gain 1 in 2.30 fixed point
constexpr int      LIMIT_DELAY = 6;                            // the interpolator's delay in samples
constexpr int      LIMIT_HEAD = 5;                             // v(m + 6) reads x'[m - 5 .. m + 6]
constexpr uint32_t LIMIT_MAX_ATTACK = 2047, LIMIT_MAX_RELEASE = 6144;      // W = attack + release + 1 <= 8 192
constexpr int      LIMIT_MAX_HALO = (int)(LIMIT_MAX_ATTACK + LIMIT_MAX_RELEASE);
constexpr int      LIMIT_PAD = 4;                              // q runs LIMIT_PAD entries past the windows' reach on either side: 2 + 4 >= 6, so every p_m has an entry
constexpr int      LIMIT_TILE = 2048;                          // outputs one workgroup of the peak, minimum and mean passes covers
constexpr int      LIMIT_THREADS = 256;
constexpr uint64_t LIMIT_TWO30_BITS = 0x41d0000000000000ull;   // 2^30
constexpr uint64_t LIMIT_TWOM30_BITS = 0x3e10000000000000ull;  // 2^-30

// What one utterance asks for, as the kernels read it (capi.cpp packs it from a zv_limiter).
struct LimitAsk
{
    float    gain, ceiling;
    uint32_t attack, release;
};

// What one utterance gets; the layout of include/zerovox_amd.h zv_limit_result.
struct LimitRow
{
    double   true_peak_before, true_peak_after;
    uint64_t limited_samples;
    float    sample_peak_before, sample_peak_after;
    float    min_gain;
    float    true_peak_before_dbtp, true_peak_after_dbtp, reduction_db;
};

// One utterance of a launch group, as the kernels find it.  With H = attack + release and G = H + LIMIT_PAD the array q holds q_j, j in
// [-G, total + G), at q0 + G + j (the pad makes G >= 6, so the peak pass meets every m in [-6, N + 4] whatever the windows), and the
// array m holds m_k, k in [-attack, total + release), at m0 + attack + k, so that
//   m[i] = min q[i + LIMIT_PAD .. i + LIMIT_PAD + H]   and   s_n = floor(sum m[n .. n + H] / W):
// both passes read a window that starts at their own index (plus the pad, which keeps 16-byte loads aligned).
struct LimitSeg
{
    int64_t x0;            // first sample in the wav and out arrays (a multiple of LOUD_CHUNK)
    int64_t N;             // samples measured: min(n_frames, T) * hop
    int64_t total;         // samples limited: T * hop
    int64_t q0, m0;        // first entries of q (a multiple of LIMIT_TILE) and m (a multiple of 4)
    int32_t tile0;         // first entry of the two peak slabs: tiles of LIMIT_TILE entries of q
    int32_t stat0;         // first entry of the statistics: tiles of LIMIT_TILE samples
};

ZV_LV_FN int64_t limit_halo(const LimitAsk &a) { return (int64_t)a.attack + a.release; }
ZV_LV_FN int64_t limit_qlen(int64_t total, int64_t halo) { return total + 2 * (halo + LIMIT_PAD); }
ZV_LV_FN int64_t limit_mlen(int64_t total, int64_t halo) { return total + halo; }
ZV_LV_FN int64_t limit_tiles(int64_t n) { return (n + LIMIT_TILE - 1) / LIMIT_TILE; }
// entries a workgroup of the minimum and mean passes stages at the group's largest halo, rounded up to 4
ZV_LV_FN int limit_stage(int max_halo) { return (LIMIT_TILE + max_halo + 3) / 4 * 4; }

// step 2: the gain a sample of peak p needs
ZV_LV_FN uint32_t limit_q(float gain, float ceiling, double p)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(p > 0.0)) return LIMIT_ONE;
    const double a = (double)gain * p;
    if (a <= (double)ceiling) return LIMIT_ONE;
    double r = (double)ceiling / a;
    r = r * mel_from_bits(LIMIT_TWO30_BITS);
    return (uint32_t)r;            // 0 <= r <= 2^30: the conversion truncates, which is the floor
}

// step 5
ZV_LV_FN float limit_apply(float x, float gain, uint32_t s)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double y = (double)x * (double)gain;
    const double g = (double)s * mel_from_bits(LIMIT_TWOM30_BITS);
    y = y * g;
    return (float)y;
}

// step 6 from the maxima (bit patterns of non-negative values), the smallest s_n and the count
ZV_LV_FN LimitRow limit_finish(uint64_t tp_before, uint32_t sp_before, uint64_t tp_after, uint32_t sp_after, uint32_t min_s, uint64_t limited)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    LimitRow r;
    r.true_peak_before = mel_from_bits(tp_before);
    r.true_peak_after = mel_from_bits(tp_after);
    r.limited_samples = limited;
    r.sample_peak_before = level_from_bits(sp_before);
    r.sample_peak_after = level_from_bits(sp_after);
    const double g = (double)min_s * mel_from_bits(LIMIT_TWOM30_BITS);
    r.min_gain = (float)g;
    r.true_peak_before_dbtp = loud_dbtp(r.true_peak_before);
    r.true_peak_after_dbtp = loud_dbtp(r.true_peak_after);
    r.reduction_db = loud_dbtp(g);
    return r;
}

// validation of a zv_limiter: null, else the name of the field that is wrong
ZV_LV_FN const char *limit_check(float gain, float ceiling, uint32_t attack, uint32_t release, uint32_t flags)
{
    if (!loud_finite(gain) || !(gain >= 0.0f && gain <= 1000.0f)) return "gain";
    if (!loud_finite(ceiling) || !(ceiling > 0.0f && ceiling <= 1.0f)) return "ceiling";
    if (attack < 1u || attack > LIMIT_MAX_ATTACK) return "attack";
    if (release < 1u || release > LIMIT_MAX_RELEASE) return "release";
    if (flags) return "flags";
    return nullptr;
}

// milliseconds at a rate as a sample count: floor(ms * rate / 1000 + 0.5), brought into [1, most]
ZV_LV_FN uint32_t limit_count(double ms, uint32_t rate, uint32_t most)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double v = ms * (double)rate;
    v = v / 1000.0;
    v = v + 0.5;
    if (!(v >= 1.0)) return 1u;
    if (v >= (double)most) return most;
    return (uint32_t)v;
}
// zv_limit_design: 0 ms means the default (1.5 ms and 60 ms).  Returns null, else the name of the argument that is wrong.
constexpr double LIMIT_ATTACK_MS = 1.5, LIMIT_RELEASE_MS = 60.0;
ZV_LV_FN const char *limit_design(uint32_t rate, float attack_ms, float release_ms, uint32_t *attack, uint32_t *release)
{
    if (rate < LOUD_MIN_RATE || rate > LOUD_MAX_RATE) return "sampling_rate";
    if (!loud_finite(attack_ms) || attack_ms < 0.0f) return "attack_ms";
    if (!loud_finite(release_ms) || release_ms < 0.0f) return "release_ms";
    *attack = limit_count(attack_ms == 0.0f ? LIMIT_ATTACK_MS : (double)attack_ms, rate, LIMIT_MAX_ATTACK);
    *release = limit_count(release_ms == 0.0f ? LIMIT_RELEASE_MS : (double)release_ms, rate, LIMIT_MAX_RELEASE);
    return nullptr;
}

// One launch group as the kernels take it (kernels.h launch_limit_*): every array holds the group's utterances one behind the other, at
// the offsets of their LimitSeg.
struct LimitJob
{
    const float *wav;              // the samples, utterance u at segs[u].x0
    float *out;                    // the limited samples, at the same offsets
    uint32_t *q, *m;               // steps 2 and 3 per sample (LimitSeg)
    uint64_t *peaks_before, *peaks_after;      // [tile][2]: a peak pass's maxima per workgroup: f64 bits of p, f32 bits of the sample peak
    uint32_t *stats;               // [tile][2]: the mean pass's smallest s_n and its count of s_n < ONE over n < N
    LimitRow *rows;                // [utterance]
    const LimitSeg *segs;
    const LimitAsk *asks;
    const LoudFilter *filter;      // the model's design, in device memory: the interpolator is loudness's
    int nseg;
    int max_halo;                  // the largest attack + release of the group: sizes the LDS of the minimum and mean passes
    int64_t max_qlen, max_total;   // the longest q and the longest capacity of the group, in samples
};

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host side only: the reference ----

// step 1 over x[0 .. N): the maxima (true peak as f64 bits, sample peak as f32 bits); p (may be null) receives p_m, m = -6 .. N + 4, at m + 6
inline void limit_peaks(const LoudFilter &F, const float *x, int64_t N, std::vector<double> *p, uint64_t *tp_bits, uint32_t *sp_bits)
{
    auto xs = [&](int64_t n) { return n >= 0 && n < N ? loud_sample(x[n]) : 0.0; };
    uint64_t tpb = 0;
    uint32_t spb = 0;
    if (p) p->assign((size_t)(N + LOUD_TP_TAIL), 0.0);
    for (int64_t m = -LIMIT_DELAY; m < N + LIMIT_HEAD; m++)
    {
        double w[LOUD_PHASE_TAPS];
        for (int k = 0; k < LOUD_PHASE_TAPS; k++) w[k] = xs(m + LIMIT_DELAY - k);
        uint64_t b = loud_dbits(fabs(xs(m)));
        for (int f = 1; f < 4; f++)
        {
            const uint64_t v = loud_dbits(fabs(loud_tp_phase(F.c, f, w)));
            b = v > b ? v : b;
        }
        tpb = b > tpb ? b : tpb;
        if (p) (*p)[(size_t)(m + LIMIT_DELAY)] = mel_from_bits(b);
        if (m >= 0 && m < N)
        {
            const uint32_t a = level_abs_bits(x[m]);
            spb = a > spb ? a : spb;
        }
    }
    *tp_bits = tpb;
    *sp_bits = spb;
}

// Host reference of the whole rule for one utterance: x[0 .. total) the waveform, N <= total the samples measured, out[0 .. total).
// s (may be null) receives s_n, n < total.  The minimum runs over a monotonic queue and the mean over a running sum: integers, so any
// other order gives the same values.
inline LimitRow limit_reference(const LoudFilter &F, const float *x, uint64_t N_, uint64_t total_, const LimitAsk &a, float *out,
                                std::vector<uint32_t> *s_out = nullptr)
{
    const int64_t N = (int64_t)N_, total = (int64_t)total_, H = limit_halo(a), W = H + 1;
    std::vector<double> p;
    uint64_t tp_before, tp_after;
    uint32_t sp_before, sp_after;
    limit_peaks(F, x, N, &p, &tp_before, &sp_before);
    const int64_t qlen = total + 2 * H, mlen = limit_mlen(total, H);
    std::vector<uint32_t> q((size_t)qlen, LIMIT_ONE), m((size_t)mlen);      // (here q_j lies at j + H: j in [-H, total + H) is what the windows reach)
    for (int64_t j = -LIMIT_DELAY; j < N + LIMIT_HEAD; j++)
        if (j + H >= 0 && j + H < qlen) q[(size_t)(j + H)] = limit_q(a.gain, a.ceiling, p[(size_t)(j + LIMIT_DELAY)]);
    std::deque<int64_t> dq;                       // indices of q, their values ascending
    for (int64_t i = 0; i < qlen; i++)
    {
        while (!dq.empty() && q[(size_t)dq.back()] >= q[(size_t)i]) dq.pop_back();
        dq.push_back(i);
        if (dq.front() + H < i) dq.pop_front();
        if (i >= H) m[(size_t)(i - H)] = q[(size_t)dq.front()];      // min q[i - H .. i]
    }
    uint64_t sum = 0, limited = 0;
    uint32_t min_s = LIMIT_ONE;
    for (int64_t i = 0; i < H; i++) sum += m[(size_t)i];
    if (s_out) s_out->resize((size_t)total);
    for (int64_t n = 0; n < total; n++)
    {
        sum += m[(size_t)(n + H)];
        const uint32_t s = (uint32_t)(sum / (uint64_t)W);
        sum -= m[(size_t)n];
        out[n] = limit_apply(x[n], a.gain, s);
        if (s_out) (*s_out)[(size_t)n] = s;
        if (n < N)
        {
            min_s = s < min_s ? s : min_s;
            limited += s < LIMIT_ONE;
        }
    }
    limit_peaks(F, out, N, nullptr, &tp_after, &sp_after);
    return limit_finish(tp_before, sp_before, tp_after, sp_after, min_s, limited);
}
#endif

}  // namespace zv
