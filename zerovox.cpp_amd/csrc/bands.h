// bands.h — band levels (include/zerovox_amd.h "band levels"): the energy of an utterance per frequency band as it runs, per frame and
// per phoneme.  Plain arithmetic shared by bands_frames_kernel / bands_phonemes_kernel (bands_kernels.hip) and the host-side test
// (tests/native/bands_check.cpp): nothing here needs HIP.
//
// A frame is a 1 024-point DFT of its Hann-windowed span in exact integers.  The span is block scaled to integers of at most 8 191 in
// magnitude (bands_quant: the pitch track's quantiser at 13 bits), the window and the twiddles are ONE table of 8-bit integers
// (bands_twiddle), so Re(k) and Im(k) are integers below 2^29: any split over lanes, digit planes and matrix instructions gives the
// same sums.  The powers, their shift and the band sums are unsigned 64-bit integers.  Behind the sums every f64 step is ONE IEEE
// operation, written as a statement of its own; the library builds with -ffp-contract=off.
#pragma once

#include <math.h>
#include <stdint.h>

#include "contour.h"       // ZV_LV_FN, level_bits, level_abs_bits, contour_extent

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

namespace zv
{

constexpr int      BANDS_N = 1024;                                 // window and DFT length
constexpr int      BANDS_BINS = BANDS_N / 2 + 1;                   // bins 0 .. 512
constexpr int      BANDS_TWIDDLE = 126;                            // twiddle scale: at 126 no table product is near a tie (bands_twiddle)
constexpr int32_t  BANDS_Q_MAX = 8191;
constexpr uint32_t BANDS_MAX = 64, BANDS_DEFAULT = 16;             // bands per utterance
constexpr uint32_t BANDS_SILENT_BITS = 0x33800000u;                // 2^-24: a span whose peak is below it is silent
constexpr double   BANDS_NORM = 48774928.0;                        // 8 * W2, W2 = the sum of round(126 * wnd(t))^2 = 6 096 866
constexpr double   BANDS_EQ_ONE = 274877906944.0;                  // 2^38: what the phonemes' kept power is scaled by
constexpr uint64_t BANDS_EQ_MAX = (uint64_t)1 << 47;               // the kept power saturates here (an RMS of about 22)
constexpr uint32_t BANDS_DEFAULT_EDGES[BANDS_DEFAULT + 1] = {1, 3, 5, 8, 12, 17, 24, 33, 45, 62, 84, 114, 155, 210, 285, 387, 513};
// a parameter row in HBM, uint32 [segment][BANDS_PARAM_STRIDE]: n_bands (0: this segment is not metered), edges[n_bands + 1] — resolved
constexpr int BANDS_PARAM_STRIDE = 68;
// rows of both tables and of the slab on the device: BANDS_MAX entries per frame row / token row, the first n_bands of them written
constexpr int BANDS_ROW_STRIDE = (int)BANDS_MAX;
// frames one workgroup of bands_frames_kernel covers: two 16-row matrix tiles
constexpr int BANDS_TILE_FRAMES = 32;

// The table in the order bands_frames_kernel reads it (B operand of v_mfma_i32_16x16x64_i8, 16 bytes of a lane at a time):
// [trig 0 cos / 1 sin][bin block of 16][k step of 64 samples][lane][16], lane l holding bin = 16 * block + (l & 15) and the samples
// t = 64 * step + 16 * (l >> 4) + j.  BANDS_BIN_BLOCKS covers the 513 bins and rounds up to a pair; bins past 512 are zeros.
constexpr int    BANDS_BIN_BLOCKS = 34, BANDS_K_STEPS = BANDS_N / 64;
constexpr size_t BANDS_TABLE_BYTES = (size_t)2 * BANDS_BIN_BLOCKS * BANDS_K_STEPS * 64 * 16;
ZV_LV_FN size_t bands_table_index(int trig, int bin, int t)
{
    const int blk = bin >> 4, step = t >> 6, lane = (bin & 15) + 16 * ((t >> 4) & 3), j = t & 15;
    return ((((size_t)trig * BANDS_BIN_BLOCKS + blk) * BANDS_K_STEPS + step) * 64 + lane) * 16 + j;
}

// Defaults and validation: n_bands 0 = 16, edges null = the default edges (then n_bands must be 0 or 16).  Fills row
// [BANDS_PARAM_STRIDE] and returns null, else the name of the field that is wrong.
ZV_LV_FN const char *bands_resolve(uint32_t n_bands, const uint32_t *edges, uint32_t *row)
{
    if (n_bands > BANDS_MAX) return "n_bands";
    if (!edges && n_bands != 0 && n_bands != BANDS_DEFAULT) return "edges";
    const uint32_t nb = n_bands ? n_bands : BANDS_DEFAULT;
    const uint32_t *e = edges ? edges : BANDS_DEFAULT_EDGES;
    for (uint32_t b = 0; b < nb; b++)
        if (!(e[b] < e[b + 1])) return "edges";
    if (e[nb] > (uint32_t)BANDS_BINS) return "edges";
    for (int i = 0; i < BANDS_PARAM_STRIDE; i++) row[i] = 0;
    row[0] = nb;
    for (uint32_t b = 0; b <= nb; b++) row[1 + b] = e[b];
    return nullptr;
}

// the span of frame f: its first sample s0 (signed; the span is w[s0 .. s0 + 1024), zeros outside the utterance)
ZV_LV_FN int64_t bands_span(uint32_t f, uint32_t hop) { return (int64_t)f * hop + hop / 2u - (uint32_t)BANDS_N / 2u; }

// the exponent k of the span whose peak has the bits pk >= BANDS_SILENT_BITS: e = (pk >> 23) - 127, k = 12 - e (-115 <= k <= 36), so
// that the peak lands in 4096 .. 8191
ZV_LV_FN int bands_exponent(uint32_t pk) { return 12 - ((int)(pk >> 23) - 127); }
ZV_LV_FN double bands_pow2(int k)
{
    const uint64_t b = (uint64_t)(1023 + k) << 52;
    double s;
    __builtin_memcpy(&s, &b, 8);
    return s;
}

// the block-scaled sample: sign(y) * min((int64)(|y| * 2^k + 0.5), 8191); a NaN or infinite sample is 0
ZV_LV_FN int32_t bands_quant(float y, double scale)
{
    const uint32_t b = level_bits(y), ab = level_abs_bits(y);
    double d = (double)level_from_bits(ab);
    d = d * scale;
    d = d + 0.5;
    int32_t q = (int32_t)d;                                        // 0.5 <= d < 8193: the conversion truncates, as the rule's (int64) does
    q = q < BANDS_Q_MAX ? q : BANDS_Q_MAX;
    return (b >> 31) ? -q : q;
}

// the two signed 8-bit digits of a quantised sample: a = 128 * hi + lo, both in [-64, 64] (the shift is arithmetic: a floor)
ZV_LV_FN void bands_digits(int32_t a, int32_t &hi, int32_t &lo)
{
    hi = (a + 64) >> 7;
    lo = a - 128 * hi;
}

// Q(k) from Re(k) and Im(k), both below 2^29 in magnitude
ZV_LV_FN uint64_t bands_power(int32_t re, int32_t im)
{
    const int64_t r = re, i = im;
    const uint64_t p = (uint64_t)(r * r) + (uint64_t)(i * i);
    return p >> 6;
}

// a band's row entry from its sum S_b and the frame's exponent k, and what is kept of it for the phonemes
ZV_LV_FN float bands_row(uint64_t S, int k, uint64_t &eq)
{
    double pw = (double)S;
    pw = pw / BANDS_NORM;
    pw = pw * bands_pow2(-2 * k);
    double v = pw * BANDS_EQ_ONE;
    v = v + 0.5;
    eq = v >= (double)BANDS_EQ_MAX ? BANDS_EQ_MAX : (uint64_t)v;
    const double r = sqrt(pw);
    return (float)r;
}

// a phoneme's row entry from the sum of its frames' kept powers and its frames
ZV_LV_FN float bands_phoneme_row(uint64_t sum, uint64_t d)
{
    if (d == 0) return 0.0f;
    double den = (double)d;
    den = den * BANDS_EQ_ONE;
    double m = (double)sum;
    m = m / den;
    m = sqrt(m);
    return (float)m;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host side only, like pitch.h's reference: the tables and the reference; a device pass sees none of it ----
// the Hann window and one table entry: trig 0 is C[k][t], trig 1 is S[k][t].  (k * t) mod N is reduced in integers ahead of the
// division.  At scale 126 no product lies within 1e-5 of a half-integer, so any libm gives the same integer.
inline double bands_window(int t) { return 0.5 - 0.5 * cos(2.0 * M_PI * (double)t / (double)BANDS_N); }
inline int bands_twiddle(int trig, int k, int t)
{
    const double ang = 2.0 * M_PI * (double)((k * t) % BANDS_N) / (double)BANDS_N;
    const double x = (double)BANDS_TWIDDLE * bands_window(t) * (trig ? sin(ang) : cos(ang));
    return (int)floor(x + 0.5);
}
// the plain tables [2][513][1024] and the kernel's image of them (bands_table_index)
inline std::vector<int8_t> bands_tables()
{
    std::vector<int8_t> tab((size_t)2 * BANDS_BINS * BANDS_N);
    for (int trig = 0; trig < 2; trig++)
        for (int k = 0; k < BANDS_BINS; k++)
            for (int t = 0; t < BANDS_N; t++) tab[((size_t)trig * BANDS_BINS + k) * BANDS_N + t] = (int8_t)bands_twiddle(trig, k, t);
    return tab;
}
inline std::vector<int8_t> bands_table_fragments(const std::vector<int8_t> &tab)
{
    std::vector<int8_t> img(BANDS_TABLE_BYTES, 0);
    for (int trig = 0; trig < 2; trig++)
        for (int k = 0; k < BANDS_BINS; k++)
            for (int t = 0; t < BANDS_N; t++) img[bands_table_index(trig, k, t)] = tab[((size_t)trig * BANDS_BINS + k) * BANDS_N + t];
    return img;
}

// Host reference of one frame: w[0 .. n) is the utterance's waveform, par a resolved parameter row, tab the plain tables.  row
// [n_bands] and eq [n_bands] receive the frame's entries.
inline void bands_frame_reference(const float *w, uint64_t n, uint32_t f, uint32_t hop, const uint32_t *par, const int8_t *tab, float *row,
                                  uint64_t *eq)
{
    const uint32_t nb = par[0];
    const int64_t s0 = bands_span(f, hop);
    float y[BANDS_N];
    uint32_t pk = 0;
    for (int t = 0; t < BANDS_N; t++)
    {
        const int64_t s = s0 + t;
        y[t] = 0.0f;
        if (s >= 0 && (uint64_t)s < n && level_abs_bits(w[s]) == (level_bits(w[s]) & 0x7fffffffu)) y[t] = w[s];
        const uint32_t a = level_abs_bits(y[t]);
        pk = a > pk ? a : pk;
    }
    for (uint32_t b = 0; b < nb; b++)
    {
        row[b] = 0.0f;
        eq[b] = 0;
    }
    if (pk < BANDS_SILENT_BITS) return;
    const int k = bands_exponent(pk);
    const double scale = bands_pow2(k);
    int32_t a[BANDS_N];
    for (int t = 0; t < BANDS_N; t++) a[t] = bands_quant(y[t], scale);
    for (uint32_t b = 0; b < nb; b++)
    {
        uint64_t S = 0;
        for (uint32_t bin = par[1 + b]; bin < par[2 + b]; bin++)
        {
            const int8_t *c = tab + (size_t)bin * BANDS_N, *s = tab + ((size_t)BANDS_BINS + bin) * BANDS_N;
            int64_t re = 0, im = 0;
            for (int t = 0; t < BANDS_N; t++)
            {
                re += (int64_t)a[t] * c[t];
                im += (int64_t)a[t] * s[t];
            }
            S += bands_power((int32_t)re, (int32_t)im);
        }
        row[b] = bands_row(S, k, eq[b]);
    }
}

// Host reference of the whole rule for one utterance: w[0 .. T * hop) is the waveform of its capacity, durations [n] its phoneme
// timings.  frames [T][n_bands] and phonemes [n][n_bands] receive the rows (either may be null).
inline void bands_reference(const float *w, uint32_t T, uint32_t hop, const uint32_t *par, const int8_t *tab, const int32_t *durations, uint32_t n,
                            float *frames, float *phonemes)
{
    const uint32_t nb = par[0];
    std::vector<uint64_t> eq((size_t)T * nb);
    std::vector<float> row(nb);
    for (uint32_t f = 0; f < T; f++)
    {
        bands_frame_reference(w, (uint64_t)T * hop, f, hop, par, tab, row.data(), eq.data() + (size_t)f * nb);
        for (uint32_t b = 0; frames && b < nb; b++) frames[(size_t)f * nb + b] = row[b];
    }
    uint64_t start = 0;
    for (uint32_t i = 0; phonemes && i < n; i++)
    {
        const uint64_t d = durations[i] > 0 ? (uint64_t)durations[i] : 0;
        for (uint32_t b = 0; b < nb; b++)
        {
            uint64_t sum = 0;
            for (uint64_t f = start; f < start + d && f < T; f++) sum += eq[(size_t)f * nb + b];
            phonemes[(size_t)i * nb + b] = bands_phoneme_row(sum, d);
        }
        start += d;
    }
}

#endif

}  // namespace zv
