// align.h — mel alignment (include/zerovox_amd.h "mel alignment"): the dynamic-time-warping path between two sequences of mel rows,
// its spectral distance and the two frame maps.  Plain arithmetic shared by the five kernels (align_kernels.hip), the C-ABI (capi.cpp)
// and the host-side test (tests/native/align_check.cpp): nothing here needs HIP.
//
// Every step is an integer or ONE IEEE f64 operation written as a statement of its own (the library builds with -ffp-contract=off):
//   quantise   q = trunc(clamp(x * scale, +-1023) +- 0.5), a non-finite x counts as +0.0
//   normalise  q' = q - floor((2 s + T) / (2 T)), s the channel's sum over the sequence (only when asked), |q'| <= 2046
//   cost       c[i][j] = sum over m of (qa'[i][m] - qb'[j][m])^2 < 2^32: on the device na[i] + nb[j] - 2 dot, the dot product in three
//              digit-plane sums of two signed base-128 digits (bands_digits) on v_mfma_i32_16x16x64_i8, joined as int64 (align_combine)
//   path       D[i][j] = c[i][j] + min over (i-1, j-1), (i-1, j), (i, j-1) in THAT order, a later one only when strictly smaller
//   walk       from the end to (0, 0) along the recorded choices: the maps, the path length L, acc += sqrt((double)c) per cell,
//              then acc / L, then / scale
// Integers are exact whatever the split over lanes, waves, tiles and workgroups; the f64 sum has ONE order, the walk's.
#pragma once

#include <math.h>
#include <stdint.h>

#include "bands.h"         // bands_digits, ZV_LV_FN, level_bits

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

namespace zv
{

constexpr uint32_t ALIGN_MAX_FRAMES = 4096;                        // rows of either sequence (include/zerovox_amd.h ZV_ALIGN_MAX_FRAMES)
constexpr uint32_t ALIGN_MAX_MELS = 256;                           // channels per row
constexpr uint64_t ALIGN_GROUP_CELLS = 1ull << 27;                 // cells of cost (u32) and choice (u8) one launch group holds: 640 MiB
constexpr int      ALIGN_DP_ROWS = 1024;                           // rows one pass of align_dp_kernel covers: a thread per row
constexpr int      ALIGN_TILE = 64;                                // rows and columns of the cost matrix one workgroup of align_cost_kernel covers
constexpr int      ALIGN_QUANT_ROWS = 16;                          // rows one workgroup of align_quant_kernel covers
constexpr int      ALIGN_SUM_CHANNELS = 64;                        // channels one workgroup of align_means_kernel covers
constexpr int      ALIGN_WINDOW = 8;                               // rows and columns of choices align_walk_kernel loads at once
constexpr float    ALIGN_SCALE = 64.0f;                            // what scale = 0 means
constexpr uint32_t ALIGN_NONE = 3;                                 // the choice of (0, 0); 0: (i-1, j-1), 1: (i-1, j), 2: (i, j-1)

// cost and choice of a pair are stored SKEWED: cell (i, j) lies in row (i + j) mod Tb, column i of a [Tb][Ta] matrix.  That is compact
// (j -> (i + j) mod Tb is one-to-one for every i), and the cells of an anti-diagonal, which the threads of the dp pass touch in ONE
// step, lie side by side instead of Tb entries apart.
ZV_LV_FN size_t align_cell(int i, int j, int Ta, int Tb) { return (size_t)((i + j) % Tb) * Ta + i; }
ZV_LV_FN int align_k(int M) { return (M + 63) / 64 * 64; }         // bytes of a row in a digit plane: M rounded up to the MFMA's 64, zero filled

// one pair of a launch group, as the kernels read it
struct AlignPair
{
    int32_t  Ta, Tb;        // rows of a and of b
    int32_t  row_a, row_b;  // their first rows among the group's sequence rows (inputs, planes, norms)
    int32_t  map0;          // first entry of [map_a (Ta) | map_b (Tb)] among the group's map entries
    int32_t  reserved;
    uint64_t cell0;         // first cell of the pair's Ta * Tb cells of cost and choice (align_cell)
};
// what the walk stores per pair; the layout of include/zerovox_amd.h zv_alignment
struct AlignRow
{
    uint64_t total;
    double   distance;
    uint32_t path_len, reserved;
};

ZV_LV_FN int64_t align_quant(float x, double scale)
{
    const uint32_t b = level_bits(x);
    const float y = (b & 0x7f800000u) == 0x7f800000u ? 0.0f : x;
    double d = (double)y * scale;
    d = d < -1023.0 ? -1023.0 : d;
    d = d > 1023.0 ? 1023.0 : d;
    d = d + (d >= 0.0 ? 0.5 : -0.5);
    return (int64_t)d;
}
// round half up of s / T, a true floor
ZV_LV_FN int32_t align_mean(int64_t s, int32_t T)
{
    const int64_t n = 2 * s + T, d = 2 * (int64_t)T;
    int64_t q = n / d;
    if (n % d != 0 && n < 0) q = q - 1;
    return (int32_t)q;
}
ZV_LV_FN int64_t align_combine(int32_t hh, int32_t mid, int32_t ll) { return 16384 * (int64_t)hh + 128 * (int64_t)mid + (int64_t)ll; }
// the predecessor of a cell: diag, up, left are D of (i-1, j-1), (i-1, j), (i, j-1); the choice is stored per cell
ZV_LV_FN int64_t align_choose(bool has_i, bool has_j, int64_t diag, int64_t up, int64_t left, uint32_t &choice)
{
    int64_t best = 0;
    choice = ALIGN_NONE;
    if (has_i && has_j) best = diag, choice = 0;
    if (has_i && (choice == ALIGN_NONE || up < best)) best = up, choice = 1;
    if (has_j && (choice == ALIGN_NONE || left < best)) best = left, choice = 2;
    return best;
}
ZV_LV_FN double align_step(double acc, uint32_t c)
{
    const double r = sqrt((double)c);
    return acc + r;
}
ZV_LV_FN double align_distance(double acc, uint32_t L, float scale)
{
    double d = acc / (double)L;
    d = d / (double)scale;
    return d;
}

// ---- the launches' geometry: ONE launch per kernel per launch group ----
struct AlignPlan
{
    bool ok;                    // 1 <= pairs, 1 <= M <= ALIGN_MAX_MELS, 1 <= max rows <= ALIGN_MAX_FRAMES
    int  means_gx, means_gy;    // align_means_kernel: blocks of ALIGN_SUM_CHANNELS channels x sequences (2 per pair)
    int  quant_gx, quant_gy;    // align_quant_kernel: tiles of ALIGN_QUANT_ROWS rows x sequences
    int  cost_gx, cost_gy, cost_gz;      // align_cost_kernel: tiles of ALIGN_TILE columns x tiles of ALIGN_TILE rows x pairs
    int  dp_gx, walk_gx;        // align_dp_kernel (ALIGN_DP_ROWS threads) and align_walk_kernel (one wave): a workgroup per pair
};
inline AlignPlan align_plan(int n_pairs, int max_ta, int max_tb, int M)
{
    const int mx = max_ta > max_tb ? max_ta : max_tb;
    const bool ok = n_pairs >= 1 && M >= 1 && M <= (int)ALIGN_MAX_MELS && max_ta >= 1 && max_tb >= 1 && mx <= (int)ALIGN_MAX_FRAMES;
    return AlignPlan{ok, (M + ALIGN_SUM_CHANNELS - 1) / ALIGN_SUM_CHANNELS, 2 * n_pairs, (mx + ALIGN_QUANT_ROWS - 1) / ALIGN_QUANT_ROWS, 2 * n_pairs,
                     (max_tb + ALIGN_TILE - 1) / ALIGN_TILE, (max_ta + ALIGN_TILE - 1) / ALIGN_TILE, n_pairs, n_pairs, n_pairs};
}
// where the launch group that starts at pair `first` ends: consecutive pairs while their cells stay within ALIGN_GROUP_CELLS (a pair
// holds at most 2^24, so a group is never empty)
inline uint32_t align_group_end(uint32_t first, uint32_t n_pairs, const uint32_t *Ta, const uint32_t *Tb)
{
    uint64_t cells = 0;
    uint32_t p = first;
    while (p < n_pairs && cells + (uint64_t)Ta[p] * Tb[p] <= ALIGN_GROUP_CELLS)
    {
        cells += (uint64_t)Ta[p] * Tb[p];
        p++;
    }
    return p > first ? p : first + 1;
}
// the steps of align_dp_kernel's loop: thread r of ALIGN_DP_ROWS takes rows r, r + ALIGN_DP_ROWS, ... and enters column 0 of pass k at
// step k * P + r, P = max(Tb, ALIGN_DP_ROWS), so the row above is always one step ahead
ZV_LV_FN int align_dp_stride(int Tb) { return Tb > ALIGN_DP_ROWS ? Tb : ALIGN_DP_ROWS; }
ZV_LV_FN int align_dp_steps(int Ta, int Tb)
{
    const int passes = (Ta + ALIGN_DP_ROWS - 1) / ALIGN_DP_ROWS, last = Ta - (passes - 1) * ALIGN_DP_ROWS;
    return (passes - 1) * align_dp_stride(Tb) + Tb + last - 1;
}

// "scale", "normalise" or null: the parameters as the entry points check them; scale is resolved (0 -> ALIGN_SCALE)
inline const char *align_resolve(float &scale, uint32_t normalise)
{
    if (scale == 0.0f) scale = ALIGN_SCALE;
    if ((level_bits(scale) & 0x7f800000u) == 0x7f800000u || !(scale > 0.0f)) return "scale";
    if (normalise > 1u) return "normalise";
    return nullptr;
}

// The timing transfer (zv_align_durations): "durations_a", "sum", "map_a" or null.
inline const char *align_durations(uint32_t n, const int32_t *da, uint32_t Ta, const int32_t *map_a, uint32_t Tb, int32_t *db)
{
    uint64_t sum = 0;
    for (uint32_t p = 0; p < n; p++)
    {
        if (da[p] < 0) return "durations_a";
        sum += (uint64_t)da[p];
    }
    if (sum != (uint64_t)Ta) return "sum";
    for (uint32_t i = 0; i < Ta; i++)
        if (map_a[i] < 0 || (uint64_t)map_a[i] >= (uint64_t)Tb || (i && map_a[i] < map_a[i - 1])) return "map_a";
    uint64_t s = 0;
    int64_t pos = 0;
    for (uint32_t p = 0; p < n; p++)
    {
        s += (uint64_t)da[p];
        const int64_t next = p + 1 == n ? (int64_t)Tb : s < (uint64_t)Ta ? (int64_t)map_a[s] : (int64_t)Tb;
        db[p] = (int32_t)(next - pos);
        pos = next;
    }
    return nullptr;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host side only: the reference, the rule in plain loops ----
// q'[T][M] of one sequence
inline std::vector<int32_t> align_rows(const float *x, uint32_t T, uint32_t M, float scale, uint32_t normalise)
{
    std::vector<int32_t> q((size_t)T * M);
    for (size_t i = 0; i < q.size(); i++) q[i] = (int32_t)align_quant(x[i], (double)scale);
    if (normalise)
        for (uint32_t m = 0; m < M; m++)
        {
            int64_t s = 0;
            for (uint32_t t = 0; t < T; t++) s += q[(size_t)t * M + m];
            const int32_t mean = align_mean(s, (int32_t)T);
            for (uint32_t t = 0; t < T; t++) q[(size_t)t * M + m] -= mean;
        }
    return q;
}
// the three steps of the reference, each on its own so that a host program can time them
// c[Ta][Tb]
inline std::vector<uint32_t> align_costs(const std::vector<int32_t> &qa, uint32_t Ta, const std::vector<int32_t> &qb, uint32_t Tb, uint32_t M)
{
    std::vector<uint32_t> c((size_t)Ta * Tb);
    for (uint32_t i = 0; i < Ta; i++)
        for (uint32_t j = 0; j < Tb; j++)
        {
            uint64_t s = 0;
            const int32_t *ra = &qa[(size_t)i * M], *rb = &qb[(size_t)j * M];
            for (uint32_t m = 0; m < M; m++)
            {
                const int64_t d = (int64_t)ra[m] - rb[m];
                s += (uint64_t)(d * d);
            }
            c[(size_t)i * Tb + j] = (uint32_t)s;
        }
    return c;
}
// the choices [Ta][Tb]; returns D of the last cell
inline int64_t align_path(const std::vector<uint32_t> &c, uint32_t Ta, uint32_t Tb, std::vector<uint8_t> &ch)
{
    ch.resize((size_t)Ta * Tb);
    std::vector<int64_t> prev(Tb), cur(Tb);
    for (uint32_t i = 0; i < Ta; i++)
    {
        for (uint32_t j = 0; j < Tb; j++)
        {
            uint32_t k;
            const int64_t best = align_choose(i > 0, j > 0, i && j ? prev[j - 1] : 0, i ? prev[j] : 0, j ? cur[j - 1] : 0, k);
            cur[j] = (int64_t)c[(size_t)i * Tb + j] + best;
            ch[(size_t)i * Tb + j] = (uint8_t)k;
        }
        prev.swap(cur);
    }
    return prev[Tb - 1];
}
// scale: resolved.  map_a [Ta] and map_b [Tb] may be null.
inline AlignRow align_walk(const std::vector<uint32_t> &c, const std::vector<uint8_t> &ch, uint32_t Ta, uint32_t Tb, int64_t total, float scale,
                           int32_t *map_a, int32_t *map_b)
{
    AlignRow r{(uint64_t)total, 0.0, 0, 0};
    double acc = 0.0;
    uint32_t i = Ta - 1, j = Tb - 1;
    for (;;)
    {
        acc = align_step(acc, c[(size_t)i * Tb + j]);
        r.path_len++;
        if (map_a) map_a[i] = (int32_t)j;
        if (map_b) map_b[j] = (int32_t)i;
        const uint32_t k = ch[(size_t)i * Tb + j];
        if (k == ALIGN_NONE) break;
        if (k != 2) i--;
        if (k != 1) j--;
    }
    r.distance = align_distance(acc, r.path_len, scale);
    return r;
}
inline AlignRow align_reference(const float *a, uint32_t Ta, const float *b, uint32_t Tb, uint32_t M, float scale, uint32_t normalise,
                                int32_t *map_a, int32_t *map_b)
{
    const std::vector<uint32_t> c = align_costs(align_rows(a, Ta, M, scale, normalise), Ta, align_rows(b, Tb, M, scale, normalise), Tb, M);
    std::vector<uint8_t> ch;
    const int64_t total = align_path(c, Ta, Tb, ch);
    return align_walk(c, ch, Ta, Tb, total, scale, map_a, map_b);
}
#endif

}  // namespace zv
