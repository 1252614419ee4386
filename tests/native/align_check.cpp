// Host-side driver of csrc/align.h for tests/test_align_cpu.py (no GPU, no HIP).
// `align_check plan` reads lines "n_pairs max_ta max_tb M" and prints "ok means_gx means_gy quant_gx quant_gy cost_gx cost_gy cost_gz dp_gx
// walk_gx" of align.h's align_plan for each.
// `align_check groups` reads "n" and n pairs "Ta Tb" and prints where the launch groups end (align_group_end), one line.
// `align_check steps` reads lines "Ta Tb" and prints align_dp_steps for each.
// `align_check durations` reads cases "n Ta Tb", n durations and Ta map entries, and prints "refused FIELD" or the n results.
// `align_check bench Ta Tb M REPS` times the reference's steps on rows it makes itself (a fixed generator) and prints the least of REPS
// runs in ms: "quantise cost path walk".
// Without arguments it reads cases from stdin until it ends.  Every float travels as the hexadecimal bit pattern of its f32 value, so
// that inf, NaN and -0.0 arrive unchanged.  A case:
//     Ta Tb M scale normalise
//     Ta * M floats, then Tb * M floats
// and prints one line per case: "total distance-bits path_len | map_a ... | map_b ...", or "refused FIELD" where align_resolve refuses.
// The reference runs twice, with and without the maps' pointers, and both runs must agree.
#include "align.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static float from_bits(unsigned b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

static int plan_mode()
{
    int n, ta, tb, M;
    while (scanf("%d %d %d %d", &n, &ta, &tb, &M) == 4)
    {
        const zv::AlignPlan p = zv::align_plan(n, ta, tb, M);
        printf("%d %d %d %d %d %d %d %d %d %d\n", (int)p.ok, p.means_gx, p.means_gy, p.quant_gx, p.quant_gy, p.cost_gx, p.cost_gy, p.cost_gz, p.dp_gx,
               p.walk_gx);
    }
    return 0;
}

static int groups_mode()
{
    unsigned n;
    if (scanf("%u", &n) != 1 || n > (1u << 20)) return fprintf(stderr, "bad count\n"), 2;
    std::vector<uint32_t> Ta(n), Tb(n);
    for (unsigned p = 0; p < n; p++)
        if (scanf("%u %u", &Ta[p], &Tb[p]) != 2) return fprintf(stderr, "short input\n"), 2;
    for (uint32_t g = 0; g < n;)
    {
        g = zv::align_group_end(g, n, Ta.data(), Tb.data());
        printf("%u ", g);
    }
    printf("\n");
    return 0;
}

static int steps_mode()
{
    int ta, tb;
    while (scanf("%d %d", &ta, &tb) == 2) printf("%d\n", zv::align_dp_steps(ta, tb));
    return 0;
}

static int durations_mode()
{
    unsigned n, Ta, Tb;
    while (scanf("%u %u %u", &n, &Ta, &Tb) == 3)
    {
        if (n > (1u << 20) || Ta > (1u << 20)) return fprintf(stderr, "bad header\n"), 2;
        std::vector<int32_t> da(n), map(Ta), db(n);
        for (int32_t &v : da)
            if (scanf("%d", &v) != 1) return fprintf(stderr, "short input\n"), 2;
        for (int32_t &v : map)
            if (scanf("%d", &v) != 1) return fprintf(stderr, "short input\n"), 2;
        if (const char *field = zv::align_durations(n, da.data(), Ta, map.data(), Tb, db.data()))
        {
            printf("refused %s\n", field);
            continue;
        }
        for (int32_t v : db) printf("%d ", v);
        printf("\n");
    }
    return 0;
}

static int bench_mode(char **argv)
{
    const unsigned Ta = (unsigned)strtoul(argv[0], nullptr, 10), Tb = (unsigned)strtoul(argv[1], nullptr, 10), M = (unsigned)strtoul(argv[2], nullptr, 10);
    const int reps = atoi(argv[3]);
    if (Ta < 1 || Tb < 1 || Ta > zv::ALIGN_MAX_FRAMES || Tb > zv::ALIGN_MAX_FRAMES || M < 1 || M > zv::ALIGN_MAX_MELS || reps < 1) return fprintf(stderr, "bad sizes\n"), 2;
    std::vector<float> a((size_t)Ta * M), b((size_t)Tb * M);
    uint32_t lcg = 12345u;
    for (std::vector<float> *v : {&a, &b})
        for (float &e : *v)
        {
            lcg = lcg * 1664525u + 1013904223u;
            e = (float)(lcg >> 8) / 16777216.0f * 8.0f - 8.0f;      // the range of natural-log mels
        }
    double best[4] = {1e30, 1e30, 1e30, 1e30};
    unsigned long long sink = 0;
    for (int r = 0; r < reps; r++)
    {
        using clk = std::chrono::steady_clock;
        const auto t0 = clk::now();
        const std::vector<int32_t> qa = zv::align_rows(a.data(), Ta, M, zv::ALIGN_SCALE, 1), qb = zv::align_rows(b.data(), Tb, M, zv::ALIGN_SCALE, 1);
        const auto t1 = clk::now();
        const std::vector<uint32_t> c = zv::align_costs(qa, Ta, qb, Tb, M);
        const auto t2 = clk::now();
        std::vector<uint8_t> ch;
        const int64_t total = zv::align_path(c, Ta, Tb, ch);
        const auto t3 = clk::now();
        std::vector<int32_t> map_a(Ta), map_b(Tb);
        const zv::AlignRow row = zv::align_walk(c, ch, Ta, Tb, total, zv::ALIGN_SCALE, map_a.data(), map_b.data());
        const auto t4 = clk::now();
        sink += row.total + row.path_len;
        const double ms[4] = {std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count(),
                              std::chrono::duration<double, std::milli>(t3 - t2).count(), std::chrono::duration<double, std::milli>(t4 - t3).count()};
        for (int k = 0; k < 4; k++) best[k] = ms[k] < best[k] ? ms[k] : best[k];
    }
    printf("%.4f %.4f %.4f %.4f\n", best[0], best[1], best[2], best[3]);
    return sink == 1 ? 3 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "bench")) return bench_mode(argv + 2);
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan_mode();
    if (argc == 2 && !strcmp(argv[1], "groups")) return groups_mode();
    if (argc == 2 && !strcmp(argv[1], "steps")) return steps_mode();
    if (argc == 2 && !strcmp(argv[1], "durations")) return durations_mode();
    long cases = 0;
    unsigned Ta, Tb, M, sc, normalise;
    while (scanf("%u %u %u %x %u", &Ta, &Tb, &M, &sc, &normalise) == 5)
    {
        if (Ta < 1 || Tb < 1 || Ta > zv::ALIGN_MAX_FRAMES || Tb > zv::ALIGN_MAX_FRAMES || M < 1 || M > zv::ALIGN_MAX_MELS)
            return fprintf(stderr, "case %ld: bad header\n", cases), 2;
        std::vector<float> a((size_t)Ta * M), b((size_t)Tb * M);
        for (std::vector<float> *v : {&a, &b})
            for (float &e : *v)
            {
                unsigned bits = 0;
                if (scanf("%x", &bits) != 1) return fprintf(stderr, "case %ld: short line\n", cases), 2;
                e = from_bits(bits);
            }
        cases++;
        float scale = from_bits(sc);
        if (const char *field = zv::align_resolve(scale, normalise))
        {
            printf("refused %s\n", field);
            continue;
        }
        std::vector<int32_t> map_a(Ta, -1), map_b(Tb, -1);
        const zv::AlignRow r = zv::align_reference(a.data(), Ta, b.data(), Tb, M, scale, normalise, map_a.data(), map_b.data());
        const zv::AlignRow bare = zv::align_reference(a.data(), Ta, b.data(), Tb, M, scale, normalise, nullptr, nullptr);
        if (memcmp(&r, &bare, sizeof r) != 0) return fprintf(stderr, "case %ld: the run without maps differs\n", cases), 2;
        unsigned long long d;
        memcpy(&d, &r.distance, 8);
        printf("%llu %llx %u |", (unsigned long long)r.total, d, r.path_len);
        for (int32_t v : map_a) printf(" %d", v);
        printf(" |");
        for (int32_t v : map_b) printf(" %d", v);
        printf("\n");
    }
    if (!feof(stdin)) return fprintf(stderr, "case %ld: malformed header\n", cases), 2;
    return 0;
}
