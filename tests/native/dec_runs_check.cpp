// Host-side driver of csrc/dec_runs.h for tests/test_dec_runs_cpu.py (no GPU, no HIP).
//   dec_runs_check sweep TMAX R...
//       for every R given and every (n, T) with 1 <= n <= T <= TMAX: the run's bounds, the expansion map against a brute-force model
//       of which rows hold the same value, and the gap sum against the plain block-order sum, as f64 bits.  Prints "ok <cases> <taken>".
//   dec_runs_check rows T R N...
//       prints the compact rows summed over the utterances and how many of them take their run.
#include "dec_runs.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace zv;

#define CHECK(cond, ...)                                          \
    do                                                            \
    {                                                             \
        if (!(cond))                                              \
        {                                                         \
            printf("n %d T %d R %d: ", n, T, R);                  \
            printf(__VA_ARGS__);                                  \
            printf("\n");                                         \
            return 1;                                             \
        }                                                         \
    } while (0)

// The model: the decoder's input is zero from row n on and its 3-tap convs reach R rows, so a row of any of its tensors can differ
// from its neighbours only within R rows of the speech [0, n) or of the end T.  Rows in [n + R, T - R) all hold one value (id -1);
// every other row is taken to hold a value of its own (its index).
static int value_id(int t, int n, int T, int R) { return (t >= n + R && t < T - R) ? -1 : t; }

static uint64_t bits(double x)
{
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}

static int one(int n, int T, int R, std::mt19937_64 &rng, long *taken)
{
    const DecRun r = dec_run(n, T, R);
    const int a = r.gap_at * 32, b = a + r.G * 32;
    // an independent restatement of the rule
    const int a0 = (n + R + 32 + 31) / 32 * 32, b0 = T - R - 1 >= 0 ? (T - R - 1) / 32 * 32 : 0;
    const bool take0 = b0 - a0 >= 32 && b0 - a0 >= DEC_RUN_MARGIN;
    CHECK((r.G > 0) == take0, "taken %d, restated %d", r.G > 0, take0);
    CHECK(r.rows_c + 32 * r.G == T, "rows_c %d + 32 * %d != T", r.rows_c, r.G);
    if (r.G <= 0)
        CHECK(r.rows_c == T && r.G == 0 && r.gap_at == 0, "not taken is not (T, 0): rows_c %d gap_at %d G %d", r.rows_c, r.gap_at, r.G);
    else
    {
        ++*taken;
        CHECK(a == a0 && b == b0, "a %d b %d, restated %d %d", a, b, a0, b0);
        CHECK(a % 32 == 0 && b % 32 == 0, "a %d b %d not block multiples", a, b);
        CHECK(a - 32 >= n + R, "block in front of the gap [%d, %d) not constant", a - 32, a);
        CHECK(b <= T - R - 1, "b %d beyond T - R - 1", b);
        CHECK(32 * r.G >= DEC_RUN_MARGIN, "saves %d rows", 32 * r.G);
        CHECK(r.rows_c == a + (T - b), "rows_c %d", r.rows_c);
    }
    // the expansion map, and the compact segment as a sequence of its own
    for (int t = 0; t < T; t++)
    {
        const int c = dec_run_compact_row(t, r.gap_at, r.G);
        CHECK(c >= 0 && c < r.rows_c, "row %d -> compact row %d of %d", t, c, r.rows_c);
        const int o = dec_run_original_row(c, r.gap_at, r.G);
        CHECK(value_id(o, n, T, R) == value_id(t, n, T, R), "row %d reads compact row %d = original row %d: another value", t, c, o);
    }
    for (int c = 0; c < r.rows_c; c++)
    {
        const int o = dec_run_original_row(c, r.gap_at, r.G);
        CHECK(o >= 0 && o < T && dec_run_compact_row(o, r.gap_at, r.G) == c, "compact row %d <-> original row %d", c, o);
        CHECK((c == 0) == (o == 0) && (c == r.rows_c - 1) == (o == T - 1), "compact row %d / original row %d: sequence ends differ", c, o);
        // a compact neighbour holds what the original neighbour holds
        if (c > 0)
            CHECK(value_id(dec_run_original_row(c - 1, r.gap_at, r.G), n, T, R) == value_id(o - 1, n, T, R), "left neighbour of compact row %d", c);
        if (c + 1 < r.rows_c)
            CHECK(value_id(dec_run_original_row(c + 1, r.gap_at, r.G), n, T, R) == value_id(o + 1, n, T, R), "right neighbour of compact row %d", c);
    }
    // the gap sum: C channels side by side, random partials per compact block; the expanded array holds the block in front of the gap
    // in the gap's blocks
    const int C = 3, nbc = (r.rows_c + 31) / 32, nb = (T + 31) / 32;
    CHECK(nbc + r.G == nb, "blocks %d + %d != %d", nbc, r.G, nb);
    std::vector<double> pc((size_t)nbc * C * 2), pe((size_t)nb * C * 2);
    std::uniform_real_distribution<double> mant(-1.0, 1.0);
    std::uniform_int_distribution<int> expo(-20, 20);
    for (double &v : pc) v = ldexp(mant(rng), expo(rng));
    for (int j = 0; j < nb; j++)
    {
        const int src = j < r.gap_at || r.G == 0 ? j : (j < r.gap_at + r.G ? r.gap_at - 1 : j - r.G);
        memcpy(&pe[(size_t)j * C * 2], &pc[(size_t)src * C * 2], sizeof(double) * C * 2);
    }
    for (int ch = 0; ch < C; ch++)
    {
        double s1 = 0.0, s2 = 0.0, g1, g2, w1, w2;
        for (int j = 0; j < nb; j++)
        {
            s1 += pe[((size_t)j * C + ch) * 2];
            s2 += pe[((size_t)j * C + ch) * 2 + 1];
        }
        dec_run_block_sum(pc.data() + ch * 2, (size_t)C * 2, nbc, r.gap_at, r.G, &g1, &g2);
        CHECK(bits(g1) == bits(s1) && bits(g2) == bits(s2), "gap sum of channel %d: %a %a, plain %a %a", ch, g1, g2, s1, s2);
        dec_run_block_sum(pe.data() + ch * 2, (size_t)C * 2, nb, 0, 0, &w1, &w2);
        CHECK(bits(w1) == bits(s1) && bits(w2) == bits(s2), "sum without a gap of channel %d", ch);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "sweep"))
    {
        const int tmax = atoi(argv[2]);
        std::mt19937_64 rng(20240917);
        long cases = 0, taken = 0;
        for (int k = 3; k < argc; k++)
            for (int T = 1; T <= tmax; T++)
                for (int n = 1; n <= T; n++, cases++)
                    if (one(n, T, atoi(argv[k]), rng, &taken)) return 1;
        printf("ok %ld %ld\n", cases, taken);
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "rows"))
    {
        const int T = atoi(argv[2]), R = atoi(argv[3]);
        long rows = 0, taken = 0;
        for (int k = 4; k < argc; k++)
        {
            const DecRun r = dec_run(atoi(argv[k]), T, R);
            rows += r.rows_c;
            taken += r.G > 0;
        }
        printf("%ld %ld\n", rows, taken);
        return 0;
    }
    fprintf(stderr, "usage: see the head of tests/native/dec_runs_check.cpp\n");
    return 2;
}
