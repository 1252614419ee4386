// Host-side driver of densely packed decoding (csrc/dec_runs.h, csrc/conv_plan.h) for tests/test_dec_pack_cpu.py (no GPU, no HIP;
// linked with csrc/knobs.cpp).
//   dec_pack_check sweep R
//       batches of small (n, T) lists (T no multiple of 32, runs taken and not, empty batch): the slots are disjoint and in order,
//       every row0_p is a multiple of 32, every guard holds 1 .. 32 rows, L_p <= sum T + 32 nseg; a zero-padded 3-tap filter over
//       the packed array with zeros in the guards equals the per-utterance filter on every live row, as f32 bits; the pair of an
//       utterance's last, partial statistics block summed by dec_pack_tail_pair has the f64 bits of the conv epilogue's chains
//       over the live rows alone, though the packed block holds guard rows.  Prints "ok <batches> <utterances> <taken>".
//   dec_pack_check rows T R N...
//       prints L_p, the 256-row tiles of the packed rows and the 256-row tiles of the utterances tiled one by one.
//   dec_pack_check plan T NSEG L_CAP
//       the plans of the decoder's conv launches (medium checkpoint: 528 / 1 056 channels, 80 mels) over NSEG segments of T rows and
//       over ONE segment of L_CAP rows that holds NSEG utterances: prints "same <launches>" when every form, template argument, LDS
//       size and grid shape (y, z) agrees, the packed grids cover L_CAP rows, and the utterance count routes as conv_plan.h says.
#include "conv_plan.h"
#include "dec_runs.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace zv;

#define CHECK(cond, ...)              \
    do                                \
    {                                 \
        if (!(cond))                  \
        {                             \
            printf(__VA_ARGS__);      \
            printf("\n");             \
            return 1;                 \
        }                             \
    } while (0)

static uint32_t bits32(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}
static uint64_t bits64(double x)
{
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}

struct Utt
{
    int n, T;
};

// the table dec_runs_kernel writes in packed mode, restated serially
struct Packed
{
    std::vector<DecRun> r;
    std::vector<int>    row0;
    int                 L_p;
};
static Packed pack(const std::vector<Utt> &b, int R)
{
    Packed p;
    p.L_p = 0;
    for (const Utt &u : b)
    {
        p.r.push_back(dec_run(u.n, u.T, R));
        p.row0.push_back(p.L_p);
        p.L_p += dec_pack_slot(p.r.back().rows_c);
    }
    return p;
}

// the conv epilogue's chains (mfma_common.h tile_stats_store) over one 32-row block of which `rows` rows count, written out apart
// from dec_pack_tail_pair: lanes 0-31 walk their 16 rows in register order, lanes 32-63 theirs, then the two are added
static void epilogue_pair(const float *x, int rows, double *sum, double *sumsq)
{
    double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int r = 0; r < 16; r++)
    {
        const int ta = (r & 3) + 8 * (r >> 2), tb = 4 + ta;
        const double xa = ta < rows ? (double)x[ta] : 0.0, xb = tb < rows ? (double)x[tb] : 0.0;
        a1 += xa, a2 += xa * xa;
        b1 += xb, b2 += xb * xb;
    }
    *sum = a1 + b1;
    *sumsq = a2 + b2;
}

static int one_batch(const std::vector<Utt> &b, int R, std::mt19937 &rng, long *taken)
{
    const Packed p = pack(b, R);
    long sumT = 0;
    for (size_t u = 0; u < b.size(); u++)
    {
        const int rows_c = p.r[u].rows_c, slot = dec_pack_slot(rows_c);
        sumT += b[u].T;
        *taken += p.r[u].G > 0;
        CHECK(p.row0[u] % 32 == 0, "utterance %zu: row0_p %d", u, p.row0[u]);
        CHECK(slot % 32 == 0 && slot - rows_c >= 1 && slot - rows_c <= 32, "utterance %zu: %d rows in a slot of %d", u, rows_c, slot);
        CHECK((rows_c % 32 == 0) == (slot - rows_c == 32), "utterance %zu: guard of %d rows behind %d", u, slot - rows_c, rows_c);
        CHECK(u + 1 == b.size() ? p.row0[u] + slot == p.L_p : p.row0[u] + slot == p.row0[u + 1], "utterance %zu: slots not back to back", u);
    }
    CHECK(p.L_p <= dec_pack_rows_cap(sumT, (int)b.size()), "L_p %d > %ld + 32 * %zu", p.L_p, sumT, b.size());
    // the 3-tap filter: y[t] = (w0 x[t - 1] + w1 x[t]) + w2 x[t + 1], rows outside the sequence zero — per utterance over its compact
    // rows, and once over the packed rows [0, L_p) with zeros in the guards and garbage nowhere else to hide
    std::uniform_real_distribution<float> val(-2.f, 2.f);
    const float w[3] = {val(rng), val(rng), val(rng)};
    std::vector<float> xp((size_t)p.L_p, 0.f), yp((size_t)p.L_p);
    std::vector<std::vector<float>> xs(b.size());
    for (size_t u = 0; u < b.size(); u++)
    {
        xs[u].resize((size_t)p.r[u].rows_c);
        for (int t = 0; t < p.r[u].rows_c; t++) xp[(size_t)p.row0[u] + t] = xs[u][t] = val(rng);
    }
    auto filt = [&](const float *x, int L, int t) {
        const float l = t > 0 ? x[t - 1] : 0.f, r = t + 1 < L ? x[t + 1] : 0.f;
        return (w[0] * l + w[1] * x[t]) + w[2] * r;
    };
    for (int t = 0; t < p.L_p; t++) yp[t] = filt(xp.data(), p.L_p, t);
    for (size_t u = 0; u < b.size(); u++)
        for (int t = 0; t < p.r[u].rows_c; t++)
            CHECK(bits32(filt(xs[u].data(), p.r[u].rows_c, t)) == bits32(yp[(size_t)p.row0[u] + t]), "utterance %zu row %d: packed filter differs", u, t);
    // the last, partial statistics block: the packed conv's output has garbage in its guard rows (yp there is not zero: the filter
    // reaches the last live row), the pair must count the live rows alone
    for (size_t u = 0; u < b.size(); u++)
    {
        const int rows_c = p.r[u].rows_c, tail = rows_c & 31;
        if (!tail) continue;
        const float *blk = yp.data() + p.row0[u] + (rows_c & ~31);
        float live[32] = {0};
        for (int t = 0; t < tail; t++) live[t] = blk[t];
        double s1, s2, e1, e2;
        dec_pack_tail_pair(blk, 1, tail, &s1, &s2);
        epilogue_pair(live, tail, &e1, &e2);
        CHECK(bits64(s1) == bits64(e1) && bits64(s2) == bits64(e2), "utterance %zu: tail pair %a %a, epilogue %a %a", u, s1, s2, e1, e2);
    }
    return 0;
}

// the decoder's conv launches on the medium checkpoint (decoder.cpp): (taps, Cin_p, Cout_p, f16 operand + conv_gemm pack, statistics, residual)
struct DecConv
{
    int  K, cin, cout;
    bool f16op, stat, res;
};
static const DecConv DEC_CONVS[] = {
    {3, 528, 528, true, true, false},   {3, 528, 1056, true, true, true},   {1, 528, 1056, true, false, false},  {3, 1056, 1056, true, true, false},
    {3, 1056, 1056, true, true, true},  {1, 528, 64, false, true, false},   {3, 1120, 1056, true, true, false},  {1, 1120, 1056, true, false, false},
    {3, 1120, 528, true, true, false},  {1, 1120, 528, true, false, false}, {3, 528, 528, true, true, true},     {3, 528, 528, true, false, true},
    {1, 528, 80, false, false, false},
};

static ConvDesc desc(const DecConv &c)
{
    return ConvDesc{c.K, 1, (c.K - 1) / 2, c.cin, c.cout, 256, c.f16op ? PRO_RAW_F16 : PRO_ACT, c.cin, c.f16op, false, c.res, c.stat, false, false};
}

// what of a plan names the kernel: form, template arguments, threads, LDS, the map over the XCDs, grid.y / grid.z — not grid.x, not tps
static bool same_kernel(const ConvPlan &a, const ConvPlan &b)
{
    return a.valid && b.valid && a.form == b.form && a.MT == b.MT && a.WN == b.WN && a.NT == b.NT && a.strip == b.strip && a.nkc == b.nkc &&
           a.gy == b.gy && a.gz == b.gz && a.threads == b.threads && a.lds_bytes == b.lds_bytes && a.tile_bytes == b.tile_bytes &&
           a.xcd_ny == b.xcd_ny && a.xcd_spread == b.xcd_spread && a.warm == b.warm;
}

static int plan(int T, int nseg, int L_cap)
{
    knob_reset();
    int launches = 0;
    for (const DecConv &c : DEC_CONVS)
    {
        const ConvDesc d = desc(c);
        const ConvCall today{1, nseg, T, 1, 256, 0, 0}, packed{1, 1, L_cap, 1, 256, 0, nseg};
        const bool g = conv_gemm_takes(d, today);
        CHECK(g == conv_gemm_takes(d, packed), "conv %d x %d -> %d: conv_gemm_kernel takes it in one layout only", c.K, c.cin, c.cout);
        int nt_begin = 0;
        if (g)
        {
            const ConvGemmPlan a = conv_gemm_plan(c.cout, today), b = conv_gemm_plan(c.cout, packed);
            CHECK(a.order == b.order && a.threads == b.threads && a.lds_bytes == b.lds_bytes, "conv_gemm_plan of %d channels", c.cout);
            CHECK(b.tps * 256 >= L_cap && b.gx >= b.tps * conv_gemm_groups(c.cout), "conv_gemm_plan's grid does not cover %d rows", L_cap);
            launches++;
            nt_begin = conv_gemm_tiles(c.cout);
            if (nt_begin * 32 >= c.cout) continue;
        }
        ConvCall a = today, b = packed;
        a.nt_begin = b.nt_begin = nt_begin;
        const ConvPlan pa = conv_plan(&d, a), pb = conv_plan(&d, b);
        CHECK(same_kernel(pa, pb), "conv %d x %d -> %d from tile %d: form %d <%d,%d,%d> today, %d <%d,%d,%d> packed", c.K, c.cin, c.cout, nt_begin,
              pa.form, pa.MT, pa.WN, pa.NT, pb.form, pb.MT, pb.WN, pb.NT);
        CHECK((long)pb.tps * (pb.form == CONV_STREAM ? 64 * pb.strip : 32 * pb.MT * (4 / pb.WN)) >= L_cap, "row tiles do not cover %d rows", L_cap);
        launches++;
    }
    // the utterance count is what routes: the output conv over one segment of 16 384 rows (two rounds of the loader-wave form's
    // workgroups) keeps that form as one utterance and takes the ordinary one as a batch; over 4 096 rows it keeps the form either way
    // and a batch is dealt by the spread map
    {
        const ConvDesc d = desc(DecConv{1, 528, 80, false, false, false});
        const ConvPlan one = conv_plan(&d, ConvCall{1, 1, 16384, 1, 256, 0, 0}), many = conv_plan(&d, ConvCall{1, 1, 16384, 1, 256, 0, 2});
        CHECK(one.valid && many.valid && one.form == CONV_LOADER && many.form == CONV_TILED, "16 384 rows: forms %d, %d", one.form, many.form);
        const ConvPlan s1 = conv_plan(&d, ConvCall{1, 1, 4096, 1, 256, 0, 0}), s2 = conv_plan(&d, ConvCall{1, 1, 4096, 1, 256, 0, 2});
        CHECK(s1.form == CONV_LOADER && s2.form == CONV_LOADER && s1.xcd_spread == 0 && s2.xcd_spread == 1, "4 096 rows: spread %d, %d", s1.xcd_spread, s2.xcd_spread);
    }
    // (a default-built ConvCall carries the scope's count, and 0 outside one)
    CHECK((ConvCall{1, 1, 1, 1, 1, 0}.nutt) == 0, "utterance count outside a scope");
    {
        const ConvPackedUtts scope(nseg);
        CHECK((ConvCall{1, 1, 1, 1, 1, 0}.nutt) == nseg, "utterance count inside a scope");
    }
    CHECK((ConvCall{1, 1, 1, 1, 1, 0}.nutt) == 0, "utterance count behind a scope");
    printf("same %d\n", launches);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "sweep"))
    {
        const int R = atoi(argv[2]);
        std::mt19937 rng(20250311);
        long batches = 0, utts = 0, taken = 0;
        {
            const std::vector<Utt> none;
            if (one_batch(none, R, rng, &taken)) return 1;
            batches++;
        }
        // every pair and a sample of triples of (n, T) over a grid that has T around the block multiples and n on both sides of a run
        const int Ts[] = {1, 31, 32, 33, 64, 100, 110, 111, 128, 130, 160, 161, 200, 352};
        std::vector<Utt> all;
        for (int T : Ts)
            for (int n : {1, 9, 18, 19, 40, T / 2, T - 1, T})
                if (n >= 1 && n <= T) all.push_back(Utt{n, T});
        for (const Utt &a : all)
        {
            if (one_batch({a}, R, rng, &taken)) return 1;
            batches++, utts++;
            for (const Utt &b : all)
            {
                if (one_batch({a, b}, R, rng, &taken)) return 1;
                batches++, utts += 2;
            }
        }
        std::uniform_int_distribution<size_t> pick(0, all.size() - 1);
        for (int k = 0; k < 2000; k++)
        {
            std::vector<Utt> b(3 + k % 6);
            for (Utt &u : b) u = all[pick(rng)];
            if (one_batch(b, R, rng, &taken)) return 1;
            batches++, utts += (long)b.size();
        }
        printf("ok %ld %ld %ld\n", batches, utts, taken);
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "rows"))
    {
        const int T = atoi(argv[2]), R = atoi(argv[3]);
        std::vector<Utt> b;
        for (int k = 4; k < argc; k++) b.push_back(Utt{atoi(argv[k]), T});
        const Packed p = pack(b, R);
        long alone = 0;
        for (const DecRun &r : p.r) alone += (r.rows_c + 255) / 256;
        printf("%d %d %ld\n", p.L_p, (p.L_p + 255) / 256, alone);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "plan")) return plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    fprintf(stderr, "usage: see the head of tests/native/dec_pack_check.cpp\n");
    return 2;
}
