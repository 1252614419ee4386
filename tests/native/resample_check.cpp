// resample_check — drives the host half of csrc/resample.h for tests/test_resample_cpu.py.  A plain host program: g++ -ffp-contract=off,
// once more with -fsanitize=address,undefined; nothing of it needs HIP.
//   resample_check design RATE_IN RATE_OUT ZEROS BETA CUTOFF [TABLE]      (BETA, CUTOFF: f32 bit patterns in hexadecimal)
//       -> "L M P", or "refused FIELD"; TABLE receives L * P raw f32 entries
//   resample_check run L M P FLAGS SEED TABLE S_IN IN OUT PCM
//       TABLE: L * P raw f32 entries; IN: S_IN raw f32 samples; OUT receives n_out raw f32 samples, PCM n_out raw int16 samples
//       -> one line: n_out and clipped in decimal, sample_peak as a hexadecimal bit pattern
//   resample_check self
//       -> resample_reference against a restatement with every loop written out, on random and adversarial inputs: "ok CASES"
//   resample_check check L M P [TABLE]
//       -> the name of what resample_check_shape (with TABLE: resample_check_table) refuses, or "ok"
//   resample_check plan MAX_N_OUT NSEG L M P
//       -> ok, grid x, grid y, and the tile: slots S, input advance D, outputs per slot R
//   resample_check groups L M S_IN...
//       -> one line: the end of every launch group, as resample_run walks the batch (resample_group_end)
//   resample_check bench L M P S_IN REPS
//       -> the least time in ms of REPS runs of resample_reference (f32 and PCM16 with dither) over S_IN samples of noise
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "resample.h"
#include "stage_plan.h"

static float f32_arg(const char *s) { return zv::level_from_bits((uint32_t)strtoul(s, nullptr, 16)); }
static uint32_t u32_arg(const char *s) { return (uint32_t)strtoul(s, nullptr, 10); }

static uint32_t lcg(uint32_t &seed)
{
    seed = seed * 1664525u + 1013904223u;
    return seed >> 8;
}

static bool read_file(const char *path, void *dst, size_t size, size_t n)
{
    FILE *f = fopen(path, "rb");
    const bool ok = f && fread(dst, size, n, f) == n;
    if (f) fclose(f);
    return ok;
}
static bool write_file(const char *path, const void *src, size_t size, size_t n)
{
    FILE *f = fopen(path, "wb");
    const bool ok = f && fwrite(src, size, n, f) == n;
    return (f && fclose(f) == 0) && ok;
}

// The rule with every loop written out and nothing shared with resample_reference but the types: the time of an output is walked (p
// advances by M, every L of it is one input sample), the count is found by walking until the time leaves [0, S_in), a step is a product
// and a sum, the PCM16 conversion and the hash are spelt out, the peak is a comparison of magnitudes.
static bool brute_equals(const std::vector<float> &h, uint32_t L, uint32_t M, uint32_t P, const std::vector<float> &x, uint32_t flags, uint32_t seed,
                         const char *what)
{
    const long S = (long)x.size(), half = P / 2;
    const uint64_t want_n = zv::resample_count((uint64_t)S, L, M);
    std::vector<float> out(want_n + 1, 123.0f);
    std::vector<int16_t> pcm(want_n + 1, 77);
    const zv::ResampleRow r = zv::resample_reference(h.data(), L, M, P, x.data(), (uint64_t)S, flags, seed, out.data(), pcm.data());
    if (out[want_n] != 123.0f || pcm[want_n] != 77) return fprintf(stderr, "%s: wrote past n_out\n", what), false;
    uint64_t n = 0, clipped = 0;
    float peak = 0.0f;
    long i0 = 0;
    uint32_t p = 0;
    while (i0 < S)      // n M / L < S_in
    {
        double acc = 0.0;
        for (long k = 0; k < (long)P; k++)
        {
            const long j = i0 - half + 1 + k;
            double v = 0.0;
            if (j >= 0 && j < S && x[(size_t)j] == x[(size_t)j] && x[(size_t)j] - x[(size_t)j] == 0.0f) v = (double)x[(size_t)j];
            const double prod = (double)h[(size_t)p * P + (size_t)k] * v;
            acc = acc + prod;
        }
        const float y = (float)acc;
        if (n >= want_n) return fprintf(stderr, "%s: more outputs than n_out = %llu\n", what, (unsigned long long)want_n), false;
        if (memcmp(&y, &out[n], 4)) return fprintf(stderr, "%s: y[%llu] = %a, reference %a\n", what, (unsigned long long)n, y, out[n]), false;
        if (y - y == 0.0f && fabsf(y) > peak) peak = fabsf(y);
        double z = (double)y * 32768.0;
        if (flags & 1u)
        {
            uint64_t rr = ((uint64_t)seed + (n % 4294967296ull) * 0x9E3779B9ull) % 4294967296ull;
            rr = rr ^ (rr >> 16);
            rr = rr * 0x7feb352dull % 4294967296ull;
            rr = rr ^ (rr >> 15);
            rr = rr * 0x846ca68bull % 4294967296ull;
            rr = rr ^ (rr >> 16);
            const double lo = (double)(rr % 65536ull), hi = (double)(rr / 65536ull);
            double d = lo + hi;
            d = d - 65535.0;
            d = d / 65536.0;
            z = z + d;
        }
        z = z + 0.5;
        long q = 0;
        bool clip = false;
        if (z != z) clip = true;
        else if (z >= 32768.0) q = 32767, clip = true;
        else if (z < -32768.0) q = -32768, clip = true;
        else q = (long)floor(z);
        clipped += clip;
        if ((long)pcm[n] != q) return fprintf(stderr, "%s: pcm[%llu] = %ld, reference %d\n", what, (unsigned long long)n, q, (int)pcm[n]), false;
        n++;
        p += M;
        while (p >= L) p -= L, i0++;
    }
    if (n != want_n || r.n_out != want_n) return fprintf(stderr, "%s: n_out %llu, walked %llu\n", what, (unsigned long long)r.n_out, (unsigned long long)n), false;
    if (r.clipped != clipped) return fprintf(stderr, "%s: clipped %llu, counted %llu\n", what, (unsigned long long)r.clipped, (unsigned long long)clipped), false;
    if (memcmp(&r.sample_peak, &peak, 4)) return fprintf(stderr, "%s: sample_peak %a, found %a\n", what, r.sample_peak, peak), false;
    // the outputs asked for one at a time give the same report; no pcm: clipped 0
    const zv::ResampleRow a = zv::resample_reference(h.data(), L, M, P, x.data(), (uint64_t)S, flags, seed, out.data(), nullptr);
    const zv::ResampleRow b = zv::resample_reference(h.data(), L, M, P, x.data(), (uint64_t)S, flags, seed, nullptr, pcm.data());
    if (a.clipped != 0 || b.clipped != clipped || a.n_out != want_n || b.n_out != want_n || memcmp(&a.sample_peak, &peak, 4) || memcmp(&b.sample_peak, &peak, 4))
        return fprintf(stderr, "%s: the report depends on the outputs asked for\n", what), false;
    return true;
}

static int self_check()
{
    static const uint32_t shapes[][3] = {{1, 1, 2}, {3, 2, 4}, {2, 3, 6}, {7, 1, 2}, {1, 6, 16}, {320, 147, 8}, {160, 441, 24}, {1280, 441, 2}, {1, 1, 512},
                                         {8, 1, 4}, {1, 8, 64}};
    uint32_t seed = 99;
    int cases = 0;
    for (const auto &sh : shapes)
    {
        const uint32_t L = sh[0], M = sh[1], P = sh[2];
        if (zv::resample_check_shape(L, M, P)) return fprintf(stderr, "shape %u %u %u refused\n", L, M, P), 1;
        std::vector<float> h((size_t)L * P);
        for (float &v : h) v = ((float)lcg(seed) / 8388608.0f - 1.0f) * (lcg(seed) % 7 == 0 ? 0.0f : 1.5f);
        for (long S : {1l, 2l, (long)P / 2 - 1, (long)P / 2, 37l, 700l})
        {
            if (S < 1) continue;
            for (int kind = 0; kind < 4; kind++)
            {
                std::vector<float> x((size_t)S);
                for (float &v : x) v = kind == 1 ? 0.0f : ((float)lcg(seed) / 8388608.0f - 1.0f) * (kind == 2 ? 3.0f : 0.4f);
                if (kind == 3)
                {
                    x[0] = NAN, x[(size_t)S - 1] = -INFINITY;
                    if (S > 4) x[(size_t)S / 2] = INFINITY, x[(size_t)S / 2 + 1] = -0.0f, x[1] = 3.0e38f;
                }
                char what[96];
                snprintf(what, sizeof what, "L %u M %u P %u S %ld kind %d", L, M, P, S, kind);
                for (uint32_t flags = 0; flags < 2; flags++)
                    for (uint32_t sd : {0u, 1u, 0xFFFFFFFFu})
                        if (!brute_equals(h, L, M, P, x, flags, sd, what)) return 1;
                cases++;
            }
        }
    }
    printf("ok %d\n", cases);
    return 0;
}

int main(int argc, char **argv)
{
    if ((argc == 7 || argc == 8) && !strcmp(argv[1], "design"))
    {
        uint32_t L = 0, M = 0, P = 0;
        const uint32_t ri = u32_arg(argv[2]), ro = u32_arg(argv[3]), zeros = u32_arg(argv[4]);
        const float beta = f32_arg(argv[5]), cutoff = f32_arg(argv[6]);
        if (const char *field = zv::resample_design(ri, ro, zeros, beta, cutoff, &L, &M, &P, nullptr))
        {
            printf("refused %s\n", field);
            return 0;
        }
        if (argc == 8)
        {
            std::vector<float> t((size_t)L * P);
            if (zv::resample_design(ri, ro, zeros, beta, cutoff, &L, &M, &P, t.data())) return 2;
            if (!write_file(argv[7], t.data(), 4, t.size())) return 3;
        }
        printf("%u %u %u\n", L, M, P);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "self")) return self_check();
    if ((argc == 5 || argc == 6) && !strcmp(argv[1], "check"))
    {
        const uint32_t L = u32_arg(argv[2]), M = u32_arg(argv[3]), P = u32_arg(argv[4]);
        const char *field = zv::resample_check_shape(L, M, P);
        if (!field && argc == 6)
        {
            std::vector<float> t((size_t)L * P);
            if (!read_file(argv[5], t.data(), 4, t.size())) return 3;
            field = zv::resample_check_table(t.data(), L, M, P);
        }
        printf("%s\n", field ? field : "ok");
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "plan"))
    {
        const zv::ResamplePlan p = zv::resample_plan(strtoll(argv[2], nullptr, 10), atoi(argv[3]), u32_arg(argv[4]), u32_arg(argv[5]), u32_arg(argv[6]));
        printf("%d %d %d %d %d %d\n", (int)p.ok, p.gx, p.gy, p.tile.S, p.tile.D, p.tile.R);
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "groups"))
    {
        const uint32_t L = u32_arg(argv[2]), M = u32_arg(argv[3]), n = (uint32_t)(argc - 4);
        std::vector<uint64_t> S(n);
        for (uint32_t u = 0; u < n; u++) S[u] = strtoull(argv[4 + u], nullptr, 10);
        for (uint32_t g0 = 0; g0 < n;)
        {
            const uint32_t g1 = zv::resample_group_end(g0, n, S.data(), L, M);
            if (g1 <= g0) return 4;      // a group without an utterance: the walk would never end
            printf("%u ", g1);
            g0 = g1;
        }
        printf("\n");
        return 0;
    }
    if (argc == 12 && !strcmp(argv[1], "run"))
    {
        const uint32_t L = u32_arg(argv[2]), M = u32_arg(argv[3]), P = u32_arg(argv[4]), flags = u32_arg(argv[5]), seed = u32_arg(argv[6]);
        if (zv::resample_check_shape(L, M, P) || (flags & ~1u)) return 2;
        std::vector<float> t((size_t)L * P);
        if (!read_file(argv[7], t.data(), 4, t.size())) return 3;
        if (zv::resample_check_table(t.data(), L, M, P)) return 2;
        const uint64_t S = strtoull(argv[8], nullptr, 10), n_out = zv::resample_count(S, L, M);
        std::vector<float> x(S), y(n_out);
        std::vector<int16_t> q(n_out);
        if (!read_file(argv[9], x.data(), 4, S)) return 3;
        const zv::ResampleRow r = zv::resample_reference(t.data(), L, M, P, x.data(), S, flags, seed, y.data(), q.data());
        if (!write_file(argv[10], y.data(), 4, n_out) || !write_file(argv[11], q.data(), 2, n_out)) return 3;
        printf("%llu %llu %x\n", (unsigned long long)r.n_out, (unsigned long long)r.clipped, zv::level_bits(r.sample_peak));
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "bench"))
    {
        const uint32_t L = u32_arg(argv[2]), M = u32_arg(argv[3]), P = u32_arg(argv[4]);
        if (zv::resample_check_shape(L, M, P)) return 2;
        const uint64_t S = strtoull(argv[5], nullptr, 10), n_out = zv::resample_count(S, L, M);
        std::vector<float> t((size_t)L * P, 1.0f / (float)P), x(S), y(n_out);
        std::vector<int16_t> q(n_out);
        uint32_t seed = 1;
        for (uint64_t i = 0; i < S; i++) x[i] = ((float)lcg(seed) / 8388608.0f - 1.0f) * 0.1f;
        double best = 1e300, sink = 0.0;
        for (int r = 0; r < atoi(argv[6]); r++)
        {
            const auto t0 = std::chrono::steady_clock::now();
            sink += zv::resample_reference(t.data(), L, M, P, x.data(), S, 1u, 0u, y.data(), q.data()).sample_peak;
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            best = ms < best ? ms : best;
        }
        printf("%.3f %g\n", best, sink);
        return 0;
    }
    fprintf(stderr, "usage: resample_check design|run|self|check|plan|groups|bench ...\n");
    return 1;
}
