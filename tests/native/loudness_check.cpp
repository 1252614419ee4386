// loudness_check — drives the host half of csrc/loudness.h for tests/test_loudness_cpu.py.  A plain host program: g++ -ffp-contract=off,
// once more with -fsanitize=address,undefined; nothing of it needs HIP.
//   loudness_check design RATE
//       -> one line: the design as hexadecimal bit patterns: 10 biquad coefficients, 16 entries of M, 49 taps, the step (decimal)
//   loudness_check run RATE N TOTAL GAIN TARGET CEILING FLAGS IN OUT
//       GAIN, TARGET, CEILING: f32 bit patterns in hexadecimal; IN: TOTAL raw f32 samples; OUT: receives TOTAL raw f32 samples, "-": meter only
//       -> one line: the result's fields as hexadecimal bit patterns in the order of zv_loudness_result (the counts in decimal)
//   loudness_check check GAIN TARGET CEILING FLAGS
//       -> the name of the field loud_check refuses, or "ok"
//   loudness_check bench RATE N REPS
//       -> the least time in ms of REPS runs of loud_reference (a meter) over N samples of noise
//   loudness_check plan RATE HOP T...
//       -> per T, for three utterances: ok, chunks, chunk workgroups, true-peak tiles, steps, apply tiles, phase-B workgroups, grid y
//   loudness_check groups HOP T...
//       -> one line: the end (one past the last utterance) of every launch group loud_group_end cuts the batch into, as loud_run walks it
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "loudness.h"
#include "stage_plan.h"

static float f32_arg(const char *s) { return zv::level_from_bits((uint32_t)strtoul(s, nullptr, 16)); }

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "design"))
    {
        zv::LoudFilter F;
        if (const char *field = zv::loud_design((uint32_t)strtoul(argv[2], nullptr, 10), &F))
        {
            printf("refused %s\n", field);
            return 0;
        }
        const double *d = F.shelf_b;      // the 26 doubles lie one behind the other
        static_assert(offsetof(zv::LoudFilter, c) == 26 * 8 && sizeof(zv::LoudFilter) == 26 * 8 + 50 * 4, "the layout of zv_loudness_filter");
        for (int i = 0; i < 26; i++) printf("%llx ", (unsigned long long)zv::loud_dbits(d[i]));
        for (int i = 0; i < zv::LOUD_TAPS; i++) printf("%x ", zv::level_bits(F.c[i]));
        printf("%u\n", F.step);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "check"))
    {
        const char *field = zv::loud_check(f32_arg(argv[2]), f32_arg(argv[3]), f32_arg(argv[4]), (uint32_t)strtoul(argv[5], nullptr, 10));
        printf("%s\n", field ? field : "ok");
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "plan"))
    {
        zv::LoudFilter F;
        if (zv::loud_design((uint32_t)strtoul(argv[2], nullptr, 10), &F)) return 2;
        const int hop = atoi(argv[3]);
        for (int i = 4; i < argc; i++)
        {
            const int T = atoi(argv[i]);
            const zv::LoudPlan p = zv::loud_plan((int64_t)T * hop, (int64_t)T * hop, 3, F.step);
            printf("%d %d %d %d %d %d %d %d\n", (int)p.ok, p.chunks, p.chunk_gx, p.tp_gx, p.steps, p.apply_gx, p.states_gx, p.gy);
        }
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "groups"))
    {
        const uint32_t hop = (uint32_t)strtoul(argv[2], nullptr, 10), n = (uint32_t)(argc - 3);
        std::vector<uint32_t> T(n);
        for (uint32_t u = 0; u < n; u++) T[u] = (uint32_t)strtoul(argv[3 + u], nullptr, 10);
        for (uint32_t g0 = 0; g0 < n;)
        {
            const uint32_t g1 = zv::loud_group_end(g0, n, T.data(), hop);
            if (g1 <= g0) return 4;      // a group without an utterance: the walk would never end
            printf("%u ", g1);
            g0 = g1;
        }
        printf("\n");
        return 0;
    }
    if (argc == 11 && !strcmp(argv[1], "run"))
    {
        zv::LoudFilter F;
        if (zv::loud_design((uint32_t)strtoul(argv[2], nullptr, 10), &F)) return 2;
        const uint64_t N = strtoull(argv[3], nullptr, 10), total = strtoull(argv[4], nullptr, 10);
        const float gain = f32_arg(argv[5]), target = f32_arg(argv[6]), ceiling = f32_arg(argv[7]);
        const uint32_t flags = (uint32_t)strtoul(argv[8], nullptr, 10);
        if (N > total || zv::loud_check(gain, target, ceiling, flags)) return 2;
        std::vector<float> x(total), y(total);
        FILE *f = fopen(argv[9], "rb");
        if (!f || fread(x.data(), 4, total, f) != total) return 3;
        fclose(f);
        const bool meter = !strcmp(argv[10], "-");
        const zv::LoudRow r = zv::loud_reference(F, x.data(), N, total, zv::loud_ask(gain, target, ceiling, flags), meter ? nullptr : y.data());
        if (!meter)
        {
            f = fopen(argv[10], "wb");
            if (!f || fwrite(y.data(), 4, total, f) != total) return 3;
            fclose(f);
        }
        printf("%llx %llx %llx %llx %u %u %u %x %x %x %x %x %x\n", (unsigned long long)zv::loud_dbits(r.integrated_ms),
               (unsigned long long)zv::loud_dbits(r.momentary_max_ms), (unsigned long long)zv::loud_dbits(r.short_term_max_ms),
               (unsigned long long)zv::loud_dbits(r.true_peak), r.blocks, r.blocks_absolute, r.blocks_gated, zv::level_bits(r.sample_peak),
               zv::level_bits(r.integrated_lufs), zv::level_bits(r.momentary_max_lufs), zv::level_bits(r.short_term_max_lufs),
               zv::level_bits(r.true_peak_dbtp), zv::level_bits(r.gain));
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "bench"))
    {
        zv::LoudFilter F;
        if (zv::loud_design((uint32_t)strtoul(argv[2], nullptr, 10), &F)) return 2;
        const uint64_t N = strtoull(argv[3], nullptr, 10);
        std::vector<float> x(N);
        uint32_t seed = 1;
        for (uint64_t i = 0; i < N; i++)
        {
            seed = seed * 1664525u + 1013904223u;
            x[i] = ((float)(seed >> 8) / 8388608.0f - 1.0f) * 0.1f;
        }
        double best = 1e300, sink = 0.0;
        for (int r = 0; r < atoi(argv[4]); r++)
        {
            const auto t0 = std::chrono::steady_clock::now();
            sink += zv::loud_reference(F, x.data(), N, N, zv::loud_ask(1.0f, 0.0f, 0.0f, 0u), nullptr).integrated_ms;
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            best = ms < best ? ms : best;
        }
        printf("%.3f %g\n", best, sink);
        return 0;
    }
    fprintf(stderr, "usage: loudness_check design|run|check|plan|groups|bench ...\n");
    return 1;
}
