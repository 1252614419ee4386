// limiter_check — drives the host half of csrc/limiter.h for tests/test_limiter_cpu.py.  A plain host program: g++ -ffp-contract=off,
// once more with -fsanitize=address,undefined; nothing of it needs HIP.
//   limiter_check taps RATE
//       -> one line: the 49 taps of the loudness design's interpolator as hexadecimal f32 bit patterns
//   limiter_check design RATE ATTACK_MS RELEASE_MS         (f32 bit patterns in hexadecimal)
//       -> "attack release", or "refused FIELD"
//   limiter_check run RATE N TOTAL GAIN CEILING ATTACK RELEASE IN OUT S
//       GAIN, CEILING: f32 bit patterns in hexadecimal; IN: TOTAL raw f32 samples; OUT: receives TOTAL raw f32 samples, S TOTAL raw u32 s_n
//       -> one line: the result's fields as hexadecimal bit patterns in the order of zv_limit_result (the count in decimal)
//   limiter_check self
//       -> limit_reference against a restatement with every window loop written out, on random and adversarial inputs: "ok CASES"
//   limiter_check check GAIN CEILING ATTACK RELEASE FLAGS
//       -> the name of the field limit_check refuses, or "ok"
//   limiter_check plan NSEG MAX_HALO MAX_TOTAL MAX_QLEN
//       -> ok, peak tiles, minimum tiles, mean tiles, grid y, staged entries, LDS bytes of the minimum and of the mean pass
//   limiter_check groups HOP T...
//       -> one line: the end of every launch group, as limit_run walks the batch (loud_group_end)
//   limiter_check bench RATE N ATTACK RELEASE REPS
//       -> the least time in ms of REPS runs of limit_reference over N samples of noise driven 12 dB over the ceiling
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "limiter.h"
#include "stage_plan.h"

static float f32_arg(const char *s) { return zv::level_from_bits((uint32_t)strtoul(s, nullptr, 16)); }

static uint32_t lcg(uint32_t &seed)
{
    seed = seed * 1664525u + 1013904223u;
    return seed >> 8;
}

// the rule with every window loop written out: p through loud_tp_phase per sample, q per sample, m and s by their definitions
static bool brute_equals(const zv::LoudFilter &F, const std::vector<float> &x, int64_t N, const zv::LimitAsk &a, const char *what)
{
    const int64_t total = (int64_t)x.size(), A = a.attack, R = a.release, W = A + R + 1;
    auto xs = [&](int64_t n) { return n >= 0 && n < N ? zv::loud_sample(x[(size_t)n]) : 0.0; };
    auto p = [&](int64_t m) {
        if (m < -6 || m > N + 4) return 0.0;
        double w[zv::LOUD_PHASE_TAPS], best = fabs(xs(m));
        for (int k = 0; k < zv::LOUD_PHASE_TAPS; k++) w[k] = xs(m + 6 - k);
        for (int f = 1; f < 4; f++)
        {
            const double v = fabs(zv::loud_tp_phase(F.c, f, w));
            best = v > best ? v : best;
        }
        return best;
    };
    std::vector<uint32_t> q((size_t)(total + 2 * (A + R)));
    for (int64_t j = -(A + R); j < total + A + R; j++) q[(size_t)(j + A + R)] = zv::limit_q(a.gain, a.ceiling, p(j));
    auto qj = [&](int64_t j) { return q[(size_t)(j + A + R)]; };
    std::vector<float> out((size_t)total), want((size_t)total);
    std::vector<uint32_t> s;
    const zv::LimitRow r = zv::limit_reference(F, x.data(), (uint64_t)N, (uint64_t)total, a, out.data(), &s);
    uint32_t min_s = zv::LIMIT_ONE;
    uint64_t limited = 0;
    double tp = 0.0;
    for (int64_t m = -6; m <= N + 4; m++) tp = p(m) > tp ? p(m) : tp;
    for (int64_t n = 0; n < total; n++)
    {
        uint64_t sum = 0;
        for (int64_t k = n - A; k <= n + R; k++)
        {
            uint32_t mk = 0xffffffffu;
            for (int64_t j = k - R; j <= k + A; j++) mk = qj(j) < mk ? qj(j) : mk;
            sum += mk;
        }
        const uint32_t sn = (uint32_t)(sum / (uint64_t)W);
        if (sn != s[(size_t)n] || sn > qj(n))
        {
            printf("%s: s[%lld] = %u, the loops give %u, q = %u\n", what, (long long)n, s[(size_t)n], sn, qj(n));
            return false;
        }
        want[(size_t)n] = zv::limit_apply(x[(size_t)n], a.gain, sn);
        if (zv::level_bits(want[(size_t)n]) != zv::level_bits(out[(size_t)n]))
        {
            printf("%s: out[%lld] differs\n", what, (long long)n);
            return false;
        }
        if (n < N)
        {
            min_s = sn < min_s ? sn : min_s;
            limited += sn < zv::LIMIT_ONE;
            if (zv::loud_finite(out[(size_t)n]) && !(fabsf(out[(size_t)n]) <= a.ceiling))
            {
                printf("%s: |out[%lld]| = %g passes the ceiling %g\n", what, (long long)n, (double)fabsf(out[(size_t)n]), (double)a.ceiling);
                return false;
            }
        }
    }
    const zv::LoudRow loud = zv::loud_reference(F, x.data(), (uint64_t)N, (uint64_t)total, zv::loud_ask(1.0f, 0.0f, 0.0f, 0u), nullptr);
    if (zv::loud_dbits(tp) != zv::loud_dbits(r.true_peak_before) || zv::loud_dbits(loud.true_peak) != zv::loud_dbits(r.true_peak_before) ||
        zv::level_bits(loud.sample_peak) != zv::level_bits(r.sample_peak_before) || limited != r.limited_samples ||
        zv::level_bits(r.min_gain) != zv::level_bits((float)((double)min_s * ldexp(1.0, -30))))
    {
        printf("%s: the report differs\n", what);
        return false;
    }
    return true;
}

static int self_check()
{
    zv::LoudFilter F;
    if (zv::loud_design(22050, &F)) return 2;
    uint32_t seed = 7;
    int cases = 0;
    const uint32_t windows[][2] = {{1, 1}, {1, 5}, {4, 2}, {7, 20}, {33, 60}};
    for (const auto &w : windows)
        for (int shape = 0; shape < 8; shape++)
        {
            const int64_t total = 40 + (int64_t)(lcg(seed) % 300), N = shape == 6 ? 0 : shape == 7 ? total : (int64_t)(lcg(seed) % (uint32_t)(total + 1));
            std::vector<float> x((size_t)total);
            for (auto &v : x) v = ((float)lcg(seed) / 8388608.0f - 1.0f) * (shape == 1 ? 1.0f : 0.2f);
            const int64_t W = w[0] + w[1] + 1;
            if (shape == 2 && N > 0) x[0] = 0.95f, x[(size_t)(N - 1)] = -0.97f;                  // peaks in the first and the last sample of the span
            if (shape == 3 && total > W + 5) x[3] = 0.9f, x[(size_t)(3 + W)] = 0.8f;             // two peaks exactly W apart
            if (shape == 3 && total > 2 * W + 9) x[(size_t)(2 * W + 7)] = 0.7f, x[(size_t)(2 * W + 8)] = -0.99f;
            if (shape == 4)
                for (auto &v : x) v = v < 0.0f ? -1.0f : 1.0f;                                   // a full-scale square wave
            if (shape == 5) x[5] = NAN, x[9] = INFINITY, x[10] = -INFINITY, x[20] = 0.9f;
            const zv::LimitAsk a{shape == 0 ? 0.0f : shape == 1 ? 1000.0f : 1.5f, shape == 4 ? 0.25f : 0.5f, w[0], w[1]};
            char what[64];
            snprintf(what, sizeof what, "attack %u release %u shape %d", w[0], w[1], shape);
            if (!brute_equals(F, x, N, a, what)) return 1;
            cases++;
        }
    printf("ok %d\n", cases);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "taps"))
    {
        zv::LoudFilter F;
        if (zv::loud_design((uint32_t)strtoul(argv[2], nullptr, 10), &F)) return 2;
        for (int i = 0; i < zv::LOUD_TAPS; i++) printf("%x ", zv::level_bits(F.c[i]));
        printf("\n");
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "design"))
    {
        uint32_t a = 0, r = 0;
        if (const char *field = zv::limit_design((uint32_t)strtoul(argv[2], nullptr, 10), f32_arg(argv[3]), f32_arg(argv[4]), &a, &r))
            printf("refused %s\n", field);
        else
            printf("%u %u\n", a, r);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "self")) return self_check();
    if (argc == 7 && !strcmp(argv[1], "check"))
    {
        const char *field = zv::limit_check(f32_arg(argv[2]), f32_arg(argv[3]), (uint32_t)strtoul(argv[4], nullptr, 10),
                                            (uint32_t)strtoul(argv[5], nullptr, 10), (uint32_t)strtoul(argv[6], nullptr, 10));
        printf("%s\n", field ? field : "ok");
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "plan"))
    {
        const zv::LimitPlan p = zv::limit_plan(strtoll(argv[5], nullptr, 10), strtoll(argv[4], nullptr, 10), atoi(argv[3]), atoi(argv[2]));
        printf("%d %d %d %d %d %d %zu %zu\n", (int)p.ok, p.peak_gx, p.min_gx, p.mean_gx, p.gy, p.stage, p.min_lds, p.mean_lds);
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
    if (argc == 12 && !strcmp(argv[1], "run"))
    {
        zv::LoudFilter F;
        if (zv::loud_design((uint32_t)strtoul(argv[2], nullptr, 10), &F)) return 2;
        const uint64_t N = strtoull(argv[3], nullptr, 10), total = strtoull(argv[4], nullptr, 10);
        const zv::LimitAsk a{f32_arg(argv[5]), f32_arg(argv[6]), (uint32_t)strtoul(argv[7], nullptr, 10), (uint32_t)strtoul(argv[8], nullptr, 10)};
        if (N > total || zv::limit_check(a.gain, a.ceiling, a.attack, a.release, 0u)) return 2;
        std::vector<float> x(total), y(total);
        std::vector<uint32_t> s;
        FILE *f = fopen(argv[9], "rb");
        if (!f || fread(x.data(), 4, total, f) != total) return 3;
        fclose(f);
        const zv::LimitRow r = zv::limit_reference(F, x.data(), N, total, a, y.data(), &s);
        f = fopen(argv[10], "wb");
        if (!f || fwrite(y.data(), 4, total, f) != total) return 3;
        fclose(f);
        f = fopen(argv[11], "wb");
        if (!f || fwrite(s.data(), 4, total, f) != total) return 3;
        fclose(f);
        printf("%llx %llx %llu %x %x %x %x %x %x\n", (unsigned long long)zv::loud_dbits(r.true_peak_before),
               (unsigned long long)zv::loud_dbits(r.true_peak_after), (unsigned long long)r.limited_samples, zv::level_bits(r.sample_peak_before),
               zv::level_bits(r.sample_peak_after), zv::level_bits(r.min_gain), zv::level_bits(r.true_peak_before_dbtp),
               zv::level_bits(r.true_peak_after_dbtp), zv::level_bits(r.reduction_db));
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "bench"))
    {
        zv::LoudFilter F;
        if (zv::loud_design((uint32_t)strtoul(argv[2], nullptr, 10), &F)) return 2;
        const uint64_t N = strtoull(argv[3], nullptr, 10);
        const zv::LimitAsk a{4.0f, 0.1f, (uint32_t)strtoul(argv[4], nullptr, 10), (uint32_t)strtoul(argv[5], nullptr, 10)};
        std::vector<float> x(N), y(N);
        uint32_t seed = 1;
        for (uint64_t i = 0; i < N; i++) x[i] = ((float)lcg(seed) / 8388608.0f - 1.0f) * 0.1f;
        double best = 1e300, sink = 0.0;
        for (int r = 0; r < atoi(argv[6]); r++)
        {
            const auto t0 = std::chrono::steady_clock::now();
            sink += zv::limit_reference(F, x.data(), N, N, a, y.data()).true_peak_after;
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            best = ms < best ? ms : best;
        }
        printf("%.3f %g\n", best, sink);
        return 0;
    }
    fprintf(stderr, "usage: limiter_check taps|design|run|self|check|plan|groups|bench ...\n");
    return 1;
}
