// limiter_kernels.hip — the look-ahead peak limiter: the peak pass with the required gains, the sliding minimum, the sliding mean with the
// apply, the reduction (the arithmetic: limiter.h).  A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "limiter.h"
#include "mfma_common.h"      // launch_lds
#include "stage_plan.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Limiter (kernels.h: launch_limit_*; the rule: limiter.h).  Five launches over ONE launch group of utterances (LimitJob), whatever the
// group; utterance u is blockIdx.y of the passes over samples and finds its arrays through segs[u].
//   peak<false>:  workgroup = LIMIT_TILE entries of q: p_m of the three interpolated phases and the sample, q_m stored per sample,
//                 peaks_before[tile0 + t] = {max p as f64 bits, max |x| as f32 bits}
//   min:          workgroup = LIMIT_TILE entries of m: m[i] = min q[i + 4 .. i + 4 + H], van Herk / Gil-Werman on the tile and its halo in LDS
//   mean:         workgroup = LIMIT_TILE samples: s_n = floor(sum m[n .. n + H] / W) from u64 prefix sums in LDS, out_n by limit_apply as
//                 float4s, stats[stat0 + t] = {min s_n, the count of s_n < ONE} over n < N
//   peak<true>:   the peak pass again on `out`, maxima only: peaks_after
//   reduce:       one wave per utterance: the maxima, the minimum, the count and the logarithms; rows[u]
// No atomics, nothing to zero: every entry a pass reads was stored by a pass before it in the same run.  Steps 2 to 4 are integer, so
// the tiling and the order inside a tile change no value.
//
// What a sample costs in the minimum and mean passes does not depend on W.  A workgroup stages S = LIMIT_TILE + H entries and scans them
// in two levels: every lane walks a run of C = ceil(S / 256) consecutive entries (made odd: lanes then read LDS at an odd stride), the 256
// run totals are scanned by shuffles (8 steps, whatever W), and every lane walks its run again from its carry.  That is two reads and a
// write per staged entry and scan, and two reads per output.  What does grow with W is the halo a tile stages: S / LIMIT_TILE entries per
// output, 1.7 at the default windows of 22 050 Hz and 5 at W = 8 192.

constexpr uint32_t LIMIT_IDENT = 0xffffffffu;      // the minimum of nothing
__device__ __forceinline__ uint32_t limit_umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

// The peak pass, in the form of loud_peak_kernel.  Workgroup (t, u) owns the entries i = LIMIT_TILE t .. + LIMIT_TILE of utterance u's q,
// that is m = i - H - LIMIT_PAD; lane l the 8 entries 8 l + r.  The samples x'[m0 - 5 .. m0 + LIMIT_TILE + 6] go to LDS as f64, the span test [0, N)
// and the finite test applied there, staged element i at i + (i >> 3) doubles.  A tile with no entry in m = -6 .. N + 4 sees zeros only:
// it stores ONE (and zero maxima) without running a chain.
constexpr int LIMIT_PK_R = 8;
constexpr int LIMIT_PK_STAGE = LIMIT_TILE + LOUD_TP_TAIL;
static_assert(LIMIT_TILE == LIMIT_THREADS * LIMIT_PK_R && LIMIT_DELAY + LIMIT_HEAD == LOUD_TP_TAIL, "8 entries per lane; the chain reads 12 samples");
__device__ __forceinline__ int limit_pk_at(int i) { return i + (i >> 3); }

template <bool AFTER>
__global__ __launch_bounds__(LIMIT_THREADS) void limit_peak_kernel(const LimitJob job)
{
    __shared__ double s_x[LIMIT_PK_STAGE + LIMIT_PK_STAGE / LIMIT_PK_R + 1];
    __shared__ float s_c[LOUD_TAPS];
    __shared__ unsigned long long red_t[4];
    __shared__ uint32_t red_p[4];
    const int u = blockIdx.y;
    const LimitSeg sg = job.segs[u];
    const LimitAsk ask = job.asks[u];
    const int64_t H = limit_halo(ask);
    const int64_t i0 = (int64_t)blockIdx.x * LIMIT_TILE;
    if (i0 >= limit_qlen(sg.total, H)) return;
    const int64_t m0 = i0 - H - LIMIT_PAD;
    unsigned long long *po = (unsigned long long *)(AFTER ? job.peaks_after : job.peaks_before) + 2 * ((size_t)sg.tile0 + blockIdx.x);
    uint32_t *qo = job.q + sg.q0 + i0 + (int64_t)threadIdx.x * LIMIT_PK_R;      // (the region holds whole tiles)
    if (m0 >= sg.N + LIMIT_HEAD || m0 + LIMIT_TILE <= -LIMIT_DELAY)
    {
        if (!AFTER)
        {
            *(uint4 *)qo = make_uint4(LIMIT_ONE, LIMIT_ONE, LIMIT_ONE, LIMIT_ONE);
            *(uint4 *)(qo + 4) = make_uint4(LIMIT_ONE, LIMIT_ONE, LIMIT_ONE, LIMIT_ONE);
        }
        if (threadIdx.x == 0) po[0] = 0, po[1] = 0;
        return;
    }
    const float *xs = (AFTER ? job.out : job.wav) + sg.x0;
    if (threadIdx.x < LOUD_TAPS) s_c[threadIdx.x] = job.filter->c[threadIdx.x];
    uint32_t sp = 0;
    for (int i = threadIdx.x; i < LIMIT_PK_STAGE; i += LIMIT_THREADS)
    {
        const int64_t g = m0 - LIMIT_HEAD + i;
        double v = 0.0;
        if (g >= 0 && g < sg.N)
        {
            const float x = xs[g];
            v = loud_sample(x);
            const uint32_t a = level_abs_bits(x);
            sp = a > sp ? a : sp;
        }
        s_x[limit_pk_at(i)] = v;
    }
    __syncthreads();
    // entry 8 l + r is m = m0 + 8 l + r; tap k of v(m + 6) reads x'[m + 6 - k] = staged element 8 l + r + 11 - k, |x'_m| element 8 l + r + 5
    double e[LIMIT_PK_R + LOUD_TP_TAIL];
    const int base = (int)threadIdx.x * LIMIT_PK_R;
#pragma unroll
    for (int j = 0; j < LIMIT_PK_R + LOUD_TP_TAIL; j++) e[j] = s_x[limit_pk_at(base + j)];
    unsigned long long p[LIMIT_PK_R];
#pragma unroll
    for (int r = 0; r < LIMIT_PK_R; r++) p[r] = loud_dbits(fabs(e[r + LIMIT_HEAD]));
#pragma unroll
    for (int f = 1; f < 4; f++)
    {
        double acc[LIMIT_PK_R];
#pragma unroll
        for (int r = 0; r < LIMIT_PK_R; r++) acc[r] = 0.0;
#pragma unroll
        for (int k = 0; k < LOUD_PHASE_TAPS; k++)
        {
            const float c = s_c[f + 4 * k];
#pragma unroll
            for (int r = 0; r < LIMIT_PK_R; r++) acc[r] = loud_tp_step(acc[r], c, e[r + LOUD_TP_TAIL - k]);
        }
#pragma unroll
        for (int r = 0; r < LIMIT_PK_R; r++)
        {
            const unsigned long long b = loud_dbits(fabs(acc[r]));
            p[r] = b > p[r] ? b : p[r];
        }
    }
    unsigned long long tp = 0;
#pragma unroll
    for (int r = 0; r < LIMIT_PK_R; r++) tp = p[r] > tp ? p[r] : tp;
    if (!AFTER)
    {
        uint32_t q[LIMIT_PK_R];
#pragma unroll
        for (int r = 0; r < LIMIT_PK_R; r++) q[r] = limit_q(ask.gain, ask.ceiling, mel_from_bits(p[r]));
        *(uint4 *)qo = make_uint4(q[0], q[1], q[2], q[3]);
        *(uint4 *)(qo + 4) = make_uint4(q[4], q[5], q[6], q[7]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        const unsigned long long t = (unsigned long long)__shfl_xor((long long)tp, o, 64);
        tp = t > tp ? t : tp;
        const uint32_t v = (uint32_t)__shfl_xor((int)sp, o, 64);
        sp = v > sp ? v : sp;
    }
    if ((threadIdx.x & 63) == 0)
    {
        red_t[threadIdx.x >> 6] = tp;
        red_p[threadIdx.x >> 6] = sp;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        for (int w = 1; w < 4; w++)
        {
            tp = red_t[w] > tp ? red_t[w] : tp;
            sp = red_p[w] > sp ? red_p[w] : sp;
        }
        po[0] = tp;
        po[1] = sp;
    }
}

// ---------------------------------------------------------------------------------------------------
// The carry of a two-level segmented minimum scan: lane t brings its run's (value, flag) — the minimum since the run's last reset, and
// whether the run held a reset — and receives the minimum of the runs before it back to the nearest run with a reset, that one
// included.  A Kogge-Stone scan per wave under the operator (v1, f1) . (v2, f2) = (f2 ? v2 : min(v1, v2), f1 | f2), then the waves
// before it, the nearest first.  red: 8 words of LDS.
__device__ __forceinline__ uint32_t limit_min_carry(uint32_t v, uint32_t f, uint32_t *red)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
        const uint32_t pv = (uint32_t)__shfl_up((int)v, o, 64), pf = (uint32_t)__shfl_up((int)f, o, 64);
        if (lane >= o)
        {
            if (!f) v = limit_umin(v, pv);
            f |= pf;
        }
    }
    __syncthreads();      // (the words may still be read from the scan before)
    if (lane == 63) red[w] = v, red[4 + w] = f;
    uint32_t ev = (uint32_t)__shfl_up((int)v, 1, 64), ef = (uint32_t)__shfl_up((int)f, 1, 64);
    if (lane == 0) ev = LIMIT_IDENT, ef = 0;
    __syncthreads();
    for (int k = w - 1; k >= 0 && !ef; k--)
    {
        ev = limit_umin(ev, red[k]);
        ef = red[4 + k];
    }
    return ev;
}

// The minimum pass.  Staged entry i is q[LIMIT_TILE t + LIMIT_PAD + i], i < S = LIMIT_TILE + H (ONE behind q's end), and output o is the minimum
// of the staged entries o .. o + H.  Cut the staged entries into blocks of W = H + 1 from entry 0: a window of W entries lies in two
// neighbouring blocks, so its minimum is min(suffix[o], prefix[o + H]), the suffix minima running to the block's end and the prefix
// minima from the block's start.  The suffix minima (of the first LIMIT_TILE entries: no output reads another) go to a second array first;
// the prefix minima then replace the entries.  The suffix
// scan walks downwards, so there lane t takes run 255 - t and the carry comes from the runs above.
__global__ __launch_bounds__(LIMIT_THREADS) void limit_min_kernel(const LimitJob job)
{
    extern __shared__ __attribute__((aligned(16))) char limit_lds[];
    const int stage = limit_stage(job.max_halo);
    uint32_t *a = (uint32_t *)limit_lds, *h = a + stage, *red = h + LIMIT_TILE;
    const int u = blockIdx.y, tid = threadIdx.x;
    const LimitSeg sg = job.segs[u];
    const int H = (int)limit_halo(job.asks[u]), W = H + 1, S = LIMIT_TILE + H;
    const int64_t i0 = (int64_t)blockIdx.x * LIMIT_TILE, mlen = limit_mlen(sg.total, H);
    if (i0 >= mlen) return;
    const int64_t qcap = limit_tiles(limit_qlen(sg.total, H)) * LIMIT_TILE;      // every entry of the region was stored by the peak pass
    const uint32_t *q = job.q + sg.q0 + i0 + LIMIT_PAD;
    for (int i = tid * 4; i < S; i += LIMIT_THREADS * 4)
    {
        uint4 v = make_uint4(LIMIT_ONE, LIMIT_ONE, LIMIT_ONE, LIMIT_ONE);
        if (i0 + LIMIT_PAD + i + 4 <= qcap) v = *(const uint4 *)(q + i);
        *(uint4 *)(a + i) = v;
    }
    __syncthreads();
    const int C = ((S + LIMIT_THREADS - 1) / LIMIT_THREADS) | 1;
    {
        // suffix minima: run c = 255 - tid covers [lo, hi), walked downwards; a reset stands AT entry i where i + 1 is a multiple of W
        const int c = LIMIT_THREADS - 1 - tid;
        const int lo = c * C < S ? c * C : S, hi = lo + C < S ? lo + C : S;
        const int first = hi / W * W - 1;      // the highest reset below hi (-1: none in any run)
        uint32_t run = LIMIT_IDENT, flag = 0;
        for (int i = hi - 1, nb = first; i >= lo; i--)
        {
            if (i == nb) run = LIMIT_IDENT, flag = 1, nb -= W;
            run = limit_umin(run, a[i]);
        }
        run = limit_min_carry(run, flag, red);
        for (int i = hi - 1, nb = first; i >= lo; i--)
        {
            if (i == nb) run = LIMIT_IDENT, nb -= W;
            run = limit_umin(run, a[i]);
            if (i < LIMIT_TILE) h[i] = run;      // (an output reads suffix[o], o < LIMIT_TILE)
        }
    }
    __syncthreads();
    {
        // prefix minima, in place: run tid covers [lo, hi), walked upwards; a reset stands at every multiple of W
        const int lo = tid * C < S ? tid * C : S, hi = lo + C < S ? lo + C : S;
        const int first = (lo + W - 1) / W * W;
        uint32_t run = LIMIT_IDENT, flag = 0;
        for (int i = lo, nb = first; i < hi; i++)
        {
            if (i == nb) run = LIMIT_IDENT, flag = 1, nb += W;
            run = limit_umin(run, a[i]);
        }
        run = limit_min_carry(run, flag, red);
        for (int i = lo, nb = first; i < hi; i++)
        {
            if (i == nb) run = LIMIT_IDENT, nb += W;
            run = limit_umin(run, a[i]);
            a[i] = run;
        }
    }
    __syncthreads();
    uint32_t *m = job.m + sg.m0 + i0;
    for (int o = tid; o < LIMIT_TILE; o += LIMIT_THREADS)
        if (i0 + o < mlen) m[o] = limit_umin(h[o], a[o + H]);
}

// The mean pass.  Staged entry i is m[LIMIT_TILE t + i], i < S; P[i] = the sum of the staged entries below i (P[0] = 0), by the same
// two-level scan; output o = (P[o + W] - P[o]) / W.  A prefix sum is below 2^30 * 10 240 < 2^44: it lies in LDS as a u32 and a u16, six
// bytes per entry instead of eight, which is what lets a second workgroup onto the CU at the largest window.  The 2 048 values s then go through LDS (over the prefix sums, which are no
// longer needed) so that a lane applies four consecutive ones to a float4.
__global__ __launch_bounds__(LIMIT_THREADS) void limit_mean_kernel(const LimitJob job)
{
    extern __shared__ __attribute__((aligned(16))) char limit_lds[];
    const int stage = limit_stage(job.max_halo);
    uint32_t *P_lo = (uint32_t *)limit_lds;
    uint16_t *P_hi = (uint16_t *)(P_lo + stage + 4);
    unsigned long long *red = (unsigned long long *)(limit_lds + (size_t)(stage + 4) * 6);
    uint32_t *red_s = (uint32_t *)(red + 4);
    auto P = [&](int i) { return (unsigned long long)P_hi[i] << 32 | P_lo[i]; };
    auto set_P = [&](int i, unsigned long long v) { P_lo[i] = (uint32_t)v, P_hi[i] = (uint16_t)(v >> 32); };
    const int u = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const LimitSeg sg = job.segs[u];
    const LimitAsk ask = job.asks[u];
    const int H = (int)limit_halo(ask), W = H + 1, S = LIMIT_TILE + H;
    const int64_t n0 = (int64_t)blockIdx.x * LIMIT_TILE, mlen = limit_mlen(sg.total, H);
    if (n0 >= sg.total) return;
    const uint32_t *m = job.m + sg.m0 + n0;
    if (tid == 0) set_P(0, 0);
    for (int i = tid; i < S; i += LIMIT_THREADS) P_lo[1 + i] = n0 + i < mlen ? m[i] : 0u;
    __syncthreads();
    {
        const int C = ((S + LIMIT_THREADS - 1) / LIMIT_THREADS) | 1;
        const int lo = tid * C < S ? tid * C : S, hi = lo + C < S ? lo + C : S;
        unsigned long long run = 0;
        for (int i = lo; i < hi; i++) run += P_lo[1 + i];
        unsigned long long inc = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1)
        {
            const unsigned long long pv = (unsigned long long)__shfl_up((long long)inc, o, 64);
            if (lane >= o) inc += pv;
        }
        if (lane == 63) red[w] = inc;
        __syncthreads();
        unsigned long long carry = inc - run;
        for (int k = 0; k < w; k++) carry += red[k];
        for (int i = lo; i < hi; i++)
        {
            carry += P_lo[1 + i];
            set_P(1 + i, carry);
        }
    }
    __syncthreads();
    uint32_t s[LIMIT_TILE / LIMIT_THREADS], mn = LIMIT_ONE, cnt = 0;
#pragma unroll
    for (int r = 0; r < LIMIT_TILE / LIMIT_THREADS; r++)
    {
        const int o = tid + r * LIMIT_THREADS;
        s[r] = LIMIT_ONE;
        if (n0 + o < sg.total)
        {
            s[r] = (uint32_t)((P(o + W) - P(o)) / (unsigned long long)W);
            if (n0 + o < sg.N)
            {
                mn = limit_umin(mn, s[r]);
                cnt += s[r] < LIMIT_ONE;
            }
        }
    }
    __syncthreads();
    uint32_t *s_s = (uint32_t *)limit_lds;
#pragma unroll
    for (int r = 0; r < LIMIT_TILE / LIMIT_THREADS; r++) s_s[tid + r * LIMIT_THREADS] = s[r];
    __syncthreads();
    const float *xs = job.wav + sg.x0 + n0;
    float *ys = job.out + sg.x0 + n0;
#pragma unroll
    for (int r = 0; r < LIMIT_TILE / (LIMIT_THREADS * 4); r++)
    {
        const int o = tid * 4 + r * LIMIT_THREADS * 4;
        if (n0 + o + 4 <= sg.total)
        {
            const float4 v = *(const float4 *)(xs + o);
            const uint4 g = *(const uint4 *)(s_s + o);
            *(float4 *)(ys + o) = make_float4(limit_apply(v.x, ask.gain, g.x), limit_apply(v.y, ask.gain, g.y), limit_apply(v.z, ask.gain, g.z),
                                              limit_apply(v.w, ask.gain, g.w));
        }
        else
            for (int j = o; j < o + 4 && n0 + j < sg.total; j++) ys[j] = limit_apply(xs[j], ask.gain, s_s[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        mn = limit_umin(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
        cnt += (uint32_t)__shfl_xor((int)cnt, o, 64);
    }
    if (lane == 0) red_s[w] = mn, red_s[4 + w] = cnt;
    __syncthreads();
    if (tid == 0)
    {
        for (int k = 1; k < 4; k++) mn = limit_umin(mn, red_s[k]), cnt += red_s[4 + k];
        uint32_t *st = job.stats + 2 * ((size_t)sg.stat0 + blockIdx.x);
        st[0] = mn;
        st[1] = cnt;
    }
}

// The reduction: one wave per utterance over the tiles' partial results.
__global__ __launch_bounds__(64) void limit_reduce_kernel(const LimitJob job)
{
    const int u = blockIdx.x, lane = threadIdx.x;
    const LimitSeg sg = job.segs[u];
    const int64_t H = limit_halo(job.asks[u]);
    const int64_t ptiles = limit_tiles(limit_qlen(sg.total, H)), stiles = limit_tiles(sg.total);
    const unsigned long long *pb = (const unsigned long long *)job.peaks_before + 2 * (size_t)sg.tile0;
    const unsigned long long *pa = (const unsigned long long *)job.peaks_after + 2 * (size_t)sg.tile0;
    unsigned long long tb = 0, ta = 0, cnt = 0;
    uint32_t sb = 0, sa = 0, mn = LIMIT_ONE;
    for (int64_t t = lane; t < ptiles; t += 64)
    {
        tb = pb[2 * t] > tb ? pb[2 * t] : tb;
        sb = (uint32_t)pb[2 * t + 1] > sb ? (uint32_t)pb[2 * t + 1] : sb;
        ta = pa[2 * t] > ta ? pa[2 * t] : ta;
        sa = (uint32_t)pa[2 * t + 1] > sa ? (uint32_t)pa[2 * t + 1] : sa;
    }
    const uint32_t *st = job.stats + 2 * (size_t)sg.stat0;
    for (int64_t t = lane; t < stiles; t += 64)
    {
        mn = limit_umin(mn, st[2 * t]);
        cnt += st[2 * t + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        unsigned long long t = (unsigned long long)__shfl_xor((long long)tb, o, 64);
        tb = t > tb ? t : tb;
        t = (unsigned long long)__shfl_xor((long long)ta, o, 64);
        ta = t > ta ? t : ta;
        cnt += (unsigned long long)__shfl_xor((long long)cnt, o, 64);
        uint32_t v = (uint32_t)__shfl_xor((int)sb, o, 64);
        sb = v > sb ? v : sb;
        v = (uint32_t)__shfl_xor((int)sa, o, 64);
        sa = v > sa ? v : sa;
        mn = limit_umin(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
    }
    if (lane == 0) job.rows[u] = limit_finish(tb, sb, ta, sa, mn, cnt);
}

static bool limit_job_ok(const LimitJob &j)
{
    return j.wav && j.out && j.q && j.m && j.peaks_before && j.peaks_after && j.stats && j.rows && j.segs && j.asks && j.filter &&
           !((uintptr_t)j.wav & 15) && !((uintptr_t)j.out & 15) && !((uintptr_t)j.q & 15) && !((uintptr_t)j.m & 15) &&
           limit_plan(j.max_qlen, j.max_total, j.max_halo, j.nseg).ok;
}

hipError_t launch_limit_peak(hipStream_t s, const LimitJob &j, bool after)
{
    if (!limit_job_ok(j)) return hipErrorInvalidValue;
    const LimitPlan p = limit_plan(j.max_qlen, j.max_total, j.max_halo, j.nseg);
    if (after) hipLaunchKernelGGL(limit_peak_kernel<true>, dim3(p.peak_gx, p.gy), dim3(LIMIT_THREADS), 0, s, j);
    else hipLaunchKernelGGL(limit_peak_kernel<false>, dim3(p.peak_gx, p.gy), dim3(LIMIT_THREADS), 0, s, j);
    return hipGetLastError();
}

hipError_t launch_limit_min(hipStream_t s, const LimitJob &j)
{
    if (!limit_job_ok(j)) return hipErrorInvalidValue;
    const LimitPlan p = limit_plan(j.max_qlen, j.max_total, j.max_halo, j.nseg);
    return launch_lds(limit_min_kernel, dim3(p.min_gx, p.gy), dim3(LIMIT_THREADS), p.min_lds, s, j);
}

hipError_t launch_limit_mean(hipStream_t s, const LimitJob &j)
{
    if (!limit_job_ok(j)) return hipErrorInvalidValue;
    const LimitPlan p = limit_plan(j.max_qlen, j.max_total, j.max_halo, j.nseg);
    return launch_lds(limit_mean_kernel, dim3(p.mean_gx, p.gy), dim3(LIMIT_THREADS), p.mean_lds, s, j);
}

hipError_t launch_limit_reduce(hipStream_t s, const LimitJob &j)
{
    if (!limit_job_ok(j)) return hipErrorInvalidValue;
    const LimitPlan p = limit_plan(j.max_qlen, j.max_total, j.max_halo, j.nseg);
    hipLaunchKernelGGL(limit_reduce_kernel, dim3(p.gy), dim3(64), 0, s, j);
    return hipGetLastError();
}

}  // namespace zv
