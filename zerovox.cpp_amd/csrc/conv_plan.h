// conv_plan.h — what a conv or ResBlock launcher then does (DESIGN.md "Launch plans"): which kernel form runs, on what tile, grid and
// LDS size, as pure host code.  Plain integers and booleans in, a small struct out; every non-diagnostic switch the launchers of
// conv.hip, conv1d_mfma.hip and conv_gemm.hip depend on is read here, through knob(), when the launch is planned.  The launchers
// validate their arguments, call their plan, copy its fields into the job table and pick the template instantiation it names.
// voc_plan.h (which launcher is called) builds on this header; tests/native/conv_plan_check.cpp pins every threshold on the host:
// nothing here needs HIP, a job table or a device pointer.
#pragma once

#include <stddef.h>

#include "conv_xcd.h"
#include "knobs.h"
#include "tile_deal.h"

namespace zv
{

// ---- the batch switches: 0 never, 1 batches, 2 always ----
// "batches" = what the launch picks by itself; where that is a capacity, BATCH_ROWS rows of it (frames for the schedules, rows of a
// launch for launch_conv).  One threshold for all of them, and not a measured one: no sweep of capacities below it is on record.
constexpr long BATCH_ROWS = 16384;
inline bool batch_switch(int value, bool picked_by_itself) { return value != 0 && (value == 2 || picked_by_itself); }
inline bool batch_rows(long rows) { return rows >= BATCH_ROWS; }

// ---- LDS budgets of a gfx950 CU (160 KB), each named once ----
constexpr size_t LDS_PER_WG = 160 * 1024;      // the most one workgroup can have
constexpr size_t LDS_TWO_WGS = 80 * 1024;      // per workgroup where two are to share a CU
constexpr size_t LDS_DEFAULT = 64 * 1024;      // what a launch gets without asking (resblock_triple_kernel stays inside it)

inline int plan_round_up(int x, int a) { return (x + a - 1) / a * a; }

// Densely packed decoding (dec_runs.h) hands a launcher ONE segment that holds many utterances back to back.  Such a launch is a
// batch and must be planned as one: the schedule states the utterance count for the launches it enqueues inside a ConvPackedUtts
// scope, and a ConvCall built without the field (the launchers' six-value form) takes it from there.  0 everywhere else: the segments
// are the utterances.  Per thread, like the enqueueing itself; no kernel argument carries it.
inline int &conv_packed_utts()
{
    static thread_local int n = 0;
    return n;
}
struct ConvPackedUtts
{
    int saved;
    explicit ConvPackedUtts(int n) : saved(conv_packed_utts()) { conv_packed_utts() = n; }
    ~ConvPackedUtts() { conv_packed_utts() = saved; }
    ConvPackedUtts(const ConvPackedUtts &) = delete;
    ConvPackedUtts &operator=(const ConvPackedUtts &) = delete;
};

// the call: jobs of the launch, the segments it covers (Segs::nseg / max_rows), rows per base row, CUs, and the first output tile of a
// generic conv launch (the tiles before it belong to conv_gemm_kernel)
struct ConvCall
{
    int njobs, nseg, max_rows, rate, n_cu, nt_begin;
    int nutt = conv_packed_utts();      // utterances the segments hold when they are not one each (packed decoding), else 0
};
// whether the launch covers several utterances: what the single-utterance forms and the spread map ask
inline bool conv_call_is_batch(const ConvCall &c) { return c.nseg > 1 || c.nutt > 1; }

// ---- conv_gemm_kernel's tiling (conv_gemm.hip) ----
// Only whole groups of 8 output tiles are packed for it
inline int conv_gemm_groups(int Cout_p) { return ((Cout_p + 31) / 32) / 8; }
// tiles the kernel covers: whole groups of 8, plus ONE leftover tile (1 056 channels = 33 tiles, 528 = 17) that the last group's
// workgroups compute on the side (one extra 32 x 32 tile per wave); more leftovers stay with conv1d_mfma_kernel
inline int conv_gemm_tiles(int Cout_p)
{
    const int nt = (Cout_p + 31) / 32, ng = nt / 8;
    return ng * 8 + ((nt - ng * 8 == 1 && ng >= 1) ? 1 : 0);
}
// steps of its K loop: (256-channel chunk, tap, 64-channel block)
inline int conv_gemm_units(int Cin_p, int K)
{
    int n = 0;
    for (int c0 = 0; c0 < Cin_p; c0 += 256) n += K * (((Cin_p - c0 < 256 ? Cin_p - c0 : 256) + 63) / 64);
    return n;
}

// ---- the generic conv (conv.hip) ----
enum ConvPrologue : int
{
    PRO_RAW_F16 = 0,      // x is already the f16 operand (written by an EPI f16 store)
    PRO_ACT = 1,          // f16(lrelu(x, slope))            (slope 1 = identity, 0 = relu)
    PRO_NORM_ACT = 2,     // f16(lrelu(((x - mean_c) * rstd_c) * g_c + b_c, slope))   InstanceNorm/AdaIN
    PRO_MELNORM = 3,      // f16((x - a_c) / b_c)            (src/hifigan.cpp:242-243)
    PRO_SUM3_ACT = 4,     // f16(lrelu(((x0 + x1) + x2) * pscale, slope))   MRF mean (src/hifigan.cpp:300-315)
    PRO_SCALE_ACT = 5     // f16(lrelu(x * pscale, slope))                  MRF mean whose sum the producer already formed
};

// loader waves of conv1d_mfma_kernel's single-utterance form (see the kernel): waves that only stage — chunk c + 1 into the second
// LDS tile while the four MFMA waves walk chunk c.  They have their own vector-memory counters: the MFMA waves' counted waits on the
// weight stream never queue behind a tile's loads.  0 = the round-3 form (every wave stages, then every wave multiplies).
#ifndef ZV_SINGLE_LW
#define ZV_SINGLE_LW 4
#endif
// a launch over several segments that passes the single-utterance form's workgroup count only as capacity, with more than a round of
// workgroups, takes the ordinary form (0: it keeps the loader-wave form on the spread map of conv_xcd.h; see conv_plan)
#ifndef ZV_CONV_BATCH_ROUTE
#define ZV_CONV_BATCH_ROUTE 1
#endif

// a conv job as the plan needs it (conv.hip: conv_desc(ConvJob))
struct ConvDesc
{
    int  K, dil, pad, Cin_p, Cout_p, ck, pro, ldx;
    bool has_w8, out_f16, has_res, has_stat, eact, three_inputs;      // ConvJob::w8, out_f16, res, stat_part, eact, x1 || x2
};

// batches of wide convs over an f16 operand tensor (the decoder's, behind its pre-pass): whole groups of 8 output tiles on
// conv_gemm_kernel, job by job; the tiles left over (conv_gemm_tiles: 1 088 channels = 4 groups + 2 tiles) on the generic kernel
inline bool conv_gemm_takes(const ConvDesc &j, const ConvCall &c)
{
    const long rows = (long)c.max_rows * c.rate * c.nseg;
    return batch_switch(knob(ZV_CONV_GEMM), batch_rows(rows)) && j.has_w8 && j.pro == PRO_RAW_F16 && j.Cin_p >= 128 &&
           conv_gemm_groups(j.Cout_p) >= 1 && !j.out_f16 && (j.ldx & 7) == 0;
}

// conv_gemm_kernel's launch: workgroup order (ZV_GEMM_ORDER), 256-row tiles per segment, grid.x, LDS
struct ConvGemmPlan
{
    int    order, tps, gx, threads;
    size_t lds_bytes;
};
inline ConvGemmPlan conv_gemm_plan(int Cout_p, const ConvCall &c)
{
    ConvGemmPlan p{};
    p.order = knob(ZV_GEMM_ORDER);
    p.tps = (c.max_rows * c.rate + 255) / 256;
    const int ng = conv_gemm_groups(Cout_p), rts = p.tps * c.nseg;
    // (grid.x covers (row tile, group) in the kernel's XCD-aware order: 8 / ng XCDs per group)
    p.gx = (p.order == 1 && (ng == 1 || ng == 2 || ng == 4)) ? plan_round_up(rts, 8 / ng) * ng : rts * ng;
    p.threads = 512;
    p.lds_bytes = 4 * (16384 + 18432);
    return p;
}

// the convs conv_stream_kernel takes: one job, 3 taps, one chunk of 64 / 128 input channels read from ONE f32 tensor, bias-only epilogue
inline bool conv_stream_ok(const ConvDesc &j, const ConvCall &c)
{
    return c.njobs == 1 && c.nt_begin == 0 && (j.pro == PRO_ACT || j.pro == PRO_SCALE_ACT) && j.K == 3 && j.dil == 1 && j.pad == 1 &&
           (j.Cin_p == 64 || j.Cin_p == 128) && j.ck == j.Cin_p && (j.ldx & 3) == 0 && !j.has_res && !j.has_stat && !j.eact && !j.out_f16 &&
           !j.three_inputs;
}

// the instantiations of conv1d_mfma_kernel<MT, WN, NT> a tiled launch can name (conv.hip: ZV_CASE)
inline bool conv_tiled_exists(int MT, int WN, int NT)
{
    return (NT == 1 && (MT == 1 || MT == 2 || MT == 4) && (WN == 1 || WN == 2 || WN == 4)) || (NT == 2 && MT == 2 && WN == 4);
}

enum ConvForm { CONV_STREAM, CONV_LOADER, CONV_TILED };       // conv_stream_kernel / conv1d_mfma_kernel<1, WN, 1, true> / <MT, WN, NT>
struct ConvPlan
{
    bool     valid;
    ConvForm form;
    int      MT, WN, NT;                    // wave tile: 32 MT rows x 32 NT channels, WN waves along the channels (of 4)
    int      strip, nkc;                    // STREAM: row tiles a workgroup walks; 16-channel steps per tap (8 or 4: the instantiation)
    int      tps;                           // row tiles (STREAM: strips) per segment
    int      gx, gy, gz, threads;
    size_t   lds_bytes;
    int      tile_bytes;                    // LOADER / TILED: one LDS tile
    int      xcd_nx, xcd_ny, xcd_spread;    // LOADER dealt over the XCDs (conv_xcd.h): row tiles, channel groups, spread map; 0: plain grid
    int      warm;                          // ZV_CONV_WARM
};

// LOADER / TILED geometry of conv1d_mfma_kernel<MT, WN, NT, loader>; false where the LDS does not fit a workgroup
inline bool conv_plan_tiles(ConvPlan &p, bool loader, int MT, int WN, int NT, int Lmax, int ntiles, int halo, int ck, int dmax, const ConvCall &c)
{
    const int BM = 32 * MT * (4 / WN);
    p.form = loader ? CONV_LOADER : CONV_TILED;
    p.MT = MT, p.WN = WN, p.NT = NT;
    p.tps = (Lmax + BM - 1) / BM;
    p.gx = p.tps * c.nseg, p.gy = (ntiles + WN * NT - 1) / (WN * NT), p.gz = c.njobs;
    const int LW = loader ? ZV_SINGLE_LW : 0;
    p.threads = 256 + 64 * LW;
    p.xcd_nx = p.xcd_ny = p.xcd_spread = 0;
    p.warm = knob(ZV_CONV_WARM) != 0;
    if (loader && knob(ZV_CONV_XCD) != 0)
    {
        // (see the kernel and conv_xcd.h) grid.x = 8 XCDs x slots; several segments: no XCD idles for want of channel groups
        p.xcd_ny = p.gy;
        p.xcd_nx = p.gx;
        p.xcd_spread = conv_call_is_batch(c);
        p.gx = conv_xcd_grid(p.xcd_nx, p.xcd_ny, p.xcd_spread), p.gy = 1;
    }
    // + dil rows: mfma_taps prefetches one tap past the end
    p.tile_bytes = plan_round_up((BM + halo + dmax) * (ck * 2 + 16), 16);
    p.lds_bytes = (size_t)p.tile_bytes * (LW > 0 ? 2 : 1);
    return p.lds_bytes <= LDS_PER_WG;
}

// conv_stream_kernel's launch
inline ConvPlan conv_stream_plan(const ConvDesc &j, const ConvCall &c)
{
    ConvPlan p{};
    const int Lmax = c.max_rows * c.rate;
    const int ntiles = (j.Cout_p + 31) / 32, gy = (ntiles + 3) / 4;
    const int occ = j.Cin_p == 128 ? 2 : 3;
    // strips of 8 tiles while that still leaves about twelve rounds of workgroups, else 4, 2
    int strip = 8;
    while (strip > 2 && (long)((Lmax + 64 * strip - 1) / (64 * strip)) * c.nseg * gy < 12L * occ * c.n_cu) strip >>= 1;
    p.valid = true;
    p.form = CONV_STREAM;
    p.strip = strip;
    p.nkc = j.Cin_p / 16;
    p.tps = (Lmax + 64 * strip - 1) / (64 * strip);
    p.gx = p.tps * c.nseg, p.gy = gy, p.gz = 1;
    p.threads = 256;
    p.lds_bytes = (size_t)2 * 66 * (j.Cin_p * 2 + 16);
    return p;
}

// One launch of the generic conv family over `jobs` (c.njobs of them, one Cout_p) from output tile c.nt_begin on.  The tile shape
// never changes an output bit: every output element is one accumulator chain over (chunk, tap, channel).
inline ConvPlan conv_plan(const ConvDesc *jobs, const ConvCall &c)
{
    ConvPlan p{};
    const int njobs = c.njobs, n_cu = c.n_cu;
    const int Lmax = c.max_rows * c.rate;
    if (njobs < 1) return p;
    int halo = 0, ck = 0, dmax = 1;
    for (int i = 0; i < njobs; i++)
    {
        dmax = jobs[i].dil > dmax ? jobs[i].dil : dmax;
        if (jobs[i].Cout_p != jobs[0].Cout_p) return p;
        const int h = (jobs[i].K - 1) * jobs[i].dil;
        if (h > halo) halo = h;
        ck = jobs[i].ck > ck ? jobs[i].ck : ck;
    }
    const int Cout_p = jobs[0].Cout_p;
    const int ntiles = (Cout_p + 31) / 32 - c.nt_begin;
    if (ntiles < 1) return p;
    // three output tiles already take four waves (one idles): the input tile is staged once instead of twice
    // (two row tiles x two output tiles per workgroup instead, so that row pairs share weight fragments: a single utterance 1.71 -> 1.79 ms)
    const int WN = ntiles >= 3 ? 4 : (ntiles >= 2 ? 2 : 1);
    // pick the tallest wave tile (most B-fragment reuse) that still gives every CU about two workgroups
    auto wgs = [&](int MT, int NT) {
        const int BM = 32 * MT * (4 / WN);
        return (long)((Lmax + BM - 1) / BM) * c.nseg * ((ntiles + WN * NT - 1) / (WN * NT)) * njobs;
    };
    int MT = 4;
    while (MT > 1 && wgs(MT, 1) < 2L * n_cu) MT >>= 1;
    while (MT > 1 && (size_t)(32 * MT * (4 / WN) + halo + dmax) * (ck * 2 + 16) > LDS_TWO_WGS) MT >>= 1;   // keep >= 2 workgroups per CU in LDS
    {
        // memory-bound convs (the polyphase transposed convs of the narrow HiFi-GAN stages: a few hundred MACs per output
        // element against 8 bytes moved) want workgroups in flight, not weight reuse: measured on the batch, the last
        // three upsample convs take 897 / 595 / 452 us with the tall tiles and 636 / 569 / 416 us with these
        const double ai = 2.0 * jobs[0].K * jobs[0].Cin_p * Cout_p / (4.0 * (jobs[0].Cin_p + Cout_p));
        const bool memory_bound = ai < 200.0 && wgs(1, 1) >= 16L * n_cu;
        // ... and the ones conv_stream_kernel takes run there (ZV_CONV_STREAM = 0 never, 2 at any length)
        if (conv_stream_ok(jobs[0], c) && batch_switch(knob(ZV_CONV_STREAM), memory_bound)) return conv_stream_plan(jobs[0], c);
        // (round 3: 64-row tiles for all of them — the 128 -> 4 x 64 channel one 573 -> 501 us: half the weight stream per row)
        if (memory_bound && MT > 2) MT = 2;
    }
    if (MT < knob(ZV_CONV_MT)) MT = knob(ZV_CONV_MT);      // measurement hook: minimum MT
    // two output tiles per wave once a conv is wide and the launch still has rounds of workgroups to spare
    const int nt_env = knob(ZV_CONV_NT);
    // ... and deep (>= 2 048 products per output element: the decoder's; the first two upsample convs, 1 536 / 768 deep, measured
    // 265 / 417 us on 64 x 64 wave tiles and 245 / 395 us on 128 x 32 ones)
    int NT = (WN == 4 && ntiles >= 8 && MT >= 2 && wgs(MT, 2) >= 4L * n_cu && jobs[0].K * jobs[0].Cin_p >= 2048) ? 2 : 1;
    if (nt_env == 1 || (nt_env == 2 && WN == 4 && ntiles >= 2 && MT >= 2)) NT = nt_env;
    if (NT == 2 && MT == 4) MT = 2;        // 64 x 64 per wave: the 128 x 64 shape does not fit 256 registers
    {
        // single-utterance launches (at most a round of workgroups, one wave per SIMD): the deep-lookahead loop for the
        // 256-channel chunks
        // ... of convs with SEVERAL such chunks (the decoder's): measured per launch at 512 frames, the one-chunk 256-channel
        // convs of HiFi-GAN stage 1 take 23.0 us on this loop against 20.0 us on mfma_taps (profiles/r02_v2_single_utterance_kernel_trace.txt
        // vs round 1's trace), the five-chunk decoder convs 29.6 against 33
        // ... and of launches the form was built for.  wgs() counts capacity, not utterances: a batch of 32 utterances x 256 phonemes
        // has 512 workgroups of 8 waves for the first conv of a variance predictor, two rounds of a form whose loader waves leave
        // room for one workgroup per CU.  Several segments and more than a round: the ordinary form (measured: DESIGN.md, "Narrow batch convs on all XCDs")
        const bool batch_rounds = ZV_CONV_BATCH_ROUTE && conv_call_is_batch(c) && wgs(1, 1) > n_cu;
        const int  single_env = knob(ZV_CONV_SINGLE);
        // (two LDS tiles that do not fit a workgroup: the tiled form below, which runs the conv on one)
        if (single_env != 0 && MT == 1 && NT == 1 && ck == 256 && wgs(1, 1) <= 2L * n_cu && !batch_rounds && (jobs[0].Cin_p > 256 || single_env == 2) &&
            WN >= 2 && conv_plan_tiles(p, true, 1, WN, 1, Lmax, ntiles, halo, ck, dmax, c))
        {
            p.valid = true;
            return p;
        }
    }
    p.valid = conv_tiled_exists(MT, WN, NT) && conv_plan_tiles(p, false, MT, WN, NT, Lmax, ntiles, halo, ck, dmax, c);
    return p;
}

// ---- the vocoder's output conv (conv.hip: out_conv_tanh_kernel) ----
// C channels -> 1, K taps: a workgroup keeps its 256 output rows' operand window (256 + K - 1 rows of Cp f16 channels, 16 bytes of
// row padding) and the K x Cp weights in LDS, inside what a launch gets without asking.  7 taps: Cp <= 112.  The loader refuses a
// checkpoint whose last stage is wider, the launcher a call that is
inline size_t out_conv_lds_bytes(int C, int K)
{
    const int Cp = plan_round_up(C, 16);
    return (size_t)(256 + K - 1) * (Cp * 2 + 16) + (size_t)K * Cp * 2;
}
inline bool out_conv_supported(int C, int K) { return C >= 1 && K >= 1 && (K & 1) == 1 && out_conv_lds_bytes(C, K) <= LDS_DEFAULT; }

// ---- the fused ResBlock kernels (conv1d_mfma.hip) ----
constexpr int TRIPLE_MAX_DIL = 3;

// A block of n_dil dilation pairs with K taps on a tile of R rows: every conv runs over the whole tile as a zero-padded sequence, so
// after the pairs the rows within the cumulative halo of a tile edge are wrong and only the TM centre rows are stored
struct BlockTile
{
    int sumd, dmax;      // sum and largest of the dilations
    int h2;              // (K - 1) / 2: rows a tap reaches to either side at dilation 1
    int halo;            // h2 (sumd + n_dil): the pairs' first convs reach h2 dil each, their second convs h2
    int TM;              // R - 2 halo
};
inline BlockTile block_tile(int K, const int *dil, int n_dil, int R)
{
    BlockTile t{0, 1, (K - 1) / 2, 0, 0};
    for (int d = 0; d < n_dil; d++)
    {
        t.sumd += dil[d];
        t.dmax = dil[d] > t.dmax ? dil[d] : t.dmax;
    }
    t.halo = t.h2 * (t.sumd + n_dil);
    t.TM = R - 2 * t.halo;
    return t;
}

// a block as launch_triple / launch_block64 get it (TripleJob)
struct BlockDesc
{
    int Cp, K, n_dil;
    int dil[TRIPLE_MAX_DIL];
};

// the MFMA loop of the fused kernels walks whole 8-step bodies (CP = 64: also half a body at the end) and at least one
inline bool pair_supported(int Cp, int K)
{
    if (!(Cp == 32 || Cp == 64 || Cp == 128 || Cp == 256) || K < 1 || (K & 1) == 0) return false;
    const int nsb = (K * (Cp / 16) + 3) >> 2;
    return nsb >= 2 && (Cp == 64 || (nsb & 1) == 0);
}
// a ResBlock (Cp channels, K taps, these dilations) fits the whole-block kernel
inline bool triple_supported(int Cp, int K, const int *dil, int n_dil)
{
    if (Cp != 32 || n_dil < 1 || n_dil > TRIPLE_MAX_DIL || !pair_supported(Cp, K) || (K & 1) == 0) return false;
    return block_tile(K, dil, n_dil, 256).TM >= 96;           // at least 3/8 of the tile's rows are output
}
// the blocks resblock_block64_kernel takes: 64 channels, few taps (the halo of n_dil pairs leaves most of the 256-row tile)
inline bool block64_supported(int Cp, int K, const int *dil, int n_dil)
{
    if (Cp != 64 || K < 3 || (K & 1) == 0 || n_dil < 1 || n_dil > TRIPLE_MAX_DIL) return false;
    return block_tile(K, dil, n_dil, 256).TM >= 192;          // at least three quarters of the tile's rows are output
}

// launch_pair: njobs dilation pairs of Cp channels, at most Kmax taps and dilation dmax; any_sum: a job carries the running MRF sum
// (PairJob::sum_in / sum_out), merged: the launch stores the sum of its jobs (merge_out), all_ring_weights: every job has its ring stream
struct PairPlan
{
    bool   valid;
    bool   ring;                  // resblock_pair64_kernel (weights through an LDS ring) instead of resblock_pair_kernel<Cp, MT>
    int    MT;
    int    deal_c, gx, gz;        // tile_deal.h chunk; grid (x a multiple of 8, z the jobs)
    int    ring_off;              // ring: byte offset of the weight ring in LDS
    size_t lds_bytes;
};
inline PairPlan pair_plan(int Cp, int Kmax, int dmax, bool any_sum, bool merged, bool all_ring_weights, const ConvCall &c)
{
    PairPlan p{};
    // the running sum exists only in resblock_pair_kernel<CP, MT, false>: not together with the merged form
    if (!(Cp == 32 || Cp == 64 || Cp == 128 || Cp == 256) || (any_sum && merged)) return p;
    const int  njobs = c.njobs, n_cu = c.n_cu, Lmax = c.max_rows * c.rate;
    const int  WN = Cp == 256 ? 4 : Cp / 32;
    auto wgs = [&](int MT) {
        const int BM = 32 * MT * (4 / WN);
        const int TM = BM - (Kmax - 1);
        return TM < 32 ? 0L : (long)((Lmax + TM - 1) / TM) * c.nseg * njobs;
    };
    p.deal_c = tile_deal_chunk(Cp);
    p.gz = merged ? 1 : njobs;
    // 64 channels, batches: the form with the weights through an LDS ring (ZV_PAIR64_RING = 0 never, 2 whenever it fits); not with
    // the running sum (the ring kernel would silently write P.out instead)
    {
        const int  ring_env = knob(ZV_PAIR64_RING);
        const bool ok = Cp == 64 && !any_sum && ring_env != 0 && Kmax >= 3 &&
                        (size_t)(256 + Kmax * dmax) * 144 + 4 * 8192 + 1024 <= LDS_TWO_WGS && all_ring_weights;
        const long rwgs = (long)((Lmax + 256 - Kmax) / (257 - Kmax)) * c.nseg * njobs;
        if (ok && (ring_env == 2 || rwgs >= 6L * n_cu))
        {
            const int BM = 256, TMmin = BM - (Kmax - 1);
            p.ring = true;
            p.gx = tile_deal_grid((Lmax + TMmin - 1) / TMmin, c.nseg, p.deal_c);
            // operand rows: BM + (K - 1) * dil, + dil: the last tap's prefetch reads one tap past the end
            p.ring_off = plan_round_up((BM + Kmax * dmax) * (64 * 2 + 16), 1024);
            p.lds_bytes = (size_t)p.ring_off + 4 * 8192;
            p.valid = p.lds_bytes <= LDS_TWO_WGS;
            return p;
        }
    }
    // tallest tile that still gives every CU about three workgroups, but never a BM so small that the
    // (k-1)-row halo dominates (MT >= 2: BM >= 64 / 128 / 256 for 128 / 64 / 32 channels)
    // measured (512 frames, batch 1): BM = 64/128/256 rows (MT = 2) beats MT = 4 at every channel count — three
    // to four workgroups per CU hide the staging / epilogue phases better than taller tiles save weight traffic
    // measured (batch of 32 x 1 024 frames): once a launch has many rounds of workgroups the 128-channel stage is
    // bound by the weight stream from L2 (1 KiB of B fragment per 2 MFMAs per wave at MT = 2) and BM = 128 is 14 % faster;
    // the 64-channel stage does not care (-1 %).  The tile height never changes an output bit.
    int MT = (Cp == 128 && wgs(4) >= 8L * n_cu) ? 4 : 2;
    // 256 channels, batches: 96-row tiles (two thirds of the weight-fragment traffic per row, 10 instead of 16 % of conv2 spent
    // on halo rows at 11 taps; 80 KB of LDS and 234 registers still give two workgroups per CU): 1 010 -> 897 us per launch.
    // (The merged form would need 330 registers.)
    if (Cp == 256 && !merged && wgs(3) >= 4L * n_cu) MT = 3;
    const int mt_env = knob(ZV_PAIR_MT);
    if (mt_env == 2 || mt_env == 4 || (mt_env == 3 && Cp == 256 && !merged)) MT = mt_env;      // (the merged form of MT = 3 needs 330 registers)
    p.MT = MT;
    const int BM = 32 * MT * (4 / WN);
    const int TMmin = BM - (Kmax - 1);
    if (TMmin < 32) return p;
    // jobs differ in K: grid.x is sized for the smallest TM (the most tiles per segment), workgroups beyond a job's extent exit at once
    p.gx = tile_deal_grid((Lmax + TMmin - 1) / TMmin, c.nseg, p.deal_c);      // multiple of 8: tile_deal.h
    // rows touched: BM + taps (K rounded up to the loop's granularity, + 1 for the last prefetch) * dil.  The loop walks
    // whole taps once a tap is at least a body (CP >= 128): K + 1 taps (51 KB for the 128-channel stage: room for three
    // workgroups per CU instead of two — measured worth 0.6 %)
    // (CP = 256: exactly K taps — the prefetch one tap past the end reads rows that exist but are never used — so that the
    // 96-row tile of MT = 3 stays under 80 KB: two workgroups per CU)
    p.lds_bytes = (size_t)(BM + (Kmax + (Cp == 256 ? 0 : (Cp >= 128 ? 1 : 4))) * dmax) * (Cp * 2 + 16);
    p.valid = true;
    return p;
}

// launch_triple: njobs whole residual blocks (32 channels) in one launch
struct TriplePlan
{
    bool   valid;
    int    R, MT;                 // tile rows; resblock_triple_kernel's wave tile
    bool   lds_form;              // resblock_block32_kernel<2, R> (weights in LDS: batches) instead of resblock_triple_kernel<32, MT, R>
    int    db_mask;               // lds_form: bit j = job j keeps two weight buffers in LDS
    int    interleave;            // lds_form: > 1 = that many jobs share grid.x, interleaved per XCD
    int    deal_c, gx, gz, threads;
    size_t lds_bytes;
};
inline TriplePlan triple_plan(const BlockDesc *jobs, const ConvCall &c)
{
    TriplePlan p{};
    const int njobs = c.njobs, Lmax = c.max_rows * c.rate;
    const int v2_env = knob(ZV_TRIPLE_V2);
    // the tile height: 512 rows (the halo recompute of the 11-tap branch falls from 1.9x to 1.3x) once there are enough rows for
    // about eight rounds of such workgroups, else 256 (measured at 512 frames: 100 vs 104 us)
    const int R = ((long)Lmax * c.nseg * njobs >= 7000L * c.n_cu || v2_env == 3) ? 512 : 256;      // (ZV_TRIPLE_V2 = 3: tests force the batches' tile)
    p.R = R, p.MT = 2;
    p.deal_c = tile_deal_chunk(32);
    p.interleave = 1;
    int    gx = 8;
    size_t lds = 0, lds2 = 0;
    for (int i = 0; i < njobs; i++)
    {
        const BlockDesc &P = jobs[i];
        if (P.Cp != jobs[0].Cp || !triple_supported(P.Cp, P.K, P.dil, P.n_dil)) return p;
        const BlockTile t = block_tile(P.K, P.dil, P.n_dil, R);
        const int g = tile_deal_grid((Lmax + t.TM - 1) / t.TM, c.nseg, p.deal_c);
        gx = g > gx ? g : gx;
        const size_t rows = R + 2 * t.h2 * t.dmax + 5 * t.dmax;
        const size_t b = rows * (P.Cp * 2 + 16);
        lds = b > lds ? b : lds;
        // the LDS form: operand tile + weight buffer(s) + 2 fragments (the last B prefetch) + the block's biases
        const int    nb = ((P.K * 2 + 3) >> 2) >> 1;
        const size_t one = (size_t)plan_round_up((int)(rows * 80), 1024) + (size_t)(8 * nb + 2) * 1024 + 1024;
        const bool   db = knob(ZV_TRIPLE_DB) != 0 && one + (size_t)8 * nb * 1024 <= LDS_TWO_WGS;
        if (db) p.db_mask |= 1 << i;
        const size_t b2 = one + (db ? (size_t)8 * nb * 1024 : 0);
        lds2 = b2 > lds2 ? b2 : lds2;
    }
    if (njobs < 1 || lds > LDS_DEFAULT) return p;
    p.gx = gx, p.gz = njobs;      // multiple of 8: tile_deal.h
    // batches: the form with the weights in LDS (two workgroups per CU); ZV_TRIPLE_V2 = 0 never, 2 always, 3 always and on 512-row tiles (A/B, tests)
    if (v2_env && (R == 512 || v2_env >= 2) && lds2 <= LDS_TWO_WGS)
    {
        p.lds_form = true;
        p.interleave = knob(ZV_TRIPLE_INTERLEAVE) != 0 ? njobs : 1;
        if (p.interleave > 1) p.gx = gx * njobs, p.gz = 1;
        p.threads = R;                               // 64 (R / 32 / 2)
        p.lds_bytes = lds2;
        p.valid = true;
        return p;
    }
    p.db_mask = 0;
    p.threads = 64 * (R / 32 / p.MT);
    p.lds_bytes = lds;
    p.valid = true;
    return p;
}

// launch_block64: the first dilation pairs of njobs 64-channel branches in one launch (resblock_block64_kernel, 256-row tiles)
struct Block64Plan
{
    bool   valid;
    int    deal_c, gx, gz, threads;
    int    ring_off;              // byte offset of the weight ring in LDS
    size_t lds_bytes;
};
inline Block64Plan block64_plan(const BlockDesc *jobs, const ConvCall &c)
{
    Block64Plan p{};
    const int Lmax = c.max_rows * c.rate;
    p.deal_c = tile_deal_chunk(64);
    int gx = 8, rows_max = 0;
    for (int i = 0; i < c.njobs; i++)
    {
        const BlockDesc &P = jobs[i];
        if (!block64_supported(P.Cp, P.K, P.dil, P.n_dil)) return p;
        const BlockTile t = block_tile(P.K, P.dil, P.n_dil, 256);
        const int g = tile_deal_grid((Lmax + t.TM - 1) / t.TM, c.nseg, p.deal_c);
        gx = g > gx ? g : gx;
        const int rows = 256 + 2 * t.h2 * t.dmax + 2 * t.dmax;
        rows_max = rows > rows_max ? rows : rows_max;
    }
    p.gx = gx, p.gz = c.njobs, p.threads = 256;
    p.ring_off = plan_round_up(rows_max * (64 * 2 + 16), 1024);
    p.lds_bytes = (size_t)p.ring_off + 4 * 8192;
    p.valid = c.njobs >= 1 && p.lds_bytes <= LDS_TWO_WGS;
    return p;
}

}  // namespace zv
