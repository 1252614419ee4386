// kernels.h — host-visible descriptors and launchers of the HIP kernels (gfx950 only).
//
// Activation layout in HBM ("tl" = time-major / channels-last): x[t * ld + c], c < Cp, where
// Cp = C rounded up to 16 and the pad channels hold zeros.  This is the layout of the stage
// boundaries themselves (hidden[t*E+e], mel[t*80+m] — reference src/fs2encoder.cpp:634,
// src/stylettsdec.cpp:432-441), so no transposes exist anywhere in the schedule, and it makes an
// MFMA operand fragment (8 consecutive input channels at one time step) one 16-byte LDS read.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_plan.h"     // the launchers' plans: ConvPrologue, conv_gemm_groups / _tiles / _units, pair_supported, triple_supported, block64_supported, TRIPLE_MAX_DIL
#include "voc_plan.h"
#include "stage_plan.h"    // att_plan, linear_plan, lr_plan, layernorm_tail_ok; the schedules' enc_plan and dec_plan
#include "level.h"        // volume controls: LEVEL_CHUNK_SAMPLES, LEVEL_VOL_STRIDE, LevelRow
#include "envelope.h"     // amplitude envelope: ENV_CTL_STRIDE, ENV_MAX_RAMP, ENV_MAX_GAIN
#include "contour.h"      // level contour: CONTOUR_CHUNK_FRAMES, ContourRow
#include "pitch.h"        // pitch track: PITCH_CHUNK_FRAMES, PITCH_PARAM_STRIDE, the rows
#include "bands.h"        // band levels: BANDS_TILE_FRAMES, BANDS_PARAM_STRIDE, BANDS_ROW_STRIDE
#include "filter.h"       // waveform filter: FILTER_TILE, FILTER_PARAM_STRIDE
#include "mel.h"          // mel analysis: MEL_SLAB_STRIDE, MEL_TABLE_BYTES, the parameter block
#include "align.h"        // mel alignment: AlignPair, AlignRow, the tiles and ALIGN_DP_ROWS
#include "loudness.h"     // loudness: LoudJob, LoudSeg, LoudAsk, LoudRow, LoudFilter
#include "limiter.h"      // limiter: LimitJob, LimitSeg, LimitAsk, LimitRow
#include "resample.h"     // resampling: ResampleJob, ResampleSeg, ResampleRow

// Timing-only ablation bits (`dbg` fields of the job structs: skip staging / MFMA loops / stores ... — WRONG results) exist only
// in diagnostic builds (-DZV_DIAG, see knobs.h).  In the shipped library every read of them is the constant 0 and the code
// they select is compiled out.
#ifdef ZV_DIAG
#define ZV_DBGBITS(x) (x)
#else
#define ZV_DBGBITS(x) 0
#endif

namespace zv
{

__host__ __device__ static inline int round_up(int x, int a) { return (x + a - 1) / a * a; }

// ---- segments: many utterances per launch ---------------------------------------------------------
// A batch is laid out as ONE row-concatenated buffer per tensor: utterance u owns rows [row0, row0 + rows) (frames
// for the decoder / vocoder, phonemes for the encoder).  Every kernel maps a workgroup to (segment, tile inside the
// segment) and treats the segment's ends as the sequence ends (zero padding of the convs, InstanceNorm / attention
// extents): each utterance keeps its own (N, T), exactly as if it had been run alone (reference
// src/fs2encoder.cpp:103-110, src/stylettsdec.cpp:359: no masks, no batch padding).  The table lives in HBM, so one
// captured hipGraph serves every batch that fits its capacity; a single utterance travels inline in the kernel
// arguments (`one`) and needs no table.  `rate` (per launch) converts base rows to the rows of a stage
// (HiFi-GAN stages: 1, 5, 25, 100, 300 samples per frame).
struct Seg
{
    int32_t row0, rows;      // base units (frames or phonemes)
    int32_t aux;             // encoder: num_phonemes the length regulator walks (reference src/fs2encoder.cpp:622)
    int32_t pad;
};
struct Segs
{
    const Seg *tab;          // device table [nseg] or null
    int        nseg;         // table entries; the grid covers all of them, empty ones (rows = 0) exit at once
    int        max_rows;     // >= rows of every entry (grid sizing), base units
    Seg        one;          // the segment when tab == null
};
__host__ __device__ static inline Seg seg_at(const Segs &s, int u)
{
    Seg g = s.tab ? s.tab[u] : s.one;
#if defined(__HIP_DEVICE_COMPILE__)
    // the table entry is the same for every lane of a workgroup: keep it (and every pointer / buffer descriptor derived
    // from it) in scalar registers — a descriptor in vector registers costs a waterfall loop per buffer instruction
    g.row0 = __builtin_amdgcn_readfirstlane(g.row0);
    g.rows = __builtin_amdgcn_readfirstlane(g.rows);
    g.aux = __builtin_amdgcn_readfirstlane(g.aux);
#endif
    return g;
}
static inline Segs segs_single(int rows, int aux = 0)
{
    Segs s;
    s.tab = nullptr;
    s.nseg = 1;
    s.max_rows = rows;
    s.one.row0 = 0;
    s.one.rows = rows;
    s.one.aux = aux;
    s.one.pad = 0;
    return s;
}

// ---- fused Conv1d ("same" length, stride 1) as implicit GEMM on v_mfma_f32_32x32x16_f16 -----------
//
//   out[t][oc] = epilogue( sum_{tap, ic} f16( prologue(x)[t + tap*dil - pad][ic] ) * w[tap][ic][oc] )
//
// which is ggml_conv_1d = im2col(F16) + mul_mat (reference ggml/src/ggml.c:3769-3786): operands f16,
// products exact in f32, f32 accumulation.  Out-of-range taps are zeros *after* the prologue.

// (ConvPrologue, the `pro` of a job: conv_plan.h)
struct ConvJob
{
    // input
    const void  *x0, *x1, *x2;
    int          ldx;
    int          pro;
    float        slope, pscale;
    const float *pa, *pb;        // per-channel: NORM g,b | MELNORM mean,scale
    const float *pstat;          // per-channel (mean, rstd) pairs
    // geometry
    int          L, Cin_p, Cout_p, K, dil, pad;
    int          ck;             // input-channel chunk staged per LDS pass (set at pack time)
    // weights packed in MFMA-fragment order (see pack_conv_weight), bias padded to 32*ntiles
    const void  *w;
    const void  *w8;             // the same weights in conv_gemm_kernel's stream order (pack_conv_weight_gemm: 16 x 16 x 32 fragments), or null
    const float *bias;
    // epilogue: v = acc + bias; v += res; v *= escale; v = lrelu(v, oslope) if eact; store f32 | f16
    const float *res;
    int          ldres;
    float        escale;
    int          eact;
    float        oslope;
    int          out_f16;
    void        *out;
    int          ldo;
    int          dbg;            // timing-only ablation bits (ZV_DBG env): 1 no staging loads, 2 no MFMA, 4 no epilogue
    // per-segment strides (floats) of the prologue's per-channel vectors: 0 = one vector for every segment
    int          pstat_seg, pab_seg;
    // InstanceNorm statistics of the OUTPUT, produced by the epilogue: per (segment, 32-row block, channel) the f64
    // pair (sum, sum of squares) of the stored values, combined later in a fixed order by launch_stats_finalize
    double      *stat_part;      // [nseg][stat_nblk][stat_C][2] or null
    int          stat_nblk, stat_C;
};

constexpr int CONV_MAX_JOBS = 4;
struct ConvJobs
{
    ConvJob j[CONV_MAX_JOBS];
    Segs    segs;
    int     rate;                // rows per base row of this launch
    int     tps;                 // row tiles per segment (grid.x = tps * nseg)
    int     nt_begin;            // first output tile of this launch (the tiles before it belong to conv_gemm_kernel)
    int     order;               // conv_gemm_kernel: workgroup order (ZV_GEMM_ORDER: 0 plain, 1 one group per XCD, 2 the 9-tile group first)
    int     tile_bytes;          // single-utterance form of conv1d_mfma_kernel: bytes of one of its two LDS tiles (set by the launcher)
    int     xcd_ny, xcd_nx;      // single-utterance form: channel groups / row tiles of the launch when the groups are dealt over the XCDs (0: plain grid)
    int     xcd_spread;          // ... and whether a launch with fewer than 8 groups deals each group's row tiles over several XCDs (conv_xcd.h)
    int     warm;                // single-utterance forms: the row tiles of a channel group warm their XCD's L2 with the group's weights first
#ifdef ZV_STAMPS
    unsigned long long *stamp;   // diagnostic build: the phase-stamp buffer this launch writes (stamp_buffer()), or null
#endif
};

// bytes of one packed conv weight: [ntile32][chunk][tap][kc][lane 64][8 halfs]
size_t packed_conv_weight_halfs(int Cin_p, int Cout_p, int K);
// input-channel chunk per LDS pass: min(Cin_p, ck_max); ck_max <= 0 means the kernel's maximum (256)
int    conv_pick_ck(int Cin_p, int ck_max = 0);
// host-side repack of a GGUF conv weight (ggml ne [K, IC, OC], f16, k fastest) into fragment order
void   pack_conv_weight(const uint16_t *w, int K, int IC, int OC, int Cin_p, int Cout_p, int ck, uint16_t *dst);
// conv_gemm_kernel (batches of wide f16-operand convs): [group of 8 output tiles][unit = (256-chunk, tap, 64-channel block)][k16 step 4]
// [tile 8][lane][8 halfs]: one unit = 32 KiB contiguous = what one workgroup moves into LDS per step of its K loop.  Only whole
// groups of 8 tiles are packed (conv_plan.h: conv_gemm_groups / conv_gemm_tiles / conv_gemm_units); the remaining tiles run on conv1d_mfma_kernel.
size_t conv_gemm_weight_halfs(int Cin_p, int Cout_p, int K);
void   pack_conv_weight_gemm(const uint16_t *w, int K, int IC, int OC, int Cin_p, int Cout_p, uint16_t *dst);
// all jobs of one launch share the segments, Cout_p and the tile configuration; job.L is ignored (rows come from segs)
hipError_t launch_conv(hipStream_t s, const ConvJob *jobs, int njobs, int n_cu, const Segs &segs, int rate);

// ---- fused HiFi-GAN dilation pair (reference src/hifigan.cpp:99-182, one loop iteration):
//   out = y + ( conv(lrelu(conv(lrelu(y), k, dil) + b1), k, 1) + b2 )
// in ONE launch: xt never leaves LDS, y is read once (+ halo) and written once -> 8 B/element of HBM traffic
// instead of the 20 B/element the two separate convs are accounted for algorithmically.
struct PairJob
{
    const float *y;          // [L][Cp] f32
    float       *out;        // [L][Cp] f32, must not alias y (neighbour workgroups read y's halo)
    const void  *w1, *w2;    // packed by pack_pair_weight16 (16 x 16 x 32 fragments; conv1: A-operand form, conv2: B-operand form)
    const void  *w1r, *w2r;  // the same as the stream resblock_pair64_kernel moves through its LDS ring (pack_pair_weight_ring), or null
    const float *b1, *b2;
    int          L, Cp, K, dil;
    float        slope;
    int          dbg;
    // the running MRF sum, branch by branch (reference src/hifigan.cpp:300-315: (y0 + y1) + y2): when sum_out is set the pair's
    // result v goes there instead of `out`, as sum_in + v (or v itself for the first branch, sum_in null); may be the same buffer
    const float *sum_in;
    float       *sum_out;
};
constexpr int PAIR_MAX_JOBS = 3;
struct PairJobs
{
    PairJob j[PAIR_MAX_JOBS];
    Segs    segs;
    int     rate;
    int     njobs, kmax;
    int     deal_c;              // tile_deal.h: tiles per chunk of the segments' deal over the XCDs (set by the launcher)
#ifdef ZV_STAMPS
    unsigned long long *stamp;   // diagnostic build: the phase-stamp buffer this launch writes (stamp_buffer()), or null
#endif
    float  *merge_out;           // non-null: store (out_0 + out_1) + out_2 here instead of the jobs' own outputs
    int     ring_off;            // resblock_pair64_kernel: byte offset of the weight ring in LDS (set by the launcher)
};
// (conv_plan.h pair_supported: whether a ResBlock conv pair with Cp (padded) channels and K taps can run on the fused kernel)
size_t     pair_weight_halfs(int Cp, int K);
// GGUF conv weight (ggml ne [K, C, C], f16) -> fused-kernel layout
void       pack_pair_weight(const uint16_t *w, int K, int C, int Cp, uint16_t *dst);
// the same weight in v_mfma_f32_16x16x32_f16 fragment order (resblock_pair_kernel, resblock_block32_kernel); conv2_layout: the
// pair's second conv (B-operand form: column c of tile wt = channel 2c + wt), else the first (A-operand form: row r = channel 16 wt + r)
size_t     pair_weight16_halfs(int Cp, int K);
void       pack_pair_weight16(const uint16_t *w, int K, int C, int Cp, uint16_t *dst, bool conv2_layout);
// the same weight as the stream resblock_pair64_kernel / resblock_block64_kernel move through their LDS ring: [tap][step of 32 channels][ntile][wt][lane][8 halfs]
size_t     pair_ring_weight_halfs(int Cp, int K);
void       pack_pair_weight_ring(const uint16_t *w, int K, int C, int Cp, uint16_t *dst, bool conv2_layout);
// merge_out (may be null): the jobs share every time tile and only the sum of their outputs, (out_0 + out_1) + out_2, is
// stored there (the MRF sum of a stage's last dilation pair); the jobs' own `out` pointers are then unused
hipError_t launch_pair(hipStream_t s, const PairJob *jobs, int njobs, int n_cu, const Segs &segs, int rate, float *merge_out = nullptr);

// ---- a whole HiFi-GAN residual block (reference src/hifigan.cpp:74-185: the loop over all dilations) in ONE launch:
// a workgroup keeps a 256-row f32 tile of y in LDS, runs the n_dil fused pairs on it and writes the centre rows once.
// HBM traffic per element: 4 B in (x halo factor) + 4 B out for the whole block instead of once per dilation pair.
struct TripleJob
{
    const float *y;                       // [L][Cp] f32 block input (may be shared by several jobs)
    float       *out;                     // [L][Cp] f32 block output, must not alias y
    // launch_triple: w1 / w2 in pack_pair_weight layout (resblock_triple_kernel: 32 x 32 x 16 fragments) and w1x / w2x in
    // pack_pair_weight16 layout (resblock_block32_kernel); launch_block64: w1 / w2 the ring stream (pack_pair_weight_ring)
    const void  *w1[TRIPLE_MAX_DIL], *w2[TRIPLE_MAX_DIL];
    const void  *w1x[TRIPLE_MAX_DIL], *w2x[TRIPLE_MAX_DIL];
    const float *b1[TRIPLE_MAX_DIL], *b2[TRIPLE_MAX_DIL];
    int          dil[TRIPLE_MAX_DIL];
    int          n_dil;
    int          L, Cp, K;
    float        slope;
    int          dbg;
};
struct TripleJobs
{
    TripleJob j[PAIR_MAX_JOBS];
    Segs      segs;
    int       rate;
    int       deal_c;            // tile_deal.h: tiles per chunk of the segments' deal over the XCDs (set by the launcher)
    int       interleave;        // resblock_block32_kernel: > 1 = that many jobs share grid.x, interleaved per XCD
    int       db_mask;           // resblock_block32_kernel: bit j = job j keeps two weight buffers in LDS (set by the launcher)
    int       ring_off;          // resblock_block64_kernel: byte offset of the weight ring in LDS (set by the launcher)
#ifdef ZV_STAMPS
    unsigned long long *stamp;   // diagnostic build: the phase-stamp buffer this launch writes (stamp_buffer()), or null
#endif
};
// (conv_plan.h triple_supported / block64_supported: the blocks the two launchers take)
// several dilation pairs of a 64-channel block in one launch (resblock_block64_kernel): w1 / w2 in pack_pair_weight_ring layout
hipError_t launch_block64(hipStream_t s, const TripleJob *jobs, int njobs, const Segs &segs, int rate);
hipError_t launch_triple(hipStream_t s, const TripleJob *jobs, int njobs, int n_cu, const Segs &segs, int rate);

// ---- vocoder tail: lrelu(0.01) -> conv k7 (C -> 1) + b -> tanh (src/hifigan.cpp:324-345) ----------
struct OutConvArgs
{
    const float *x0, *x1, *x2;   // MRF branches of the last stage, summed in the prologue
    int          ldx, L, C, K;
    float        pscale, slope;
    const uint16_t *w;           // f16 [K][Cp]
    float        bias;
    float       *out;            // wav[L]
    Segs         segs;
    int          rate;
    int          runs;           // segs is a run table (launch_voc_runs): samples of the frames behind seg.aux land seg.pad frames further on
};
hipError_t launch_out_conv(hipStream_t s, const OutConvArgs &a);

// ---- InstanceNorm statistics over time (ggml_norm, ggml-cpu.c:6880-6929: mean and biased variance in f64, --------
// scale = 1/sqrtf(var + eps)).  Two steps: per (segment, 32-row block, channel) partial sums (sum, sum of squares, both
// f64; written by the producing conv's epilogue, by launch_stats_partial for tensors that no conv of ours produced,
// or by launch_norm_apply for its own output), then launch_stats_finalize adds the blocks of a segment in block order
// and stores (mean, rstd).  The 32-row blocks do not depend on any tile shape, so neither do the statistics.
//   part[((u * nblk) + blk) * C + c] = double2(sum, sumsq);  nblk >= ceil(max_rows * rate / 32)
//   stat[u * stat_seg + 2 * (c_off + c) + {0, 1}] = mean, rstd
// packed (here and in launch_norm_apply; rate must be 1): segs is the run table of densely packed decoding (dec_runs.h), whose row0
// are multiples of 32 in ONE packed row space — segment u's blocks are then part[(row0 / 32 + blk) * C + c], where a conv over the
// packed rows as one segment stores them too, and nblk only bounds the blocks of one segment
hipError_t launch_stats_partial(hipStream_t s, const float *x, int ldx, int C, double *part, int nblk, const Segs &segs, int rate,
                                int packed = 0);
// dec_runs (here and in launch_norm_act_f16), a sum of:
//   DEC_TAB_RUNS        segs is a decoder run table (launch_dec_runs) — behind block seg.aux - 1 that block's pair is added seg.pad
//                       more times and the sums are divided by rows + 32 * pad (dec_runs.h); rate must be 1
//   DEC_TAB_PACKED      ... of densely packed decoding: the blocks of `part` as under `packed` above
//   DEC_TAB_CONV_TAIL   ... and `part` was stored by a conv over the packed rows as one segment, whose last block of a segment with
//                       rows % 32 != 0 also counts guard rows: that block's pair is summed again from x (the tensor the conv
//                       stored, ldx floats per row, channel c in column c) in the epilogue's order — dec_pack_tail_pair
constexpr int DEC_TAB_RUNS = 1, DEC_TAB_PACKED = 2, DEC_TAB_CONV_TAIL = 4;
hipError_t launch_stats_finalize(hipStream_t s, const double *part, int nblk, int C, float eps, float *stat, int stat_seg,
                                 int c_off, const Segs &segs, int rate, int dec_runs = 0, const float *x = nullptr, int ldx = 0);
// y[t][c] = ((x - mean) * rstd) * g[c] + b[c]; `part` (may be null) receives the partial sums of y
hipError_t launch_norm_apply(hipStream_t s, const float *x, int ldx, int C, const float *stat, int stat_seg, const float *g,
                             const float *b, float *y, int ldy, double *part, int nblk, const Segs &segs, int packed = 0);

// out[i] = f16(lrelu(((x0[i] + x1[i]) + x2[i]) * pscale, slope)) over n contiguous elements (x1 = x2 = null: x0[i] * pscale): the
// operand pre-pass of the upsample convs that run on conv_gemm_kernel
hipError_t launch_act_f16(hipStream_t s, const float *x0, const float *x1, const float *x2, float pscale, float slope, void *out, size_t n);
// y = f16(lrelu(((x - mean) * rstd) * g + b, slope)) for C channels (a multiple of 4): the PRO_NORM_ACT operand written out
// once (PRO_RAW_F16 consumers).  Channels below Cpart get their statistics from `part` (and store them in `stat`), the
// others read `stat`.  g / b: per-segment stride gb_seg (0 = shared).  yraw (may be null, same layout as y): f16(x) itself — the
// operand of the block's 1x1 shortcut conv (reference src/stylettsdec.cpp:132-140,287-296 converts x to f16 in its im2col).
// DEC_TAB_PACKED: y and yraw also get zeros in the guard rows [rows, dec_pack_slot(rows)) of every segment's slot.
hipError_t launch_norm_act_f16(hipStream_t s, const float *x, int ldx, int C, const double *part, int nblk, int Cpart, float eps,
                               float *stat, int stat_seg, const float *ga, const float *be, int gb_seg, float slope, void *y,
                               int ldy, const Segs &segs, void *yraw = nullptr, int dec_runs = 0);

// ---- f32 linear layers: y[n][o] = dot(W[o][:], x[n][:]) + b[o] (ggml_mul_mat on f32 weights) --------
// `extra` (may be null) is a second per-output addend applied after the bias: (acc + b[o]) + extra[o]
// (AdaIN: gamma = h[:C] + 1, reference src/stylettsdec.cpp:186-189)
hipError_t launch_linear(hipStream_t s, const float *x, int ldx, int in, const float *W, const float *b, int out, float *y,
                         int ldy, const float *extra, const Segs &segs);

// ---- tests (zv_debug_mfma_chain): out[32][32] = c0 + a[32][K] * b[K][32] as ONE k-ordered chain of one wave, on the matrix-core
// instruction the kernels of `form` use — 0: v_mfma_f32_32x32x16_f16, 1: v_mfma_f32_16x16x32_f16 (a, b f16), 2:
// v_mfma_f32_32x32x2_f32 (a, b f32).  K a multiple of 32.  All pointers device.
hipError_t launch_mfma_chain(hipStream_t s, int form, const void *a, const void *b, const float *c0, int K, float *out);

// ---- encoder pieces (reference src/fs2encoder.cpp) -------------------------------------------------
hipError_t launch_embed(hipStream_t s, const int32_t *ids, const int32_t *puncts, const float *wemb, int emb,
                        const float *pemb, int pdim, const float *posenc, float *x, int ld, const Segs &segs);
// softmax(q k^T * inv_temp) v per (segment, head); q, k, v [rows][ld] token-major, heads side by side
hipError_t launch_attention(hipStream_t s, const float *q, const float *k, const float *v, int ld, int H, int dk,
                            float inv_temp, float *o, int ldo, const Segs &segs);
// Prosody controls (include/zerovox_amd.h zv_prosody): f32 [segment][CTL_STRIDE], one row per utterance of the batch, read by the
// kernels below as ctl[segment * CTL_STRIDE + field].  A null ctl is the uncontrolled instruction path (uniform branch).
constexpr int CTL_STRIDE = 8;
constexpr int CTL_DURATION = 0;        // duration_scale
constexpr int CTL_PITCH = 1;           // pitch_scale, pitch_shift
constexpr int CTL_ENERGY = 3;          // energy_scale, energy_shift
constexpr int CTL_TARGET = 5;          // target frames as an exact f32 integer, 0 = none (launch_fit_durations; slots 6, 7 unused)
// Per-phoneme controls (include/zerovox_amd.h zv_phoneme_controls): f32 [token row][PCTL_STRIDE], indexed by ABSOLUTE token row (so
// the batch's segments, tokens_merged() and the inline single segment index them alike).  A null pctl is the uncontrolled path.
constexpr int PCTL_STRIDE = 4;
constexpr int PCTL_FRAMES = 0;         // forced frames, -1 = none (integers up to 32768 are exact in f32)
constexpr int PCTL_DURATION = 1;       // duration scale, after the utterance's
constexpr int PCTL_PITCH = 2;          // pitch shift, after the utterance's scale / shift
constexpr int PCTL_ENERGY = 3;         // energy shift

// y = LayerNorm(x + res) * w + b  over the C real channels (res may be null); channels [C, Cp) are zeroed
hipError_t launch_add_layernorm(hipStream_t s, const float *x, int ldx, const float *res, int ldr, int C, int Cp,
                                const float *w, const float *b, float eps, float *y, int ldy, const Segs &segs);
// the same LayerNorm with a tail in the same launch (short utterances: every launch is latency), each part optional:
//   y += post[segment][:]                                   (post_seg: floats between segments' vectors)
//   pred[row] = dot(y[row][:C], dot_w) + dot_b[0]           (launch_rowdot's chain)
//   bucket[row] = clamp((int)(pred * (nbins - 1) + 0.5)); feat[row][:embC] += emb[bucket][:]   (launch_bucket_embed_add; needs dot_w)
//     ctl (or null): pred -> pred * ctl[seg][ctl_field] + ctl[seg][ctl_field + 1] before the bucket (pred itself is stored raw)
//     pctl (or null): per-phoneme rows offset to their field (PCTL_PITCH / PCTL_ENERGY): then pred -> pred + pctl[row * PCTL_STRIDE]
// stage_plan.h layernorm_tail_ok(C): the tail exists in the rows-in-registers form only (C <= 768); a wider C is refused
hipError_t launch_layernorm_tail(hipStream_t s, const float *x, int ldx, const float *res, int ldr, int C, int Cp, const float *w,
                                 const float *b, float eps, float *y, int ldy, const Segs &segs, const float *post, int post_seg,
                                 const float *dot_w, const float *dot_b, float *pred, const float *emb, int nbins, int embC, float *feat,
                                 int ldf, int32_t *bucket, const float *ctl = nullptr, int ctl_field = 0,
                                 const float *pctl = nullptr);
// x[row][:] += v[segment][:]
hipError_t launch_add_rowvec(hipStream_t s, float *x, int ld, int C, const float *v, int v_seg, const Segs &segs);
// pred[n] = dot(x[n][:], w) + b
hipError_t launch_rowdot(hipStream_t s, const float *x, int ld, int C, const float *w, const float *b, float *y, const Segs &segs);
// bucket[n] = clamp((int)(pred*(nbins-1) + 0.5), 0, nbins-1); x[n][:] += emb[bucket[n]][:]
//   ctl (or null): pred -> pred * ctl[seg][ctl_field] + ctl[seg][ctl_field + 1] first
//   pctl (or null): per-phoneme rows offset to their field, then pred -> pred + pctl[n * PCTL_STRIDE]
hipError_t launch_bucket_embed_add(hipStream_t s, const float *pred, int nbins, const float *emb, int C, float *x, int ld,
                                   int32_t *bucket, const Segs &segs, const float *ctl = nullptr, int ctl_field = 0,
                                   const float *pctl = nullptr);
// device length regulator: rounded durations of the first `aux` tokens of a segment -> inclusive scan (cum[], one int
// per token row) -> gather into the segment's frames, zero tail; n_frames[segment] = frames
//   ctl (or null): each duration is multiplied by ctl[seg][CTL_DURATION] (f32) before it is rounded
//   pctl (or null): then by pctl[row][PCTL_DURATION]; after rounding, pctl[row][PCTL_FRAMES] >= 0 replaces d by min(frames, T)
hipError_t launch_length_regulator(hipStream_t s, const float *feat, int ld, const float *logdur, int C, float *hidden,
                                   int ldh, int32_t *cum, int32_t *n_frames, const Segs &tokens, const Segs &frames,
                                   const float *ctl = nullptr, const float *pctl = nullptr);

// target durations (include/zerovox_amd.h "target durations", fit_durations.h): for every segment whose ctl[seg][CTL_TARGET] > 0 the
// integer durations that sum to the target replace pctl[row][PCTL_FRAMES] of the segment's first `aux` token rows IN PLACE (the
// pointer is const for every other kernel), so the length regulator launched next takes them as forced frames.  ctl and pctl must
// both be set; at most FIT_MAX_TOKENS tokens per segment (two 64-bit LDS entries each, with the workgroup's 8 KiB of sums inside the
// 64 KiB a workgroup gets by default), else hipErrorInvalidValue
constexpr int FIT_MAX_TOKENS = 3584;
hipError_t launch_fit_durations(hipStream_t s, const float *logdur, const float *ctl, const float *pctl, const Segs &tokens,
                                const Segs &frames);

// ---- fitted mode (include/zerovox_amd.h zv_synthesize_fitted): the decoder and the vocoder run over the frames the length regulator
// filled instead of the capacity.  live[u] = {frames[u].row0, min(n_frames[u], frames[u].rows), 0, 0} for the nseg entries of
// `frames` (table or inline segment), written on the device so that the schedule stays one graph without a host round trip
hipError_t launch_live_frames(hipStream_t s, const int32_t *n_frames, Seg *live, const Segs &frames);
// x[row][0 .. C) = 0 for the rows [live[u].rows * rate, frames[u].rows * rate) of every segment (x: rows of C floats at `rate` rows per
// base row, laid out by `frames`): what the fitted schedule leaves unwritten of a segment's capacity
hipError_t launch_zero_tail(hipStream_t s, float *x, int C, const Segs &frames, const Segs &live, int rate);

// ---- run-shortened vocoding (unfitted path): behind an utterance's end the mel rows are bit-identical, and over a run of identical
// rows the vocoder's output is one frame, repeated (it is shift-invariant with a reach of H = Model::vocoder_halo_frames() frames).
// For every segment of `frames`, with [a, b) its first longest run of bitwise-equal mel rows and Rmin = 2H + 1:
//   taken (b - a >= Rmin + VOC_RUN_MARGIN): mel_c = rows [0, a + Rmin) ++ rows [b, T);  runs[u] = {row0, T - (b - a) + Rmin, aux = a + H, pad = b - a - Rmin}
//   otherwise:                              mel_c = mel;                                 runs[u] = {row0, T, aux = T, pad = 0}
// aux is the SPLIT frame and pad the SHIFT: compact frame f' is wav frame f' up to the split and f' + shift behind it
// (OutConvArgs::runs); wav frames (split, split + shift] are copies of frame `split` (launch_voc_run_fill).
// eq: int32 scratch, one per row of the batch.  mel [rows][M] dense.  No host round trip: one graph replays for any lengths.
constexpr int VOC_RUN_MARGIN = 16;      // frames a run must save to be taken: below a row tile of the narrow stages nothing is saved
hipError_t launch_voc_runs(hipStream_t s, const float *mel, int M, float *mel_c, int32_t *eq, Seg *runs, const Segs &frames, int H);
hipError_t launch_voc_run_fill(hipStream_t s, float *x, const Segs &runs, int rate);

// ---- run-shortened decoding (unfitted path, dec_runs.h): behind an utterance's n frames `hidden` is zero, so every tensor of the
// decoder is constant over the rows [n + R, T - R) (R: the reach of its 3-tap convs) and the decoder runs over rows [0, a) ++ [b, T)
// only, a and b multiples of the 32-row statistics block.  For every segment of `frames` (capacity T), from the regulator's counts:
//   runs[u] = {row0, rows_c = a + (T - b), aux = a / 32, pad = G = (b - a) / 32}     taken (dec_run)
//   runs[u] = {row0, T, 0, 0}                                                        otherwise
// Every decoder launch takes its extents from this table; the statistics add the dropped blocks back (launch_stats_finalize).  No
// host round trip: one graph replays for any lengths.
// packed (densely packed decoding, dec_runs.h): runs[u].row0 = row0_p[u], the sum of dec_pack_slot(rows_c) over the segments in front
// of u, and runs has one entry more: runs[nseg] = {0, L_p, 0, 0}, the packed rows as the ONE segment the convs run over
hipError_t launch_dec_runs(hipStream_t s, const int32_t *n_frames, Seg *runs, const Segs &frames, int R, int packed = 0);
// xp[runs[u].row0 + t][0 .. C) = x[frames[u].row0 + t][0 .. C) for t < runs[u].rows and zeros for the guard rows up to
// dec_pack_slot(rows): a tensor of the capacity layout into the packed one.  C a multiple of 4; x and xp must not overlap
hipError_t launch_dec_pack_rows(hipStream_t s, const float *x, float *xp, int C, const Segs &runs, const Segs &frames);
// mel[row0 + t][0 .. M) = mel_c[runs[u].row0 + dec_run_compact_row(t)][0 .. M) for all T rows of every segment of `frames`: the
// compact mel (the rows the decoder computed: at the segment's own row0, or at its slot of the packed rows) expanded to the
// capacity.  mel_c and mel must not overlap
hipError_t launch_dec_run_expand(hipStream_t s, const float *mel_c, float *mel, int M, const Segs &runs, const Segs &frames);

// ---- volume controls (include/zerovox_amd.h "volume controls", level.h): two passes over the finished waveform wav [rows * hop], laid
// out by `frames` (the CAPACITY table or inline segment); n_frames [nseg] are the regulator's counts on the device, so the speech of
// segment u is its first min(n_frames[u], rows) * hop samples.
//   measure: slab[u * level_chunks + c] = {sum of squared 1.19 magnitudes, peak bits, 0} of chunk c (LEVEL_CHUNK_SAMPLES samples) of
//            segment u's speech, one 16-byte store per workgroup; chunks behind the speech are not written
//   apply:   adds a segment's entries, takes the gain from vol[u * LEVEL_VOL_STRIDE + {0, 1, 2}] = {gain, target_rms, peak_ceiling}
//            (level_report), multiplies all rows * hop samples of the segment by it and stores levels[u]
// slab: 16-byte aligned, nseg * level_chunks(frames.max_rows, hop) entries of 16 bytes; levels: 16-byte aligned.  No atomics, nothing
// to zero: apply reads only what measure has stored in the same run.
int        level_chunks(int max_rows, int hop);
hipError_t launch_level_measure(hipStream_t s, const float *wav, const int32_t *n_frames, void *slab, const Segs &frames, int hop);
hipError_t launch_level_apply(hipStream_t s, float *wav, const int32_t *n_frames, const void *slab, const float *vol, LevelRow *levels,
                              const Segs &frames, int hop);

// ---- amplitude envelope (include/zerovox_amd.h "amplitude envelope", envelope.h): two passes ahead of the volume passes, over the same
// finished waveform.  cum [token rows] is the length regulator's scan and gain [token rows] the per-phoneme gains, both indexed by
// absolute token row (`tokens`); env [nseg][ENV_CTL_STRIDE] = {ramp_frames, fade_in_samples, fade_out_samples, unused}; n_frames [nseg]
// the regulator's counts; `frames` the CAPACITY table or inline segment.
//   knots: knots[frames[u].row0 + u + f] = B[f], f = 0 .. nf of segment u (uint32; the table has capacity rows + nseg entries); a segment
//          without speech writes nothing
//   apply: multiplies all rows * hop samples of every segment by the rule's per-sample gain (env_sample_gain), in place
// No atomics, nothing to zero: apply reads only the knots of the same run.  env_hop_supported: the apply pass keeps the knots of one
// chunk of LEVEL_CHUNK_SAMPLES samples in LDS, which bounds the hop from below (10 samples); launch_env_apply refuses any other.
bool       env_hop_supported(int hop);
hipError_t launch_env_knots(hipStream_t s, const int32_t *cum, const float *gain, const int32_t *env, const int32_t *n_frames,
                            uint32_t *knots, const Segs &tokens, const Segs &frames);
hipError_t launch_env_apply(hipStream_t s, float *wav, const int32_t *n_frames, const uint32_t *knots, const int32_t *env,
                            const Segs &frames, int hop);

// ---- level contour (include/zerovox_amd.h "level contour", contour.h): two passes behind the volume passes, over the waveform the
// caller receives.  `frames` is the CAPACITY table or inline segment, `tokens` the token table; both passes index by ABSOLUTE row.
//   frames:   slab[frames[u].row0 + f] = {S_f lo, S_f hi, P_f, 0} for every frame f of every segment's capacity, 16 bytes each, and,
//             where rows is not null, rows[frames[u].row0 + f] = {rms, peak} of the frame
//   phonemes: rows[tokens[u].row0 + i] = {rms, peak} of phoneme i, for every token row of every segment; its frames come from cum [token
//             rows], the length regulator's scan, clipped to the segment's capacity as the phoneme timings are (contour_extent)
// slab: 16-byte aligned, one entry per frame row; rows: 8-byte aligned.  No atomics, nothing to zero: phonemes reads only what frames
// has stored in the same run.  The frames pass reads whole 16-byte loads per frame: launch_contour_frames refuses a hop that is no
// multiple of 4 (contour_hop_supported) — the loader accepts hop 300 alone, so no scalar path could ever run.
bool       contour_hop_supported(int hop);
hipError_t launch_contour_frames(hipStream_t s, const float *wav, void *slab, ContourRow *rows, const Segs &frames, int hop);
hipError_t launch_contour_phonemes(hipStream_t s, const int32_t *cum, const void *slab, ContourRow *rows, const Segs &tokens,
                                   const Segs &frames, int hop);

// ---- pitch track (include/zerovox_amd.h "pitch track", pitch.h): two passes behind the level contour's, over the waveform the caller
// receives.  `frames` is the CAPACITY table or inline segment, `tokens` the token table; both passes index by ABSOLUTE row.
//   frames:   slab[frames[u].row0 + f] = {Fq, voiced} for every frame f of every segment's capacity, 8 bytes each, and, where rows is
//             not null, rows[frames[u].row0 + f] = {f0_hz, strength}.  par [segments][PITCH_PARAM_STRIDE]: each segment's resolved
//             parameters (pitch_params_resolve), read at run time; a row outside the rule's bounds makes its segment's waves return
//             without a store.  A span never leaves its segment's own samples [row0 * hop, (row0 + rows) * hop).
//   phonemes: rows[tokens[u].row0 + i] = {mean f0 of the voiced frames, their share} of phoneme i, for every token row of every segment;
//             its frames come from cum, the length regulator's scan, clipped to the capacity (contour_extent)
// slab and rows: 8-byte aligned.  No atomics, nothing to zero: phonemes reads only what frames has stored in the same run.
hipError_t launch_pitch_frames(hipStream_t s, const float *wav, void *slab, PitchFrameRow *rows, const uint32_t *par, const Segs &frames, int hop,
                               int sr);
hipError_t launch_pitch_phonemes(hipStream_t s, const int32_t *cum, const void *slab, PitchPhonemeRow *rows, const Segs &tokens, const Segs &frames);

// ---- band levels (include/zerovox_amd.h "band levels", bands.h): two passes behind the pitch track's, over the waveform the caller
// receives.  `frames` is the CAPACITY table or inline segment, `tokens` the token table; both passes index by ABSOLUTE row, and every
// row of rows and slab has BANDS_ROW_STRIDE entries of which the segment's first n_bands are written.
//   frames:   slab[(frames[u].row0 + f) * BANDS_ROW_STRIDE + b] = the kept power Eq of band b of frame f (u64), for every frame of every
//             segment's capacity, and, where rows is not null, rows[...same index] = the band's level.  table: the twiddle table in
//             fragment order (bands_table_fragments, BANDS_TABLE_BYTES, 16-byte aligned).  par [segments][BANDS_PARAM_STRIDE]: each
//             segment's resolved row (bands_resolve), read at run time; n_bands == 0 there: the segment is skipped by both passes.  A
//             span never leaves its segment's own samples [row0 * hop, (row0 + rows) * hop).  The pass reads aligned 8-byte loads:
//             wav 16-byte aligned and, as for the contour, a hop that is a multiple of 4 (contour_hop_supported), else it is refused.
//   phonemes: rows[(tokens[u].row0 + i) * BANDS_ROW_STRIDE + b] = band b's level over phoneme i, for every token row of every segment;
//             its frames come from cum, the length regulator's scan, clipped to the capacity (contour_extent)
// slab: 8-byte aligned.  No HBM atomics, nothing to zero: phonemes reads only what frames has stored in the same run.
hipError_t launch_bands_frames(hipStream_t s, const float *wav, const void *table, void *slab, float *rows, const uint32_t *par, const Segs &frames,
                               int hop);
hipError_t launch_bands_phonemes(hipStream_t s, const int32_t *cum, const void *slab, float *rows, const uint32_t *par, const Segs &tokens,
                                 const Segs &frames);

// ---- waveform filter (include/zerovox_amd.h "waveform filter", filter.h): one pass behind the output conv and ahead of the envelope,
// from `in` to `out` (never in place; both indexed like the waveform, by ABSOLUTE frame row times hop).  `frames` is the CAPACITY table
// or inline segment, `live` the table of the frames the vocoder ran over (the capacity again where the call is not fitted).  par
// [segments][FILTER_PARAM_STRIDE]: each segment's row (filter_pack), read at run time.  Per segment, with S = min(live rows, capacity
// rows) * hop: n_taps == 0 copies the capacity bit for bit; else out[0 .. S) is the rule over in[0 .. S) and out[S .. capacity) is
// +0.0.  Nothing outside the segment's own span [row0 * hop, row0 * hop + S) is read.
hipError_t launch_filter(hipStream_t s, const float *in, float *out, const uint32_t *par, const Segs &frames, const Segs &live, int hop);

// ---- mel analysis (include/zerovox_amd.h "mel analysis", mel.h): two passes over a waveform laid out like the vocoder's output, by
// ABSOLUTE frame row times hop.  `frames` is the table of the utterances' frames or the inline segment; par the call's ONE parameter
// block (mel_resolve, mel_par_words(num_mels) words), read at run time; the grids: stage_plan.h mel_plan.
//   frames: slab[(frames[u].row0 + f) * MEL_SLAB_STRIDE + k] = the magnitude of bin k of frame f (f64), for every frame of every segment.
//           table: both digit planes in fragment order (mel_table_fragments, MEL_TABLE_BYTES, 16-byte aligned).  A span never leaves
//           its segment's own samples [row0 * hop, (row0 + rows) * hop): what lies outside is zero or the segment's own reflection.
//   rows:   rows[(frames[u].row0 + f) * num_mels + c] = channel c of frame f, from the slab the frames pass stored in the same run.
// The hop is a multiple of 4, as for the band levels, else both are refused.  No atomics, nothing to zero.
hipError_t launch_mel_frames(hipStream_t s, const float *wav, const void *table, double *slab, const uint32_t *par, const Segs &frames, int hop,
                             int num_mels);
hipError_t launch_mel_rows(hipStream_t s, const double *slab, float *rows, const uint32_t *par, const Segs &frames, int hop, int num_mels);

// ---- mel alignment (include/zerovox_amd.h "mel alignment", align.h): five passes over ONE launch group of pairs, a launch each whatever
// the group (align.h align_plan).  pairs[n_pairs] says where a pair's rows, cells and map entries lie (AlignPair); x holds the group's
// f32 rows [row][M], sequence after sequence.
//   means: means[(2 pair + side) * ALIGN_MAX_MELS + c] = the rounded mean of channel c of the sequence's quantised rows, or 0 without normalise
//   quant: the two digit planes [row][align_k(M)] of q' (16-byte aligned, zeros behind channel M) and norms[row] = the sum of q'^2
//   cost:  cost[cell0 + i * Tb + j] = norms[a i] + norms[b j] - 2 dot, the dot product in three digit-plane sums on the i8 matrix cores
//   dp:    choice[cell0 + i * Tb + j] = the predecessor taken (0, 1, 2; ALIGN_NONE at the first cell), totals[pair] = D of the last cell
//   walk:  rows[pair] = total, distance and path length, maps[map0 ..] = [map_a (Ta) | map_b (Tb)]
// No atomics, nothing to zero: every entry a pass reads was stored by the passes before it in the same run.
struct AlignJob
{
    const float *x;
    int32_t *means;
    int8_t *hi_plane, *lo_plane;
    int32_t *norms;
    uint32_t *cost;
    uint8_t *choice;
    int64_t *totals;
    AlignRow *rows;
    int32_t *maps;
    const AlignPair *pairs;
    int n_pairs, max_ta, max_tb, M;
    float scale;            // resolved: finite and positive
    uint32_t normalise;
};
hipError_t launch_align_means(hipStream_t s, const AlignJob &j);
hipError_t launch_align_quant(hipStream_t s, const AlignJob &j);
hipError_t launch_align_cost(hipStream_t s, const AlignJob &j);
hipError_t launch_align_dp(hipStream_t s, const AlignJob &j);
hipError_t launch_align_walk(hipStream_t s, const AlignJob &j);

// ---- loudness (include/zerovox_amd.h "loudness", loudness.h): six passes over ONE launch group of utterances (LoudJob), a launch each
// whatever the group (stage_plan.h loud_plan).  segs[nseg] says where an utterance's samples, chunks, steps and tiles lie (LoudSeg); every
// utterance's samples start at a multiple of LOUD_CHUNK floats behind the 16-byte aligned wav and own whole chunks up to its capacity.
//   chunks (phase_c false): state[chunk] = the end state of the chunk run from zero;  states: state[chunk] = its entry state, in place
//   chunks (phase_c true):  runs[chunk] = the chunk's two run sums;  peak: peaks[tile] = the tile's true-peak and sample-peak bits
//   gate:  rows[u] = the result (LoudRow), the gain included;  apply: wav scaled by rows[u].gain over the capacity, in place
// No atomics, nothing to zero.  A group without a measured sample (max_N == 0) launches gate and apply alone.
hipError_t launch_loud_chunks(hipStream_t s, const LoudJob &j, bool phase_c);
hipError_t launch_loud_states(hipStream_t s, const LoudJob &j);
hipError_t launch_loud_peak(hipStream_t s, const LoudJob &j);
hipError_t launch_loud_gate(hipStream_t s, const LoudJob &j);
hipError_t launch_loud_apply(hipStream_t s, const LoudJob &j);

// ---- limiter (include/zerovox_amd.h "limiter", limiter.h): five passes over ONE launch group of utterances (LimitJob), a launch each
// whatever the group (stage_plan.h limit_plan).  segs[nseg] says where an utterance's samples, q, m, peak tiles and statistics lie
// (LimitSeg); wav, out, q and m are 16-byte aligned, every utterance's q region holds whole tiles of LIMIT_TILE entries.
//   peak (before): q per sample and peaks_before per tile from wav;  min: m from q;  mean: out and stats from m and wav;
//   peak (after): peaks_after per tile from out;  reduce: rows[u] = the result (LimitRow)
// hipErrorInvalidValue: a null or misaligned pointer, or a group limit_plan does not accept.
hipError_t launch_limit_peak(hipStream_t s, const LimitJob &j, bool after);
hipError_t launch_limit_min(hipStream_t s, const LimitJob &j);
hipError_t launch_limit_mean(hipStream_t s, const LimitJob &j);
hipError_t launch_limit_reduce(hipStream_t s, const LimitJob &j);

// ---- resampling (include/zerovox_amd.h "resampling", resample.h): two passes over ONE launch group of utterances (ResampleJob), a launch
// each whatever the group (stage_plan.h resample_plan).  segs[nseg] says where an utterance's input, output and statistics lie
// (ResampleSeg); wav, out and pcm are 16-byte aligned, the table 8-byte; out or pcm may be null, not both.
//   resample: out and pcm per output and a (peak, clips) pair per tile from wav and the table;  reduce: rows[u] = the result (ResampleRow)
// hipErrorInvalidValue: a null or misaligned pointer, or a group resample_plan does not accept.
hipError_t launch_resample(hipStream_t s, const ResampleJob &j);
hipError_t launch_resample_reduce(hipStream_t s, const ResampleJob &j);

}  // namespace zv
