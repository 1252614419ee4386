// stage_plan.h — what the encoder-side launchers then do and which regime the encoder and decoder schedules run in (DESIGN.md
// "Switches", "Launch plans"), as pure host code.  Plain integers and booleans in, a small struct out; every non-diagnostic switch
// concerned is read here, through knob(), when the call is planned.  The launchers of encoder_kernels.hip and regulator_kernels.hip
// validate their arguments, call their plan and launch what it says; encoder.cpp, decoder.cpp and capi.cpp ask enc_plan / dec_plan.
// With voc_plan.h (the vocoder's regime) and conv_plan.h (the conv and ResBlock launchers) this is every kernel-form decision of the
// library; tests/native/stage_plan_check.cpp pins every threshold on the host: nothing here needs HIP, a Model or a device pointer.
#pragma once

#include <stddef.h>

#include "conv_plan.h"      // batch_switch / batch_rows, plan_round_up
#include "knobs.h"
#include "mel.h"            // MEL_TILE_FRAMES, MEL_ROWS_FRAMES, MEL_MAX_MELS
#include "loudness.h"       // LOUD_CHUNK, LOUD_WG_CHUNKS, LOUD_TP_TILE
#include "limiter.h"        // LIMIT_TILE, LIMIT_MAX_HALO
#include "resample.h"       // resample_tile, resample_check_shape

namespace zv
{

// ---- attention (encoder_kernels.hip) ----
constexpr int    ATT_NS_MAX = 144;                      // k pairs of a query fragment a lane keeps in registers: dk <= 288
constexpr size_t ATT_LDS_MAX = 160 * 1024 - 4096;       // attention_mfma_kernel's dynamic LDS (it has 3 KB of static LDS besides)
constexpr long   ATT_MIN_WGS = 48;                      // fewer 64-query workgroups do not fill the chip; (queries x heads) blocks do
constexpr size_t ATT_LDS_NO_ATTR = 48 * 1024;           // dynamic LDS a launch may have without the function attribute
constexpr size_t ATT_SCALAR_LDS_MAX = 60 * 1024;        // the scalar form's query row and score row
enum AttForm { ATT_INVALID, ATT_MFMA, ATT_SCALAR };
struct AttPlan
{
    AttForm form;
    int     gx, gy, gz;         // grid: (64-query tiles | queries, heads, segments)
    size_t  lds;                // dynamic LDS bytes
    bool    raise_lds;          // hipFuncAttributeMaxDynamicSharedMemorySize must be set to lds first
};
// matrix cores: K rows at an odd stride of dk | 1 floats for 64 keys, one pad float, then 64 scores per key of the longest utterance
// rounded up to a 32-key tile — where the head dim is a multiple of 4 the fragment registers hold, the rows load as float4 and the
// workgroups are enough.  ZV_ATT_SCALAR / ZV_ATT_MFMA: test hooks (the latter lifts the workgroup count alone).
inline AttPlan att_plan(int n_max, int H, int dk, int ld, int nseg)
{
    const size_t lds_mfma = ((size_t)64 * (dk | 1) + 1 + (size_t)plan_round_up(n_max, 32) * 64) * sizeof(float);
    const long   wgs_mfma = (long)((n_max + 63) / 64) * H * nseg;
    if (knob(ZV_ATT_SCALAR) == 0 && (dk & 3) == 0 && dk <= 2 * ATT_NS_MAX && (ld & 3) == 0 && lds_mfma <= ATT_LDS_MAX &&
        (wgs_mfma >= ATT_MIN_WGS || knob(ZV_ATT_MFMA) != 0))
        return AttPlan{ATT_MFMA, (n_max + 63) / 64, H, nseg, lds_mfma, lds_mfma > ATT_LDS_NO_ATTR};
    const size_t lds = (size_t)(dk + n_max) * sizeof(float);
    return AttPlan{lds > ATT_SCALAR_LDS_MAX ? ATT_INVALID : ATT_SCALAR, n_max, H, nseg, lds, false};
}

// ---- f32 linear layers (encoder_kernels.hip) ----
// 64-row workgroups (a W operand feeds two MFMAs) once they fill the chip, 32-row ones for short inputs; the shape never changes a
// bit: every output element is one k-ordered chain
constexpr long LINEAR_WG64_MIN = 256;
struct LinearPlan
{
    int rows;                   // rows of a workgroup: 64 or 32 (linear_mfma_kernel<rows / 32>)
    int tps;                    // row tiles per segment
    int gx, gy;                 // grid: (groups of 128 outputs, tiles of all segments)
};
inline LinearPlan linear_plan(int max_rows, int nseg, int out)
{
    const int  gx = (out + 127) / 128;
    const long wg64 = (long)((max_rows + 63) / 64) * nseg * gx;
    const int  rows = wg64 >= LINEAR_WG64_MIN ? 64 : 32, tps = (max_rows + rows - 1) / rows;
    return LinearPlan{rows, tps, gx, tps * nseg};
}

// ---- length regulator (regulator_kernels.hip) ----
constexpr int    LR_FUSED_TOKENS = 1024;                // lr_fused16_kernel keeps a segment's scan in LDS: 4 tokens x 256 threads
constexpr size_t LR_GATHER16_LDS_MAX = 48 * 1024;       // lr_gather16_kernel's copy of the scan, 4 bytes per token: 12 288 tokens
enum LrForm { LR_FUSED, LR_SCAN_GATHER16, LR_SCAN_GATHER };
struct LrPlan
{
    LrForm form;
    int    scan_gx;             // lr_scan_kernel's grid (one workgroup per segment); 0: the fused form scans by itself
    int    gx, gy;              // grid of the fused or gathering kernel: (16-frame tiles | frames, segments)
    size_t lds;                 // the gathering kernel's dynamic LDS bytes
};
// Rows that move as float4 (C, ld, ldh multiples of 4) take the 16-frame forms: scan and gather in one launch while the longest
// utterance's scan fits, else a scan launch and the gather that reads the scan from LDS.  LR_SCAN_GATHER, the frame-per-workgroup
// gather, is what is left: a width that is no multiple of 4 (which no loadable checkpoint has — the loader requires E % 16 == 0 — so
// only a direct call of the launcher reaches it) or more tokens than the LDS copy holds.
inline LrPlan lr_plan(int C, int ld, int ldh, int tokens_max, int frames_max, int nseg)
{
    const bool vec4 = (C & 3) == 0 && (ld & 3) == 0 && (ldh & 3) == 0;
    const int  g16 = (frames_max + 15) / 16;
    if (vec4 && tokens_max >= 1 && tokens_max <= LR_FUSED_TOKENS && frames_max >= 1) return LrPlan{LR_FUSED, 0, g16, nseg, 0};
    if (vec4 && tokens_max >= 1 && (size_t)tokens_max * 4 <= LR_GATHER16_LDS_MAX)
        return LrPlan{LR_SCAN_GATHER16, nseg, g16, nseg, (size_t)tokens_max * 4};
    return LrPlan{LR_SCAN_GATHER, nseg, frames_max, nseg, 0};
}

// ---- LayerNorm launches that carry tail work (encoder_kernels.hip: launch_layernorm_tail) ----
constexpr int LN_TAIL_MAX = 64 * 12;                    // the tail exists in the rows-in-registers form only: 12 channels per lane
inline bool layernorm_tail_ok(int C) { return C <= LN_TAIL_MAX; }

// ---- mel analysis (mel_kernels.hip): ONE launch per kernel over the segment table, whatever the batch ----
struct MelPlan
{
    bool ok;                    // the hop is a multiple of 4 (as for the band levels), 1 <= num_mels <= MEL_MAX_MELS, a frame exists
    int  frames_gx, rows_gx;    // mel_frames_kernel: tiles of MEL_TILE_FRAMES frames; mel_rows_kernel: groups of MEL_ROWS_FRAMES frames
    int  gy;                    // segments, of both grids
};
inline MelPlan mel_plan(int max_rows, int nseg, int hop, int num_mels)
{
    const bool ok = max_rows >= 1 && nseg >= 1 && hop >= 4 && (hop & 3) == 0 && num_mels >= 1 && num_mels <= (int)MEL_MAX_MELS;
    return MelPlan{ok, (max_rows + MEL_TILE_FRAMES - 1) / MEL_TILE_FRAMES, (max_rows + MEL_ROWS_FRAMES - 1) / MEL_ROWS_FRAMES, nseg};
}

// ---- the encoder's schedule (encoder.cpp) ----
struct EncPlan
{
    bool merged;                // the per-token layers (linear, 1-tap conv, plain LayerNorm) see one dense segment (ZV_LINEAR_MERGED)
    bool tails;                 // the style add, the predictors' linear layer and the bucket + embedding step ride on LayerNorm launches
};
// tails: 6 launches fewer per call, same operations in the same order (ZV_LN_TAIL = 0: separate launches); a debug tap wants the
// separate launches' tensors.  E: the encoder's width, V: the variance predictors'.
inline EncPlan enc_plan(int E, int V, bool dbg_active)
{
    return EncPlan{knob(ZV_LINEAR_MERGED) != 0, !dbg_active && knob(ZV_LN_TAIL) != 0 && layernorm_tail_ok(E) && layernorm_tail_ok(V)};
}

// ---- the decoder's schedule (decoder.cpp; capi.cpp gives a chain its run table where `runs` says so) ----
constexpr long DEC_PREPASS_ROWS = 256;
struct DecPlan
{
    bool prepass;               // the convs read an f16 operand written by a pass of its own
    bool runs;                  // run-shortened decoding: a chain over this batch gets a run table (Batch::d_dec_runs)
    bool pack;                  // densely packed decoding (dec_runs.h) of the run table the batch carries
};
// prepass.  Two ways to feed a conv its normalised operand, same bits (tests): (a) the conv normalises while it stages its input tile
// (PRO_NORM_ACT) — no extra launch, right for a very short utterance where every launch is latency; (b) one pass writes the f16
// operand (launch_norm_act_f16) and the conv copies it (PRO_RAW_F16) — right when launches have many rounds of workgroups: a
// 1 056-wide conv stages every input tile 9 times (once per group of 128 output channels), so (a) repeats the f32 prologue 9 times
// and reads twice the bytes.  (Round 4: with the single-utterance conv form's loader waves the pass pays from 256 frames on — it takes
// the statistics launch's place and leaves the loaders a plain copy: one utterance of 128 / 256 / 512 / 1 024 frames 1.32 / 1.345 /
// 1.62 / 2.16 ms fused, 1.33 / 1.33 / 1.58 / 2.07 ms with the pass.)  ZV_DEC_PREPASS >= 0: test / A-B hook.
// runs.  Batches (ZV_DEC_RUNS = 1): by capacity, with the threshold of ZV_VOC_RUNS and the other batch switches, so that a single
// utterance keeps its schedule; no sweep of capacities below it is on record.  Off in fitted mode, under a debug tap and
// where the pre-pass is off.
// pack.  Wherever a batch has a run table (has_table: the tap entry points and a stand-alone decode pass none even where `runs`
// holds).  One utterance has nothing to pack: its rows are tiled as they are either way, and the pass that packs would be one launch
// more.
inline DecPlan dec_plan(int nseg, int t_max, size_t t_rows, bool fitted, bool dbg_active, bool has_table)
{
    DecPlan    p{};
    const int pre_env = knob(ZV_DEC_PREPASS);
    p.prepass = pre_env >= 0 ? pre_env != 0 : (long)t_max * nseg >= DEC_PREPASS_ROWS;
    p.runs = !fitted && !dbg_active && p.prepass && batch_switch(knob(ZV_DEC_RUNS), batch_rows((long)t_rows));
    p.pack = has_table && nseg > 1 && knob(ZV_DEC_PACK) != 0;
    return p;
}

// ---- loudness (loudness_kernels.hip): ONE launch per kernel over a launch group's utterances ----
constexpr int LOUD_APPLY_TILE = 4096;                    // samples one workgroup of the apply pass scales: 256 lanes, four float4 each
struct LoudPlan
{
    bool ok;                    // a sample is measured, the step holds a chunk (a chunk meets at most two steps)
    int  chunks, chunk_gx;      // chunks of the longest span; phases A and C: workgroups of LOUD_WG_CHUNKS chunks, a lane each
    int  tp_gx;                 // the true-peak pass: tiles of LOUD_TP_TILE outputs over the span and the interpolator's tail
    int  steps;                 // whole 100 ms steps of the longest span
    int  apply_gx;              // the apply pass: tiles of LOUD_APPLY_TILE samples of the longest capacity
    int  states_gx, gy;         // phase B: a lane per utterance, 64 to a workgroup; utterances: grid y of A, C, true peak and apply, grid x of the gate
};
inline LoudPlan loud_plan(int64_t max_N, int64_t max_total, int nseg, uint32_t step)
{
    const bool ok = max_total >= 1 && max_N >= 0 && max_N <= max_total && nseg >= 1 && step >= (uint32_t)LOUD_CHUNK;
    return LoudPlan{ok, (int)loud_chunks(max_N), (int)((loud_chunks(max_N) + LOUD_WG_CHUNKS - 1) / LOUD_WG_CHUNKS), (int)loud_tp_tiles(max_N),
                    (int)(max_N / (step ? step : 1u)), (int)((max_total + LOUD_APPLY_TILE - 1) / LOUD_APPLY_TILE), (nseg + 63) / 64, nseg};
}

// ---- limiter (limiter_kernels.hip): ONE launch per kernel over a launch group's utterances ----
// A workgroup of the minimum and mean passes stages its LIMIT_TILE outputs' windows, LIMIT_TILE + halo entries: the minimum pass as u32
// (the entries, over which the prefix minima are written) with LIMIT_TILE suffix minima behind them, the mean pass as 48-bit prefix sums
// (a u32 and a u16 array) with a zero in front.  At the largest halo that is 48 KB and 60 KB: three and two workgroups fit a CU's
// 160 KB.  LIMIT_LDS_TAIL bytes behind them hold the waves' partial results.
constexpr int LIMIT_LDS_TAIL = 64;
struct LimitPlan
{
    bool   ok;
    int    peak_gx;             // the peak passes: tiles of LIMIT_TILE entries of the longest q
    int    min_gx;              // the minimum pass: tiles of the longest m (at most the longest capacity + the largest halo)
    int    mean_gx;             // the mean pass: tiles of the longest capacity
    int    gy;                  // utterances: grid y of those passes, grid x of the reduction
    int    stage;               // entries a workgroup stages, rounded up to 4
    size_t min_lds, mean_lds;   // dynamic LDS of the two passes, in bytes
};
inline LimitPlan limit_plan(int64_t max_qlen, int64_t max_total, int max_halo, int nseg)
{
    const bool ok = max_total >= 1 && max_halo >= 2 && max_halo <= LIMIT_MAX_HALO && max_qlen >= limit_qlen(max_total, 2) && max_qlen <= limit_qlen(max_total, max_halo) &&
                    nseg >= 1 && nseg <= 65535;
    const int stage = limit_stage(max_halo);
    return LimitPlan{ok, (int)limit_tiles(max_qlen), (int)limit_tiles(max_total + max_halo), (int)limit_tiles(max_total), nseg, stage,
                     (size_t)(stage + LIMIT_TILE) * 4 + LIMIT_LDS_TAIL, (size_t)(stage + 4) * 6 + LIMIT_LDS_TAIL};
}

// ---- resampling (resample_kernels.hip): ONE launch per kernel over a launch group's utterances ----
// A workgroup covers one tile of resample_tile(L, M, P): R * S outputs, their input samples staged as f64 (RESAMPLE_STAGE at the most,
// 64 000 bytes: two workgroups fit a CU's 160 KB); the reduction is a wave per utterance.
struct ResamplePlan
{
    bool ok;
    int  gx;        // tiles of the longest output
    int  gy;        // utterances: grid y of the pass, grid x of the reduction
    ResampleTile tile;
};
inline ResamplePlan resample_plan(int64_t max_n_out, int nseg, uint32_t L, uint32_t M, uint32_t P)
{
    if (max_n_out < 1 || nseg < 1 || nseg > 65535 || resample_check_shape(L, M, P)) return ResamplePlan{false, 0, 0, ResampleTile{0, 0, 0}};
    const ResampleTile t = resample_tile(L, M, P);
    const int64_t gx = resample_tiles(max_n_out, resample_tile_outputs(t));
    return ResamplePlan{gx <= 0x7fffffff && resample_tile_stage(L, M, P, t.S, t.R) <= RESAMPLE_STAGE, (int)gx, nseg, t};
}

}  // namespace zv
