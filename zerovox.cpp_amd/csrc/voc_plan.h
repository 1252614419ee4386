// voc_plan.h — which kernel forms a vocoder call runs (DESIGN.md "Switches"): the decisions of Model::vocode_group as pure host code.
// Plain integers and booleans in, booleans out; every switch is read here, through knob(), when the call is planned, so a switch set
// on a live model holds from the next call on (captured graphs are keyed on knob_epoch()).  Shared by the schedule (vocoder.cpp,
// decoder.cpp, capi.cpp) and the host-side test (tests/native/voc_plan_check.cpp): nothing here needs HIP, a Model or a device
// pointer.  What each launcher then does is planned in conv_plan.h, which also says what the fused ResBlock kernels take.
#pragma once

#include <stddef.h>

#include "conv_plan.h"      // batch_switch / batch_rows, pair_supported / triple_supported / block64_supported, TRIPLE_MAX_DIL
#include "knobs.h"

namespace zv
{

// ---- a checkpoint's geometry, filled once by the loader ----
constexpr int VOC_MAX_STAGES = 8, VOC_MAX_DIL = 8, VOC_BRANCHES = 3;
struct VocPairGeom
{
    int  k1, k2;                // taps of the dilated conv and of the plain conv
    bool fused, ring, x16;      // packed weight forms that exist: fused (32 x 32 x 16 fragments), LDS-ring stream, 16 x 16 x 32 fragments
};
struct VocStageGeom
{
    int         scale;          // rows out per row in
    int         Cp;             // padded channels of the residual blocks
    bool        up_gemm;        // the upsample conv has its conv_gemm_kernel pack
    int         up_Cin_p;       // its padded input channels
    VocPairGeom pair[VOC_BRANCHES][VOC_MAX_DIL];
};
struct VocGeom
{
    int          n_up, n_dil;
    int          dil[VOC_MAX_DIL];
    int          in_Cout_p;     // padded output channels of the input conv
    VocStageGeom st[VOC_MAX_STAGES];
};

// ---- one call's numbers ----
// A tail group (Model::vocode_tail) is planned from its own sub-batch: nseg counts the group's segments, t_rows stays the whole
// batch's capacity.
struct VocCall
{
    int    nseg, t_max;         // Batch::nseg, Batch::t_max
    size_t t_rows;              // Batch::t_rows
    int    n_cu;
    bool   fitted;              // Batch::d_frm_live
    bool   runs_off;            // Model::voc_runs_off
    bool   dbg_active;          // a debug layer of any kind is tapped
    int    dbg_stage;           // the stage whose residual blocks a ZV_LAYER_VOC_RESBLOCK tap sits in, or -1
};

enum VocMerge { VOC_MERGE_NONE, VOC_MERGE_ONE, VOC_MERGE_SEQ };       // the stage's MRF sum: three outputs / one launch / three summing launches
struct VocStagePlan
{
    bool     up_pass;           // the upsample conv's operand as an f16 pass of its own, the conv on conv_gemm_kernel
    bool     all_fusable, enough_rows, fused;
    bool     whole_block;       // all dilations of the three branches in one launch (launch_triple)
    bool     block64[VOC_BRANCHES];       // the branch's first two dilation pairs in one launch (launch_block64)
    VocMerge merge;             // of the last dilation pair
};
struct VocPlan
{
    bool         runs;          // run-shortened schedule
    bool         c0_f16;        // the input conv writes the first upsample conv's f16 operand
    VocStagePlan st[VOC_MAX_STAGES];
};

// batches (ZV_VOC_RUNS = 1): by capacity — a single short utterance has no rounds of workgroups to give back, and its three extra
// launches would only add latency (small batches and long single utterances may be giving a gain away: see BATCH_ROWS)
inline bool voc_runs(const VocCall &c)
{
    return !c.runs_off && !c.fitted && !c.dbg_active && batch_switch(knob(ZV_VOC_RUNS), batch_rows((long)c.t_rows));
}

// batches, wide upsample convs on conv_gemm_kernel over an f16 operand tensor (ZV_UP_GEMM; ZV_CONV_GEMM = 0 takes the kernel away)
inline bool voc_up_gemm(const VocStageGeom &s, size_t rows_in)
{
    return s.up_gemm && knob(ZV_CONV_GEMM) != 0 && batch_switch(knob(ZV_UP_GEMM), batch_rows((long)rows_in));
}

inline VocStagePlan voc_plan_stage(const VocGeom &g, int i, const VocCall &c, bool c0_f16)
{
    const VocStageGeom &s = g.st[i];
    VocStagePlan p{};
    int rate = 1;
    for (int q = 0; q < i; q++) rate *= g.st[q].scale;
    const size_t L = c.t_rows * rate, Lo = L * s.scale;       // capacity rows in and out
    rate *= s.scale;
    const int  Cp = s.Cp;
    const long Lbatch = (long)c.t_max * rate * c.nseg;        // rows the launches of this stage cover
    // the first stage reads the input conv's f16 output where there is one; else a pass pays while the operand (f16, Cin_p wide) is
    // no more bytes than the conv's f32 output
    p.up_pass = !(i == 0 && c0_f16) && voc_up_gemm(s, L) && (size_t)s.up_Cin_p * 2 * L <= Lo * Cp * 4;

    // every pair of the stage must have fused weights (one K for both convs, pair_supported): a stage runs fused or not as a
    // whole, so the MRF sum keeps one association whichever kernels a checkpoint's tap counts allow
    p.all_fusable = true;
    for (int jb = 0; jb < VOC_BRANCHES; jb++)
        for (int d = 0; d < g.n_dil; d++) p.all_fusable = p.all_fusable && s.pair[jb][d].fused;
    // 256-channel stage: the fused kernel needs all 256 xt channels in one workgroup, which leaves few workgroups per
    // branch for a short utterance — two unfused launches (480 workgroups at 512 frames) win below about a round
    // of fused ones (round 4, on the 16 x 16 x 32 kernel, whole vocoder under graph replay: 128 frames 0.276 unfused /
    // 0.291 fused ms, 256: 0.320 / 0.333, 512: 0.470 / 0.465, 1 024: 0.852 / 0.814)
    p.enough_rows = Cp != 256 || knob(ZV_FUSE256) != 0 || (Lbatch / 54) * 3 >= (long)c.n_cu;
    p.fused = knob(ZV_NO_FUSE) == 0 && p.all_fusable && p.enough_rows;

    // narrow stages: the whole residual block; one K per job (TripleJob::K), so every dilation pair of a branch must have it
    p.whole_block = p.fused && knob(ZV_NO_TRIPLE) == 0 && g.n_dil <= TRIPLE_MAX_DIL;
    for (int jb = 0; jb < VOC_BRANCHES && p.whole_block; jb++)
    {
        const int K = s.pair[jb][0].k1;
        p.whole_block = triple_supported(Cp, K, g.dil, g.n_dil);
        for (int d = 0; d < g.n_dil && p.whole_block; d++) p.whole_block = s.pair[jb][d].fused && s.pair[jb][d].k1 == K && s.pair[jb][d].k2 == K;
    }

    // 64 channels, batches: the first two dilation pairs of the branches with few taps in one launch (the branch's tensor crosses
    // HBM once instead of twice; ZV_BLOCK64 = most taps it takes, 0 = never; negative: at any length)
    const int k64 = knob(ZV_BLOCK64), kmax64 = k64 < 0 ? -k64 : k64;
    if (p.fused && !p.whole_block && Cp == 64 && g.n_dil == 3 && kmax64 >= 3 && (k64 < 0 || Lbatch / 244 >= 4L * c.n_cu))
        for (int jb = 0; jb < VOC_BRANCHES; jb++)
        {
            const VocPairGeom *rp = s.pair[jb];
            const bool one_k = rp[1].k1 == rp[0].k1 && rp[0].k2 == rp[0].k1 && rp[1].k2 == rp[0].k1;       // TripleJob::K
            p.block64[jb] = one_k && rp[0].k1 <= kmax64 && rp[0].ring && rp[1].ring && block64_supported(Cp, rp[0].k1, g.dil, 2);
        }

    // the last pair of the stage: the three branches' outputs are only ever used summed (MRF), so the workgroups run all three
    // branches of a tile and store the sum alone
    // ... once the merged launch (a third of the workgroups, each three times as long) still has rounds of workgroups to
    // spare: at one round (a single 512-frame utterance) the merged 128- / 64-channel launches took 45.7 / 37.3 us against
    // 28.4 / 32.8 us for the three branches side by side, more than the upsample conv gains from reading one tensor
    const int  merge_tile = Cp >= 256 ? 54 : (Cp == 128 ? 118 : 246);
    const bool merge_pays = knob(ZV_MERGE_ALWAYS) != 0 || (Lbatch / merge_tile >= 4L * c.n_cu && Cp <= knob(ZV_MERGE_MAXC));
    const bool merge = p.fused && !p.whole_block && knob(ZV_NO_MERGE) == 0 && c.dbg_stage != i && merge_pays;
    // 256 channels: the branches one launch each on the side-by-side kernel (96-row tiles, all staging loads in flight:
    // 1 020 us for the three against 1 105 us for the three-branches-per-workgroup form; at 128 channels the single-
    // branch launches' tails cost more than they gain: 1 422 against 1 386 us), every launch adding its term into the
    // running sum — (y0 + y1) + y2, the merged form's association, hence its bits
    p.merge = !merge ? VOC_MERGE_NONE : (Cp >= 256 && knob(ZV_MERGE_SEQ) != 0 ? VOC_MERGE_SEQ : VOC_MERGE_ONE);
    return p;
}

inline VocPlan voc_plan(const VocGeom &g, const VocCall &c)
{
    VocPlan p{};
    p.runs = voc_runs(c);
    // batches: the first upsample conv's operand f16(lrelu(c0, 0.1)) straight from the input conv, its only reader
    p.c0_f16 = !c.dbg_active && g.n_up > 0 && voc_up_gemm(g.st[0], c.t_rows) && g.st[0].up_Cin_p == g.in_Cout_p;
    for (int i = 0; i < g.n_up; i++) p.st[i] = voc_plan_stage(g, i, c, p.c0_f16);
    return p;
}

// Utterance groups of a large batch's last vocoder stage (ZV_TAIL_GROUPS = sw; capi.cpp): as many as the switch asks for, of at
// least two utterances each — a group of one utterance leaves the whole-block kernel two rounds of workgroups (measured 21.4 / 21.1 /
// 21.1 / 22.7 ms per batch with 4 / 8 / 16 / 32 groups of 32 utterances).  A profile and a debug tap want one schedule.
constexpr size_t TAIL_GROUPS_MIN_BYTES = (size_t)16 << 20;
inline int voc_tail_groups(int sw, int nseg, size_t wav_bytes, bool profiling, bool dbg_active)
{
    if (sw <= 1 || nseg < 4 || wav_bytes < TAIL_GROUPS_MIN_BYTES || profiling || dbg_active) return 1;
    return sw < nseg / 2 ? sw : nseg / 2;
}
// the call's own: the switch read here, when the call is planned
inline int voc_tail_groups(int nseg, size_t wav_bytes, bool profiling, bool dbg_active)
{
    return voc_tail_groups(knob(ZV_TAIL_GROUPS), nseg, wav_bytes, profiling, dbg_active);
}

}  // namespace zv
