// Host-side driver of csrc/voc_plan.h for tests/test_voc_plan_cpu.py (no GPU, no HIP; linked with csrc/knobs.cpp).
//   voc_plan_check cases
//       the table below: every expectation was derived by hand from the schedule as it stood before the header existed (inline in
//       Model::vocode_group, vocoder.cpp of commit 7a64b33: the line numbers quoted are that file's, unless another is named).
//       Prints "ok <cases>".
//   voc_plan_check regime NAME [ZV_X=V ...]
//       one utterance of 16 frames on the medium geometry under these switches against REGIMES[NAME]; prints "ok".
//   voc_plan_check plan GEOM NSEG T_MAX T_ROWS [ZV_X=V ...]
//       prints the plan (a test that needs a shape on either side of a threshold can ask).
//
// A plan as text: "r<runs> h<input conv writes the f16 operand>" and per stage five fields,
//     p / -    the upsample conv behind an operand pass
//     W F N    whole-block launch / fused pair launches / two launches per pair
//     3 x 0/1  the branches whose first two pairs resblock_block64_kernel takes
//     - 1 3    the last pair's MRF sum: three outputs / one launch / three summing launches
// The medium checkpoint: 512 -> 256 / 128 / 64 / 32 channels at 5 / 25 / 100 / 300 rows per frame, branches of 3 / 7 / 11 taps,
// dilations 1 / 3 / 5, 256 CUs.  Its upsample convs are 3 taps deep over 512 / 256 / 128 / 64 channels, so the first two have a
// conv_gemm_kernel pack (model_load.cpp:117: Cin_p >= 128 and K Cin_p >= 768); pair_supported holds for every (width, taps) of it.
#include "voc_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace zv;

// geometries: "medium"; "k5": its 32-channel stage's first branch has 5 taps (pair_supported(32, 5) is false: no fused weights);
// "mixed64": the second branch of its 64-channel stage has 3 taps in its first pair and 5 in the other two;
// "v256", "v496", "v768", "v1024": the small checkpoint with that many vocoder channels (synth.VOC_WIDTH_GEOMETRIES).  What the loader
// derives from the width, restated (model_load.cpp): a stage has (width >> (i + 1)) channels, padded to 16; its upsample conv reads
// (width >> i) channels, padded to 16, and has scale x Cp output channels; the conv has its conv_gemm_kernel pack where Cin_p >= 128,
// Cin_p % 64 == 0, there is a whole group of 8 output tiles and 3 Cin_p >= 768 (load_upsample).  WIDTHS below pins the result by hand.
static int width_of(const std::string &name)
{
    return name == "v256" ? 256 : name == "v496" ? 496 : name == "v768" ? 768 : name == "v1024" ? 1024 : 512;
}
static VocGeom geometry(const std::string &name)
{
    VocGeom g{};
    g.n_up = 4;
    g.n_dil = 3;
    g.dil[0] = 1, g.dil[1] = 3, g.dil[2] = 5;
    const int width = width_of(name);
    g.in_Cout_p = plan_round_up(width, 16);
    const int scales[4] = {5, 5, 4, 3}, taps[3] = {3, 7, 11};
    for (int i = 0; i < 4; i++)
    {
        VocStageGeom &s = g.st[i];
        s.scale = scales[i];
        s.Cp = plan_round_up(width >> (i + 1), 16);
        s.up_Cin_p = plan_round_up(width >> i, 16);
        s.up_gemm = s.up_Cin_p >= 128 && (s.up_Cin_p & 63) == 0 && conv_gemm_groups(s.scale * s.Cp) >= 1 && 3 * s.up_Cin_p >= 768;
        for (int j = 0; j < 3; j++)
            for (int d = 0; d < 3; d++)
            {
                int K = taps[j];
                if (name == "k5" && i == 3 && j == 0) K = 5;
                if (name == "mixed64" && i == 2 && j == 1) K = d == 0 ? 3 : 5;
                const bool f = pair_supported(s.Cp, K);            // the loader packs a pair's weights where this holds (model_load.cpp:259)
                s.pair[j][d] = VocPairGeom{K, K, f, f && s.Cp == 64, f};
            }
    }
    return g;
}

static std::string text(const VocGeom &g, const VocPlan &p)
{
    std::string s = std::string("r") + (p.runs ? "1" : "0") + " h" + (p.c0_f16 ? "1" : "0");
    for (int i = 0; i < g.n_up; i++)
    {
        const VocStagePlan &q = p.st[i];
        s += ' ';
        s += q.up_pass ? 'p' : '-';
        s += q.whole_block ? 'W' : (q.fused ? 'F' : 'N');
        for (int j = 0; j < 3; j++) s += q.block64[j] ? '1' : '0';
        s += q.merge == VOC_MERGE_NONE ? '-' : (q.merge == VOC_MERGE_ONE ? '1' : '3');
    }
    return s;
}

static bool set_switches(const char *list)       // "ZV_X=V ZV_Y=W", after a reset
{
    knob_reset();
    std::string s(list);
    for (size_t a = 0; a < s.size();)
    {
        size_t b = s.find(' ', a);
        if (b == std::string::npos) b = s.size();
        const std::string kv = s.substr(a, b - a);
        const size_t eq = kv.find('=');
        if (eq == std::string::npos || !knob_set(kv.substr(0, eq).c_str(), atoi(kv.c_str() + eq + 1))) return false;
        a = b + 1;
    }
    return true;
}

static VocCall call(int nseg, int t_max, size_t t_rows)
{
    return VocCall{nseg, t_max, t_rows, 256, false, false, false, -1};
}

struct Case
{
    const char *geom, *switches;
    VocCall     c;
    const char *want;
};
#define ONE(T) call(1, T, T)
static const VocCall BENCH = call(32, 1024, 32768), TAIL4 = call(4, 1024, 32768);
static VocCall with(VocCall c, bool fitted, bool runs_off, bool dbg_active, int dbg_stage)
{
    c.fitted = fitted, c.runs_off = runs_off, c.dbg_active = dbg_active, c.dbg_stage = dbg_stage;
    return c;
}

static const Case CASES[] = {
    // :246 enough_rows, 256 channels: (5 T / 54) x 3 >= 256 CUs from 929 frames on; :253-264 the 32-channel stage as whole blocks
    {"medium", "", ONE(16), "r0 h0 -N000- -F000- -F000- -W000-"},
    {"medium", "", ONE(928), "r0 h0 -N000- -F000- -F000- -W000-"},
    {"medium", "", ONE(929), "r0 h0 -F000- -F000- -F000- -W000-"},
    // :302 block64, default ZV_BLOCK64 = 3 (the 3-tap branch alone, :312): 100 T / 244 >= 4 x 256 from 2 499 frames on
    {"medium", "", ONE(2498), "r0 h0 -F000- -F000- -F000- -W000-"},
    {"medium", "", ONE(2499), "r0 h0 -F000- -F000- -F100- -W000-"},
    // :395-396 merged sum at 64 channels (tile 246): 100 T / 246 >= 1 024 from 2 520 on; :404 one launch below 256 channels
    {"medium", "", ONE(2519), "r0 h0 -F000- -F000- -F100- -W000-"},
    {"medium", "", ONE(2520), "r0 h0 -F000- -F000- -F1001 -W000-"},
    // :208 the second upsample conv's operand pass: its 5 T input rows >= 16 384 from 3 277 on (256 x 2 x L <= 5 L x 128 x 4 holds)
    {"medium", "", ONE(3276), "r0 h0 -F000- -F000- -F1001 -W000-"},
    {"medium", "", ONE(3277), "r0 h0 -F000- pF000- -F1001 -W000-"},
    // :395-396 at 128 channels (tile 118): 25 T / 118 >= 1 024 from 4 834 on
    {"medium", "", ONE(4833), "r0 h0 -F000- pF000- -F1001 -W000-"},
    {"medium", "", ONE(4834), "r0 h0 -F000- pF0001 -F1001 -W000-"},
    // :395-396 at 256 channels (tile 54): 5 T / 54 >= 1 024 from 11 060 on; :404 as three summing launches (ZV_MERGE_SEQ = 1)
    {"medium", "", ONE(11059), "r0 h0 -F000- pF0001 -F1001 -W000-"},
    {"medium", "", ONE(11060), "r0 h0 -F0003 pF0001 -F1001 -W000-"},
    {"medium", "ZV_MERGE_SEQ=0", ONE(11060), "r0 h0 -F0001 pF0001 -F1001 -W000-"},
    // :395-396 at 32 channels (tile 246; :253 ZV_NO_TRIPLE takes the whole-block launch away): 300 T / 246 >= 1 024 from 840 on
    {"medium", "ZV_NO_TRIPLE=1", ONE(839), "r0 h0 -N000- -F000- -F000- -F000-"},
    {"medium", "ZV_NO_TRIPLE=1", ONE(840), "r0 h0 -N000- -F000- -F000- -F0001"},
    // :396 ZV_MERGE_MAXC: no wider stage stores the sum
    {"medium", "ZV_MERGE_MAXC=64", ONE(11060), "r0 h0 -F000- pF000- -F1001 -W000-"},
    // :90 run-shortening and :141-142 the input conv's f16 output, both by capacity: 16 384 rows (:203 no pass for stage 0 then)
    {"medium", "", ONE(16383), "r0 h0 -F0003 pF0001 -F1001 -W000-"},
    {"medium", "", ONE(16384), "r1 h1 -F0003 pF0001 -F1001 -W000-"},
    {"medium", "", call(16, 1024, 16384), "r1 h1 -F0003 pF0001 -F1001 -W000-"},
    {"medium", "ZV_VOC_RUNS=0", ONE(16384), "r0 h1 -F0003 pF0001 -F1001 -W000-"},
    {"medium", "ZV_VOC_RUNS=2", ONE(16), "r1 h0 -N000- -F000- -F000- -W000-"},
    // :90 not in fitted mode, not where the caller turns it off, not under a debug tap; :141 a tap also keeps c0 f32, and
    // :208 stage 0 then gets the pass of its own (512 x 2 x L <= 5 L x 256 x 4)
    {"medium", "", with(ONE(16384), true, false, false, -1), "r0 h1 -F0003 pF0001 -F1001 -W000-"},
    {"medium", "", with(ONE(16384), false, true, false, -1), "r0 h1 -F0003 pF0001 -F1001 -W000-"},
    {"medium", "", with(ONE(16384), false, false, true, -1), "r0 h0 pF0003 pF0001 -F1001 -W000-"},
    // :397 !dbg_here: the stage a residual-block tap sits in keeps its three outputs
    {"medium", "", with(ONE(16384), false, false, true, 1), "r0 h0 pF0003 pF000- -F1001 -W000-"},
    // :208 ZV_CONV_GEMM = 0 takes conv_gemm_kernel away from the upsample convs too
    {"medium", "ZV_CONV_GEMM=0", ONE(16384), "r1 h0 -F0003 -F0001 -F1001 -W000-"},
    // the benchmark batch, 32 x 1 024 frames (README.md): run-shortened, the two deep upsample convs on conv_gemm_kernel (the first
    // reads the input conv's f16 output, the second behind a pass), fused pairs with the merged sum, block64 for the 3-tap branch, whole blocks
    {"medium", "", BENCH, "r1 h1 -F0003 pF0001 -F1001 -W000-"},
    // :96-100, :233 a tail group of 4 of its utterances: Lbatch counts 4 segments (5 x 1 024 x 4 / 54 = 379 < 1 024: no merged sum at
    // 256 channels, 25 x 4 096 / 118 = 867: nor at 128), capacities stay the batch's
    {"medium", "", TAIL4, "r1 h1 -F000- pF000- -F1001 -W000-"},
    // :241, :247 a pair without fused weights: the stage runs unfused as a whole
    {"k5", "", ONE(16), "r0 h0 -N000- -F000- -F000- -N000-"},
    {"k5", "", BENCH, "r1 h1 -F0003 pF0001 -F1001 -N000-"},
    // :311-312 one K for the two pairs block64 runs: the branch with 3 and 5 taps is left out, its neighbours are taken —
    // also where its first pair alone would pass the tap limit
    {"mixed64", "ZV_BLOCK64=-11", ONE(16), "r0 h0 -N000- -F000- -F101- -W000-"},
    {"mixed64", "ZV_BLOCK64=-3", ONE(16), "r0 h0 -N000- -F000- -F100- -W000-"},
    {"mixed64", "ZV_BLOCK64=5", BENCH, "r1 h1 -F0003 pF0001 -F1001 -W000-"},
    {"medium", "ZV_BLOCK64=-11", ONE(16), "r0 h0 -N000- -F000- -F111- -W000-"},

    // ---- other vocoder widths (synth.VOC_WIDTH_GEOMETRIES): a kernel goes with a stage's padded channel count, not its position.
    // Per width: one short utterance, tests/parity_helpers.py BATCH_REGIME on one utterance of 40 frames, the benchmark batch's shape
    // (large enough for every merged sum), and ZV_MERGE_ALWAYS on 40 frames (tests/test_gpu_vocoder_widths.py runs these shapes)
#define BATCH_REGIME_SW "ZV_BLOCK64=-11 ZV_CONV_STREAM=2 ZV_CONV_GEMM=2 ZV_UP_GEMM=2 ZV_PAIR64_RING=2 ZV_TRIPLE_V2=3 ZV_FUSE256=1 ZV_PAIR_MT=0 ZV_DEC_PREPASS=1"
    // 256: 128 / 64 / 32 / 16 channels.  Pairs of 128 at rate 5, of 64 at 25, whole blocks at 100 (its three outputs feed the next
    // upsample conv), the 16-channel last stage unfused.  The first upsample conv alone has the pack (256 -> 5 x 128: 20 tiles, 768 deep)
    // and reads the input conv's f16 output (256 == 256).  Batch: 5 x 32 768 / 118 = 1 388 >= 1 024 merges the 128-channel stage,
    // 25 x 32 768 / 246 = 3 330 the 64-channel one, whose 3-tap branch goes to block64 (/ 244 = 3 357)
    {"v256", "", ONE(24), "r0 h0 -F000- -F000- -W000- -N000-"},
    {"v256", BATCH_REGIME_SW, ONE(40), "r0 h1 -F000- -F111- -W000- -N000-"},
    {"v256", "", BENCH, "r1 h1 -F0001 -F1001 -W000- -N000-"},
    {"v256", "ZV_MERGE_ALWAYS=1", ONE(40), "r0 h0 -F0001 -F0001 -W000- -N000-"},
    // 496: 248 / 124 / 62 / 31 channels in 256 / 128 / 64 / 32 padded ones: medium's kernels.  The first upsample conv reads 496
    // channels, no multiple of 64: no pack, so the input conv never writes f16; the second (256 -> 5 x 128) has it
    {"v496", "", ONE(24), "r0 h0 -N000- -F000- -F000- -W000-"},
    {"v496", BATCH_REGIME_SW, ONE(40), "r0 h0 -F000- pF000- -F111- -W000-"},
    {"v496", "", BENCH, "r1 h0 -F0003 pF0001 -F1001 -W000-"},
    {"v496", "ZV_MERGE_ALWAYS=1", ONE(40), "r0 h0 -N000- -F0001 -F0001 -W000-"},
    {"v496", "ZV_MERGE_ALWAYS=1 ZV_MERGE_SEQ=0", ONE(40), "r0 h0 -N000- -F0001 -F0001 -W000-"},
    // ... the whole-block kernel never merges: the output conv reads a merged sum of 31 channels only without it
    {"v496", "ZV_MERGE_ALWAYS=1 ZV_NO_TRIPLE=1", ONE(40), "r0 h0 -N000- -F0001 -F0001 -F0001"},
    // 768: 384 / 192 / 96 / 48 channels: pair_supported takes none of them.  Packs for 768 -> 5 x 384 (60 tiles: 7 groups + 4 tiles)
    // and 384 -> 5 x 192 (30 tiles: 3 groups + 6); 192 -> 4 x 96 is 576 deep: none
    {"v768", "", ONE(24), "r0 h0 -N000- -N000- -N000- -N000-"},
    {"v768", BATCH_REGIME_SW, ONE(40), "r0 h1 -N000- pN000- -N000- -N000-"},
    {"v768", "", BENCH, "r1 h1 -N000- pN000- -N000- -N000-"},
    {"v768", "ZV_MERGE_ALWAYS=1", ONE(40), "r0 h0 -N000- -N000- -N000- -N000-"},
    // 1024: 512 / 256 / 128 / 64 channels.  The 512-channel stage unfused; 256 channels at rate 25: (25 x 24 / 54) x 3 = 33 < 256 CUs, not
    // enough rows for one short utterance; pairs of 128 at rate 100 and of 64 at rate 300, the last stage: its merged sum is the
    // output conv's only input.  Packs for the first three upsample convs (1 024 -> 5 x 512, 512 -> 5 x 256, 256 -> 4 x 128: 768 deep)
    {"v1024", "", ONE(24), "r0 h0 -N000- -N000- -F000- -F000-"},
    {"v1024", BATCH_REGIME_SW, ONE(40), "r0 h1 -N000- pF000- pF000- -F111-"},
    {"v1024", "", BENCH, "r1 h1 -N000- pF0003 pF0001 -F1001"},
    {"v1024", "ZV_MERGE_ALWAYS=1", ONE(40), "r0 h0 -N000- -N000- -F0001 -F0001"},
    {"v1024", "ZV_MERGE_ALWAYS=1 ZV_MERGE_SEQ=0", ONE(40), "r0 h0 -N000- -N000- -F0001 -F0001"},
    {"v1024", BATCH_REGIME_SW " ZV_MERGE_ALWAYS=1", ONE(40), "r0 h1 -N000- pF0003 pF0001 -F1111"},
    // a tail group of 4 utterances of a 16 x 900-frame batch (tests/test_gpu_vocoder_widths.py), fitted: 300 x 900 x 4 / 246 = 4 390 >= 1 024
    // merges the 64-channel last stage inside the group, / 244 = 4 426 gives its 3-tap branch to block64; width 256: nothing to fuse there
    // (a group runs its last stage only; the stages before it are planned, and run, for the whole batch)
    {"v1024", "", with(call(4, 900, 14400), true, false, false, -1), "r0 h0 -N000- pF0003 pF0001 -F1001"},
    {"v256", "", with(call(4, 900, 14400), true, false, false, -1), "r0 h0 -F000- -F000- -W000- -N000-"},
};

// what the loader makes of a width: padded output channels of the input conv; per stage padded channels, padded input channels of
// the upsample conv, whether it has its conv_gemm_kernel pack
static const struct { const char *name; int in_Cout_p, Cp[4], up_Cin_p[4]; bool up_gemm[4]; } WIDTHS[] = {
    {"medium", 512, {256, 128, 64, 32}, {512, 256, 128, 64}, {true, true, false, false}},
    {"v256", 256, {128, 64, 32, 16}, {256, 128, 64, 32}, {true, false, false, false}},
    {"v496", 496, {256, 128, 64, 32}, {496, 256, 128, 64}, {false, true, false, false}},
    {"v768", 768, {384, 192, 96, 48}, {768, 384, 192, 96}, {true, true, false, false}},
    {"v1024", 1024, {512, 256, 128, 64}, {1024, 512, 256, 128}, {true, true, true, false}},
};

// one utterance of 16 frames, medium geometry (tests/parity_helpers.py: VOCODER_REGIMES by name, BATCH_REGIME as "batch_regime").
// D: 80 rows at 256 channels are not enough_rows (:246), no length threshold is met, the 32-channel stage runs whole blocks.
#define D "r0 h0 -N000- -F000- -F000- -W000-"
static const struct { const char *name, *want; } REGIMES[] = {
    {"default", D},
    {"fuse256", "r0 h0 -F000- -F000- -F000- -W000-"},                          // :246
    {"no_triple", "r0 h0 -N000- -F000- -F000- -F000-"},                        // :253
    {"no_fuse", "r0 h0 -N000- -N000- -N000- -N000-"},                          // :247
    {"no_merge", D},                                                          // :397 (nothing merges at 16 frames anyway)
    {"fuse256_no_merge", "r0 h0 -F000- -F000- -F000- -W000-"},
    {"merge", "r0 h0 -N000- -F0001 -F0001 -W000-"},                            // :396 any length; :397 fused stages only, not whole blocks (:337)
    {"fuse256_merge", "r0 h0 -F0003 -F0001 -F0001 -W000-"},                    // :404
    {"merge_in_one_workgroup", "r0 h0 -N000- -F0001 -F0001 -W000-"},
    {"fuse256_merge_in_one_workgroup", "r0 h0 -F0001 -F0001 -F0001 -W000-"},   // :404 ZV_MERGE_SEQ = 0
    {"fuse256_merge_mt3", "r0 h0 -F0003 -F0001 -F0001 -W000-"},                // (ZV_PAIR_MT: the launcher's)
    {"pair64_ring_merge", "r0 h0 -N000- -F0001 -F0001 -W000-"},                // (ZV_PAIR64_RING: the launcher's)
    {"single_loop_everywhere", D}, {"no_single_loop", D},                     // (launch_conv's)
    {"block_v1", D}, {"block_v2", D}, {"block_v2_512", D}, {"block_v2_512_one_weight_buffer", D}, {"block_v2_not_interleaved", D},      // (launch_triple's)
    {"pair64_ring", D}, {"pair64_ring_no_merge", D}, {"pair64_no_ring", D},
    {"upsample_gemm", "r0 h1 -N000- pF000- -F000- -W000-"},                    // :141-142, :203, :208: the two convs that have the pack
    {"upsample_no_gemm", D},
    {"block64_3_merge", "r0 h0 -N000- -F0001 -F1001 -W000-"},                  // :302 negative: at any length; :312 the 3-tap branch
    {"block64_3_no_merge", "r0 h0 -N000- -F000- -F100- -W000-"},
    {"block64_11", "r0 h0 -N000- -F000- -F111- -W000-"},                       // :312 3, 7 and 11 taps
    {"no_block64", D},
    {"upsample_stream", D}, {"upsample_no_stream", D},                        // (launch_conv's)
    {"pair_mt4", "r0 h0 -F000- -F000- -F000- -W000-"},
    {"pair_no_ring_no_triple", "r0 h0 -N000- -F0001 -F0001 -F0001"},           // :253, then :396-397 at 32 channels
    {"single_loop_everywhere_plain_grid", D}, {"plain_grid", D},
    {"batch_regime", "r0 h1 -F000- pF000- -F111- -W000-"},
};

// capi.cpp:723-724 (of the same commit): more than one group only for sw > 1, at least 4 utterances and 16 MiB of waveform, outside
// profiles and debug taps; then min(sw, nseg / 2)
static const struct { int sw, nseg; size_t bytes; bool prof, dbg; int want; } GROUPS[] = {
    {0, 3, 16u << 20, false, false, 1}, {1, 3, 16u << 20, false, false, 1}, {5, 3, 16u << 20, false, false, 1}, {8, 3, 16u << 20, false, false, 1},
    {0, 4, (16u << 20) - 1, false, false, 1}, {1, 4, (16u << 20) - 1, false, false, 1}, {5, 4, (16u << 20) - 1, false, false, 1},
    {8, 4, (16u << 20) - 1, false, false, 1},
    {0, 4, 16u << 20, false, false, 1}, {1, 4, 16u << 20, false, false, 1}, {5, 4, 16u << 20, false, false, 2}, {8, 4, 16u << 20, false, false, 2},
    {2, 4, 16u << 20, false, false, 2}, {5, 32, 157286400, false, false, 5}, {8, 32, 157286400, false, false, 8}, {20, 32, 157286400, false, false, 16},
    {5, 3, (16u << 20) - 1, false, false, 1}, {8, 32, 157286400, true, false, 1}, {8, 32, 157286400, false, true, 1},
};

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    std::string sw;
    for (int i = mode == "regime" ? 3 : 6; i < argc; i++) sw += (sw.empty() ? "" : " ") + std::string(argv[i]);
    if (mode == "cases" && argc == 2)
    {
        int n = 0;
        for (const Case &c : CASES)
        {
            if (!set_switches(c.switches)) return printf("bad switch list '%s'\n", c.switches), 1;
            const VocGeom g = geometry(c.geom);
            const std::string got = text(g, voc_plan(g, c.c));
            if (got != c.want)
                return printf("%s [%s] nseg %d t_max %d t_rows %zu fitted %d runs_off %d dbg %d/%d:\n  got  %s\n  want %s\n", c.geom, c.switches, c.c.nseg,
                              c.c.t_max, c.c.t_rows, c.c.fitted, c.c.runs_off, c.c.dbg_active, c.c.dbg_stage, got.c_str(), c.want), 1;
            n++;
        }
        for (const auto &q : WIDTHS)
        {
            const VocGeom g = geometry(q.name);
            bool same = g.in_Cout_p == q.in_Cout_p;
            for (int i = 0; i < 4; i++) same = same && g.st[i].Cp == q.Cp[i] && g.st[i].up_Cin_p == q.up_Cin_p[i] && g.st[i].up_gemm == q.up_gemm[i];
            if (!same) return printf("geometry %s: not what the table says\n", q.name), 1;
            n++;
        }
        for (const auto &q : GROUPS)
        {
            const int got = voc_tail_groups(q.sw, q.nseg, q.bytes, q.prof, q.dbg);
            if (got != q.want) return printf("groups: switch %d nseg %d bytes %zu profiling %d dbg %d: got %d, want %d\n", q.sw, q.nseg, q.bytes, q.prof, q.dbg, got, q.want), 1;
            n++;
        }
        // the shared rule (vocoder.cpp:90): 0 never, 1 what the launch picks by itself, 2 always; 16 384 rows
        for (int v = 0; v < 3; v++)
            for (int by_itself = 0; by_itself < 2; by_itself++, n++)
                if (batch_switch(v, by_itself) != (v == 2 || (v == 1 && by_itself))) return printf("batch_switch(%d, %d)\n", v, by_itself), 1;
        if (batch_rows(16383) || !batch_rows(16384)) return printf("batch_rows\n"), 1;
        printf("ok %d\n", n + 1);
        return 0;
    }
    if (mode == "regime" && argc >= 3)
    {
        if (!set_switches(sw.c_str())) return printf("bad switch list '%s'\n", sw.c_str()), 1;
        const VocGeom g = geometry("medium");
        const std::string got = text(g, voc_plan(g, ONE(16)));
        for (const auto &r : REGIMES)
            if (strcmp(r.name, argv[2]) == 0)
            {
                if (got != r.want) return printf("regime %s [%s]:\n  got  %s\n  want %s\n", r.name, sw.c_str(), got.c_str(), r.want), 1;
                printf("ok\n");
                return 0;
            }
        return printf("regime %s: no expectation in tests/native/voc_plan_check.cpp\n", argv[2]), 1;
    }
    if (mode == "plan" && argc >= 6)
    {
        if (!set_switches(sw.c_str())) return printf("bad switch list '%s'\n", sw.c_str()), 1;
        const VocGeom g = geometry(argv[2]);
        printf("%s\n", text(g, voc_plan(g, call(atoi(argv[3]), atoi(argv[4]), (size_t)atol(argv[5])))).c_str());
        return 0;
    }
    fprintf(stderr, "usage: see the head of tests/native/voc_plan_check.cpp\n");
    return 2;
}
