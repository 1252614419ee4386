// vocoder.cpp — the HiFi-GAN vocoder's arena layout and kernel schedule (see model.h).
#include "schedule.h"

#include <algorithm>
#include <cmath>

namespace zv
{

uint32_t Model::vocoder_halo_frames() const
{
    double frames = (voc_.in_conv.K - 1) / 2;            // input conv, at the frame rate
    double rate = 1.0;                                   // samples per frame at the current stage
    for (int i = 0; i < voc_.n_up; i++)
    {
        // polyphase transposed conv: ups[i].K taps at the INPUT rate of the stage
        frames += (double)voc_.ups[i].K / rate;
        rate *= voc_.scales[i];
        // residual blocks: per branch, every pair's dilated conv + plain conv (each conv's own K); the widest branch
        int reach = 0;
        for (int j = 0; j < voc_.n_rb; j++)
        {
            int r = 0;
            for (int d = 0; d < voc_.n_dil; d++)
            {
                const ResPair &rp = voc_.pairs[((size_t)i * voc_.n_rb + j) * voc_.n_dil + d];
                r += (rp.c1.K - 1) / 2 * voc_.dil[d] + (rp.c2.K - 1) / 2;
            }
            reach = std::max(reach, r);
        }
        frames += (double)reach / rate;
    }
    frames += (double)((voc_.out_K - 1) / 2) / rate;
    return (uint32_t)std::ceil(frames) + 1;
}

int Model::voc_stage_rate(int stage) const
{
    int r = 1;
    for (int i = 0; i <= stage && i < voc_.n_up; i++) r *= voc_.scales[i];
    return r;
}

int Model::voc_stage_channels(int stage) const { return voc_.in_conv.Cout >> (stage + 1); }

// The vocoder's buffers: the input conv's output, then two ping-pong pools; stage i carves (up + 3 y + 3 xt) out of pool i & 1, a pool is as large as its largest stage
Model::VocLayout Model::voc_layout(DeviceArena &a, const Batch &bt) const
{
    VocLayout v{};
    v.c0 = a.take_n<float>(bt.t_rows * voc_.in_conv.Cout_p);
    DeviceArena pool[2] = {DeviceArena::counter(), DeviceArena::counter()};
    for (int pass = 0; pass < 2; pass++)         // 0: the stages' carves measure the pools, 1: they carve them
    {
        size_t L = bt.t_rows, need[2] = {0, 0};
        for (int i = 0; i < voc_.n_up; i++)
        {
            DeviceArena &p = pool[i & 1];
            VocLayout::Stage &s = v.st[i];
            L *= voc_.scales[i];
            const size_t n = L * round_up(voc_.in_conv.Cout >> (i + 1), 16);
            p.used = 0;
            s.ub = p.take_n<float>(n);
            for (int j = 0; j < 3; j++) s.y[j] = p.take_n<float>(n);
            for (int j = 0; j < 3; j++) s.xt[j] = (_Float16 *)p.take_n<float>(n);   // f16 xt, or f32 ping-pong partner of y (fused path)
            need[i & 1] = std::max(need[i & 1], p.used);
        }
        for (int k = 0; k < 2 && pass == 0; k++) pool[k] = DeviceArena{(char *)a.take(need[k]), need[k], 0};
    }
    // the run-shortened schedule's compacted mel, flags and table: carved whether or not a call uses them (fitted, stream and
    // switch-off calls pay t_rows x (num_mels + 1) words of arena too), so that a layout depends on the batch's shape alone
    v.mel_c = a.take_n<float>(bt.t_rows * hp.audio_num_mels);
    v.eq = a.take_n<int32_t>(bt.t_rows);
    v.runs = a.take_n<Seg>(bt.nseg);
    return v;
}

// HiFi-GAN vocoder (reference src/hifigan.cpp:187-377): fixed schedule of 2 + n_up * 7 launches
void Model::vocode_dev(const Batch &bt, const float *d_mel, float *d_wav)
{
    if (bt.t_rows == 0 || bt.t_max <= 0) fail(ZV_ERR_ARG, "T must be > 0");
    vocode_group(bt, d_mel, d_wav);
}

// batches (ZV_VOC_RUNS = 1): by capacity, as the other batch switches — a single short utterance has no rounds of workgroups to
// give back, and its three extra launches would only add latency.  The threshold is the other batch switches', not a measured
// one: no sweep of capacities below it is on record, so small batches and long single utterances may be giving a gain away
bool Model::voc_runs_on(const Batch &bt) const
{
    const int k = knob(ZV_VOC_RUNS);
    return !voc_runs_off && !bt.d_frm_live && dbg_layer.kind < 0 && k != 0 && (k == 2 || (long)bt.t_rows >= 16384);
}

void Model::vocode_tail(const Batch &bt, const float *d_mel, float *d_wav, int g0, int cnt)
{
    if (!bt.d_frm || g0 < 0 || cnt < 1 || g0 + cnt > bt.nseg) fail(ZV_ERR_ARG, "internal: bad segment group");
    Batch sub = bt;
    sub.d_frm = bt.d_frm + g0;
    if (bt.d_frm_live) sub.d_frm_live = bt.d_frm_live + g0;
    sub.nseg = cnt;
    vocode_group(sub, d_mel, d_wav, 2, g0);
}

void Model::vocode_group(const Batch &bt, const float *d_mel, float *d_wav, int part, int seg0)
{
    struct Unskip { bool &f; ~Unskip() { f = false; } } unskip{skip_launch_};
    skip_launch_ = part == 2;
    const VocLayout lay = voc_layout(stage_arena(bt), bt);
    const int M = hp.audio_num_mels;
    // Run-shortened schedule: every launch below takes its extents from the run table and the input conv reads the compacted mel;
    // the output conv puts the samples back where they belong and a fill repeats the one frame the run stands for.  The head
    // (part 0 / 1) writes table and mel, a tail (part 2) finds its segments' entries from seg0 on.
    const bool runs = voc_runs_on(bt);
    const Segs fr = runs ? Segs{lay.runs + seg0, bt.nseg, bt.t_max, bt.frm1} : bt.frames();
    if (part != 2)
    {
        lane().runs_tab = runs ? lay.runs : nullptr;
        lane().runs_n = runs ? bt.nseg : 0;
    }
    if (runs)
    {
        ZV_LAUNCH("voc_runs", 12.0 * bt.t_rows * M, 0.0,
                  launch_voc_runs(stream(), d_mel, M, lay.mel_c, lay.eq, lay.runs, bt.frames_cap(), (int)vocoder_halo_frames()));
        d_mel = lay.mel_c;
    }
    size_t L = bt.t_rows;                       // capacity rows at the current stage (buffer sizes)
    double La = std::min((double)bt.t_rows, (double)bt.t_max * bt.nseg);      // rows this call covers (accounting)
    if (runs && profiling)
    {
        // the profile states work done: the rows the table holds (this path is eager and the host waits anyway)
        std::vector<Seg> tab((size_t)bt.nseg);
        ZV_HIP(hipMemcpyAsync(tab.data(), lay.runs + seg0, tab.size() * sizeof(Seg), hipMemcpyDeviceToHost, stream()));
        ZV_HIP(hipStreamSynchronize(stream()));
        La = 0;
        for (const Seg &g : tab) La += g.rows;
    }
    int rate = 1;
    int C = voc_.in_conv.Cout;
    float *c0 = lay.c0;
    // batches: the first upsample conv runs on conv_gemm_kernel over an f16 operand tensor (see below) — the input conv writes it
    const int upg0 = knob(ZV_UP_GEMM);
    const bool c0_f16 = dbg_layer.kind < 0 && voc_.n_up > 0 && voc_.ups[0].w8 && upg0 && knob(ZV_CONV_GEMM) != 0 &&
                        (upg0 == 2 || (long)L >= 16384) && voc_.ups[0].Cin_p == voc_.in_conv.Cout_p;

    // V0: (mel - mean) / scale -> input conv k7 + bias            (src/hifigan.cpp:242-265)
    {
        ConvJob j = job(voc_.in_conv);
        j.x0 = d_mel;
        j.ldx = M;
        j.pro = PRO_MELNORM;
        j.pa = voc_.mean;
        j.pb = voc_.scale;
        j.out = c0;
        if (c0_f16)
        {   // the only reader is the first upsample conv on conv_gemm_kernel: its operand f16(lrelu(c0, 0.1)) straight from here
            j.eact = 1;
            j.oslope = 0.1f;
            j.out_f16 = 1;
        }
        conv(&j, 1, fr, rate, "voc_input_conv", conv_bytes(La, M, C, j.K, false), conv_flops(La, M, C, j.K));
        if (dbg_layer.kind == ZV_LAYER_VOC_INPUT)
        {
            dbg_extract(c0, voc_.in_conv.Cout_p, C, L);
            return;
        }
    }

    const float third = (float)(1.0 / (float)voc_.n_rb);            // src/hifigan.cpp:315
    const float *prev_y[3] = {nullptr, nullptr, nullptr};
    const float *prev_merged = nullptr;          // the previous stage stored (y0 + y1) + y2 instead of the three branches
    for (int i = 0; i < voc_.n_up; i++)
    {
        const bool last_stage = i == voc_.n_up - 1;
        skip_launch_ = part == 2;                 // the head runs every upsample conv, the last stage's too (whole batch)
        const int s = voc_.scales[i];
        const ConvW &up = voc_.ups[i];
        const int Cout = C >> 1, Cp = round_up(Cout, 16);
        const size_t Lo = L * s;
        float *ub = lay.st[i].ub;
        float *y[3] = {lay.st[i].y[0], lay.st[i].y[1], lay.st[i].y[2]};
        _Float16 *const *xt = lay.st[i].xt;

        // V1: leaky_relu(0.1) -> transposed conv (polyphase) + bias      (src/hifigan.cpp:281-297, 22-71)
        {
            ConvJob j = job(up);
            j.slope = 0.1f;
            if (i == 0) { j.x0 = c0; j.pro = PRO_ACT; }
            else if (prev_merged) { j.x0 = prev_merged; j.pro = PRO_SCALE_ACT; j.pscale = third; }
            else { j.x0 = prev_y[0]; j.x1 = prev_y[1]; j.x2 = prev_y[2]; j.pro = PRO_SUM3_ACT; j.pscale = third; }
            const bool dbg_up = dbg_layer.kind == ZV_LAYER_VOC_UPSAMPLE && dbg_layer.index == i;
            if (dbg_up)
            {
                // the layer's input is what enters leaky_relu (src/hifigan.cpp:281): the input conv's output / the MRF mean
                float *in = i == 0 ? c0 : const_cast<float *>(prev_merged ? prev_merged : prev_y[0]);
                dbg_inject(in, up.Cin_p, C, L);
                j.x0 = in;
                j.x1 = j.x2 = nullptr;
                if (i > 0) { j.pro = PRO_SCALE_ACT; j.pscale = 1.0f; }
            }
            j.out = ub;
            // batches, wide upsample convs: the prologue as a pass of its own (f16 operand tensor, parked in the stage's last xt
            // buffer — free until the residual blocks run), the conv on conv_gemm_kernel (ZV_UP_GEMM = 0 never, 2 at any length)
            const int upg = knob(ZV_UP_GEMM);
            if (i == 0 && c0_f16)
            {
                j.x0 = c0;
                j.pro = PRO_RAW_F16;
            }
            else if (up.w8 && upg && knob(ZV_CONV_GEMM) != 0 && (upg == 2 || (long)L >= 16384) && (size_t)up.Cin_p * 2 * L <= Lo * Cp * 4)
            {
                ZV_LAUNCH("voc_upsample", 0.0, 0.0, launch_act_f16(stream(), (const float *)j.x0, (const float *)j.x1, (const float *)j.x2,
                                                                   j.pro == PRO_ACT ? 1.0f : j.pscale, j.slope, xt[2], (size_t)L * up.Cin_p));
                j.x0 = xt[2];
                j.x1 = j.x2 = nullptr;
                j.pro = PRO_RAW_F16;
                j.pscale = 1.0f;
            }
            // algorithmic: true polyphase MAC count L_in*Cin*Cout*k
            conv(&j, 1, fr, rate, "voc_upsample", 4.0 * La * C * (i == 0 ? 1 : 3) + 4.0 * La * s * Cout + 2.0 * C * Cout * 2 * s,
                 2.0 * La * C * Cout * 2 * s);
        }
        if (dbg_layer.kind == ZV_LAYER_VOC_UPSAMPLE && dbg_layer.index == i)
        {
            dbg_extract(ub, Cp, Cout, Lo);
            return;
        }
        skip_launch_ = (part == 1 && last_stage) || (part == 2 && !last_stage);
        L = Lo;
        La *= s;
        rate *= s;
        C = Cout;
        const bool dbg_here = dbg_layer.kind == 0 && dbg_layer.index / voc_.n_rb == i;
        if (dbg_here) dbg_inject(ub, Cp, Cout, L);
        const long Lbatch = (long)bt.t_max * rate * bt.nseg;       // rows the launches of this stage cover

        // V2: the 3 MRF branches run side by side (one job each).  Fused path: one launch per dilation
        // (conv -> lrelu -> conv -> + residual, xt kept in LDS), y ping-pongs between two buffers because a
        // workgroup's halo rows belong to its neighbours' output tiles.
        // every pair of the stage must have fused weights (one K for both convs, pair_supported): a stage runs fused or not as a
        // whole, so the MRF sum keeps one association whichever kernels a checkpoint's tap counts allow
        bool all_fusable = true;
        for (int q = 0; q < voc_.n_rb * voc_.n_dil; q++) all_fusable = all_fusable && voc_.pairs[(size_t)i * voc_.n_rb * voc_.n_dil + q].p1;
        // 256-channel stage: the fused kernel needs all 256 xt channels in one workgroup, which leaves few workgroups per
        // branch for a short utterance — two unfused launches (480 workgroups at 512 frames) win below about a round
        // of fused ones (round 4, on the 16 x 16 x 32 kernel, whole vocoder under graph replay: 128 frames 0.276 unfused /
        // 0.291 fused ms, 256: 0.320 / 0.333, 512: 0.470 / 0.465, 1 024: 0.852 / 0.814)
        const bool enough_rows = Cp != 256 || force_fuse256_ || (Lbatch / 54) * 3 >= (long)n_cu;
        const bool fused = !no_fuse_ && all_fusable && enough_rows;
        const float *ycur[3] = {ub, ub, ub};
        const float *merged_sum = nullptr;
        group_begin();
        // narrow stages: the whole residual block (all dilations) of the three branches in ONE launch, y tile kept
        // in registers between the dilation pairs (launch_triple)
        bool whole_block = fused && !no_triple_ && voc_.n_dil <= TRIPLE_MAX_DIL;
        for (int jb = 0; jb < 3 && whole_block; jb++)
        {
            // one K per job (TripleJob::K): every dilation pair of the branch must have it
            const ResPair &r0 = voc_.pairs[((size_t)i * voc_.n_rb + jb) * voc_.n_dil];
            whole_block = triple_supported(Cp, r0.c1.K, voc_.dil, voc_.n_dil);
            for (int d = 0; d < voc_.n_dil && whole_block; d++)
            {
                const ResPair &rp = voc_.pairs[((size_t)i * voc_.n_rb + jb) * voc_.n_dil + d];
                whole_block = rp.p1 != nullptr && rp.c1.K == r0.c1.K && rp.c2.K == r0.c1.K;
            }
        }
        if (whole_block)
        {
            TripleJob tj[3];
            double bb = 0, ff = 0;
            for (int jb = 0; jb < 3; jb++)
            {
                TripleJob &t = tj[jb];
                memset(&t, 0, sizeof(t));
                t.y = ub;
                t.out = y[jb];
                t.n_dil = voc_.n_dil;
                t.Cp = Cp;
                t.slope = 0.1f;
                for (int d = 0; d < voc_.n_dil; d++)
                {
                    const ResPair &rp = voc_.pairs[((size_t)i * voc_.n_rb + jb) * voc_.n_dil + d];
                    t.K = rp.c1.K;
                    t.w1[d] = rp.p1;
                    t.w2[d] = rp.p2;
                    t.w1x[d] = rp.x1;
                    t.w2x[d] = rp.x2;
                    t.b1[d] = rp.c1.bias;
                    t.b2[d] = rp.c2.bias;
                    t.dil[d] = voc_.dil[d];
                    bb += conv_bytes(La, C, C, rp.c1.K, false) + conv_bytes(La, C, C, rp.c2.K, true);
                    ff += conv_flops(La, C, C, rp.c1.K) + conv_flops(La, C, C, rp.c2.K);
                }
                ycur[jb] = y[jb];
            }
            ZV_LAUNCH("voc_resblock_conv", bb, ff, launch_triple(stream(), tj, 3, n_cu, fr, rate));
        }
        // 64 channels, batches: the first two dilation pairs of the branches with few taps in ONE launch (resblock_block64_kernel:
        // the branch's tensor crosses HBM once instead of twice; ZV_BLOCK64 = most taps it takes, 0 = never; negative: at any length)
        bool b64[3] = {false, false, false};
        {
            const int k64 = knob(ZV_BLOCK64);
            const int kmax64 = k64 < 0 ? -k64 : k64;
            if (fused && !whole_block && Cp == 64 && voc_.n_dil == 3 && kmax64 >= 3 && (k64 < 0 || Lbatch / 244 >= 4L * n_cu))
            {
                TripleJob tj[3];
                int nj = 0;
                double bb = 0, ff = 0;
                for (int jb = 0; jb < 3; jb++)
                {
                    const ResPair *rp = &voc_.pairs[((size_t)i * voc_.n_rb + jb) * voc_.n_dil];
                    // one K for the two pairs it runs (TripleJob::K)
                    const bool one_k = rp[1].c1.K == rp[0].c1.K && rp[0].c2.K == rp[0].c1.K && rp[1].c2.K == rp[0].c1.K;
                    if (!one_k || rp[0].c1.K > kmax64 || !rp[0].r1 || !rp[0].r2 || !rp[1].r1 || !rp[1].r2 || !block64_supported(Cp, rp[0].c1.K, voc_.dil, 2)) continue;
                    TripleJob &t = tj[nj++];
                    memset(&t, 0, sizeof(t));
                    t.y = ub;
                    t.out = (float *)xt[jb];
                    t.n_dil = 2;
                    t.Cp = Cp;
                    t.K = rp[0].c1.K;
                    t.slope = 0.1f;
                    for (int d = 0; d < t.n_dil; d++)
                    {
                        t.w1[d] = rp[d].r1;
                        t.w2[d] = rp[d].r2;
                        t.b1[d] = rp[d].c1.bias;
                        t.b2[d] = rp[d].c2.bias;
                        t.dil[d] = voc_.dil[d];
                        bb += conv_bytes(La, C, C, rp[d].c1.K, false) + conv_bytes(La, C, C, rp[d].c2.K, true);
                        ff += conv_flops(La, C, C, rp[d].c1.K) + conv_flops(La, C, C, rp[d].c2.K);
                    }
                    b64[jb] = true;
                    ycur[jb] = (float *)xt[jb];
                }
                if (nj) ZV_LAUNCH("voc_resblock_conv", bb, ff, launch_block64(stream(), tj, nj, fr, rate));
            }
        }
        for (int d = 0; d < voc_.n_dil && !whole_block; d++)
        {
            ConvJob j1[3], j2[3];
            PairJob pj[3];
            double b1 = 0, f1 = 0, b2 = 0, f2 = 0;
            int npj = 0;                     // pair jobs of this dilation (the branches resblock_block64_kernel has not covered)
            for (int jb = 0; jb < 3; jb++)
            {
                if (b64[jb] && d < 2) continue;
                const ResPair &rp = voc_.pairs[((size_t)i * voc_.n_rb + jb) * voc_.n_dil + d];
                const float *yin = ycur[jb];
                float *yout = fused ? ((d & 1) ? (float *)xt[jb] : y[jb]) : y[jb];
                if (fused && !rp.p1) fail(ZV_ERR_SHAPE, "residual block %d: branches of one stage must all be fusable", i * voc_.n_rb + jb);
                // xt = lrelu(conv(lrelu(y), k, dil) + b)  kept as the f16 operand of the next conv (:108-150)
                ConvJob a = job(rp.c1);
                a.x0 = yin;
                a.pro = PRO_ACT;
                a.slope = 0.1f;
                a.dil = voc_.dil[d];
                a.pad = (rp.c1.K - 1) / 2 * voc_.dil[d];
                a.eact = 1;
                a.oslope = 0.1f;
                a.out_f16 = 1;
                a.out = xt[jb];
                j1[jb] = a;
                // y = y + (conv(xt, k, 1) + b)                                                    (:169-181)
                ConvJob b = job(rp.c2);
                b.x0 = xt[jb];
                b.pro = PRO_RAW_F16;
                b.res = yin;
                b.ldres = Cp;
                b.out = y[jb];
                j2[jb] = b;
                PairJob &p = pj[npj++];
                memset(&p, 0, sizeof(p));
                p.y = yin;
                p.out = yout;
                p.w1 = rp.x1;
                p.w2 = rp.x2;
                p.w1r = rp.r1;
                p.w2r = rp.r2;
                p.b1 = rp.c1.bias;
                p.b2 = rp.c2.bias;
                p.Cp = Cp;
                p.K = rp.c1.K;
                p.dil = voc_.dil[d];
                p.slope = 0.1f;
                ycur[jb] = fused ? yout : y[jb];
                b1 += conv_bytes(La, C, C, rp.c1.K, false);
                f1 += conv_flops(La, C, C, rp.c1.K);
                b2 += conv_bytes(La, C, C, rp.c2.K, true);
                f2 += conv_flops(La, C, C, rp.c2.K);
            }
            // the last pair of the stage: the three branches' outputs are only ever used summed (MRF, :300-315), so the
            // workgroups run all three branches of a tile and store the sum alone
            // ... once the merged launch (a third of the workgroups, each three times as long) still has rounds of workgroups to
            // spare: at one round (a single 512-frame utterance) the merged 128- / 64-channel launches took 45.7 / 37.3 us against
            // 28.4 / 32.8 us for the three branches side by side, more than the upsample conv gains from reading one tensor
            const int merge_tile = Cp >= 256 ? 54 : (Cp == 128 ? 118 : 246);
            const bool merge_pays = knob(ZV_MERGE_ALWAYS) != 0 || (Lbatch / merge_tile >= 4L * n_cu && Cp <= knob(ZV_MERGE_MAXC));
            const bool merge = fused && !no_merge_ && !dbg_here && d == voc_.n_dil - 1 && merge_pays;
            if (merge)
            {
                bool ms_free = true;
                for (int q = 0; q < npj; q++) ms_free = ms_free && pj[0].out != pj[q].y;
                float *ms = ms_free ? pj[0].out : nullptr;
                if (!ms) fail(ZV_ERR_DEVICE, "internal: no free buffer for the merged MRF sum");
                if (Cp >= 256 && knob(ZV_MERGE_SEQ) != 0)
                {
                    // 256 channels: the branches one launch each on the side-by-side kernel (96-row tiles, all staging loads in flight:
                    // 1 020 us for the three against 1 105 us for the three-branches-per-workgroup form; at 128 channels the single-
                    // branch launches' tails cost more than they gain: 1 422 against 1 386 us), every launch adding its term into the
                    // running sum — (y0 + y1) + y2, the merged form's association, hence its bits
                    for (int jb = 0; jb < 3; jb++)
                    {
                        PairJob q = pj[jb];
                        q.sum_out = ms;
                        q.sum_in = jb ? ms : nullptr;
                        ZV_LAUNCH("voc_resblock_conv", (b1 + b2) / 3, (f1 + f2) / 3, launch_pair(stream(), &q, 1, n_cu, fr, rate));
                    }
                }
                else
                    ZV_LAUNCH("voc_resblock_conv", b1 + b2, f1 + f2,
                              launch_pair(stream(), pj, npj, n_cu, fr, rate, ms));
                merged_sum = ms;
            }
            else if (fused)
            {
                if (npj) ZV_LAUNCH("voc_resblock_conv", b1 + b2, f1 + f2, launch_pair(stream(), pj, npj, n_cu, fr, rate));
            }
            else
            {
                conv(j1, 3, fr, rate, "voc_resblock_conv", b1, f1);
                conv(j2, 3, fr, rate, "voc_resblock_conv", b2, f2);
            }
        }
        // one profile entry per stage (bench.py prices every stage against its own binding roof)
        static const char *const rb_names[8] = {"voc_resblock_s0", "voc_resblock_s1", "voc_resblock_s2", "voc_resblock_s3",
                                                "voc_resblock_s4", "voc_resblock_s5", "voc_resblock_s6", "voc_resblock_s7"};
        group_end(rb_names[i < 8 ? i : 7]);
        if (dbg_here)
        {
            dbg_extract(ycur[dbg_layer.index % voc_.n_rb], Cp, Cout, L);
            return;
        }
        for (int jb = 0; jb < 3; jb++) y[jb] = const_cast<float *>(ycur[jb]);
        for (int jb = 0; jb < 3; jb++) prev_y[jb] = y[jb];
        prev_merged = merged_sum;
    }

    // V3: (sum of branches)/3 -> leaky_relu(0.01) -> conv k7 (C -> 1) + b -> tanh          (:315-345)
    skip_launch_ = part == 1;
    {
        OutConvArgs a;
        a.x0 = prev_merged ? prev_merged : prev_y[0];
        a.x1 = prev_merged ? nullptr : prev_y[1];
        a.x2 = prev_merged ? nullptr : prev_y[2];
        a.ldx = round_up(C, 16);
        a.L = 0;
        a.C = C;
        a.K = voc_.out_K;
        a.pscale = third;
        a.slope = (float)1e-2;
        a.w = voc_.out_w;
        a.bias = voc_.out_b;
        a.out = d_wav;
        a.segs = fr;
        a.rate = rate;
        a.runs = runs;
        if (dbg_layer.kind == ZV_LAYER_VOC_OUTPUT)
        {
            // the layer's input is the MRF mean that enters leaky_relu(0.01) (src/hifigan.cpp:315-324)
            float *in = const_cast<float *>(a.x0);
            dbg_inject(in, a.ldx, C, L);
            a.x1 = a.x2 = nullptr;
            a.pscale = 1.0f;
        }
        ZV_LAUNCH("voc_output_conv", 12.0 * La * C + 4.0 * La, 2.0 * La * C * a.K, launch_out_conv(stream(), a));
        if (runs) ZV_LAUNCH("voc_run_fill", 8.0 * (L - La), 0.0, launch_voc_run_fill(stream(), d_wav, fr, rate));
        if (dbg_layer.kind == ZV_LAYER_VOC_OUTPUT) dbg_extract(d_wav, 1, 1, L);
        // fitted: the output conv stops at each utterance's last frame; the rest of its capacity is silence
        if (bt.d_frm_live) ZV_LAUNCH("voc_zero_tail", 4.0 * La, 0.0, launch_zero_tail(stream(), d_wav, 1, bt.frames_cap(), fr, rate));
    }
}

}  // namespace zv
