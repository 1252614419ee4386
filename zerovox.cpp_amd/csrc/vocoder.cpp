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
    v.level_slab = a.take(level_slab_entries(bt) * 16);
    v.env_knots = a.take_n<uint32_t>(env_knot_entries(bt));
    v.contour_slab = a.take(bt.t_rows * 16);
    v.pitch_slab = a.take(bt.t_rows * sizeof(PitchSlabRow));
    // the filter's input: the one region that exists only where a call asks for it (a waveform's worth of arena)
    v.filter_in = bt.wave.d_flt_par ? a.take_n<float>(bt.t_rows * hp.audio_hop_size) : nullptr;
    v.runs = a.take_n<Seg>(bt.nseg);
    return v;
}

// nseg * ceil(t_max * hop / chunk) <= nseg * t_max * hop / chunk + nseg <= t_rows * hop / chunk + t_rows / t_max
size_t Model::level_slab_entries(const Batch &bt) const
{
    return (bt.t_rows * hp.audio_hop_size + LEVEL_CHUNK_SAMPLES - 1) / LEVEL_CHUNK_SAMPLES + bt.t_rows / (size_t)std::max(bt.t_max, 1) + 1;
}

size_t Model::env_knot_entries(const Batch &bt) const { return bt.t_rows + bt.t_rows / (size_t)std::max(bt.t_max, 1) + 1; }

// HiFi-GAN vocoder (reference src/hifigan.cpp:187-377): fixed schedule of 2 + n_up * 7 launches
void Model::vocode_dev(const Batch &bt, const float *d_mel, float *d_wav)
{
    if (bt.t_rows == 0 || bt.t_max <= 0) fail(ZV_ERR_ARG, "T must be > 0");
    vocode_group(bt, d_mel, d_wav);
}

VocCall Model::voc_call(const Batch &bt) const
{
    return VocCall{bt.nseg, bt.t_max, bt.t_rows, n_cu, bt.d_frm_live != nullptr, voc_runs_off, dbg_layer.kind >= 0,
                   dbg_layer.kind == 0 ? dbg_layer.index / voc_.n_rb : -1};
}

bool Model::voc_runs_on(const Batch &bt) const { return voc_runs(voc_call(bt)); }

void Model::vocode_tail(const Batch &bt, const float *d_mel, float *d_wav, int g0, int cnt)
{
    if (!bt.d_frm || g0 < 0 || cnt < 1 || g0 + cnt > bt.nseg) fail(ZV_ERR_ARG, "internal: bad segment group");
    Batch sub = bt;
    sub.d_frm = bt.d_frm + g0;
    if (bt.d_frm_live) sub.d_frm_live = bt.d_frm_live + g0;
    sub.wave = bt.wave.group(g0);
    sub.nseg = cnt;
    vocode_group(sub, d_mel, d_wav, 2, g0);
}

TripleJob Model::block_job(const ResPair *rp, int n_dil, bool ring, const float *y, float *out) const
{
    TripleJob t;
    memset(&t, 0, sizeof(t));
    t.y = y;
    t.out = out;
    t.n_dil = n_dil;
    t.Cp = rp[0].c1.Cout_p;
    t.K = rp[0].c1.K;            // one K per job: voc_plan.h takes no other branch
    t.slope = 0.1f;
    for (int d = 0; d < n_dil; d++)
    {
        t.w1[d] = ring ? rp[d].r1 : rp[d].p1;
        t.w2[d] = ring ? rp[d].r2 : rp[d].p2;
        if (!ring)
        {
            t.w1x[d] = rp[d].x1;
            t.w2x[d] = rp[d].x2;
        }
        t.b1[d] = rp[d].c1.bias;
        t.b2[d] = rp[d].c2.bias;
        t.dil[d] = voc_.dil[d];
    }
    return t;
}

Model::DilPairJobs Model::pair_jobs(const ResPair &rp, int dil, const float *yin, float *yout, _Float16 *xt, float *y) const
{
    DilPairJobs r;
    // xt = lrelu(conv(lrelu(y), k, dil) + b)  kept as the f16 operand of the next conv (:108-150)
    r.c1 = job(rp.c1);
    r.c1.x0 = yin;
    r.c1.pro = PRO_ACT;
    r.c1.slope = 0.1f;
    r.c1.dil = dil;
    r.c1.pad = (rp.c1.K - 1) / 2 * dil;
    r.c1.eact = 1;
    r.c1.oslope = 0.1f;
    r.c1.out_f16 = 1;
    r.c1.out = xt;
    // y = y + (conv(xt, k, 1) + b)                                                    (:169-181)
    r.c2 = job(rp.c2);
    r.c2.x0 = xt;
    r.c2.pro = PRO_RAW_F16;
    r.c2.res = yin;
    r.c2.ldres = rp.c1.Cout_p;
    r.c2.out = y;
    memset(&r.p, 0, sizeof(r.p));
    r.p.y = yin;
    r.p.out = yout;
    r.p.w1 = rp.x1;
    r.p.w2 = rp.x2;
    r.p.w1r = rp.r1;
    r.p.w2r = rp.r2;
    r.p.b1 = rp.c1.bias;
    r.p.b2 = rp.c2.bias;
    r.p.Cp = rp.c1.Cout_p;
    r.p.K = rp.c1.K;
    r.p.dil = dil;
    r.p.slope = 0.1f;
    return r;
}

void Model::vocode_group(const Batch &bt, const float *d_mel, float *d_wav, int part, int seg0)
{
    struct Unskip { bool &f; ~Unskip() { f = false; } } unskip{skip_launch_};
    skip_launch_ = part == 2;
    const VocLayout lay = voc_layout(stage_arena(bt), bt);
    const int M = hp.audio_num_mels;
    const VocPlan plan = voc_plan(voc_geom_, voc_call(bt));       // a tail group's plan from its own sub-batch, as its launches
    // Run-shortened schedule: every launch below takes its extents from the run table and the input conv reads the compacted mel;
    // the output conv puts the samples back where they belong and a fill repeats the one frame the run stands for.  The head
    // (part 0 / 1) writes table and mel, a tail (part 2) finds its segments' entries from seg0 on.
    const bool runs = plan.runs;
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

    // V0: (mel - mean) / scale -> input conv k7 + bias            (src/hifigan.cpp:242-265)
    {
        ConvJob j = job(voc_.in_conv);
        j.x0 = d_mel;
        j.ldx = M;
        j.pro = PRO_MELNORM;
        j.pa = voc_.mean;
        j.pb = voc_.scale;
        j.out = c0;
        if (plan.c0_f16)
        {   // batches: the only reader is the first upsample conv on conv_gemm_kernel: its operand f16(lrelu(c0, 0.1)) straight from here
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
        const VocStagePlan &sp = plan.st[i];
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
            if (i == 0 && plan.c0_f16)
            {
                j.x0 = c0;
                j.pro = PRO_RAW_F16;
            }
            else if (sp.up_pass)
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
        // V2: the 3 MRF branches run side by side (one job each).  Fused path: one launch per dilation
        // (conv -> lrelu -> conv -> + residual, xt kept in LDS), y ping-pongs between two buffers because a
        // workgroup's halo rows belong to its neighbours' output tiles.  Which form a stage runs: voc_plan.h
        const ResPair *const rps = &voc_.pairs[(size_t)i * voc_.n_rb * voc_.n_dil];       // [branch][dilation]
        const float *ycur[3] = {ub, ub, ub};
        const float *merged_sum = nullptr;
        // the profile's bytes and flops of a branch's first n dilation pairs
        auto block_cost = [&](const ResPair *rp, int n, double &bytes, double &flops) {
            for (int d = 0; d < n; d++)
            {
                bytes += conv_bytes(La, C, C, rp[d].c1.K, false) + conv_bytes(La, C, C, rp[d].c2.K, true);
                flops += conv_flops(La, C, C, rp[d].c1.K) + conv_flops(La, C, C, rp[d].c2.K);
            }
        };
        group_begin();
        // narrow stages: the whole residual block (all dilations) of the three branches in ONE launch, y tile kept
        // in registers between the dilation pairs (launch_triple)
        if (sp.whole_block)
        {
            TripleJob tj[3];
            double bb = 0, ff = 0;
            for (int jb = 0; jb < 3; jb++)
            {
                tj[jb] = block_job(rps + jb * voc_.n_dil, voc_.n_dil, false, ub, y[jb]);
                block_cost(rps + jb * voc_.n_dil, voc_.n_dil, bb, ff);
                ycur[jb] = y[jb];
            }
            ZV_LAUNCH("voc_resblock_conv", bb, ff, launch_triple(stream(), tj, 3, n_cu, fr, rate));
        }
        // 64 channels, batches: the first two dilation pairs of the branches with few taps in ONE launch (resblock_block64_kernel)
        {
            TripleJob tj[3];
            int nj = 0;
            double bb = 0, ff = 0;
            for (int jb = 0; jb < 3; jb++)
            {
                if (!sp.block64[jb]) continue;
                tj[nj++] = block_job(rps + jb * voc_.n_dil, 2, true, ub, (float *)xt[jb]);
                block_cost(rps + jb * voc_.n_dil, 2, bb, ff);
                ycur[jb] = (float *)xt[jb];
            }
            if (nj) ZV_LAUNCH("voc_resblock_conv", bb, ff, launch_block64(stream(), tj, nj, fr, rate));
        }
        for (int d = 0; d < voc_.n_dil && !sp.whole_block; d++)
        {
            ConvJob j1[3], j2[3];
            PairJob pj[3];
            double b1 = 0, f1 = 0, b2 = 0, f2 = 0;
            int npj = 0;                     // pair jobs of this dilation (the branches resblock_block64_kernel has not covered)
            for (int jb = 0; jb < 3; jb++)
            {
                if (sp.block64[jb] && d < 2) continue;
                const ResPair &rp = rps[jb * voc_.n_dil + d];
                float *yout = sp.fused ? ((d & 1) ? (float *)xt[jb] : y[jb]) : y[jb];
                if (sp.fused && !rp.p1) fail(ZV_ERR_SHAPE, "residual block %d: branches of one stage must all be fusable", i * voc_.n_rb + jb);
                const DilPairJobs pq = pair_jobs(rp, voc_.dil[d], ycur[jb], yout, xt[jb], y[jb]);
                j1[jb] = pq.c1;
                j2[jb] = pq.c2;
                pj[npj++] = pq.p;
                ycur[jb] = sp.fused ? yout : y[jb];
                b1 += conv_bytes(La, C, C, rp.c1.K, false);
                f1 += conv_flops(La, C, C, rp.c1.K);
                b2 += conv_bytes(La, C, C, rp.c2.K, true);
                f2 += conv_flops(La, C, C, rp.c2.K);
            }
            // the last pair of the stage: the three branches' outputs are only ever used summed (MRF, :300-315), so the
            // workgroups run all three branches of a tile and store the sum alone, where voc_plan.h says it pays
            if (d == voc_.n_dil - 1 && sp.merge != VOC_MERGE_NONE)
            {
                bool ms_free = true;
                for (int q = 0; q < npj; q++) ms_free = ms_free && pj[0].out != pj[q].y;
                float *ms = ms_free ? pj[0].out : nullptr;
                if (!ms) fail(ZV_ERR_DEVICE, "internal: no free buffer for the merged MRF sum");
                if (sp.merge == VOC_MERGE_SEQ)
                {
                    // the branches one launch each on the side-by-side kernel, every launch adding its term into the running
                    // sum — (y0 + y1) + y2, the merged form's association, hence its bits
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
            else if (sp.fused)
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
    // Waveform filter (filter.h): with a request the convolution, the fill and the fitted tail's zeros go to the filter-input region
    // and the filter pass writes d_wav, so nothing behind it changes.  Never under a one-layer tap.
    const bool filtered = bt.wave.d_flt_par && dbg_layer.kind < 0;
    if (filtered && !lay.filter_in) fail(ZV_ERR_DEVICE, "internal: a filter without its input region");
    float *const conv_out = filtered ? lay.filter_in : d_wav;
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
        a.out = conv_out;
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
        if (runs) ZV_LAUNCH("voc_run_fill", 8.0 * (L - La), 0.0, launch_voc_run_fill(stream(), conv_out, fr, rate));
        if (dbg_layer.kind == ZV_LAYER_VOC_OUTPUT) dbg_extract(conv_out, 1, 1, L);
        // fitted: the output conv stops at each utterance's last frame; the rest of its capacity is silence
        if (bt.d_frm_live) ZV_LAUNCH("voc_zero_tail", 4.0 * La, 0.0, launch_zero_tail(stream(), conv_out, 1, bt.frames_cap(), fr, rate));
    }
    // the waveform of these segments is final: the stages a call carries, never under a one-layer tap
    if (dbg_layer.kind < 0) wave_stage_launches(bt, lay, d_wav, rate, seg0);
}

}  // namespace zv
