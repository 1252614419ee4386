// decoder.cpp — the StyleTTS mel decoder's arena layout and kernel schedule (see model.h).
#include "schedule.h"
#include "dec_runs.h"

#include <algorithm>
#include <cmath>

namespace zv
{

// The decoder's buffers: per-segment vectors and statistics partials, then the [t_rows] activations and f16 operands.
Model::DecLayout Model::dec_layout(DeviceArena &a, const Batch &bt) const
{
    // Rows and statistics blocks by the packed layout's worst case (dec_runs.h: every utterance's slot ends in up to 32 guard rows),
    // whether or not a call packs: a layout depends on the batch's shape alone.
    // Packed decoding keeps the packed copy of `hidden` in xa, which no block writes before decode block 2 and `hidden`'s last
    // reader, the asr conv, runs ahead of decode block 0 (2 E floats per row against hidden's E).
    const size_t S = (size_t)bt.nseg, L = (size_t)dec_pack_rows_cap((long)bt.t_rows, bt.nseg), B = 2 * E(), R = (size_t)dec_.R, CAT = B + R;
    DecLayout d{(bt.t_max + 31) / 32, round_up(dec_.fc_out + 64, 64), 2 * (int)CAT + 64};
    d.rows = (int)L;
    d.nblk_all = std::max(bt.nseg * d.nblk, (d.rows + 31) / 32);
    d.h = a.take_n<float>(S * d.hs);
    for (float **st : {&d.st_x, &d.st_t, &d.st_y, &d.st_a}) *st = a.take_n<float>(S * d.ss);
    for (double **p : {&d.part_t, &d.part_o}) *p = a.take_n<double>((size_t)d.nblk_all * CAT * 2);
    d.cat = a.take_n<float>(L * CAT);
    for (float **x : {&d.t1, &d.sc, &d.x0, &d.xa}) *x = a.take_n<float>(L * B);
    d.asr_t = a.take_n<float>(L * R);
    d.xa16 = a.take_n<_Float16>(L * CAT);
    d.t16 = a.take_n<_Float16>(L * B);
    d.xr16 = a.take_n<_Float16>(L * CAT);
    // carved whether or not a call decodes run-shortened, so that a layout depends on the batch's shape alone
    d.mel_c = a.take_n<float>(L * dec_.M);
    return d;
}

// a residual block reaches as far as the longer of its two paths (conv1 -> conv2, the shortcut); the concat joins the encode
// blocks' path and the asr conv's; the output conv ends the chain
int Model::dec_reach_frames() const
{
    auto half = [](const ConvW &w) { return w.K > 0 ? (w.K - 1) / 2 : 0; };
    auto blk = [&](const DecBlk &b) { return std::max(half(b.conv1) + half(b.conv2), b.learned_sc ? half(b.sc) : 0); };
    int r = std::max(blk(dec_.enc[0]) + blk(dec_.enc[1]), half(dec_.asr0));
    for (const DecBlk &b : dec_.dec) r += blk(b);
    return r + half(dec_.to_out);
}

// StyleTTS mel decoder (reference src/stylettsdec.cpp:306-470)
void Model::decode_dev(const Batch &bt, const float *d_hidden, const float *d_styles, float *d_mel)
{
    if (bt.t_rows == 0 || bt.t_max <= 0) fail(ZV_ERR_ARG, "T must be > 0");
    const DecLayout lay = dec_layout(stage_arena(bt), bt);
    // Run-shortened decoding: every launch below takes its extents from the run table the encoder wrote, the statistics add the
    // dropped blocks back, the last conv writes the compact mel and one pass expands it to d_mel's T rows per utterance.
    const DecPlan plan = dec_plan(bt);
    const bool runs = bt.d_dec_runs != nullptr;
    if (runs && !plan.runs) fail(ZV_ERR_ARG, "internal: a decoder run table on a schedule that takes none");
    const Segs fr = runs ? Segs{bt.d_dec_runs, bt.nseg, bt.t_max, bt.frm1} : bt.frames();
    // Densely packed decoding (dec_runs.h): the table's row0 are the utterances' slots in ONE packed row space.  The elementwise and
    // statistics launches keep the per-utterance table `fr`; every conv runs over the packed rows as the one segment of entry nseg
    // (`frc`), planned as the batch it is (conv_plan.h ConvPackedUtts), and stores its partial sums by global block, which is where
    // the finalising launches look (DEC_TAB_PACKED) — the last block of an utterance whose rows are no multiple of 32 apart
    // (DEC_TAB_CONV_TAIL).  The f16 operands carry zeros in the guard rows; what the convs leave in guard rows is never read.
    const bool pack = plan.pack;
    const Segs frc = pack ? Segs{bt.d_dec_runs + bt.nseg, 1, lay.rows, Seg{0, 0, 0, 0}} : fr;
    const ConvPackedUtts packed_utts(pack ? bt.nseg : 0);
    const int tab_mode = runs ? DEC_TAB_RUNS | (pack ? DEC_TAB_PACKED : 0) : 0, conv_tail = pack ? DEC_TAB_CONV_TAIL : 0;
    const int nblk_c = pack ? lay.nblk_all : lay.nblk;                  // the blocks a conv's partial sums are laid out by
    const int Ed = (int)E(), B = 2 * Ed, R = dec_.R, CAT = B + R, S = bt.nseg;
    const size_t L = bt.t_rows;                     // (capacity rows: the debug taps', which never pack)
    const int nblk = lay.nblk, hs = lay.hs, ss = lay.ss;
    float *const h = lay.h, *const st_x = lay.st_x, *const st_t = lay.st_t, *const st_y = lay.st_y, *const st_a = lay.st_a;
    double *const part_t = lay.part_t, *const part_o = lay.part_o;
    float *const cat = lay.cat, *const t1 = lay.t1, *const sc = lay.sc, *const x0 = lay.x0, *const xa = lay.xa, *const asr_t = lay.asr_t;
    _Float16 *const xa16 = lay.xa16, *const t16 = lay.t16, *const xr16 = lay.xr16;
    double Ld = (double)L;                          // rows the launches cover (accounting)
    if (runs && profiling)
    {
        // the profile states work done: the rows the table holds (this path is eager and the host waits anyway)
        std::vector<Seg> tab((size_t)S);
        ZV_HIP(hipMemcpyAsync(tab.data(), bt.d_dec_runs, tab.size() * sizeof(Seg), hipMemcpyDeviceToHost, stream()));
        ZV_HIP(hipStreamSynchronize(stream()));
        Ld = 0;
        for (const Seg &g : tab) Ld += g.rows;
    }
    const bool prepass = plan.prepass;

    // D2: all ten AdaIN fc layers at once for every utterance's style vector            (src/stylettsdec.cpp:175-189)
    ZV_LAUNCH("dec_adain_fc", 4.0 * dec_.fc_out * (Ed + 2), 2.0 * S * dec_.fc_out * Ed,
              launch_linear(stream(), d_styles, Ed, Ed, dec_.fcW, dec_.fcB, dec_.fc_out, h, hs, dec_.fcExtra, segs_single(S)));

    const float rsqrt2 = (float)(1.0 / sqrt(2.0));                       // src/stylettsdec.cpp:146,301

    // xconv: the tensor whose partial sums a conv stored in `part` (null: an elementwise launch stored them)
    auto finalize = [&](const double *part, int C, float *stat, int c_off, const float *xconv = nullptr, int ldxc = 0) {
        ZV_LAUNCH("dec_in_stats", 16.0 * S * nblk * C, 4.0 * S * nblk * C,
                  launch_stats_finalize(stream(), part, nblk, C, 1e-5f, stat, ss, c_off, fr, 1, tab_mode | (xconv ? conv_tail : 0), xconv, ldxc));
    };
    // make `j` read lrelu(norm(x)) with x's statistics still in `part` (channels [0, Cpart)); stores them in `stat`
    // from_conv: a conv stored x and `part` (else an elementwise launch did)
    auto norm_input = [&](ConvJob &j, const float *x, int ldx, int C, const double *part, int Cpart, float *stat, const float *g,
                          const float *b, int gb_seg, bool from_conv, _Float16 *op16, _Float16 *raw16 = nullptr) {
        if (prepass)
        {
            ZV_LAUNCH("dec_norm_operand", 6.0 * Ld * C, 8.0 * Ld * C,
                      launch_norm_act_f16(stream(), x, ldx, C, part, nblk, Cpart, 1e-5f, stat, ss, g, b, gb_seg, 0.2f, op16, C, fr, raw16,
                                          tab_mode | (from_conv ? conv_tail : 0)));
            j.x0 = op16;
            j.ldx = C;
            j.pro = PRO_RAW_F16;
        }
        else
        {
            finalize(part, Cpart, stat, 0);
            j.x0 = x;
            j.ldx = ldx;
            j.pro = PRO_NORM_ACT;
            j.pstat = stat;
            j.pstat_seg = ss;
            j.pa = g;
            j.pb = b;
            j.pab_seg = gb_seg;
            j.slope = 0.2f;
        }
    };

    // InstanceNorm statistics of the stage input (it comes from the encoder or the host, not from a conv of ours)
    const float *hidden = d_hidden;
    if (pack)
    {
        ZV_LAUNCH("dec_pack_rows", 8.0 * Ld * Ed, 0.0, launch_dec_pack_rows(stream(), d_hidden, xa, Ed, fr, bt.frames_cap()));
        hidden = xa;
    }
    ZV_LAUNCH("dec_in_stats", 4.0 * Ld * Ed, 3.0 * Ld * Ed, launch_stats_partial(stream(), hidden, Ed, Ed, part_o, nblk, fr, 1, pack));

    // one residual block: IN/AdaIN -> lrelu -> conv1 -> IN/AdaIN -> lrelu -> conv2 -> (+ shortcut) / sqrt2.
    // The partial sums of x's statistics are in part_o (channels [0, Cpart) of x; the others are final in st_in already);
    // the block leaves the partial sums of its output in part_o again when want_stats.  gb_seg: per-segment stride of the
    // affine vectors (0 for the encode blocks' shared InstanceNorm weights, hs for the decode blocks' AdaIN vectors).
    int blk_no = 0;              // 0,1: encode blocks; 2..6: decode blocks (dbg_layer.index)
    auto block = [&](const DecBlk &b, const float *x, int ldx, int Cpart, bool x_from_conv, float *st_in, const float *g1, const float *b1,
                     const float *g2, const float *b2, int gb_seg, float *out, int ldo, bool want_stats) {
        const bool dbg_here = dbg_layer.kind == 2 && dbg_layer.index == blk_no && !dbg_layer.done;
        blk_no++;
        if (dbg_layer.done) return;
        if (dbg_here)
        {   // the layer's input comes from the host; its statistics are recomputed for every channel
            dbg_inject(const_cast<float *>(x), ldx, b.cin, L);
            ZV_HIP(launch_stats_partial(stream(), x, ldx, b.cin, part_o, nblk, fr, 1));
            Cpart = b.cin;
            x_from_conv = false;
        }
        const float *res = x;
        int ldres = ldx;
        ConvJob jj[2];
        int nj = 0;
        {
            ConvJob j = job(b.conv1);
            // (a learned shortcut reads f16(x): with the pre-pass on, that operand is written by the same pass)
            norm_input(j, x, ldx, b.cin, part_o, Cpart, st_in, g1, b1, gb_seg, x_from_conv, xa16, b.learned_sc ? xr16 : nullptr);
            j.out = t1;
            j.stat_part = part_t;
            j.stat_nblk = nblk_c;
            j.stat_C = b.conv1.Cout;
            jj[nj++] = j;
        }
        double bytes = conv_bytes(Ld, b.cin, b.conv1.Cout, 3, false), flops = conv_flops(Ld, b.cin, b.conv1.Cout, 3);
        if (b.learned_sc)
        {
            ConvJob j = job(b.sc);
            j.x0 = x;
            j.ldx = ldx;
            if (prepass)
            {
                j.x0 = xr16;
                j.ldx = b.cin;
                j.pro = PRO_RAW_F16;
            }
            j.out = sc;
            res = sc;
            ldres = b.sc.Cout_p;
            const double sb = conv_bytes(Ld, b.cin, b.cout, 1, false), sf = conv_flops(Ld, b.cin, b.cout, 1);
            if (b.sc.Cout_p == b.conv1.Cout_p)
            {   // same output width as conv1: second job of the same launch
                jj[nj++] = j;
                bytes += sb;
                flops += sf;
            }
            else
                conv(&j, 1, frc, 1, "dec_conv", sb, sf);
        }
        conv(jj, nj, frc, 1, "dec_conv", bytes, flops);
        const int Cm = b.conv1.Cout;
        {
            ConvJob j = job(b.conv2);
            norm_input(j, t1, b.conv1.Cout_p, Cm, part_t, Cm, st_t, g2, b2, gb_seg, true, t16);
            j.res = res;
            j.ldres = ldres;
            j.escale = rsqrt2;
            j.out = out;
            j.ldo = ldo;
            if (want_stats)
            {
                j.stat_part = part_o;
                j.stat_nblk = nblk_c;
                j.stat_C = b.cout;
            }
            conv(&j, 1, frc, 1, "dec_conv", conv_bytes(Ld, Cm, b.cout, 3, true), conv_flops(Ld, Cm, b.cout, 3));
        }
        if (dbg_here) dbg_extract(out, ldo, b.cout, L);
    };

    // AdaIN1d alone (sub-block tap, ZV_LAYER_DEC_ADAIN; index = 2 * decode block + (norm - 1); reference src/stylettsdec.cpp:171-200):
    // the production fc GEMM above, the production statistics (partial sums + finalise) and the prologue's arithmetic
    // ((x - mean) * rstd) * gamma + beta written out by norm_apply_kernel — no activation, no conv
    if (dbg_layer.kind == ZV_LAYER_DEC_ADAIN)
    {
        const int bi = dbg_layer.index / 2, k = dbg_layer.index & 1;
        if (bi < 0 || bi >= 5) return;
        const DecBlk &b = dec_.dec[bi];
        const int Cn = k ? b.cout : b.cin, go = k ? b.g2 : b.g1;
        float *xin = cat;                                  // [L][Cn] with leading dimension Cn: any buffer of L * CAT floats
        dbg_inject(xin, Cn, Cn, L);
        ZV_HIP(launch_stats_partial(stream(), xin, Cn, Cn, part_o, nblk, fr, 1));
        ZV_HIP(launch_stats_finalize(stream(), part_o, nblk, Cn, 1e-5f, st_x, ss, 0, fr, 1));
        ZV_HIP(launch_norm_apply(stream(), xin, Cn, Cn, st_x, ss, h + go, h + go + Cn, t1, Cn, nullptr, nblk, fr));
        dbg_extract(t1, Cn, Cn, L);
        return;
    }

    // encode0 / encode1: ResBlk1d with affine InstanceNorm                         (src/stylettsdec.cpp:69-149,373-374)
    block(dec_.enc[0], hidden, Ed, Ed, false, st_x, dec_.enc[0].n1w, dec_.enc[0].n1b, dec_.enc[0].n2w, dec_.enc[0].n2b, 0, x0, B, true);
    block(dec_.enc[1], x0, B, B, true, st_y, dec_.enc[1].n1w, dec_.enc[1].n1b, dec_.enc[1].n2w, dec_.enc[1].n2b, 0, cat, CAT, true);

    // asr_res = IN_affine(conv1x1(enc_seq) + b) written straight into the concat buffer      (:382-404)
    if (dbg_layer.done) return;
    {
        ConvJob j = job(dec_.asr0);
        j.x0 = hidden;
        j.ldx = Ed;
        j.out = asr_t;
        j.stat_part = part_t;
        j.stat_nblk = nblk_c;
        j.stat_C = R;
        conv(&j, 1, frc, 1, "dec_conv", conv_bytes(Ld, Ed, R, 1, false), conv_flops(Ld, Ed, R, 1));
        finalize(part_t, R, st_a, 0, asr_t, R);
        ZV_LAUNCH("dec_norm_apply", 8.0 * Ld * R, 3.0 * Ld * R,
                  launch_norm_apply(stream(), asr_t, R, R, st_a, ss, dec_.asr1w, dec_.asr1b, cat + B, CAT, part_t, nblk, fr, pack));
        finalize(part_t, R, st_x, B);            // statistics of the concat's asr columns: final for decode0..2
        if (dbg_layer.kind == ZV_LAYER_DEC_ASR_RES)
        {
            dbg_extract(cat + B, CAT, R, L);
            return;
        }
    }

    // decode0..4: AdainResBlk1d; blocks 0..2 read cat([x, asr]) and 0,1 write x back into it   (:406-428).  The x
    // columns' statistics arrive as partial sums from the producing conv2, the asr columns' are already in st_x.
    const float *cur = cat;
    int ldc = CAT;
    float *outs[5] = {cat, cat, xa, x0, xa};
    const int ldos[5] = {CAT, CAT, Ed, Ed, Ed};
    const int cparts[5] = {B, B, B, Ed, Ed};
    float *sts[5] = {st_x, st_x, st_x, st_y, st_y};
    for (int i = 0; i < 5; i++)
    {
        const DecBlk &b = dec_.dec[i];
        block(b, cur, ldc, cparts[i], true, sts[i], h + b.g1, h + b.g1 + b.cin, h + b.g2, h + b.g2 + b.cout, hs, outs[i], ldos[i], i < 4);
        cur = outs[i];
        ldc = ldos[i];
    }
    // to_out: conv1x1 E -> num_mels + b, emitted frame-major                                       (:432-441)
    if (dbg_layer.done) return;
    {
        ConvJob j = job(dec_.to_out);
        j.x0 = cur;
        j.ldx = ldc;
        j.out = runs ? lay.mel_c : d_mel;
        j.ldo = dec_.M;
        if (dbg_layer.kind == ZV_LAYER_DEC_TO_OUT) dbg_inject(const_cast<float *>(cur), ldc, Ed, L);
        conv(&j, 1, frc, 1, "dec_conv", conv_bytes(Ld, Ed, dec_.M, 1, false), conv_flops(Ld, Ed, dec_.M, 1));
        if (dbg_layer.kind == ZV_LAYER_DEC_TO_OUT) dbg_extract(d_mel, dec_.M, dec_.M, L);
    }
    // all T rows of every utterance's mel from the rows computed: the vocoder sees the mel it always saw
    if (runs)
        ZV_LAUNCH("dec_run_expand", 4.0 * (Ld + (double)L) * dec_.M, 0.0,
                  launch_dec_run_expand(stream(), lay.mel_c, d_mel, dec_.M, fr, bt.frames_cap()));
}

}  // namespace zv
