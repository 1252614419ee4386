// encoder.cpp — the FastSpeech2 encoder's arena layout and kernel schedule (see model.h).
#include "schedule.h"

#include <cmath>

namespace zv
{

// The encoder's buffers, all [n_rows]: the FFT blocks' activations, the FFN's f16 operand, the predictors' pair, the taps.
Model::EncLayout Model::enc_layout(DeviceArena &a, const Batch &bt) const
{
    const size_t n = bt.n_rows, Ed = E();
    EncLayout e{round_up(enc_.dur.V, 16)};
    for (float **p : {&e.x, &e.y}) *p = a.take_n<float>(n * Ed);
    e.qkv = a.take_n<float>(n * 3 * Ed);
    for (float **p : {&e.o, &e.f}) *p = a.take_n<float>(n * Ed);
    e.hh = a.take_n<_Float16>(n * round_up(hp.conv_filter_size, 16));
    for (float **p : {&e.va, &e.vb}) *p = a.take_n<float>(n * e.Vp);
    for (float **p : {&e.t.logdur, &e.t.pitch, &e.t.energy}) *p = a.take_n<float>(n);
    for (int32_t **p : {&e.t.pitch_bucket, &e.t.energy_bucket}) *p = a.take_n<int32_t>(n);
    e.t.cum = bt.d_cum ? bt.d_cum : a.take_n<int32_t>(n);
    e.t.features = e.x;
    return e;
}

// FastSpeech2 encoder + variance adaptor + length regulator (reference src/fs2encoder.cpp:289-336,477-656)
Model::EncoderTaps Model::encode_dev(const Batch &bt, const int32_t *d_ids, const int32_t *d_puncts, const float *d_styles,
                                     float *d_hidden, int32_t *d_nframes)
{
    if (bt.n_rows == 0 || bt.t_rows == 0 || bt.n_max <= 0 || bt.t_max <= 0) fail(ZV_ERR_ARG, "N and T must be > 0");
    // the real extents decide (the kernels walk each segment's own rows); n_max is a capacity rounded up for grid sizing
    const int n_longest = bt.n_real > 0 ? bt.n_real : bt.n_max;
    if (n_longest > enc_.posenc_rows) fail(ZV_ERR_ARG, "%d phonemes exceed the %d rows of the sinusoid table", n_longest, enc_.posenc_rows);
    const EncLayout lay = enc_layout(stage_arena(bt), bt);
    const Segs tk = bt.tokens(), fr = bt.frames_cap();       // (the regulator clamps and zero-fills by capacity, fitted or not)
    const EncPlan plan = enc_plan((int)E(), enc_.dur.V, dbg_layer.kind >= 0);
    const Segs tkm = plan.merged ? bt.tokens_merged() : tk;      // the per-token layers (linear, 1-tap conv, plain LayerNorm) see one dense segment
    const int Ed = (int)E(), H = hp.encoder_head, dk = Ed / H;
    const size_t n = bt.n_rows;
    const double nd = (double)n;
    const int Vp = lay.Vp;
    float *const x = lay.x, *const y = lay.y, *const qkv = lay.qkv, *const o = lay.o, *const f = lay.f, *const va = lay.va, *const vb = lay.vb;
    _Float16 *const hh = lay.hh;
    const bool tails = plan.tails;       // LayerNorm launches that carry tail work (kernels.h: launch_layernorm_tail)
    const EncoderTaps t = lay.t;

    ZV_LAUNCH("enc_embed", 8.0 * nd * Ed, 1.0 * nd * Ed,
              launch_embed(stream(), d_ids, d_puncts, enc_.wemb, hp.emb_dim, enc_.pemb, hp.punct_emb_dim, enc_.posenc, x, Ed, tk));
    if (dbg_layer.kind == ZV_LAYER_ENC_EMBED)
    {
        dbg_extract(x, Ed, Ed, n);
        return t;
    }
    const float temperature = (float)pow((double)dk, 0.5);               // src/fs2encoder.cpp:66
    const float inv_t = (float)(1.0 / temperature);                      // :107
    int layer_no = 0;
    for (const EncLayer &Ly : enc_.layers)
    {
        const bool dbg_here = dbg_layer.kind == 1 && dbg_layer.index == layer_no;
        // sub-block taps (the reference's tensor_dbg taps any node, src/utils.cpp:19-44): the attention sublayer alone
        // (ZV_LAYER_ENC_MHA: x -> y) and the conv feed-forward sublayer alone (ZV_LAYER_ENC_FFN: y -> x)
        const bool dbg_mha = dbg_layer.kind == ZV_LAYER_ENC_MHA && dbg_layer.index == layer_no;
        const bool dbg_ffn = dbg_layer.kind == ZV_LAYER_ENC_FFN && dbg_layer.index == layer_no;
        layer_no++;
        if (dbg_here || dbg_mha) dbg_inject(x, Ed, Ed, n);
        ZV_LAUNCH("enc_linear", 4.0 * (3.0 * Ed * Ed + 4.0 * nd * Ed), 6.0 * nd * Ed * Ed,
                  launch_linear(stream(), x, Ed, Ed, Ly.qkvW, Ly.qkvB, 3 * Ed, qkv, 3 * Ed, nullptr, tkm));
        ZV_LAUNCH("enc_attention", 16.0 * nd * Ed, 4.0 * nd * bt.n_max * Ed,
                  launch_attention(stream(), qkv, qkv + Ed, qkv + 2 * Ed, 3 * Ed, H, dk, inv_t, o, Ed, tk));
        ZV_LAUNCH("enc_linear", 4.0 * (1.0 * Ed * Ed + 2.0 * nd * Ed), 2.0 * nd * Ed * Ed,
                  launch_linear(stream(), o, Ed, Ed, Ly.fcW, Ly.fcB, Ed, f, Ed, nullptr, tkm));
        ZV_LAUNCH("enc_layernorm", 12.0 * nd * Ed, 8.0 * nd * Ed,
                  launch_add_layernorm(stream(), f, Ed, x, Ed, Ed, Ed, Ly.ln1w, Ly.ln1b, 1e-5f, y, Ed, tkm));
        if (dbg_mha)
        {
            dbg_extract(y, Ed, Ed, n);
            return t;
        }
        if (dbg_ffn) dbg_inject(y, Ed, Ed, n);
        {   // FFN: conv k9 + b -> relu (kept as f16 operand) -> conv k1 + b            (src/fs2encoder.cpp:190-214)
            ConvJob a = job(Ly.w1);
            a.x0 = y;
            a.eact = 1;
            a.oslope = 0.f;
            a.out_f16 = 1;
            a.out = hh;
            conv(&a, 1, tk, 1, "enc_conv", conv_bytes(nd, Ed, Ly.w1.Cout, Ly.w1.K, false), conv_flops(nd, Ed, Ly.w1.Cout, Ly.w1.K));
            ConvJob b = job(Ly.w2);
            b.x0 = hh;
            b.pro = PRO_RAW_F16;
            b.out = f;
            // (a 1-tap conv is per token: like the linear layers it takes the batch as one dense segment)
            conv(&b, 1, Ly.w2.K == 1 ? tkm : tk, 1, "enc_conv", conv_bytes(nd, Ly.w1.Cout, Ed, Ly.w2.K, false), conv_flops(nd, Ly.w1.Cout, Ed, Ly.w2.K));
        }
        // (the last layer's LayerNorm also adds the style vector: features = encoder output + style_embed, :550-552)
        if (tails && layer_no == (int)enc_.layers.size())
            ZV_LAUNCH("enc_layernorm", 12.0 * nd * Ed, 9.0 * nd * Ed,
                      launch_layernorm_tail(stream(), f, Ed, y, Ed, Ed, Ed, Ly.ln2w, Ly.ln2b, 1e-5f, x, Ed, tk, d_styles, Ed, nullptr, nullptr,
                                            nullptr, nullptr, 0, 0, nullptr, 0, nullptr));
        else
            ZV_LAUNCH("enc_layernorm", 12.0 * nd * Ed, 8.0 * nd * Ed,
                      launch_add_layernorm(stream(), f, Ed, y, Ed, Ed, Ed, Ly.ln2w, Ly.ln2b, 1e-5f, x, Ed, tkm));
        if (dbg_here || dbg_ffn)
        {
            dbg_extract(x, Ed, Ed, n);
            return t;
        }
    }
    // features = encoder output + style_embed                                             (:550-552)
    if (!(tails && !enc_.layers.empty()))
        ZV_LAUNCH("enc_add_style", 8.0 * nd * Ed, 1.0 * nd * Ed, launch_add_rowvec(stream(), x, Ed, Ed, d_styles, Ed, tk));

    int pred_no = 0;
    // VariancePredictor::graph (:386-440): conv + relu, LayerNorm, conv + relu, LayerNorm, linear.  `emb` (pitch / energy): the
    // prediction's bucket and x += embedding[bucket] (:442-474, 565-569) follow.  With `tails` the second LayerNorm's launch also
    // does the linear layer and the bucket / embedding step (5 + 1 launches -> 4).
    // ctl_field / pctl_field: the prosody control of the bucket step (kernels.h CTL_PITCH / CTL_ENERGY) and the per-phoneme one
    // (PCTL_PITCH / PCTL_ENERGY), used when bt.d_ctl / bt.d_pctl are set
    auto predictor = [&](const VarPred &v, float *out, const float *emb, int32_t *bucket, int ctl_field, int pctl_field) {
        const float *pctl = emb && bt.d_pctl ? bt.d_pctl + pctl_field : nullptr;
        const bool dbg_here = dbg_layer.kind == 3 && dbg_layer.index == pred_no && !dbg_layer.done;
        pred_no++;
        if (dbg_layer.done) return;
        if (dbg_here) dbg_inject(x, Ed, Ed, n);
        ConvJob a = job(v.c1);
        a.x0 = x;
        a.eact = 1;
        a.oslope = 0.f;
        a.out = va;
        conv(&a, 1, tk, 1, "enc_conv", conv_bytes(nd, Ed, v.V, 3, false), conv_flops(nd, Ed, v.V, 3));
        ZV_LAUNCH("enc_layernorm", 8.0 * nd * v.V, 8.0 * nd * v.V,
                  launch_add_layernorm(stream(), va, Vp, nullptr, 0, v.V, Vp, v.l1w, v.l1b, 1e-5f, vb, Vp, tkm));
        ConvJob b = job(v.c2);
        b.x0 = vb;
        b.pad = 1;                                              // literal 1 in the reference (:417)
        b.eact = 1;
        b.oslope = 0.f;
        b.out = va;
        conv(&b, 1, tk, 1, "enc_conv", conv_bytes(nd, v.V, v.V, 3, false), conv_flops(nd, v.V, v.V, 3));
        if (tails)
        {
            ZV_LAUNCH("enc_layernorm", 8.0 * nd * v.V + (emb ? 12.0 * nd * Ed : 0.0), 10.0 * nd * v.V,
                      launch_layernorm_tail(stream(), va, Vp, nullptr, 0, v.V, Vp, v.l2w, v.l2b, 1e-5f, vb, Vp, tk, nullptr, 0, v.lw, v.lb, out,
                                            emb, (int)hp.encoder_ve_n_bins, Ed, x, Ed, bucket, emb ? bt.d_ctl : nullptr, ctl_field, pctl));
            return;
        }
        ZV_LAUNCH("enc_layernorm", 8.0 * nd * v.V, 8.0 * nd * v.V,
                  launch_add_layernorm(stream(), va, Vp, nullptr, 0, v.V, Vp, v.l2w, v.l2b, 1e-5f, vb, Vp, tkm));
        ZV_LAUNCH("enc_rowdot", 4.0 * nd * v.V, 2.0 * nd * v.V, launch_rowdot(stream(), vb, Vp, v.V, v.lw, v.lb, out, tk));
        if (dbg_here) dbg_extract(out, 1, 1, n);
        if (emb && !dbg_layer.done)
            ZV_LAUNCH("enc_bucket_embed", 12.0 * nd * Ed, 1.0 * nd * Ed,
                      launch_bucket_embed_add(stream(), out, hp.encoder_ve_n_bins, emb, Ed, x, Ed, bucket, tk, bt.d_ctl, ctl_field, pctl));
    };
    predictor(enc_.dur, t.logdur, nullptr, nullptr, 0, 0);
    predictor(enc_.pitch, t.pitch, enc_.pitch_emb, t.pitch_bucket, CTL_PITCH, PCTL_PITCH);
    if (dbg_layer.done) return t;
    predictor(enc_.energy, t.energy, enc_.energy_emb, t.energy_bucket, CTL_ENERGY, PCTL_ENERGY);      // sees the pitch-augmented features (:569-572)
    if (dbg_layer.done) return t;
    // target durations: the integer durations that sum to each utterance's target become forced frames in the phoneme control rows,
    // which the regulator below reads as it reads a caller's (kernels.h launch_fit_durations)
    if (bt.has_targets)
    {
        if (!bt.d_ctl || !bt.d_pctl) fail(ZV_ERR_ARG, "a batch with target durations needs its control rows");
        ZV_LAUNCH("enc_fit_durations", 24.0 * nd, 0.0, launch_fit_durations(stream(), t.logdur, bt.d_ctl, bt.d_pctl, tk, fr));
    }
    ZV_LAUNCH("enc_length_regulator", 4.0 * (nd + (double)bt.t_rows) * Ed, 0.0,
              launch_length_regulator(stream(), x, Ed, t.logdur, Ed, d_hidden, Ed, t.cum, d_nframes, tk, fr, bt.d_ctl, bt.d_pctl));
    // fitted: the frame table of everything downstream, from the counts the regulator has just stored
    if (bt.d_frm_live)
        ZV_LAUNCH("enc_live_frames", 36.0 * bt.nseg, 0.0, launch_live_frames(stream(), d_nframes, bt.d_frm_live, fr));
    // run-shortened decoding: the decoder's run table, from the same counts
    if (bt.d_dec_runs)
        ZV_LAUNCH("enc_dec_runs", 36.0 * bt.nseg, 0.0, launch_dec_runs(stream(), d_nframes, bt.d_dec_runs, fr, dec_reach_frames(), dec_plan(bt).pack));
    return t;
}

// the LayerNorm of FFT block index / 2's attention (even index) / feed-forward (odd) sublayer, launched as the encoder launches
// it but without the residual, on n given rows; an index past the encoder leaves dbg_layer.done false
void Model::debug_layernorm(int index, uint32_t n)
{
    const int l = index >> 1, Ed = (int)E();
    if (index < 0 || l >= (int)enc_.layers.size()) return;
    const EncLayer &Ly = enc_.layers[l];
    float *d = (float *)io_scratch(2 * (size_t)n * Ed * 4), *y = d + (size_t)n * Ed;
    dbg_inject(d, Ed, Ed, n);
    ZV_HIP(launch_add_layernorm(stream(), d, Ed, nullptr, 0, Ed, Ed, (index & 1) ? Ly.ln2w : Ly.ln1w, (index & 1) ? Ly.ln2b : Ly.ln1b,
                                1e-5f, y, Ed, segs_single((int)n)));
    dbg_extract(y, Ed, Ed, n);
}

}  // namespace zv
