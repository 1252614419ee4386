// zerovox_facade.cpp — ZeroVOX:: classes of csrc/zerovox.h implemented over the C-ABI.
#include "zerovox.h"

#include <cstdlib>
#include <cstring>
#include <vector>

#include "bands.h"         // BANDS_DEFAULT, BANDS_MAX, BANDS_DEFAULT_EDGES
#include "common.h"

namespace ZeroVOX
{

static void chk(zv_status st)
{
    if (st != ZV_OK) throw zv::Error(st, zv_last_error());
}

static void expect(bool ok, const char *what)
{
    if (!ok) throw zv::Error(ZV_ERR_SHAPE, std::string("constructor argument does not match the GGUF file: ") + what);
}

FS2Encoder::FS2Encoder(weights_t &ctx_w, backend_t backend, uint32_t max_n_phonemes_, uint32_t embed_dim,
                       uint32_t punct_embed_dim, uint32_t encoder_layer, uint32_t encoder_head, uint32_t conv_filter_size,
                       uint32_t conv_kernel_size[2], uint32_t vp_kernel_size, uint32_t ve_n_bins, uint32_t max_seq_len_)
    : model(&ctx_w), max_n_phonemes(max_n_phonemes_), max_seq_len(max_seq_len_)
{
    (void)backend;
    zv_hparams hp;
    chk(zv_model_get_hparams(model, &hp));
    expect(hp.emb_dim == embed_dim && hp.punct_emb_dim == punct_embed_dim, "embed_dim / punct_embed_dim");
    expect(hp.encoder_layer == encoder_layer && hp.encoder_head == encoder_head, "encoder_layer / encoder_head");
    expect(hp.conv_filter_size == conv_filter_size, "conv_filter_size");
    expect(hp.conv_kernel_size[0] == conv_kernel_size[0] && hp.conv_kernel_size[1] == conv_kernel_size[1], "conv_kernel_size");
    expect(hp.encoder_vp_kernel_size == vp_kernel_size && hp.encoder_ve_n_bins == ve_n_bins, "vp_kernel_size / ve_n_bins");
    if (max_n_phonemes == 0 || max_seq_len == 0) throw zv::Error(ZV_ERR_ARG, "max_n_phonemes and max_seq_len must be > 0");
    chk(zv_model_reserve(model, max_n_phonemes, max_seq_len));
}

uint32_t FS2Encoder::eval(const int32_t *src_seq_data, const int32_t *puncts_data, const float *style_embed_data,
                          uint32_t num_phonemes, float *x)
{
    // The reference graph always encodes max_n_phonemes tokens (no mask, src/fs2encoder.cpp:103-110,598-600: all
    // max_n_phonemes ids are uploaded) and the regulator walks the first num_phonemes of them (:622).
    if (num_phonemes > max_n_phonemes)
        throw zv::Error(ZV_ERR_ARG, "FS2Encoder::eval: num_phonemes exceeds max_n_phonemes");
    uint32_t n_frames = 0;
    chk(zv_encode_taps(model, src_seq_data, puncts_data, style_embed_data, max_n_phonemes, num_phonemes, max_seq_len, x,
                       &n_frames, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    return n_frames;
}

StyleTTSDecoder::StyleTTSDecoder(weights_t &ctx_w, backend_t backend, uint32_t max_seq_len_, uint32_t dim_in,
                                 uint32_t style_dim, uint32_t residual_dim, uint32_t dim_out)
    : model(&ctx_w), max_seq_len(max_seq_len_)
{
    (void)backend;
    (void)residual_dim;        // taken from the asr_res tensor shape; the reference hard-codes 64
    zv_hparams hp;
    chk(zv_model_get_hparams(model, &hp));
    expect(hp.emb_dim + hp.punct_emb_dim == dim_in && dim_in == style_dim, "dim_in / style_dim");
    expect(hp.audio_num_mels == dim_out, "dim_out");
    if (max_seq_len == 0) throw zv::Error(ZV_ERR_ARG, "max_seq_len must be > 0");
    chk(zv_model_reserve(model, 1, max_seq_len));
}

void StyleTTSDecoder::eval(const float *enc_seq_data, const float *spk_emb_data, float *mel)
{
    chk(zv_decode(model, enc_seq_data, spk_emb_data, max_seq_len, mel));
}

HiFiGAN::HiFiGAN(weights_t &ctx_w, backend_t backend, uint32_t max_seq_len_, uint32_t in_channels, uint32_t hop_size,
                 uint32_t kernel_size, int num_upsamples, const int *upsample_scales, int num_resblocks,
                 int num_resblock_dilations, const int64_t *resblock_dilations)
    : model(&ctx_w), max_seq_len(max_seq_len_)
{
    (void)backend;
    zv_hparams hp;
    chk(zv_model_get_hparams(model, &hp));
    expect(hp.audio_num_mels == in_channels && hp.audio_hop_size == hop_size, "in_channels / hop_size");
    expect(kernel_size == 7, "kernel_size (the stored input/output convs are k7)");
    expect((int)hp.voc_num_upsamples == num_upsamples && (int)hp.voc_num_resblocks == num_resblocks, "num_upsamples / num_resblocks");
    for (int i = 0; i < num_upsamples; i++) expect((int)hp.voc_upsample_scales[i] == upsample_scales[i], "upsample_scales");
    expect(num_resblock_dilations == 3, "num_resblock_dilations");
    for (int j = 0; j < num_resblocks; j++)
        expect(resblock_dilations[j * 3] == 1 && resblock_dilations[j * 3 + 1] == 3 && resblock_dilations[j * 3 + 2] == 5, "resblock_dilations {1,3,5}");
    if (max_seq_len == 0) throw zv::Error(ZV_ERR_ARG, "max_seq_len must be > 0");
    chk(zv_model_reserve(model, 1, max_seq_len));
}

void HiFiGAN::eval(const float *mel, float *wav)
{
    chk(zv_vocode(model, mel, max_seq_len, wav));
}

void HiFiGAN::eval_batch(uint32_t n, const float *const *mels, const uint32_t *T, float *const *wavs)
{
    chk(zv_vocode_batch(model, n, mels, T, wavs));
}

void HiFiGAN::analyze(const float *wav, float *mel)
{
    zv_mel q{};
    q.pad = 1;
    q.log = 1;
    chk(zv_mel_wave(model, wav, max_seq_len, &q, mel));
}

zv_loudness_result HiFiGAN::loudness(const float *wav, const zv_loudness *ask, float *out)
{
    zv_loudness_result res{};
    chk(zv_loudness_wave(model, wav, max_seq_len, max_seq_len, ask, &res, out));
    return res;
}

zv_limit_result HiFiGAN::limit(const float *wav, const zv_limiter *ask, float *out)
{
    zv_limit_result res{};
    chk(zv_limit_wave(model, wav, max_seq_len, max_seq_len, ask, &res, out));
    return res;
}

zv_resample_result HiFiGAN::resample(const float *wav, const zv_resample *ask, float *out, int16_t *pcm)
{
    zv_resample_result res{};
    zv_hparams hp;
    chk(zv_model_get_hparams(model, &hp));
    chk(zv_resample_wave(model, wav, (uint64_t)max_seq_len * hp.audio_hop_size, ask, &res, out, pcm));
    return res;
}

// ---------------------------------------------------------------------------------------------------

ZeroVOXModel::ZeroVOXModel(const std::string &fname)
    : model(nullptr), encoder(nullptr), decoder(nullptr), meldec(nullptr), hidden_state(nullptr), mel(nullptr), wav(nullptr), n_frames(0),
      prosody{1.0f, 1.0f, 0.0f, 1.0f, 0.0f}, has_prosody(false)
{
    int device = 0;
    if (const char *e = getenv("ZEROVOX_DEVICE")) device = atoi(e);
    chk(zv_model_load(fname.c_str(), device, &model));
    try
    {
        chk(zv_model_get_hparams(model, &hparams));
        const uint32_t emb_size = hparams.emb_dim + hparams.punct_emb_dim;
        hidden_state = new float[(size_t)hparams.max_seq_len * emb_size];
        mel = new float[(size_t)hparams.max_seq_len * hparams.audio_num_mels];
        wav = new float[(size_t)hparams.max_seq_len * hparams.audio_hop_size];
        encoder = new FS2Encoder(*model, model, MAX_N_PHONEMES, hparams.emb_dim, hparams.punct_emb_dim, hparams.encoder_layer,
                                 hparams.encoder_head, hparams.conv_filter_size, hparams.conv_kernel_size,
                                 hparams.encoder_vp_kernel_size, hparams.encoder_ve_n_bins, hparams.max_seq_len);
        decoder = new StyleTTSDecoder(*model, model, hparams.max_seq_len, emb_size, emb_size, 64, hparams.audio_num_mels);
        int scales[8];
        for (uint32_t i = 0; i < hparams.voc_num_upsamples; i++) scales[i] = (int)hparams.voc_upsample_scales[i];
        std::vector<int64_t> dil;
        for (uint32_t j = 0; j < hparams.voc_num_resblocks; j++) { dil.push_back(1); dil.push_back(3); dil.push_back(5); }
        meldec = new HiFiGAN(*model, model, hparams.max_seq_len, hparams.audio_num_mels, hparams.audio_hop_size, 7,
                             (int)hparams.voc_num_upsamples, scales, (int)hparams.voc_num_resblocks, 3, dil.data());
    }
    catch (...)
    {
        release();
        throw;
    }
}

ZeroVOXModel::~ZeroVOXModel() { release(); }

void ZeroVOXModel::release()
{
    delete encoder;
    delete decoder;
    delete meldec;
    delete[] hidden_state;
    delete[] mel;
    delete[] wav;
    encoder = nullptr; decoder = nullptr; meldec = nullptr;
    hidden_state = mel = wav = nullptr;
    if (model) zv_model_free(model);
    model = nullptr;
}

void ZeroVOXModel::set_prosody(const zv_prosody &p)
{
    prosody = p;
    has_prosody = true;
}

void ZeroVOXModel::set_phoneme_controls(const zv_phoneme_controls *p, uint32_t n)
{
    auto take = [n](auto *src, auto &dst) {
        if (src) dst.assign(src, src + n);
        else dst.clear();
    };
    has_phonemes = p != nullptr;
    pc_n = p ? n : 0;
    take(p ? p->duration_frames : nullptr, pc_frames);
    take(p ? p->duration_scale : nullptr, pc_scale);
    take(p ? p->pitch_shift : nullptr, pc_pitch);
    take(p ? p->energy_shift : nullptr, pc_energy);
    record_durations = true;
}

void ZeroVOXModel::set_pitch(bool frames, bool phonemes, const zv_pitch *params)
{
    pitch_frames = frames;
    pitch_phonemes = phonemes;
    pitch_params = params ? *params : zv_pitch{nullptr, nullptr, 0, 0, 0, 0.0f};
    pitch_params.frames = nullptr;
    pitch_params.phonemes = nullptr;
}

void ZeroVOXModel::set_bands(bool frames, bool phonemes, uint32_t n_bands, const uint32_t *edges)
{
    band_frames = frames;
    band_phonemes = phonemes;
    band_count = n_bands;
    // (a count the library will refuse copies nothing: eval() reports it)
    if (edges && n_bands <= zv::BANDS_MAX) band_edges.assign(edges, edges + (n_bands ? n_bands : zv::BANDS_DEFAULT) + 1);
    else band_edges.clear();
}

std::vector<uint32_t> ZeroVOXModel::get_band_edges() const
{
    if (!band_edges.empty()) return band_edges;
    return std::vector<uint32_t>(zv::BANDS_DEFAULT_EDGES, zv::BANDS_DEFAULT_EDGES + zv::BANDS_DEFAULT + 1);
}

void ZeroVOXModel::set_filter(const float *taps, uint32_t n_taps)
{
    has_filter = taps != nullptr;
    filter_n = n_taps;
    // (a count the library will refuse copies one tap: eval() reports it)
    if (taps) filter_taps.assign(taps, taps + (n_taps >= 1 && n_taps <= 511 ? n_taps : 1));
    else filter_taps.clear();
}

void ZeroVOXModel::set_envelope(const zv_envelope *e, uint32_t n)
{
    has_envelope = e != nullptr;
    env_gain_set = e && e->phoneme_gain;
    if (env_gain_set) env_gain.assign(e->phoneme_gain, e->phoneme_gain + n);
    else env_gain.clear();
    envelope = e ? *e : zv_envelope{nullptr, 0, 0, 0};
    envelope.phoneme_gain = nullptr;          // the gains live in env_gain
}

zv_alignment ZeroVOXModel::align(const float *a, uint32_t Ta, const float *b, uint32_t Tb, uint32_t M, const zv_align *params, int32_t *map_a,
                                 int32_t *map_b)
{
    const zv_align q{};
    zv_alignment out{};
    chk(zv_mel_align(model, a, Ta, b, Tb, M, params ? params : &q, &out, map_a, map_b));
    return out;
}

zv_loudness_result ZeroVOXModel::loudness(const float *wav, uint32_t T, uint32_t n_frames, const zv_loudness *ask, float *out)
{
    zv_loudness_result res{};
    chk(zv_loudness_wave(model, wav, T, n_frames, ask, &res, out));
    return res;
}

zv_limit_result ZeroVOXModel::limit(const float *wav, uint32_t T, uint32_t n_frames, const zv_limiter *ask, float *out)
{
    zv_limit_result res{};
    chk(zv_limit_wave(model, wav, T, n_frames, ask, &res, out));
    return res;
}

zv_resample_result ZeroVOXModel::resample(const float *wav, uint64_t S_in, const zv_resample *ask, float *out, int16_t *pcm)
{
    zv_resample_result res{};
    chk(zv_resample_wave(model, wav, S_in, ask, &res, out, pcm));
    return res;
}

void ZeroVOXModel::set_time_like(const float *ref_wav, size_t n_samples)
{
    if (ref_wav) like_wav.assign(ref_wav, ref_wav + n_samples);
    else like_wav.clear();
}

void ZeroVOXModel::eval(const int32_t *src_seq, const int32_t *puncts, const float *style_embed, uint32_t num_phonemes)
{
    if (!like_wav.empty())
    {
        // the two runs of set_time_like: this function again, with the reference put aside
        const size_t hop = hparams.audio_hop_size, Tb = like_wav.size() / hop;
        if (!pc_frames.empty() || target_frames) throw zv::Error(ZV_ERR_ARG, "set_time_like: the reference gives the timing, duration_frames and a target exclude it");
        if (Tb < 1 || Tb > hparams.max_seq_len)
            throw zv::Error(ZV_ERR_ARG, "set_time_like: the reference holds " + std::to_string(Tb) + " frames, 1 .. max_seq_len = " +
                                            std::to_string(hparams.max_seq_len) + " are needed");
        std::vector<float> ref;
        ref.swap(like_wav);
        const bool was_fitted = fitted, had_phonemes = has_phonemes, recorded = record_durations;
        auto restore = [&] {
            like_wav.swap(ref);
            fitted = was_fitted, has_phonemes = had_phonemes, record_durations = recorded;
            pc_frames.clear();
            if (!had_phonemes) pc_n = 0;
        };
        try
        {
            fitted = true;
            record_durations = true;
            eval(src_seq, puncts, style_embed, num_phonemes);
            const uint32_t Ta = n_frames, M = hparams.audio_num_mels;
            if (!Ta) throw zv::Error(ZV_ERR_ARG, "set_time_like: the model's own synthesis has no frames");
            std::vector<float> rows_a((size_t)Ta * M), rows_b(Tb * M);
            zv_mel mq{};
            mq.log = 1;
            const float *wavs[2] = {wav, ref.data()};
            const uint32_t Ts[2] = {Ta, (uint32_t)Tb};
            float *outs[2] = {rows_a.data(), rows_b.data()};
            chk(zv_mel_wave_batch(model, 2, wavs, Ts, &mq, outs));
            const zv_align aq{0.0f, 1};
            std::vector<int32_t> map_a(Ta), frames(num_phonemes);
            alignment = align(rows_a.data(), Ta, rows_b.data(), (uint32_t)Tb, M, &aq, map_a.data(), nullptr);
            chk(zv_align_durations(num_phonemes, durations.data(), Ta, map_a.data(), (uint32_t)Tb, frames.data()));
            pc_frames = frames;
            has_phonemes = true;
            pc_n = num_phonemes;
            eval(src_seq, puncts, style_embed, num_phonemes);
        }
        catch (...)
        {
            restore();
            throw;
        }
        restore();
        return;
    }
    if (has_envelope && env_gain_set && env_gain.size() != num_phonemes)
        throw zv::Error(ZV_ERR_ARG, "set_envelope: gains for " + std::to_string(env_gain.size()) + " phonemes, eval() has " +
                                        std::to_string(num_phonemes));
    // (set_phoneme_controls also turns the timings on, so every call that carries controls goes to a form that takes them)
    if (has_phonemes && pc_n != num_phonemes)
        throw zv::Error(ZV_ERR_ARG, "set_phoneme_controls: controls for " + std::to_string(pc_n) + " phonemes, eval() has " +
                                        std::to_string(num_phonemes));
    frame_levels.assign(contour_frames ? hparams.max_seq_len : 0, zv_frame_level{0.0f, 0.0f});
    phoneme_levels.assign(contour_phonemes ? num_phonemes : 0, zv_frame_level{0.0f, 0.0f});
    pitch_frame_rows.assign(pitch_frames ? hparams.max_seq_len : 0, zv_pitch_frame{0.0f, 0.0f});
    pitch_phoneme_rows.assign(pitch_phonemes ? num_phonemes : 0, zv_pitch_phoneme{0.0f, 0.0f});
    const size_t band_w = band_count && band_count <= zv::BANDS_MAX ? band_count : zv::BANDS_DEFAULT;
    band_frame_rows.assign(band_frames ? (size_t)hparams.max_seq_len * band_w : 0, 0.0f);
    band_phoneme_rows.assign(band_phonemes ? (size_t)num_phonemes * band_w : 0, 0.0f);
    if (record_durations) durations.assign(num_phonemes, 0);

    // what the setters asked for, each as the entry points take it; which of them a form takes is its place on the ladder
    auto ptr = [](auto &v) { return v.empty() ? nullptr : v.data(); };
    const zv_prosody *pr = has_prosody ? &prosody : nullptr;
    const zv_phoneme_controls pc = {ptr(pc_frames), ptr(pc_scale), ptr(pc_pitch), ptr(pc_energy)};
    const zv_phoneme_controls *pcp = has_phonemes ? &pc : nullptr;
    int32_t *dur = record_durations ? durations.data() : nullptr;
    const int fit = fitted ? 1 : 0;
    const zv_volume *vol = has_volume ? &volume : nullptr;
    zv_level *lev = has_volume ? &level : nullptr;
    const zv_envelope env = {env_gain_set ? env_gain.data() : nullptr, envelope.ramp_frames, envelope.fade_in_samples,
                             envelope.fade_out_samples};
    const zv_envelope *envp = has_envelope ? &env : nullptr;
    const zv_contour ctr = {contour_frames ? frame_levels.data() : nullptr, contour_phonemes ? phoneme_levels.data() : nullptr};
    const zv_pitch pit = {pitch_frames ? pitch_frame_rows.data() : nullptr, pitch_phonemes ? pitch_phoneme_rows.data() : nullptr,
                          pitch_params.min_lag, pitch_params.max_lag, pitch_params.window, pitch_params.voiced_threshold};
    const zv_bands bnd = {band_frames ? band_frame_rows.data() : nullptr, band_phonemes ? band_phoneme_rows.data() : nullptr, band_count,
                          ptr(band_edges)};
    const zv_filter flt = {filter_taps.data(), filter_n};
    // a synthesize form on the whole utterance (N = num_phonemes), and an encoder form ahead of the stage objects (N = MAX_N_PHONEMES)
    auto synthesize = [&](auto form, auto... more) {
        chk(form(model, src_seq, puncts, style_embed, num_phonemes, hparams.max_seq_len, wav, &n_frames, more...));
    };
    auto stages = [&](auto form, auto... more) {
        chk(form(model, src_seq, puncts, style_embed, MAX_N_PHONEMES, num_phonemes, hparams.max_seq_len, hidden_state, &n_frames, nullptr,
                 nullptr, nullptr, nullptr, nullptr, nullptr, more...));
        decoder->eval(hidden_state, style_embed, mel);
        meldec->eval(mel, wav);
    };
    const bool one_pass = fitted || num_phonemes != (uint32_t)MAX_N_PHONEMES;      // the stage objects are pinned to MAX_N_PHONEMES

    // the waveform stages work on the finished waveform of the one-pass chain: the highest form asked for, never below _contour
    if (has_filter)
        synthesize(zv_synthesize_filter, pr, pcp, dur, target_frames, fit, vol, lev, envp, &ctr, &pit, &bnd, &flt);
    else if (band_frames || band_phonemes)
        synthesize(zv_synthesize_bands, pr, pcp, dur, target_frames, fit, vol, lev, envp, &ctr, &pit, &bnd);
    else if (pitch_frames || pitch_phonemes)
        synthesize(zv_synthesize_pitch, pr, pcp, dur, target_frames, fit, vol, lev, envp, &ctr, &pit);
    else if (has_volume || has_envelope || contour_frames || contour_phonemes)
        synthesize(zv_synthesize_contour, pr, pcp, dur, target_frames, fit, vol, lev, envp, &ctr);
    else if (target_frames)
    {
        if (one_pass) synthesize(zv_synthesize_target, pr, pcp, dur, target_frames, fit);
        else stages(zv_encode_taps_target, pr, pcp, dur, target_frames);
    }
    else if (fitted)
        synthesize(zv_synthesize_fitted, pr, pcp, dur);
    else if (record_durations)
    {
        if (one_pass) synthesize(zv_synthesize_phonemes, pr, pcp, dur);
        else stages(zv_encode_taps_phonemes, pr, pcp, dur);
    }
    else if (one_pass)
        synthesize(zv_synthesize_prosody, pr);
    else if (pr)
        stages(zv_encode_taps_prosody, pr);
    else
    {
        // the reference's own sequence of stage calls
        n_frames = encoder->eval(src_seq, puncts, style_embed, num_phonemes, hidden_state);
        decoder->eval(hidden_state, style_embed, mel);
        meldec->eval(mel, wav);
    }
}

void ZeroVOXModel::eval(void)
{
    // The reference hard-codes one utterance here (src/zerovox.cpp:204-314: 120 phoneme / punctuation ids of a German
    // sentence and a 528-float style vector from its speaker encoder); the same data drives this entry point
    // (zv_demo_utterance).  A checkpoint whose style width differs from 528 gets the first min(E, 528) values, zeros behind.
    const int32_t *ids = nullptr, *puncts = nullptr;
    const float *sty = nullptr;
    uint32_t n = 0, ns = 0;
    zv_demo_utterance(&ids, &puncts, &sty, &n, &ns);
    std::vector<float> style(hparams.emb_dim + hparams.punct_emb_dim, 0.0f);
    for (size_t i = 0; i < style.size() && i < ns; i++) style[i] = sty[i];
    eval(ids, puncts, style.data(), n);
}

bool ZeroVOXModel::write_wav_file(const std::string &fname)
{
    // like the reference, all max_seq_len * hop_size samples are written (src/zerovox.cpp:369)
    return zv_write_wav(fname.c_str(), wav, (size_t)hparams.max_seq_len * hparams.audio_hop_size, hparams.audio_sampling_rate) == ZV_OK;
}

}  // namespace ZeroVOX
