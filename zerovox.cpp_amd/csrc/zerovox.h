// zerovox.h — host-side mirror of the reference's stage API (namespace ZeroVOX), over the C-ABI.
//
// Same class names, constructor argument positions and eval() signatures as the reference's
// src/zerovox.h:173-223 (FS2Encoder), :310-360 (StyleTTSDecoder), :362-402 (HiFiGAN), :405-430
// (ZeroVOXModel), so that a caller written like the reference's src/zerovox.cpp compiles against this
// header unchanged apart from the two ggml handle types, which cannot travel:
//
//     reference                       here
//     ggml_context  &ctx_w      ->    ZeroVOX::weights_t &ctx_w     (the loaded model: weights in HBM)
//     ggml_backend_t backend    ->    ZeroVOX::backend_t  backend   (the device the model lives on)
//
// With -DZEROVOX_GGML_COMPAT_NAMES the two names are also typedef'ed as ggml_context / ggml_backend_t.
//
// Behavioural notes: the geometry arguments are checked against what the GGUF file
// says (a mismatch throws instead of silently building a different graph); eval() is synchronous;
// errors are std::runtime_error (zv::Error) — never exit() or abort().
#pragma once

#include <cinttypes>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zerovox_amd.h"

namespace ZeroVOX
{

// the GGUF KV names, verbatim from the file format contract (reference src/zerovox.h:17-33)
#define HPARAM_MAX_SEQ_LEN            "zerovox-resnet-fs2-styletts.max_seq_len"
#define HPARAM_EMB_DIM                "zerovox-resnet-fs2-styletts.emb_dim"
#define HPARAM_PUNCT_EMB_DIM          "zerovox-resnet-fs2-styletts.punct_emb_dim"
#define HPARAM_DECODER_N_HEAD         "zerovox-resnet-fs2-styletts.decoder.n_head"
#define HPARAM_CONV_FILTER_SIZE       "zerovox-resnet-fs2-styletts.decoder.conv_filter_size"
#define HPARAM_CONV_KERNEL_SIZE_0     "zerovox-resnet-fs2-styletts.decoder.conv_kernel_size.0"
#define HPARAM_CONV_KERNEL_SIZE_1     "zerovox-resnet-fs2-styletts.decoder.conv_kernel_size.1"
#define HPARAM_ENCODER_LAYER          "zerovox-resnet-fs2-styletts.encoder.layer"
#define HPARAM_ENCODER_HEAD           "zerovox-resnet-fs2-styletts.encoder.head"
#define HPARAM_ENCODER_VP_FILTER_SIZE "zerovox-resnet-fs2-styletts.encoder.vp_filter_size"
#define HPARAM_ENCODER_VP_KERNEL_SIZE "zerovox-resnet-fs2-styletts.encoder.vp_kernel_size"
#define HPARAM_ENCODER_VE_N_BINS      "zerovox-resnet-fs2-styletts.encoder.ve_n_bins"
#define HPARAM_AUDIO_NUM_MELS         "zerovox-resnet-fs2-styletts.audio.num_mels"
#define HPARAM_AUDIO_HOP_SIZE         "zerovox-resnet-fs2-styletts.audio.hop_size"
#define HPARAM_AUDIO_SAMPLING_RATE    "zerovox-resnet-fs2-styletts.audio.sampling_rate"

const int NUM_PHONEMES   = 154;
const int NUM_PUNCTS     =   6;
const int MAX_N_PHONEMES = 120;

typedef zv_hparams zerovox_hparams;      // superset of the reference struct (src/zerovox.h:39-58)

typedef zv_model  weights_t;
typedef zv_model *backend_t;

class FS2Encoder
{
  public:
    FS2Encoder(weights_t &ctx_w, backend_t backend, uint32_t max_n_phonemes, uint32_t embed_dim,
               uint32_t punct_embed_dim, uint32_t encoder_layer, uint32_t encoder_head, uint32_t conv_filter_size,
               uint32_t conv_kernel_size[2], uint32_t vp_kernel_size, uint32_t ve_n_bins, uint32_t max_seq_len);
    ~FS2Encoder() = default;

    // x must hold max_seq_len * (embed_dim + punct_embed_dim) floats; returns the regulator's frame count.
    // src_seq_data / puncts_data must hold max_n_phonemes entries, all of which are encoded (no mask).
    uint32_t eval(const int32_t *src_seq_data, const int32_t *puncts_data, const float *style_embed_data,
                  uint32_t num_phonemes, float *x);

  private:
    zv_model *model;
    uint32_t  max_n_phonemes, max_seq_len;
};

class StyleTTSDecoder
{
  public:
    StyleTTSDecoder(weights_t &ctx_w, backend_t backend, uint32_t max_seq_len, uint32_t dim_in, uint32_t style_dim,
                    uint32_t residual_dim, uint32_t dim_out);
    ~StyleTTSDecoder() = default;

    void eval(const float *enc_seq_data, const float *spk_emb_data, float *mel);

  private:
    zv_model *model;
    uint32_t  max_seq_len;
};

class HiFiGAN
{
  public:
    HiFiGAN(weights_t &ctx_w, backend_t backend, uint32_t max_seq_len, uint32_t in_channels, uint32_t hop_size,
            uint32_t kernel_size, int num_upsamples, const int *upsample_scales, int num_resblocks,
            int num_resblock_dilations, const int64_t *resblock_dilations);

    void eval(const float *mel, float *wav);
    // (not in the reference) n utterances in one call, mels[u] [T[u]][in_channels] -> wavs[u] [T[u] * hop_size]: zv_vocode_batch, every
    // waveform the bits of a single vocode of that mel
    void eval_batch(uint32_t n, const float *const *mels, const uint32_t *T, float *const *wavs);
    // (not in the reference) the way back: wav [max_seq_len * hop_size] -> mel [max_seq_len][in_channels], zv_mel_wave with natural-log
    // Slaney mels over 0 .. Nyquist, reflect padding, centre 0 and the default floor — the domain eval reads
    void analyze(const float *wav, float *mel);
    // (not in the reference) the delivery meter: zv_loudness_wave over wav [max_seq_len * hop_size] — BS.1770 integrated loudness (LUFS),
    // true peak (dBTP) and, where out [max_seq_len * hop_size] is given, the waveform under ask's gain, target and ceiling (nullptr: the
    // identity, a meter)
    zv_loudness_result loudness(const float *wav, const zv_loudness *ask = nullptr, float *out = nullptr);
    // (not in the reference) the stage behind it: zv_limit_wave over wav [max_seq_len * hop_size] — the look-ahead peak limiter; out
    // [max_seq_len * hop_size] is required; ask nullptr: gain 1, ceiling 1, the default windows.
    zv_limit_result limit(const float *wav, const zv_limiter *ask, float *out);
    // (not in the reference) the step behind that: zv_resample_wave over wav [max_seq_len * hop_size] — another sample rate, as f32
    // (out), as PCM16 (pcm) or both, each [zv_resample_count(max_seq_len * hop_size, L, M)]; at least one of the two.
    zv_resample_result resample(const float *wav, const zv_resample *ask, float *out, int16_t *pcm);

  private:
    zv_model *model;
    uint32_t  max_seq_len;
};

class ZeroVOXModel
{
  public:
    ZeroVOXModel(const std::string &fname);
    ~ZeroVOXModel();

    // the reference synthesises a hard-coded sentence (src/zerovox.cpp:198-335); same here, plus an
    // overload that takes the utterance
    void eval(void);
    void eval(const int32_t *src_seq, const int32_t *puncts, const float *style_embed, uint32_t num_phonemes);

    bool write_wav_file(const std::string &fname);

    // prosody controls (include/zerovox_amd.h zv_prosody: speaking rate, pitch, energy) for the eval() calls that follow, until
    // set again; the identity {1, 1, 0, 1, 0} gives the uncontrolled bits.  Values are checked when eval() runs (ZV_ERR_ARG).
    void set_prosody(const zv_prosody &p);
    // per-phoneme controls (include/zerovox_amd.h zv_phoneme_controls) of the next eval() calls' utterance of n phonemes, copied; any
    // pointer may be NULL, p == NULL clears the controls.  From the first call on, eval() also records the phoneme timings
    // (get_durations()).  n must equal eval()'s num_phonemes (ZV_ERR_ARG otherwise).
    void set_phoneme_controls(const zv_phoneme_controls *p, uint32_t n);
    // the phoneme timings of the last eval() after set_phoneme_controls(): frames of each phoneme in the hidden state / waveform
    const std::vector<int32_t> &get_durations() const { return durations; }
    // fitted synthesis (include/zerovox_amd.h zv_synthesize_fitted) for the eval() calls that follow: max_seq_len stays the
    // capacity, the utterance is decoded and vocoded as the get_num_frames() frames the length regulator fills, the rest of
    // get_wav() is zero.  Prosody, per-phoneme controls and timings work as without it.
    void set_fitted(bool on) { fitted = on; }
    // target durations (include/zerovox_amd.h "target durations") for the eval() calls that follow: the utterance's durations are
    // fitted to sum to exactly `frames` (<= max_seq_len, ZV_ERR_ARG otherwise; 0 = none).  Works with everything above.
    void set_target_frames(uint32_t frames) { target_frames = frames; }
    // volume controls (include/zerovox_amd.h "volume controls") for the eval() calls that follow: the waveform is measured and scaled
    // on the device (gain, loudness target, peak ceiling; the identity {1, 0, 0} only meters) and get_level() holds the speech's
    // rms and peak before the gain and the gain applied.  Works with everything above; values are checked when eval() runs.
    void set_volume(const zv_volume &v) { volume = v; has_volume = true; }
    const zv_level &get_level() const { return level; }
    // amplitude envelope (include/zerovox_amd.h "amplitude envelope") for the eval() calls that follow: per-phoneme gains (copied:
    // e->phoneme_gain is [n] or null; n must be eval()'s phoneme count), cross-fade half-width and the two fades, applied on the
    // device ahead of the volume controls.  nullptr: none.  Works with everything above; values are checked when eval() runs.
    void set_envelope(const zv_envelope *e, uint32_t n);
    // level contour (include/zerovox_amd.h "level contour") for the eval() calls that follow: the level and peak of every frame of the
    // capacity and / or of every phoneme, metered on the device on the waveform get_wav() holds (behind envelope and volume).  A
    // meter: nothing is scaled.  Works with everything above.
    void set_contour(bool frames, bool phonemes) { contour_frames = frames; contour_phonemes = phonemes; }
    const std::vector<zv_frame_level> &get_frame_levels() const { return frame_levels; }         // [max_seq_len], empty unless asked for
    const std::vector<zv_frame_level> &get_phoneme_levels() const { return phoneme_levels; }     // [num_phonemes], likewise
    // pitch track (include/zerovox_amd.h "pitch track") for the eval() calls that follow: the fundamental frequency and voicing of
    // every frame of the capacity and / or of every phoneme, metered on the device on the waveform get_wav() holds.  params: the lags,
    // the window and the threshold (its table pointers are ignored; nullptr or zeros: the defaults); they are checked when eval() runs.
    // A meter: nothing is scaled.  Works with everything above.
    void set_pitch(bool frames, bool phonemes, const zv_pitch *params = nullptr);
    const std::vector<zv_pitch_frame> &get_pitch_frames() const { return pitch_frame_rows; }         // [max_seq_len], empty unless asked for
    const std::vector<zv_pitch_phoneme> &get_pitch_phonemes() const { return pitch_phoneme_rows; }   // [num_phonemes], likewise

    // band levels (include/zerovox_amd.h "band levels") for the eval() calls that follow: the level per frequency band of every frame of
    // the capacity and / or of every phoneme, metered on the device on the waveform get_wav() holds.  n_bands 0: 16; edges: n_bands + 1
    // DFT bins, copied here, or nullptr: the default edges; they are checked when eval() runs.  A meter: nothing is scaled.
    void set_bands(bool frames, bool phonemes, uint32_t n_bands = 0, const uint32_t *edges = nullptr);
    uint32_t get_band_count() const { return (uint32_t)get_band_edges().size() - 1; }       // entries of a row
    std::vector<uint32_t> get_band_edges() const;                                           // the edges in force: set_bands' or the library's defaults
    const std::vector<float> &get_band_frames() const { return band_frame_rows; }           // [max_seq_len][bands], empty unless asked for
    const std::vector<float> &get_band_phonemes() const { return band_phoneme_rows; }       // [num_phonemes][bands], likewise

    // waveform filter (include/zerovox_amd.h "waveform filter") for the eval() calls that follow: n_taps taps of a linear-phase FIR,
    // copied here, applied on the device ahead of envelope, volume and every meter; nullptr: none.  They are checked when eval() runs.
    void set_filter(const float *taps, uint32_t n_taps);

    // mel alignment (include/zerovox_amd.h "mel alignment"): zv_mel_align of the rows a [Ta][M] and b [Tb][M]; params nullptr: scale 64
    // without normalisation; the maps may be nullptr.  Next to HiFiGAN::analyze, whose rows it takes.
    zv_alignment align(const float *a, uint32_t Ta, const float *b, uint32_t Tb, uint32_t M, const zv_align *params = nullptr,
                       int32_t *map_a = nullptr, int32_t *map_b = nullptr);
    // "say this with the timing of that take" for the eval() calls that follow: ref_wav (copied; its whole hops, Tb <= max_seq_len
    // frames) is a recording at the model's rate.  eval() then runs twice, fitted: the model's own timing first; the mel rows of both
    // waveforms (zv_mel_wave_batch, natural logarithm) are aligned (zv_mel_align with normalise), zv_align_durations moves the phoneme
    // boundaries onto the reference's clock, and the second run takes them as duration_frames: get_num_frames() == Tb, get_durations()
    // the new timings, get_alignment() the alignment.  nullptr: off.  It excludes per-phoneme duration_frames and a target.
    void set_time_like(const float *ref_wav, size_t n_samples);
    const zv_alignment &get_alignment() const { return alignment; }
    // loudness (include/zerovox_amd.h "loudness"): zv_loudness_wave over any waveform of T frames at the model's rate, its first
    // n_frames measured; ask nullptr: the identity; out [T * hop] or nullptr (a meter).  Next to HiFiGAN::loudness, for other lengths.
    zv_loudness_result loudness(const float *wav, uint32_t T, uint32_t n_frames, const zv_loudness *ask = nullptr, float *out = nullptr);
    // limiter (include/zerovox_amd.h "limiter"): zv_limit_wave over any waveform of T frames at the model's rate, its first n_frames
    // measured; ask nullptr: gain 1, ceiling 1, the default windows; out [T * hop].  Next to HiFiGAN::limit, for other lengths.
    zv_limit_result limit(const float *wav, uint32_t T, uint32_t n_frames, const zv_limiter *ask, float *out);
    // resampling (include/zerovox_amd.h "resampling"): zv_resample_wave over any waveform of S_in samples — another sample rate, as f32
    // (out), as PCM16 (pcm) or both, each [zv_resample_count(S_in, L, M)].  Next to HiFiGAN::resample, for other lengths.
    zv_resample_result resample(const float *wav, uint64_t S_in, const zv_resample *ask, float *out, int16_t *pcm);

    const zerovox_hparams &get_hparams() const { return hparams; }
    const float *get_wav() const { return wav; }
    uint32_t     get_num_frames() const { return n_frames; }

  private:
    void release();
    zerovox_hparams  hparams;
    zv_model        *model;
    FS2Encoder      *encoder;
    StyleTTSDecoder *decoder;
    HiFiGAN         *meldec;
    float           *hidden_state;
    float           *mel;
    float           *wav;
    uint32_t         n_frames;
    zv_prosody       prosody;
    bool             has_prosody;
    // per-phoneme controls (owned copies; an empty vector = that field is NULL) and the recorded timings
    std::vector<int32_t> pc_frames;
    std::vector<float>   pc_scale, pc_pitch, pc_energy;
    uint32_t             pc_n = 0;
    bool                 has_phonemes = false, record_durations = false;
    std::vector<int32_t> durations;
    bool                 fitted = false;
    uint32_t             target_frames = 0;
    zv_volume            volume = {1.0f, 0.0f, 0.0f};
    bool                 has_volume = false;
    zv_level             level = {0.0f, 0.0f, 0.0f, 0};
    zv_envelope          envelope = {nullptr, 0, 0, 0};
    std::vector<float>   env_gain;
    bool                 has_envelope = false, env_gain_set = false;
    bool                 contour_frames = false, contour_phonemes = false;
    std::vector<zv_frame_level> frame_levels, phoneme_levels;
    bool                 pitch_frames = false, pitch_phonemes = false;
    zv_pitch             pitch_params = {nullptr, nullptr, 0, 0, 0, 0.0f};
    std::vector<zv_pitch_frame>   pitch_frame_rows;
    std::vector<zv_pitch_phoneme> pitch_phoneme_rows;
    bool                 band_frames = false, band_phonemes = false;
    uint32_t             band_count = 0;
    std::vector<uint32_t> band_edges;
    std::vector<float>   band_frame_rows, band_phoneme_rows;
    bool                 has_filter = false;
    uint32_t             filter_n = 0;
    std::vector<float>   filter_taps;
    std::vector<float>   like_wav;
    zv_alignment         alignment = {0, 0.0, 0, 0};
};

}  // namespace ZeroVOX

#ifdef ZEROVOX_GGML_COMPAT_NAMES
typedef ZeroVOX::weights_t ggml_context;
typedef ZeroVOX::backend_t ggml_backend_t;
#endif
