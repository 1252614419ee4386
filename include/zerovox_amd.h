/* zerovox_amd.h — C-ABI of the MI355X-native ZeroVox hot path (libzerovox_amd.so).
 *
 * This is the drop-in boundary: plain pointers, sizes and status codes, no ggml / HIP / torch
 * types.  Each entry point replaces one piece of the reference's C++ class API
 * (/root/reference/src/zerovox.h, namespace ZeroVOX); the C++ facade with the reference's own
 * class names and method signatures (zerovox.cpp_amd/csrc/zerovox.h) is a thin layer over it.
 *
 *   zv_model_load      <- ZeroVOXModel::ZeroVOXModel(fname)   src/zerovox.cpp:21-179 (GGUF KV ->
 *                         hparams, weight upload, stage construction)
 *   zv_encode          <- FS2Encoder::eval                    src/zerovox.h:191, src/fs2encoder.cpp:594-656
 *   zv_decode          <- StyleTTSDecoder::eval               src/zerovox.h:323, src/stylettsdec.cpp:457-470
 *   zv_vocode          <- HiFiGAN::eval                       src/zerovox.h:378, src/hifigan.cpp:358-377
 *   zv_synthesize      <- ZeroVOXModel::eval                  src/zerovox.cpp:198-335 (three stages back to back)
 *   *_prosody          the same with per-utterance duration / pitch / energy controls (zv_prosody)
 *   *_phonemes         the same with per-phoneme controls as well (zv_phoneme_controls) and the phoneme timings out
 *   *_target           the same with a target frame count the utterance's durations are fitted to
 *   *_volume           the same with a gain, a loudness target and a peak ceiling per utterance (zv_volume) and the measured level out
 *   *_envelope         the same with per-phoneme gains, cross-fades and fades per utterance (zv_envelope)
 *   *_contour          the same with the level and peak of every frame and every phoneme out (zv_contour)
 *   *_pitch            the same with the fundamental frequency and voicing of every frame and every phoneme out (zv_pitch)
 *   zv_pitch_track     the pitch track of any waveform the caller brings
 *   *_bands            the same with the level per frequency band of every frame and every phoneme out (zv_bands)
 *   zv_band_levels     the band levels of any waveform the caller brings
 *   *_filter           the same with a linear-phase FIR filter per utterance applied to the waveform on the device (zv_filter)
 *   zv_filter_wave     the filter on any waveform the caller brings; zv_filter_design: band gains to taps, on the host
 *   zv_mel_wave        the log-mel rows of any waveform the caller brings (the vocoder's input domain); zv_mel_wave_batch: a batch of
 *                      them in one launch per kernel; zv_mel_design: Slaney mel weights, on the host
 *   zv_mel_align       the dynamic-time-warping path between two sequences of mel rows: its spectral distance and the frame maps;
 *                      zv_mel_align_batch: a batch of pairs in one launch per kernel; zv_align_durations: the timing transfer, on the host
 *   zv_loudness_wave   the BS.1770 loudness (LUFS) and true peak (dBTP) of any waveform the caller brings, and the waveform brought to a
 *                      LUFS target under a dBTP ceiling; zv_loudness_wave_batch: a batch of them in one launch per kernel;
 *                      zv_loudness_design: the K-weighting filters, the step and the interpolator for a rate, on the host
 *   zv_limit_wave      any waveform the caller brings behind a look-ahead peak limiter: a gain, then no sample above a ceiling;
 *                      zv_limit_wave_batch: a batch of them in one launch per kernel; zv_limit_design: milliseconds as sample counts, on
 *                      the host
 *   zv_resample_wave   any waveform the caller brings at another sample rate, as f32, as PCM16 with TPDF dither or both: the delivery
 *                      step behind the limiter and the way in for a recording; zv_resample_wave_batch: a batch of them in one launch
 *                      per kernel; zv_resample_design, zv_resample_count, zv_write_wav_pcm16: on the host
 *   zv_write_wav       <- ZeroVOXModel::write_wav_file       src/zerovox.cpp:337-391 (PCM16 mono RIFF)
 *   zv_last_error      <- std::runtime_error / die_fmt / GGML_ASSERT messages (src/zerovox.h:435-455)
 *
 * Differences that are deliberate: the number of phonemes N and the number of frames
 * T are run-time arguments (the reference fixes them at graph-build time: MAX_N_PHONEMES, max_seq_len);
 * results for a given (N, T) are those of a reference instance built for exactly that (N, T) — there
 * is no attention mask and InstanceNorm statistics run over all T frames (SURVEY Appx C-H2).
 * Bad ids / sizes return ZV_ERR_ARG instead of aborting.
 *
 * Threading: calls on one zv_model are serialised by the caller (one HIP stream per model);
 * several models per process are allowed (e.g. one per GPU).
 */
#ifndef ZEROVOX_AMD_H
#define ZEROVOX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zv_model zv_model;

typedef enum
{
    ZV_OK = 0,
    ZV_ERR_IO = 1,             /* file cannot be opened / read                          */
    ZV_ERR_FORMAT = 2,         /* not a GGUF v3 file, bad KV type, truncated            */
    ZV_ERR_MISSING = 3,        /* required KV key or tensor not found                   */
    ZV_ERR_SHAPE = 4,          /* tensor shape / dtype does not match the contract      */
    ZV_ERR_ARG = 5,            /* bad argument (null pointer, id out of range, T = 0 …) */
    ZV_ERR_DEVICE = 6,         /* HIP runtime error, no gfx950 device, kernel failure   */
    ZV_ERR_OOM = 7
} zv_status;

/* the reference's zerovox_hparams (src/zerovox.h:39-58) + the derived vocoder geometry */
typedef struct
{
    uint32_t max_seq_len;
    uint32_t emb_dim;
    uint32_t punct_emb_dim;
    uint32_t decoder_n_head;
    uint32_t conv_filter_size;
    uint32_t conv_kernel_size[2];
    uint32_t encoder_layer;
    uint32_t encoder_head;
    uint32_t encoder_vp_filter_size;
    uint32_t encoder_vp_kernel_size;
    uint32_t encoder_ve_n_bins;
    uint32_t audio_sampling_rate;
    uint32_t audio_num_mels;
    uint32_t audio_hop_size;
    /* inferred from tensor shapes (the reference hard-codes these, src/zerovox.cpp:127-138) */
    uint32_t voc_channels;
    uint32_t voc_num_upsamples;
    uint32_t voc_upsample_scales[8];
    uint32_t voc_num_resblocks;
    uint32_t voc_resblock_kernels[8];
} zv_hparams;

const char *zv_last_error(void);                 /* thread-local message of the last failure */
const char *zv_version(void);

/* ---- model life cycle ------------------------------------------------------------------- */
zv_status zv_model_load(const char *gguf_path, int device, zv_model **out);
void      zv_model_free(zv_model *m);
zv_status zv_model_get_hparams(const zv_model *m, zv_hparams *out);
/* size the activation arena up-front for the largest (N, T) that will be used (optional:
 * the arena also grows on demand, outside any timed / captured region) */
zv_status zv_model_reserve(zv_model *m, uint32_t max_phonemes, uint32_t max_frames);

/* ---- prosody controls (speaking rate, pitch, energy), one set per utterance ----------------------------------------
 * The variance adaptor's three decisions, steered per utterance.  All arithmetic is f32, every step rounded separately (the
 * library builds with -ffp-contract=off):
 *   duration: dur = (float)(exp((double)logdur) - 1.0); dur = dur * duration_scale;  d = (int)((double)dur + 0.5) clamped to
 *             [0, T]; the cumulative durations and n_frames follow from the scaled d
 *   pitch:    p = pred; p = p * pitch_scale; p = p + pitch_shift; p = p * (float)(nbins - 1);  bucket = (int)((double)p + 0.5)
 *             (truncating) clamped to [0, nbins - 1]; the pitch embedding added to the features is the one at this bucket, so
 *             the energy predictor sees it (reference src/fs2encoder.cpp:565-572)
 *   energy:   the same steps with energy_scale / energy_shift
 * Taps: logdur, pitch and energy stay the RAW predictions; pitch_bucket, energy_bucket, features, hidden and n_frames are the
 * controlled values.  The identity {1, 1, 0, 1, 0} gives exactly the bits of the uncontrolled entry points (x * 1.0f and
 * x + 0.0f are exact), and so does prosody == NULL.
 * Validation: every field finite and 0 < duration_scale <= 16, else ZV_ERR_ARG before any work is enqueued (the message names
 * the utterance index and the field). */
typedef struct
{
    float duration_scale;               /* > 0; 1 = as predicted, 2 = every phoneme twice as long */
    float pitch_scale, pitch_shift;     /* pitch prediction p -> p * pitch_scale + pitch_shift before bucketing */
    float energy_scale, energy_shift;   /* the same for energy */
} zv_prosody;                           /* identity: {1, 1, 0, 1, 0} */

/* ---- per-phoneme controls (forced durations, local rate, local pitch / energy) and phoneme timings -------------------------
 * One struct per utterance; every pointer is [n] (the utterance's phoneme count) or NULL = no control of that kind, so a
 * zero-initialised struct is the identity.  They act after the utterance's zv_prosody (NULL prosody = its identity).  All
 * arithmetic is f32, every step rounded separately:
 *   duration, for token i < num_phonemes:
 *     1. dur = (float)(exp((double)logdur) - 1.0)
 *     2. dur = dur * prosody.duration_scale                      (if prosody is given)
 *     3. dur = dur * duration_scale[i]                           (if given)
 *     4. d = (int)((double)dur + 0.5), clamped to [0, T]
 *     5. if duration_frames[i] >= 0: d = min(duration_frames[i], T)
 *     tokens at or past num_phonemes keep d = 0, even when a duration is forced for them
 *   pitch, for every token i < n:
 *     1. p = pred
 *     2. p = p * prosody.pitch_scale; p = p + prosody.pitch_shift
 *     3. p = p + pitch_shift[i]
 *     4. p = p * (float)(nbins - 1)
 *     5. bucket = (int)((double)p + 0.5), clamped to [0, nbins - 1]
 *   energy:   the same steps with energy_scale / energy_shift / energy_shift[i]
 * The identity values (frames -1, scale 1, shift 0), NULL pointers and a NULL struct give exactly the bits of the same call
 * without per-phoneme controls (x * 1.0f and x + 0.0f are exact; a -0.0 may become +0.0, which lands in the same bucket).
 * Taps: logdur, pitch and energy stay RAW; buckets, features, hidden, n_frames and durations are the controlled values.
 * Timings: durations[i] = min(cum_i, T) - min(cum_{i-1}, T), cum the running sum of d (cum_{-1} = 0): the frames phoneme i
 * occupies in hidden, starting at start_i = durations[0] + ... + durations[i-1]; its samples in wav are
 * [hop * start_i, hop * (start_i + durations[i])).  The durations sum to n_frames; phonemes cut off by T get the part that
 * fits, or 0.
 * Validation: ZV_ERR_ARG before any work is enqueued when a duration_frames[i] < -1 or > min(32768, zv_max_frames()), a
 * duration_scale[i] is not finite or outside (0, 16], or a shift is not finite (the message names the utterance index, the
 * field and the phoneme index). */
typedef struct
{
    const int32_t *duration_frames;     /* -1: keep the (scaled) prediction; 0..32768: phoneme i lasts exactly this many frames */
    const float   *duration_scale;      /* > 0, <= 16: multiplies phoneme i's duration after the utterance's duration_scale     */
    const float   *pitch_shift;         /* added to phoneme i's pitch prediction after the utterance's scale / shift           */
    const float   *energy_shift;        /* the same for energy                                                                  */
} zv_phoneme_controls;

/* ---- the hot path: host buffers in / out, synchronous (same protocol as the reference) ---- */
/* ids[n], puncts[n] i32; style[E] f32; hidden[T*E] f32 frame-major, zero-padded tail; returns the
 * regulator's frame count in *n_frames (may be NULL).  Optional taps (NULL to skip): logdur[n],
 * pitch_bucket[n], energy_bucket[n], features[n*E] — the pre-regulator values parity tests need. */
zv_status zv_encode(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style,
                    uint32_t n, uint32_t T, float *hidden, uint32_t *n_frames);
/* n = the encoder's max_n_phonemes: all n ids are embedded and attended to (no mask, src/fs2encoder.cpp:103-110,598-600);
 * num_phonemes <= n = how many of them the length regulator walks (FS2Encoder::eval's argument, :622).  zv_encode is
 * the num_phonemes == n case, which is what the reference's only caller passes (src/zerovox.cpp:200). */
zv_status zv_encode_taps(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style,
                         uint32_t n, uint32_t num_phonemes, uint32_t T, float *hidden, uint32_t *n_frames,
                         float *features, float *logdur, float *pitch, float *energy, int32_t *pitch_bucket,
                         int32_t *energy_bucket);
/* zv_encode_taps with prosody controls (NULL = identity: the bits of zv_encode_taps) */
zv_status zv_encode_taps_prosody(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n,
                                 uint32_t num_phonemes, uint32_t T, float *hidden, uint32_t *n_frames, float *features, float *logdur,
                                 float *pitch, float *energy, int32_t *pitch_bucket, int32_t *energy_bucket, const zv_prosody *prosody);
/* zv_encode_taps_prosody with per-phoneme controls (NULL = none) and the phoneme timings durations[n] (NULL to skip) */
zv_status zv_encode_taps_phonemes(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n,
                                  uint32_t num_phonemes, uint32_t T, float *hidden, uint32_t *n_frames, float *features, float *logdur,
                                  float *pitch, float *energy, int32_t *pitch_bucket, int32_t *energy_bucket, const zv_prosody *prosody,
                                  const zv_phoneme_controls *phonemes, int32_t *durations);
/* hidden[T*E], style[E] -> mel[T*num_mels] frame-major */
zv_status zv_decode(zv_model *m, const float *hidden, const float *style, uint32_t T, float *mel);
/* mel[T*num_mels] -> wav[T*hop_size]
 * Run-shortened vocoding (every unfitted entry point that vocodes, batches by default: switch ZV_VOC_RUNS).  The vocoder has no
 * normalisation over time and a reach of zv_vocoder_halo_frames() = H frames, so over a run of bit-identical mel rows — what the
 * decoder produces behind an utterance's end — its output is one hop-long frame, repeated.  A small kernel finds, per utterance,
 * the longest run [a, b) of mel rows that are equal as BITS (-0 and +0 differ, equal NaN patterns are equal); when the run is
 * longer than 2H + 1 rows by at least 16, only 2H + 1 of its rows are vocoded, the samples behind them land b - a - (2H + 1)
 * frames further on and the frames in between are copies of frame a + H.  All on the device, inside the same captured graph.
 * Results are UNCHANGED, bit for bit: every vocoder kernel sums in an order that does not depend on the tile or on T (the
 * promise zv_vocode_stream relies on).  Off in fitted mode, in zv_vocode_stream and under zv_debug_layer. */
zv_status zv_vocode(zv_model *m, const float *mel, uint32_t T, float *wav);

/* ---- "next" row f-3 (streaming): chunked vocoding with halo ------------------------------------
 * Vocodes mel[T][n_mels] in chunks of chunk_frames frames and hands every finished chunk to `sink` (called on the
 * calling thread, in order, with a pointer that is valid only during the call).  Each chunk is computed from its own
 * frames plus zv_vocoder_halo_frames() frames of context on either side, so the samples are bit-identical to those of
 * zv_vocode() on the whole mel (every vocoder kernel sums in an order that does not depend on the tile or on T); the
 * first audio is available after one chunk instead of after the whole utterance. */
typedef void (*zv_wav_sink)(void *user, const float *wav, uint64_t first_sample, uint64_t n_samples);
zv_status zv_vocode_stream(zv_model *m, const float *mel, uint32_t T, uint32_t chunk_frames, zv_wav_sink sink, void *user);
/* frames of context (per side) outside which a mel frame cannot influence a sample: the vocoder's receptive field */
uint32_t  zv_vocoder_halo_frames(zv_model *m);
/* encoder -> decoder -> vocoder with every intermediate kept in HBM; wav[T*hop_size]
 * Run-shortened decoding (the unfitted synthesize entry points, batches by default: switch ZV_DEC_RUNS).  Behind an utterance's
 * n_frames the decoder's input is zero up to T and its convs reach 14 frames, so its tensors are constant in between: the
 * decoder computes the rows in front of a = round_up(n_frames + 14 + 32, 32) and from b = round_down(T - 15, 32) on, counts the
 * 32-row blocks in between in its InstanceNorm statistics as copies of the block in front of a, and one pass writes all T mel
 * rows.  Results are UNCHANGED, bit for bit.  Off in fitted mode, under zv_debug_layer and in zv_decode*, whose hidden is the
 * caller's. */
zv_status zv_synthesize(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style,
                        uint32_t n, uint32_t T, float *wav, uint32_t *n_frames);
/* zv_synthesize with prosody controls (NULL = identity: the bits of zv_synthesize) */
zv_status zv_synthesize_prosody(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                                float *wav, uint32_t *n_frames, const zv_prosody *prosody);
/* zv_synthesize_prosody with per-phoneme controls (NULL = none) and the phoneme timings durations[n] (NULL to skip) */
zv_status zv_synthesize_phonemes(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                                 float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                 int32_t *durations);

/* n_utt independent utterances, each with its own (n_phonemes[u], T[u]): bit for bit the result of n_utt zv_synthesize
 * calls (no batch padding: padding would change the numbers, SURVEY Appx C-H2).  Up to 64 utterances / 64 Ki frames go
 * through the three stages as ONE launch per kernel: tensors are row-concatenated over the group and a segment table in
 * HBM tells every kernel where each utterance begins and ends, so the launches have many rounds of workgroups and the
 * whole group — input upload included — is one hipGraph (captured once per capacity bucket when graph mode is on).  For a
 * large group the graph ends before the last vocoder stage's residual blocks: those and the output conv run in
 * utterance sub-groups and a finished sub-group's waveforms are copied to the host (second stream) and into wav[] while
 * the next one computes; wav[u] is complete when the call returns, as before.
 * BASELINE.json configs[3]/[4]; with several GPUs the caller shards the list (one model per GPU, no collective). */
zv_status zv_synthesize_batch(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                              const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                              float *const *wav, uint32_t *n_frames);
/* the same with prosody controls: prosody[n_utt], one set per utterance (NULL = identity for all: the bits of
 * zv_synthesize_batch).  The controls travel in the batch's device input block with the styles, so a replayed graph picks
 * up new values without being captured again; utterance u gives the bits of zv_synthesize_prosody(..., &prosody[u]). */
zv_status zv_synthesize_batch_prosody(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                      const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                                      float *const *wav, uint32_t *n_frames, const zv_prosody *prosody);
/* the same with per-phoneme controls, phonemes[n_utt] (NULL = none for all; each struct is [n_phonemes[u]]), and the phoneme
 * timings, durations[n_utt] (NULL to skip; each entry [n_phonemes[u]] or NULL).  The rows travel in the batch's device input
 * block like the prosody rows, so a replayed graph reads new values; utterance u gives the bits and the durations of
 * zv_synthesize_phonemes(..., &prosody[u], &phonemes[u], durations[u]). */
zv_status zv_synthesize_batch_phonemes(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                       const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                                       float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                       const zv_phoneme_controls *phonemes, int32_t *const *durations);

/* The two halves of zv_synthesize_batch for a serving loop that keeps a batch in flight per lane (additive):
 * _begin builds the input block, enqueues the upload, the kernels and the waveform downloads of ONE launch group (at most
 * 64 utterances / 64 Ki frames of capacity, else ZV_ERR_ARG) on lane `lane` (< ZV_BATCH_LANES; each lane owns a stream, an
 * activation arena and a pinned staging block) and returns; _end waits for that batch and fills wav[] / n_frames[], which
 * — like T[] and the pointer arrays' targets — must stay valid until then.  While one lane's last kernels and downloads
 * run, the next lane's upload and first kernels already do.  Results are those of zv_synthesize_batch, bit for bit.
 * Two batches in flight (begin k, end k - 1) keep the GPU busy all the time (zv_batch_timeline: no gap); more lanes work
 * and buy nothing.
 * Every other entry point may be called in between (they use lane 0's stream: not while lane 0 has a batch in flight). */
#define ZV_BATCH_LANES 4
zv_status zv_synthesize_batch_begin(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                    const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                    const uint32_t *T, float *const *wav, uint32_t *n_frames);
/* _begin with prosody controls, prosody[n_utt] (NULL = identity); the array is read before the call returns */
zv_status zv_synthesize_batch_begin_prosody(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                            const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                            const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody);
/* _begin with per-phoneme controls and timings (as zv_synthesize_batch_phonemes): the controls are read before the call returns;
 * _end fills durations[u], whose buffers must stay valid until then */
zv_status zv_synthesize_batch_begin_phonemes(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                             const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                             const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                             const zv_phoneme_controls *phonemes, int32_t *const *durations);
zv_status zv_synthesize_batch_end(zv_model *m, uint32_t lane);

/* ---- fitted synthesis: only the frames the length regulator fills ----------------------------------------------------
 * Every synthesize call takes T, a frame CAPACITY chosen before the duration predictor has run; the calls above decode and
 * vocode all T frames (the reference's static graph does, src/zerovox.cpp:326-334), zero tail of `hidden` included, so the
 * audio of an utterance depends on the capacity its caller picked (the decoder's InstanceNorm / AdaIN statistics run over the
 * tail too) and the tail's samples are computed for nobody.  The fitted forms keep T[u] as the size of buffers and grids, but
 * the decoder and the vocoder treat utterance u as exactly n_frames[u] frames long: after the length regulator a small kernel
 * writes a second frame table in HBM, {row0 of the capacity table, n_frames[u]}, and every later kernel reads its extents
 * there — one pass, one captured graph, no host round trip; a replayed graph picks up new lengths like new controls.
 * With nf the frame count the length regulator produces under capacity T (controls included), for each utterance:
 *   - wav[0 .. nf*hop) has exactly the bits of the unfitted call of the same kind (zv_synthesize / _prosody / _phonemes, or
 *     utterance u of the batch forms) with the same inputs and T = nf.  (Well defined: with T' = nf no duration clamp becomes
 *     active that was not before — every d_i <= sum d = nf when nothing was cut off, nf = T otherwise — so the encoder gives
 *     the same nf and the same hidden[0 .. nf).)
 *   - wav[nf*hop .. T*hop) is 0.0f.
 *   - *n_frames = nf; durations[] mean what they mean in the _phonemes forms and sum to nf.
 *   - nf == 0 (every walked phoneme got 0 frames): ZV_OK, n_frames = 0, all of wav 0.0f.
 *   - nf == T: the bits of the unfitted call at T, all of them.
 * Arguments, validation, limits (zv_max_frames(), 64 utterances / 64 Ki frames of CAPACITY per launch group) and error
 * messages are those of the _phonemes forms; prosody, phonemes and durations may be NULL.  The copies to the host stay sized
 * by capacity.  zv_synthesize_batch_begin_fitted is finished by zv_synthesize_batch_end like every other _begin. */
zv_status zv_synthesize_fitted(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                               float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                               int32_t *durations);
zv_status zv_synthesize_batch_fitted(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                     const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                                     float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                     const zv_phoneme_controls *phonemes, int32_t *const *durations);
zv_status zv_synthesize_batch_begin_fitted(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                           const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                           const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                           const zv_phoneme_controls *phonemes, int32_t *const *durations);
/* ---- target durations: fit an utterance to an exact frame count ------------------------------------------------------------
 * "Say this in exactly target frames" (dubbing, subtitle and animation sync, fixed-length slots), in one pass: between the
 * duration predictor and the length regulator a device step turns the predicted durations and the target into integer
 * durations that sum to the target exactly, and the length regulator takes them as forced frame counts.  The target travels in
 * the batch's device input block like the other controls, so a replayed graph picks up new targets.  A target in seconds is
 * floor(seconds * audio_sampling_rate / audio_hop_size + 0.5) frames (the caller converts).
 * The rule, per utterance with 0 < target <= T (target == 0: none), over the tokens i < num_phonemes, in 64-bit integers from the
 * weights on, so that it does not depend on the order of any sum and can be restated bit for bit:
 *   dur_i    steps 1-3 of the per-phoneme duration rule above: (float)(exp((double)logdur) - 1.0), times prosody.duration_scale
 *            (if prosody is given), times duration_scale[i] (if given), f32, every step rounded separately
 *   forced   phonemes with duration_frames[i] >= 0 keep d_i = min(duration_frames[i], T); Fs = their sum
 *   free     all the others share R = target - Fs.  R <= 0 or no free phoneme: every free phoneme gets 0 (forced durations
 *            win; n_frames = min(Fs, T) as without a target)
 *   weights  q_i = dur_i > 0 ? (int64)min((double)dur_i * 65536.0, 2^40) : 0  (NaN and values <= 0 give 0, +inf gives 2^40);
 *            Q = sum of q_i over the free phonemes; Q == 0: every free q_i = 1 and Q = the number of free phonemes (equal shares)
 *   shares   base_i = (q_i * R) / Q, rem_i = (q_i * R) % Q; L = R - sum of base_i (0 <= L < number of free phonemes); the L free
 *            phonemes with the largest rem_i — ties go to the lower index — get d_i = base_i + 1, the others d_i = base_i
 *   tokens at or past num_phonemes keep 0.
 * sum d_i = target whenever a free phoneme exists and Fs <= target; every d_i <= T.  The result is defined as exactly the bits
 * of the _phonemes call (fitted != 0: the _fitted call) with duration_frames[i] = d_i for every i < num_phonemes: hidden,
 * n_frames, durations[] and wav.  A uniform duration_scale changes nothing but the rounding of q_i; per-phoneme scales shift
 * the shares.  Pitch and energy decisions do not depend on durations and stay as they are; the taps logdur, pitch, energy stay RAW.
 * With fitted != 0 and a reachable target, wav[0 .. target*hop) is the audio and the rest is 0.0f.
 * target_frames == 0 (batches: a NULL array, or 0 for that utterance) gives the bits of the same call without a target.
 * Arguments, limits and messages are those of the _phonemes / _fitted forms; in addition ZV_ERR_ARG before any work is enqueued
 * when target_frames[u] > T[u] (the message names the entry point, the utterance and target_frames), or when a request with
 * a target has an utterance of more than 3584 phonemes.  The header csrc/fit_durations.h holds the rule as plain C++ (host
 * reference included).  zv_synthesize_batch_begin_target is finished by zv_synthesize_batch_end. */
zv_status zv_encode_taps_target(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n,
                                uint32_t num_phonemes, uint32_t T, float *hidden, uint32_t *n_frames, float *features, float *logdur,
                                float *pitch, float *energy, int32_t *pitch_bucket, int32_t *energy_bucket, const zv_prosody *prosody,
                                const zv_phoneme_controls *phonemes, int32_t *durations, uint32_t target_frames);
zv_status zv_synthesize_target(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                               float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                               int32_t *durations, uint32_t target_frames, int fitted);
zv_status zv_synthesize_batch_target(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                     const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                                     float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                     const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                     const uint32_t *target_frames, int fitted);
zv_status zv_synthesize_batch_begin_target(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                           const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                           const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                           const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                           const uint32_t *target_frames, int fitted);
/* ---- volume controls: gain, loudness target, peak ceiling, level meter ----------------------------------------------------------
 * The level of an utterance is otherwise whatever the vocoder's tanh gives.  The volume forms measure the finished waveform on the
 * device and scale it there, inside the same captured graph and — for a large batch — per tail group, ahead of that group's
 * download: two small memory-bound passes over data that is still in HBM.  The output stays f32 at the model's rate; nothing is
 * resampled or converted.  The volume rows travel in the batch's device input block like the other controls, so a replayed graph
 * picks up new values.  dB is the caller's: gain = 10^(dB / 20), a level in dBFS likewise (full scale = 1.0).
 * The rule, per utterance, with hop = audio_hop_size, T the capacity, nf = min(n_frames, T) and x[0 .. T*hop) the waveform the
 * same call gives without volume; integers wherever the order of a sum could matter, so that it can be restated bit for bit and does
 * not depend on how the kernels split the work:
 *   measure  over the speech only, the samples i < nf*hop.  A finite x_i: a = min(|x_i|, 1.0f), q_i = (int64)((double)a * 524288.0
 *            + 0.5), truncating (0 <= q_i <= 2^19); a NaN or infinite x_i: q_i = 0, and it is left out of the peak.
 *            S = sum of q_i^2, an unsigned 64-bit integer (< 2^62 up to zv_max_frames()).  peak = the largest finite |x_i|, unclamped:
 *            the maximum of the sign-cleared f32 bit patterns, 0 when there is no finite sample.
 *   level    S > 0: rms = sqrt((double)S / ((double)(nf*hop) * 274877906944.0)); otherwise rms = 0.
 *   gain     gd = (double)gain.  If target_rms > 0 and S > 0: gd = (double)target_rms / rms * (double)gain.  If peak_ceiling > 0 and
 *            peak > 0 and gd * (double)peak > (double)peak_ceiling: gd = (double)peak_ceiling / (double)peak (the ceiling wins).
 *            g = (float)gd; where the ceiling applied, while (float)(g * peak) > peak_ceiling: g = nextafterf(g, 0) (at most four
 *            steps; two suffice).  So no finite sample of the result exceeds the ceiling in magnitude.
 *   apply    wav[i] = x_i * g for all T*hop samples, one f32 multiply each: fitted zeros stay zero, an unfitted tail is scaled like
 *            the speech.
 *   report   zv_level {rms = (float)rms, peak, gain = g, reserved = 0}: level and peak BEFORE the gain.
 * Every f64 step is one IEEE operation (a u64 -> f64 conversion, *, / or sqrt).  csrc/level.h holds the rule as plain C++ (host
 * reference included).
 * volume == NULL and levels == NULL: the request of the _target call, the same launches, the same bits.  volume == NULL with levels
 * given: a meter only — g = 1, the waveform's bits unchanged.  The identity {1, 0, 0} gives the unchanged bits too (x * 1.0f is
 * exact).  Batches: volume[n_utt] and levels[n_utt], each may be NULL; utterance u gives the bits and the level of
 * zv_synthesize_volume(..., &volume[u], &levels[u]).  levels must stay valid until the call (batches in flight: _end) returns.
 * Arguments, limits and messages are those of the _target forms; in addition ZV_ERR_ARG before any work is enqueued when a field is
 * not finite, gain is outside [0, 1000], or target_rms or peak_ceiling is outside [0, 1] (the message names the entry point, the
 * utterance and the field).  zv_synthesize_batch_begin_volume is finished by zv_synthesize_batch_end.
 * Out of scope: zv_vocode*, zv_vocode_device and zv_vocode_stream (they have no n_frames, and a stream has not seen the whole
 * utterance when its first chunk leaves).  Per-phoneme gain and fades: the amplitude envelope below. */
typedef struct
{
    float gain;             /* linear, 0 .. 1000; multiplies the result of the loudness target (1 = none)            */
    float target_rms;       /* 0 = none; else the level the speech is brought to, 0 < target_rms <= 1                 */
    float peak_ceiling;     /* 0 = none; else no finite sample of the result exceeds it, 0 < peak_ceiling <= 1        */
} zv_volume;                /* identity: {1, 0, 0} */
typedef struct
{
    float    rms, peak;     /* of the speech, before the gain */
    float    gain;          /* the factor every sample was multiplied by */
    uint32_t reserved;      /* 0 */
} zv_level;
zv_status zv_synthesize_volume(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                               float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                               int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels);
zv_status zv_synthesize_batch_volume(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                     const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                                     float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                     const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                     const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels);
zv_status zv_synthesize_batch_begin_volume(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                           const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                           const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                           const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                           const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels);
/* ---- amplitude envelope: per-phoneme gain, cross-fades and fades -----------------------------------------------------------------
 * The per-phoneme form of the volume controls.  A caller who has the phoneme timings (durations[]) can stress a word, duck a phrase or
 * soften the cut where T truncates an utterance, without walking the waveform on the host: the envelope forms scale the finished
 * waveform on the device, inside the same captured graph and — for a large batch — per tail group, ahead of that group's download
 * and ahead of the volume passes, so a loudness target or a peak ceiling holds on what the caller receives.  The gains and the
 * scalars travel in the batch's device input block like the other controls, so a replayed graph picks up new values.
 * The rule, per utterance, with hop = audio_hop_size, T the capacity, nf = min(n_frames, T), n = nf*hop, x[0 .. T*hop) the waveform
 * the same call gives without an envelope and without volume, and durations[] the phoneme timings of that call as the _phonemes
 * forms define them (after prosody, per-phoneme controls, forced frames and a target), start_i the sum of the durations before i:
 *   gains    G_i = (int64)((double)phoneme_gain[i] * 65536.0 + 0.5), truncating, so 0 <= G_i <= 2^20; phoneme_gain == NULL: every
 *            G_i = 65536.  Tokens at or past num_phonemes own no frame and are never read.
 *   frames   for 0 <= f < nf: F[f] = G_i of the phoneme that owns frame f (start_i <= f < start_i + durations[i]; a phoneme of 0
 *            frames owns nothing).  Outside that range F is edge-replicated: F[f < 0] = F[0], F[f >= nf] = F[nf - 1].
 *   windows  r = ramp_frames, W = 2r + 1, A[f] = sum of F[j] for j = f - r .. f + r: an integer sum, its order does not matter.
 *   knots    B[f] = A[f - 1] + A[f] for 0 <= f <= nf, at the frame starts; B[f] <= 2 * 129 * 2^20 < 2^29, one uint32.
 *   sample   s = f*hop + j with 0 <= j < hop; every step one IEEE f64 operation (the library builds with -ffp-contract=off):
 *            1. num = B[f]*(hop - j) + B[f + 1]*j for s < n, num = B[nf]*hop for s >= n (int64, below 2^38)
 *            2. den = 2*W*hop*65536
 *            3. d = (double)num / (double)den
 *            4. Fi = fade_in_samples > 0 and s < Fi: t = (double)s / (double)Fi; d = d * t
 *            5. Fo = fade_out_samples > 0 and k = n - 1 - s < Fo: t = (double)max(k, 0) / (double)Fo; d = d * t (so s >= n - 1 gives 0)
 *            6. e = (float)d; y[s] = x[s] * e, one f32 multiply
 *   nf == 0  there are no knots: e = 1 for every sample when Fo == 0, e = 0 when Fo > 0.
 *   volume   if the call carries a zv_volume or asks for levels: measured on y over y[0 .. n) and applied to y, wav[s] = y[s] * g —
 *            two separately rounded f32 multiplies, in that order.  The zv_level reports the level and the peak of the enveloped
 *            speech, before g.
 * What follows: the gain curve is piecewise linear and continuous.  Inside a phoneme of more than 2r + 2 frames it is exactly
 * (float)(G_i / 65536) from r + 1 frames after the phoneme's start to r + 1 frames before its end (knots start_i + r + 1 ..
 * start_i + durations[i] - r - 1: one whole frame at exactly 2r + 3 frames); a transition spans 2r + 2 frames centred on the
 * boundary.  e never leaves [min G, max G] / 65536.  When every G_i is 65536 and both fades are 0, num == den and e == 1.0f:
 * envelope == NULL, a zeroed struct and all-ones gains at any ramp_frames give the unchanged bits (x * 1.0f is exact).  Fitted zeros
 * stay zero; without a fade-out an unfitted tail is scaled by the last knot, like the end of the speech.  csrc/envelope.h holds the
 * rule as plain C++ (host reference included).
 * envelope == NULL: the request of the _volume call, the same launches, the same bits.  Batches: envelope[n_utt] or NULL, each
 * struct's phoneme_gain [n_phonemes[u]] or NULL; utterance u gives the bits of zv_synthesize_envelope(..., &envelope[u]).  The arrays
 * are read before the call returns.  Arguments, limits and messages are those of the _volume forms; in addition ZV_ERR_ARG before
 * any work is enqueued when a gain is not finite or outside [0, 16], ramp_frames > 64 or a fade is above 0x7fffffff (the message
 * names the entry point, the utterance, the field and, for a gain, the phoneme index), or when the checkpoint's audio_hop_size is
 * below 10.  zv_synthesize_batch_begin_envelope is finished by zv_synthesize_batch_end.
 * Out of scope: zv_vocode* and zv_vocode_stream (they have no timings); curve shapes other than linear. */
typedef struct
{
    const float *phoneme_gain;     /* [n] or NULL (= all 1): linear gain of phoneme i, finite, 0 .. 16           */
    uint32_t     ramp_frames;      /* 0 .. 64: half-width r of the cross-fade between neighbouring phonemes        */
    uint32_t     fade_in_samples;  /* 0 = none; the first samples of the speech rise linearly from 0               */
    uint32_t     fade_out_samples; /* 0 = none; the last samples of the speech fall linearly to 0, the rest is 0   */
} zv_envelope;                     /* zero-initialised = identity */
zv_status zv_synthesize_envelope(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                                 float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                 int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                 const zv_envelope *envelope);
zv_status zv_synthesize_batch_envelope(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                       const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                                       float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                       const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                       const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                       const zv_envelope *envelope);
zv_status zv_synthesize_batch_begin_envelope(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                             const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                             const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                             const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                             const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                             const zv_envelope *envelope);
/* ---- level contour: per-frame and per-phoneme level and peak ----------------------------------------------------------------------
 * The read side of the envelope and the missing half of the phoneme timings: durations[] tell WHEN a phoneme sounds, the contour HOW
 * LOUD, at the same granularity and from the same call.  A caller who drives a mouth shape or a level meter, trims the model's
 * leading and trailing silence, checks that a ducked phrase came out 6 dB down or looks for the one clipped phoneme of a batch needs
 * no pass over the samples on the host: the contour forms meter the finished waveform on the device, inside the same captured graph
 * and — for a large batch — per tail group, ahead of that group's download and behind the envelope and the volume passes.  The
 * contour is a meter: it scales nothing.
 * The rule, per utterance, with hop = audio_hop_size, T the capacity, w[0 .. T*hop) the waveform the SAME call writes to wav (after
 * fitted zeroing, envelope and volume: what the caller receives), durations[] the phoneme timings of that call as the _phonemes
 * forms define them, start_i the sum of the durations before i, and q_i, the peak's bit patterns and rms as the volume controls
 * define them (a NaN or infinite sample: q = 0 and left out of the peak; -0.0 counts as 0):
 *   frame    for 0 <= f < T, over the capacity: S_f = sum of q^2 over the samples w[f*hop .. f*hop + hop), an unsigned 64-bit integer;
 *            P_f = the largest sign-cleared bit pattern of the finite samples among them, 0 when there is none.
 *            frames[f] = {(float)rms(S_f, hop), the f32 with the bits P_f}, rms(S, k) = S > 0 ? sqrt((double)S / ((double)k *
 *            274877906944.0)) : 0.  Fitted zeros give {0, 0}; an unfitted tail is measured like the speech.
 *   phoneme  for 0 <= i < n, d = durations[i]: S = sum of S_f and P = max of P_f over start_i <= f < start_i + d (S < 2^62 as for the
 *            volume controls).  phonemes[i] = {(float)rms(S, d*hop), the f32 with the bits P}.  d == 0 gives {0, 0}: a phoneme cut off
 *            by T, a forced 0, a token at or past num_phonemes.
 * Every f64 step is one IEEE operation and nothing depends on how the work is split: sums of integers, maxima of bit patterns.
 * csrc/contour.h holds the rule as plain C++ (host reference included).  What follows, with nf = min(n_frames, T): the maximum of
 * frames[f].peak over f < nf is the zv_level peak of a meter-only call (volume == NULL, levels given); the sum of S_f over f < nf is
 * that call's S; the phonemes' sums partition the sum of S_f over f < min(sum of durations, T), and their maxima its peak.
 * contour == NULL, or every struct with both pointers NULL: the request of the _envelope call, the same launches, the same graph,
 * the same bits.  With a contour the waveform, n_frames, durations and levels keep exactly their bits.  Batches: contour[n_utt] or
 * NULL; an utterance may ask for one table, both or none, and gives the rows of zv_synthesize_contour(..., &contour[u]).  The struct
 * array is read before the call (_begin) returns; the tables it points to must stay valid until the call (batches in flight: _end)
 * returns.  Arguments, limits and messages are those of the _envelope forms.  The frames pass reads whole 16-byte loads per frame,
 * so a checkpoint's audio_hop_size must be a multiple of 4: the launcher refuses any other with ZV_ERR_DEVICE rather than carry a
 * scalar path that no loadable checkpoint can reach (the loader accepts hop 300 alone).
 * zv_synthesize_batch_begin_contour is finished by zv_synthesize_batch_end.
 * Out of scope: zv_vocode*, zv_vocode_stream and the encode / decode entry points (they have no timings); any filtering or weighting
 * of the level (A-weighting, LUFS gating); trimming itself — the caller trims from the contour. */
typedef struct
{
    float rms, peak;
} zv_frame_level;
typedef struct
{
    zv_frame_level *frames;     /* [T] or NULL: one row per frame of the capacity       */
    zv_frame_level *phonemes;   /* [n] or NULL: one row per token                       */
} zv_contour;                   /* zero-initialised = none */
zv_status zv_synthesize_contour(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                                float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                const zv_envelope *envelope, const zv_contour *contour);
zv_status zv_synthesize_batch_contour(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                      const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                                      float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                      const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                      const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                      const zv_envelope *envelope, const zv_contour *contour);
zv_status zv_synthesize_batch_begin_contour(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                            const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                            const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                            const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                            const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                            const zv_envelope *envelope, const zv_contour *contour);
/* ---- pitch track: per-frame and per-phoneme fundamental frequency and voicing ------------------------------------------------------
 * The read side of the pitch controls.  pitch_scale, pitch_shift and the per-phoneme pitch_shift[i] act on the variance predictor's
 * output in prediction units; the pitch track tells what fundamental frequency came out, in Hz, per frame and per phoneme, from the
 * same call and with no pass over the samples on the host: the pitch forms meter the finished waveform on the device, inside the same
 * captured graph and — for a large batch — per tail group, ahead of that group's download and behind envelope, volume and contour.
 * The pitch track is a meter: it changes no sample.  zv_pitch_track meters any waveform the caller brings (a reference recording).
 * The rule, per utterance, with sr = audio_sampling_rate, hop = audio_hop_size, T the capacity, w[0 .. T*hop) the waveform the SAME
 * call writes to wav (after fitted zeroing, envelope and volume: what the caller receives), durations[] and start_i as for the contour.
 * Parameters, per utterance, each one at 0 takes its default: min_lag = sr / 441, max_lag = sr / 63, window = 2 * hop (integer
 * divisions; lags in samples: 50, 350 and 600 at 22 050 Hz and hop 300, i.e. 63 .. 441 Hz), voiced_threshold = 0.5f.  With the
 * defaults filled in, ZV_ERR_ARG before any work is enqueued unless 8 <= min_lag < max_lag <= 512, max_lag <= 8 * min_lag,
 * 64 <= window <= 1024 and voiced_threshold is finite and in (0, 1]; the message names the entry point, the utterance and the
 * field, and says so when the value is a default (the checkpoint's rate then needs explicit lags).  Three octaves at most: the
 * search below starts at min_lag and must start outside the zero-lag lobe of the longest period it may report, which
 * max_lag <= 8 * min_lag ensures even for a pure sinusoid.
 * For frame 0 <= f < T, with Lmin = min_lag, Lmax = max_lag, W = window, M = W + Lmax + 1:
 *   span     s0 = f*hop + hop/2 - M/2 (signed; both divisions of non-negative integers); y[t] = w[s0 + t] for 0 <= t < M where
 *            0 <= s0 + t < T*hop and the sample is finite, else +0.0.  The span never reads another utterance's samples.
 *   scale    Pk = the largest sign-cleared bit pattern in y.  Pk < 0x33800000 (a peak below 2^-24): the frame is silent, its row
 *            {0, 0}.  Else e = (Pk >> 23) - 127, k = 9 - e, a[t] = sign(y[t]) * min((int64)((double)|y[t]| * 2^k + 0.5), 1023): the
 *            conversion truncates, the product and the sum are single f64 operations; |a[t]| <= 1023, the peak lands in 512 .. 1023.
 *   sums     for L in [Lmin - 1, Lmax + 1]: c(L) = sum over t < W of a[t] * a[t+L], E(L) = sum over t < W of a[t+L]^2, and
 *            E0 = sum over t < W of a[t]^2: integers below 2^30, so no order of summation can show.
 *   corr     r(L) = min((double)c(L) / sqrt((double)(uint64)(E0 * E(L))), 1.0) when c(L) > 0, E0 > 0 and E(L) > 0, else 0.
 *   pick     rmax = max r(L) over Lmin <= L <= Lmax; rmax == 0: the row is {0, 0}.  L0 = the smallest L in that range with
 *            r(L) >= 0.875 * rmax; L* = the smallest L >= L0 with L == Lmax or r(L+1) <= r(L); strength = r(L*).
 *   refine   p = r(L*-1) - r(L*), n = r(L*+1) - r(L*), den = p + n.  den < 0: delta = ((r(L*-1) - r(L*+1)) / den) * 0.5, set to 0
 *            unless -0.5 <= delta <= 0.5; else delta = 0.  f0 = (double)sr / ((double)L* + delta).
 *   row      voiced = strength >= (double)voiced_threshold; frames[f] = {voiced ? (float)f0 : 0, (float)strength}; kept for the
 *            phonemes: Fq = voiced ? (uint32)(f0 * 256.0 + 0.5) : 0, and the voiced flag.
 * For phoneme 0 <= i < n, d = durations[i], over the frames start_i <= f < start_i + d: nv = the number of voiced frames, SF = the sum
 * of their Fq (unsigned 64-bit); phonemes[i] = {nv > 0 ? (float)((double)SF / ((double)nv * 256.0)) : 0, d > 0 ? (float)((double)nv /
 * (double)d) : 0}.  d == 0 gives {0, 0}.
 * Every f64 step is one IEEE operation (the library builds with -ffp-contract=off); csrc/pitch.h holds the rule as plain C++ (host
 * reference included).  What follows:
 *   - multiplying the waveform by a power of two changes no row, as long as no sample becomes subnormal or infinite and the span's
 *     peak stays at or above 2^-24;
 *   - fitted zeros give {0, 0}; an unfitted tail is measured like the speech;
 *   - a frame whose span reaches outside [0, T*hop) sees zeros there: its lag may be off near the two ends of an utterance.  That
 *     is part of the rule, not an error;
 *   - nothing depends on how lags or samples are dealt over lanes: integer sums, maxima and minima, ties going to the lower lag.
 * pitch == NULL, or every struct with both table pointers NULL: the request of the _contour call, the same launches, the same graph,
 * the same bits (the parameters of such a struct are not looked at).  With a pitch track the waveform, n_frames, durations, levels
 * and contour rows keep exactly their bits.  Batches: pitch[n_utt] or NULL; an utterance may ask for one table, both or none, with
 * its own parameters, and gives the rows of zv_synthesize_pitch(..., &pitch[u]).  The parameters travel in the batch's device input
 * block like the other controls, so a replayed graph picks up new values.  The struct array is read before the call (_begin)
 * returns; the tables it points to must stay valid until the call (batches in flight: _end) returns.  Arguments, limits and messages
 * are otherwise those of the _contour forms.  zv_synthesize_batch_begin_pitch is finished by zv_synthesize_batch_end.
 * zv_pitch_track meters a host waveform wav[T * hop] at the model's rate and hop, eagerly, on lane 0: pitch->frames is required,
 * pitch->phonemes must be NULL (there are no timings), 0 < T <= zv_max_frames(), else ZV_ERR_ARG; the rows are those of the rule
 * with w = wav.
 * Out of scope: zv_vocode*, zv_vocode_stream and the encode / decode entry points; smoothing or tracking across frames (Viterbi,
 * median filters: the caller filters the rows); any change of the pitch controls themselves; resampling. */
typedef struct
{
    float f0_hz, strength;
} zv_pitch_frame;               /* f0_hz 0 = unvoiced or silent */
typedef struct
{
    float f0_hz, voiced;
} zv_pitch_phoneme;             /* mean F0 of the voiced frames; share of voiced frames */
typedef struct
{
    zv_pitch_frame   *frames;     /* [T] or NULL: one row per frame of the capacity */
    zv_pitch_phoneme *phonemes;   /* [n] or NULL: one row per token                 */
    uint32_t min_lag, max_lag, window;   /* 0 = default */
    float    voiced_threshold;           /* 0 = default */
} zv_pitch;                     /* zero-initialised = none */
zv_status zv_synthesize_pitch(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                              float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                              int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                              const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch);
zv_status zv_synthesize_batch_pitch(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                    const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                                    float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                    const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                    const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                    const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch);
zv_status zv_synthesize_batch_begin_pitch(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                          const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                          const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                          const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                          const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                          const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch);
zv_status zv_pitch_track(zv_model *m, const float *wav, uint32_t T, const zv_pitch *pitch);
/* ---- band levels: per-frame and per-phoneme level per frequency band ----------------------------------------------------------------
 * The read side of timbre: the level of the waveform in up to 64 frequency bands, per frame and per phoneme, from the same call and
 * with no pass over the samples on the host (a spectrogram view, a viseme driver, a sibilance check, the one muffled phoneme of a
 * batch).  The bands forms meter the finished waveform on the device, inside the same captured graph and — for a large batch — per
 * tail group, ahead of that group's download and behind envelope, volume, contour and pitch track.  Band levels are a meter: they
 * change no sample.  zv_band_levels meters any waveform the caller brings.
 * The rule, per utterance, with hop = audio_hop_size, T the capacity, w[0 .. T*hop) the waveform the SAME call writes to wav (what
 * the caller receives), durations[] and start_i as for the contour.  N = 1024; bins 0 .. 512 of the N-point DFT; bin k lies at
 * k * sr / 1024 Hz.  n_bands = 0 takes 16; edges = NULL takes the default edges 1,3,5,8,12,17,24,33,45,62,84,114,155,210,285,387,513
 * (roughly third-octave steps from 22 Hz to the Nyquist frequency at 22 050 Hz, without DC) and then needs n_bands 0 or 16.  Band b
 * covers the bins edges[b] <= k < edges[b+1].  ZV_ERR_ARG before any work is enqueued when n_bands > 64, when the edges are not
 * strictly ascending, when edges[n_bands] > 513, or when edges is NULL and n_bands is neither 0 nor 16; the message names the entry
 * point, the utterance and the field.
 *   tables   wnd(t) = 0.5 - 0.5*cos(2*pi*t/N); C[k][t] = (int)floor(126*wnd(t)*cos(2*pi*((k*t) mod N)/N) + 0.5), S[k][t] likewise with
 *            sin, (k*t) mod N reduced in integers: 8-bit integers in [-126, 126].  At the scale 126 no product comes nearer than
 *            1.27e-5 to a half-integer, so any libm gives the same table.  It is built on the host at the first request and uploaded
 *            once (1 MiB of device memory per model, outside the lanes' arenas).
 *   frame    for 0 <= f < T: s0 = f*hop + hop/2 - N/2 (signed); y[t] = w[s0 + t] for 0 <= t < N where 0 <= s0 + t < T*hop and the
 *            sample is finite, else +0.0.  The span never reads another utterance's samples.
 *   scale    Pk = the largest sign-cleared bit pattern in y.  Pk < 0x33800000 (a peak below 2^-24): the frame is silent, its row all
 *            zeros.  Else e = (Pk >> 23) - 127, k = 12 - e, a[t] = sign(y[t]) * min((int64)((double)|y[t]| * 2^k + 0.5), 8191): the
 *            pitch track's quantiser at 13 bits.
 *   sums     Re(k) = sum over t of a[t]*C[k][t], Im(k) = sum over t of a[t]*S[k][t]: integers below 2^29 (the rows of |C| and |S| sum
 *            to at most 64 512), so no order of summation can show.  P(k) = Re^2 + Im^2 (unsigned 64-bit, below 2^59), Q(k) =
 *            P(k) >> 6, S_b = the sum of Q(k) over band b's bins (below 2^63).
 *   row      pw_b = ((double)S_b / 48774928.0) * 2^(-2k); frames[f][b] = (float)sqrt(pw_b).  48 774 928 = 8 * the sum of
 *            round(126*wnd(t))^2: a sinusoid of amplitude A inside a band reads A / sqrt(2), the measure of the level contour.
 *            Kept for the phonemes: v = pw_b * 2^38 + 0.5, Eq[f][b] = v >= 2^47 ? 2^47 : (uint64)v (it saturates above an RMS of
 *            about 22, so 32 768 frames sum below 2^62).
 * For phoneme 0 <= i < n, d = durations[i], SE = the sum of Eq[f][b] over the frames start_i <= f < start_i + d:
 * phonemes[i][b] = d > 0 ? (float)sqrt((double)SE / ((double)d * 274877906944.0)) : 0.
 * Every f64 step is one IEEE operation (the library builds with -ffp-contract=off); csrc/bands.h holds the rule as plain C++ (host
 * reference included).  What follows:
 *   - fitted zeros give zero rows; an unfitted tail is measured like the speech;
 *   - a frame near either end of the utterance sees zeros outside [0, T*hop).  That is part of the rule, not an error;
 *   - bins 0 and 512 are counted like the others (their power is not halved); the default edges leave out DC;
 *   - multiplying the waveform by a power of two scales every row by it exactly, as long as no sample becomes subnormal or
 *     infinite, the span's peak stays at or above 2^-24 and the kept power stays below its ceiling;
 *   - the dynamic range inside ONE frame is bounded by the 8-bit twiddles: a band far from a strong tone reads about 50 dB below it
 *     at the least, whatever is there.  Across frames the block scaling keeps the full range of the samples;
 *   - nothing depends on how frames, bins or samples are dealt over lanes and matrix instructions: integer sums throughout.
 * bands == NULL, or every struct with both table pointers NULL: the request of the _pitch call, the same launches, the same graph,
 * the same bits (n_bands and edges of such a struct are not looked at).  With band levels the waveform, n_frames, durations, levels,
 * contour rows and pitch rows keep exactly their bits.  Batches: bands[n_utt] or NULL; an utterance may ask for one table, both or
 * none, with its own n_bands and edges, and gives the rows of zv_synthesize_bands(..., &bands[u]).  n_bands and the edges travel in
 * the batch's device input block like the other controls, so a replayed graph picks up new values.  The struct array and the edges
 * are read before the call (_begin) returns; the tables must stay valid until the call (batches in flight: _end) returns.
 * Arguments, limits and messages are otherwise those of the _pitch forms.  zv_synthesize_batch_begin_bands is finished by
 * zv_synthesize_batch_end.
 * zv_band_levels meters a host waveform wav[T * hop] at the model's rate and hop, eagerly, on lane 0: bands->frames is required,
 * bands->phonemes must be NULL (there are no timings), 0 < T <= zv_max_frames(), else ZV_ERR_ARG; the rows are those of the rule
 * with w = wav.
 * Out of scope: zv_vocode*, zv_vocode_stream and the encode / decode entry points; a full 513-bin table (64 caller-chosen bands
 * cover it); mel or triangular weighting, log compression, MFCCs; a second twiddle digit for more than about 50 dB of range; other
 * window lengths; smoothing across frames.  The write side of the rows, an equaliser per utterance, is zv_filter below. */
typedef struct
{
    float          *frames;    /* [T][n_bands] or NULL: one row per frame of the capacity */
    float          *phonemes;  /* [n][n_bands] or NULL: one row per token                 */
    uint32_t        n_bands;   /* 0 = default (16); else 1 .. 64                          */
    const uint32_t *edges;     /* [n_bands + 1] DFT bins, or NULL = the default edges     */
} zv_bands;                    /* zero-initialised = none */
zv_status zv_synthesize_bands(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                              float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                              int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                              const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch, const zv_bands *bands);
zv_status zv_synthesize_batch_bands(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                    const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                                    float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                    const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                    const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                    const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch,
                                    const zv_bands *bands);
zv_status zv_synthesize_batch_begin_bands(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                          const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                          const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                          const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                          const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                          const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch,
                                          const zv_bands *bands);
zv_status zv_band_levels(zv_model *m, const float *wav, uint32_t T, const zv_bands *bands);
/* ---- waveform filter: a linear-phase FIR equaliser per utterance ---------------------------------------------------------------------
 * The write side of band levels: a telephone band, a bass cut for a small speaker, a presence lift, a softened sibilant band or a
 * low-pass ahead of the caller's decimation, applied while the waveform is still in device memory.  The filter forms run it behind the
 * vocoder's last convolution and AHEAD of envelope, volume controls and all meters, inside the same captured graph and — for a large
 * batch — per tail group: the peak ceiling holds for the filtered signal, and contour, pitch and band rows describe the waveform
 * the caller receives.  zv_filter_wave filters any waveform the caller brings; zv_filter_design turns band gains into taps.
 * The rule, per utterance, with hop = audio_hop_size, F = n_frames in fitted mode and the capacity T otherwise, S = F*hop, x[0 .. S)
 * the vocoder's waveform (what the _bands call would have written ahead of its envelope), L = n_taps, c = (L-1)/2, h = taps:
 *   span     x'[j] = x[j] where 0 <= j < S and the sample is finite, else +0.0.  The span never reads another utterance's samples.
 *   sample   for 0 <= n < S: acc = +0.0 (a double); for k = 0, 1, ..., L-1 in that order acc = acc + (double)h[k] * (double)x'[n + c - k];
 *            y[n] = (float)acc.  The product of two f32 values is exact in f64, so every step is ONE IEEE addition whether or not a
 *            compiler fuses it; the ascending order per output sample is part of the rule.
 *   tail     for S <= n < T*hop: y[n] = +0.0f.  The fitted promise survives: wav[0 .. nf*hop) has the bits of the unfitted filtered
 *            call at T = nf, and the rest is zero.
 * y takes x's place for everything that follows in the call.  The centre tap is aligned with the sample: a symmetric filter adds no
 * delay, so timings, contour, pitch and band rows keep pointing at the right samples.  Nothing depends on how samples are dealt over
 * lanes, waves or workgroups.  csrc/filter.h holds the rule as plain C++ (host reference included).  What follows:
 *   - L = 1, h = {1} returns x with -0.0 as +0.0 and non-finite samples as +0.0;
 *   - a result beyond the f32 range becomes infinite by the conversion;
 *   - samples near either end of the utterance see zeros outside [0, S).  That is part of the rule, not an error.
 * ZV_ERR_ARG before any work is enqueued, the message naming the entry point, the utterance and the field: n_taps even or above 511,
 * or 0 with taps not NULL ("filter n_taps"); a tap that is not finite ("filter taps").
 * filter == NULL, or every struct with taps == NULL (n_taps of such a struct is not looked at): the request of the _bands call, the
 * same launches, the same graph, the same bits.  Batches: filter[n_utt] or NULL; in a batch where some utterances carry a filter the
 * others come through as exact copies of their bits (-0.0 and NaN patterns included) and give what the _bands call gives.  Tap counts
 * and taps travel in the batch's device input block like the band edges, one row of 1 + 511 32-bit words per utterance, so a replayed
 * graph picks up new taps and new tap counts.  The struct array and the taps are read before the call (_begin) returns.  With a
 * filter the lane's arena holds one waveform more (the filter's input).  The filter never runs under zv_debug_layer.  Arguments,
 * limits and messages are otherwise those of the _bands forms.  zv_synthesize_batch_begin_filter is finished by
 * zv_synthesize_batch_end.
 * zv_filter_wave filters a host waveform wav[T * hop] at the model's hop, eagerly, on lane 0, into out[T * hop] (out may be wav):
 * the rule with x = wav and S = T*hop; filter->taps == NULL copies.  0 < T <= zv_max_frames(), else ZV_ERR_ARG.
 * zv_filter_design is host only and needs no model and no device.  edges are bins of the 1 024-point DFT of zv_bands, with its
 * defaults and its validation (n_bands 0 = 16; edges NULL = the default edges, then n_bands 0 or 16); gains[n_bands] are linear, >= 0
 * and finite, else ZV_ERR_ARG ("gains"); n_taps as above; taps[n_taps] receives the result.  In f64, each tap rounded to f32 once:
 *   m = -c .. c; w[m] = 0.5 + 0.5*cos(2*pi*m/(L+1)); lp(f)[m] = 2f at m = 0, else sin(2*pi*f*m)/(pi*m);
 *   band b covers bins edges[b] <= k < edges[b+1], its cut-offs f_lo = max(edges[b] - 0.5, 0)/1024 and
 *   f_hi = min(edges[b+1] - 0.5, 512)/1024 cycles per sample;
 *   h[m+c] = [m == 0] + the sum over b, in order, of (gains[b] - 1) * (lp(f_hi)[m] - lp(f_lo)[m]) * w[m].
 * All-ones gains give the delta filter exactly; bins outside every band keep gain 1.  The resolution is the window's: a step between
 * neighbouring bands takes about 4096/(L+1) bins to complete — 16 bins, about 345 Hz at 22 050 Hz, at L = 255 — so the narrow
 * low bands of the default edges cannot be set apart from their neighbours; away from the edges by that much the response is within
 * 0.0063 times the sum of the gain steps of the gains asked for.
 * Out of scope: filters that change inside an utterance (per phoneme, time-varying); IIR filters; resampling or any change of the
 * output's rate or sample type; zv_vocode*, zv_vocode_stream and the encode / decode entry points. */
typedef struct
{
    const float *taps;    /* [n_taps] or NULL = no filter */
    uint32_t     n_taps;  /* odd, 1 .. 511; 0 with taps NULL */
} zv_filter;              /* zero-initialised = none */
zv_status zv_synthesize_filter(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                               float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                               int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                               const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch, const zv_bands *bands,
                               const zv_filter *filter);
zv_status zv_synthesize_batch_filter(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                     const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                                     float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                     const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                     const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                     const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch,
                                     const zv_bands *bands, const zv_filter *filter);
zv_status zv_synthesize_batch_begin_filter(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                           const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                           const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                           const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                           const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                           const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch,
                                           const zv_bands *bands, const zv_filter *filter);
zv_status zv_filter_wave(zv_model *m, const float *wav, uint32_t T, const zv_filter *filter, float *out);
zv_status zv_filter_design(uint32_t n_bands, const uint32_t *edges, const float *gains, uint32_t n_taps, float *taps);
/* ---- mel analysis: a waveform's log-mel rows ---------------------------------------------------------------------------------------------
 * The way back into the vocoder's input domain: zv_vocode* reads raw log-mel rows (hifigan.mean / hifigan.scale are applied inside the
 * vocoder) and zv_mel_wave turns samples into such rows — for analysis-resynthesis of a converted checkpoint (wav -> mel -> zv_vocode ->
 * wav), for the mel of a served waveform against the mel that went in, and for mels of recorded audio.  The transform is the band
 * levels' 1 024-point DFT at twice the digits on both operands, exact on the i8 matrix cores.
 * The rule, per utterance, with hop = audio_hop_size, M = audio_num_mels, S = T*hop samples x[0 .. S), N = 1024, 513 bins.  Every row
 * can be restated bit for bit (csrc/mel.h holds the rule as plain C++, host reference included); nothing depends on how work is split
 * over lanes, waves, instructions or workgroups.
 *   span       frame f (0 <= f < T) covers the samples f*hop + centre - 512 + t, t = 0 .. 1023; centre is 0 .. hop-1 (0: librosa's
 *              center=True; hop/2: the band levels' spans).  Outside [0, S): pad = 0 reads +0.0; pad = 1 reflects without repeating the
 *              edge (-j -> j, S-1+j -> S-1-j) and needs S >= 513.  A non-finite sample counts as +0.0.  A span never reads another
 *              utterance's samples.
 *   quantise   the band levels' block quantiser: the span's peak exponent gives k, a = sign(y) * min((int64)(|y| * 2^k + 0.5), 8191); a
 *              span whose peak is below 2^-24 is silent.  Two signed base-128 digits: hi = (a + 64) >> 7, lo = a - 128*hi.
 *   table      C[k][t] = floor(8188 * w[t] * cos(2*pi*k*t/1024) + 0.5), S[k][t] likewise with sin, w the periodic Hann window of 1 024;
 *              the entries are split into the same two digits.  (At 8 188 no product is within 1.4e-5 of a tie.)
 *   sums       three i32 sums per (frame, bin, cos / sin): a2 = sum hi*Chi, a1 = sum (hi*Clo + lo*Chi), a0 = sum lo*Clo, each below 2^23;
 *              Re = 16384*a2 + 128*a1 + a0 as int64 (below 2^37), Im likewise.
 *   magnitude  each step one IEEE f64 operation: r = (double)Re; i = (double)Im; p = r*r; q = i*i; p = p + q; g = sqrt(p);
 *              g = g * 2^-k; g = g / 8188.0.
 *   mel        channel c: acc = +0.0, then for k = 0 .. 512 ascending acc = acc + (double)W[c][k] * g[k] — one multiply and one add,
 *              each rounded.  W is the caller's weights[M*513] (finite f32) or the design below.
 *   level      v = max(acc, (double)floor), floor 0 meaning 1e-10f; out = (float)L(v) for log = 0 (log10) or 1 (ln), (float)v for
 *              log = 2.  L is not libm's logarithm but a fixed sequence of f64 steps (csrc/mel.h mel_ln: frexp, m folded into
 *              [sqrt(1/2), sqrt(2)), s = (m-1)/(m+1), Horner over 1/13 .. 1/3, 1 in s*s, ln v = e*LN2 + 2*s*poly, log10 = ln * LOG10E,
 *              the constants given as bit patterns), within 1e-11 of the logarithm.  A silent frame gives L(floor) in every channel.
 * zv_mel_wave takes a host waveform wav[T * hop] at the model's rate and hop, eagerly, on lane 0, into out[T * num_mels];
 * zv_mel_wave_batch takes n_utt of them in ONE launch per kernel, and utterance u receives the bits of its single call.  One zv_mel
 * serves the batch.  0 < T[u] <= zv_max_frames(); the hop must be a multiple of 4, as for the band levels.  ZV_ERR_ARG before any
 * work is enqueued, the message naming the entry point, the utterance and the field: centre >= hop, pad above 1 or pad = 1 with an
 * utterance below 513 samples, log above 2, a floor that is negative or not finite, a weight that is not finite, or what
 * zv_mel_design refuses.  The table (two digit planes, 2.2 MB) is built on the host at the first request; the weights travel with
 * the call.  Never part of a captured graph or of the zv_synthesize* chain.
 * zv_mel_design is host only and needs no model and no device: Slaney-scale triangular filters with Slaney area normalisation
 * (librosa's defaults) on the bin centres f_k = k * sampling_rate / 1024, in f64, each weight rounded to f32 once:
 *   mel(f) = 3f/200 below 1 000 Hz, else 15 + 27 * ln(f/1000) / ln(6.4), and hz() its inverse;
 *   p[i] = hz(mel(fmin) + i * (mel(fmax) - mel(fmin)) / (num_mels + 1)), i = 0 .. num_mels + 1;
 *   W[c][k] = max(0, min((f_k - p[c]) / (p[c+1] - p[c]), (p[c+2] - f_k) / (p[c+2] - p[c+1]))) * 2 / (p[c+2] - p[c]).
 * fmax_hz = 0 means Nyquist.  ZV_ERR_ARG for a value that is not finite or negative, fmin_hz >= fmax_hz, fmax_hz above Nyquist, or
 * num_mels 0 or above 256.
 * Out of scope: other DFT sizes or window lengths; mel analysis inside the zv_synthesize* chain or a captured graph; a distance between
 * mels (see "mel alignment" below: zv_mel_align); resampling. */
typedef struct
{
    const float *weights;   /* [num_mels*513] or NULL = zv_mel_design(rate, num_mels, fmin_hz, fmax_hz) */
    float        fmin_hz, fmax_hz;
    uint32_t     centre, pad, log;
    float        floor;
} zv_mel;                   /* zero-initialised = Slaney 0 .. Nyquist, centre 0, zero padding, log10, floor 1e-10 */
zv_status zv_mel_wave(zv_model *m, const float *wav, uint32_t T, const zv_mel *mel, float *out /* [T*num_mels] */);
zv_status zv_mel_wave_batch(zv_model *m, uint32_t n_utt, const float *const *wav, const uint32_t *T, const zv_mel *mel /* one for the batch */,
                            float *const *out);
zv_status zv_mel_design(uint32_t sampling_rate, uint32_t num_mels, float fmin_hz, float fmax_hz, float *weights);
/* ---- mel alignment: the DTW path between two sequences of mel rows, its distance and the timing transfer ---------------------------------
 * Two sequences of mel rows rarely have the same number of frames: synthesised against recorded speech, the mel of a re-timed waveform
 * against the mel that went in, a recording whose timing a synthesis is to follow.  zv_mel_align finds the dynamic-time-warping path
 * between a[Ta][M] and b[Tb][M] (f32 rows of any kind: zv_mel_wave rows, decoder mels, anything of the same width), the spectral
 * distance along it and the two frame maps; zv_align_durations turns a map into the durations of the other side.
 * The rule, per pair.  Every output can be restated bit for bit (csrc/align.h holds the rule as plain C++, host reference included);
 * nothing depends on how cells are dealt over lanes, waves, tiles or workgroups.
 *   quantise   a non-finite value counts as +0.0; d = (double)x * (double)scale; d = min(max(d, -1023.0), 1023.0);
 *              d = d + (d >= 0 ? 0.5 : -0.5); q = (int64)d, truncating — each one IEEE f64 operation.
 *   normalise  (normalise = 1 only; per sequence and per channel m: it removes a recording's gain and a fixed channel response)
 *              s = sum over t of q[t][m]; mean = floor((2*s + T) / (2*T)), a true floor (round half up); q' = q - mean.  Else q' = q.
 *              |q'| <= 2046.
 *   cost       c[i][j] = sum over m of (qa'[i][m] - qb'[j][m])^2, an integer below 2^32 (256 * 4092^2 = 4 286 582 784).
 *   path       D[0][0] = c[0][0], else D[i][j] = c[i][j] + the least D of the predecessors that exist, examined in the order
 *              (i-1, j-1), (i-1, j), (i, j-1); a later one wins only when it is strictly smaller.  D is int64 (below 2^45);
 *              total = D[Ta-1][Tb-1].
 *   walk       from (Ta-1, Tb-1) back to (0, 0) along the choices taken: path_len = L, the number of cells; map_a[i] = the smallest j
 *              on the path in row i, map_b[j] = the smallest i on the path in column j.  The distance in walk order, from the end to
 *              the start: acc = +0.0; per cell acc = acc + sqrt((double)c[i][j]); then acc = acc / (double)L; acc = acc / (double)scale
 *              — each one IEEE operation.  distance is the mean Euclidean distance per path cell, in the rows' own unit.
 * Limits: 1 <= M <= 256, 1 <= Ta, Tb <= ZV_ALIGN_MAX_FRAMES.  params->scale = 0 means 64.0, otherwise it must be finite and positive;
 * params->normalise is 0 or 1; a zero-initialised zv_align is scale 64 without normalisation.  Everything else returns ZV_ERR_ARG
 * before any work is enqueued, the message naming the entry point, the pair (batch form) and the field.  map_a [Ta] and map_b [Tb]
 * may be NULL.  The calls run eagerly, on lane 0, like zv_mel_wave_batch.
 * zv_mel_align_batch: ONE launch per kernel for a launch group of pairs, and pair p receives the bits of its single call.  A group
 * holds at most 2^27 cells (Ta*Tb summed), where cost (u32) and choice (u8) take 640 MiB of the lane's I/O block; a larger batch runs
 * as consecutive groups of consecutive pairs.  One zv_align serves the batch; the arrays map_a / map_b or entries of them may be NULL.
 * The dot products of the cost run on v_mfma_i32_16x16x64_i8 over two signed base-128 digits of q' (hi = (q' + 64) >> 7,
 * lo = q' - 128*hi), c = |qa'|^2 + |qb'|^2 - 2*(16384*hh + 128*(hl + lh) + ll) in int64.
 * zv_align_durations is host only and needs neither a model nor a device: the timing transfer.  durations_a[n] are the frames per
 * phoneme of sequence a (their sum must be Ta), map_a[Ta] the map of an alignment of a against a sequence of Tb frames.  With s_p
 * the sum of durations_a before p: pos_0 = 0, pos_p = map_a[s_p] when s_p < Ta, else Tb, pos_n = Tb; durations_b[p] = pos_{p+1} - pos_p.
 * ZV_ERR_ARG for a NULL pointer, a negative duration ("durations_a"), a sum other than Ta, or a map_a that is not non-decreasing
 * inside [0, Tb).  The result is non-negative, sums to Tb, and is valid as zv_phoneme_controls duration_frames when
 * Tb <= min(32768, zv_max_frames()).
 * Out of scope: band constraints; other step patterns or slope weights; open-ended (sub-sequence) alignment; cepstra / MCD in dB (the
 * caller converts distance); sequences beyond 4096 frames; alignment inside the zv_synthesize* chain or a captured graph; a pitch or
 * energy transfer (zv_pitch_track and the maps give the caller what it needs); resampling. */
#define ZV_ALIGN_MAX_FRAMES 4096
typedef struct
{
    float    scale;         /* 0 = 64.0 */
    uint32_t normalise;     /* 0 or 1 */
} zv_align;                 /* zero-initialised = scale 64, no normalisation */
typedef struct
{
    uint64_t total;         /* D[Ta-1][Tb-1] */
    double   distance;
    uint32_t path_len;
    uint32_t reserved;
} zv_alignment;
zv_status zv_mel_align(zv_model *m, const float *a, uint32_t Ta, const float *b, uint32_t Tb, uint32_t M, const zv_align *params,
                       zv_alignment *out, int32_t *map_a /* [Ta] or NULL */, int32_t *map_b /* [Tb] or NULL */);
zv_status zv_mel_align_batch(zv_model *m, uint32_t n_pairs, const float *const *a, const uint32_t *Ta, const float *const *b,
                             const uint32_t *Tb, uint32_t M, const zv_align *params /* one for the batch */, zv_alignment *out,
                             int32_t *const *map_a /* array or entries may be NULL */, int32_t *const *map_b);
zv_status zv_align_durations(uint32_t n, const int32_t *durations_a, uint32_t Ta, const int32_t *map_a, uint32_t Tb,
                             int32_t *durations_b);
/* ---- loudness: ITU-R BS.1770 integrated loudness, true peak and normalisation -------------------------------------------------------------
 * Delivery specifications speak LUFS and dBTP ("-16 LUFS integrated, -1 dBTP"), not the RMS and sample peak of the volume controls.
 * zv_loudness_wave takes a host waveform of T frames (T * hop samples at the model's rate), measures its first N = min(n_frames, T) * hop
 * samples and, where out is given, returns all T * hop samples scaled by ONE gain: exactly the volume controls' division of labour.
 * zv_loudness_wave_batch takes n_utt of them, one launch per kernel per launch group of consecutive utterances (at most 2^26 samples,
 * capacities rounded up to 256); utterance u receives exactly the bits of its single call.  Both run eagerly on lane 0 like
 * zv_mel_wave_batch, are never part of a captured graph or of the zv_synthesize* chain, and use scratch of lane 0's arena.
 * zv_loudness_design is host only and needs neither a model nor a device.
 *
 * THE RULE.  Every f64 step is ONE IEEE operation (nothing is contracted into a fused multiply-add), denormals are kept, a sample that is not finite
 * counts as +0.0: x'_n, n in [0, N); x' is +0.0 outside.  Nothing depends on how the work is split, because the rule fixes the split.
 *   1. design (f64, on the host; the kernels take it as data).  With K = tan(pi f0 / fs):
 *        shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G/20), Vb = Vh^0.4996667741545416,
 *                   a0 = 1 + K/Q + K^2, b0 = (Vh + Vb K/Q + K^2)/a0, b1 = 2 (K^2 - Vh)/a0, b2 = (Vh - Vb K/Q + K^2)/a0,
 *                   a1 = 2 (K^2 - 1)/a0, a2 = (1 - K/Q + K^2)/a0
 *        high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, b = (1, -2, 1), a1' and a2' by the same two formulas
 *      (at 48 000 Hz the standard's table).  step = (fs + 5) / 10 samples.  M = A^256 by eight squarings P <- P P, every entry the
 *      chain acc <- fma(P[i][k], P[k][j], acc), k = 0 .. 3 from +0.0 (four fused multiply-adds, written out; the one place besides
 *      step 4 where a product is not rounded on its own), where A is the zero-input transition of the cascade
 *      below on (p1, p2, q1, q2): rows (-a1, 1, 0, 0), (-a2, 0, 0, 0), (-2 - a1', 0, -a1', 1), (1 - a2', 0, -a2', 0).
 *      interp[j] = (float)(sinc((j - 24)/4) * 0.5 (1 - cos(2 pi j / 48))), j = 0 .. 48, entries with |.| < 1e-6 set to 0.
 *      sampling_rate must lie in 4 000 .. 768 000 (a step holds a chunk; the shelf lies below Nyquist).
 *   2. K-weighting in chunks of 256 samples; chunk k covers x'[256 k .. 256 k + 256), k < ceil(N / 256).  One sample through the
 *      cascade (transposed direct form II), state (p1, p2, q1, q2):
 *        y = b0 x + p1;   p1 <- (b1 x + p2) - a1 y;   p2 <- b2 x - a2 y;
 *        w = y + q1;      q1 <- (q2 - 2 y) - a1' w;   q2 <- y - a2' w            (y, w from the OLD state; every product, sum and
 *      difference rounded on its own)
 *      A: z_k = the state after chunk k run from the zero state.
 *      B: s_0 = 0, s_(k+1)[r] = (((M[r][0] s_k[0] + M[r][1] s_k[1]) + M[r][2] s_k[2]) + M[r][3] s_k[3]) + z_k[r], r = 0 .. 3, in k.
 *      C: chunk k run again from s_k; its outputs w are squared and added in ascending sample order, from +0.0, into the chunk's two
 *         RUN sums: run 0 takes the samples n < e, run 1 those from e on, e = (256 k / step + 1) * step (integer division): the
 *         intersections of the chunk with the 100 ms steps it meets.
 *      D: E_j, j < J = N / step (whole steps only) = +0.0 plus the runs of step j, chunk after chunk in ascending order.
 *   3. gating.  Momentary block i, 0 <= i <= J - 4: z_i = (((E_i + E_(i+1)) + E_(i+2)) + E_(i+3)) / (double)(4 step).  Absolute gate
 *      z_i > Ga, Ga the f64 with the bits 0x3e7f791ec6e1d5aa (10^((-70 + 0.691)/10)); Gr = 0.1 * (sum / (double)count) over the blocks
 *      past Ga; integrated = sum / (double)count over the blocks with z_i > Ga and z_i > Gr; both sums start at +0.0 and run in
 *      ascending i.  momentary_max = max z_i.  Short-term block i, i + 30 <= J: (+0.0 + E_i + ... + E_(i+29), ascending) /
 *      (double)(30 step); short_term_max their maximum.  No block, or none past the gates: mean square 0, LUFS -inf, a target does nothing.
 *   4. true peak.  For f = 1, 2, 3 and n = 0 .. N + 10: v = the chain acc <- acc + (double)interp[f + 4 k] * x'_(n - k), k = 0 .. 11
 *      ascending from +0.0 (the products are exact).  true_peak = the maximum of all |v| and of (double)sample_peak; sample_peak the
 *      largest finite |x_n|, n < N.
 *   5. gain.  zt = 10^(((double)target_lufs + 0.691) / 10) (the host's pow).  gd = (double)gain; with the target on and integrated > 0:
 *      gd = sqrt(zt / integrated) * (double)gain; with the ceiling on and gd * true_peak > (double)ceiling: gd = (double)ceiling /
 *      true_peak; g = (float)gd; where the ceiling applied, g steps one bit pattern towards 0 while (float)((double)g * true_peak) >
 *      ceiling (at most four times).  out[i] = wav[i] * g, one f32 multiply, for all T * hop samples.
 *   6. report.  lufs(z) = (float)(-0.691 + 10 * (L(z) * log10 e)) with L the fixed-sequence logarithm of the mel analysis (above), -inf
 *      for z below 2^-1022; true_peak_dbtp = (float)(20 * (L(tp) * log10 e)) likewise.
 * csrc/loudness.h holds the rule as plain C++ with a host reference, loud_reference(); tests/loudness_rule.py restates it in numpy.
 *
 * Arguments: every field finite; gain in [0, 1000]; flags within bits 0 and 1; with bit 0 target_lufs in [-70, 0]; with bit 1
 * true_peak_ceiling in (0, 1] (linear: -1 dBTP is 10^(-1/20)); 0 < T <= zv_max_frames(); n_frames beyond T counts as T.  ask == NULL is the
 * identity for every utterance; out == NULL (or a NULL entry) meters only and changes nothing in the result.
 * Not covered: loudness range (LRA); channel weights (mono); resampling; a stage of the zv_synthesize* chain or a captured graph. */
#define ZV_LOUDNESS_TARGET  1u
#define ZV_LOUDNESS_CEILING 2u
typedef struct
{
    float    gain;                  /* linear, applied with or without a target */
    float    target_lufs;           /* bit 0 of flags */
    float    true_peak_ceiling;     /* linear, bit 1 of flags */
    uint32_t flags;
} zv_loudness;                      /* identity: {1, 0, 0, 0} */
typedef struct
{
    double   integrated_ms, momentary_max_ms, short_term_max_ms;     /* mean squares of the K-weighted signal */
    double   true_peak;             /* linear */
    uint32_t blocks, blocks_absolute, blocks_gated;      /* 400 ms blocks: all, past the absolute gate, past both gates */
    float    sample_peak;
    float    integrated_lufs, momentary_max_lufs, short_term_max_lufs, true_peak_dbtp;
    float    gain;                  /* applied to out */
    uint32_t reserved;
} zv_loudness_result;
typedef struct
{
    double   shelf_b[3], shelf_a[2];            /* b0 b1 b2, a1 a2 */
    double   highpass_b[3], highpass_a[2];
    double   M[16];                             /* row major */
    float    interp[49];
    uint32_t step;
} zv_loudness_filter;
zv_status zv_loudness_design(uint32_t sampling_rate, zv_loudness_filter *out);
zv_status zv_loudness_wave(zv_model *m, const float *wav, uint32_t T, uint32_t n_frames, const zv_loudness *ask, zv_loudness_result *res,
                           float *out /* [T * hop] or NULL: meter only */);
zv_status zv_loudness_wave_batch(zv_model *m, uint32_t n_utt, const float *const *wav, const uint32_t *T,
                                 const uint32_t *n_frames /* NULL = T */, const zv_loudness *ask /* [n_utt] or NULL */,
                                 zv_loudness_result *res /* [n_utt] */, float *const *out /* array or entries may be NULL */);
/* ---- limiter: a look-ahead peak limiter behind the loudness stage -----------------------------------------------------------------------
 * zv_loudness_wave meets a LUFS target under a dBTP ceiling with ONE gain, so where the two conflict the target is missed (step 5
 * above) — the normal case for speech, whose true peak often lies more than 15 dB above its integrated loudness.  The limiter takes
 * the gain the target asked for, pulls down the samples around a peak and leaves the rest alone.
 * zv_limit_wave takes a host waveform of T frames, measures its first N = min(n_frames, T) * hop samples and returns all T * hop samples
 * limited; zv_limit_wave_batch takes n_utt of them, one launch per kernel per launch group of consecutive utterances (cut as for
 * zv_loudness_wave_batch), and utterance u receives exactly the bits of its single call.  Both run eagerly on lane 0, are never part of
 * a captured graph or of the zv_synthesize* chain, and use scratch of lane 0's arena.  The model's rate must lie in 4 000 .. 768 000, and
 * the interpolator is the loudness design's.  zv_limit_design is host only.
 *
 * THE RULE.  Nothing in it is recursive along time and everything behind step 2 is integer, so no result depends on how the work is
 * split.  Every f64 step is ONE IEEE operation (nothing is contracted); a sample that is not finite or lies outside [0, N) counts as
 * +0.0 (x'), as in loudness.  ONE = 2^30, W = attack + release + 1.
 *   1. peaks.  v_f(n), f = 1, 2, 3: loudness step 4's chain over interp[f + 4 k], k = 0 .. 11 ascending from +0.0.  For every integer m:
 *      p_m = max(|x'_m| as f64, |v_1(m + 6)|, |v_2(m + 6)|, |v_3(m + 6)|), the peak of the interval [m, m + 1) on the 4x grid (the
 *      interpolator's delay is 6 samples); p_m = 0 outside m in [-6, N + 4].  true_peak_before = max p_m, bit for bit zv_loudness_wave's
 *      true_peak of the same span; sample_peak_before is its sample_peak.
 *   2. required gain, 2.30 fixed point.  a_m = (double)gain * p_m; q_m = ONE where a_m <= (double)ceiling, else
 *      q_m = (uint32_t)(((double)ceiling / a_m) * 2^30): one division, one exact scaling, truncated.  q_m = ONE wherever p_m = 0.
 *   3. sliding minimum.  m_k = min q_j, j in [k - release, k + attack].
 *   4. sliding mean.  s_n = floor((sum of m_k, k in [n - attack, n + release]) / W) in 64-bit integers.  Every window of step 3 that
 *      enters this sum contains n, so s_n <= q_n: the gain has fallen to what a peak needs when the peak arrives; it falls over `attack`
 *      samples and rises over `release` samples, in straight ramps.
 *   5. apply, for all n in [0, T * hop): out_n = (float)(((double)wav_n * (double)gain) * ((double)s_n * 2^-30)).  wav_n is used as
 *      stored (what is not finite passes through IEEE arithmetic); the tail behind N is scaled and not measured.
 *   6. report.  true_peak_after, sample_peak_after: step 1 on out over [0, N).  min_gain = (float)((double)min s_n * 2^-30) over n in
 *      [0, N) (1 where N = 0); limited_samples counts the n in [0, N) with s_n < ONE; true_peak_*_dbtp as in loudness step 6 and
 *      reduction_db = (float)(20 * (L(min s_n * 2^-30) * log10 e)), -inf where min s_n = 0.
 * THE PROMISE: every finite |out_n|, n in [0, N), is at most ceiling.  fl(|wav_n| gain) <= a_n because p_n >= |x'_n| and rounding is
 * monotonic; s_n 2^-30 <= q_n 2^-30 <= fl(ceiling / a_n) <= (ceiling / a_n)(1 + 2^-53); so the f64 product of step 5 passes ceiling by
 * at most a few units of 2^-52 relative, and since ceiling is an f32 value, whose upper neighbour lies 2^-23 relative above it, the
 * rounding to f32 brings the product back to it.  true_peak_after <= ceiling is NOT promised: a gain that varies in time moves the
 * peaks between the samples a little.
 * csrc/limiter.h holds the rule as plain C++ with a host reference, limit_reference(); tests/limiter_rule.py restates it in numpy.
 *
 * Arguments: gain finite in [0, 1000] (applied ahead of the limiter: pass the gain a target-only zv_loudness_wave returned); ceiling
 * in (0, 1], linear; attack in [1, 2047] and release in [1, 6144] samples; flags 0; wav, res and out (or every entry of theirs)
 * non-NULL — a limiter without an output is the true-peak meter of zv_loudness_wave; 0 < T <= zv_max_frames(); n_frames beyond T counts
 * as T.  ask == NULL is the identity for every utterance: gain 1, ceiling 1 and zv_limit_design's defaults for the model's rate.
 * zv_limit_design: attack = floor(attack_ms * sampling_rate / 1000 + 0.5) in f64, brought into [1, 2047], release likewise into
 * [1, 6144]; 0 ms means the default, 1.5 ms and 60 ms; negative or non-finite milliseconds and a rate outside 4 000 .. 768 000 are refused.
 * Not covered: more than one channel; a ceiling on the true peak AFTER the limiter; a stage of the zv_synthesize* chain. */
typedef struct
{
    float    gain;                  /* linear, applied ahead of the limiter */
    float    ceiling;               /* linear, in (0, 1] */
    uint32_t attack, release;       /* samples */
    uint32_t flags;                 /* 0 */
} zv_limiter;
typedef struct
{
    double   true_peak_before, true_peak_after;     /* linear */
    uint64_t limited_samples;
    float    sample_peak_before, sample_peak_after;
    float    min_gain;
    float    true_peak_before_dbtp, true_peak_after_dbtp, reduction_db;
} zv_limit_result;
zv_status zv_limit_design(uint32_t sampling_rate, float attack_ms /* 0: 1.5 */, float release_ms /* 0: 60 */, uint32_t *attack,
                          uint32_t *release);
zv_status zv_limit_wave(zv_model *m, const float *wav, uint32_t T, uint32_t n_frames, const zv_limiter *ask, zv_limit_result *res,
                        float *out /* [T * hop] */);
zv_status zv_limit_wave_batch(zv_model *m, uint32_t n_utt, const float *const *wav, const uint32_t *T,
                              const uint32_t *n_frames /* NULL = T */, const zv_limiter *ask /* [n_utt] or NULL */,
                              zv_limit_result *res /* [n_utt] */, float *const *out /* [n_utt], every entry [T * hop] */);
/* ---- resampling: sample-rate conversion and PCM16 delivery, the step behind the limiter --------------------------------------------------
 * The delivery chain filter -> loudness -> limiter ends in f32 at the model's rate; what a caller ships is 8 or 16 kHz for telephony,
 * 44.1 or 48 kHz for video and broadcast, as 16-bit PCM with dither.  zv_resample_wave takes a host waveform of S_in SAMPLES (not
 * frames: a recording is no multiple of the model's hop) and returns it at another rate as f32, as PCM16 or both; zv_resample_wave_batch
 * takes n_utt of them under ONE ask, one launch per kernel per launch group of consecutive utterances (cut as for
 * zv_loudness_wave_batch, over the padded input plus output samples), and utterance u dithers with seed + u and receives exactly the
 * bits of its single call with that seed.  Both run eagerly on lane 0, are never part of a captured graph or of the zv_synthesize*
 * chain, and use scratch of lane 0's arena.  The same call is the way in: a recording at 44.1 or 48 kHz is brought to the model's rate
 * before zv_mel_wave, zv_loudness_wave or zv_limit_wave see it.  zv_resample_design, zv_resample_count and zv_write_wav_pcm16 are host
 * only.
 *
 * THE RULE is a rational polyphase FIR.  Nothing in it is recursive along time, so nothing depends on how the work is split.
 * g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g; the table h[L][P] is f32 and P is even; half = P / 2; x[0 .. S_in) is
 * the input.
 *   count.   n_out = floor((S_in L + M - 1) / M) in 64-bit integers (zv_resample_count): the outputs whose time n M / L lies inside
 *            [0, S_in).  zv_resample_count takes any S_in: it returns 0 where M is 0 and 2^64 - 1 where S_in L + M - 1 does not fit 64
 *            bits (S_in above about 2^64 / L); the entry points bound S_in by zv_max_frames() * hop, far below.
 *   span.    x'[j] = x[j] where 0 <= j < S_in and the sample is finite, else +0.0: the waveform filter's span rule.  It never reads
 *            another utterance's samples.
 *   sample.  For 0 <= n < n_out: t = n M (64-bit), i0 = t div L, p = t mod L; acc = +0.0 (double); for k = 0 .. P - 1 ascending:
 *            acc = acc + (double)h[p][k] * (double)x'[i0 - half + 1 + k]; y[n] = (float)acc.  A product of two f32 values is exact in
 *            f64, so each step is one IEEE addition whether or not it is fused.  The ascending order is part of the rule.  Output n
 *            sits at input time n M / L with no delay, so frame and phoneme timings scale by L / M and keep pointing at the right samples.
 *   PCM16    (only where a pcm output is asked for), per output, each step one IEEE f64 operation: z = (double)y[n] * 32768.0.  With
 *            dither (flag bit 0): r = seed + (uint32_t)n * 0x9E3779B9; r ^= r >> 16; r *= 0x7feb352d; r ^= r >> 15; r *= 0x846ca68b;
 *            r ^= r >> 16 (all mod 2^32); d = ((double)((r & 0xFFFF) + (r >> 16)) - 65535.0) * 2^-16 — TPDF with zero mean, +-1 LSB —
 *            and z = z + d.  Then z = z + 0.5; q = floor(z), clamped to [-32768, 32767].  A NaN gives 0.  `clipped` counts the clamped
 *            and the NaN samples.  Without the flag the dither step is left out entirely.
 *   report.  n_out; clipped, 0 where no pcm output is asked for; sample_peak, the largest finite |y[n]| as a maximum of bit patterns,
 *            like the level meter.
 * csrc/resample.h holds the rule as plain C++ with a host reference, resample_reference(); tests/resample_rule.py restates it in numpy.
 *
 * THE DESIGN (zv_resample_design: host only, no model, no device) is data to the rule.  With s = min(1, L / M): half = ceil(zeros / s),
 * P = 2 half.  For d = k - half + 1 - p / L: g(d) = s cutoff sinc(s cutoff d) I0(beta sqrt(1 - (d / half)^2)) / I0(beta), 0 where
 * |d| > half; sinc(v) = sin(pi v) / (pi v); I0 is the power series sum ((v / 2)^j / j!)^2 in f64, summed until a term falls below
 * 10^-17 of the sum.  Each phase row is divided by its own f64 sum — every phase has DC gain 1, a constant stays constant — and each
 * entry is then rounded to f32 once.  A field that is 0 means its default: zeros = 32, beta = 9.0, cutoff = 0.91 (the fraction of the
 * narrower Nyquist frequency at -6 dB).  Refused by name (ZV_ERR_ARG): rates outside 4 000 .. 768 000; L or M above 1 280;
 * max(L / M, M / L) above 8; zeros outside 4 .. 64; beta outside (0, 20]; cutoff outside (0, 1]; P above 512; L P above 65 536.
 * rate_in == rate_out is allowed and no special case: L = M = 1, a low-pass.  table == NULL returns the sizes only.
 * What the defaults give, measured on the prototype assembled from the f32 rows by an FFT of 2^22 .. 2^23 points, for 22050 -> 48000
 * (L 320, M 147, P 64), 22050 -> 8000 (160 / 441, P 178), 22050 -> 16000, 48000 -> 22050, 44100 -> 22050 and 22050 -> 44100: the stop
 * band, from the narrower Nyquist frequency upward, -90.0 .. -90.6 dB; the pass band, up to 0.82 of it, -0.00028 .. +0.00027 dB; the
 * level at 0.91 of it -6.00 .. -6.03 dB.
 *
 * Arguments: 1 <= S_in <= zv_max_frames() * hop; wav, ask and res non-NULL; at least one of out and pcm (in a batch: the array, and then
 * every entry of it); flags within bit 0.  ask->table == NULL asks for the design of (rate_in, rate_out, zeros, beta, cutoff), built on
 * the host at the first request and kept with the model.  A caller's table [L][P] travels with the call and is checked: finite entries,
 * the limits above and gcd(L, M) = 1; the rates are then not looked at.  Everything is refused by name before any work is enqueued.
 * zv_write_wav_pcm16 writes int16 samples as they are, a mono RIFF/WAVE file.
 * Not covered: more than one channel; arbitrary (irrational or time-varying) ratios; noise-shaped dither; a rung of the
 * zv_synthesize* chain (the chain's output stays f32 at the model's rate). */
typedef struct
{
    uint32_t     rate_in, rate_out, zeros;      /* the design's: looked at where table == NULL */
    float        beta, cutoff;
    const float *table;                         /* a caller's table [L][P], or NULL = the design */
    uint32_t     L, M, P;                       /* the caller's table's */
    uint32_t     flags;                         /* bit 0: TPDF dither */
    uint32_t     seed;
} zv_resample;
typedef struct
{
    uint64_t n_out, clipped;
    float    sample_peak;
} zv_resample_result;
uint64_t  zv_resample_count(uint64_t S_in, uint32_t L, uint32_t M);
zv_status zv_resample_design(uint32_t rate_in, uint32_t rate_out, uint32_t zeros /* 0: 32 */, float beta /* 0: 9 */, float cutoff /* 0: 0.91 */,
                             uint32_t *L, uint32_t *M, uint32_t *P, float *table /* [L][P], or NULL: the sizes only */);
zv_status zv_resample_wave(zv_model *m, const float *wav, uint64_t S_in, const zv_resample *ask, zv_resample_result *res,
                           float *out /* [n_out] or NULL */, int16_t *pcm /* [n_out] or NULL */);
zv_status zv_resample_wave_batch(zv_model *m, uint32_t n_utt, const float *const *wav, const uint64_t *S_in, const zv_resample *ask /* one */,
                                 zv_resample_result *res /* [n_utt] */, float *const *out /* [n_utt] or NULL */,
                                 int16_t *const *pcm /* [n_utt] or NULL */);
zv_status zv_write_wav_pcm16(const char *path, const int16_t *pcm, size_t n, uint32_t sampling_rate);
/* When the last batches ran on the GPU (measurement): for the most recent min(cap, batches begun, 64) batches, oldest first,
 * the times in ms — relative to the first one's start — at which the batch's first operation started and its last kernel
 * ended (HIP events on the lanes' streams; waits for every lane first).  The gaps of the union of [start, end] are the time the
 * GPU had no batch to work on: bench.py reports them as extra.gpu_idle_ms_per_step. */
zv_status zv_batch_timeline(zv_model *m, uint32_t cap, double *start_ms, double *end_ms, uint32_t *n);

/* longest single utterance in frames (buffer descriptors address one utterance with 32-bit byte offsets; at most
 * 32768 frames = 7.4 min of audio).  Longer T returns ZV_ERR_ARG; zv_vocode_stream has no such limit on the total. */
uint32_t  zv_max_frames(const zv_model *m);

/* the utterance the reference's ZeroVOXModel::eval() hard-codes (src/zerovox.cpp:204-314): 120 phoneme ids, 120
 * punctuation ids, a 528-float style vector.  Pointers to static data; any argument may be NULL. */
void      zv_demo_utterance(const int32_t **ids, const int32_t **puncts, const float **style, uint32_t *n_phonemes,
                            uint32_t *style_len);

/* ---- device-resident variants (inputs already in HBM) ------------------------------------------
 * zv_vocode_device / zv_decode_device enqueue on LANE 0's stream and return; zv_memcpy_h2d / _d2h copy on that same stream
 * (so they are ordered with those calls whatever lane a batch was last begun on) and wait for the copy; zv_synchronize waits
 * for EVERY lane.  zv_profile_begin / _end bracket work of the synchronous entry points (lane 0). */
void     *zv_device_alloc(zv_model *m, size_t bytes);
void      zv_device_free(zv_model *m, void *p);
zv_status zv_memcpy_h2d(zv_model *m, void *dst, const void *src, size_t bytes);
zv_status zv_memcpy_d2h(zv_model *m, void *dst, const void *src, size_t bytes);
zv_status zv_vocode_device(zv_model *m, const float *d_mel, uint32_t T, float *d_wav);
zv_status zv_decode_device(zv_model *m, const float *d_hidden, const float *d_style, uint32_t T, float *d_mel);
zv_status zv_synchronize(zv_model *m);
/* capture the vocoder schedule for a given T into a hipGraph and replay it on later calls with the
 * same (T, d_mel, d_wav); 0 turns graph replay off */
zv_status zv_set_graph_mode(zv_model *m, int on);
/* The cache of captured graphs.  With graph mode on, a call that is not being profiled looks its graph up and replays it, or captures
 * it first.  KEY: the entry point's kind, the lane, the switch epoch (every zv_debug_set advances it), the batch's capacities
 * (utterances, longest phoneme count rounded up to 32, longest frame capacity rounded up to 64), which options the call carries and
 * the lane's buffers it runs on.  The utterances' real lengths and every option's VALUES are read at run time and key nothing.
 * VICTIM: the cache holds `capacity` graphs (16 by default).  A capture that finds it full removes exactly one: a graph of an older
 * switch epoch if there is one (it can never be replayed again), otherwise the graph replayed or captured least recently; among
 * several candidates the least recently used.  A lane that regrows its activation arena or one of its I/O blocks loses its own graphs,
 * the other lanes keep theirs.  EVICTION WAITS FOR NO LANE: the removed graph is destroyed once the lane that replays it has passed
 * an event recorded at that moment, which later captures check; only when more than `capacity` graphs wait like that does a capture wait,
 * for the oldest of them alone.  A replay adds no event, no wait and no allocation.  Turning graph mode off keeps the graphs.
 * The waveform's bits do not depend on whether a call was captured, replayed or run eagerly.
 * zv_graph_stats, counts since zv_model_load:
 *   capacity         the slots of the cache
 *   entries          graphs held now, <= capacity
 *   retired          graphs removed from the cache and not yet destroyed, <= capacity
 *   lookups          calls that went through the cache (graph mode on, not profiling); a synthesize call is one or two of them
 *   hits             lookups that replayed a held graph
 *   captures         lookups that captured a new one
 *   evictions        graphs of the current switch epoch removed as the least recently used (a full cache, or a smaller capacity)
 *   stale_evictions  graphs of an older switch epoch removed for the same reasons
 *   lane_drops       graphs removed because their lane regrew its arena or a block
 *   full_drops       graphs removed when everything goes (zv_model_free)
 * Always: lookups = hits + captures, and captures = entries + evictions + stale_evictions + lane_drops + full_drops.
 * zv_set_graph_cache: capacity 1 .. 1024, anything else is ZV_ERR_ARG ("graph cache capacity") and changes nothing; a smaller capacity
 * evicts by the victim rule until the cache fits.  zv_graph_cache_stats waits for nothing and touches no stream. */
typedef struct
{
    uint32_t capacity, entries, retired, reserved; /* reserved = 0 */
    uint64_t lookups, hits, captures, evictions, stale_evictions, lane_drops, full_drops;
} zv_graph_stats;
zv_status zv_set_graph_cache(zv_model *m, uint32_t capacity);
zv_status zv_graph_cache_stats(zv_model *m, zv_graph_stats *out);

/* ---- stages in batches -------------------------------------------------------------------- */
/* The three stage calls over a batch: what zv_synthesize_batch does for the chain — row-concatenated tensors, a segment table in HBM,
 * one launch per kernel, launch groups of at most 64 utterances / 64 Ki frames of capacity, a captured graph in graph mode — for one
 * stage at a time.  For a caller that must know the frame counts before it picks capacities, a caller whose mels come from elsewhere,
 * a caller that wants a batch's hidden or mel.  Utterance u's result is, bit for bit, that of the single call on its arguments:
 *   zv_encode_batch   hidden, n_frames and durations of zv_encode_taps_target(m, ids[u], puncts[u], styles[u], n_phonemes[u],
 *                     n_phonemes[u], T[u], hidden[u], &n_frames[u], NULL x 6, &prosody[u], &phonemes[u], durations[u],
 *                     target_frames[u]), with that call's NULL conventions (prosody, phonemes, durations, target_frames, each NULL =
 *                     none; an entry of durations may be NULL); n_frames and durations are also those zv_synthesize_batch_target
 *                     gives for the same arguments.  hidden == NULL, or hidden[u] == NULL, is the PLANNING call: that utterance's
 *                     hidden is neither staged nor downloaded, and with every hidden NULL only the frame counts (and the scan, where
 *                     durations are asked for) travel to the host — the frame counts of a batch ahead of its synthesis, for fitted
 *                     capacities, subtitle layout or slot fitting.
 *   zv_decode_batch   mel of zv_decode(m, hidden[u], styles[u], T[u], mel[u]): the statistics cover exactly T[u] rows, and as for
 *                     every stand-alone decode there is no run table (the hidden is the caller's).
 *   zv_vocode_batch   wav of zv_vocode(m, mel[u], T[u], wav[u]); a padded tail is run-shortened as in any batch, and a batch whose
 *                     waveforms reach 16 MiB runs its last stage in utterance groups whose downloads overlap the next group's kernels.
 * zv_vocode_batch_begin / _end are the two halves on lane `lane` (< ZV_BATCH_LANES), as zv_synthesize_batch_begin / _end: one launch
 * group (else ZV_ERR_ARG), mel[], T[], wav[] and their targets valid until _end, the bits of the synchronous call.  A lane holds one
 * batch in flight of either kind, and each kind has its own _end: zv_synthesize_batch_end on a vocode batch, zv_vocode_batch_end on a
 * synthesize batch or on an idle lane is ZV_ERR_ARG and leaves the lane as it is.
 * Every argument is checked before anything is enqueued (ZV_ERR_ARG; the message names the entry point, the utterance and the
 * argument): a NULL array or entry other than the optional ones above, n_utt == 0, n_phonemes[u] == 0, T[u] == 0 or above
 * zv_max_frames(), and for zv_encode_batch the ids and controls as zv_synthesize_batch_target checks them.
 * No waveform stage (volume ... filter) is taken here, and the tensors are the host's. */
zv_status zv_encode_batch(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                          const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T,
                          float *const *hidden,            /* NULL, or [n_utt] of which each may be NULL: not downloaded */
                          uint32_t *n_frames,              /* [n_utt] */
                          const zv_prosody *prosody, const zv_phoneme_controls *phonemes, int32_t *const *durations,
                          const uint32_t *target_frames);
zv_status zv_decode_batch(zv_model *m, uint32_t n_utt, const float *const *hidden, const float *const *styles, const uint32_t *T,
                          float *const *mel);
zv_status zv_vocode_batch(zv_model *m, uint32_t n_utt, const float *const *mel, const uint32_t *T, float *const *wav);
zv_status zv_vocode_batch_begin(zv_model *m, uint32_t lane, uint32_t n_utt, const float *const *mel, const uint32_t *T,
                                float *const *wav);
zv_status zv_vocode_batch_end(zv_model *m, uint32_t lane);

/* ---- measurement ------------------------------------------------------------------------ */
/* per-kernel-family timing measured with HIP events on the model's stream (eager launches).  algo_bytes / algo_flops are
 * priced by CAPACITY rows, also for a fitted call (whose kernels do less than that when n_frames < T); the vocoder launches of
 * a run-shortened pass (zv_vocode) are priced by the rows its run table holds, read back once per profiled pass */
typedef struct
{
    char     name[48];
    uint32_t launches;
    double   total_ms;
    double   algo_bytes;       /* algorithmic bytes moved by those launches */
    double   algo_flops;
} zv_kernel_stat;
zv_status zv_profile_begin(zv_model *m);
/* stops profiling, copies up to cap entries, returns the entry count in *n */
zv_status zv_profile_end(zv_model *m, zv_kernel_stat *stats, uint32_t cap, uint32_t *n);

/* ---- one layer at a time (tests) — the counterpart of the reference's tensor_dbg (src/utils.cpp:19-44): runs ONE layer of
 * the production schedule on a caller-supplied input, so a per-layer comparison against the reference semantics does not
 * compound.  x [rows][cin] and out [rows][cout] are host, time-major, unpadded; rows are rows at the layer's own rate.
 *   ZV_LAYER_VOC_RESBLOCK  index n = stage * num_resblocks + branch: HiFiGANResidualBlock n (src/hifigan.cpp:74-185), fused
 *                          kernels; rows must be a multiple of the stage's samples per frame
 *   ZV_LAYER_ENC_FFT       index l: FFTBlock l = attention sublayer + conv FFN (src/fs2encoder.cpp:71-140,174-228)
 *   ZV_LAYER_DEC_BLOCK     index 0,1: ResBlk1d encode.{0,1}; 2..6: AdainResBlk1d decode.{0..4} with `style`
 *                          (src/stylettsdec.cpp:69-149,242-304); cin as the reference (decode.0..2 take the 2E+64 concat)
 *   ZV_LAYER_VAR_PRED      index 0 duration / 1 pitch / 2 energy: VariancePredictor (src/fs2encoder.cpp:386-440), out [rows]
 *   ZV_LAYER_VOC_UPSAMPLE  index i: leaky_relu(0.1) + conv_transpose1d i (src/hifigan.cpp:22-71,281-297); x [rows][Cin] at the
 *                          stage's INPUT rate (rows a multiple of it), out [rows * scale_i][Cout]
 *   ZV_LAYER_VOC_INPUT     mel normalisation + input conv k7 (src/hifigan.cpp:242-265): x [T][num_mels] -> out [T][channels]
 *   ZV_LAYER_VOC_OUTPUT    leaky_relu(0.01) + output conv k7 + tanh (src/hifigan.cpp:324-345): x [T * hop][C_last] (the MRF mean)
 *                          -> out [T * hop]
 *   ZV_LAYER_DEC_ASR_RES   asr_res: conv 1x1 + InstanceNorm (src/stylettsdec.cpp:382-396): x [T][E] -> out [T][64]
 *   ZV_LAYER_DEC_TO_OUT    to_out: conv 1x1 + bias (src/stylettsdec.cpp:432-441): x [T][E] -> out [T][num_mels]
 *   ZV_LAYER_ENC_EMBED     word + punctuation embedding + positional encoding (src/fs2encoder.cpp:306-324): x [N][2] = (phoneme id,
 *                          punctuation id) as floats -> out [N][E]
 *   ZV_LAYER_ENC_MHA       index l: MultiHeadAttention l alone, with its residual + LayerNorm (src/fs2encoder.cpp:71-140)
 *   ZV_LAYER_ENC_FFN       index l: PositionwiseFeedForward l alone, with its residual + LayerNorm (src/fs2encoder.cpp:174-228)
 *   ZV_LAYER_DEC_ADAIN     index 2 * b + (norm - 1): AdaIN1d norm1 / norm2 of AdainResBlk1d decode.b alone, with `style`
 *                          (src/stylettsdec.cpp:171-200): x [T][C] -> out [T][C], C = the block's cin (norm1) / cout (norm2)
 *   ZV_LAYER_ENC_LN        index 2 * l + j: the LayerNorm of FFT block l's attention (j = 0) / feed-forward (j = 1) sublayer alone,
 *                          x being its input (src/fs2encoder.cpp:132-137, 219-224): x [N][E] -> out [N][E] */
typedef enum { ZV_LAYER_VOC_RESBLOCK = 0, ZV_LAYER_ENC_FFT = 1, ZV_LAYER_DEC_BLOCK = 2, ZV_LAYER_VAR_PRED = 3,
               ZV_LAYER_VOC_UPSAMPLE = 4, ZV_LAYER_VOC_INPUT = 5, ZV_LAYER_VOC_OUTPUT = 6, ZV_LAYER_DEC_ASR_RES = 7,
               ZV_LAYER_DEC_TO_OUT = 8, ZV_LAYER_ENC_EMBED = 9, ZV_LAYER_ENC_MHA = 10, ZV_LAYER_ENC_FFN = 11,
               ZV_LAYER_DEC_ADAIN = 12, ZV_LAYER_ENC_LN = 13 } zv_layer_kind;
zv_status zv_debug_layer(zv_model *m, int kind, int index, const float *x, uint32_t rows, const float *style, float *out);
/* Tests: one matrix-core accumulation chain at instruction level — out[32][32] = c0[32][32] + a[32][K] . b[K][32] (host, row-major)
 * by ONE wave, every element one k-ordered chain on the instruction the product's kernels accumulate with:
 *   form 0  v_mfma_f32_32x32x16_f16 (single-utterance and generic conv kernels): a, b are f16 (uint16 bit patterns)
 *   form 1  v_mfma_f32_16x16x32_f16 (batch kernels), as four 16x16 tiles: a, b f16
 *   form 2  v_mfma_f32_32x32x2_f32 (f32 linear layers, attention): a, b f32
 * The promise "batch == stand-alone, streamed == whole, bit for bit" rests on forms 0 and 1 giving the same bits
 * (tests/test_gpu_mfma_chain.py measures it on operands that span the f16 range).  K a multiple of 32, at most 4096, else ZV_ERR_ARG. */
zv_status zv_debug_mfma_chain(zv_model *m, int form, const void *a, const void *b, const float *c0, uint32_t K, float *out);

/* ---- test / measurement switches (none is needed in production; no reference counterpart: the reference's only run-time
 * switch is the thread count, src/zerovox.cpp:86-91).  The shipped library never reads the environment: a switch changes
 * only through this call (the Python test binding forwards ZV_* environment variables through it so that a shell script can
 * A/B a run).  Every switch is read at every call, where the schedule is decided: one set on a live model holds from its
 * next call on (ZV_ARENA_FILL keeps its meaning, the byte a fresh arena gets when it is allocated: it reaches the arenas
 * allocated after it is set); a captured hipGraph replays the regime it was captured in, so every call of zv_debug_set
 * makes the models capture anew.  name == NULL resets every switch to its built-in default.  ZV_ERR_ARG for an unknown
 * name.  The list: zerovox.cpp_amd/csrc/knobs.h (timing-only ablation switches that give wrong results exist only in
 * diagnostic builds, -DZV_DIAG).  zv_debug_get reads a switch. */
zv_status zv_debug_set(const char *name, int value);
zv_status zv_debug_get(const char *name, int *value);
/* Tests: the run table of the most recent vocoder pass on `lane` (run-shortened vocoding, see zv_vocode), after waiting for the
 * lane: up to cap entries of four int32 each — {first row of the utterance in the batch, frames vocoded, split frame, frames
 * skipped} — and in *n how many utterances the table has, 0 when that pass ran without one
 * or when the lane's buffers were reallocated since.  Valid until the lane's next call.  The selected lane stays selected. */
zv_status zv_debug_voc_runs(zv_model *m, uint32_t lane, int32_t *table, uint32_t cap, uint32_t *n);
/* Tests: overwrite what `lane` keeps between calls, so that a comparison of two calls on one lane can see a write that did not
 * happen.  Waits for the lane's stream and copy stream, then fills with `byte` (0..255) the whole capacity of the lane's activation
 * arena and device I/O block (on the lane's own stream, then waits) and of its pinned staging block; filled[3] (may be NULL)
 * receives the bytes filled in the three, 0 for a block not yet allocated (a lane never used: ZV_OK, all 0).  Allocates nothing and
 * leaves captured graphs alone (their pointers stay valid: a replay must work on poisoned buffers); the lane's run table
 * (zv_debug_voc_runs) is forgotten until its next call.  ZV_ERR_ARG, and nothing is touched, while the lane has a batch in flight,
 * for lane >= ZV_BATCH_LANES and for a byte outside 0..255.  Not a switch: no graph is captured anew.  The selected lane stays
 * selected. */
zv_status zv_debug_poison(zv_model *m, uint32_t lane, int byte, size_t filled[3]);

/* ---- GGUF inspection without a device (loader half of the boundary; used by the CPU test-suite) ----
 * Parses the file exactly as zv_model_load does and reports the counts; *max_seq_len receives the
 * `<arch>.max_seq_len` KV.  tensor_index >= 0 additionally returns that tensor's name (<= 63 chars + NUL),
 * ggml type code and shape (ne[4], missing dims = 1). */
zv_status zv_gguf_inspect(const char *gguf_path, uint32_t *n_tensors, uint32_t *max_seq_len, int tensor_index,
                          char *name_out, uint32_t *type_out, int64_t *ne_out);

/* ---- "next" row f-2: WAV writer (PCM16 mono, 44-byte RIFF header) --------------------------- */
zv_status zv_write_wav(const char *path, const float *wav, size_t n_samples, uint32_t sampling_rate);

#ifdef __cplusplus
}
#endif
#endif
