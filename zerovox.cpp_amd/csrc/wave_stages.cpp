// wave_stages.cpp — the launches of the waveform stages behind the vocoder's output convolution (wave_stages.h, see model.h): filter,
// envelope, volume, contour, pitch track, band levels, in that order, each only where the call carries it.
#include "schedule.h"

#include <algorithm>
#include <vector>

namespace zv
{

// bt's segments are final in d_wav (with a filter: in the filter-input region); per tail group, seg0 the group's first segment in the batch
void Model::wave_stage_launches(const Batch &bt, const VocLayout &lay, float *d_wav, int rate, int seg0)
{
    const WaveStages &w = bt.wave;
    if (const char *what = w.inconsistent(bt.d_cum)) fail(ZV_ERR_DEVICE, "%s", what);
    const Segs cap = bt.frames_cap();
    const Segs tk{bt.d_tok ? bt.d_tok + seg0 : nullptr, bt.nseg, bt.n_max, bt.tok1};
    const double cap_rows = std::min((double)bt.t_rows, (double)bt.t_max * bt.nseg);
    const double tok_rows = std::min((double)bt.n_rows, (double)bt.n_max * bt.nseg);
    const double cap_samples = cap_rows * rate;

    // Waveform filter (filter.h): the output convolution wrote the filter-input region (vocode_group), the filter writes d_wav.
    // Algorithmic bytes: the capacity read and written once.  Operations, by capacity and at 255 taps (the counts are the device's: a
    // caller's taps change the work, not this price): 2 per multiply-add.
    if (w.d_flt_par)
        ZV_LAUNCH("voc_filter", 8.0 * cap_samples, 2.0 * 255.0 * cap_samples,
                  launch_filter(stream(), lay.filter_in, d_wav, w.d_flt_par, cap, bt.frames(), rate));

    // Amplitude envelope (envelope.h): knots from the regulator's scan, then scale — ahead of the volume passes, which measure the result.
    if (w.d_env)
    {
        // (the hop was checked with the request, capi.cpp check_request; launch_env_apply refuses any other)
        // Segment u of THIS call keeps its knots at row0 + u + f, u counted from the call's first segment: consecutive tail groups write
        // overlapping ranges of the table.  That is sound only because a group's knots pass and apply pass run back to back on the lane's
        // one stream, ahead of the next group's; groups on streams of their own would need the batch's segment index (seg0 + u) here.
        if (bt.t_rows + (size_t)bt.nseg > env_knot_entries(bt)) fail(ZV_ERR_DEVICE, "internal: envelope knot table too small");
        // algorithmic bytes: the knots written (by capacity) and the scan and gains read once; the waveform read and written
        ZV_LAUNCH("voc_env_knots", 4.0 * (cap_rows + bt.nseg) + 8.0 * tok_rows, 0.0,
                  launch_env_knots(stream(), bt.d_cum, w.d_env_gain, w.d_env, w.d_nframes, lay.env_knots, tk, cap));
        ZV_LAUNCH("voc_env_apply", 8.0 * cap_rows * rate, 0.0, launch_env_apply(stream(), d_wav, w.d_nframes, lay.env_knots, w.d_env, cap, rate));
    }

    // Volume controls (level.h): measure the speech and scale the capacity.
    if (w.d_vol)
    {
        if ((size_t)bt.nseg * level_chunks(cap.max_rows, rate) > level_slab_entries(bt)) fail(ZV_ERR_DEVICE, "internal: level slab too small");
        double speech_samples = cap_samples;
        if (profiling && !skip_launch_)
        {
            // the profile states bytes moved: the speech the regulator produced (this path is eager and the host waits anyway)
            std::vector<int32_t> nf((size_t)bt.nseg);
            ZV_HIP(hipMemcpyAsync(nf.data(), w.d_nframes, nf.size() * 4, hipMemcpyDeviceToHost, stream()));
            ZV_HIP(hipStreamSynchronize(stream()));
            speech_samples = 0;
            for (int32_t f : nf) speech_samples += (double)std::min(std::max(f, 0), bt.t_max) * rate;
        }
        ZV_LAUNCH("voc_level_measure", 4.0 * speech_samples, 0.0, launch_level_measure(stream(), d_wav, w.d_nframes, lay.level_slab, cap, rate));
        ZV_LAUNCH("voc_level_apply", 8.0 * cap_samples, 0.0,
                  launch_level_apply(stream(), d_wav, w.d_nframes, lay.level_slab, w.d_vol, w.d_levels, cap, rate));
    }

    // Level contour (contour.h): behind the envelope and the volume passes, so it meters the waveform the caller receives.
    if (w.d_ctr_frames)
    {
        // Slab entries and rows sit at a segment's ABSOLUTE frame row (the table's row0, which a sub-batch keeps) and absolute token
        // row: consecutive tail groups write disjoint ranges.  Unlike the envelope's knot table this relies on no order between the
        // groups, only on the phonemes pass running behind the frames pass of its own group on the lane's stream.
        // algorithmic bytes: the capacity's samples read once; the slab entries read (by capacity) and the phoneme rows written
        ZV_LAUNCH("voc_contour_frames", 4.0 * cap_rows * rate, 0.0, launch_contour_frames(stream(), d_wav, lay.contour_slab, w.d_ctr_frames, cap, rate));
        ZV_LAUNCH("voc_contour_phonemes", 16.0 * cap_rows + 8.0 * tok_rows, 0.0,
                  launch_contour_phonemes(stream(), bt.d_cum, lay.contour_slab, w.d_ctr_phonemes, tk, cap, rate));
    }

    // Pitch track (pitch.h): behind everything that changes the waveform, like the contour and with its indexing.
    if (w.d_pit_frames)
    {
        // algorithmic bytes: the capacity's samples read once, a slab entry and a row written per frame; the slab read and a row written
        // per token.  Operations, by capacity and at the DEFAULT parameters (the values are the device's: a caller's lags change the
        // work, not this price): 2 per multiply-add, window x (max_lag - min_lag + 3) multiply-adds per frame.
        const double macs = 2.0 * (double)rate * (double)(hp.audio_sampling_rate / 63 - hp.audio_sampling_rate / 441 + 3);
        ZV_LAUNCH("voc_pitch_frames", 4.0 * cap_rows * rate + 16.0 * cap_rows, 2.0 * macs * cap_rows,
                  launch_pitch_frames(stream(), d_wav, lay.pitch_slab, w.d_pit_frames, w.d_pit_par, cap, rate, (int)hp.audio_sampling_rate));
        ZV_LAUNCH("voc_pitch_phonemes", 8.0 * cap_rows + 8.0 * tok_rows, 0.0,
                  launch_pitch_phonemes(stream(), bt.d_cum, lay.pitch_slab, w.d_pit_phonemes, tk, cap));
    }

    // Band levels (bands.h): behind the pitch track's passes, with their indexing.
    if (w.d_bnd_frames)
    {
        // algorithmic bytes: the capacity's samples read once, the table once per tile of frames, a slab row and a row written per
        // frame; the slab read and a row written per token.  Operations: 2 per 8-bit multiply-add, both digit planes, 1 026 columns.
        const double row_b = (double)BANDS_ROW_STRIDE;
        ZV_LAUNCH("voc_bands_frames", 4.0 * cap_rows * rate + (double)BANDS_TABLE_BYTES * cap_rows / BANDS_TILE_FRAMES + 12.0 * row_b * cap_rows,
                  2.0 * 2.0 * (double)BANDS_N * 2.0 * BANDS_BINS * cap_rows,
                  launch_bands_frames(stream(), d_wav, w.d_bnd_table, w.d_bnd_slab, w.d_bnd_frames, w.d_bnd_par, cap, rate));
        ZV_LAUNCH("voc_bands_phonemes", 8.0 * row_b * cap_rows + 4.0 * row_b * tok_rows, 0.0,
                  launch_bands_phonemes(stream(), bt.d_cum, w.d_bnd_slab, w.d_bnd_phonemes, w.d_bnd_par, tk, cap));
    }
}

// Mel analysis (mel.h): no stage of the chain — the stand-alone entry points' two launches over a waveform the caller brought.
void Model::mel_launches(const float *d_wav, double *d_slab, float *d_rows, const uint32_t *d_par, const Segs &frames, size_t total_rows)
{
    const int hop = (int)hp.audio_hop_size, M = (int)hp.audio_num_mels;
    const double rows = (double)total_rows;
    // algorithmic bytes: the samples read once, the table once per tile of frames, a slab row written per frame; the slab read, the
    // weights once and a row written per frame.  Operations: 2 per 8-bit multiply-add, four digit-plane products, 1 026 columns.
    ZV_LAUNCH("mel_frames", 4.0 * rows * hop + (double)MEL_TABLE_BYTES * rows / MEL_TILE_FRAMES + 8.0 * MEL_SLAB_STRIDE * rows,
              2.0 * 4.0 * (double)BANDS_N * 2.0 * BANDS_BINS * rows,
              launch_mel_frames(stream(), d_wav, mel_table(), d_slab, d_par, frames, hop, M));
    ZV_LAUNCH("mel_rows", 8.0 * MEL_SLAB_STRIDE * rows + 4.0 * M * (rows + BANDS_BINS), 0.0, launch_mel_rows(stream(), d_slab, d_rows, d_par, frames, hop, M));
}

// Mel alignment (align.h): no stage of the chain either — the stand-alone entry points' five launches over one launch group of pairs.
void Model::align_launches(const AlignJob &job, size_t n_rows, size_t n_cells)
{
    const double rows = (double)n_rows, cells = (double)n_cells, M = job.M, K = align_k(job.M);
    // algorithmic bytes: the rows read once per pass, the planes and norms written once; the planes read once per tile row / column (an
    // upper estimate: rows * K * 2 per 64 cells' side), a u32 per cell; dp reads it and writes a byte; the walk is the path only.
    // Operations: 2 per 8-bit multiply-add, four digit-plane products, K channels per cell.
    ZV_LAUNCH("align_means", job.normalise ? 4.0 * rows * M : 0.0, 0.0, launch_align_means(stream(), job));
    ZV_LAUNCH("align_quant", 4.0 * rows * M + 2.0 * rows * K + 4.0 * rows, 0.0, launch_align_quant(stream(), job));
    ZV_LAUNCH("align_cost", 4.0 * cells + 2.0 * 2.0 * K * cells / ALIGN_TILE, 2.0 * 4.0 * K * cells, launch_align_cost(stream(), job));
    ZV_LAUNCH("align_dp", 5.0 * cells, 0.0, launch_align_dp(stream(), job));
    ZV_LAUNCH("align_walk", 5.0 * rows, 0.0, launch_align_walk(stream(), job));
}

// Loudness (loudness.h): no stage of the chain either — the stand-alone entry points' launches over one launch group of utterances.
void Model::loud_launches(const LoudJob &job, bool apply, size_t samples, size_t capacity)
{
    const double n = (double)samples, chunks = n / LOUD_CHUNK;
    // algorithmic bytes: the samples read once per pass; a state (32 bytes) or two run sums (16) per chunk.  Operations: 16 f64 operations
    // per sample in phase A, two more for the square in phase C; 28 per chunk in phase B; 3 x 12 multiply-adds per sample for the true peak.
    ZV_LAUNCH("loud_chunks_a", 4.0 * n + 32.0 * chunks, 16.0 * n, launch_loud_chunks(stream(), job, false));
    ZV_LAUNCH("loud_states", 64.0 * chunks, 28.0 * chunks, launch_loud_states(stream(), job));
    ZV_LAUNCH("loud_chunks_c", 4.0 * n + 48.0 * chunks, 18.0 * n, launch_loud_chunks(stream(), job, true));
    ZV_LAUNCH("loud_peak", 4.0 * n, 2.0 * 36.0 * n, launch_loud_peak(stream(), job));
    ZV_LAUNCH("loud_gate", 16.0 * chunks, 0.0, launch_loud_gate(stream(), job));
    if (apply) ZV_LAUNCH("loud_apply", 8.0 * (double)capacity, (double)capacity, launch_loud_apply(stream(), job));
}

// Limiter (limiter.h): no stage of the chain either — the stand-alone entry points' launches over one launch group of utterances.
void Model::limit_launches(const LimitJob &job, size_t samples, size_t capacity, size_t entries)
{
    const double n = (double)samples, cap = (double)capacity, q = (double)entries;
    // algorithmic bytes: the measured samples read and a q written per entry; q read and m written; m and the samples read and the
    // output written; the output's measured span read.  Operations: 3 x 12 multiply-adds per sample for a peak pass and the required
    // gain's multiply and divide; three comparisons per entry and scan, two scans; three additions per entry and a 64-bit division and
    // four f64 operations per sample.
    ZV_LAUNCH("limit_peak", 4.0 * n + 4.0 * q, 2.0 * 36.0 * n + 2.0 * n, launch_limit_peak(stream(), job, false));
    ZV_LAUNCH("limit_min", 8.0 * q, 6.0 * q, launch_limit_min(stream(), job));
    ZV_LAUNCH("limit_mean", 12.0 * cap + 4.0 * q, 3.0 * q + 5.0 * cap, launch_limit_mean(stream(), job));
    ZV_LAUNCH("limit_peak_after", 4.0 * n, 2.0 * 36.0 * n, launch_limit_peak(stream(), job, true));
    ZV_LAUNCH("limit_reduce", 24.0 * q / LIMIT_TILE, 0.0, launch_limit_reduce(stream(), job));
}

// Resampling (resample.h): no stage of the chain either — the stand-alone entry points' launches over one launch group of utterances.
void Model::resample_launches(const ResampleJob &job, size_t in, size_t out)
{
    const double x = (double)in, y = (double)out, P = job.P;
    // algorithmic bytes: the input read once, the table once, the outputs written (4 and 2 bytes a sample); a pair of words per tile.
    // Operations: P f64 multiply-adds per output, and the dozen of the PCM16 conversion.
    ZV_LAUNCH("resample", 4.0 * x + 4.0 * job.L * P + (job.out ? 4.0 : 0.0) * y + (job.pcm ? 2.0 : 0.0) * y, 2.0 * P * y + (job.pcm ? 12.0 * y : 0.0),
              launch_resample(stream(), job));
    ZV_LAUNCH("resample_reduce", 8.0 * y / resample_tile_outputs(resample_tile(job.L, job.M, job.P)), 0.0, launch_resample_reduce(stream(), job));
}

}  // namespace zv
