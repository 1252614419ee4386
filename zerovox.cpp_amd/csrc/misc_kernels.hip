// misc_kernels.hip — the non-conv kernels of the fixed schedule compiled as ONE translation unit, a file per kernel family, in the
// order they always had; conv_kernels.hip says why families compile together.  Every kernel maps a workgroup to (segment, tile inside
// the segment) — see `Segs` in kernels.h — so one launch covers all utterances of a batch while each utterance keeps its own extents.
#include "norm_kernels.hip"           // InstanceNorm statistics and operand passes
#include "encoder_kernels.hip"        // linear, embedding, attention, LayerNorm, variance-adaptor rows
#include "regulator_kernels.hip"      // length regulator, target durations, fitted mode's frame table
#include "runs_kernels.hip"           // run tables of vocoder and decoder
#include "level_kernels.hip"          // level meter
#include "envelope_kernels.hip"       // amplitude envelope
#include "contour_kernels.hip"        // level contour
#include "pitch_kernels.hip"          // pitch track
#include "bands_kernels.hip"          // band levels
#include "filter_kernels.hip"         // waveform filter
#include "mel_kernels.hip"            // mel analysis
#include "align_kernels.hip"          // mel alignment
#include "loudness_kernels.hip"       // loudness
#include "limiter_kernels.hip"        // limiter
#include "resample_kernels.hip"       // resampling
#include "mfma_chain_kernel.hip"      // test-only MFMA chain
