// stage_range.h — which of the three stages a batch request runs, and which regions of its three blocks exist for that range.
// Pure host code: capi.cpp's batch_enqueue carves its blocks through batch_carve, tests/native/stage_range_check.cpp pins the carve on
// the CPU (every range: aligned, disjoint, nothing carved that the range does not touch; the full range: the offsets batch_enqueue had
// when it carved inline).
// A request of the full range is the chain zv_synthesize_batch* runs; the stage-batch entry points (zv_encode_batch, zv_decode_batch,
// zv_vocode_batch*) ask for one stage each.  ADDING A REGION: its id, its line in batch_region_bytes, its place in batch_carve.
#pragma once

#include "wave_stages.h"

namespace zv
{

enum StageId { ST_ENCODER, ST_DECODER, ST_VOCODER, ST_COUNT };

// stages [first, last] of encoder -> decoder -> vocoder
struct StageRange
{
    int first = ST_ENCODER, last = ST_VOCODER;
    constexpr bool valid() const { return ST_ENCODER <= first && first <= last && last <= ST_VOCODER; }
    constexpr bool has(int s) const { return first <= s && s <= last; }
    constexpr bool full() const { return first == ST_ENCODER && last == ST_VOCODER; }
    constexpr bool only(int s) const { return first == s && last == s; }
    // part of a captured graph's kind (Model::chain_dev): 0 for the full range, so the chain's graphs keep the kinds they had
    constexpr int key() const { return full() ? 0 : 1 + first * ST_COUNT + last; }
    // the tensor the range reads from the caller (first: -1 for the encoder, whose input is the token table) and the one it hands back,
    // as the stage that writes it: the encoder writes hidden, the decoder mel, the vocoder the waveform
    constexpr int source() const { return first - 1; }
    constexpr int result() const { return last; }
};

// A request's numbers, as batch_enqueue knows them before it carves: the capacities of the Batch, the model's row widths, which optional
// rows the request carries, and the exact bytes of what travels over the host (source: the caller's hidden or mel, all utterances;
// result: the rows of the utterances that want them back)
struct BatchShape
{
    size_t nseg = 1, n_rows = 0, t_rows = 0;      // capacities (Batch)
    size_t E = 0, mels = 0, hop = 0;              // floats of a hidden / mel / waveform frame
    bool   ctl = false, pctl = false;             // control rows, per-phoneme control rows
    bool   timings = false;                       // some utterance asks for its phoneme timings
    bool   fitted = false;
    size_t n_tokens = 0, n_frames = 0;            // what the utterances hold: the sum of their phonemes, of their frame capacities
    size_t source_bytes = 0, result_bytes = 0;
};

// floats of a frame row of the tensor stage `s` writes
constexpr size_t stage_row_floats(int s, const BatchShape &q) { return s == ST_ENCODER ? q.E : s == ST_DECODER ? q.mels : q.hop; }

enum BatchRegionId
{
    // the input block: built in pinned memory, uploaded in one copy (the first node of the schedule)
    BI_TOK, BI_FRM, BI_IDS, BI_PUN, BI_STY, BI_CTL, BI_PCTL,
    // the device block
    BD_NF, BD_IN, BD_HID, BD_MEL, BD_WAV, BD_CUM, BD_LIVE, BD_RUNS,
    // the pinned block
    BP_IN, BP_NF, BP_OUT, BP_CUM, BP_SRC,
    BR_COUNT
};

// sizeof(Seg) and the bytes of a CTL_STRIDE / PCTL_STRIDE row (kernels.h, which needs HIP); capi.cpp asserts that they agree
constexpr size_t SEG_BYTES = 16, CTL_ROW_BYTES = 32, PCTL_ROW_BYTES = 16;

// The bytes of a region for a range: zero where the range does not touch it.  in_bytes: the input block's size (BD_IN, BP_IN).
inline size_t batch_region_bytes(int id, const StageRange &r, const BatchShape &q, const WaveAsk &ask, size_t in_bytes)
{
    const bool enc = r.has(ST_ENCODER), dec = r.has(ST_DECODER), voc = r.has(ST_VOCODER);
    const size_t tab = (q.nseg + 1) * SEG_BYTES;      // one entry per utterance + one that spans all of them
    switch (id)
    {
    case BI_TOK: return enc ? tab : 0;
    case BI_FRM: return tab;
    case BI_IDS:
    case BI_PUN: return enc ? q.n_rows * 4 : 0;
    case BI_STY: return enc || dec ? q.nseg * q.E * 4 : 0;
    case BI_CTL: return enc && q.ctl ? q.nseg * CTL_ROW_BYTES : 0;
    case BI_PCTL: return enc && q.pctl ? q.n_rows * PCTL_ROW_BYTES : 0;
    case BD_NF: return enc ? q.nseg * 4 : 0;
    case BD_IN:
    case BP_IN: return in_bytes;
    case BD_HID: return enc || dec ? q.t_rows * q.E * 4 : 0;            // the encoder writes it, the decoder reads it
    case BD_MEL: return dec || voc ? q.t_rows * q.mels * 4 : 0;
    case BD_WAV: return voc ? q.t_rows * q.hop * 4 : 0;
    // the regulator's scan outside the arena: for the timings, or for a waveform stage behind the vocoder that reads it
    case BD_CUM: return enc && (q.timings || (voc && ask.needs_scan())) ? q.n_rows * 4 : 0;
    case BD_LIVE: return enc && dec && q.fitted ? q.nseg * SEG_BYTES : 0;           // written by the encoder, read from the decoder on
    case BD_RUNS: return enc && dec && !q.fitted ? tab : 0;                         // the decoder's run table: a chain's alone
    case BP_NF: return enc ? q.nseg * 4 : 0;
    case BP_OUT: return q.result_bytes;
    case BP_CUM: return enc && q.timings ? q.n_rows * 4 : 0;
    case BP_SRC: return r.first > ST_ENCODER ? q.source_bytes : 0;
    }
    return 0;
}

struct BatchOffsets
{
    size_t      at[BR_COUNT] = {};
    size_t      in_bytes = 0, dev_bytes = 0, pin_bytes = 0;      // the three blocks' sizes
    WaveOffsets wave;
};

// The three blocks of a launch group, carved in the order they always were:
//   input   [token table][frame table][ids][puncts][styles][controls][phoneme controls][the waveform stages' input regions]
//   device  [frame counts][input block][hidden][mel][wav][scan][live frame table][decoder run table][the stages' device regions]
//   pinned  [input block][frame counts][result rows, utterance after utterance][scan][the stages' staging regions][source rows]
// The waveform stages belong to the vocoder: a range without it carves none of their regions.
inline BatchOffsets batch_carve(const StageRange &r, const BatchShape &q, const WaveAsk &ask_in)
{
    const WaveAsk ask = r.has(ST_VOCODER) ? ask_in : WaveAsk{};
    BatchOffsets  o;
    Layout        in, dev, pin;
    auto take = [&](Layout &L, int id) { o.at[id] = L.at(batch_region_bytes(id, r, q, ask, o.in_bytes)); };
    for (int id = BI_TOK; id <= BI_PCTL; id++) take(in, id);
    const WaveRows cap_rows{q.nseg, q.n_rows, q.t_rows};
    wave_carve(in, ask, cap_rows, WR_INPUT, o.wave);
    o.in_bytes = in.size();
    for (int id = BD_NF; id <= BD_RUNS; id++) take(dev, id);
    wave_carve(dev, ask, cap_rows, WR_DEVICE, o.wave);
    o.dev_bytes = dev.size();
    for (int id = BP_IN; id <= BP_CUM; id++) take(pin, id);
    wave_carve(pin, ask, WaveRows{q.nseg, q.n_tokens, q.n_frames}, WR_HOST, o.wave);
    take(pin, BP_SRC);      // the newest region, behind the others: no offset of the chain's has moved
    o.pin_bytes = pin.size();
    return o;
}

}  // namespace zv
