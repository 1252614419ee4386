// schedule.h — what the stage schedules (vocoder.cpp, decoder.cpp, encoder.cpp) and the runtime (model.cpp) share; private to them.
#pragma once

#include "model.h"
#include "knobs.h"

#define ZV_LAUNCH(name, bytes, flops, call)          \
    do                                               \
    {                                                \
        if (skip_launch_) break;                     \
        hipEvent_t _e0;                              \
        tick(&_e0);                                  \
        ZV_HIP(call);                                \
        tock(_e0, name, bytes, flops);               \
    } while (0)

namespace zv
{

// algorithmic bytes / flops of one conv layer: f32 activations in + out (+ residual),
// f16 weights, f32 bias; 2*L*Cin*Cout*K flops.  L = the batch's capacity rows (exact for a single utterance and for
// batches of equal-length utterances).
inline double conv_bytes(double L, int Cin, int Cout, int K, bool res)
{
    return 4.0 * L * Cin + 4.0 * L * Cout + (res ? 4.0 * L * Cout : 0.0) + 2.0 * Cin * Cout * K + 4.0 * Cout;
}
inline double conv_flops(double L, int Cin, int Cout, int K) { return 2.0 * L * Cin * Cout * K; }

}  // namespace zv
