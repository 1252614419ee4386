// Host-side driver of csrc/conv_plan.h for tests/test_conv_plan_cpu.py (no GPU, no HIP; linked with csrc/knobs.cpp).
//   conv_plan_check cases
//       the tables below: every expectation was worked out by hand from the launchers as they stood before the header existed
//       (commit 31d1b8e: conv.hip, conv1d_mfma.hip and conv_gemm.hip; the line numbers quoted are those files'), never by running
//       the header.  Prints "ok <cases>".
//   conv_plan_check gemm_tiles
//       "<Cout_p> <groups> <tiles>" for every Cout_p from 16 to 2 112 in steps of 16 (the pytest file compares them with the
//       restatement in tests/parity_helpers.py).
//
// 256 CUs throughout.  A plan as text:
//   generic conv   "S strip= nkc= tps= g=x,y,z t= lds="                   conv_stream_kernel<nkc>
//                  "L wn= tps= g=x,y,z t= lds= tb= xcd=nx,ny,spread w="   conv1d_mfma_kernel<1, wn, 1, true> (the loader-wave form)
//                  "T mt,wn,nt tps= g=x,y,z t= lds="                      conv1d_mfma_kernel<mt, wn, nt>
//   pair           "R g=x,z off= lds="  resblock_pair64_kernel (ring);    "P mt= g=x,z lds="  resblock_pair_kernel<Cp, mt>
//   whole block    "B R= db= il= g=x,z t= lds="  resblock_block32_kernel<2, R>;   "T R= g=x,z t= lds="  resblock_triple_kernel<32, 2, R>
//   block64        "g=x,z off= lds="
//   anything the launcher answers with hipErrorInvalidValue: "invalid"
// Row bytes of an LDS tile are 2 ck + 16: 528 at 256-channel chunks, 272 at 128, 144 at 64, 80 at 32.
#include "conv_plan.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace zv;

static bool set_switches(const char *list)       // "ZV_X=V ZV_Y=W", after a reset
{
    knob_reset();
    std::string s(list);
    for (size_t a = 0; a < s.size();)
    {
        size_t b = s.find(' ', a);
        if (b == std::string::npos) b = s.size();
        const std::string kv = s.substr(a, b - a);
        const size_t eq = kv.find('=');
        if (eq == std::string::npos || !knob_set(kv.substr(0, eq).c_str(), atoi(kv.c_str() + eq + 1))) return false;
        a = b + 1;
    }
    return true;
}

static std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char *f, ...)
{
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

static ConvCall call(int njobs, int nseg, int max_rows, int rate = 1, int nt_begin = 0) { return ConvCall{njobs, nseg, max_rows, rate, 256, nt_begin}; }

// ---- generic conv ----
// a conv with K taps at dilation dil ("same" padding), chunks of min(Cin_p, 256) channels, reading one f32 tensor behind the
// InstanceNorm prologue: what the encoder's and decoder's convs look like to the plan
static ConvDesc conv(int K, int Cin_p, int Cout_p, int dil = 1)
{
    return ConvDesc{K, dil, (K - 1) / 2 * dil, Cin_p, Cout_p, Cin_p < 256 ? Cin_p : 256, PRO_NORM_ACT, Cin_p, false, false, false, false, false, false};
}
// the upsample convs conv_stream_kernel was built for: 3 taps, one chunk, f16(lrelu(x))
static ConvDesc up(int Cin_p, int Cout_p)
{
    ConvDesc d = conv(3, Cin_p, Cout_p);
    d.pro = PRO_ACT;
    return d;
}
// a decoder conv behind the operand pre-pass, with its conv_gemm_kernel pack
static ConvDesc dec(int Cin_p, int Cout_p)
{
    ConvDesc d = conv(3, Cin_p, Cout_p);
    d.pro = PRO_RAW_F16;
    d.has_w8 = true;
    return d;
}
template <class F>
static ConvDesc with(ConvDesc d, F f)
{
    f(d);
    return d;
}

static std::string text(const ConvPlan &p)
{
    if (!p.valid) return "invalid";
    if (p.form == CONV_STREAM) return fmt("S strip=%d nkc=%d tps=%d g=%d,%d,%d t=%d lds=%zu", p.strip, p.nkc, p.tps, p.gx, p.gy, p.gz, p.threads, p.lds_bytes);
    if (p.form == CONV_LOADER)
        return fmt("L wn=%d tps=%d g=%d,%d,%d t=%d lds=%zu tb=%d xcd=%d,%d,%d w=%d", p.WN, p.tps, p.gx, p.gy, p.gz, p.threads, p.lds_bytes, p.tile_bytes,
                   p.xcd_nx, p.xcd_ny, p.xcd_spread, p.warm) + ((p.MT != 1 || p.NT != 1) ? " (not <1, wn, 1>)" : "");
    return fmt("T %d,%d,%d tps=%d g=%d,%d,%d t=%d lds=%zu", p.MT, p.WN, p.NT, p.tps, p.gx, p.gy, p.gz, p.threads, p.lds_bytes) +
           ((size_t)p.tile_bytes != p.lds_bytes ? " (tile_bytes differ)" : "");
}

struct ConvCase
{
    const char *switches;
    ConvDesc    j;
    ConvCall    c;
    const char *want;
};
#define SET(field, value) [](ConvDesc &d) { d.field = value; }
// the benchmark batch at the last-but-one upsample conv (128 -> 64 channels at 100 rows per frame) and what it plans to without the stream kernel
static const ConvCall UP_BENCH = call(1, 32, 1024, 100);
#define UP_TILED "T 2,2,1 tps=800 g=25600,1,1 t=256 lds=35632"

static const ConvCase CONV_CASES[] = {
    // conv.hip:1270 WN by 1 / 2 / >= 3 output tiles; one utterance of 512 frames: :1278 wgs(4,1) and wgs(2,1) are far below 512, MT = 1
    // 1 tile: BM = 128, 4 row tiles; :1313-1314 the loader form has no WN = 1: <1,1,1>, tile (128 + 0 + 1) x 528
    {"", conv(1, 528, 32), call(1, 1, 512), "T 1,1,1 tps=4 g=4,1,1 t=256 lds=68112"},
    // 2 tiles (asr0, case (iii)): BM = 64, 8 row tiles; :1310 loader form, :1031-1037 one group: grid 8 x 8; two tiles of 65 x 528
    {"", conv(1, 528, 64), call(1, 1, 512), "L wn=2 tps=8 g=64,1,1 t=512 lds=68640 tb=34320 xcd=8,1,0 w=1"},
    // 3 tiles (to_out's 80 mels, case (iii)): BM = 32, 16 row tiles, grid 8 x 16; two tiles of 33 x 528
    {"", conv(1, 528, 96), call(1, 1, 512), "L wn=4 tps=16 g=128,1,1 t=512 lds=34848 tb=17424 xcd=16,1,0 w=1"},
    {"", conv(1, 528, 80), call(1, 1, 512), "L wn=4 tps=16 g=128,1,1 t=512 lds=34848 tb=17424 xcd=16,1,0 w=1"},

    // :1278 the MT ladder, 256 -> 256 channels, 3 taps (8 tiles, WN = 4, 2 channel groups; 768 deep: NT = 1; ai = 192 but wgs(1,1) < 4 096):
    // wgs(4,1) = 2 ceil(L / 128) >= 512 from 32 641 rows on; wgs(2,1) = 2 ceil(L / 64) >= 512 from 16 321 on; tiles (32 MT + 2 + 1) x 528
    {"", conv(3, 256, 256), call(1, 1, 32641), "T 4,4,1 tps=256 g=256,2,1 t=256 lds=69168"},
    {"", conv(3, 256, 256), call(1, 1, 32640), "T 2,4,1 tps=510 g=510,2,1 t=256 lds=35376"},
    {"", conv(3, 256, 256), call(1, 1, 16321), "T 2,4,1 tps=256 g=256,2,1 t=256 lds=35376"},
    {"", conv(3, 256, 256), call(1, 1, 16320), "T 1,4,1 tps=510 g=510,2,1 t=256 lds=18480"},       // (1 020 workgroups: no loader form, :1310)
    // :1279 the 80 KB cut at 40 000 rows (MT = 4 by the ladder): dilation 9 -> 128 + 18 + 9 = 155 rows x 528 = 81 840 stays, dilation 10 -> 158 rows go to MT = 2
    {"", conv(3, 256, 256, 9), call(1, 1, 40000), "T 4,4,1 tps=313 g=313,2,1 t=256 lds=81840"},
    {"", conv(3, 256, 256, 10), call(1, 1, 40000), "T 2,4,1 tps=625 g=625,2,1 t=256 lds=49632"},
    // :1290 ai < 200 (here 192) and wgs(1,1) = 2 ceil(L / 32) >= 4 096 from 65 505 rows on: MT capped at 2
    {"", conv(3, 256, 256), call(1, 1, 65505), "T 2,4,1 tps=1024 g=1024,2,1 t=256 lds=35376"},
    {"", conv(3, 256, 256), call(1, 1, 65504), "T 4,4,1 tps=512 g=512,2,1 t=256 lds=69168"},
    // ... not at ai = 256 (256 -> 512 channels; 768 deep: NT = 1)
    {"", conv(3, 256, 512), call(1, 1, 65505), "T 4,4,1 tps=512 g=512,4,1 t=256 lds=69168"},
    // :1292 ZV_CONV_MT is a minimum; 3 has no instantiation (:1319-1323)
    {"ZV_CONV_MT=4", conv(3, 256, 256), call(1, 1, 16320), "T 4,4,1 tps=128 g=128,2,1 t=256 lds=69168"},
    {"ZV_CONV_MT=2", conv(3, 256, 256), call(1, 1, 32641), "T 4,4,1 tps=256 g=256,2,1 t=256 lds=69168"},
    {"ZV_CONV_MT=3", conv(3, 256, 256), call(1, 1, 16320), "invalid"},

    // :1297 NT = 2: WN = 4 (implied by 8 tiles), ntiles >= 8, MT >= 2, wgs(MT,2) >= 1 024, K Cin_p >= 2 048; :1299 then MT = 4 -> 2.
    // 768 -> 256 channels (2 304 deep, ai = 288): wgs(4,2) = ceil(L / 128) >= 1 024 from 130 945 rows on
    {"", conv(3, 768, 256), call(1, 1, 130945), "T 2,4,2 tps=2047 g=2047,1,1 t=256 lds=35376"},
    {"", conv(3, 768, 256), call(1, 1, 130944), "T 4,4,1 tps=1023 g=1023,2,1 t=256 lds=69168"},
    {"", conv(3, 768, 224), call(1, 1, 130945), "T 4,4,1 tps=1024 g=1024,2,1 t=256 lds=69168"},       // 7 tiles
    {"", conv(3, 672, 256), call(1, 1, 130945), "T 4,4,1 tps=1024 g=1024,2,1 t=256 lds=69168"},       // 2 016 deep
    {"", conv(3, 688, 256), call(1, 1, 130945), "T 2,4,2 tps=2047 g=2047,1,1 t=256 lds=35376"},       // 2 064 deep
    // MT = 1 (by :1279: dilation 31 -> 64 + 93 rows do not fit 80 KB, 32 + 93 = 125 do): NT stays 1
    {"", conv(3, 768, 256, 31), call(1, 1, 130945), "T 1,4,1 tps=4093 g=4093,2,1 t=256 lds=66000"},
    // :1298 ZV_CONV_NT: 1 always; 2 where WN = 4, two tiles and MT >= 2
    {"ZV_CONV_NT=1", conv(3, 768, 256), call(1, 1, 130945), "T 4,4,1 tps=1024 g=1024,2,1 t=256 lds=69168"},
    {"ZV_CONV_NT=2", conv(3, 768, 256), call(1, 1, 130944), "T 2,4,2 tps=2046 g=2046,1,1 t=256 lds=35376"},
    {"ZV_CONV_NT=2", conv(3, 768, 224), call(1, 1, 130945), "T 2,4,2 tps=2047 g=2047,1,1 t=256 lds=35376"},
    {"ZV_CONV_NT=2", conv(3, 256, 256), call(1, 1, 16320), "T 1,4,1 tps=510 g=510,2,1 t=256 lds=18480"},

    // ---- stream (:1172-1177 conv_stream_ok, :1287 the pick, :1190-1197 its launch) ----
    // the benchmark batch, 128 -> 64 channels at 100 rows per frame: ai = 64, wgs(1,1) = 1 600 x 32; strips of 8: 200 x 32 = 6 400 >= 12 x 2 x 256
    {"", up(128, 64), UP_BENCH, "S strip=8 nkc=8 tps=200 g=6400,1,1 t=256 lds=35904"},
    // 64 -> 32 channels at 300 rows per frame: occupancy 3, strips of 8: 600 x 32 = 19 200 >= 9 216
    {"", up(64, 32), call(1, 32, 1024, 300), "S strip=8 nkc=4 tps=600 g=19200,1,1 t=256 lds=19008"},
    // :1194 the ladder, one segment: 6 144 strips of 8 from 3 145 217 rows on, else strips of 4; strips of 2 where those are fewer too
    {"", up(128, 64), call(1, 1, 3145217), "S strip=8 nkc=8 tps=6144 g=6144,1,1 t=256 lds=35904"},
    {"", up(128, 64), call(1, 1, 3145216), "S strip=4 nkc=8 tps=12286 g=12286,1,1 t=256 lds=35904"},
    {"ZV_CONV_STREAM=2", up(128, 64), call(1, 1, 102400), "S strip=2 nkc=8 tps=800 g=800,1,1 t=256 lds=35904"},
    // :1287 by itself from wgs(1,1) = ceil(L / 64) >= 4 096 on: 262 081 rows; below: MT = 4 (not memory-bound), BM = 256
    {"", up(128, 64), call(1, 1, 262081), "S strip=2 nkc=8 tps=2048 g=2048,1,1 t=256 lds=35904"},
    {"", up(128, 64), call(1, 1, 262080), "T 4,2,1 tps=1024 g=1024,1,1 t=256 lds=70448"},
    // ZV_CONV_STREAM = 0: :1290 the 64-row wave tiles (MT = 2, BM = 128: tile 131 x 272)
    {"ZV_CONV_STREAM=0", up(128, 64), UP_BENCH, UP_TILED},
    // each clause of conv_stream_ok alone
    {"", up(128, 64), call(2, 32, 1024, 100), "T 2,2,1 tps=800 g=25600,1,2 t=256 lds=35632"},
    {"", up(128, 64), call(1, 32, 1024, 100, 1), "T 2,1,1 tps=400 g=12800,1,1 t=256 lds=70448"},      // one tile left: WN = 1, BM = 256
    {"", with(up(128, 64), SET(pro, PRO_NORM_ACT)), UP_BENCH, UP_TILED},
    {"", with(up(128, 64), SET(pro, PRO_SUM3_ACT)), UP_BENCH, UP_TILED},
    {"", with(conv(5, 128, 64), SET(pro, PRO_ACT)), UP_BENCH, "T 2,2,1 tps=800 g=25600,1,1 t=256 lds=36176"},       // 128 + 4 + 1 rows
    {"", with(up(128, 64), SET(dil, 2)), UP_BENCH, "T 2,2,1 tps=800 g=25600,1,1 t=256 lds=36448"},                  // 128 + 4 + 2 rows
    {"", with(up(128, 64), SET(pad, 0)), UP_BENCH, UP_TILED},
    {"", up(96, 64), UP_BENCH, "T 2,2,1 tps=800 g=25600,1,1 t=256 lds=27248"},                                      // 131 x 208
    {"", with(up(128, 64), SET(ck, 64)), UP_BENCH, "T 2,2,1 tps=800 g=25600,1,1 t=256 lds=18864"},                   // 131 x 144
    {"", with(up(128, 64), SET(ldx, 130)), UP_BENCH, UP_TILED},
    {"", with(up(128, 64), SET(has_res, true)), UP_BENCH, UP_TILED},
    {"", with(up(128, 64), SET(has_stat, true)), UP_BENCH, UP_TILED},
    {"", with(up(128, 64), SET(eact, true)), UP_BENCH, UP_TILED},
    {"", with(up(128, 64), SET(out_f16, true)), UP_BENCH, UP_TILED},
    {"", with(up(128, 64), SET(three_inputs, true)), UP_BENCH, UP_TILED},
    {"", with(up(128, 64), SET(pro, PRO_SCALE_ACT)), UP_BENCH, "S strip=8 nkc=8 tps=200 g=6400,1,1 t=256 lds=35904"},

    // ---- the loader form (:1309-1315; its geometry :1016-1042) ----
    // a decoder conv of one 512-frame utterance, 1 056 -> 528 channels (17 tiles: 5 channel groups; 16 row tiles; case (iii)): grid 8 x 16 x ceil(5 / 8)
    {"", conv(3, 1056, 528), call(1, 1, 512), "L wn=4 tps=16 g=128,1,1 t=512 lds=36960 tb=18480 xcd=16,5,0 w=1"},
    {"ZV_CONV_XCD=0", conv(3, 1056, 528), call(1, 1, 512), "L wn=4 tps=16 g=16,5,1 t=512 lds=36960 tb=18480 xcd=0,0,0 w=1"},
    {"ZV_CONV_WARM=0", conv(3, 1056, 528), call(1, 1, 512), "L wn=4 tps=16 g=128,1,1 t=512 lds=36960 tb=18480 xcd=16,5,0 w=0"},
    {"ZV_CONV_SINGLE=0", conv(3, 1056, 528), call(1, 1, 512), "T 1,4,1 tps=16 g=16,5,1 t=256 lds=18480"},
    {"ZV_CONV_MT=2", conv(3, 1056, 528), call(1, 1, 512), "T 2,4,1 tps=8 g=8,5,1 t=256 lds=35376"},                  // MT != 1 (NT = 2 needs MT >= 2: never alone)
    {"", with(conv(3, 528, 528), SET(ck, 128)), call(1, 1, 512), "T 1,4,1 tps=16 g=16,5,1 t=256 lds=9520"},         // ck != 256: 35 x 272
    // wgs(1,1) <= 2 n_cu, 528 -> 96 channels (one group): 512 row tiles at 16 384 rows, 513 at 16 385
    {"", conv(3, 528, 96), call(1, 1, 16384), "L wn=4 tps=512 g=4096,1,1 t=512 lds=36960 tb=18480 xcd=512,1,0 w=1"},
    {"", conv(3, 528, 96), call(1, 1, 16385), "T 1,4,1 tps=513 g=513,1,1 t=256 lds=18480"},
    // :1309 several segments and more than a round: 256 segments of one row tile stay (spread map: 8 XCDs per group, conv_xcd.h), 257 go
    {"", conv(3, 528, 96), call(1, 256, 32), "L wn=4 tps=1 g=256,1,1 t=512 lds=36960 tb=18480 xcd=256,1,1 w=1"},
    {"", conv(3, 528, 96), call(1, 257, 32), "T 1,4,1 tps=1 g=257,1,1 t=256 lds=18480"},
    {"", conv(3, 528, 96), call(1, 2, 4096), "L wn=4 tps=128 g=256,1,1 t=512 lds=36960 tb=18480 xcd=256,1,1 w=1"},
    // :1311 one-chunk convs only under ZV_CONV_SINGLE = 2
    {"", conv(3, 256, 256), call(1, 1, 512), "T 1,4,1 tps=16 g=16,2,1 t=256 lds=18480"},
    {"ZV_CONV_SINGLE=2", conv(3, 256, 256), call(1, 1, 512), "L wn=4 tps=16 g=128,1,1 t=512 lds=36960 tb=18480 xcd=16,2,0 w=1"},
    // :1041 two tiles against 160 KB: dilation 41 -> 32 + 82 + 41 = 155 rows x 528 x 2 = 163 680 fit; dilation 42 -> 158 rows do not.  The
    // parent answered hipErrorInvalidValue there; the plan is the one-tile form <1,4,1> the conv runs on (the one intended difference)
    {"", conv(3, 528, 528, 41), call(1, 1, 512), "L wn=4 tps=16 g=128,1,1 t=512 lds=163680 tb=81840 xcd=16,5,0 w=1"},
    {"", conv(3, 528, 528, 42), call(1, 1, 512), "T 1,4,1 tps=16 g=16,5,1 t=256 lds=83424"},
    {"", conv(9, 528, 528, 16), call(1, 1, 512), "T 1,4,1 tps=16 g=16,5,1 t=256 lds=92928"},                        // 32 + 128 + 16 rows
    {"", conv(9, 528, 528, 32), call(1, 1, 512), "invalid"},                                                       // 320 rows: not even one tile

    // ---- the shapes tests/test_gpu_conv_xcd.py was built for (medium checkpoint: 528 encoder channels, 1 056 decoder channels, 80 mels) ----
    // (i) 3 utterances, capacity 96 phonemes / 128 frames: loader form on the spread map with 1, 1, 2, 5 and 9 channel groups
    {"", with(conv(1, 528, 64), SET(has_stat, true)), call(1, 3, 128), "L wn=2 tps=2 g=8,1,1 t=512 lds=68640 tb=34320 xcd=6,1,1 w=1"},        // asr0: 6 row tiles over 8 XCDs
    {"", conv(1, 528, 80), call(1, 3, 128), "L wn=4 tps=4 g=16,1,1 t=512 lds=34848 tb=17424 xcd=12,1,1 w=1"},                                // to_out: 12 over 8
    {"", conv(3, 528, 256), call(1, 3, 96), "L wn=4 tps=3 g=24,1,1 t=512 lds=36960 tb=18480 xcd=9,2,1 w=1"},                                 // predictors: 9 over 4
    {"", dec(1056, 528), call(1, 3, 128), "L wn=4 tps=4 g=96,1,1 t=512 lds=36960 tb=18480 xcd=12,5,1 w=1"},                                  // 5 groups: one XCD each
    {"", dec(528, 1056), call(1, 3, 128), "L wn=4 tps=4 g=192,1,1 t=512 lds=36960 tb=18480 xcd=12,9,1 w=1"},                                 // 9 groups: the group map
    // (ii) 32 utterances of 256 phonemes: 8 x 32 x 2 = 512 workgroups pass :1310's count but are two rounds: the ordinary form
    {"", conv(3, 528, 256), call(1, 32, 256), "T 1,4,1 tps=8 g=256,2,1 t=256 lds=18480"},
    {"ZV_CONV_SINGLE=0", conv(3, 528, 256), call(1, 32, 256), "T 1,4,1 tps=8 g=256,2,1 t=256 lds=18480"},
    // (iii) one utterance, 128 phonemes (asr0, to_out and the decoder conv at 512 frames: above)
    {"", conv(3, 528, 256), call(1, 1, 128), "L wn=4 tps=4 g=32,1,1 t=512 lds=36960 tb=18480 xcd=4,2,0 w=1"},
    // the generic launch behind conv_gemm_kernel for 1 088 channels: tiles 32 and 33 of 16 x 1 024 frames, WN = 2, 256 workgroups
    {"", dec(1056, 1088), call(1, 16, 1024, 1, 32), "L wn=2 tps=16 g=256,1,1 t=512 lds=70752 tb=35376 xcd=256,1,1 w=1"},
};

// ---- the GEMM split (conv.hip:1213-1237; conv_gemm.hip:29-36) ----
static const struct { const char *switches; ConvDesc j; ConvCall c; bool takes; } GEMM_TAKES[] = {
    {"", dec(1056, 1056), call(1, 16, 1024), true},       {"", dec(1056, 1056), call(1, 1, 16383), false},
    {"ZV_CONV_GEMM=0", dec(1056, 1056), call(1, 16, 1024), false}, {"ZV_CONV_GEMM=0", dec(1056, 1056), call(1, 1, 16383), false},
    {"ZV_CONV_GEMM=2", dec(1056, 1056), call(1, 16, 1024), true},  {"ZV_CONV_GEMM=2", dec(1056, 1056), call(1, 1, 16383), true},
    {"", dec(1056, 1088), call(1, 1, 16384), true},       {"", dec(1056, 528), call(1, 1, 16384), true},
    {"", dec(1056, 224), call(1, 1, 16384), false},       {"ZV_CONV_GEMM=2", dec(1056, 224), call(1, 1, 16), false},       // no whole group of 8 tiles
    {"", dec(1056, 256), call(1, 1, 16384), true},
    {"", dec(1056, 1056), call(1, 1, 4096, 4), true},     {"", dec(1056, 1056), call(1, 1, 4095, 4), false},               // rows = max_rows x rate x nseg
    // each disqualifying property alone
    {"", with(dec(1056, 1056), SET(has_w8, false)), call(1, 1, 16384), false},
    {"", with(dec(1056, 1056), SET(pro, PRO_NORM_ACT)), call(1, 1, 16384), false},
    {"", dec(112, 1056), call(1, 1, 16384), false},       {"", dec(128, 1056), call(1, 1, 16384), true},
    {"", with(dec(1056, 1056), SET(out_f16, true)), call(1, 1, 16384), false},
    {"", with(dec(1056, 1056), SET(ldx, 1060)), call(1, 1, 16384), false},
    // the benchmark batch's decoder convs (32 x 1 024 frames; 528, 1 056 and the concat's 1 120 channels in)
    {"", dec(528, 1056), call(1, 32, 1024), true},        {"", dec(1056, 1056), call(2, 32, 1024), true},
    {"", dec(1120, 1056), call(2, 32, 1024), true},       {"", dec(1056, 528), call(2, 32, 1024), true},
    {"", dec(528, 528), call(1, 32, 1024), true},
};
// Cout_p, groups, tiles on conv_gemm_kernel, tiles left (parity_helpers.conv_tile_split: (33, 33, 0) for 1 056 channels, (17, 17, 0) for 528)
static const int GEMM_SPLIT[][4] = {{1056, 4, 33, 0}, {1088, 4, 32, 2}, {528, 2, 17, 0}, {224, 0, 0, 7}, {256, 1, 8, 0}, {288, 1, 9, 0}, {320, 1, 8, 2}, {32, 0, 0, 1}};
// conv_gemm.hip:478-485: order, 256-row tiles per segment, grid.x; 512 threads, 4 x (16 384 + 18 432) bytes
static const struct { const char *switches; int Cout_p; ConvCall c; int order, tps, gx; } GEMM_PLANS[] = {
    {"", 1056, call(1, 32, 1024), 2, 4, 512},       {"ZV_GEMM_ORDER=1", 1056, call(1, 32, 1024), 1, 4, 512},
    {"ZV_GEMM_ORDER=0", 528, call(1, 1, 300), 0, 2, 4}, {"ZV_GEMM_ORDER=1", 528, call(1, 1, 300), 1, 2, 8},       // 2 groups: 4 XCDs each, row tiles rounded up to 4
    {"ZV_GEMM_ORDER=1", 768, call(1, 1, 300), 1, 2, 6},       // 3 groups: the plain grid
    {"", 1056, call(1, 1, 257, 2), 2, 3, 12},
};
// conv_gemm_units: conv_gemm.hip:46-51, per 256-channel chunk K x ceil(chunk / 64)
static const int GEMM_UNITS[][3] = {{1056, 3, 51}, {528, 3, 27}, {256, 1, 4}, {128, 3, 6}, {320, 7, 35}, {1120, 3, 54}};

// ---- pair (conv1d_mfma.hip:1161-1230, :1141-1159, :846-856); Kmax, dmax of the medium checkpoint's last dilation: 11 taps, dilation 5 ----
struct PairCase
{
    const char *switches;
    int         Cp, Kmax, dmax;
    bool        any_sum, merged, all_ring;
    ConvCall    c;
    const char *want;
};
static std::string text(const PairPlan &p)
{
    if (!p.valid) return "invalid";
    return p.ring ? fmt("R g=%d,%d off=%d lds=%zu", p.gx, p.gz, p.ring_off, p.lds_bytes) : fmt("P mt=%d g=%d,%d lds=%zu", p.MT, p.gx, p.gz, p.lds_bytes);
}
static const PairCase PAIR_CASES[] = {
    // :1207-1210 the ring form: one job, rwgs = floor((L + 245) / 246) >= 1 536 from 377 611 rows on; :848-854 1 536 tiles of 246,
    // ring behind round_up(311 x 144, 1 024), + 4 x 8 KiB.  Below: MT = 2, BM = 128, 3 201 tiles of 118 -> 3 208, (128 + 15 x 5) x 144
    {"", 64, 11, 5, false, false, true, call(1, 1, 377611), "R g=1536,1 off=45056 lds=77824"},
    {"", 64, 11, 5, false, false, true, call(1, 1, 377610), "P mt=2 g=3208,1 lds=29232"},
    // three jobs: 3 x 512 from 125 707 rows on (3 x 511 = 1 533 below); 1 066 tiles of 118 -> 1 072
    {"", 64, 11, 5, false, false, true, call(3, 1, 125707), "R g=512,3 off=45056 lds=77824"},
    {"", 64, 11, 5, false, false, true, call(3, 1, 125706), "P mt=2 g=1072,3 lds=29232"},
    // each clause alone
    {"", 64, 11, 5, true, false, true, call(1, 1, 377611), "P mt=2 g=3208,1 lds=29232"},
    {"", 64, 11, 5, false, false, false, call(1, 1, 377611), "P mt=2 g=3208,1 lds=29232"},
    {"ZV_PAIR64_RING=0", 64, 11, 5, false, false, true, call(1, 1, 377611), "P mt=2 g=3208,1 lds=29232"},
    {"ZV_PAIR64_RING=2", 64, 1, 1, false, false, true, call(1, 1, 377611), "P mt=2 g=2952,1 lds=19152"},             // Kmax < 3
    {"", 64, 11, 8, false, false, true, call(1, 1, 377611), "P mt=2 g=3208,1 lds=35712"},                            // (256 + 88) x 144 + 33 792 > 80 KB
    {"", 64, 13, 6, false, false, true, call(1, 1, 377611), "R g=1552,1 off=48128 lds=80896"},                       // (256 + 78) x 144 + 33 792 = 81 888 fits
    {"", 128, 11, 5, false, false, true, call(1, 1, 377611), "P mt=4 g=3208,1 lds=51136"},                           // not 64 channels (3 201 tiles of 118)
    // ZV_PAIR64_RING = 2: at any length; merged: one workgroup per tile
    {"ZV_PAIR64_RING=2", 64, 11, 5, false, false, true, call(3, 1, 1600), "R g=8,3 off=45056 lds=77824"},
    {"ZV_PAIR64_RING=2", 64, 11, 5, false, true, true, call(3, 1, 1600), "R g=8,1 off=45056 lds=77824"},
    // :1216 128 channels: wgs(4) = 3 ceil(L / 118) >= 2 048 from 80 477 rows on (683 tiles -> 688; (128 + 12 x 5) x 272); below 1 491 tiles of 54
    {"", 128, 11, 5, false, false, false, call(3, 1, 80477), "P mt=4 g=688,3 lds=51136"},
    {"", 128, 11, 5, false, false, false, call(3, 1, 80476), "P mt=2 g=1496,3 lds=33728"},
    // :1220 256 channels: wgs(3) = ceil(L / 86) >= 1 024 from 87 979 rows on ((96 + 11 x 5) x 528); not merged
    {"", 256, 11, 5, true, false, false, call(1, 1, 87979), "P mt=3 g=1024,1 lds=79728"},
    {"", 256, 11, 5, true, false, false, call(1, 1, 87978), "P mt=2 g=1632,1 lds=62832"},
    {"", 256, 11, 5, false, true, false, call(3, 1, 87979), "P mt=2 g=1632,1 lds=62832"},
    // :1189 the running sum and the merged form exclude each other
    {"", 256, 11, 5, true, true, false, call(3, 1, 87979), "invalid"},
    // :1221 ZV_PAIR_MT on each width, three jobs of 1 600 rows (3 only at 256 channels and not merged)
    {"ZV_PAIR_MT=2", 32, 11, 5, false, false, false, call(3, 1, 1600), "P mt=2 g=8,3 lds=26480"},
    {"ZV_PAIR_MT=3", 32, 11, 5, false, false, false, call(3, 1, 1600), "P mt=2 g=8,3 lds=26480"},
    {"ZV_PAIR_MT=4", 32, 11, 5, false, false, false, call(3, 1, 1600), "P mt=4 g=8,3 lds=46960"},
    {"ZV_PAIR_MT=2", 64, 11, 5, false, false, true, call(3, 1, 1600), "P mt=2 g=16,3 lds=29232"},
    {"ZV_PAIR_MT=3", 64, 11, 5, false, false, true, call(3, 1, 1600), "P mt=2 g=16,3 lds=29232"},
    {"ZV_PAIR_MT=4", 64, 11, 5, false, false, true, call(3, 1, 1600), "P mt=4 g=8,3 lds=47664"},
    {"ZV_PAIR_MT=2", 128, 11, 5, false, false, false, call(3, 1, 1600), "P mt=2 g=32,3 lds=33728"},
    {"ZV_PAIR_MT=3", 128, 11, 5, false, false, false, call(3, 1, 1600), "P mt=2 g=32,3 lds=33728"},
    {"ZV_PAIR_MT=4", 128, 11, 5, false, false, false, call(3, 1, 1600), "P mt=4 g=16,3 lds=51136"},
    {"ZV_PAIR_MT=2", 256, 11, 5, false, false, false, call(3, 1, 1600), "P mt=2 g=32,3 lds=62832"},
    {"ZV_PAIR_MT=3", 256, 11, 5, false, false, false, call(3, 1, 1600), "P mt=3 g=24,3 lds=79728"},
    {"ZV_PAIR_MT=4", 256, 11, 5, false, false, false, call(3, 1, 1600), "P mt=4 g=16,3 lds=96624"},
    {"ZV_PAIR_MT=3", 256, 11, 5, false, true, false, call(3, 1, 1600), "P mt=2 g=32,1 lds=62832"},
    // :1146 TMmin = BM - (Kmax - 1) < 32: 64-row tiles carry 33 taps, not 35
    {"", 128, 33, 1, false, false, false, call(3, 1, 1600), "P mt=2 g=56,3 lds=26656"},
    {"", 128, 35, 1, false, false, false, call(3, 1, 1600), "invalid"},
    {"", 48, 3, 1, false, false, false, call(1, 1, 1600), "invalid"},
    // :1154 LDS bytes, MT = 2, one job of 1 600 rows at dilation 5: (BM + (K + 4 | 4 | 1 | 0) x 5) x (2 Cp + 16) at 32 / 64 / 128 / 256 channels
    {"", 32, 3, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=8,1 lds=23280"},
    {"", 32, 7, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=8,1 lds=24880"},
    {"", 32, 11, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=8,1 lds=26480"},
    {"", 64, 3, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=16,1 lds=23472"},
    {"", 64, 7, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=16,1 lds=26352"},
    {"", 64, 11, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=16,1 lds=29232"},
    {"", 128, 3, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=32,1 lds=22848"},
    {"", 128, 7, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=32,1 lds=28288"},
    {"", 128, 11, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=32,1 lds=33728"},
    {"", 256, 3, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=32,1 lds=41712"},
    {"", 256, 7, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=32,1 lds=52272"},
    {"", 256, 11, 5, false, false, false, call(1, 1, 1600), "P mt=2 g=32,1 lds=62832"},
    // the benchmark batch's 128-channel stage (25 rows per frame): 217 tiles of 118 per segment in chunks of 8 -> 32 slots per XCD and segment (tile_deal.h)
    {"", 128, 11, 5, false, false, false, call(3, 32, 1024, 25), "P mt=4 g=8192,3 lds=51136"},
};

// ---- whole blocks (conv1d_mfma.hip:1732-1815) and block64 (:1110-1138) ----
struct BlockCase
{
    const char *switches;
    int         njobs;
    BlockDesc   j[3];
    ConvCall    c;
    const char *want;
};
#define B32(K) BlockDesc{32, K, 3, {1, 3, 5}}
#define MEDIUM32 3, {B32(3), B32(7), B32(11)}
static std::string text(const TriplePlan &p)
{
    if (!p.valid) return "invalid";
    if (p.lds_form) return fmt("B R=%d db=%d il=%d g=%d,%d t=%d lds=%zu", p.R, p.db_mask, p.interleave, p.gx, p.gz, p.threads, p.lds_bytes);
    return fmt("T R=%d g=%d,%d t=%d lds=%zu", p.R, p.gx, p.gz, p.threads, p.lds_bytes) + ((p.MT != 2 || p.db_mask || p.interleave != 1) ? " (MT, db_mask or interleave)" : "");
}
static std::string text(const Block64Plan &p)
{
    return !p.valid ? "invalid" : fmt("g=%d,%d off=%d lds=%zu", p.gx, p.gz, p.ring_off, p.lds_bytes) + (p.threads != 256 ? " (threads)" : "");
}
// The medium checkpoint's 32-channel stage: taps 3 / 7 / 11, dilations 1 / 3 / 5: halo 12 / 36 / 60, rows R + 35 / 55 / 75.
// :1787 LDS form, R = 512: 44 032 / 46 080 / 47 104 + (8 nb + 3) KiB, nb = 1 / 2 / 3: 55 296 / 65 536 / 74 752; a second weight buffer
// fits 80 KB for 3 and 7 taps (63 488, 81 920): db_mask 3, lds 81 920.  R = 256: 34 816 / 45 056 / 54 272, all doubled: 43 008 / 61 440 / 78 848.
static const BlockCase TRIPLE_CASES[] = {
    // :1735 R = 512 from 3 L >= 7 000 x 256 on: 597 334 rows (1 524 tiles of 392 -> 1 528, three jobs interleaved); below, ZV_TRIPLE_V2 = 1 leaves
    // resblock_triple_kernel (4 393 tiles of 136 -> 4 400; 331 rows x 80)
    {"", MEDIUM32, call(3, 1, 597334), "B R=512 db=3 il=3 g=4584,1 t=512 lds=81920"},
    {"", MEDIUM32, call(3, 1, 597333), "T R=256 g=4400,3 t=256 lds=26480"},
    {"ZV_TRIPLE_V2=0", MEDIUM32, call(3, 1, 597334), "T R=512 g=1528,3 t=512 lds=46960"},
    {"ZV_TRIPLE_V2=2", MEDIUM32, call(3, 1, 597333), "B R=256 db=7 il=3 g=13200,1 t=256 lds=78848"},
    // one utterance of 16 frames (4 800 rows)
    {"", MEDIUM32, call(3, 1, 16, 300), "T R=256 g=40,3 t=256 lds=26480"},
    {"ZV_TRIPLE_V2=3", MEDIUM32, call(3, 1, 16, 300), "B R=512 db=3 il=3 g=48,1 t=512 lds=81920"},
    {"ZV_TRIPLE_V2=3 ZV_TRIPLE_DB=0", MEDIUM32, call(3, 1, 16, 300), "B R=512 db=0 il=3 g=48,1 t=512 lds=74752"},
    {"ZV_TRIPLE_V2=2 ZV_TRIPLE_DB=0", MEDIUM32, call(3, 1, 16, 300), "B R=256 db=0 il=3 g=120,1 t=256 lds=54272"},
    {"ZV_TRIPLE_V2=2 ZV_TRIPLE_INTERLEAVE=0", MEDIUM32, call(3, 1, 16, 300), "B R=256 db=7 il=1 g=40,3 t=256 lds=78848"},
    // each tap count by itself at R = 512: 3 and 7 taps get the second buffer, 11 do not
    {"ZV_TRIPLE_V2=3", 1, {B32(3)}, call(1, 1, 16, 300), "B R=512 db=1 il=1 g=16,1 t=512 lds=63488"},
    {"ZV_TRIPLE_V2=3", 1, {B32(7)}, call(1, 1, 16, 300), "B R=512 db=1 il=1 g=16,1 t=512 lds=81920"},
    {"ZV_TRIPLE_V2=3", 1, {B32(11)}, call(1, 1, 16, 300), "B R=512 db=0 il=1 g=16,1 t=512 lds=74752"},
    // the benchmark batch: 784 tiles of 392 per segment in chunks of 4 -> 100 slots per XCD and segment, x 8 x 32 segments x 3 jobs
    {"", MEDIUM32, call(3, 32, 1024, 300), "B R=512 db=3 il=3 g=76800,1 t=512 lds=81920"},
    // :1792 an LDS form that does not fit: 11 taps at dilation 12, R = 512: 692 rows -> 56 320 + 27 648 > 80 KB; resblock_triple_kernel (55 360 <= 64 KB)
    {"ZV_TRIPLE_V2=3", 1, {BlockDesc{32, 11, 1, {12}}}, call(1, 1, 16, 300), "T R=512 g=16,1 t=512 lds=55360"},
    // :1762 blocks the kernels do not take
    {"", 1, {B32(5)}, call(1, 1, 16, 300), "invalid"},
    {"", 1, {BlockDesc{64, 3, 3, {1, 3, 5}}}, call(1, 1, 16, 300), "invalid"},
    {"", 1, {BlockDesc{32, 11, 1, {16}}}, call(1, 1, 16, 300), "invalid"},        // 256 - 10 x 17 = 86 rows of output
};
#define B64(K, ...) BlockDesc{64, K, 2, {__VA_ARGS__}}
static const BlockCase BLOCK64_CASES[] = {
    // 3 taps, dilations 1 and 3: TM = 244; 268 rows x 144 -> 38 912, + 32 KiB; 420 tiles -> 424
    {"", 1, {B64(3, 1, 3)}, call(1, 1, 1024, 100), "g=424,1 off=38912 lds=71680"},
    {"", 1, {B64(3, 1, 3)}, call(1, 32, 1024, 100), "g=13568,1 off=38912 lds=71680"},      // chunks of 1: 53 slots x 8 x 32
    // 11 taps: TM = 196 (523 tiles -> 528), 292 rows; with the 3-tap branch: the larger of each
    {"", 1, {B64(11, 1, 3)}, call(1, 1, 1024, 100), "g=528,1 off=43008 lds=75776"},
    {"", 2, {B64(3, 1, 3), B64(11, 1, 3)}, call(2, 1, 1024, 100), "g=528,2 off=43008 lds=75776"},
    // :1136 80 KB: one pair at dilation 21 -> 340 rows, 49 152 + 32 768 fits; dilation 22 does not
    {"", 1, {BlockDesc{64, 3, 1, {21}}}, call(1, 1, 1024, 100), "g=488,1 off=49152 lds=81920"},
    {"", 1, {BlockDesc{64, 3, 1, {22}}}, call(1, 1, 1024, 100), "invalid"},
    // :1126 not block64's: 13 taps leave 184 rows of 256; 32 channels
    {"", 1, {B64(13, 1, 3)}, call(1, 1, 1024, 100), "invalid"},
    {"", 1, {BlockDesc{32, 3, 2, {1, 3}}}, call(1, 1, 1024, 100), "invalid"},
};
// the one tile helper: K, dilations, R -> sumd, dmax, h2, halo, TM
static const struct { int K, n_dil, dil[3], R; BlockTile want; } TILES[] = {
    {3, 3, {1, 3, 5}, 256, {9, 5, 1, 12, 232}}, {7, 3, {1, 3, 5}, 256, {9, 5, 3, 36, 184}}, {11, 3, {1, 3, 5}, 512, {9, 5, 5, 60, 392}},
    {3, 2, {1, 3}, 256, {4, 3, 1, 6, 244}},     {1, 1, {1}, 256, {1, 1, 0, 0, 256}},
};

// out_conv_lds_bytes / out_conv_supported: C, K -> bytes, fits LDS_DEFAULT
static const struct { int C, K; size_t lds; bool ok; } OUT_CONV[] = {
    {112, 7, 64448, true},  {128, 7, 73056, false}, {97, 7, 64448, true},   {113, 7, 73056, false}, {64, 7, 38624, true},
    {48, 7, 30016, true},   {32, 7, 21408, true},   {31, 7, 21408, true},   {16, 7, 12800, true},   {3, 7, 12800, true},
    {112, 1, 61664, true},  {128, 1, 69888, false},
};

#define FAIL(...) return printf(__VA_ARGS__), 1

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "gemm_tiles" && argc == 2)
    {
        for (int c = 16; c <= 2112; c += 16) printf("%d %d %d\n", c, conv_gemm_groups(c), conv_gemm_tiles(c));
        return 0;
    }
    if (mode != "cases" || argc != 2)
    {
        fprintf(stderr, "usage: see the head of tests/native/conv_plan_check.cpp\n");
        return 2;
    }
    int n = 0;
    if (LDS_PER_WG != 163840 || LDS_TWO_WGS != 81920 || LDS_DEFAULT != 65536) FAIL("LDS budgets\n");
    for (const ConvCase &q : CONV_CASES)
    {
        if (!set_switches(q.switches)) FAIL("bad switch list '%s'\n", q.switches);
        ConvDesc jobs[4] = {q.j, q.j, q.j, q.j};
        const std::string got = text(conv_plan(jobs, q.c));
        if (got != q.want)
            FAIL("conv [%s] K %d dil %d Cin_p %d Cout_p %d ck %d, njobs %d nseg %d max_rows %d rate %d nt_begin %d:\n  got  %s\n  want %s\n", q.switches, q.j.K, q.j.dil,
                 q.j.Cin_p, q.j.Cout_p, q.j.ck, q.c.njobs, q.c.nseg, q.c.max_rows, q.c.rate, q.c.nt_begin, got.c_str(), q.want);
        n++;
    }
    {
        // jobs of one launch share Cout_p (conv.hip:1258)
        knob_reset();
        ConvDesc jobs[2] = {conv(3, 528, 256), conv(3, 528, 288)};
        if (conv_plan(jobs, call(2, 1, 128)).valid || conv_plan(jobs, call(0, 1, 128)).valid || conv_plan(jobs, call(1, 1, 128, 1, 8)).valid) FAIL("conv: invalid calls\n");
        n++;
    }
    for (const auto &q : GEMM_TAKES)
    {
        if (!set_switches(q.switches)) FAIL("bad switch list '%s'\n", q.switches);
        if (conv_gemm_takes(q.j, q.c) != q.takes) FAIL("conv_gemm_takes [%s] Cin_p %d Cout_p %d max_rows %d rate %d nseg %d: want %d\n", q.switches, q.j.Cin_p, q.j.Cout_p, q.c.max_rows, q.c.rate, q.c.nseg, q.takes);
        n++;
    }
    for (const auto &q : GEMM_SPLIT)
    {
        const int nt = (q[0] + 31) / 32;
        if (conv_gemm_groups(q[0]) != q[1] || conv_gemm_tiles(q[0]) != q[2] || nt - conv_gemm_tiles(q[0]) != q[3])
            FAIL("gemm split of %d channels: %d groups, %d tiles of %d\n", q[0], conv_gemm_groups(q[0]), conv_gemm_tiles(q[0]), nt);
        n++;
    }
    for (const auto &q : GEMM_PLANS)
    {
        if (!set_switches(q.switches)) FAIL("bad switch list '%s'\n", q.switches);
        const ConvGemmPlan p = conv_gemm_plan(q.Cout_p, q.c);
        if (p.order != q.order || p.tps != q.tps || p.gx != q.gx || p.threads != 512 || p.lds_bytes != 139264)
            FAIL("conv_gemm_plan [%s] %d channels: order %d tps %d gx %d threads %d lds %zu\n", q.switches, q.Cout_p, p.order, p.tps, p.gx, p.threads, p.lds_bytes);
        n++;
    }
    for (const auto &q : GEMM_UNITS)
    {
        if (conv_gemm_units(q[0], q[1]) != q[2]) FAIL("conv_gemm_units(%d, %d) = %d, want %d\n", q[0], q[1], conv_gemm_units(q[0], q[1]), q[2]);
        n++;
    }
    for (const PairCase &q : PAIR_CASES)
    {
        if (!set_switches(q.switches)) FAIL("bad switch list '%s'\n", q.switches);
        const std::string got = text(pair_plan(q.Cp, q.Kmax, q.dmax, q.any_sum, q.merged, q.all_ring, q.c));
        if (got != q.want)
            FAIL("pair [%s] Cp %d Kmax %d dmax %d sum %d merged %d ring weights %d, njobs %d nseg %d max_rows %d rate %d:\n  got  %s\n  want %s\n", q.switches, q.Cp, q.Kmax,
                 q.dmax, q.any_sum, q.merged, q.all_ring, q.c.njobs, q.c.nseg, q.c.max_rows, q.c.rate, got.c_str(), q.want);
        n++;
    }
    for (const BlockCase &q : TRIPLE_CASES)
    {
        if (!set_switches(q.switches)) FAIL("bad switch list '%s'\n", q.switches);
        const std::string got = text(triple_plan(q.j, q.c));
        if (got != q.want) FAIL("whole block [%s] first job K %d, njobs %d nseg %d max_rows %d rate %d:\n  got  %s\n  want %s\n", q.switches, q.j[0].K, q.c.njobs, q.c.nseg, q.c.max_rows, q.c.rate, got.c_str(), q.want);
        n++;
    }
    for (const BlockCase &q : BLOCK64_CASES)
    {
        if (!set_switches(q.switches)) FAIL("bad switch list '%s'\n", q.switches);
        const std::string got = text(block64_plan(q.j, q.c));
        if (got != q.want) FAIL("block64 [%s] first job K %d, njobs %d nseg %d max_rows %d rate %d:\n  got  %s\n  want %s\n", q.switches, q.j[0].K, q.c.njobs, q.c.nseg, q.c.max_rows, q.c.rate, got.c_str(), q.want);
        n++;
    }
    for (const auto &q : TILES)
    {
        const BlockTile t = block_tile(q.K, q.dil, q.n_dil, q.R);
        if (t.sumd != q.want.sumd || t.dmax != q.want.dmax || t.h2 != q.want.h2 || t.halo != q.want.halo || t.TM != q.want.TM) FAIL("block_tile(K %d, %d dilations, R %d)\n", q.K, q.n_dil, q.R);
        n++;
    }
    // the output conv's LDS: (256 + K - 1) rows of (2 Cp + 16) bytes + K Cp f16 weights within 64 KiB.  7 taps: 112 channels take
    // 262 x 240 + 1 568 = 64 448 bytes, 128 take 262 x 272 + 1 792 = 73 056; real channels count padded to 16 (97 .. 112 are one Cp,
    // 113 the next); the last stages the suite runs (64, 48, 32, 31, 16, 3 channels); an even or missing tap count is no 'same' conv
    for (const auto &q : OUT_CONV)
    {
        if (out_conv_lds_bytes(q.C, q.K) != q.lds || out_conv_supported(q.C, q.K) != q.ok)
            FAIL("out_conv(C %d, K %d): %zu bytes, supported %d; want %zu, %d\n", q.C, q.K, out_conv_lds_bytes(q.C, q.K), out_conv_supported(q.C, q.K), q.lds, q.ok);
        n++;
    }
    if (out_conv_supported(0, 7) || out_conv_supported(32, 0) || out_conv_supported(32, 6)) FAIL("out_conv: degenerate shapes\n");
    n++;
    printf("ok %d\n", n);
    return 0;
}
