// Host-side driver of csrc/stage_plan.h for tests/test_stage_plan_cpu.py (no GPU, no HIP; linked with csrc/knobs.cpp).
//   stage_plan_check cases
//       the tables below: every expectation was worked out by hand from the code as it stood inline before the header existed
//       (commit ec7fe77; "misc:" quotes csrc/misc_kernels.hip of that commit, "dec:" csrc/decoder.cpp, "enc:" csrc/encoder.cpp), never
//       by running the header.  Prints "ok <cases>".
//   stage_plan_check att_limits
//       "<dk> <most tokens the matrix-core attention takes, 0: none>" for every even dk from 2 to 600, with ZV_ATT_MFMA set so that the
//       workgroup count does not enter (the pytest file compares them with the restatement in tests/parity_helpers.py).
//   stage_plan_check constants
//       "<ATT_NS_MAX> <ATT_LDS_MAX> <LN_TAIL_MAX>"
//
// A plan as text:
//   attention   "M g=x,y,z lds= a="  attention_mfma_kernel (a: the 48 KiB attribute is raised);  "S g=x,y,z lds="  attention_kernel;
//               "invalid": the launcher answers hipErrorInvalidValue
//   linear      "r= tps= g=x,y"      linear_mfma_kernel<r / 32>
//   regulator   "F g=x,y"  lr_fused16_kernel;  "G16 scan= g=x,y lds="  lr_scan_kernel + lr_gather16_kernel;  "G scan= g=x,y"  + lr_gather_kernel
//   encoder     "m= t="              merged, tails
//   decoder     "p= r= k="           prepass, runs, pack
#include "stage_plan.h"

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

static std::string text(const AttPlan &p)
{
    if (p.form == ATT_INVALID) return "invalid";
    if (p.form == ATT_SCALAR) return fmt("S g=%d,%d,%d lds=%zu", p.gx, p.gy, p.gz, p.lds);
    return fmt("M g=%d,%d,%d lds=%zu a=%d", p.gx, p.gy, p.gz, p.lds, (int)p.raise_lds);
}
static std::string text(const LinearPlan &p) { return fmt("r=%d tps=%d g=%d,%d", p.rows, p.tps, p.gx, p.gy); }
static std::string text(const LrPlan &p)
{
    if (p.form == LR_FUSED) return fmt("F g=%d,%d", p.gx, p.gy);
    if (p.form == LR_SCAN_GATHER16) return fmt("G16 scan=%d g=%d,%d lds=%zu", p.scan_gx, p.gx, p.gy, p.lds);
    return fmt("G scan=%d g=%d,%d", p.scan_gx, p.gx, p.gy);
}
static std::string text(const EncPlan &p) { return fmt("m=%d t=%d", (int)p.merged, (int)p.tails); }
static std::string text(const DecPlan &p) { return fmt("p=%d r=%d k=%d", (int)p.prepass, (int)p.runs, (int)p.pack); }

// ---- attention (misc:933-958) ----
// matrix cores where: no ZV_ATT_SCALAR, dk % 4 == 0, dk <= 288, ld % 4 == 0, lds = (64 (dk | 1) + 1 + 64 round_up(n, 32)) * 4 <= 159 744
// (misc:939,942, ATT_LDS_MAX misc:656), ceil(n / 64) H nseg >= 48 or ZV_ATT_MFMA (misc:941,943); grid (ceil(n / 64), H, nseg) (misc:951), the
// attribute for lds > 49 152 (misc:946).  Else scalar: lds = (dk + n) * 4, refused above 61 440 (misc:954-955), grid (n, H, nseg) (misc:956).
struct AttCase
{
    const char *switches;
    int         n, H, dk, ld, nseg;
    const char *want;
};
static const AttCase ATT_CASES[] = {
    // the LDS limit at E = 528 and H = 2, 3, 4, the numbers of tests/test_gpu_attention_heads.py.
    // dk = 264: 64 * 265 + 1 = 16 961; 352 tokens: + 22 528 = 39 489 floats = 157 956 B; 353 -> 384 rows: 41 537 floats = 166 148 B
    {"", 352, 2, 264, 1584, 4, "M g=6,2,4 lds=157956 a=1"},
    {"", 353, 2, 264, 1584, 4, "S g=353,2,4 lds=2468"},
    // dk = 176: 11 329; 416 tokens: + 26 624 = 37 953 floats = 151 812 B; 417 -> 448 rows: 40 001 floats = 160 004 B
    {"", 416, 3, 176, 1584, 3, "M g=7,3,3 lds=151812 a=1"},
    {"", 417, 3, 176, 1584, 3, "S g=417,3,3 lds=2372"},
    // dk = 132: 8 513; 480 tokens: + 30 720 = 39 233 floats = 156 932 B; 481 -> 512 rows: 41 281 floats = 165 124 B
    {"", 480, 4, 132, 1584, 2, "M g=8,4,2 lds=156932 a=1"},
    {"", 481, 4, 132, 1584, 2, "S g=481,4,2 lds=2452"},
    // dk <= 2 ATT_NS_MAX = 288 (geometry e576) against 292; 64 * 289 + 1 + 4 096 = 22 593 floats
    {"", 64, 2, 288, 1728, 24, "M g=1,2,24 lds=90372 a=1"},
    {"", 64, 2, 292, 1752, 24, "S g=64,2,24 lds=1424"},
    {"ZV_ATT_MFMA=1", 64, 2, 292, 1752, 24, "S g=64,2,24 lds=1424"},
    // dk % 4: dk = 66 (E = 528, H = 8)
    {"", 64, 8, 66, 1584, 6, "S g=64,8,6 lds=520"},
    {"ZV_ATT_MFMA=1", 64, 8, 66, 1584, 6, "S g=64,8,6 lds=520"},
    // ld % 4: 11 329 + 8 192 = 19 521 floats
    {"", 128, 3, 176, 1584, 8, "M g=2,3,8 lds=78084 a=1"},
    {"", 128, 3, 176, 1586, 8, "S g=128,3,8 lds=1216"},
    // 47 against 48 workgroups, through nseg, H and the 64-query tiles; 11 329 + 4 096 = 15 425 floats
    {"", 64, 1, 176, 528, 47, "S g=64,1,47 lds=960"},
    {"", 64, 1, 176, 528, 48, "M g=1,1,48 lds=61700 a=1"},
    {"ZV_ATT_MFMA=1", 64, 1, 176, 528, 47, "M g=1,1,47 lds=61700 a=1"},
    {"ZV_ATT_MFMA=1", 64, 1, 176, 528, 1, "M g=1,1,1 lds=61700 a=1"},
    {"", 64, 3, 176, 1584, 16, "M g=1,3,16 lds=61700 a=1"},
    {"", 64, 3, 176, 1584, 15, "S g=64,3,15 lds=960"},
    {"", 65, 3, 176, 1584, 8, "M g=2,3,8 lds=69892 a=1"},           // 11 329 + 6 144 = 17 473 floats
    {"ZV_ATT_SCALAR=1", 64, 1, 176, 528, 48, "S g=64,1,48 lds=960"},
    {"ZV_ATT_SCALAR=1 ZV_ATT_MFMA=1", 64, 1, 176, 528, 48, "S g=64,1,48 lds=960"},
    // the 48 KiB attribute: dk = 64: 4 161; 96 tokens: + 6 144 = 10 305 floats = 41 220 B; 97 -> 128 rows: 12 353 floats = 49 412 B
    {"", 96, 8, 64, 1536, 3, "M g=2,8,3 lds=41220 a=0"},
    {"", 97, 8, 64, 1536, 3, "M g=2,8,3 lds=49412 a=1"},
    // the scalar form's 60 KiB: dk + n = 15 360 against 15 361, reached by a head width the matrix cores refuse and by their LDS limit
    {"", 15294, 1, 66, 198, 1, "S g=15294,1,1 lds=61440"},
    {"", 15295, 1, 66, 198, 1, "invalid"},
    {"", 15184, 1, 176, 528, 1, "S g=15184,1,1 lds=61440"},
    {"", 15185, 1, 176, 528, 1, "invalid"},
    {"ZV_ATT_MFMA=1", 15185, 1, 176, 528, 1, "invalid"},
    // the benchmark batch: 32 utterances of at most 256 tokens, E = 528, H = 2; 16 961 + 16 384 = 33 345 floats
    {"", 256, 2, 264, 1584, 32, "M g=4,2,32 lds=133380 a=1"},
    // one short utterance of it: 4 x 2 workgroups
    {"", 256, 2, 264, 1584, 1, "S g=256,2,1 lds=2080"},
};

// ---- linear (misc:494-514) ----
// 64-row workgroups where ceil(rows / 64) nseg ceil(out / 128) >= 256 (misc:500-501), else 32-row; tps = ceil(rows / tile), grid
// (ceil(out / 128), tps nseg) (misc:503-504, 509-510)
struct LinearCase
{
    int         rows, nseg, out;
    const char *want;
};
static const LinearCase LINEAR_CASES[] = {
    // one segment, 1 584 outputs = 13 column groups: 19 row tiles = 247 workgroups, 20 = 260
    {1216, 1, 1584, "r=32 tps=38 g=13,38"},
    {1217, 1, 1584, "r=64 tps=20 g=13,20"},
    // 255 against 256 exactly
    {16320, 1, 128, "r=32 tps=510 g=1,510"},
    {16321, 1, 128, "r=64 tps=256 g=1,256"},
    {64, 255, 128, "r=32 tps=2 g=1,510"},
    {64, 256, 128, "r=64 tps=1 g=1,256"},
    {64, 1, 128 * 255, "r=32 tps=2 g=255,2"},
    {64, 1, 128 * 255 + 1, "r=64 tps=1 g=256,1"},
    // a batch reaches it through nseg: 2 row tiles x 13 x 9 = 234, x 10 = 260
    {128, 9, 1584, "r=32 tps=4 g=13,36"},
    {128, 10, 1584, "r=64 tps=2 g=13,20"},
    // the benchmark batch's merged token rows (32 x 256, one segment): 128 x 13 = 1 664 workgroups
    {8192, 1, 1584, "r=64 tps=128 g=13,128"},
    // one 128-token utterance; a row count that is no multiple of the tile
    {128, 1, 1584, "r=32 tps=4 g=13,4"},
    {33, 1, 528, "r=32 tps=2 g=5,2"},
};

// ---- length regulator (misc:1425-1446) ----
// C, ld, ldh all multiples of 4 and 1 <= tokens <= 1 024 and frames >= 1: fused, grid (ceil(frames / 16), nseg) (misc:1431-1435); else the scan,
// grid (nseg) (misc:1438), and — the multiples of 4 again, 1 <= tokens, tokens * 4 <= 49 152 — gather16, grid as the fused form's, LDS
// tokens * 4 (misc:1439-1441); else the gather, grid (frames, nseg) (misc:1443)
struct LrCase
{
    int         C, ld, ldh, tokens, frames, nseg;
    const char *want;
};
static const LrCase LR_CASES[] = {
    {528, 528, 528, 1024, 1024, 1, "F g=64,1"},
    {528, 528, 528, 1025, 1024, 1, "G16 scan=1 g=64,1 lds=4100"},
    {528, 528, 528, 1100, 2048, 1, "G16 scan=1 g=128,1 lds=4400"},      // tests/test_gpu_prosody.py
    {528, 528, 528, 1, 1, 1, "F g=1,1"},
    {528, 528, 528, 256, 17, 3, "F g=2,3"},
    {528, 528, 528, 256, 1024, 32, "F g=64,32"},                        // the benchmark batch
    // a width that is no multiple of 4, each of the three
    {530, 532, 532, 100, 1024, 1, "G scan=1 g=1024,1"},
    {528, 530, 528, 100, 1024, 2, "G scan=2 g=1024,2"},
    {528, 528, 530, 100, 1024, 1, "G scan=1 g=1024,1"},
    // the gather's LDS: 12 288 tokens = 49 152 B
    {528, 528, 528, 12288, 16385, 2, "G16 scan=2 g=1025,2 lds=49152"},
    {528, 528, 528, 12289, 16385, 2, "G scan=2 g=16385,2"},
    // no tokens, no frames: the forms that ask for one of either stand back
    {528, 528, 528, 0, 64, 1, "G scan=1 g=64,1"},
    {528, 528, 528, 10, 0, 1, "G16 scan=1 g=0,1 lds=40"},
};

// ---- the encoder's schedule (enc:36,45; layernorm_tail_ok misc:1134: C <= 64 * 12) ----
struct EncCase
{
    const char *switches;
    int         E, V;
    bool        dbg;
    const char *want;
};
static const EncCase ENC_CASES[] = {
    {"", 528, 256, false, "m=1 t=1"},
    {"", 528, 256, true, "m=1 t=0"},
    {"ZV_LN_TAIL=0", 528, 256, false, "m=1 t=0"},
    {"ZV_LINEAR_MERGED=0", 528, 256, false, "m=0 t=1"},
    {"", 768, 768, false, "m=1 t=1"},
    {"", 769, 256, false, "m=1 t=0"},
    {"", 528, 769, false, "m=1 t=0"},
    {"", 720, 784, false, "m=1 t=0"},       // medium_e720: through V alone
    {"", 720, 768, false, "m=1 t=1"},
    {"", 1024, 256, false, "m=1 t=0"},      // medium_e1024
};

// ---- the decoder's schedule (dec:41-60) ----
// prepass: ZV_DEC_PREPASS >= 0 ? != 0 : t_max nseg >= 256 (dec:43,47); runs: not fitted, no tap, prepass, ZV_DEC_RUNS as a batch switch over
// t_rows >= 16 384 (dec:54-55; conv_plan.h BATCH_ROWS); pack: a run table, nseg > 1, ZV_DEC_PACK (dec:60)
struct DecCase
{
    const char *switches;
    int         nseg, t_max;
    size_t      t_rows;
    bool        fitted, dbg, table;
    const char *want;
};
static const DecCase DEC_CASES[] = {
    {"", 1, 255, 255, false, false, false, "p=0 r=0 k=0"},
    {"", 1, 256, 256, false, false, false, "p=1 r=0 k=0"},
    {"", 3, 85, 255, false, false, false, "p=0 r=0 k=0"},
    {"", 4, 64, 256, false, false, false, "p=1 r=0 k=0"},
    {"ZV_DEC_PREPASS=-1", 1, 16, 16, false, false, false, "p=0 r=0 k=0"},
    {"ZV_DEC_PREPASS=1", 1, 16, 16, false, false, false, "p=1 r=0 k=0"},
    {"ZV_DEC_PREPASS=0", 32, 1024, 32768, false, false, false, "p=0 r=0 k=0"},
    {"ZV_DEC_PREPASS=1 ZV_DEC_RUNS=2", 1, 16, 16, false, false, true, "p=1 r=1 k=0"},
    // the capacity
    {"", 1, 16383, 16383, false, false, false, "p=1 r=0 k=0"},
    {"", 1, 16384, 16384, false, false, true, "p=1 r=1 k=0"},
    {"", 3, 5461, 16383, false, false, false, "p=1 r=0 k=0"},
    {"", 4, 4096, 16384, false, false, true, "p=1 r=1 k=1"},
    // ZV_DEC_RUNS
    {"ZV_DEC_RUNS=0", 32, 1024, 32768, false, false, false, "p=1 r=0 k=0"},
    {"ZV_DEC_RUNS=1", 32, 1024, 32768, false, false, true, "p=1 r=1 k=1"},
    {"ZV_DEC_RUNS=2", 1, 256, 256, false, false, true, "p=1 r=1 k=0"},
    {"ZV_DEC_RUNS=2", 1, 255, 255, false, false, false, "p=0 r=0 k=0"},
    {"ZV_DEC_RUNS=2 ZV_DEC_PREPASS=0", 32, 1024, 32768, false, false, false, "p=0 r=0 k=0"},
    // fitted mode, a debug tap
    {"", 32, 1024, 32768, true, false, false, "p=1 r=0 k=0"},
    {"", 32, 1024, 32768, false, true, false, "p=1 r=0 k=0"},
    {"ZV_DEC_RUNS=2", 32, 1024, 32768, true, false, false, "p=1 r=0 k=0"},
    {"ZV_DEC_RUNS=2", 32, 1024, 32768, false, true, false, "p=1 r=0 k=0"},
    // pack: 1 against 2 utterances, with and without a run table (the tap entry points pass none where runs holds), ZV_DEC_PACK = 0
    {"", 1, 16384, 16384, false, false, true, "p=1 r=1 k=0"},
    {"", 2, 8192, 16384, false, false, true, "p=1 r=1 k=1"},
    {"", 2, 8192, 16384, false, false, false, "p=1 r=1 k=0"},
    {"ZV_DEC_PACK=0", 2, 8192, 16384, false, false, true, "p=1 r=1 k=0"},
    {"ZV_DEC_PACK=0", 32, 1024, 32768, false, false, true, "p=1 r=1 k=0"},
    // the benchmark batch: 32 utterances of 1 024 frames
    {"", 32, 1024, 32768, false, false, true, "p=1 r=1 k=1"},
};

#define FAIL(...) return printf(__VA_ARGS__), 1

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "att_limits" && argc == 2)
    {
        if (!set_switches("ZV_ATT_MFMA=1")) return 2;
        for (int dk = 2; dk <= 600; dk += 2)
        {
            int n = 0;      // the form can only be lost as n grows: the first n that is not taken ends the search
            while (att_plan(n + 1, 1, dk, dk, 1).form == ATT_MFMA) n++;
            printf("%d %d\n", dk, n);
        }
        return 0;
    }
    if (mode == "constants" && argc == 2)
    {
        printf("%d %zu %d\n", ATT_NS_MAX, ATT_LDS_MAX, LN_TAIL_MAX);
        return 0;
    }
    if (mode != "cases" || argc != 2)
    {
        fprintf(stderr, "usage: see the head of tests/native/stage_plan_check.cpp\n");
        return 2;
    }
    int n = 0;
    if (ATT_NS_MAX != 144 || ATT_LDS_MAX != 159744 || LN_TAIL_MAX != 768) FAIL("constants\n");
    for (const AttCase &q : ATT_CASES)
    {
        if (!set_switches(q.switches)) FAIL("bad switch list '%s'\n", q.switches);
        const std::string got = text(att_plan(q.n, q.H, q.dk, q.ld, q.nseg));
        if (got != q.want) FAIL("attention [%s] n %d H %d dk %d ld %d nseg %d:\n  got  %s\n  want %s\n", q.switches, q.n, q.H, q.dk, q.ld, q.nseg, got.c_str(), q.want);
        n++;
    }
    knob_reset();
    for (const LinearCase &q : LINEAR_CASES)
    {
        const std::string got = text(linear_plan(q.rows, q.nseg, q.out));
        if (got != q.want) FAIL("linear rows %d nseg %d out %d:\n  got  %s\n  want %s\n", q.rows, q.nseg, q.out, got.c_str(), q.want);
        n++;
    }
    for (const LrCase &q : LR_CASES)
    {
        const std::string got = text(lr_plan(q.C, q.ld, q.ldh, q.tokens, q.frames, q.nseg));
        if (got != q.want) FAIL("regulator C %d ld %d ldh %d tokens %d frames %d nseg %d:\n  got  %s\n  want %s\n", q.C, q.ld, q.ldh, q.tokens, q.frames, q.nseg, got.c_str(), q.want);
        n++;
    }
    if (!layernorm_tail_ok(768) || layernorm_tail_ok(769) || !layernorm_tail_ok(16)) FAIL("layernorm_tail_ok\n");
    n++;
    for (const EncCase &q : ENC_CASES)
    {
        if (!set_switches(q.switches)) FAIL("bad switch list '%s'\n", q.switches);
        const std::string got = text(enc_plan(q.E, q.V, q.dbg));
        if (got != q.want) FAIL("encoder [%s] E %d V %d dbg %d:\n  got  %s\n  want %s\n", q.switches, q.E, q.V, (int)q.dbg, got.c_str(), q.want);
        n++;
    }
    for (const DecCase &q : DEC_CASES)
    {
        if (!set_switches(q.switches)) FAIL("bad switch list '%s'\n", q.switches);
        const std::string got = text(dec_plan(q.nseg, q.t_max, q.t_rows, q.fitted, q.dbg, q.table));
        if (got != q.want)
            FAIL("decoder [%s] nseg %d t_max %d t_rows %zu fitted %d dbg %d table %d:\n  got  %s\n  want %s\n", q.switches, q.nseg, q.t_max, q.t_rows, (int)q.fitted,
                 (int)q.dbg, (int)q.table, got.c_str(), q.want);
        n++;
    }
    knob_reset();
    printf("ok %d\n", n);
    return 0;
}
