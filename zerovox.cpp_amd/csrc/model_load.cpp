// model_load.cpp — the loader: GGUF weights re-laid-out in HBM, the constructor's checkpoint reading (see model.h).
#include "model.h"
#include "knobs.h"

#include <algorithm>

namespace zv
{

static const char *KV_PREFIX = "zerovox-resnet-fs2-styletts.";   // reference src/zerovox.h:17-33

void *Model::dev_alloc(size_t bytes)
{
    void *p = nullptr;
    if (bytes == 0) bytes = 16;
    if (hipMalloc(&p, bytes) != hipSuccess) fail(ZV_ERR_OOM, "hipMalloc(%zu) failed", bytes);
    allocs_.push_back(p);
    return p;
}

const void *Model::bands_table()
{
#if !defined(__HIP_DEVICE_COMPILE__)      // (bands.h keeps its host half out of device passes)
    if (!bands_table_)
    {
        const std::vector<int8_t> img = bands_table_fragments(bands_tables());
        void *d = dev_alloc(img.size());
        ZV_HIP(hipMemcpy(d, img.data(), img.size(), hipMemcpyHostToDevice));
        bands_table_ = d;
    }
#endif
    return bands_table_;
}

const void *Model::mel_table()
{
#if !defined(__HIP_DEVICE_COMPILE__)      // (mel.h keeps its host half out of device passes)
    if (!mel_table_)
    {
        const std::vector<int8_t> img = mel_table_fragments(mel_tables());
        void *d = dev_alloc(img.size());
        ZV_HIP(hipMemcpy(d, img.data(), img.size(), hipMemcpyHostToDevice));
        mel_table_ = d;
    }
#endif
    return mel_table_;
}

float *Model::upload_f32(const GgufTensor &t, int pad_to, float pad_value)
{
    if (t.type != GGML_F32) fail(ZV_ERR_SHAPE, "tensor %s: expected f32", t.name.c_str());
    const size_t n = (size_t)t.nelements();
    const size_t np = pad_to > 0 ? (size_t)std::max<int64_t>(pad_to, (int64_t)n) : n;
    std::vector<float> h(np + 64, pad_value);            // 64 floats of slack: prologues read whole float4 groups
    memcpy(h.data(), t.data, n * sizeof(float));
    float *d = (float *)dev_alloc(h.size() * sizeof(float));
    ZV_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return d;
}

float *Model::upload_vec(const GgufFile &g, const std::string &name, int expect_n, int pad_to, float pad_value)
{
    const GgufTensor &t = g.get(name);
    if (t.nelements() != expect_n) fail(ZV_ERR_SHAPE, "tensor %s: expected %d elements, found %lld", name.c_str(), expect_n, (long long)t.nelements());
    return upload_f32(t, pad_to, pad_value);
}

// GGUF conv weight: ggml ne [K, IC, OC] f16 (k fastest), bias f32 [OC]  (SURVEY.md Appx A)
ConvW Model::load_conv(const GgufFile &g, const std::string &wname, const std::string &bname, int expect_cin, bool gemm_pack)
{
    const GgufTensor &w = g.get(wname);
    if (w.type != GGML_F16) fail(ZV_ERR_SHAPE, "tensor %s: conv weights must be f16", wname.c_str());
    ConvW c;
    c.K = (int)w.ne[0];
    c.Cin = (int)w.ne[1];
    c.Cout = (int)w.ne[2];
    if (expect_cin >= 0 && c.Cin != expect_cin) fail(ZV_ERR_SHAPE, "tensor %s: expected %d input channels, found %d", wname.c_str(), expect_cin, c.Cin);
    if ((c.K & 1) == 0) fail(ZV_ERR_SHAPE, "tensor %s: even kernel size %d is not a 'same' conv", wname.c_str(), c.K);
    c.Cin_p = round_up(c.Cin, 16);
    c.Cout_p = round_up(c.Cout, 16);
    c.ck = conv_pick_ck(c.Cin_p);
    std::vector<uint16_t> packed(packed_conv_weight_halfs(c.Cin_p, c.Cout_p, c.K));
    pack_conv_weight((const uint16_t *)w.data, c.K, c.Cin, c.Cout, c.Cin_p, c.Cout_p, c.ck, packed.data());
    c.w = dev_alloc(packed.size() * 2 + 32768);      // slack: the MFMA loops request up to 16 KiB past the last block
    ZV_HIP(hipMemcpy(c.w, packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
    if (gemm_pack && c.Cin_p >= 256 && conv_gemm_groups(c.Cout_p) >= 1)
    {
        // batches run the wide decoder convs on conv_gemm_kernel: the same weights once more, in its stream order
        std::vector<uint16_t> p8(conv_gemm_weight_halfs(c.Cin_p, c.Cout_p, c.K));
        pack_conv_weight_gemm((const uint16_t *)w.data, c.K, c.Cin, c.Cout, c.Cin_p, c.Cout_p, p8.data());
        c.w8 = dev_alloc(p8.size() * 2);
        ZV_HIP(hipMemcpy(c.w8, p8.data(), p8.size() * 2, hipMemcpyHostToDevice));
    }
    if (!bname.empty())
    {
        const GgufTensor &b = g.get(bname);
        if (b.type != GGML_F32 || b.nelements() != c.Cout) fail(ZV_ERR_SHAPE, "tensor %s: expected f32[%d]", bname.c_str(), c.Cout);
        c.bias = upload_f32(b, round_up(c.Cout_p, 32), 0.f);
    }
    return c;
}

// ConvTranspose1d(stride s, kernel K, padding p = s/2 + s%2, output_padding s%2) as the reference defines it:
// zero-stuff + conv with the stored, already flipped kernel (src/hifigan.cpp:22-71).  Output sample
// t = q*s + r only sees stuffed positions off + i*s, i.e. taps k = off - r + (i - q)*s: per phase r a
// short conv over the *un-stuffed* input.  All s phases become one ordinary conv with s*Cout_p output
// channels (channel r*Cout_p + oc) whose channels-last output [L][s*Cout_p] IS the up-sampled
// sequence [L*s][Cout_p] — no stuffed buffer, no s-fold wasted MACs.
ConvW Model::load_upsample(const GgufFile &g, int idx, int stride, int expect_cin)
{
    char nm[96];
    snprintf(nm, sizeof(nm), "_meldec.upsamples.%d.1.w", idx);
    const GgufTensor &w = g.get(nm);
    if (w.type != GGML_F16) fail(ZV_ERR_SHAPE, "tensor %s: conv weights must be f16", nm);
    const int K = (int)w.ne[0], IC = (int)w.ne[1], OC = (int)w.ne[2];
    if (IC != expect_cin) fail(ZV_ERR_SHAPE, "tensor %s: expected %d input channels, found %d", nm, expect_cin, IC);
    const int s = stride;
    const int p = s / 2 + s % 2, op = s % 2;
    const int off = (K - 1) - p;
    // reference output length: (L-1)*s + 1 + 2*off + op - (K-1) must equal L*s
    if (2 * off + op + 1 - (K - 1) != s) fail(ZV_ERR_SHAPE, "tensor %s: kernel %d / stride %d do not give L*s outputs", nm, K, s);
    // delta = i - q over all (k, r):  k = off - r + delta*s
    int dmin = 0, dmax = 0;
    for (int r = 0; r < s; r++)
        for (int k = 0; k < K; k++)
            if ((k - off + r) % s == 0)
            {
                const int d = (k - off + r) / s;
                dmin = std::min(dmin, d);
                dmax = std::max(dmax, d);
            }
    const int nd = std::max(-dmin, dmax);          // symmetric window so the conv stays a "same" conv
    ConvW c;
    c.K = 2 * nd + 1;
    c.Cin = IC;
    c.Cin_p = round_up(IC, 16);
    const int OCp = round_up(OC, 16);
    c.Cout = s * OCp;
    c.Cout_p = s * OCp;
    // batches run the wide ones (at least one group of 8 output tiles, input channels in 64-channel blocks) on conv_gemm_kernel
    // behind an f16 operand pre-pass; its chains walk 256-channel chunks, so these convs do everywhere (same bits in every regime)
    // (at least 768 products per output element: measured 225 -> 181 + 15 us and 365 -> 192 + 75 + 50 us (kernel + leftover tiles +
    // pre-pass) for the 1 536- and 768-deep ones; the 384-deep one 496 -> 364 + 120 us — conv_gemm_kernel's one workgroup per CU
    // spends a six-unit contraction mostly in its prologue and its 256-KiB epilogue — stays on conv1d_mfma_kernel)
    const bool gemm_pack = c.Cin_p >= 128 && (c.Cin_p & 63) == 0 && conv_gemm_groups(c.Cout_p) >= 1 && c.K * c.Cin_p >= 768;
    c.ck = conv_pick_ck(c.Cin_p, gemm_pack ? 256 : 128);      // measured: the 3-input (MRF mean) prologue of these convs prefers 128-channel chunks
    // virtual weight in GGUF conv layout [OC'][IC][K'] (k fastest)
    std::vector<uint16_t> v((size_t)c.Cout * IC * c.K, 0);
    const uint16_t *src = (const uint16_t *)w.data;
    for (int r = 0; r < s; r++)
        for (int oc = 0; oc < OC; oc++)
            for (int ic = 0; ic < IC; ic++)
                for (int tp = 0; tp < c.K; tp++)
                {
                    const int k = off - r + (tp - nd) * s;
                    if (k >= 0 && k < K) v[((size_t)(r * OCp + oc) * IC + ic) * c.K + tp] = src[((size_t)oc * IC + ic) * K + k];
                }
    std::vector<uint16_t> packed(packed_conv_weight_halfs(c.Cin_p, c.Cout_p, c.K));
    pack_conv_weight(v.data(), c.K, IC, c.Cout, c.Cin_p, c.Cout_p, c.ck, packed.data());
    c.w = dev_alloc(packed.size() * 2 + 32768);      // slack: as in load_conv
    ZV_HIP(hipMemcpy(c.w, packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
    if (gemm_pack)
    {
        std::vector<uint16_t> p8(conv_gemm_weight_halfs(c.Cin_p, c.Cout_p, c.K));
        pack_conv_weight_gemm(v.data(), c.K, IC, c.Cout, c.Cin_p, c.Cout_p, p8.data());
        c.w8 = dev_alloc(p8.size() * 2);
        ZV_HIP(hipMemcpy(c.w8, p8.data(), p8.size() * 2, hipMemcpyHostToDevice));
    }
    snprintf(nm, sizeof(nm), "_meldec.upsamples.%d.1.b", idx);
    const GgufTensor &b = g.get(nm);
    if (b.type != GGML_F32 || b.nelements() != OC) fail(ZV_ERR_SHAPE, "tensor %s: expected f32[%d]", nm, OC);
    std::vector<float> hb(round_up(c.Cout_p, 32) + 64, 0.f);
    for (int r = 0; r < s; r++) memcpy(hb.data() + (size_t)r * OCp, b.data, (size_t)OC * 4);
    c.bias = (float *)dev_alloc(hb.size() * 4);
    ZV_HIP(hipMemcpy(c.bias, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
    return c;
}

Model::Model(const std::string &path, int dev) : device(dev)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) fail(ZV_ERR_DEVICE, "no HIP device available");
    if (dev < 0 || dev >= ndev) fail(ZV_ERR_ARG, "device %d out of range (%d devices)", dev, ndev);
    ZV_HIP(hipSetDevice(dev));
    hipDeviceProp_t prop;
    ZV_HIP(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) fail(ZV_ERR_DEVICE, "device %d is %s; this library is built for gfx950 only", dev, prop.gcnArchName);
    n_cu = prop.multiProcessorCount;
    lanes_.resize(1);
    ZV_HIP(hipStreamCreateWithFlags(&lanes_[0].stream, hipStreamNonBlocking));

    GgufFile g;
    g.open(path);
    auto kv = [&](const char *k) { return g.get_u32(std::string(KV_PREFIX) + k); };
    // all 15 keys are required, as in the reference (src/zerovox.cpp:39-56)
    hp.max_seq_len = kv("max_seq_len");
    hp.emb_dim = kv("emb_dim");
    hp.punct_emb_dim = kv("punct_emb_dim");
    hp.decoder_n_head = kv("decoder.n_head");
    hp.conv_filter_size = kv("decoder.conv_filter_size");
    hp.conv_kernel_size[0] = kv("decoder.conv_kernel_size.0");
    hp.conv_kernel_size[1] = kv("decoder.conv_kernel_size.1");
    hp.encoder_layer = kv("encoder.layer");
    hp.encoder_head = kv("encoder.head");
    hp.encoder_vp_filter_size = kv("encoder.vp_filter_size");
    hp.encoder_vp_kernel_size = kv("encoder.vp_kernel_size");
    hp.encoder_ve_n_bins = kv("encoder.ve_n_bins");
    hp.audio_sampling_rate = kv("audio.sampling_rate");
    hp.audio_num_mels = kv("audio.num_mels");
    hp.audio_hop_size = kv("audio.hop_size");

    const int Ed = (int)E();
    if (Ed % 16) fail(ZV_ERR_SHAPE, "emb_dim + punct_emb_dim = %d must be a multiple of 16", Ed);
    if (hp.audio_num_mels % 16) fail(ZV_ERR_SHAPE, "num_mels = %u must be a multiple of 16", hp.audio_num_mels);
    if (hp.encoder_head == 0 || Ed % hp.encoder_head) fail(ZV_ERR_SHAPE, "encoder.head = %u does not divide %d", hp.encoder_head, Ed);
    if (hp.encoder_vp_kernel_size != 3) fail(ZV_ERR_SHAPE, "vp_kernel_size = %u: the reference pads the second predictor conv with a literal 1 (src/fs2encoder.cpp:417), only 3 is a 'same' conv", hp.encoder_vp_kernel_size);
    char nm[128], nb[128];

    // ---------------- vocoder (src/hifigan.cpp:208-218; geometry from tensor shapes) ----------------
    const int M = (int)hp.audio_num_mels;
    voc_.mean = upload_vec(g, "hifigan.mean", M);
    voc_.scale = upload_vec(g, "hifigan.scale", M, 0, 1.f);
    voc_.in_conv = load_conv(g, "_meldec.input_conv.w", "_meldec.input_conv.b", M);
    // the reference pads the input and output convs for kernel_size = 7 whatever the file holds (src/hifigan.cpp:261,338)
    if (voc_.in_conv.K != 7) fail(ZV_ERR_SHAPE, "tensor _meldec.input_conv.w: kernel size %d, the reference pads for 7", voc_.in_conv.K);
    int C = voc_.in_conv.Cout;
    hp.voc_channels = C;
    int n_up = 0;
    while (n_up < 8)
    {
        snprintf(nm, sizeof(nm), "_meldec.upsamples.%d.1.w", n_up);
        if (!g.find(nm)) break;
        n_up++;
    }
    if (n_up == 0) fail(ZV_ERR_MISSING, "tensor '_meldec.upsamples.0.1.w' not found");
    // the stride is not stored in the file: the reference hard-codes 4 stages of {5,5,4,3} (src/zerovox.cpp:127-129);
    // every HiFi-GAN config has kernel = 2 * stride, which is what we derive, and a file whose strides differ is refused.
    static const int REF_SCALES[4] = {5, 5, 4, 3};
    if (n_up != 4) fail(ZV_ERR_SHAPE, "tensor _meldec.upsamples.%d.1.w: %s; the reference runs 4 upsample stages, the file has %d", std::min(n_up, 4),
                          n_up < 4 ? "missing" : "unexpected", n_up);
    int hop = 1;
    voc_.n_up = n_up;
    hp.voc_num_upsamples = n_up;
    int n_blocks = 0;
    while (true)
    {
        snprintf(nm, sizeof(nm), "_meldec.blocks.%d.convs1.0.1.w", n_blocks);
        if (!g.find(nm)) break;
        n_blocks++;
    }
    if (n_blocks == 0 || n_blocks % n_up) fail(ZV_ERR_SHAPE, "%d residual blocks do not divide over %d upsample stages", n_blocks, n_up);
    voc_.n_rb = n_blocks / n_up;
    if (voc_.n_rb != 3) fail(ZV_ERR_SHAPE, "num_resblocks = %d: the schedule (like the reference caller) is built for 3", voc_.n_rb);
    hp.voc_num_resblocks = voc_.n_rb;
    for (int i = 0; i < n_up; i++)
    {
        snprintf(nm, sizeof(nm), "_meldec.upsamples.%d.1.w", i);
        const int K = (int)g.get(nm).ne[0];
        if (K % 2) fail(ZV_ERR_SHAPE, "tensor %s: odd transposed-conv kernel %d", nm, K);
        const int s = K / 2;
        if (s != REF_SCALES[i]) fail(ZV_ERR_SHAPE, "tensor %s: kernel %d gives stride %d, the reference uses %d at stage %d", nm, K, s, REF_SCALES[i], i);
        voc_.scales[i] = s;
        hp.voc_upsample_scales[i] = s;
        hop *= s;
        voc_.ups[i] = load_upsample(g, i, s, C);
        // the schedule's buffers are sized for channel halving per stage (every HiFi-GAN generator; 512 -> 32 here)
        if ((int)g.get(nm).ne[2] * 2 != C) fail(ZV_ERR_SHAPE, "tensor %s: %lld output channels, expected %d (channels halve per upsample stage)", nm, (long long)g.get(nm).ne[2], C / 2);
        C = (int)g.get(nm).ne[2];
        for (int j = 0; j < voc_.n_rb; j++)
            for (int d = 0; d < voc_.n_dil; d++)
            {
                ResPair rp;
                const int n = i * voc_.n_rb + j;
                snprintf(nm, sizeof(nm), "_meldec.blocks.%d.convs1.%d.1.w", n, d);
                snprintf(nb, sizeof(nb), "_meldec.blocks.%d.convs1.%d.1.b", n, d);
                rp.c1 = load_conv(g, nm, nb, C);
                snprintf(nm, sizeof(nm), "_meldec.blocks.%d.convs2.%d.1.w", n, d);
                snprintf(nb, sizeof(nb), "_meldec.blocks.%d.convs2.%d.1.b", n, d);
                rp.c2 = load_conv(g, nm, nb, C);
                if (rp.c1.Cout != C || rp.c2.Cout != C) fail(ZV_ERR_SHAPE, "residual block %d: channel mismatch", n);
                if (rp.c1.K == rp.c2.K && pair_supported(rp.c1.Cout_p, rp.c1.K))
                {
                    std::vector<uint16_t> pk(pair_weight_halfs(rp.c1.Cout_p, rp.c1.K));
                    void **dst[2] = {&rp.p1, &rp.p2};
                    const char *fmt[2] = {"_meldec.blocks.%d.convs1.%d.1.w", "_meldec.blocks.%d.convs2.%d.1.w"};
                    for (int q = 0; q < 2; q++)
                    {
                        snprintf(nm, sizeof(nm), fmt[q], n, d);
                        pack_pair_weight((const uint16_t *)g.get(nm).data, rp.c1.K, C, rp.c1.Cout_p, pk.data());
                        *dst[q] = dev_alloc(pk.size() * 2 + 8192);
                        ZV_HIP(hipMemcpy(*dst[q], pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
                        {   // the same weights in 16 x 16 x 32 fragment order (resblock_pair_kernel, resblock_block32_kernel): conv1 as the A operand, conv2 as B
                            std::vector<uint16_t> xk(pair_weight16_halfs(rp.c1.Cout_p, rp.c1.K));
                            pack_pair_weight16((const uint16_t *)g.get(nm).data, rp.c1.K, C, rp.c1.Cout_p, xk.data(), q == 1);
                            void **xd = q ? &rp.x2 : &rp.x1;
                            *xd = dev_alloc(xk.size() * 2 + 8192);
                            ZV_HIP(hipMemcpy(*xd, xk.data(), xk.size() * 2, hipMemcpyHostToDevice));
                        }
                        if (rp.c1.Cout_p == 64)
                        {
                            std::vector<uint16_t> rk(pair_ring_weight_halfs(64, rp.c1.K));
                            pack_pair_weight_ring((const uint16_t *)g.get(nm).data, rp.c1.K, C, 64, rk.data(), q == 1);
                            void **rd = q ? &rp.r2 : &rp.r1;
                            *rd = dev_alloc(rk.size() * 2);
                            ZV_HIP(hipMemcpy(*rd, rk.data(), rk.size() * 2, hipMemcpyHostToDevice));
                        }
                    }
                }
                if (i == 0 && d == 0) hp.voc_resblock_kernels[j] = rp.c1.K;
                voc_.pairs.push_back(rp);
            }
    }
    if ((uint32_t)hop != hp.audio_hop_size) fail(ZV_ERR_SHAPE, "product of upsample scales %d != audio.hop_size %u", hop, hp.audio_hop_size);
    {
        const GgufTensor &w = g.get("_meldec.output_conv.1.w");
        const GgufTensor &b = g.get("_meldec.output_conv.1.b");
        if (w.type != GGML_F16 || w.ne[1] != C || w.ne[2] != 1) fail(ZV_ERR_SHAPE, "_meldec.output_conv.1.w: expected f16 [K,%d,1]", C);
        if (b.type != GGML_F32 || b.nelements() != 1) fail(ZV_ERR_SHAPE, "_meldec.output_conv.1.b: expected f32 [1]");
        if ((hp.voc_channels >> n_up) != (uint32_t)C) fail(ZV_ERR_SHAPE, "vocoder channels %u do not halve down to %d over %d stages", hp.voc_channels, C, n_up);
        voc_.out_K = (int)w.ne[0];
        if (voc_.out_K != 7) fail(ZV_ERR_SHAPE, "tensor _meldec.output_conv.1.w: kernel size %d, the reference pads for 7", voc_.out_K);
        // the output conv keeps a tile's operand rows and its weights in LDS (conv_plan.h): 7 taps take at most 112 channels
        if (!out_conv_supported(C, voc_.out_K))
            fail(ZV_ERR_SHAPE, "tensor _meldec.output_conv.1.w: %d input channels; the output conv runs at most 112 (%zu bytes of LDS, %zu allowed)", C,
                 out_conv_lds_bytes(C, voc_.out_K), LDS_DEFAULT);
        voc_.out_C = C;
        const int Cp = round_up(C, 16);
        std::vector<uint16_t> h((size_t)voc_.out_K * Cp, 0);
        const uint16_t *src = (const uint16_t *)w.data;
        for (int ic = 0; ic < C; ic++)
            for (int k = 0; k < voc_.out_K; k++) h[(size_t)k * Cp + ic] = src[(size_t)ic * voc_.out_K + k];
        voc_.out_w = (uint16_t *)dev_alloc(h.size() * 2);
        ZV_HIP(hipMemcpy(voc_.out_w, h.data(), h.size() * 2, hipMemcpyHostToDevice));
        voc_.out_b = ((const float *)b.data)[0];
    }
    // what the schedule's decisions read of all this (voc_plan.h)
    static_assert(sizeof(voc_.scales) / sizeof(voc_.scales[0]) <= VOC_MAX_STAGES, "VocGeom::st holds every upsample stage");
    if (voc_.n_rb != VOC_BRANCHES || voc_.n_dil > VOC_MAX_DIL) fail(ZV_ERR_SHAPE, "internal: %d branches of %d dilations do not fit the plan's geometry", voc_.n_rb, voc_.n_dil);
    voc_geom_.n_up = n_up;
    voc_geom_.n_dil = voc_.n_dil;
    for (int d = 0; d < voc_.n_dil; d++) voc_geom_.dil[d] = voc_.dil[d];
    voc_geom_.in_Cout_p = voc_.in_conv.Cout_p;
    for (int i = 0; i < n_up; i++)
    {
        VocStageGeom &s = voc_geom_.st[i];
        s.scale = voc_.scales[i];
        s.Cp = round_up(voc_.in_conv.Cout >> (i + 1), 16);
        s.up_gemm = voc_.ups[i].w8 != nullptr;
        s.up_Cin_p = voc_.ups[i].Cin_p;
        for (int j = 0; j < voc_.n_rb; j++)
            for (int d = 0; d < voc_.n_dil; d++)
            {
                const ResPair &rp = voc_.pairs[((size_t)i * voc_.n_rb + j) * voc_.n_dil + d];
                s.pair[j][d] = VocPairGeom{rp.c1.K, rp.c2.K, rp.p1 != nullptr, rp.r1 && rp.r2, rp.x1 != nullptr};
            }
    }

    // ---------------- decoder (src/stylettsdec.cpp:33-66,163-168,220-239,334-340) ----------------
    {
        dec_.M = M;
        const GgufTensor &a0 = g.get("_mel_decoder.asr_res.0.w");
        dec_.R = (int)a0.ne[2];
        const int R = dec_.R, B = 2 * Ed, CAT = B + R;
        if (R % 16) fail(ZV_ERR_SHAPE, "residual_dim = %d must be a multiple of 16", R);
        const int edims[2][2] = {{Ed, B}, {B, B}};
        for (int i = 0; i < 2; i++)
        {
            DecBlk &b = dec_.enc[i];
            b.cin = edims[i][0];
            b.cout = edims[i][1];
            b.learned_sc = b.cin != b.cout;
            snprintf(nm, sizeof(nm), "_mel_decoder.encode.%d.conv1.w", i);
            snprintf(nb, sizeof(nb), "_mel_decoder.encode.%d.conv1.b", i);
            b.conv1 = load_conv(g, nm, nb, b.cin, true);
            snprintf(nm, sizeof(nm), "_mel_decoder.encode.%d.conv2.w", i);
            snprintf(nb, sizeof(nb), "_mel_decoder.encode.%d.conv2.b", i);
            b.conv2 = load_conv(g, nm, nb, b.cin, true);
            if (b.conv1.Cout != b.cin || b.conv2.Cout != b.cout) fail(ZV_ERR_SHAPE, "_mel_decoder.encode.%d: channel mismatch", i);
            if (b.learned_sc)
            {
                snprintf(nm, sizeof(nm), "_mel_decoder.encode.%d.conv1x1.w", i);
                b.sc = load_conv(g, nm, "", b.cin, true);
            }
            snprintf(nm, sizeof(nm), "_mel_decoder.encode.%d.norm1.w", i); b.n1w = upload_vec(g, nm, b.cin);
            snprintf(nm, sizeof(nm), "_mel_decoder.encode.%d.norm1.b", i); b.n1b = upload_vec(g, nm, b.cin);
            snprintf(nm, sizeof(nm), "_mel_decoder.encode.%d.norm2.w", i); b.n2w = upload_vec(g, nm, b.cin);
            snprintf(nm, sizeof(nm), "_mel_decoder.encode.%d.norm2.b", i); b.n2b = upload_vec(g, nm, b.cin);
        }
        dec_.asr0 = load_conv(g, "_mel_decoder.asr_res.0.w", "_mel_decoder.asr_res.0.b", Ed);
        dec_.asr1w = upload_vec(g, "_mel_decoder.asr_res.1.w", R);
        dec_.asr1b = upload_vec(g, "_mel_decoder.asr_res.1.b", R);
        const int ddims[5][2] = {{CAT, B}, {CAT, B}, {CAT, Ed}, {Ed, Ed}, {Ed, Ed}};
        // all ten AdaIN fc layers (Linear(E -> 2C)) concatenated into one GEMV; `extra` carries the +1 of gamma
        int fc_out = 0;
        for (int i = 0; i < 5; i++) fc_out += 2 * ddims[i][0] + 2 * ddims[i][1];
        std::vector<float> W((size_t)fc_out * Ed), Bv(fc_out + 64, 0.f), Ex(fc_out + 64, 0.f);
        int o = 0;
        for (int i = 0; i < 5; i++)
        {
            DecBlk &b = dec_.dec[i];
            b.cin = ddims[i][0];
            b.cout = ddims[i][1];
            b.learned_sc = b.cin != b.cout;
            snprintf(nm, sizeof(nm), "_mel_decoder.decode.%d.conv1.w", i);
            snprintf(nb, sizeof(nb), "_mel_decoder.decode.%d.conv1.b", i);
            b.conv1 = load_conv(g, nm, nb, b.cin, true);
            snprintf(nm, sizeof(nm), "_mel_decoder.decode.%d.conv2.w", i);
            snprintf(nb, sizeof(nb), "_mel_decoder.decode.%d.conv2.b", i);
            b.conv2 = load_conv(g, nm, nb, b.cout, true);
            if (b.conv1.Cout != b.cout || b.conv2.Cout != b.cout) fail(ZV_ERR_SHAPE, "_mel_decoder.decode.%d: channel mismatch", i);
            if (b.learned_sc)
            {
                snprintf(nm, sizeof(nm), "_mel_decoder.decode.%d.conv1x1.w", i);
                b.sc = load_conv(g, nm, "", b.cin, true);
            }
            for (int k = 1; k <= 2; k++)
            {
                const int Cn = (k == 1) ? b.cin : b.cout;
                snprintf(nm, sizeof(nm), "_mel_decoder.decode.%d.norm%d.fc.w", i, k);
                snprintf(nb, sizeof(nb), "_mel_decoder.decode.%d.norm%d.fc.b", i, k);
                const GgufTensor &fw = g.get(nm), &fb = g.get(nb);
                if (fw.type != GGML_F32 || fw.ne[0] != Ed || fw.ne[1] != 2 * Cn) fail(ZV_ERR_SHAPE, "tensor %s: expected f32 [%d, %d]", nm, Ed, 2 * Cn);
                if (fb.type != GGML_F32 || fb.nelements() != 2 * Cn) fail(ZV_ERR_SHAPE, "tensor %s: expected f32 [%d]", nb, 2 * Cn);
                memcpy(W.data() + (size_t)o * Ed, fw.data, (size_t)2 * Cn * Ed * 4);
                memcpy(Bv.data() + o, fb.data, (size_t)2 * Cn * 4);
                for (int c = 0; c < Cn; c++) Ex[o + c] = 1.0f;
                (k == 1 ? b.g1 : b.g2) = o;
                o += 2 * Cn;
            }
        }
        dec_.fc_out = fc_out;
        dec_.fcW = (float *)dev_alloc(W.size() * 4);
        dec_.fcB = (float *)dev_alloc(Bv.size() * 4);
        dec_.fcExtra = (float *)dev_alloc(Ex.size() * 4);
        ZV_HIP(hipMemcpy(dec_.fcW, W.data(), W.size() * 4, hipMemcpyHostToDevice));
        ZV_HIP(hipMemcpy(dec_.fcB, Bv.data(), Bv.size() * 4, hipMemcpyHostToDevice));
        ZV_HIP(hipMemcpy(dec_.fcExtra, Ex.data(), Ex.size() * 4, hipMemcpyHostToDevice));
        dec_.to_out = load_conv(g, "_mel_decoder.to_out.0.w", "_mel_decoder.to_out.0.b", Ed);
        if (dec_.to_out.Cout != M) fail(ZV_ERR_SHAPE, "_mel_decoder.to_out.0.w: expected %d output channels", M);
    }

    // ---------------- encoder (src/fs2encoder.cpp:29-62,152-171,256-261,344-382,504-505) ----------------
    {
        const GgufTensor &we = g.get("_pe._enc.src_word_emb.w");
        const GgufTensor &pe = g.get("_pe._enc.punct_embed.w");
        const GgufTensor &st = g.get("sinusoid_encoding_table");
        if (we.ne[0] != hp.emb_dim || pe.ne[0] != hp.punct_emb_dim || st.ne[0] != Ed) fail(ZV_ERR_SHAPE, "embedding / position tables do not match emb_dim/punct_emb_dim");
        if (we.ne[1] < 1 || pe.ne[1] < 1 || st.ne[1] < 1) fail(ZV_ERR_SHAPE, "empty embedding / position table");
        enc_.wemb = upload_f32(we);
        enc_.pemb = upload_f32(pe);
        enc_.posenc = upload_f32(st);
        enc_.posenc_rows = (int)st.ne[1];
        enc_.wemb_rows = (int)we.ne[1];          // ids are checked against what the file holds (155 / 7 rows in the
        enc_.pemb_rows = (int)pe.ne[1];          // reference's checkpoints, src/zerovox.h:35-36)
        enc_.layers.resize(hp.encoder_layer);
        for (uint32_t l = 0; l < hp.encoder_layer; l++)
        {
            EncLayer &L = enc_.layers[l];
            std::vector<float> W((size_t)3 * Ed * Ed), Bv(3 * Ed + 64, 0.f);
            const char *names[3] = {"w_qs", "w_ks", "w_vs"};
            for (int i = 0; i < 3; i++)
            {
                snprintf(nm, sizeof(nm), "_pe._enc.laystk.%u.slf_attn.%s.w", l, names[i]);
                snprintf(nb, sizeof(nb), "_pe._enc.laystk.%u.slf_attn.%s.b", l, names[i]);
                const GgufTensor &w = g.get(nm), &b = g.get(nb);
                if (w.type != GGML_F32 || w.ne[0] != Ed || w.ne[1] != Ed || b.nelements() != Ed) fail(ZV_ERR_SHAPE, "tensor %s: expected f32 [%d, %d]", nm, Ed, Ed);
                memcpy(W.data() + (size_t)i * Ed * Ed, w.data, (size_t)Ed * Ed * 4);
                memcpy(Bv.data() + (size_t)i * Ed, b.data, (size_t)Ed * 4);
            }
            L.qkvW = (float *)dev_alloc(W.size() * 4);
            L.qkvB = (float *)dev_alloc(Bv.size() * 4);
            ZV_HIP(hipMemcpy(L.qkvW, W.data(), W.size() * 4, hipMemcpyHostToDevice));
            ZV_HIP(hipMemcpy(L.qkvB, Bv.data(), Bv.size() * 4, hipMemcpyHostToDevice));
            snprintf(nm, sizeof(nm), "_pe._enc.laystk.%u.slf_attn.fc.w", l);
            const GgufTensor &fw = g.get(nm);
            if (fw.type != GGML_F32 || fw.ne[0] != Ed || fw.ne[1] != Ed) fail(ZV_ERR_SHAPE, "tensor %s: expected f32 [%d, %d]", nm, Ed, Ed);
            L.fcW = upload_f32(fw);
            snprintf(nm, sizeof(nm), "_pe._enc.laystk.%u.slf_attn.fc.b", l); L.fcB = upload_vec(g, nm, Ed);
            snprintf(nm, sizeof(nm), "_pe._enc.laystk.%u.slf_attn.layer_norm.w", l); L.ln1w = upload_vec(g, nm, Ed);
            snprintf(nm, sizeof(nm), "_pe._enc.laystk.%u.slf_attn.layer_norm.b", l); L.ln1b = upload_vec(g, nm, Ed);
            snprintf(nm, sizeof(nm), "_pe._enc.laystk.%u.pos_ffn.layer_norm.w", l); L.ln2w = upload_vec(g, nm, Ed);
            snprintf(nm, sizeof(nm), "_pe._enc.laystk.%u.pos_ffn.layer_norm.b", l); L.ln2b = upload_vec(g, nm, Ed);
            snprintf(nm, sizeof(nm), "_pe._enc.laystk.%u.pos_ffn.w_1.w", l);
            snprintf(nb, sizeof(nb), "_pe._enc.laystk.%u.pos_ffn.w_1.b", l);
            L.w1 = load_conv(g, nm, nb, Ed);
            snprintf(nm, sizeof(nm), "_pe._enc.laystk.%u.pos_ffn.w_2.w", l);
            snprintf(nb, sizeof(nb), "_pe._enc.laystk.%u.pos_ffn.w_2.b", l);
            L.w2 = load_conv(g, nm, nb, L.w1.Cout);
            if (L.w2.Cout != Ed) fail(ZV_ERR_SHAPE, "pos_ffn.w_2 must map back to %d channels", Ed);
            if (L.w1.K != (int)hp.conv_kernel_size[0] || L.w2.K != (int)hp.conv_kernel_size[1]) fail(ZV_ERR_SHAPE, "pos_ffn kernel sizes do not match the KV keys");
        }
        auto load_vp = [&](VarPred &v, const char *prefix) {
            snprintf(nm, sizeof(nm), "%s.conv_layer.conv1d_1.conv.w", prefix);
            snprintf(nb, sizeof(nb), "%s.conv_layer.conv1d_1.conv.b", prefix);
            v.c1 = load_conv(g, nm, nb, Ed);
            v.V = v.c1.Cout;
            snprintf(nm, sizeof(nm), "%s.conv_layer.conv1d_2.conv.w", prefix);
            snprintf(nb, sizeof(nb), "%s.conv_layer.conv1d_2.conv.b", prefix);
            v.c2 = load_conv(g, nm, nb, v.V);
            if (v.c1.K != 3 || v.c2.K != 3 || v.c2.Cout != v.V) fail(ZV_ERR_SHAPE, "%s: predictor convs must be k3, %d -> %d", prefix, v.V, v.V);
            snprintf(nm, sizeof(nm), "%s.conv_layer.layer_norm_1.w", prefix); v.l1w = upload_vec(g, nm, v.V);
            snprintf(nm, sizeof(nm), "%s.conv_layer.layer_norm_1.b", prefix); v.l1b = upload_vec(g, nm, v.V);
            snprintf(nm, sizeof(nm), "%s.conv_layer.layer_norm_2.w", prefix); v.l2w = upload_vec(g, nm, v.V);
            snprintf(nm, sizeof(nm), "%s.conv_layer.layer_norm_2.b", prefix); v.l2b = upload_vec(g, nm, v.V);
            snprintf(nm, sizeof(nm), "%s.linear_layer.w", prefix); v.lw = upload_vec(g, nm, v.V);
            snprintf(nm, sizeof(nm), "%s.linear_layer.b", prefix); v.lb = upload_vec(g, nm, 1);
        };
        load_vp(enc_.dur, "_pe._var_adapt.duration_predictor");
        load_vp(enc_.pitch, "_pe._var_adapt.pitch_predictor");
        load_vp(enc_.energy, "_pe._var_adapt.engy_pred");
        const GgufTensor &pemb = g.get("_pe._var_adapt.pitch_embedding.w"), &eemb = g.get("_pe._var_adapt.energy_embedding.w");
        if (pemb.ne[0] != Ed || pemb.ne[1] != hp.encoder_ve_n_bins || eemb.ne[0] != Ed || eemb.ne[1] != hp.encoder_ve_n_bins)
            fail(ZV_ERR_SHAPE, "pitch/energy embedding: expected f32 [%d, %u]", Ed, hp.encoder_ve_n_bins);
        enc_.pitch_emb = upload_f32(pemb);
        enc_.energy_emb = upload_f32(eemb);
    }
    ZV_HIP(hipDeviceSynchronize());
}

}  // namespace zv
