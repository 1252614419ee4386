"""CPU: the drop-in boundary without a GPU — the C-ABI library loads and exports every declared symbol,
the product's C++ GGUF reader parses what the contract says, errors map to status codes, the WAV writer and
the synthetic-checkpoint generator are deterministic."""
import hashlib
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "zerovox_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(zv_[a-z0-9_]+)\s*\(", header)))
    assert declared, "no declarations found"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/zerovox_amd.h but not exported"
    assert sorted(capi.SYMBOLS) == declared
    assert b"gfx950" in lib.zv_version()


def test_facade_header_mirrors_reference_signatures():
    """same class names and eval() signatures as the reference's src/zerovox.h:191,323,378,408-413"""
    h = open(os.path.join(ROOT, "zerovox.cpp_amd", "csrc", "zerovox.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert "uint32_t eval(const int32_t *src_seq_data, const int32_t *puncts_data, const float *style_embed_data, uint32_t num_phonemes, float *x);" in flat
    assert "void eval(const float *enc_seq_data, const float *spk_emb_data, float *mel);" in flat
    assert "void eval(const float *mel, float *wav);" in flat
    assert "ZeroVOXModel(const std::string &fname);" in flat and "bool write_wav_file(const std::string &fname);" in flat
    for cls in ("class FS2Encoder", "class StyleTTSDecoder", "class HiFiGAN", "class ZeroVOXModel"):
        assert cls in h


def test_cpp_gguf_reader_matches_contract(tmp_path):
    from zerovox_cpp_amd import capi, gguf, synth
    for trim in (False, True):
        p = str(tmp_path / f"t{int(trim)}.gguf")
        synth.write_checkpoint(p, synth.TINY, 5, trim_dims=trim)
        _, tensors = gguf.read_gguf(p)
        n, T = capi.gguf_inspect(p)
        assert n == len(tensors) == 291 and T == synth.TINY.max_seq_len
        names = list(tensors)
        for i in (0, 1, 2, 57, n - 1):
            _, _, name, typ, ne = capi.gguf_inspect(p, i)
            arr = tensors[names[i]]
            assert name == names[i]
            assert typ == {np.dtype(np.float32): 0, np.dtype(np.float16): 1}[arr.dtype]
            assert ne == list(arr.shape[::-1]) + [1] * (4 - arr.ndim)       # missing dims padded with 1


def test_gguf_error_mapping(tmp_path):
    from zerovox_cpp_amd import capi, gguf, synth
    with pytest.raises(capi.ZvError) as e:
        capi.gguf_inspect(str(tmp_path / "missing.gguf"))
    assert e.value.status == 1                                   # ZV_ERR_IO
    bad = tmp_path / "bad.gguf"
    bad.write_bytes(b"GGUX" + b"\0" * 64)
    with pytest.raises(capi.ZvError) as e:
        capi.gguf_inspect(str(bad))
    assert e.value.status == 2                                   # ZV_ERR_FORMAT
    good = str(tmp_path / "g.gguf")
    synth.write_checkpoint(good, synth.TINY, 5)
    data = open(good, "rb").read()
    trunc = tmp_path / "trunc.gguf"
    trunc.write_bytes(data[: len(data) // 2])
    with pytest.raises(capi.ZvError) as e:
        capi.gguf_inspect(str(trunc))
    assert e.value.status == 2
    v2 = tmp_path / "v2.gguf"
    v2.write_bytes(data[:4] + struct.pack("<I", 2) + data[8:])
    with pytest.raises(capi.ZvError) as e:
        capi.gguf_inspect(str(v2))
    assert e.value.status == 2 and "version" in str(e.value)
    # a required KV missing -> ZV_ERR_MISSING (the reference exit(1)s here, src/zerovox.h:452-454)
    kv = synth.TINY.kv()
    kv.pop("zerovox-resnet-fs2-styletts.max_seq_len")
    nokey = str(tmp_path / "nokey.gguf")
    gguf.write_gguf(nokey, kv, synth.make_tensors(synth.TINY, 5)[:3])
    with pytest.raises(capi.ZvError) as e:
        capi.gguf_inspect(nokey)
    assert e.value.status == 3


def test_model_load_fails_loudly_without_gpu(tmp_path):
    """no CPU fallback: without a gfx950 device zv_model_load must fail with ZV_ERR_DEVICE"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from zerovox_cpp_amd import capi, synth
    p = str(tmp_path / "t.gguf")
    synth.write_checkpoint(p, synth.TINY, 5)
    with pytest.raises(capi.ZvError) as e:
        capi.Model(p, 0)
    assert e.value.status == 6


def test_wav_writer(tmp_path):
    from zerovox_cpp_amd import capi
    wav = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 1e-5], np.float32)
    p = str(tmp_path / "o.wav")
    capi.write_wav(p, wav, 22050)
    b = open(p, "rb").read()
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and b[36:40] == b"data"
    fmt, ch, sr, br, ba, bits = struct.unpack("<HHIIHH", b[20:36])
    assert (fmt, ch, sr, br, ba, bits) == (1, 1, 22050, 44100, 2, 16)
    assert struct.unpack("<I", b[40:44])[0] == 16 and struct.unpack("<I", b[4:8])[0] == 36 + 16
    pcm = np.frombuffer(b[44:], np.int16)
    assert pcm.tolist() == [0, 16384, -16384, 32767, -32767, 32767, -32768, 0]


def test_synthetic_checkpoint_is_deterministic():
    """the GPU box regenerates the goldens' checkpoints from (geometry, seed): pin the generator"""
    from zerovox_cpp_amd import synth
    t = dict(synth.make_tensors(synth.TINY, 1234))
    h = hashlib.sha256()
    for k in sorted(t):
        h.update(k.encode())
        h.update(np.ascontiguousarray(t[k]).tobytes())
    assert h.hexdigest() == PINNED_TINY_SHA256, h.hexdigest()
    u = synth.u01(7, "x", 4)
    assert np.allclose(u, synth.u01(7, "x", 4)) and not np.allclose(u, synth.u01(8, "x", 4))
    ids, puncts, style = synth.encoder_inputs(synth.TINY, 5, 200)
    assert ids.min() >= 1 and ids.max() <= 154 and puncts.min() >= 0 and puncts.max() <= 6


PINNED_TINY_SHA256 = "b7573a897ac23670e07dd746b9e3be836911ebd22bd02463eeefe2853c457d68"


CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zerovox.cpp_amd", "zerovox")


def test_cli_help_info_and_loud_failure(tmp_path):
    """`zerovox` is the counterpart of the reference's main (src/zerovox.cpp:396-406): same defaults, plus flags.
    Without a GPU it must list a checkpoint (--info needs no device) and fail loudly on synthesis."""
    import subprocess
    import torch
    from zerovox_cpp_amd import synth
    assert os.access(CLI, os.X_OK), "run __graft_entry__.build() first"
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "medium-ldec.gguf" in r.stdout and "foo.wav" in r.stdout
    r = subprocess.run([CLI, "--bogus"], capture_output=True, text=True)
    assert r.returncode == 2
    p = str(tmp_path / "t.gguf")
    synth.write_checkpoint(p, synth.TINY, 5)
    r = subprocess.run([CLI, "-m", p, "--info"], capture_output=True, text=True)
    assert r.returncode == 0 and "hifigan.mean" in r.stdout and "sinusoid_encoding_table" in r.stdout
    r = subprocess.run([CLI, "-m", str(tmp_path / "missing.gguf"), "--info"], capture_output=True, text=True)
    assert r.returncode == 1 and "zerovox:" in r.stderr
    if not torch.cuda.is_available():
        r = subprocess.run([CLI, "-m", p, "-o", str(tmp_path / "o.wav")], capture_output=True, text=True)
        assert r.returncode == 1 and "zerovox:" in r.stderr and not os.path.exists(tmp_path / "o.wav")


def test_loader_survives_corrupt_files_under_sanitizers():
    """host code of the library built with -fsanitize=address,undefined (GPU ASan does not exist on this pool): the
    GGUF loader and the WAV writer are driven with ~2 000 truncated / corrupted checkpoints and must answer each
    with a status code — no crash, no out-of-bounds read, no leak (tests/native/host_fuzz.cpp)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["bash", os.path.join(root, "scripts", "asan_host.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "no crash" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def _build_callsite(out_dir):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(out_dir), "facade_callsite")
    pkg = os.path.join(root, "zerovox.cpp_amd")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(root, "tests", "native", "facade_callsite.cpp"),
                        "-o", exe, "-L" + pkg, "-l:libzerovox_amd.so", "-Wl,-rpath," + pkg], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_reference_style_call_site_compiles(tmp_path):
    """tests/native/facade_callsite.cpp constructs and drives the three stage classes with the argument lists of the
    reference's own driver (src/zerovox.cpp:104-137, 326-334), using the ggml handle names: it must build against
    csrc/zerovox.h without warnings and, with no GPU, fail with a message instead of aborting"""
    import subprocess
    import torch
    from zerovox_cpp_amd import synth
    exe = _build_callsite(tmp_path)
    if not torch.cuda.is_available():
        p = str(tmp_path / "t.gguf")
        synth.write_checkpoint(p, synth.TINY, 5)
        r = subprocess.run([exe, p, "8", str(tmp_path / "o.f32")], capture_output=True, text=True)
        assert r.returncode == 1 and "facade_callsite:" in r.stderr


def test_receptive_radius_of_the_vocoder_geometries(ckpt):
    """parity_helpers.receptive_radius (the bound tests/test_gpu_vocoder_geometries.py holds zv_vocoder_halo_frames to) on synth.MEDIUM:
    3 / 7 / 11 everywhere, 60 rows per stage -> 20 frames; medium_rb_c1c2 (one convs2 of 13 taps) stays at 20; medium_rb_c2wide
    (convs2 of 25 taps in the 11-tap branch) reaches 25 frames — beyond the 23 of a halo counted from the convs1 of dilation 0
    alone, so that geometry fails a halo that leaves convs2 out"""
    import math
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from parity_helpers import receptive_radius, upsample_window

    def halo_from_convs1_d0(g, t):
        """ceil(sum of per-layer reaches in frames) + 1, each stage's residual blocks counted as (K - 1) / 2 (sum d + 3) with K the
        widest convs1 of dilation 0"""
        frames, rate = (t["_meldec.input_conv.w"].shape[2] - 1) // 2, 1
        for i, s in enumerate(g.upsample_scales):
            lo, hi = upsample_window(t[f"_meldec.upsamples.{i}.1.w"].shape[2], s)
            frames += (2 * max(-lo, hi) + 1) / rate
            rate *= s
            k = max(t[f"_meldec.blocks.{3 * i + j}.convs1.0.1.w"].shape[2] for j in range(3))
            frames += (k - 1) // 2 * (sum(g.resblock_dilations) + 3) / rate
        frames += (t["_meldec.output_conv.1.w"].shape[2] - 1) // 2 / rate
        return math.ceil(frames) + 1

    want = {"medium": 20, "medium_rb_c1c2": 20, "medium_rb_c2wide": 25}
    for name, r in want.items():
        _, g, tensors = ckpt(name)
        assert receptive_radius(g, tensors) == r, name
        assert halo_from_convs1_d0(g, tensors) == 23, name


def test_voc_width_geometries_reach_what_they_claim(ckpt):
    """synth.VOC_WIDTH_GEOMETRIES: the width changes no tap count, so the receptive radius stays medium's 20 frames (the bound
    tests/test_gpu_vocoder_widths.py holds zv_vocoder_halo_frames to); the tensors carry the width, halved per stage, the reference's
    strides and 3 / 7 / 11 taps; the stages are the real and padded channel counts synth.py names (496: pad channels in every stage,
    15.5 output tiles of the input conv; 768 and the first stage of 1024: no width a fused kernel takes); and the first upsample conv
    of 768 channels splits into 7 groups of 8 tiles on conv_gemm_kernel and 4 tiles at nt_begin = 56"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from parity_helpers import conv_gemm_groups, conv_gemm_tiles, receptive_radius
    from zerovox_cpp_amd import synth
    stages = {"small_v256": ((128, 64, 32, 16), (128, 64, 32, 16)), "small_v496": ((248, 124, 62, 31), (256, 128, 64, 32)),
              "small_v768": ((384, 192, 96, 48), (384, 192, 96, 48)), "small_v1024": ((512, 256, 128, 64), (512, 256, 128, 64))}
    assert tuple(stages) == synth.VOC_WIDTH_GEOMETRIES
    fused = (32, 64, 128, 256)                              # csrc/conv_plan.h pair_supported
    small = synth.SMALL
    for name, (real, padded) in stages.items():
        _, g, t = ckpt(name)
        assert (g.E, g.conv_filter_size, g.encoder_layer, g.num_mels, g.max_seq_len) == (small.E, small.conv_filter_size, small.encoder_layer,
                                                                                        small.num_mels, small.max_seq_len), name
        assert g.upsample_scales == (5, 5, 4, 3) and g.resblock_kernels == (3, 7, 11) and g.hop_size == 300 and g.voc_kernel_size == 7, name
        assert receptive_radius(g, t) == 20, name
        C = g.voc_channels
        assert C % 16 == 0 and t["_meldec.input_conv.w"].shape == (C, g.num_mels, 7), name
        for i, (c, cp) in enumerate(zip(real, padded)):
            assert c == C >> (i + 1) and cp == (c + 15) // 16 * 16, (name, i)
            assert t[f"_meldec.upsamples.{i}.1.w"].shape == (c, C >> i, 2 * g.upsample_scales[i]), (name, i)
            for j, k in enumerate(g.resblock_kernels):
                for d in range(3):
                    assert t[f"_meldec.blocks.{3 * i + j}.convs1.{d}.1.w"].shape == (c, c, k), (name, i, j, d)
                    assert t[f"_meldec.blocks.{3 * i + j}.convs2.{d}.1.w"].shape == (c, c, k), (name, i, j, d)
        assert t["_meldec.output_conv.1.w"].shape == (1, real[3], 7), name
    assert all(cp in fused for cp in stages["small_v496"][1]) and all(c != cp for c, cp in zip(*stages["small_v496"]))
    assert (496 + 15) // 16 * 16 == 496 and 496 % 32 == 16                     # the input conv's last output tile is half padding
    assert not any(cp in fused for cp in stages["small_v768"][1]) and stages["small_v1024"][1][0] not in fused
    assert [cp in fused for cp in stages["small_v256"][1]] == [True, True, True, False]
    assert (5 * 384 // 32, conv_gemm_groups(5 * 384), conv_gemm_tiles(5 * 384)) == (60, 7, 56)


def test_encdec_geometries_reach_what_they_claim(ckpt):
    """synth.ENCDEC_GEOMETRIES: every one is legal for the loader (E % 16 == 0, H divides E, odd FFN taps, num_mels % 16 == 0) and
    splits its decoder convs (E and 2E output channels) over conv_gemm_kernel and the generic kernel as synth.py says — e576 / e720
    / e304 leave 2 / 4, 7 / 5 and 2 / 3 tiles at nt_begin > 0 (medium's 17 / 33 tiles leave one, which the GEMM takes; e1024's
    none); e576's head dim is the matrix-core attention's widest, e720's V turns the LayerNorm tails off alone.  And the tensors
    carry the KVs' shapes"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from parity_helpers import ATT_NS_MAX, LN_TAIL_MAX, conv_tile_split
    from zerovox_cpp_amd import synth
    split = {"medium": ((17, 17, 0), (33, 33, 0)), "medium_e576": ((18, 16, 2), (36, 32, 4)),
             "medium_e720": ((23, 16, 7), (45, 40, 5)), "small_e304": ((10, 8, 2), (19, 16, 3)),
             "medium_e1024": ((32, 32, 0), (64, 64, 0))}
    assert set(split) == {"medium", *synth.ENCDEC_GEOMETRIES}
    for name, want in split.items():
        g = synth.GEOMETRIES[name]
        E, H = g.E, g.encoder_head
        assert E % 16 == 0 and E % H == 0 and g.num_mels % 16 == 0, name
        assert all(k % 2 == 1 for k in g.conv_kernel_size), name
        assert (conv_tile_split(E), conv_tile_split(2 * E)) == want, name
    g = synth.GEOMETRIES["medium_e576"]
    assert g.E // g.encoder_head == 2 * ATT_NS_MAX
    g = synth.GEOMETRIES["medium_e720"]
    assert g.E <= LN_TAIL_MAX < g.vp_filter_size and g.num_mels > 256 and g.E % 32 == 16 and g.num_mels % 32 == 16
    assert synth.GEOMETRIES["medium_e1024"].E > LN_TAIL_MAX
    g = synth.GEOMETRIES["small_e304"]
    assert g.encoder_layer == 1 and g.conv_filter_size % 16 != 0 and g.conv_kernel_size == (1, 5)
    for name in synth.ENCDEC_GEOMETRIES:
        _, g, t = ckpt(name)
        assert t["_pe._enc.laystk.0.pos_ffn.w_1.w"].shape == (g.conv_filter_size, g.E, g.conv_kernel_size[0]), name
        assert t["_pe._enc.laystk.0.pos_ffn.w_2.w"].shape == (g.E, g.conv_filter_size, g.conv_kernel_size[1]), name
        assert t["_mel_decoder.to_out.0.w"].shape == (g.num_mels, g.E, 1) and t["_meldec.input_conv.w"].shape[1] == g.num_mels
        assert f"_pe._enc.laystk.{g.encoder_layer}.pos_ffn.w_1.w" not in t, name
    assert synth.GEOMETRIES["medium_m100"].num_mels % 16 and synth.GEOMETRIES["medium_ffn8"].conv_kernel_size[0] % 2 == 0
