"""CPU: the binding of the stage-batch entry points (zerovox.cpp_amd/capi.py: zv_encode_batch, zv_decode_batch, zv_vocode_batch,
zv_vocode_batch_begin, zv_vocode_batch_end), without a device.
 * signatures: _bind gives the five symbols the argtypes written out below, on a stub and on the library itself, and the header
   declares them with those parameters;
 * a stub library records that encode_batch / decode_batch / vocode_batch / vocode_batch_begin pass their arrays in the header's order;
 * an older library without the five symbols binds, runs what it has, and fails only these calls, with AttributeError naming the symbol."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zv_encode_batch", "zv_decode_batch", "zv_vocode_batch", "zv_vocode_batch_begin", "zv_vocode_batch_end")
E, MELS, HOP = 12, 5, 4


def _stub_lib(symbols):
    lib = types.SimpleNamespace(calls=[])
    for name in symbols:
        setattr(lib, name, lambda *a, _n=name: lib.calls.append((_n, a)) or 0)
    return lib


def _stub_model(capi, lib):
    def chk(status):
        assert status == 0
    return types.SimpleNamespace(lib=lib, h="handle", E=E, hp=types.SimpleNamespace(audio_hop_size=HOP, audio_num_mels=MELS), _chk=chk)


def _signatures(capi):
    vp, u32 = C.c_void_p, C.c_uint32
    pvp, pu32 = C.POINTER(vp), C.POINTER(u32)
    return {
        "zv_encode_batch": [vp, u32, pvp, pvp, pvp, pu32, pu32, pvp, pu32, C.POINTER(capi.Prosody), C.POINTER(capi.PhonemeControlsC), pvp, pu32],
        "zv_decode_batch": [vp, u32, pvp, pvp, pu32, pvp],
        "zv_vocode_batch": [vp, u32, pvp, pu32, pvp],
        "zv_vocode_batch_begin": [vp, u32, u32, pvp, pu32, pvp],
        "zv_vocode_batch_end": [vp, u32],
    }


def test_bind_gives_the_five_symbols_the_argtypes_written_out_here():
    from zerovox_cpp_amd import capi
    assert set(NEW) <= set(capi.SYMBOLS)
    assert not [s for s in NEW if s.startswith(("zv_synthesize", "zv_encode_taps"))]      # outside the frozen ladders
    want = _signatures(capi)
    for lib in (_stub_lib(capi.SYMBOLS), capi.load_library()):
        if not hasattr(lib, "_handle"):
            capi._bind(lib)
        for name, types_ in want.items():
            assert getattr(lib, name).argtypes == types_, name


def test_the_header_declares_them_with_these_parameters():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zerovox_amd.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", header)
    for decl in (
        "zv_status zv_encode_batch(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts, "
        "const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *hidden, uint32_t *n_frames, "
        "const zv_prosody *prosody, const zv_phoneme_controls *phonemes, int32_t *const *durations, const uint32_t *target_frames);",
        "zv_status zv_decode_batch(zv_model *m, uint32_t n_utt, const float *const *hidden, const float *const *styles, const uint32_t *T, "
        "float *const *mel);",
        "zv_status zv_vocode_batch(zv_model *m, uint32_t n_utt, const float *const *mel, const uint32_t *T, float *const *wav);",
        "zv_status zv_vocode_batch_begin(zv_model *m, uint32_t lane, uint32_t n_utt, const float *const *mel, const uint32_t *T, "
        "float *const *wav);",
        "zv_status zv_vocode_batch_end(zv_model *m, uint32_t lane);",
    ):
        assert decl in flat, decl
    facade = re.sub(r"\s+", " ", open(os.path.join(ROOT, "zerovox.cpp_amd", "csrc", "zerovox.h")).read())
    assert "void eval_batch(uint32_t n, const float *const *mels, const uint32_t *T, float *const *wavs);" in facade


def _utts():
    ids = [np.arange(1, 4, dtype=np.int32), np.arange(1, 6, dtype=np.int32)]
    return [(ids[0], np.zeros(3, np.int32), np.full(E, 0.5, np.float32), 7),
            (ids[1], np.ones(5, np.int32), np.zeros(E, np.float32), 9, (1.5, 1.0, 0.0, 1.0, 0.0), dict(duration_frames=[2] * 5), 8)]


def _addresses(ptr_array):
    return [int(p) if p else 0 for p in ptr_array]


def test_the_calls_pass_their_arrays_in_the_headers_order():
    from zerovox_cpp_amd import capi
    lib = _stub_lib(capi.SYMBOLS)
    model = _stub_model(capi, lib)
    # ---- encode_batch: (m, n_utt, ids, puncts, styles, n_phonemes, T, hidden, n_frames, prosody, phonemes, durations, target_frames)
    utts = _utts()
    out = capi.Model.encode_batch(model, utts, return_durations=True)
    name, a = lib.calls[-1]
    assert name == "zv_encode_batch" and len(a) == 13 and a[0] == "handle" and a[1] == 2
    for k, col in ((2, 0), (3, 1), (4, 2)):                         # the pointer arrays name the utterances' own (already typed) arrays
        assert _addresses(a[k]) == [u[col].ctypes.data for u in utts], k
    assert list(a[5]) == [3, 5] and list(a[6]) == [7, 9]
    assert _addresses(a[7]) == [o["hidden"].ctypes.data for o in out] and [o["hidden"].shape for o in out] == [(7, E), (9, E)]
    assert len(a[8]) == 2 and [o["n_frames"] for o in out] == [0, 0]
    assert isinstance(a[9][0], capi.Prosody) and (a[9][1].duration_scale, a[9][0].duration_scale) == (1.5, 1.0)
    assert isinstance(a[10][0], capi.PhonemeControlsC) and bool(a[10][1].duration_frames) and not a[10][0].duration_frames
    assert _addresses(a[11]) == [o["durations"].ctypes.data for o in out] and [o["durations"].shape for o in out] == [(3,), (5,)]
    assert list(a[12]) == [0, 8]
    # the planning call: no hidden, and without options every optional array is NULL
    out = capi.Model.encode_batch(model, [u[:4] for u in utts], return_hidden=False)
    name, a = lib.calls[-1]
    assert name == "zv_encode_batch" and a[7] is None and a[9:] == (None, None, None, None) and all(set(o) == {"n_frames"} for o in out)
    # ---- decode_batch: (m, n_utt, hidden, styles, T, mel)
    hid = [np.zeros((4, E), np.float32), np.ones((6, E), np.float32)]
    sty = [np.zeros(E, np.float32), np.ones(E, np.float32)]
    mels = capi.Model.decode_batch(model, hid, sty)
    name, a = lib.calls[-1]
    assert name == "zv_decode_batch" and len(a) == 6 and a[:2] == ("handle", 2)
    assert _addresses(a[2]) == [h.ctypes.data for h in hid] and _addresses(a[3]) == [s.ctypes.data for s in sty]
    assert list(a[4]) == [4, 6] and _addresses(a[5]) == [m.ctypes.data for m in mels] and [m.shape for m in mels] == [(4, MELS), (6, MELS)]
    with pytest.raises(ValueError, match="2 hiddens, 1 styles"):
        capi.Model.decode_batch(model, hid, sty[:1])
    # ---- vocode_batch: (m, n_utt, mel, T, wav); _begin: (m, lane, n_utt, mel, T, wav); _end: (m, lane)
    mel = [np.zeros((3, MELS), np.float32), np.ones((1, MELS), np.float32)]
    wavs = capi.Model.vocode_batch(model, mel)
    name, a = lib.calls[-1]
    assert name == "zv_vocode_batch" and len(a) == 5 and a[:2] == ("handle", 2)
    assert _addresses(a[2]) == [m.ctypes.data for m in mel] and list(a[3]) == [3, 1]
    assert _addresses(a[4]) == [w.ctypes.data for w in wavs] and [w.shape for w in wavs] == [(3 * HOP,), (1 * HOP,)]
    capi.Model.vocode_batch_begin(model, 2, mel)
    name, a = lib.calls[-1]
    assert name == "zv_vocode_batch_begin" and len(a) == 6 and a[:3] == ("handle", 2, 2)
    assert _addresses(a[3]) == [m.ctypes.data for m in mel] and list(a[4]) == [3, 1]
    got = capi.Model.vocode_batch_end(model, 2)
    assert lib.calls[-1] == ("zv_vocode_batch_end", ("handle", 2))
    assert _addresses(a[5]) == [w.ctypes.data for w in got] and [w.shape for w in got] == [(3 * HOP,), (1 * HOP,)]
    assert capi.Model.vocode_batch_end(model, 1) is None            # (the stub accepts it; the library refuses an idle lane)


def test_an_older_library_binds_and_fails_only_these_calls():
    from zerovox_cpp_amd import capi
    lib = _stub_lib([s for s in capi.SYMBOLS if s not in NEW])
    capi._bind(lib)                                                  # binds what it has
    assert lib.zv_synthesize_batch.argtypes and lib.zv_vocode.argtypes
    model = _stub_model(capi, lib)
    capi.BatchCall(model, [u[:4] for u in _utts()]).run()
    assert [c[0] for c in lib.calls] == ["zv_synthesize_batch"]
    mel = [np.zeros((3, MELS), np.float32)]
    for name, call in (("zv_encode_batch", lambda: capi.Model.encode_batch(model, _utts())),
                       ("zv_decode_batch", lambda: capi.Model.decode_batch(model, [np.zeros((4, E), np.float32)], [np.zeros(E, np.float32)])),
                       ("zv_vocode_batch", lambda: capi.Model.vocode_batch(model, mel)),
                       ("zv_vocode_batch_begin", lambda: capi.Model.vocode_batch_begin(model, 0, mel)),
                       ("zv_vocode_batch_end", lambda: capi.Model.vocode_batch_end(model, 0))):
        with pytest.raises(AttributeError, match=name + r"\b"):
            call()
    assert len(lib.calls) == 1


def test_the_cli_knows_plan_and_fails_without_a_model(tmp_path):
    import subprocess
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--plan" in r.stdout and "index n_phonemes n_frames seconds" in r.stdout
    r = subprocess.run([cli, "-m", str(tmp_path / "missing.gguf"), "--plan"], capture_output=True, text=True)      # no model: an error, no rows
    assert r.returncode == 1 and r.stderr.startswith("zerovox: ") and r.stdout == ""
