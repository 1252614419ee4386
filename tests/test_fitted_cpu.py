"""CPU: the boundary of fitted synthesis (include/zerovox_amd.h zv_synthesize_fitted) — the three exported entry points and their
signatures, the Python binding's argument checks (they run before anything reaches a device), the CLI's flag, and the argument
the header's contract rests on: running the duration rule again with the capacity T' = n_frames gives the same durations."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
PAIRS = {"zv_synthesize_fitted": "zv_synthesize_phonemes", "zv_synthesize_batch_fitted": "zv_synthesize_batch_phonemes",
         "zv_synthesize_batch_begin_fitted": "zv_synthesize_batch_begin_phonemes"}


def _declaration(header, name):
    """the parameter types of `name`'s declaration in the header, comments and parameter names removed"""
    m = re.search(r"zv_status\s+%s\s*\((.*?)\)\s*;" % name, header, flags=re.S)
    assert m, name
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    return [re.sub(r"\s*\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace(" *", "*") for p in params]


def test_entry_points_are_declared_exported_and_bound_like_their_phonemes_forms():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zerovox_amd.h")).read(), flags=re.S)
    for name, twin in PAIRS.items():
        assert hasattr(lib, name) and name in capi.SYMBOLS, name
        # the full argument list of the _phonemes counterpart: in the header and in the binding
        assert _declaration(header, name) == _declaration(header, twin), name
        assert getattr(lib, name).argtypes == getattr(lib, twin).argtypes, name
        assert C.POINTER(capi.PhonemeControlsC) in getattr(lib, name).argtypes and C.POINTER(capi.Prosody) in getattr(lib, name).argtypes
    single = _declaration(header, "zv_synthesize_fitted")
    assert single == ["zv_model*", "const int32_t*", "const int32_t*", "const float*", "uint32_t", "uint32_t", "float*", "uint32_t*",
                      "const zv_prosody*", "const zv_phoneme_controls*", "int32_t*"], single
    begin = _declaration(header, "zv_synthesize_batch_begin_fitted")
    assert begin[:3] == ["zv_model*", "uint32_t", "uint32_t"] and begin[-1] == "int32_t*const*", begin
    # no _end of its own: the existing one finishes a fitted batch
    assert not re.search(r"\bzv_synthesize_batch_end_fitted\b", header)


def test_null_model_is_refused_by_every_entry_point():
    """ZV_ERR_ARG from the request check, before any device call (this machine has no GPU)"""
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    n = C.c_uint32(0)
    assert lib.zv_synthesize_fitted(None, None, None, None, 4, 8, None, C.byref(n), None, None, None) == 5
    assert b"zv_synthesize_fitted" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_fitted(None, 1, None, None, None, None, None, None, None, None, None, None) == 5
    assert b"zv_synthesize_batch_fitted" in lib.zv_last_error()
    assert lib.zv_synthesize_batch_begin_fitted(None, 0, 1, None, None, None, None, None, None, None, None, None, None) == 5
    assert b"zv_synthesize_batch_begin_fitted" in lib.zv_last_error()


class _NoDevice:
    """stands where a capi.Model would: any touch of the library or the handle fails the test"""
    hp = types.SimpleNamespace(audio_hop_size=300)

    def __getattr__(self, name):
        raise AssertionError(f"the binding touched .{name} before it had checked its arguments")


def test_binding_refuses_bad_arguments_before_touching_a_device():
    from zerovox_cpp_amd import capi
    ids, puncts, style = np.ones(4, np.int32), np.zeros(4, np.int32), np.zeros(528, np.float32)
    fake = _NoDevice()
    syn = capi.Model.synthesize
    for fitted in ("yes", 1, None, 0.0):
        with pytest.raises(TypeError, match="fitted must be a bool"):
            syn(fake, ids, puncts, style, 64, fitted=fitted)
        with pytest.raises(TypeError, match="fitted must be a bool"):
            capi.BatchCall(fake, [(ids, puncts, style, 64)], fitted=fitted)
    for T in (0, -3):
        with pytest.raises(ValueError, match="capacity must be > 0"):
            syn(fake, ids, puncts, style, T, fitted=True)
        with pytest.raises(ValueError, match="capacity must be > 0"):
            capi.BatchCall(fake, [(ids, puncts, style, 64), (ids, puncts, style, T)], fitted=True)
    for T in (12.0, "64", None, True):
        with pytest.raises(TypeError, match="integer frame capacity"):
            syn(fake, ids, puncts, style, T, fitted=True)
    # controls are converted (and their shapes checked) before the call as well
    with pytest.raises(ValueError, match="the utterance has 4 phonemes"):
        syn(_ChecksOnly(), ids, puncts, style, 64, fitted=True, phonemes=dict(duration_frames=[1, 2, 3]))
    # a well-formed fitted BatchCall is built without a device: capacity-shaped outputs, the flag kept for run() / begin()
    bc = capi.BatchCall(fake, [(ids, puncts, style, 64), (ids, puncts, style, np.int64(7))], durations=True, fitted=True)
    assert bc.fitted is True and [w.shape for w in bc.wavs] == [(64 * 300,), (7 * 300,)] and len(bc.durations) == 2
    assert capi.BatchCall(fake, [(ids, puncts, style, 64)]).fitted is False


class _ChecksOnly(_NoDevice):
    """lets synthesize() read the handle fields it needs to build its arguments; the library itself stays out of reach"""
    h = None

    @property
    def lib(self):
        raise AssertionError("the binding reached the library before it had checked the controls")


def test_call_variant_routes_fitted_calls_to_the_fitted_symbol():
    from zerovox_cpp_amd import capi
    seen = []
    lib = types.SimpleNamespace(**{name: (lambda *a, _n=name: seen.append((_n, a)) or 0)
                                   for name in ("zv_synthesize", "zv_synthesize_prosody", "zv_synthesize_phonemes", "zv_synthesize_fitted")})
    capi._call_variant(lib, "zv_synthesize", (1, 2), fitted=True)
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr", "pc", "dur", fitted=True)
    capi._call_variant(lib, "zv_synthesize", (1, 2), "pr")
    capi._call_variant(lib, "zv_synthesize", (1, 2))
    assert seen == [("zv_synthesize_fitted", (1, 2, None, None, None)), ("zv_synthesize_fitted", (1, 2, "pr", "pc", "dur")),
                    ("zv_synthesize_prosody", (1, 2, "pr")), ("zv_synthesize", (1, 2))]


def test_cli_knows_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--fit" in r.stdout and "--trim" in r.stdout
    r = subprocess.run([CLI, "--fit", "--no-such-flag"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--no-such-flag" in r.stderr


# ---- the duration rule under T' = n_frames (a copy of restate_durations / timings of tests/test_gpu_phoneme_controls.py) ---------

def _trunc_int(x64):
    return np.trunc(np.clip(x64, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def restate_durations(logdur, num_phonemes, T, uscale=1.0, frames=None, scale=None):
    dur = (np.exp(np.asarray(logdur, np.float32).astype(np.float64)) - 1.0).astype(np.float32)
    dur = (dur * np.float32(uscale)).astype(np.float32)
    if scale is not None:
        dur = (dur * np.asarray(scale, np.float32)).astype(np.float32)
    d = np.clip(_trunc_int(dur.astype(np.float64) + 0.5), 0, T)
    if frames is not None:
        fr = np.asarray(frames, np.int64)
        d = np.where(fr >= 0, np.minimum(fr, T), d)
    d[num_phonemes:] = 0
    return d


def timings(d, T):
    c = np.minimum(np.cumsum(d), T)
    return np.diff(np.concatenate([[0], c])).astype(np.int32)


def frame_owner(d, T):
    """the phoneme each of the T frames is gathered from (len(d) = none: a zero frame), the length regulator's search"""
    return np.searchsorted(np.cumsum(d), np.arange(T), side="right")


def test_capacity_n_frames_reproduces_the_durations():
    """With nf = min(sum d, T) under capacity T: the rule at T' = nf yields the same frame count, the same phoneme timings and the
    same owner for every frame below nf — so `the unfitted call at T = n_frames` is the same utterance.  Not cut off: every
    d_i <= sum d = nf, no clamp bites.  Cut off: nf = T, nothing changes."""
    rng = np.random.default_rng(20261016)
    cut = uncut = empty = forced_over = 0
    for case in range(4000):
        n = int(rng.integers(1, 70))
        walk = n if rng.random() < 0.7 else int(rng.integers(0, n + 1))
        logdur = rng.normal(rng.uniform(-0.5, 2.0), rng.uniform(0.1, 1.5), n).astype(np.float32)
        uscale = float(rng.choice([0.25, 0.5, 1.0, 2.0, 16.0]))
        scale = rng.uniform(0.1, 16.0, n).astype(np.float32) if rng.random() < 0.4 else None
        frames = None
        if rng.random() < 0.5:
            frames = np.where(rng.random(n) < 0.5, rng.integers(0, 60, n), -1).astype(np.int32)
        free = restate_durations(logdur, walk, 1 << 30, uscale, frames, scale)
        total = int(free.sum())
        T = int(rng.choice([1, 2, 7, 64, 65, max(1, total // 2), max(1, total - 1), max(1, total), total + 1, 2 * total + 7, 1500]))
        d = restate_durations(logdur, walk, T, uscale, frames, scale)
        nf = int(min(int(d.sum()), T))
        assert int(timings(d, T).sum()) == nf
        if nf == 0:
            empty += 1
            assert not timings(d, T).any()
            continue
        d2 = restate_durations(logdur, walk, nf, uscale, frames, scale)
        nf2 = int(min(int(d2.sum()), nf))
        assert nf2 == nf, (case, nf, nf2)
        assert np.array_equal(timings(d2, nf), timings(d, T)), case
        assert np.array_equal(frame_owner(d2, nf), frame_owner(d, T)[:nf]), case
        if int(d.sum()) >= T:
            cut += 1
            assert nf == T
        else:
            uncut += 1
            assert np.array_equal(d2, d) and int(d.max()) <= nf, case
        forced_over += frames is not None and bool((frames > T).any())
    assert cut > 300 and uncut > 300 and empty > 5 and forced_over > 50, (cut, uncut, empty, forced_over)
