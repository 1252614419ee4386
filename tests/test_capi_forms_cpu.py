"""The binding's table of entry-point forms and its per-option descriptors (zerovox.cpp_amd/capi.py), without a device and without
reading the table: every expectation here is written out, or comes from the if-chain the binding had before the table.
 * routing: over every subset of the twelve arguments _call_variant reaches the symbol, with the arguments, of that if-chain, for the
   single, batch and batch-begin entry points; likewise zv_encode_taps over its three rungs;
 * signatures: _bind gives every form the argtypes written out below;
 * an older library without the _bands and _filter symbols binds, runs a plain batch and fails a bands call with AttributeError;
 * a BatchCall settles its symbol and arguments once: run() and begin() pass the instance's own arrays, before and after every set_*;
 * the order in which BatchCall checks its arguments, and that synthesize checks a capacity before a table request sizes a buffer."""
import ctypes as C
import itertools
import types

import numpy as np
import pytest

KEYWORDS = ("prosody", "phonemes", "durations", "fitted", "target", "volume", "levels", "envelope", "contour", "pitch", "bands", "filter")
ENTRY_POINTS = ("zv_synthesize", "zv_synthesize_batch", "zv_synthesize_batch_begin")
IDS, PUNCTS, STYLE = np.ones(4, np.int32), np.zeros(4, np.int32), np.zeros(528, np.float32)


def _chain(lib, name, args, prosody=None, phonemes=None, durations=None, fitted=False, target=None, volume=None, levels=None,
           envelope=None, contour=None, pitch=None, bands=None, filter=None):
    """the dispatch as it was written before the table, verbatim"""
    if filter is not None:
        return getattr(lib, name + "_filter")(*args, prosody, phonemes, durations, target, int(fitted), volume, levels, envelope, contour,
                                              pitch, bands, filter)
    if bands is not None:
        return getattr(lib, name + "_bands")(*args, prosody, phonemes, durations, target, int(fitted), volume, levels, envelope, contour,
                                             pitch, bands)
    if pitch is not None:
        return getattr(lib, name + "_pitch")(*args, prosody, phonemes, durations, target, int(fitted), volume, levels, envelope, contour, pitch)
    if contour is not None:
        return getattr(lib, name + "_contour")(*args, prosody, phonemes, durations, target, int(fitted), volume, levels, envelope, contour)
    if envelope is not None:
        return getattr(lib, name + "_envelope")(*args, prosody, phonemes, durations, target, int(fitted), volume, levels, envelope)
    if volume is not None or levels is not None:
        return getattr(lib, name + "_volume")(*args, prosody, phonemes, durations, target, int(fitted), volume, levels)
    if target is not None:
        return getattr(lib, name + "_target")(*args, prosody, phonemes, durations, target, int(fitted))
    if fitted:
        return getattr(lib, name + "_fitted")(*args, prosody, phonemes, durations)
    if phonemes is not None or durations is not None:
        return getattr(lib, name + "_phonemes")(*args, prosody, phonemes, durations)
    if prosody is not None:
        return getattr(lib, name + "_prosody")(*args, prosody)
    return getattr(lib, name)(*args)


def _stub_lib(symbols):
    """an object with a recording function per symbol (a function takes attributes, as a CDLL's do); .calls is the record"""
    lib = types.SimpleNamespace(calls=[])
    for name in symbols:
        setattr(lib, name, lambda *a, _n=name: lib.calls.append((_n, a)) or 0)
    return lib


def _stub_model(lib):
    def chk(status):
        assert status == 0
    return types.SimpleNamespace(lib=lib, h="handle", hp=types.SimpleNamespace(audio_hop_size=300), _chk=chk)


def _same(got, want):
    """two recorded calls: the same symbol and, by identity and in order, the same arguments (numbers by value)"""
    return got[0] == want[0] and len(got[1]) == len(want[1]) and all(
        g is w or (isinstance(w, int) and type(g) is type(w) and g == w) for g, w in zip(got[1], want[1]))


def _typed(call):
    """a recorded call with the type of every argument beside it: True is not 1 here"""
    return call[0], [(type(a), a) for a in call[1]]


def test_call_variant_routes_every_subset_as_the_chain_did():
    from zerovox_cpp_amd import capi
    lib = _stub_lib(capi.SYMBOLS)
    n = 0
    for present in itertools.product((False, True), repeat=len(KEYWORDS)):
        kw = {k: True if k == "fitted" else "<%s>" % k for k, p in zip(KEYWORDS, present) if p}
        for target in (0, 7) if "target" in kw else (None,):
            if target is not None:
                kw["target"] = target
            for name in ENTRY_POINTS:
                del lib.calls[:]
                _chain(lib, name, ("a", "b"), **kw)
                capi._call_variant(lib, name, ("a", "b"), **kw)
                assert _typed(lib.calls[1]) == _typed(lib.calls[0]), (name, kw)
                n += 1
    assert n == 3 * (2048 + 2 * 2048)
    del lib.calls[:]
    every = ["<%s>" % k for k in KEYWORDS]
    every[3], every[4] = True, 7
    capi._call_variant(lib, "zv_synthesize_batch", ("a",), *every)                    # the positional order
    assert lib.calls == [("zv_synthesize_batch_filter", ("a", "<prosody>", "<phonemes>", "<durations>", 7, 1, "<volume>", "<levels>",
                                                         "<envelope>", "<contour>", "<pitch>", "<bands>", "<filter>"))]
    assert type(lib.calls[0][1][5]) is int                                            # fitted goes as int, not as the bool
    other = _stub_lib(["zv_other", "zv_other_target"])                                # a name outside the table takes the whole ladder
    capi._call_variant(other, "zv_other", ("a",), fitted=True, target=0)
    capi._call_variant(other, "zv_other", ("a",))
    assert [_typed(c) for c in other.calls] == [_typed(("zv_other_target", ("a", None, None, None, 0, 1))), _typed(("zv_other", ("a",)))]


def test_call_variant_routes_encode_taps_over_its_three_rungs():
    from zerovox_cpp_amd import capi
    lib = _stub_lib(capi.SYMBOLS)
    for present in itertools.product((False, True), repeat=3):
        kw = {k: "<%s>" % k for k, p in zip(KEYWORDS[:3], present) if p}
        for target in (None, 0, 7):
            del lib.calls[:]
            if target is None:
                _chain(lib, "zv_encode_taps", ("a", "b"), **kw)
                capi._call_variant(lib, "zv_encode_taps", ("a", "b"), **kw)
            else:       # encode() called the _target form itself: everything below it and the count, with no fitted flag
                lib.zv_encode_taps_target("a", "b", kw.get("prosody"), kw.get("phonemes"), kw.get("durations"), target)
                capi._call_variant(lib, "zv_encode_taps", ("a", "b"), target=target, **kw)
            assert _typed(lib.calls[1]) == _typed(lib.calls[0]), (kw, target)


def _signatures(capi):
    t = dict(vp=C.c_void_p, u32=C.c_uint32, int=C.c_int, pu32=C.POINTER(C.c_uint32), pvp=C.POINTER(C.c_void_p),
             PR=C.POINTER(capi.Prosody), PC=C.POINTER(capi.PhonemeControlsC), VOL=C.POINTER(capi.Volume), LEV=C.POINTER(capi.Level),
             ENV=C.POINTER(capi.EnvelopeC), CTR=C.POINTER(capi.ContourC), PIT=C.POINTER(capi.PitchC), BND=C.POINTER(capi.BandsC),
             FLT=C.POINTER(capi.FilterC))
    text = """
    zv_synthesize                      vp vp vp vp u32 u32 vp pu32
    zv_synthesize_prosody              vp vp vp vp u32 u32 vp pu32 PR
    zv_synthesize_phonemes             vp vp vp vp u32 u32 vp pu32 PR PC vp
    zv_synthesize_fitted               vp vp vp vp u32 u32 vp pu32 PR PC vp
    zv_synthesize_target               vp vp vp vp u32 u32 vp pu32 PR PC vp u32 int
    zv_synthesize_volume               vp vp vp vp u32 u32 vp pu32 PR PC vp u32 int VOL LEV
    zv_synthesize_envelope             vp vp vp vp u32 u32 vp pu32 PR PC vp u32 int VOL LEV ENV
    zv_synthesize_contour              vp vp vp vp u32 u32 vp pu32 PR PC vp u32 int VOL LEV ENV CTR
    zv_synthesize_pitch                vp vp vp vp u32 u32 vp pu32 PR PC vp u32 int VOL LEV ENV CTR PIT
    zv_synthesize_bands                vp vp vp vp u32 u32 vp pu32 PR PC vp u32 int VOL LEV ENV CTR PIT BND
    zv_synthesize_filter               vp vp vp vp u32 u32 vp pu32 PR PC vp u32 int VOL LEV ENV CTR PIT BND FLT
    zv_synthesize_batch                vp u32 pvp pvp pvp pu32 pu32 pvp pu32
    zv_synthesize_batch_prosody        vp u32 pvp pvp pvp pu32 pu32 pvp pu32 PR
    zv_synthesize_batch_phonemes       vp u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp
    zv_synthesize_batch_fitted         vp u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp
    zv_synthesize_batch_target         vp u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int
    zv_synthesize_batch_volume         vp u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV
    zv_synthesize_batch_envelope       vp u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV ENV
    zv_synthesize_batch_contour        vp u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV ENV CTR
    zv_synthesize_batch_pitch          vp u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV ENV CTR PIT
    zv_synthesize_batch_bands          vp u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV ENV CTR PIT BND
    zv_synthesize_batch_filter         vp u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV ENV CTR PIT BND FLT
    zv_synthesize_batch_begin          vp u32 u32 pvp pvp pvp pu32 pu32 pvp pu32
    zv_synthesize_batch_begin_prosody  vp u32 u32 pvp pvp pvp pu32 pu32 pvp pu32 PR
    zv_synthesize_batch_begin_phonemes vp u32 u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp
    zv_synthesize_batch_begin_fitted   vp u32 u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp
    zv_synthesize_batch_begin_target   vp u32 u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int
    zv_synthesize_batch_begin_volume   vp u32 u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV
    zv_synthesize_batch_begin_envelope vp u32 u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV ENV
    zv_synthesize_batch_begin_contour  vp u32 u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV ENV CTR
    zv_synthesize_batch_begin_pitch    vp u32 u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV ENV CTR PIT
    zv_synthesize_batch_begin_bands    vp u32 u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV ENV CTR PIT BND
    zv_synthesize_batch_begin_filter   vp u32 u32 pvp pvp pvp pu32 pu32 pvp pu32 PR PC pvp pu32 int VOL LEV ENV CTR PIT BND FLT
    zv_encode_taps                     vp vp vp vp u32 u32 u32 vp pu32 vp vp vp vp vp vp
    zv_encode_taps_prosody             vp vp vp vp u32 u32 u32 vp pu32 vp vp vp vp vp vp PR
    zv_encode_taps_phonemes            vp vp vp vp u32 u32 u32 vp pu32 vp vp vp vp vp vp PR PC vp
    zv_encode_taps_target              vp vp vp vp u32 u32 u32 vp pu32 vp vp vp vp vp vp PR PC vp u32
    zv_synthesize_batch_end            vp u32
    zv_pitch_track                     vp vp u32 PIT
    zv_band_levels                     vp vp u32 BND
    zv_filter_wave                     vp vp u32 FLT vp
    zv_filter_design                   u32 vp vp u32 vp
    """
    return {line.split()[0]: [t[w] for w in line.split()[1:]] for line in text.strip().splitlines()}


def test_bind_gives_every_form_the_argtypes_written_out_here():
    from zerovox_cpp_amd import capi
    lib = _stub_lib(capi.SYMBOLS)
    capi._bind(lib)
    want = _signatures(capi)
    forms = [s for s in capi.SYMBOLS if s.startswith(ENTRY_POINTS + ("zv_encode_taps",))]
    assert sorted(forms + ["zv_pitch_track", "zv_band_levels", "zv_filter_wave", "zv_filter_design"]) == sorted(want)
    for name, types_ in want.items():
        assert getattr(lib, name).argtypes == types_, name
    assert lib.zv_last_error.restype is C.c_char_p and lib.zv_max_frames.restype is C.c_uint32 and lib.zv_model_free.restype is None
    real = capi.load_library()                      # and the library itself went through the same step
    for name, types_ in want.items():
        assert getattr(real, name).argtypes == types_, name


def test_an_older_library_binds_and_fails_only_the_call_that_needs_a_missing_rung():
    from zerovox_cpp_amd import capi
    newer = ("zv_synthesize_bands", "zv_synthesize_batch_bands", "zv_synthesize_batch_begin_bands", "zv_band_levels",
             "zv_synthesize_filter", "zv_synthesize_batch_filter", "zv_synthesize_batch_begin_filter", "zv_filter_wave", "zv_filter_design")
    lib = _stub_lib([s for s in capi.SYMBOLS if s not in newer])
    capi._bind(lib)
    want = _signatures(capi)
    for name in want:
        if name not in newer:
            assert getattr(lib, name).argtypes == want[name], name
    model = _stub_model(lib)
    two = [(IDS, PUNCTS, STYLE, 8), (IDS, PUNCTS, STYLE, 5)]
    capi.BatchCall(model, two).run()
    capi.BatchCall(model, two, return_pitch=True).begin(1)
    assert [c[0] for c in lib.calls] == ["zv_synthesize_batch", "zv_synthesize_batch_begin_pitch"]
    bands = capi.BatchCall(model, two, return_bands=True)
    with pytest.raises(AttributeError, match="zv_synthesize_batch_bands"):
        bands.run()
    with pytest.raises(AttributeError, match="zv_synthesize_batch_begin_bands"):
        bands.begin(0)
    with pytest.raises(AttributeError, match="zv_synthesize_filter"):
        capi.Model.synthesize(model, IDS, PUNCTS, STYLE, 8, filter=[1.0])
    assert len(lib.calls) == 2


def _batch_cases(capi):
    """(BatchCall arguments, the suffix its calls must carry, the setters to try): each option alone, and all together"""
    base = (IDS, PUNCTS, STYLE)
    plain = [base + (8,), base + (5,)]
    env = capi.Envelope([1.0, 0.5, 0.25, 2.0], ramp_frames=2)
    setters = dict(prosody=("set_prosody", (1.25, 1.0, 0.0, 1.0, 0.0)), phonemes=("set_phoneme_controls", dict(pitch_shift=[0.5] * 4)),
                   target=("set_target_frames", 3), volume=("set_volume", (0.5, 0.0, 0.0)), envelope=("set_envelope", env),
                   pitch=("set_pitch", "frames"), bands=("set_bands", capi.BandLevels(4)), filter=("set_filter", [0.25, 0.5, 0.25]))
    full = [base + (8, capi.Prosody(1.5), dict(duration_scale=[2.0] * 4), 6), base + (5, None, None, None)]
    every = dict(durations=True, fitted=True, volume=[None, (2.0, 0.0, 0.5)], return_levels=True, envelope=[env, None],
                 return_contour="frames", return_pitch=[True, False], return_bands=capi.BandLevels(8), filter=[None, [1.0]])
    return [
        ("plain", plain, {}, "", ()),
        ("prosody", [base + (8, capi.Prosody(1.5)), plain[1]], {}, "_prosody", ("prosody",)),
        ("phonemes", [base + (8, None, dict(duration_scale=[2.0] * 4)), plain[1]], {}, "_phonemes", ("phonemes",)),
        ("durations", plain, dict(durations=True), "_phonemes", ("phonemes",)),
        ("fitted", plain, dict(fitted=True), "_fitted", ()),
        ("target", [base + (8, None, None, 6), plain[1]], {}, "_target", ("target",)),
        ("volume", plain, dict(volume=[None, (2.0, 0.0, 0.5)]), "_volume", ("volume",)),
        ("levels", plain, dict(return_levels=True), "_volume", ()),
        ("envelope", plain, dict(envelope=[env, None]), "_envelope", ("envelope",)),
        ("contour", plain, dict(return_contour="frames"), "_contour", ()),
        ("pitch", plain, dict(return_pitch=[True, False]), "_pitch", ("pitch",)),
        ("bands", plain, dict(return_bands=capi.BandLevels(8)), "_bands", ("bands",)),
        ("filter", plain, dict(filter=[None, [1.0]]), "_filter", ("filter",)),
        ("everything", full, every, "_filter", tuple(setters)),
    ], setters


def test_a_batch_call_settles_its_symbol_and_arguments_once():
    from zerovox_cpp_amd import capi
    lib = _stub_lib(capi.SYMBOLS)
    model = _stub_model(lib)
    cases, setters = _batch_cases(capi)
    for label, utts, kw, suffix, to_set in cases:
        bc = capi.BatchCall(model, utts, **kw)

        def expect(name, lead):
            """what the chain passes for the instance's arrays as they are now"""
            rec = _stub_lib(capi.SYMBOLS)
            _chain(rec, name, lead + (bc.ids_p, bc.pun_p, bc.sty_p, bc.Ns, bc.Ts, bc.wav_p, bc.nf), bc.prosody, bc.phonemes, bc.dur_p,
                   bc.fitted, bc.targets, bc.volume, bc.levels, bc.envelope, bc.contour, bc.pitch, bc.band, bc.filter)
            assert rec.calls[0][0] == name + suffix, (label, rec.calls[0][0])
            return rec.calls[0]

        arrays = expect("zv_synthesize_batch", ("handle", 2))[1]
        for method, value in [(None, None)] + [setters[k] for k in to_set]:
            if method:
                getattr(bc, method)(1, value)
                getattr(bc, method)(0, None)
            del lib.calls[:]
            bc.run()
            bc.begin(3)
            assert len(lib.calls) == 2, label
            assert _same(lib.calls[0], expect("zv_synthesize_batch", ("handle", 2))), (label, method, lib.calls[0][0])
            assert _same(lib.calls[1], expect("zv_synthesize_batch_begin", ("handle", 3, 2))), (label, method, lib.calls[1][0])
            assert _same(lib.calls[0], ("zv_synthesize_batch" + suffix, arrays)), (label, method)      # the objects it was built with
    bc = capi.BatchCall(model, cases[-1][1], **cases[-1][2])
    assert None not in (bc.prosody, bc.phonemes, bc.dur_p, bc.targets, bc.volume, bc.levels, bc.envelope, bc.contour, bc.pitch, bc.band, bc.filter)
    bc.set_target_frames(0, 4)
    bc.set_pitch(1, capi.PitchTrack(min_lag=20))
    assert (bc.targets[0], bc.pitch[1].min_lag, bc.pitches[1].params.min_lag, bc.pitch[0].frames) == (4, 20, 20, bc.pitches[0].frames.ctypes.data)


BAD = [      # in the order BatchCall checks: (label, utterance tail, keywords, exception, message)
    ("fitted", (), dict(fitted="yes"), TypeError, "fitted must be a bool"),
    ("filter", (), dict(filter=[None, "taps"]), TypeError, "utterance 1: filter must be a Filter"),
    ("bands", (), dict(return_bands="both"), ValueError, "return_bands = 'both'"),
    ("pitch", (), dict(return_pitch=[True, 3]), TypeError, "utterance 1: return_pitch must be a bool"),
    ("contour", (), dict(return_contour="both"), ValueError, "return_contour = 'both'"),
    ("envelope", (), dict(envelope=[dict(bogus=1), None]), ValueError, "utterance 0: unknown envelope field"),
    ("levels", (), dict(return_levels="yes"), TypeError, "return_levels must be a bool"),
    ("volume", (), dict(volume=[None, (1.0, 2.0)]), ValueError, "utterance 1: a volume is"),
    ("targets", (None, None, -1), {}, ValueError, "target_frames = -1"),
    ("prosody", (dict(bogus=1),), {}, TypeError, "bogus"),
    ("phoneme controls", (None, dict(bogus=[0.0] * 4)), {}, ValueError, "unknown phoneme control"),
]


def _bad_call(capi, model, *entries, T=8):
    tail, kw = [None, None, None], {}
    for _, t, k, _, _ in entries:
        for i, v in enumerate(t):
            tail[i] = v if v is not None else tail[i]
        kw.update(k)
    return lambda: capi.BatchCall(model, [(IDS, PUNCTS, STYLE, 5), (IDS, PUNCTS, STYLE, T) + tuple(tail)], **kw)


def test_batch_call_checks_its_arguments_in_the_order_it_always_did():
    from zerovox_cpp_amd import capi
    model = _stub_model(_stub_lib(capi.SYMBOLS))
    for entry in BAD:                                    # each alone raises its own message
        with pytest.raises(entry[3], match=entry[4]):
            _bad_call(capi, model, entry)()
    for first, second in zip(BAD, BAD[1:]):              # of two bad arguments the earlier one is reported
        with pytest.raises(first[3], match=first[4]):
            _bad_call(capi, model, first, second)()
    with pytest.raises(ValueError, match="T = 0: the frame capacity must be > 0"):      # the capacities go with fitted
        _bad_call(capi, model, BAD[1], T=0)()
    with pytest.raises(ValueError, match="filter has 1 entries, the batch has 2 utterances"):
        capi.BatchCall(model, [(IDS, PUNCTS, STYLE, 5)] * 2, filter=[None], return_bands="both")
    assert model.lib.calls == []


def test_synthesize_checks_the_capacity_before_it_sizes_a_table():
    from zerovox_cpp_amd import capi
    model = _stub_model(_stub_lib(capi.SYMBOLS))
    tables = [dict(return_contour=True), dict(return_pitch="frames"), dict(return_bands=True),
              dict(return_contour="phonemes", return_pitch=capi.PitchTrack(20), return_bands=capi.BandLevels(4)), {}]
    for kw in tables:
        for T, exc, msg in ((-1, ValueError, "T = -1: the frame capacity must be > 0"), (0, ValueError, "T = 0: the frame capacity must be > 0"),
                            ("8", TypeError, "T must be an integer frame capacity, not str"), (2.5, TypeError, "T must be an integer frame capacity, not float"),
                            (None, TypeError, "T must be an integer frame capacity, not NoneType"), (True, TypeError, "T must be an integer frame capacity, not bool")):
            with pytest.raises(exc, match=msg):
                capi.Model.synthesize(model, IDS, PUNCTS, STYLE, T, **kw)
        with pytest.raises(TypeError, match="fitted must be a bool"):          # and the flag, ahead of the capacity
            capi.Model.synthesize(model, IDS, PUNCTS, STYLE, -1, fitted="yes", **kw)
        with pytest.raises(ValueError, match="target_frames = 9 exceeds the frame capacity T = 8"):
            capi.Model.synthesize(model, IDS, PUNCTS, STYLE, 8, target_frames=9, volume=(1.0, 2.0), **kw)
    with pytest.raises(ValueError, match="return_contour = 'both'"):           # a bad wish is still reported ahead of a bad capacity
        capi.Model.synthesize(model, IDS, PUNCTS, STYLE, -1, return_contour="both", return_pitch=3)
    with pytest.raises(TypeError, match="filter must be a Filter"):            # and the filter ahead of everything, ids included
        capi.Model.synthesize(model, 5, PUNCTS, STYLE, -1, filter="taps", return_contour="both")
    assert model.lib.calls == []
    out = capi.Model.synthesize(model, IDS, PUNCTS, STYLE, 8, return_contour=True, return_pitch="frames", return_bands=True)
    assert [type(x).__name__ for x in out] == ["ndarray", "int", "Contour", "Pitch", "Bands"] and out[2].frames.shape == (8, 2)
    assert out[3].phonemes is None and out[4].phonemes.shape == (4, 16) and [c[0] for c in model.lib.calls] == ["zv_synthesize_bands"]
