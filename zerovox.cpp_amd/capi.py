"""ctypes binding of libzerovox_amd.so (the C-ABI of include/zerovox_amd.h).

Used by the parity tests, bench.py and smoke(): the same entry points a C/C++ host would call.
There is NO CPU fallback: if the library is missing or no gfx950 device is present, loading fails.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZEROVOX_AMD_LIB") or os.path.join(HERE, "libzerovox_amd.so")   # env override: A/B builds

# every symbol include/zerovox_amd.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "zv_last_error", "zv_version", "zv_model_load", "zv_model_free", "zv_model_get_hparams", "zv_model_reserve",
    "zv_encode", "zv_encode_taps", "zv_decode", "zv_vocode", "zv_synthesize", "zv_synthesize_batch", "zv_synthesize_batch_begin", "zv_synthesize_batch_end", "zv_device_alloc", "zv_device_free",
    "zv_memcpy_h2d", "zv_memcpy_d2h", "zv_vocode_device", "zv_vocode_stream", "zv_vocoder_halo_frames", "zv_decode_device", "zv_synchronize", "zv_set_graph_mode",
    "zv_profile_begin", "zv_profile_end", "zv_write_wav", "zv_gguf_inspect", "zv_max_frames", "zv_demo_utterance", "zv_debug_layer", "zv_debug_set",
    "zv_debug_get", "zv_batch_timeline", "zv_encode_taps_prosody", "zv_synthesize_prosody", "zv_synthesize_batch_prosody",
    "zv_synthesize_batch_begin_prosody", "zv_encode_taps_phonemes", "zv_synthesize_phonemes", "zv_synthesize_batch_phonemes",
    "zv_synthesize_batch_begin_phonemes", "zv_synthesize_fitted", "zv_synthesize_batch_fitted", "zv_synthesize_batch_begin_fitted",
    "zv_debug_voc_runs", "zv_debug_poison", "zv_encode_taps_target", "zv_synthesize_target", "zv_synthesize_batch_target",
    "zv_synthesize_batch_begin_target", "zv_synthesize_volume", "zv_synthesize_batch_volume", "zv_synthesize_batch_begin_volume",
    "zv_debug_mfma_chain", "zv_synthesize_envelope", "zv_synthesize_batch_envelope", "zv_synthesize_batch_begin_envelope",
    "zv_synthesize_contour", "zv_synthesize_batch_contour", "zv_synthesize_batch_begin_contour",
    "zv_synthesize_pitch", "zv_synthesize_batch_pitch", "zv_synthesize_batch_begin_pitch", "zv_pitch_track",
    "zv_synthesize_bands", "zv_synthesize_batch_bands", "zv_synthesize_batch_begin_bands", "zv_band_levels",
    "zv_synthesize_filter", "zv_synthesize_batch_filter", "zv_synthesize_batch_begin_filter", "zv_filter_wave", "zv_filter_design",
]


WAV_SINK = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_float), C.c_uint64, C.c_uint64)
BATCH_LANES = 4      # ZV_BATCH_LANES of include/zerovox_amd.h


class HParams(C.Structure):
    _fields_ = [("max_seq_len", C.c_uint32), ("emb_dim", C.c_uint32), ("punct_emb_dim", C.c_uint32),
                ("decoder_n_head", C.c_uint32), ("conv_filter_size", C.c_uint32), ("conv_kernel_size", C.c_uint32 * 2),
                ("encoder_layer", C.c_uint32), ("encoder_head", C.c_uint32), ("encoder_vp_filter_size", C.c_uint32),
                ("encoder_vp_kernel_size", C.c_uint32), ("encoder_ve_n_bins", C.c_uint32),
                ("audio_sampling_rate", C.c_uint32), ("audio_num_mels", C.c_uint32), ("audio_hop_size", C.c_uint32),
                ("voc_channels", C.c_uint32), ("voc_num_upsamples", C.c_uint32), ("voc_upsample_scales", C.c_uint32 * 8),
                ("voc_num_resblocks", C.c_uint32), ("voc_resblock_kernels", C.c_uint32 * 8)]


class Prosody(C.Structure):
    """zv_prosody of include/zerovox_amd.h: per-utterance speaking rate, pitch and energy controls (identity: the defaults)"""
    _fields_ = [("duration_scale", C.c_float), ("pitch_scale", C.c_float), ("pitch_shift", C.c_float),
                ("energy_scale", C.c_float), ("energy_shift", C.c_float)]

    def __init__(self, duration_scale=1.0, pitch_scale=1.0, pitch_shift=0.0, energy_scale=1.0, energy_shift=0.0):
        super().__init__(duration_scale, pitch_scale, pitch_shift, energy_scale, energy_shift)

    def __repr__(self):
        return (f"Prosody(duration_scale={self.duration_scale}, pitch_scale={self.pitch_scale}, pitch_shift={self.pitch_shift}, "
                f"energy_scale={self.energy_scale}, energy_shift={self.energy_shift})")


def _prosody(p) -> Optional[Prosody]:
    """None, a Prosody, a dict of its fields or a 5-sequence -> Prosody / None"""
    if p is None or isinstance(p, Prosody):
        return p
    if isinstance(p, dict):
        return Prosody(**p)
    return Prosody(*p)


class Volume(C.Structure):
    """zv_volume of include/zerovox_amd.h: per-utterance linear gain, loudness (RMS) target and peak ceiling; 0 = no target / no
    ceiling, the defaults are the identity.  from_db() converts from dB / dBFS."""
    _fields_ = [("gain", C.c_float), ("target_rms", C.c_float), ("peak_ceiling", C.c_float)]

    def __init__(self, gain=1.0, target_rms=0.0, peak_ceiling=0.0):
        super().__init__(gain, target_rms, peak_ceiling)

    @classmethod
    def from_db(cls, gain_db=0, target_dbfs=None, peak_dbfs=None):
        """gain_db: the gain in dB; target_dbfs: the RMS level the speech is brought to, in dB re full scale (None: none);
        peak_dbfs: the peak ceiling likewise (None: none).  linear = 10 ** (dB / 20)"""
        lin = lambda db: 10.0 ** (float(db) / 20.0)
        return cls(lin(gain_db), 0.0 if target_dbfs is None else lin(target_dbfs), 0.0 if peak_dbfs is None else lin(peak_dbfs))

    def __repr__(self):
        return f"Volume(gain={self.gain}, target_rms={self.target_rms}, peak_ceiling={self.peak_ceiling})"


class Level(C.Structure):
    """zv_level of include/zerovox_amd.h: the speech's rms and peak before the gain, and the gain every sample was multiplied by"""
    _fields_ = [("rms", C.c_float), ("peak", C.c_float), ("gain", C.c_float), ("reserved", C.c_uint32)]

    def __repr__(self):
        return f"Level(rms={self.rms}, peak={self.peak}, gain={self.gain})"


VOLUME_LIMITS = (("gain", 1000.0), ("target_rms", 1.0), ("peak_ceiling", 1.0))


def _volume(v, where: str = "") -> Optional[Volume]:
    """None, a Volume, a dict of its fields or a 3-sequence -> Volume / None, checked before anything reaches the library: every
    field a finite number, gain in [0, 1000], target_rms and peak_ceiling in [0, 1]"""
    if v is None:
        return None
    if isinstance(v, Volume):
        vals = (v.gain, v.target_rms, v.peak_ceiling)
    elif isinstance(v, dict):
        unknown = sorted(set(v) - {n for n, _ in VOLUME_LIMITS})
        if unknown:
            raise ValueError(f"{where}unknown volume field(s) {unknown}")
        vals = (v.get("gain", 1.0), v.get("target_rms", 0.0), v.get("peak_ceiling", 0.0))
    else:
        vals = tuple(v)
        if len(vals) != 3:
            raise ValueError(f"{where}a volume is (gain, target_rms, peak_ceiling), got {len(vals)} values")
    out = []
    for (name, hi), x in zip(VOLUME_LIMITS, vals):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise TypeError(f"{where}volume {name} must be a number, not {type(x).__name__}")
        x = float(np.float32(x))
        if not np.isfinite(x):
            raise ValueError(f"{where}volume {name} = {x} is not finite")
        if not 0.0 <= x <= hi:
            raise ValueError(f"{where}volume {name} = {x} is outside [0, {hi:g}]")
        out.append(x)
    return Volume(*out)


def _check_levels(return_levels):
    if not isinstance(return_levels, (bool, np.bool_)):
        raise TypeError(f"return_levels must be a bool, not {type(return_levels).__name__}")
    return bool(return_levels)


class ContourC(C.Structure):
    """zv_contour of include/zerovox_amd.h: the two tables' pointers, zv_frame_level [T] and [n], each or NULL (a zeroed struct asks
    for nothing)"""
    _fields_ = [("frames", C.c_void_p), ("phonemes", C.c_void_p)]


class Contour:
    """An utterance's level contour (include/zerovox_amd.h "level contour"): .frames float32 [T, 2] and .phonemes float32 [n, 2],
    columns (rms, peak) of the waveform the same call returned; None for a table that was not asked for.  dbfs() converts a
    column or a table to dB re full scale (0 -> -inf).  .struct is the zv_contour, which points into the arrays (kept alive here)."""
    CHOICES = (False, True, "frames", "phonemes")

    def __init__(self, T: int, n: int, frames: bool = True, phonemes: bool = True):
        self.frames = np.zeros((T, 2), np.float32) if frames else None
        self.phonemes = np.zeros((n, 2), np.float32) if phonemes else None

    @property
    def struct(self) -> ContourC:
        return ContourC(None if self.frames is None else self.frames.ctypes.data,
                        None if self.phonemes is None else self.phonemes.ctypes.data)

    @staticmethod
    def dbfs(levels) -> np.ndarray:
        """20 * log10(level), full scale = 1.0; -inf for a level of 0"""
        a = np.asarray(levels, dtype=np.float64)
        with np.errstate(divide="ignore"):
            return 20.0 * np.log10(a)

    def __repr__(self):
        shape = lambda a: None if a is None else a.shape
        return f"Contour(frames={shape(self.frames)}, phonemes={shape(self.phonemes)})"


def _check_contour(return_contour, where: str = ""):
    """return_contour -> (frames asked for, phonemes asked for), checked before anything reaches the library: False, True (both
    tables), "frames" or "phonemes" """
    if isinstance(return_contour, (bool, np.bool_)):
        return bool(return_contour), bool(return_contour)
    if isinstance(return_contour, str):
        if return_contour in ("frames", "phonemes"):
            return return_contour == "frames", return_contour == "phonemes"
        raise ValueError(f"{where}return_contour = {return_contour!r}: expected False, True, 'frames' or 'phonemes'")
    raise TypeError(f"{where}return_contour must be a bool, 'frames' or 'phonemes', not {type(return_contour).__name__}")


class PitchC(C.Structure):
    """zv_pitch of include/zerovox_amd.h: the two tables' pointers, zv_pitch_frame [T] and zv_pitch_phoneme [n], each or NULL, and the
    parameters, 0 = default (a zeroed struct asks for nothing)"""
    _fields_ = [("frames", C.c_void_p), ("phonemes", C.c_void_p), ("min_lag", C.c_uint32), ("max_lag", C.c_uint32),
                ("window", C.c_uint32), ("voiced_threshold", C.c_float)]


class PitchTrack:
    """What a pitch track is asked for (include/zerovox_amd.h "pitch track"): the lags in samples, the window, the voicing threshold
    (each 0: the default) and which tables.  from_hz converts a frequency range at a sampling rate to lags as the CLI does."""

    def __init__(self, min_lag: int = 0, max_lag: int = 0, window: int = 0, voiced_threshold: float = 0.0, frames: bool = True,
                 phonemes: bool = True):
        for name, v in (("min_lag", min_lag), ("max_lag", max_lag), ("window", window)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"PitchTrack {name} must be an integer, not {type(v).__name__}")
            if not 0 <= v <= 0xffffffff:
                raise ValueError(f"PitchTrack {name} = {v} is outside [0, 4294967295]")
        if isinstance(voiced_threshold, (bool, np.bool_)) or not isinstance(voiced_threshold, (int, float, np.integer, np.floating)):
            raise TypeError(f"PitchTrack voiced_threshold must be a number, not {type(voiced_threshold).__name__}")
        if not (isinstance(frames, (bool, np.bool_)) and isinstance(phonemes, (bool, np.bool_))):
            raise TypeError("PitchTrack frames and phonemes must be bools")
        self.min_lag, self.max_lag, self.window = int(min_lag), int(max_lag), int(window)
        self.voiced_threshold = float(voiced_threshold)
        self.frames, self.phonemes = bool(frames), bool(phonemes)

    @classmethod
    def from_hz(cls, sampling_rate: int, min_hz: float = 0.0, max_hz: float = 0.0, **kw):
        """min_lag = sr / max_hz, max_lag = sr / min_hz, truncated; a frequency at 0 leaves its lag at the default"""
        return cls(min_lag=int(sampling_rate / max_hz) if max_hz else 0, max_lag=int(sampling_rate / min_hz) if min_hz else 0, **kw)

    def __repr__(self):
        return (f"PitchTrack(min_lag={self.min_lag}, max_lag={self.max_lag}, window={self.window}, "
                f"voiced_threshold={self.voiced_threshold}, frames={self.frames}, phonemes={self.phonemes})")


class Pitch:
    """An utterance's pitch track: .frames float32 [T, 2], columns (f0_hz, strength), and .phonemes float32 [n, 2], columns (mean
    f0_hz of the voiced frames, share of voiced frames), of the waveform the same call returned; None for a table that was not asked
    for.  .params is the PitchTrack; .struct is the zv_pitch, which points into the arrays (kept alive here)."""

    def __init__(self, T: int, n: int, params: PitchTrack):
        self.params = params
        self.frames = np.zeros((T, 2), np.float32) if params.frames else None
        self.phonemes = np.zeros((n, 2), np.float32) if params.phonemes else None

    @property
    def struct(self) -> PitchC:
        p = self.params
        return PitchC(None if self.frames is None else self.frames.ctypes.data, None if self.phonemes is None else self.phonemes.ctypes.data,
                      p.min_lag, p.max_lag, p.window, p.voiced_threshold)

    def __repr__(self):
        shape = lambda a: None if a is None else a.shape
        return f"Pitch(frames={shape(self.frames)}, phonemes={shape(self.phonemes)})"


def _check_pitch(return_pitch, where: str = ""):
    """return_pitch -> a PitchTrack or None (nothing asked for), checked before anything reaches the library: False, True (both
    tables, default parameters), "frames", "phonemes" or a PitchTrack"""
    if isinstance(return_pitch, PitchTrack):
        return return_pitch if return_pitch.frames or return_pitch.phonemes else None
    if isinstance(return_pitch, (bool, np.bool_)):
        return PitchTrack() if return_pitch else None
    if isinstance(return_pitch, str):
        if return_pitch in ("frames", "phonemes"):
            return PitchTrack(frames=return_pitch == "frames", phonemes=return_pitch == "phonemes")
        raise ValueError(f"{where}return_pitch = {return_pitch!r}: expected False, True, 'frames', 'phonemes' or a PitchTrack")
    raise TypeError(f"{where}return_pitch must be a bool, 'frames', 'phonemes' or a PitchTrack, not {type(return_pitch).__name__}")


class BandsC(C.Structure):
    """zv_bands of include/zerovox_amd.h: the two tables' pointers, float [T][n_bands] and [n][n_bands], each or NULL, the band count
    (0 = 16) and the edges' pointer, uint32 [n_bands + 1] or NULL = the default edges (a zeroed struct asks for nothing)"""
    _fields_ = [("frames", C.c_void_p), ("phonemes", C.c_void_p), ("n_bands", C.c_uint32), ("edges", C.c_void_p)]


class BandLevels:
    """What band levels are asked for (include/zerovox_amd.h "band levels"): the band count (0: the default, 16), the edges in DFT bins
    of the 1 024-point transform (None: the default edges; else n_bands + 1 ascending bins, n_bands 0 then meaning len(edges) - 1) and
    which tables.  The library checks the values.  from_hz converts edges in Hz at a sampling rate as the CLI does."""
    N = 1024
    DEFAULT_EDGES = (1, 3, 5, 8, 12, 17, 24, 33, 45, 62, 84, 114, 155, 210, 285, 387, 513)

    def __init__(self, n_bands: int = 0, edges=None, frames: bool = True, phonemes: bool = True):
        if isinstance(n_bands, (bool, np.bool_)) or not isinstance(n_bands, (int, np.integer)):
            raise TypeError(f"BandLevels n_bands must be an integer, not {type(n_bands).__name__}")
        if not 0 <= n_bands <= 0xffffffff:
            raise ValueError(f"BandLevels n_bands = {n_bands} is outside [0, 4294967295]")
        if not (isinstance(frames, (bool, np.bool_)) and isinstance(phonemes, (bool, np.bool_))):
            raise TypeError("BandLevels frames and phonemes must be bools")
        self.edges = None
        if edges is not None:
            e = np.asarray(edges)
            if e.ndim != 1 or e.size < 2 or e.dtype.kind not in "iu" or (e < 0).any() or (e > 0xffffffff).any():
                raise ValueError("BandLevels edges must be a 1-D sequence of at least two non-negative integers")
            if n_bands and e.size != n_bands + 1:
                raise ValueError(f"BandLevels edges has {e.size} entries, n_bands = {n_bands} needs {n_bands + 1}")
            self.edges = np.ascontiguousarray(e, dtype=np.uint32)
            n_bands = e.size - 1
        self.n_bands = int(n_bands)
        self.frames, self.phonemes = bool(frames), bool(phonemes)

    @property
    def width(self) -> int:
        """entries of a row: the band count with the default filled in"""
        return self.n_bands or 16

    @classmethod
    def from_hz(cls, sampling_rate: int, edges_hz, **kw):
        """edges in Hz -> bins round(hz * 1024 / sr); duplicates after rounding are refused"""
        bins = [int(np.floor(float(hz) * cls.N / sampling_rate + 0.5)) for hz in edges_hz]
        if any(b1 <= b0 for b0, b1 in zip(bins, bins[1:])):
            raise ValueError(f"band edges {list(edges_hz)} Hz give the bins {bins}, which do not ascend strictly")
        return cls(edges=bins, **kw)

    def __repr__(self):
        return (f"BandLevels(n_bands={self.n_bands}, edges={None if self.edges is None else self.edges.tolist()}, "
                f"frames={self.frames}, phonemes={self.phonemes})")


class Bands:
    """An utterance's band levels: .frames float32 [T, n_bands] and .phonemes float32 [n, n_bands], the level (RMS re full scale) of
    each band of the waveform the same call returned; None for a table that was not asked for.  .params is the BandLevels; .edges the
    bins in force; dbfs() converts levels to dB re full scale (0 -> -inf); .struct is the zv_bands, which points into the arrays and
    the edges (kept alive here)."""

    def __init__(self, T: int, n: int, params: BandLevels):
        self.params = params
        self.frames = np.zeros((T, params.width), np.float32) if params.frames else None
        self.phonemes = np.zeros((n, params.width), np.float32) if params.phonemes else None

    @property
    def edges(self) -> np.ndarray:
        return np.asarray(BandLevels.DEFAULT_EDGES, np.uint32) if self.params.edges is None else self.params.edges

    @property
    def struct(self) -> BandsC:
        p = self.params
        return BandsC(None if self.frames is None else self.frames.ctypes.data, None if self.phonemes is None else self.phonemes.ctypes.data,
                      p.n_bands, None if p.edges is None else p.edges.ctypes.data)

    @staticmethod
    def dbfs(levels) -> np.ndarray:
        """20 * log10(level), full scale = 1.0; -inf for a level of 0"""
        a = np.asarray(levels, dtype=np.float64)
        with np.errstate(divide="ignore"):
            return 20.0 * np.log10(a)

    def __repr__(self):
        shape = lambda a: None if a is None else a.shape
        return f"Bands(frames={shape(self.frames)}, phonemes={shape(self.phonemes)})"


def _check_bands(return_bands, where: str = ""):
    """return_bands -> a BandLevels or None (nothing asked for), checked before anything reaches the library: False, True (both
    tables, default bands), "frames", "phonemes" or a BandLevels"""
    if isinstance(return_bands, BandLevels):
        return return_bands if return_bands.frames or return_bands.phonemes else None
    if isinstance(return_bands, (bool, np.bool_)):
        return BandLevels() if return_bands else None
    if isinstance(return_bands, str):
        if return_bands in ("frames", "phonemes"):
            return BandLevels(frames=return_bands == "frames", phonemes=return_bands == "phonemes")
        raise ValueError(f"{where}return_bands = {return_bands!r}: expected False, True, 'frames', 'phonemes' or a BandLevels")
    raise TypeError(f"{where}return_bands must be a bool, 'frames', 'phonemes' or a BandLevels, not {type(return_bands).__name__}")


class FilterC(C.Structure):
    """zv_filter of include/zerovox_amd.h: the taps' pointer, float [n_taps] or NULL = no filter, and the tap count (a zeroed struct is
    no filter)"""
    _fields_ = [("taps", C.c_void_p), ("n_taps", C.c_uint32)]


class Filter:
    """A waveform filter (include/zerovox_amd.h "waveform filter"): .taps float32 [n_taps], a linear-phase FIR whose centre tap is
    aligned with the sample, applied on the device ahead of envelope, volume and all meters.  The library checks the values (an odd
    count of 1 .. 511 finite taps).  Filter(None) is "no filter" (n_taps is then not looked at); from_band_gains_db designs the taps
    from gains per band.  .struct is the zv_filter, which points into the array (kept alive here)."""

    def __init__(self, taps, n_taps: Optional[int] = None):
        if taps is None:
            self.taps = None
            self.n_taps = int(n_taps or 0)
            return
        t = np.ascontiguousarray(taps, dtype=np.float32)
        if t.ndim != 1:
            raise ValueError(f"Filter taps must be a 1-D sequence, got shape {t.shape}")
        self.taps = t
        self.n_taps = int(t.size if n_taps is None else n_taps)

    @classmethod
    def from_band_gains_db(cls, gains_db, edges=None, n_taps: int = 255):
        """taps from a gain in dB per band (zv_filter_design): edges in bins of the 1 024-point DFT, None: the default edges of the
        band levels (then 16 gains)"""
        g = np.power(10.0, np.asarray(gains_db, dtype=np.float64) / 20.0).astype(np.float32)
        return cls(filter_design(g, edges, n_taps))

    @property
    def struct(self) -> FilterC:
        return FilterC(None if self.taps is None else self.taps.ctypes.data, self.n_taps)

    def __repr__(self):
        return f"Filter(n_taps={self.n_taps})" if self.taps is not None else "Filter(None)"


def _filter(f, where: str = "") -> Optional[Filter]:
    """filter= -> a Filter or None (nothing passed): a Filter, or a sequence of taps"""
    if f is None or isinstance(f, Filter):
        return f
    if isinstance(f, (str, bytes, dict)):
        raise TypeError(f"{where}filter must be a Filter, a sequence of taps or None, not {type(f).__name__}")
    return Filter(f)


def filter_design(gains, edges=None, n_taps: int = 255, lib=None) -> np.ndarray:
    """zv_filter_design: linear gains per band -> float32 [n_taps]; edges: n_bands + 1 bins of the 1 024-point DFT, or None: the default
    edges of the band levels (then 16 gains).  Host only: no model, no device."""
    lib = lib or load_library()
    g = np.ascontiguousarray(gains, dtype=np.float32)
    if g.ndim != 1 or g.size == 0:
        raise ValueError(f"filter_design: gains must be a non-empty 1-D sequence, got shape {g.shape}")
    e = None
    if edges is not None:
        e = np.asarray(edges)
        if e.ndim != 1 or e.dtype.kind not in "iu" or (e < 0).any() or (e > 0xffffffff).any():
            raise ValueError("filter_design: edges must be a 1-D sequence of non-negative integers")
        if e.size != g.size + 1:
            raise ValueError(f"filter_design: edges has {e.size} entries, {g.size} gains need {g.size + 1}")
        e = np.ascontiguousarray(e, dtype=np.uint32)
    if isinstance(n_taps, (bool, np.bool_)) or not isinstance(n_taps, (int, np.integer)) or not 0 <= n_taps <= 0xffffffff:
        raise ValueError(f"filter_design: n_taps = {n_taps!r} must be an integer in [0, 4294967295]")
    taps = np.zeros(max(int(n_taps), 1), np.float32)
    st = lib.zv_filter_design(g.size, _ptr(e), _ptr(g), int(n_taps), _ptr(taps))
    if st != 0:
        raise ZvError(st, lib.zv_last_error().decode("utf-8", "replace"))
    return taps[:int(n_taps)]


class EnvelopeC(C.Structure):
    """zv_envelope of include/zerovox_amd.h: the gains' pointer ([n] or NULL) and three integers (a zeroed struct is the identity)"""
    _fields_ = [("phoneme_gain", C.c_void_p), ("ramp_frames", C.c_uint32), ("fade_in_samples", C.c_uint32),
                ("fade_out_samples", C.c_uint32)]


ENVELOPE_MAX_GAIN, ENVELOPE_MAX_RAMP, ENVELOPE_MAX_FADE = 16.0, 64, 0x7fffffff


class Envelope:
    """An utterance's amplitude envelope (include/zerovox_amd.h "amplitude envelope"): linear per-phoneme gains (an array [n] or
    None: all 1), the cross-fade half-width in frames and the two fades in samples; the defaults are the identity.  from_db()
    converts from dB and milliseconds.  .struct is the zv_envelope, which points into .phoneme_gain (kept alive here)."""

    def __init__(self, phoneme_gain=None, ramp_frames=0, fade_in_samples=0, fade_out_samples=0):
        self.phoneme_gain = None if phoneme_gain is None else np.ascontiguousarray(phoneme_gain, dtype=np.float32)
        self.ramp_frames, self.fade_in_samples, self.fade_out_samples = ramp_frames, fade_in_samples, fade_out_samples

    @classmethod
    def from_db(cls, phoneme_gain_db=None, ramp_frames=0, fade_in_ms=0, fade_out_ms=0, rate=None):
        """phoneme_gain_db: one gain in dB per phoneme (None: all 0 dB), linear = 10 ** (dB / 20); fade_in_ms / fade_out_ms: the
        fades in milliseconds at `rate` samples per second (needed when one is not 0), floor(ms * rate / 1000 + 0.5) samples"""
        def samples(ms, name):
            if not ms:
                return 0
            if rate is None:
                raise ValueError(f"{name} needs rate, the sampling rate")
            return int(math.floor(float(ms) * float(rate) / 1000.0 + 0.5))
        gain = None if phoneme_gain_db is None else np.array([10.0 ** (float(d) / 20.0) for d in phoneme_gain_db], np.float32)
        return cls(gain, ramp_frames, samples(fade_in_ms, "fade_in_ms"), samples(fade_out_ms, "fade_out_ms"))

    @property
    def struct(self) -> EnvelopeC:
        return EnvelopeC(None if self.phoneme_gain is None else self.phoneme_gain.ctypes.data, self.ramp_frames, self.fade_in_samples,
                         self.fade_out_samples)

    def __repr__(self):
        return (f"Envelope(phoneme_gain={None if self.phoneme_gain is None else self.phoneme_gain.tolist()}, ramp_frames={self.ramp_frames}, "
                f"fade_in_samples={self.fade_in_samples}, fade_out_samples={self.fade_out_samples})")


def _envelope(e, n: int, where: str = "") -> Optional[Envelope]:
    """None, an Envelope or a dict of its fields -> a checked Envelope of its own / None, before anything reaches the library: the
    gains [n] finite numbers in [0, 16], ramp_frames an integer in [0, 64], the fades integers in [0, 0x7fffffff]"""
    if e is None:
        return None
    if isinstance(e, dict):
        unknown = sorted(set(e) - {"phoneme_gain", "ramp_frames", "fade_in_samples", "fade_out_samples"})
        if unknown:
            raise ValueError(f"{where}unknown envelope field(s) {unknown}")
        e = Envelope(**e)
    if not isinstance(e, Envelope):
        raise TypeError(f"{where}an envelope is an Envelope, a dict of its fields or None, not {type(e).__name__}")
    gain = e.phoneme_gain
    if gain is not None:
        gain = np.array(gain, dtype=np.float32)
        if gain.shape != (n,):
            raise ValueError(f"{where}envelope phoneme_gain has shape {gain.shape}, the utterance has {n} phonemes")
        bad = np.flatnonzero(~np.isfinite(gain))
        if bad.size:
            raise ValueError(f"{where}envelope phoneme_gain[{bad[0]}] = {gain[bad[0]]} is not finite")
        bad = np.flatnonzero((gain < 0.0) | (gain > ENVELOPE_MAX_GAIN))
        if bad.size:
            raise ValueError(f"{where}envelope phoneme_gain[{bad[0]}] = {gain[bad[0]]} is outside [0, {ENVELOPE_MAX_GAIN:g}]")
    ints = []
    for name, hi in (("ramp_frames", ENVELOPE_MAX_RAMP), ("fade_in_samples", ENVELOPE_MAX_FADE), ("fade_out_samples", ENVELOPE_MAX_FADE)):
        x = getattr(e, name)
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
            raise TypeError(f"{where}envelope {name} must be an integer, not {type(x).__name__}")
        if not 0 <= x <= hi:
            raise ValueError(f"{where}envelope {name} = {x} is outside [0, {hi}]")
        ints.append(int(x))
    return Envelope(gain, *ints)


class PhonemeControlsC(C.Structure):
    """zv_phoneme_controls of include/zerovox_amd.h: four pointers, each [n] or NULL (a zeroed struct is the identity)"""
    _fields_ = [("duration_frames", C.c_void_p), ("duration_scale", C.c_void_p), ("pitch_shift", C.c_void_p),
                ("energy_shift", C.c_void_p)]


PHONEME_FIELDS = (("duration_frames", np.int32), ("duration_scale", np.float32), ("pitch_shift", np.float32),
                  ("energy_shift", np.float32))


class PhonemeControls:
    """Per-phoneme controls of one utterance of n phonemes: a dict (or keywords) of arrays [n], or None per field (no control of
    that kind).  .struct is the zv_phoneme_controls the C calls read; the converted arrays are kept alive here for the call."""

    def __init__(self, n: int, controls: Optional[dict] = None, **fields):
        d = dict(controls or {})
        d.update(fields)
        names = [name for name, _ in PHONEME_FIELDS]
        unknown = sorted(set(d) - set(names))
        if unknown:
            raise ValueError(f"unknown phoneme control(s) {unknown}; known: {names}")
        self.n = int(n)
        self.arrays = {}
        self.struct = PhonemeControlsC()
        for name, dt in PHONEME_FIELDS:
            v = d.get(name)
            if v is None:
                continue
            a = np.ascontiguousarray(v, dtype=dt)
            if a.ndim != 1 or a.shape[0] != self.n:
                raise ValueError(f"{name}: shape {a.shape}, the utterance has {self.n} phonemes")
            self.arrays[name] = a
            setattr(self.struct, name, a.ctypes.data)

    def __repr__(self):
        return f"PhonemeControls(n={self.n}, fields={sorted(self.arrays)})"


def _phoneme_controls(p, n: int) -> Optional[PhonemeControls]:
    """None, a PhonemeControls for n phonemes or a dict of its fields -> PhonemeControls / None"""
    if p is None:
        return None
    if isinstance(p, PhonemeControls):
        if p.n != n:
            raise ValueError(f"PhonemeControls for {p.n} phonemes, the utterance has {n}")
        return p
    return PhonemeControls(n, p)


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint32), ("total_ms", C.c_double),
                ("algo_bytes", C.c_double), ("algo_flops", C.c_double)]


class ZvError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"zv_status {status}: {msg}")
        self.status = status


_lib = None


def load_library(path: Optional[str] = None):
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ZvError(-1, f"{p} not found: build it with `make -C zerovox.cpp_amd/csrc` (no CPU fallback exists)")
    lib = C.CDLL(p)
    vp, u32, i32p, fp = C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p
    lib.zv_last_error.restype = C.c_char_p
    lib.zv_version.restype = C.c_char_p
    lib.zv_model_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    lib.zv_model_free.argtypes = [vp]
    lib.zv_model_free.restype = None
    lib.zv_model_get_hparams.argtypes = [vp, C.POINTER(HParams)]
    lib.zv_model_reserve.argtypes = [vp, u32, u32]
    lib.zv_encode.argtypes = [vp, i32p, i32p, fp, u32, u32, fp, C.POINTER(u32)]
    lib.zv_encode_taps.argtypes = [vp, i32p, i32p, fp, u32, u32, u32, fp, C.POINTER(u32), fp, fp, fp, fp, i32p, i32p]
    lib.zv_debug_layer.argtypes = [vp, C.c_int, C.c_int, fp, u32, fp, fp]
    if hasattr(lib, "zv_debug_mfma_chain"):
        lib.zv_debug_mfma_chain.argtypes = [vp, C.c_int, C.c_void_p, C.c_void_p, fp, u32, fp]
    lib.zv_debug_set.argtypes = [C.c_char_p, C.c_int]
    lib.zv_debug_get.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    if hasattr(lib, "zv_debug_voc_runs"):        # (an older build named by ZEROVOX_AMD_LIB for an A/B run lacks it)
        lib.zv_debug_voc_runs.argtypes = [vp, u32, C.c_void_p, u32, C.POINTER(u32)]
    if hasattr(lib, "zv_debug_poison"):
        lib.zv_debug_poison.argtypes = [vp, u32, C.c_int, C.POINTER(C.c_size_t)]
    lib.zv_batch_timeline.argtypes = [vp, u32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u32)]
    lib.zv_max_frames.argtypes = [vp]
    lib.zv_max_frames.restype = u32
    lib.zv_demo_utterance.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]
    lib.zv_demo_utterance.restype = None
    lib.zv_decode.argtypes = [vp, fp, fp, u32, fp]
    lib.zv_vocode.argtypes = [vp, fp, u32, fp]
    lib.zv_synthesize.argtypes = [vp, i32p, i32p, fp, u32, u32, fp, C.POINTER(u32)]
    lib.zv_synthesize_batch.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u32), C.POINTER(u32),
                                        C.POINTER(vp), C.POINTER(u32)]
    lib.zv_synthesize_batch_begin.argtypes = [vp, u32, u32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u32), C.POINTER(u32),
                                              C.POINTER(vp), C.POINTER(u32)]
    lib.zv_synthesize_batch_end.argtypes = [vp, u32]
    pp = C.POINTER(Prosody)
    lib.zv_encode_taps_prosody.argtypes = lib.zv_encode_taps.argtypes + [pp]
    lib.zv_synthesize_prosody.argtypes = lib.zv_synthesize.argtypes + [pp]
    lib.zv_synthesize_batch_prosody.argtypes = lib.zv_synthesize_batch.argtypes + [pp]
    lib.zv_synthesize_batch_begin_prosody.argtypes = lib.zv_synthesize_batch_begin.argtypes + [pp]
    pc = C.POINTER(PhonemeControlsC)
    lib.zv_encode_taps_phonemes.argtypes = lib.zv_encode_taps_prosody.argtypes + [pc, i32p]
    lib.zv_synthesize_phonemes.argtypes = lib.zv_synthesize_prosody.argtypes + [pc, i32p]
    lib.zv_synthesize_batch_phonemes.argtypes = lib.zv_synthesize_batch_prosody.argtypes + [pc, C.POINTER(vp)]
    lib.zv_synthesize_batch_begin_phonemes.argtypes = lib.zv_synthesize_batch_begin_prosody.argtypes + [pc, C.POINTER(vp)]
    # the fitted forms take the argument lists of their _phonemes counterparts (an older build named by ZEROVOX_AMD_LIB for an A/B
    # run may lack them: calling one then fails with AttributeError; build() checks SYMBOLS on the tree's own library)
    if hasattr(lib, "zv_synthesize_fitted"):
        lib.zv_synthesize_fitted.argtypes = lib.zv_synthesize_phonemes.argtypes
        lib.zv_synthesize_batch_fitted.argtypes = lib.zv_synthesize_batch_phonemes.argtypes
        lib.zv_synthesize_batch_begin_fitted.argtypes = lib.zv_synthesize_batch_begin_phonemes.argtypes
    # the target forms: the _phonemes argument lists, the target (batches: uint32 [n_utt] or NULL) and, for the synthesize forms, fitted
    if hasattr(lib, "zv_synthesize_target"):
        lib.zv_encode_taps_target.argtypes = lib.zv_encode_taps_phonemes.argtypes + [u32]
        lib.zv_synthesize_target.argtypes = lib.zv_synthesize_phonemes.argtypes + [u32, C.c_int]
        lib.zv_synthesize_batch_target.argtypes = lib.zv_synthesize_batch_phonemes.argtypes + [C.POINTER(u32), C.c_int]
        lib.zv_synthesize_batch_begin_target.argtypes = lib.zv_synthesize_batch_begin_phonemes.argtypes + [C.POINTER(u32), C.c_int]
    # the volume forms: the _target argument lists, the volumes (zv_volume, batches [n_utt]) and the levels (zv_level, likewise), each or NULL
    if hasattr(lib, "zv_synthesize_volume"):
        vl = [C.POINTER(Volume), C.POINTER(Level)]
        lib.zv_synthesize_volume.argtypes = lib.zv_synthesize_target.argtypes + vl
        lib.zv_synthesize_batch_volume.argtypes = lib.zv_synthesize_batch_target.argtypes + vl
        lib.zv_synthesize_batch_begin_volume.argtypes = lib.zv_synthesize_batch_begin_target.argtypes + vl
    # the envelope forms: the _volume argument lists and the envelopes (zv_envelope, batches [n_utt]) or NULL
    if hasattr(lib, "zv_synthesize_envelope"):
        ev = [C.POINTER(EnvelopeC)]
        lib.zv_synthesize_envelope.argtypes = lib.zv_synthesize_volume.argtypes + ev
        lib.zv_synthesize_batch_envelope.argtypes = lib.zv_synthesize_batch_volume.argtypes + ev
        lib.zv_synthesize_batch_begin_envelope.argtypes = lib.zv_synthesize_batch_begin_volume.argtypes + ev
    # the contour forms: the _envelope argument lists and the contours (zv_contour, batches [n_utt]) or NULL
    if hasattr(lib, "zv_synthesize_contour"):
        ct = [C.POINTER(ContourC)]
        lib.zv_synthesize_contour.argtypes = lib.zv_synthesize_envelope.argtypes + ct
        lib.zv_synthesize_batch_contour.argtypes = lib.zv_synthesize_batch_envelope.argtypes + ct
        lib.zv_synthesize_batch_begin_contour.argtypes = lib.zv_synthesize_batch_begin_envelope.argtypes + ct
    # the pitch forms: the _contour argument lists and the pitch tracks (zv_pitch, batches [n_utt]) or NULL; the stand-alone meter
    if hasattr(lib, "zv_synthesize_pitch"):
        pt = [C.POINTER(PitchC)]
        lib.zv_synthesize_pitch.argtypes = lib.zv_synthesize_contour.argtypes + pt
        lib.zv_synthesize_batch_pitch.argtypes = lib.zv_synthesize_batch_contour.argtypes + pt
        lib.zv_synthesize_batch_begin_pitch.argtypes = lib.zv_synthesize_batch_begin_contour.argtypes + pt
        lib.zv_pitch_track.argtypes = [vp, vp, C.c_uint32, C.POINTER(PitchC)]
    # the bands forms: the _pitch argument lists and the band levels (zv_bands, batches [n_utt]) or NULL; the stand-alone meter
    if hasattr(lib, "zv_synthesize_bands"):
        bt = [C.POINTER(BandsC)]
        lib.zv_synthesize_bands.argtypes = lib.zv_synthesize_pitch.argtypes + bt
        lib.zv_synthesize_batch_bands.argtypes = lib.zv_synthesize_batch_pitch.argtypes + bt
        lib.zv_synthesize_batch_begin_bands.argtypes = lib.zv_synthesize_batch_begin_pitch.argtypes + bt
        lib.zv_band_levels.argtypes = [vp, vp, C.c_uint32, C.POINTER(BandsC)]
    # the filter forms: the _bands argument lists and the waveform filter (zv_filter, batches [n_utt]) or NULL; the stand-alone filter
    # and the design
    if hasattr(lib, "zv_synthesize_filter"):
        ft = [C.POINTER(FilterC)]
        lib.zv_synthesize_filter.argtypes = lib.zv_synthesize_bands.argtypes + ft
        lib.zv_synthesize_batch_filter.argtypes = lib.zv_synthesize_batch_bands.argtypes + ft
        lib.zv_synthesize_batch_begin_filter.argtypes = lib.zv_synthesize_batch_begin_bands.argtypes + ft
        lib.zv_filter_wave.argtypes = [vp, vp, C.c_uint32, C.POINTER(FilterC), vp]
        lib.zv_filter_design.argtypes = [C.c_uint32, vp, vp, C.c_uint32, vp]
    lib.zv_device_alloc.argtypes = [vp, C.c_size_t]
    lib.zv_device_alloc.restype = vp
    lib.zv_device_free.argtypes = [vp, vp]
    lib.zv_device_free.restype = None
    lib.zv_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    lib.zv_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    lib.zv_vocode_device.argtypes = [vp, vp, u32, vp]
    lib.zv_vocode_stream.argtypes = [vp, fp, u32, u32, WAV_SINK, vp]
    lib.zv_vocoder_halo_frames.argtypes = [vp]
    lib.zv_vocoder_halo_frames.restype = u32
    lib.zv_decode_device.argtypes = [vp, vp, vp, u32, vp]
    lib.zv_synchronize.argtypes = [vp]
    lib.zv_set_graph_mode.argtypes = [vp, C.c_int]
    lib.zv_profile_begin.argtypes = [vp]
    lib.zv_profile_end.argtypes = [vp, C.POINTER(KernelStat), u32, C.POINTER(u32)]
    lib.zv_write_wav.argtypes = [C.c_char_p, fp, C.c_size_t, u32]
    lib.zv_gguf_inspect.argtypes = [C.c_char_p, C.POINTER(u32), C.POINTER(u32), C.c_int, C.c_char_p, C.POINTER(u32),
                                    C.POINTER(C.c_int64)]
    if path is None:
        _lib = lib
    _forward_env_switches(lib)
    return lib


def _forward_env_switches(lib):
    """The shipped library never reads the environment.  This test / bench binding forwards ZV_* variables that name a switch
    (csrc/knobs.h) through zv_debug_set, once per load, so that `ZV_PAIR_MT=4 python bench.py` still A/Bs a run; variables that
    name no switch of this build (ZV_BENCH_LANES, a diagnostic switch on a shipped build ...) are left alone."""
    for k, v in sorted(os.environ.items()):
        if not k.startswith("ZV_"):
            continue
        try:
            val = int(v)
        except ValueError:
            continue
        cur = C.c_int(0)
        if lib.zv_debug_get(k.encode(), C.byref(cur)) == 0:
            lib.zv_debug_set(k.encode(), val)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ref(x):
    return None if x is None else C.byref(x)


def _check_fitted(fitted, Ts):
    """the `fitted` flag and the frame capacities of a synthesize call, checked before anything reaches the library"""
    if not isinstance(fitted, (bool, np.bool_)):
        raise TypeError(f"fitted must be a bool, not {type(fitted).__name__}")
    for T in Ts:
        if isinstance(T, (bool, np.bool_)) or not isinstance(T, (int, np.integer)):
            raise TypeError(f"T must be an integer frame capacity, not {type(T).__name__}")
        if T <= 0:
            raise ValueError(f"T = {T}: the frame capacity must be > 0")
    return bool(fitted)


def _check_target(target, T):
    """a target frame count (None: the call has none) against the capacity T, checked before anything reaches the library"""
    if target is None:
        return None
    if isinstance(target, (bool, np.bool_)) or not isinstance(target, (int, np.integer)):
        raise TypeError(f"target_frames must be an integer frame count, not {type(target).__name__}")
    if target < 0:
        raise ValueError(f"target_frames = {target}: a frame count cannot be negative")
    if target > T:
        raise ValueError(f"target_frames = {target} exceeds the frame capacity T = {T}")
    return int(target)


def _call_variant(lib, name, args, prosody=None, phonemes=None, durations=None, fitted=False, target=None, volume=None, levels=None,
                  envelope=None, contour=None, pitch=None, bands=None, filter=None):
    """entry point `name` in the form that carries what the call has: name_phonemes with per-phoneme controls or timings,
    name_prosody with prosody alone, `name` itself with neither (the forms agree bit for bit on NULL controls); its status.
    fitted: name_fitted, which takes everything (NULL for what the call lacks).  target (a frame count, or the batches' uint32
    array): name_target, which takes everything and the fitted flag.  volume / levels (a zv_volume and a zv_level, or the batches'
    arrays): name_volume, which takes everything the _target form takes and the two (a call without a target passes 0 / NULL).
    envelope (a zv_envelope, or the batches' array): name_envelope, which takes everything the _volume form takes and the envelope.
    contour (a zv_contour, or the batches' array): name_contour, which takes everything the _envelope form takes and the contour;
    only a call that asks for a contour goes there.  pitch (a zv_pitch, or the batches' array): name_pitch, which takes everything the
    _contour form takes and the pitch track; only a call that asks for a pitch track goes there.  bands (a zv_bands, or the batches'
    array): name_bands, which takes everything the _pitch form takes and the band levels; only a call that asks for them goes there.
    filter (a zv_filter, or the batches' array): name_filter, which takes everything the _bands form takes and the filter; only a call
    that passes a filter goes there"""
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


def debug_set(name: Optional[str], value: int = 0):
    """zv_debug_set: one test / measurement switch (csrc/knobs.h); name None resets every switch to its default"""
    lib = load_library()
    st = lib.zv_debug_set(None if name is None else name.encode(), int(value))
    if st != 0:
        raise ZvError(st, lib.zv_last_error().decode())


def debug_get(name: str) -> int:
    lib = load_library()
    v = C.c_int(0)
    st = lib.zv_debug_get(name.encode(), C.byref(v))
    if st != 0:
        raise ZvError(st, lib.zv_last_error().decode())
    return int(v.value)


class switches:
    """`with capi.switches(ZV_NO_FUSE=1, ...):` — the switches hold inside the block (every one is read at every
    call, so a call runs in a regime exactly when it sits inside the block, whenever its model was built; captured graphs are
    re-captured) and go back to the values they had
    before it afterwards (not to their built-in defaults: a value set for the whole run, e.g. ZV_ARENA_FILL=255, survives,
    and blocks nest)"""

    def __init__(self, **kw):
        self.kw = kw
        self.saved = {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.saved[k] = debug_get(k)
            debug_set(k, int(v))
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            debug_set(k, v)
        return False


class Model:
    """One loaded checkpoint on one MI355X (zv_model)."""

    def __init__(self, gguf_path: str, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        st = self.lib.zv_model_load(gguf_path.encode(), device, C.byref(h))
        if st != 0:
            raise ZvError(st, self.lib.zv_last_error().decode())
        self.h = h
        hp = HParams()
        self._chk(self.lib.zv_model_get_hparams(self.h, C.byref(hp)))
        self.hp = hp
        self.E = hp.emb_dim + hp.punct_emb_dim

    def close(self):
        if getattr(self, "h", None):
            self.lib.zv_model_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st):
        if st != 0:
            raise ZvError(st, self.lib.zv_last_error().decode())

    # ---- host-buffer API (same call protocol as the reference's eval methods) ----
    def vocode(self, mel: np.ndarray) -> np.ndarray:
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        T = mel.shape[0]
        wav = np.empty(T * self.hp.audio_hop_size, np.float32)
        self._chk(self.lib.zv_vocode(self.h, _ptr(mel), T, _ptr(wav)))
        return wav

    def vocode_stream(self, mel: np.ndarray, chunk_frames: int):
        """chunked vocoding with halo (zv_vocode_stream): list of (first_sample, samples) in delivery order"""
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        chunks = []

        def sink(_user, wav, first, n):
            chunks.append((int(first), np.ctypeslib.as_array(wav, shape=(int(n),)).copy()))

        cb = WAV_SINK(sink)
        self._chk(self.lib.zv_vocode_stream(self.h, _ptr(mel), mel.shape[0], chunk_frames, cb, None))
        return chunks

    def vocoder_halo_frames(self) -> int:
        return int(self.lib.zv_vocoder_halo_frames(self.h))

    def decode(self, hidden: np.ndarray, style: np.ndarray) -> np.ndarray:
        hidden = np.ascontiguousarray(hidden, dtype=np.float32)
        style = np.ascontiguousarray(style, dtype=np.float32)
        T = hidden.shape[0]
        mel = np.empty((T, self.hp.audio_num_mels), np.float32)
        self._chk(self.lib.zv_decode(self.h, _ptr(hidden), _ptr(style), T, _ptr(mel)))
        return mel

    LAYER_VOC_RESBLOCK, LAYER_ENC_FFT, LAYER_DEC_BLOCK, LAYER_VAR_PRED = 0, 1, 2, 3
    LAYER_VOC_UPSAMPLE, LAYER_VOC_INPUT, LAYER_VOC_OUTPUT, LAYER_DEC_ASR_RES, LAYER_DEC_TO_OUT, LAYER_ENC_EMBED = 4, 5, 6, 7, 8, 9
    LAYER_ENC_MHA, LAYER_ENC_FFN, LAYER_DEC_ADAIN, LAYER_ENC_LN = 10, 11, 12, 13

    def debug_layer(self, kind: int, index: int, x: np.ndarray, out_cols: int, style=None, out_rows: Optional[int] = None) -> np.ndarray:
        """zv_debug_layer: one layer of the production schedule on the given input (time-major [rows][cin]); out_rows when the
        layer changes the rate (transposed conv: rows x scale)"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        orows = x.shape[0] if out_rows is None else out_rows
        out = np.empty((orows, out_cols) if out_cols else (orows,), np.float32)
        st = None if style is None else np.ascontiguousarray(style, dtype=np.float32)
        self._chk(self.lib.zv_debug_layer(self.h, kind, index, _ptr(x), x.shape[0], _ptr(st), _ptr(out)))
        return out

    MFMA_32X32X16_F16, MFMA_16X16X32_F16, MFMA_32X32X2_F32 = 0, 1, 2

    def debug_mfma_chain(self, form: int, a: np.ndarray, b: np.ndarray, c0: np.ndarray) -> np.ndarray:
        """zv_debug_mfma_chain: out[32][32] = c0 + a[32][K] . b[K][32], every element one k-ordered chain of one wave on the
        matrix-core instruction `form` (0: 32x32x16 f16, 1: 16x16x32 f16 — a, b float16; 2: 32x32x2 f32 — a, b float32)"""
        dt = np.float32 if form == self.MFMA_32X32X2_F32 else np.float16
        if a.dtype != dt or b.dtype != dt:
            raise TypeError(f"form {form} takes {np.dtype(dt).name} operands, not {a.dtype} / {b.dtype}")
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        c0 = np.ascontiguousarray(c0, dtype=np.float32)
        K = a.shape[1] if a.ndim == 2 else -1
        if a.shape != (32, K) or b.shape != (K, 32) or c0.shape != (32, 32):
            raise ValueError(f"shapes a {a.shape}, b {b.shape}, c0 {c0.shape}: want [32][K], [K][32], [32][32]")
        out = np.empty((32, 32), np.float32)
        self._chk(self.lib.zv_debug_mfma_chain(self.h, form, a.ctypes.data, b.ctypes.data, _ptr(c0), K, _ptr(out)))
        return out

    def voc_rate(self, stage: int) -> int:
        r = 1
        for i in range(stage + 1):
            r *= self.hp.voc_upsample_scales[i]
        return r

    def voc_channels(self, stage: int) -> int:
        return self.hp.voc_channels >> (stage + 1)

    def max_frames(self) -> int:
        return int(self.lib.zv_max_frames(self.h))

    def encode(self, ids, puncts, style, T: int, num_phonemes: Optional[int] = None, prosody=None, phonemes=None,
               return_durations: bool = False, target_frames: Optional[int] = None) -> dict:
        """num_phonemes < len(ids): all ids are encoded, the length regulator walks the first num_phonemes (FS2Encoder::eval).
        prosody (Prosody, dict or 5-sequence): zv_encode_taps_prosody; None: zv_encode_taps.
        phonemes (PhonemeControls or dict of arrays [len(ids)]) or return_durations: zv_encode_taps_phonemes, and the result gains
        "durations" (the phoneme timings, int32 [len(ids)]).
        target_frames (0 <= frames <= T): zv_encode_taps_target — the durations are fitted to sum to exactly that many frames (0: the
        bits of the call without it); None: the entry points above"""
        target = _check_target(target_frames, T)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        puncts = np.ascontiguousarray(puncts, dtype=np.int32)
        style = np.ascontiguousarray(style, dtype=np.float32)
        N, E = len(ids), self.E
        out = dict(hidden=np.empty((T, E), np.float32), features=np.empty((N, E), np.float32),
                   logdur=np.empty(N, np.float32), pitch=np.empty(N, np.float32), energy=np.empty(N, np.float32),
                   pitch_bucket=np.empty(N, np.int32), energy_bucket=np.empty(N, np.int32))
        nf = C.c_uint32(0)
        args = (self.h, _ptr(ids), _ptr(puncts), _ptr(style), N, N if num_phonemes is None else num_phonemes, T, _ptr(out["hidden"]),
                C.byref(nf), _ptr(out["features"]), _ptr(out["logdur"]), _ptr(out["pitch"]), _ptr(out["energy"]),
                _ptr(out["pitch_bucket"]), _ptr(out["energy_bucket"]))
        pc = _phoneme_controls(phonemes, N)
        if pc is not None or return_durations:
            out["durations"] = np.empty(N, np.int32)
        if target is not None:
            self._chk(self.lib.zv_encode_taps_target(*args, _ref(_prosody(prosody)), _ref(None if pc is None else pc.struct),
                                                     _ptr(out.get("durations")), target))
        else:
            self._chk(_call_variant(self.lib, "zv_encode_taps", args, _ref(_prosody(prosody)), _ref(None if pc is None else pc.struct),
                                    _ptr(out.get("durations"))))
        out["n_frames"] = int(nf.value)
        return out

    def synthesize(self, ids, puncts, style, T: int, prosody=None, phonemes=None, return_durations: bool = False,
                   fitted: bool = False, target_frames: Optional[int] = None, *, volume=None, return_levels: bool = False,
                   envelope=None, return_contour=False, return_pitch=False, return_bands=False, filter=None):
        """prosody (Prosody, dict or 5-sequence): zv_synthesize_prosody; None: zv_synthesize.  phonemes (PhonemeControls or dict of
        arrays [len(ids)]) or return_durations: zv_synthesize_phonemes; return_durations adds the phoneme timings (int32 [len(ids)])
        as a third element.  fitted: zv_synthesize_fitted — T is a capacity, the utterance is decoded and vocoded as the n_frames
        the length regulator fills; wav keeps the capacity shape [T * hop], zero behind n_frames * hop.
        target_frames (0 <= frames <= T): zv_synthesize_target — the durations are fitted to sum to exactly that many frames (0: the
        bits of the call without it); None: the entry points above.
        volume (Volume, dict or (gain, target_rms, peak_ceiling)) or return_levels: zv_synthesize_volume — the waveform is measured
        and scaled on the device; return_levels adds the Level (rms and peak before the gain, the gain) as the last element.
        envelope (Envelope or dict of its fields): zv_synthesize_envelope — per-phoneme gains, cross-fades and fades, applied on the
        device ahead of the volume.
        return_contour (False, True, "frames" or "phonemes"): zv_synthesize_contour — the level and peak of every frame and / or every
        phoneme of the returned waveform, metered on the device; adds a Contour as the last element.
        return_pitch (False, True, "frames", "phonemes" or a PitchTrack): zv_synthesize_pitch — the fundamental frequency and voicing
        of every frame and / or every phoneme of the returned waveform, metered on the device; adds a Pitch as the last element.
        return_bands (False, True, "frames", "phonemes" or a BandLevels): zv_synthesize_bands — the level per frequency band of every
        frame and / or every phoneme of the returned waveform, metered on the device; adds a Bands as the last element.
        filter (a Filter, a sequence of taps or None): zv_synthesize_filter — a linear-phase FIR applied to the waveform on the device,
        ahead of envelope, volume and all meters"""
        flt = _filter(filter)
        want_frames, want_phonemes = _check_contour(return_contour)
        track = _check_pitch(return_pitch)
        spec = _check_bands(return_bands)
        fitted = _check_fitted(fitted, [T])
        target = _check_target(target_frames, T)
        vol, return_levels = _volume(volume), _check_levels(return_levels)
        env = _envelope(envelope, len(ids))
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        puncts = np.ascontiguousarray(puncts, dtype=np.int32)
        style = np.ascontiguousarray(style, dtype=np.float32)
        wav = np.empty(T * self.hp.audio_hop_size, np.float32)
        nf = C.c_uint32(0)
        args = (self.h, _ptr(ids), _ptr(puncts), _ptr(style), len(ids), T, _ptr(wav), C.byref(nf))
        pc = _phoneme_controls(phonemes, len(ids))
        dur = np.empty(len(ids), np.int32) if return_durations else None
        level = Level() if vol is not None or return_levels else None
        contour = Contour(T, len(ids), want_frames, want_phonemes) if want_frames or want_phonemes else None
        pitch = Pitch(T, len(ids), track) if track is not None else None
        bands = Bands(T, len(ids), spec) if spec is not None else None
        if (level is not None or env is not None or contour is not None or pitch is not None or bands is not None or flt is not None) and target is None:
            target = 0                       # the _volume, _envelope, _contour, _pitch, _bands and _filter forms take a count, 0 = none
        self._chk(_call_variant(self.lib, "zv_synthesize", args, _ref(_prosody(prosody)), _ref(None if pc is None else pc.struct), _ptr(dur),
                                fitted, target, _ref(vol), _ref(level), _ref(None if env is None else env.struct),
                                _ref(None if contour is None else contour.struct), _ref(None if pitch is None else pitch.struct),
                                _ref(None if bands is None else bands.struct), _ref(None if flt is None else flt.struct)))
        out = (wav, int(nf.value), dur) if return_durations else (wav, int(nf.value))
        out = out + (level,) if return_levels else out
        out = out + (contour,) if contour is not None else out
        out = out + (pitch,) if pitch is not None else out
        return out + (bands,) if bands is not None else out

    def filter_wave(self, wav, filter) -> np.ndarray:
        """zv_filter_wave: a waveform the caller brings (float32 [T * hop] at the model's hop) through the filter (a Filter or a
        sequence of taps) on the device; returns the filtered waveform"""
        flt = _filter(filter)
        if flt is None:
            raise TypeError("filter_wave: filter must be a Filter or a sequence of taps, not None")
        w = np.ascontiguousarray(wav, dtype=np.float32)
        hop = self.hp.audio_hop_size
        if w.ndim != 1 or w.size == 0 or w.size % hop:
            raise ValueError(f"filter_wave: the waveform must be a non-empty 1-D array of a multiple of {hop} samples, got shape {w.shape}")
        out = np.empty_like(w)
        st = flt.struct
        self._chk(self.lib.zv_filter_wave(self.h, _ptr(w), w.size // hop, C.byref(st), _ptr(out)))
        return out

    def band_levels(self, wav, params=None) -> Bands:
        """zv_band_levels: the band levels of a waveform the caller brings (float32 [T * hop] at the model's rate and hop), frames
        only; params: a BandLevels or None (the default bands)"""
        if params is not None and not isinstance(params, BandLevels):
            raise TypeError(f"band_levels: params must be a BandLevels or None, not {type(params).__name__}")
        p = params or BandLevels()
        spec = BandLevels(p.n_bands if p.edges is None else 0, p.edges, True, False)      # a waveform has no timings
        w = np.ascontiguousarray(wav, dtype=np.float32)
        hop = self.hp.audio_hop_size
        if w.ndim != 1 or w.size == 0 or w.size % hop:
            raise ValueError(f"band_levels: the waveform must be a non-empty 1-D array of a multiple of {hop} samples, got shape {w.shape}")
        bands = Bands(w.size // hop, 0, spec)
        st = bands.struct
        self._chk(self.lib.zv_band_levels(self.h, _ptr(w), w.size // hop, C.byref(st)))
        return bands

    def pitch_track(self, wav, params=None) -> Pitch:
        """zv_pitch_track: the pitch track of a waveform the caller brings (float32 [T * hop] at the model's rate and hop), frames
        only; params: a PitchTrack or None (the defaults)"""
        if params is not None and not isinstance(params, PitchTrack):
            raise TypeError(f"pitch_track: params must be a PitchTrack or None, not {type(params).__name__}")
        p = params or PitchTrack()
        track = PitchTrack(p.min_lag, p.max_lag, p.window, p.voiced_threshold, True, False)      # a waveform has no timings
        w = np.ascontiguousarray(wav, dtype=np.float32)
        hop = self.hp.audio_hop_size
        if w.ndim != 1 or w.size == 0 or w.size % hop:
            raise ValueError(f"pitch_track: the waveform must be a non-empty 1-D array of a multiple of {hop} samples, got shape {w.shape}")
        pitch = Pitch(w.size // hop, 0, track)
        st = pitch.struct
        self._chk(self.lib.zv_pitch_track(self.h, _ptr(w), w.size // hop, C.byref(st)))
        return pitch

    def prepare_batch(self, utterances, durations: bool = False, fitted: bool = False, *, volume=None,
                      return_levels: bool = False, envelope=None, return_contour=False, return_pitch=False,
                      return_bands=False, filter=None) -> "BatchCall":
        """argument arrays and output buffers of one zv_synthesize_batch call, built once (a C host would keep its
        buffers too): .run() is exactly one call of the C entry point, .results() the (wav, n_frames) list.  fitted: the
        zv_synthesize_batch_fitted / _begin_fitted entry points (the lane form: .begin(lane) / .end(lane))"""
        return BatchCall(self, utterances, durations, fitted, volume=volume, return_levels=return_levels, envelope=envelope,
                         return_contour=return_contour, return_pitch=return_pitch, return_bands=return_bands, filter=filter)

    def synthesize_batch(self, utterances, return_durations: bool = False, fitted: bool = False, *, volume=None,
                         return_levels: bool = False, envelope=None, return_contour=False, return_pitch=False, return_bands=False,
                         filter=None):
        """utterances: list of (ids, puncts, style, T[, prosody[, phonemes[, target_frames]]]) -> list of (wav, n_frames); each
        utterance keeps its own (N, T) and, with a fifth element, its own prosody controls (None: identity), with a sixth its
        per-phoneme controls (PhonemeControls, dict of arrays or None), with a seventh its target frame count (None / 0: none).  return_durations: (wav, n_frames, durations) tuples.  fitted:
        zv_synthesize_batch_fitted — every T is a capacity, wav keeps the capacity shape with zeros behind n_frames * hop.
        volume: a list, one Volume (dict, 3-sequence) or None per utterance — zv_synthesize_batch_volume; return_levels: every tuple
        gains the utterance's Level as its last element.  envelope: a list, one Envelope (dict) or None per utterance —
        zv_synthesize_batch_envelope.  return_contour: False, True, "frames" or "phonemes" for the whole batch, or a list with one of
        them per utterance — zv_synthesize_batch_contour; every tuple gains the utterance's Contour (None where it asked for none) as
        its last element.  return_pitch: False, True, "frames", "phonemes" or a PitchTrack for the whole batch, or a list with one of
        them per utterance — zv_synthesize_batch_pitch; every tuple gains the utterance's Pitch (None where it asked for none) last.
        return_bands: likewise with a BandLevels — zv_synthesize_batch_bands; every tuple gains the utterance's Bands last.
        filter: a list with a Filter, a sequence of taps or None per utterance — zv_synthesize_batch_filter"""
        call = BatchCall(self, utterances, return_durations, fitted, volume=volume, return_levels=return_levels, envelope=envelope,
                         return_contour=return_contour, return_pitch=return_pitch, return_bands=return_bands, filter=filter)
        call.run()
        res = call.results()
        if return_durations:
            res = [r + (d,) for r, d in zip(res, call.durations)]
        if call.return_levels:
            res = [r + (Level.from_buffer_copy(lv),) for r, lv in zip(res, call.levels)]
        if call.contour is not None:
            res = [r + (c,) for r, c in zip(res, call.contours)]
        if call.pitch is not None:
            res = [r + (p,) for r, p in zip(res, call.pitches)]
        if call.band is not None:
            res = [r + (b,) for r, b in zip(res, call.bands)]
        return res

    # ---- device-resident API ----
    def device_alloc(self, nbytes: int) -> int:
        p = self.lib.zv_device_alloc(self.h, nbytes)
        if not p:
            raise ZvError(7, "zv_device_alloc failed")
        return p

    def device_free(self, p: int):
        self.lib.zv_device_free(self.h, p)

    def h2d(self, dst: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._chk(self.lib.zv_memcpy_h2d(self.h, dst, _ptr(arr), arr.nbytes))

    def d2h(self, arr: np.ndarray, src: int):
        self._chk(self.lib.zv_memcpy_d2h(self.h, _ptr(arr), src, arr.nbytes))

    def vocode_device(self, d_mel: int, T: int, d_wav: int):
        self._chk(self.lib.zv_vocode_device(self.h, d_mel, T, d_wav))

    def decode_device(self, d_hidden: int, d_style: int, T: int, d_mel: int):
        self._chk(self.lib.zv_decode_device(self.h, d_hidden, d_style, T, d_mel))

    def synchronize(self):
        self._chk(self.lib.zv_synchronize(self.h))

    def set_graph_mode(self, on: bool):
        self._chk(self.lib.zv_set_graph_mode(self.h, int(on)))

    def reserve(self, max_phonemes: int, max_frames: int):
        self._chk(self.lib.zv_model_reserve(self.h, max_phonemes, max_frames))

    def batch_timeline(self, cap: int = 64):
        """zv_batch_timeline: [(start_ms, end_ms)] of the most recent batches, oldest first"""
        a, b, n = (C.c_double * cap)(), (C.c_double * cap)(), C.c_uint32(0)
        self._chk(self.lib.zv_batch_timeline(self.h, cap, a, b, C.byref(n)))
        return [(a[i], b[i]) for i in range(n.value)]

    def voc_runs(self, lane: int = 0) -> np.ndarray:
        """zv_debug_voc_runs: the run table of the lane's most recent vocoder pass, int32 [utterances][4] = (row0, frames vocoded,
        split frame, frames skipped); no rows when that pass ran without run-shortening"""
        cap = 64
        tab = np.zeros((cap, 4), np.int32)
        n = C.c_uint32(0)
        self._chk(self.lib.zv_debug_voc_runs(self.h, lane, _ptr(tab), cap, C.byref(n)))
        return tab[:min(cap, n.value)].copy()

    def poison(self, byte: int = 0xFF, lane: int = 0):
        """zv_debug_poison: fills everything `lane` keeps between calls (activation arena, device I/O block, pinned staging block)
        with `byte`; (arena_bytes, io_bytes, pinned_bytes) filled, 0 for a block the lane has not allocated yet"""
        filled = (C.c_size_t * 3)()
        self._chk(self.lib.zv_debug_poison(self.h, lane, int(byte), filled))
        return int(filled[0]), int(filled[1]), int(filled[2])

    def profile_begin(self):
        self._chk(self.lib.zv_profile_begin(self.h))

    def profile_end(self) -> list:
        cap = 64
        arr = (KernelStat * cap)()
        n = C.c_uint32(0)
        self._chk(self.lib.zv_profile_end(self.h, arr, cap, C.byref(n)))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms,
                     algo_bytes=arr[i].algo_bytes, algo_flops=arr[i].algo_flops) for i in range(min(cap, n.value))]


class BatchCall:
    """utterances: (ids, puncts, style, T), (ids, puncts, style, T, prosody), (ids, puncts, style, T, prosody, phonemes) or
    (ids, puncts, style, T, prosody, phonemes, target_frames) tuples.  When any utterance carries a target frame count (a seventh
    element that is not None) the _target entry points are called with the uint32 array .targets (0 for the others), which
    set_target_frames() rewrites in place: the next run() / begin() fits the durations to the new targets with the same buffers.  When any utterance carries a prosody (the others get the identity) the _prosody entry points are called with the
    array .prosody, which set_prosody() rewrites in place: the next run() / begin() uses the new values with the same buffers (a
    captured graph replays with them).  When any utterance carries per-phoneme controls, or durations=True, the _phonemes entry
    points are called with the array .phonemes (set_phoneme_controls() rewrites an entry) and .durations[i] holds utterance i's
    phoneme timings after run() / end().  fitted: the _fitted entry points, whatever controls the utterances carry.
    volume (a list, one Volume / dict / 3-sequence or None per utterance) or return_levels: the _volume entry points, with the array
    .volume (None entries get the identity; set_volume() rewrites an entry in place for the next run() / begin()) and the array .levels,
    which holds every utterance's Level after run() / end().
    envelope (a list, one Envelope / dict or None per utterance): the _envelope entry points, with the zv_envelope array .envelope (None
    entries get the identity; set_envelope() rewrites an entry for the next run() / begin()); .ekeep[i] is utterance i's checked
    Envelope, whose gains the array points into.
    return_contour (False, True, "frames" or "phonemes" for the whole batch, or a list with one of them per utterance): where any
    utterance asks for a table, the _contour entry points, with the zv_contour array .contour; .contours[i] is utterance i's Contour
    (None where it asked for none), whose arrays hold its rows after run() / end().
    return_pitch (False, True, "frames", "phonemes" or a PitchTrack for the whole batch, or a list with one of them per utterance): where
    any utterance asks for a table, the _pitch entry points, with the zv_pitch array .pitch; .pitches[i] is utterance i's Pitch (None
    where it asked for none); set_pitch() rewrites an entry's parameters and tables for the next run() / begin().
    return_bands (False, True, "frames", "phonemes" or a BandLevels for the whole batch, or a list with one of them per utterance): where
    any utterance asks for a table, the _bands entry points, with the zv_bands array .band; .bands[i] is utterance i's Bands (None where
    it asked for none); set_bands() rewrites an entry's band count, edges and tables for the next run() / begin().
    filter (a list with a Filter, a sequence of taps or None per utterance): the _filter entry points, with the zv_filter array .filter;
    set_filter() rewrites an entry's taps for the next run() / begin()."""

    def __init__(self, model: Model, utterances, durations: bool = False, fitted: bool = False, *, volume=None,
                 return_levels: bool = False, envelope=None, return_contour=False, return_pitch=False, return_bands=False, filter=None):
        self.fitted = _check_fitted(fitted, [u[3] for u in utterances])
        self.filter = self.fkeep = None
        if filter is not None:
            flts = list(filter)
            if len(flts) != len(utterances):
                raise ValueError(f"filter has {len(flts)} entries, the batch has {len(utterances)} utterances")
            self.fkeep = [_filter(f, f"utterance {i}: ") for i, f in enumerate(flts)]
            self.filter = (FilterC * len(utterances))(*[f.struct if f is not None else FilterC() for f in self.fkeep])
        if isinstance(return_bands, (list, tuple)):
            if len(return_bands) != len(utterances):
                raise ValueError(f"return_bands has {len(return_bands)} entries, the batch has {len(utterances)} utterances")
            specs = [_check_bands(w, f"utterance {i}: ") for i, w in enumerate(return_bands)]
        else:
            specs = [_check_bands(return_bands)] * len(utterances)
        self.band = self.bands = None
        if any(t is not None for t in specs):
            self.bands = [Bands(u[3], len(u[0]), t) if t is not None else None for t, u in zip(specs, utterances)]
            self.band = (BandsC * len(utterances))(*[b.struct if b is not None else BandsC() for b in self.bands])
        if isinstance(return_pitch, (list, tuple)):
            if len(return_pitch) != len(utterances):
                raise ValueError(f"return_pitch has {len(return_pitch)} entries, the batch has {len(utterances)} utterances")
            tracks = [_check_pitch(w, f"utterance {i}: ") for i, w in enumerate(return_pitch)]
        else:
            tracks = [_check_pitch(return_pitch)] * len(utterances)
        self.pitch = self.pitches = None
        if any(t is not None for t in tracks):
            self.pitches = [Pitch(u[3], len(u[0]), t) if t is not None else None for t, u in zip(tracks, utterances)]
            self.pitch = (PitchC * len(utterances))(*[p.struct if p is not None else PitchC() for p in self.pitches])
        if isinstance(return_contour, (list, tuple)):
            if len(return_contour) != len(utterances):
                raise ValueError(f"return_contour has {len(return_contour)} entries, the batch has {len(utterances)} utterances")
            wishes = [_check_contour(w, f"utterance {i}: ") for i, w in enumerate(return_contour)]
        else:
            wishes = [_check_contour(return_contour)] * len(utterances)
        self.contour = self.contours = None
        if any(f or p for f, p in wishes):
            self.contours = [Contour(u[3], len(u[0]), f, p) if f or p else None for (f, p), u in zip(wishes, utterances)]
            self.contour = (ContourC * len(utterances))(*[c.struct if c is not None else ContourC() for c in self.contours])
        self.envelope = self.ekeep = None
        if envelope is not None:
            envs = list(envelope)
            if len(envs) != len(utterances):
                raise ValueError(f"envelope has {len(envs)} entries, the batch has {len(utterances)} utterances")
            self.ekeep = [_envelope(e, len(u[0]), f"utterance {i}: ") for i, (e, u) in enumerate(zip(envs, utterances))]
            self.envelope = (EnvelopeC * len(utterances))(*[e.struct if e is not None else EnvelopeC() for e in self.ekeep])
        self.return_levels = _check_levels(return_levels)
        self.volume = self.levels = None
        if volume is not None:
            vols = list(volume)
            if len(vols) != len(utterances):
                raise ValueError(f"volume has {len(vols)} entries, the batch has {len(utterances)} utterances")
            vols = [_volume(v, f"utterance {i}: ") for i, v in enumerate(vols)]
            self.volume = (Volume * len(utterances))(*[v if v is not None else Volume() for v in vols])
        if self.volume is not None or self.return_levels:
            self.levels = (Level * len(utterances))()
        tgs = [_check_target(u[6], u[3]) if len(u) > 6 else None for u in utterances]
        self.targets = None
        if any(t is not None for t in tgs):
            self.targets = (C.c_uint32 * len(utterances))(*[t or 0 for t in tgs])
        self.model = model
        n = self.n = len(utterances)
        self.keep, self.wavs = [], []
        P = C.c_void_p * n
        self.ids_p, self.pun_p, self.sty_p, self.wav_p = P(), P(), P(), P()
        self.Ns, self.Ts, self.nf = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_uint32 * n)()
        prs = [_prosody(u[4]) if len(u) > 4 else None for u in utterances]
        self.prosody = None
        if any(p is not None for p in prs):
            self.prosody = (Prosody * n)(*[p if p is not None else Prosody() for p in prs])
        for i, (ids, puncts, style, T) in enumerate(u[:4] for u in utterances):
            a = np.ascontiguousarray(ids, dtype=np.int32)
            b = np.ascontiguousarray(puncts, dtype=np.int32)
            c = np.ascontiguousarray(style, dtype=np.float32)
            w = np.zeros(T * model.hp.audio_hop_size, np.float32)
            self.keep += [a, b, c]
            self.wavs.append(w)
            self.ids_p[i], self.pun_p[i], self.sty_p[i], self.wav_p[i] = a.ctypes.data, b.ctypes.data, c.ctypes.data, w.ctypes.data
            self.Ns[i], self.Ts[i] = len(a), T
        pcs = [_phoneme_controls(u[5], len(u[0])) if len(u) > 5 else None for u in utterances]
        self.phonemes = self.durations = self.dur_p = None
        self.pkeep = pcs
        if durations or any(p is not None for p in pcs):
            self.phonemes = (PhonemeControlsC * n)(*[p.struct if p is not None else PhonemeControlsC() for p in pcs])
            self.durations = [np.zeros(int(self.Ns[i]), np.int32) for i in range(n)]
            self.dur_p = P(*[d.ctypes.data for d in self.durations])

    def set_phoneme_controls(self, i: int, controls):
        """utterance i's per-phoneme controls (PhonemeControls, dict of arrays or None) for the following run() / begin() (the call
        must have been built with per-phoneme controls or durations=True)"""
        if self.phonemes is None:
            raise ValueError("this BatchCall was built without per-phoneme controls")
        pc = _phoneme_controls(controls, int(self.Ns[i]))
        self.pkeep[i] = pc
        self.phonemes[i] = pc.struct if pc is not None else PhonemeControlsC()

    def set_target_frames(self, i: int, frames):
        """utterance i's target frame count (0 / None: none) for the following run() / begin() (the call must have been built with a
        target on some utterance)"""
        if self.targets is None:
            raise ValueError("this BatchCall was built without target frame counts")
        self.targets[i] = _check_target(frames, int(self.Ts[i])) or 0

    def set_volume(self, i: int, volume):
        """utterance i's volume (None: the identity) for the following run() / begin() (the call must have been built with volume=)"""
        if self.volume is None:
            raise ValueError("this BatchCall was built without volume controls")
        self.volume[i] = _volume(volume, f"utterance {i}: ") or Volume()

    def set_envelope(self, i: int, envelope):
        """utterance i's envelope (None: the identity) for the following run() / begin() (the call must have been built with envelope=)"""
        if self.envelope is None:
            raise ValueError("this BatchCall was built without envelopes")
        e = _envelope(envelope, int(self.Ns[i]), f"utterance {i}: ")
        self.ekeep[i] = e
        self.envelope[i] = e.struct if e is not None else EnvelopeC()

    def set_pitch(self, i: int, return_pitch):
        """utterance i's pitch request (False / None: none) for the following run() / begin() (the call must have been built with
        return_pitch=); .pitches[i] is replaced"""
        if self.pitch is None:
            raise ValueError("this BatchCall was built without a pitch track")
        t = _check_pitch(False if return_pitch is None else return_pitch, f"utterance {i}: ")
        self.pitches[i] = Pitch(int(self.Ts[i]), int(self.Ns[i]), t) if t is not None else None
        self.pitch[i] = self.pitches[i].struct if t is not None else PitchC()

    def set_bands(self, i: int, return_bands):
        """utterance i's band request (False / None: none) for the following run() / begin() (the call must have been built with
        return_bands=); .bands[i] is replaced"""
        if self.band is None:
            raise ValueError("this BatchCall was built without band levels")
        t = _check_bands(False if return_bands is None else return_bands, f"utterance {i}: ")
        self.bands[i] = Bands(int(self.Ts[i]), int(self.Ns[i]), t) if t is not None else None
        self.band[i] = self.bands[i].struct if t is not None else BandsC()

    def set_filter(self, i: int, filter):
        """utterance i's filter (a Filter, a sequence of taps or None: none) for the following run() / begin() (the call must have been
        built with filter=)"""
        if self.filter is None:
            raise ValueError("this BatchCall was built without filters")
        self.fkeep[i] = _filter(filter, f"utterance {i}: ")
        self.filter[i] = self.fkeep[i].struct if self.fkeep[i] is not None else FilterC()

    def set_prosody(self, i: int, prosody):
        """utterance i's controls for the following run() / begin() (the call must have been built with controls)"""
        if self.prosody is None:
            raise ValueError("this BatchCall was built without prosody controls")
        self.prosody[i] = _prosody(prosody) or Prosody()

    def run(self):
        m = self.model
        args = (m.h, self.n, self.ids_p, self.pun_p, self.sty_p, self.Ns, self.Ts, self.wav_p, self.nf)
        m._chk(_call_variant(m.lib, "zv_synthesize_batch", args, self.prosody, self.phonemes, self.dur_p, self.fitted, self.targets,
                             self.volume, self.levels, self.envelope, self.contour, self.pitch, self.band, self.filter))

    def begin(self, lane: int):
        """zv_synthesize_batch_begin on `lane`: returns once everything is enqueued; results are valid after end(lane)"""
        m = self.model
        args = (m.h, lane, self.n, self.ids_p, self.pun_p, self.sty_p, self.Ns, self.Ts, self.wav_p, self.nf)
        m._chk(_call_variant(m.lib, "zv_synthesize_batch_begin", args, self.prosody, self.phonemes, self.dur_p, self.fitted, self.targets,
                             self.volume, self.levels, self.envelope, self.contour, self.pitch, self.band, self.filter))

    def end(self, lane: int):
        m = self.model
        m._chk(m.lib.zv_synthesize_batch_end(m.h, lane))

    def results(self):
        return [(self.wavs[i], int(self.nf[i])) for i in range(self.n)]


def demo_utterance():
    """(ids[120], puncts[120], style[528]) of the reference's ZeroVOXModel::eval() (needs no GPU)"""
    lib = load_library()
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    n, ns = C.c_uint32(0), C.c_uint32(0)
    lib.zv_demo_utterance(C.byref(a), C.byref(b), C.byref(c), C.byref(n), C.byref(ns))
    ids = np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_int32)), shape=(n.value,)).copy()
    pun = np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_int32)), shape=(n.value,)).copy()
    sty = np.ctypeslib.as_array(C.cast(c, C.POINTER(C.c_float)), shape=(ns.value,)).copy()
    return ids, pun, sty


def gguf_inspect(path: str, tensor_index: int = -1):
    """(n_tensors, max_seq_len[, name, ggml_type, ne]) as parsed by the product's C++ GGUF reader (no GPU needed)."""
    lib = load_library()
    n, T, typ = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    name = C.create_string_buffer(64)
    ne = (C.c_int64 * 4)()
    st = lib.zv_gguf_inspect(path.encode(), C.byref(n), C.byref(T), tensor_index, name, C.byref(typ), ne)
    if st != 0:
        raise ZvError(st, lib.zv_last_error().decode())
    if tensor_index < 0:
        return n.value, T.value
    return n.value, T.value, name.value.decode(), typ.value, list(ne)


def write_wav(path: str, wav: np.ndarray, sampling_rate: int):
    lib = load_library()
    wav = np.ascontiguousarray(wav, dtype=np.float32)
    st = lib.zv_write_wav(path.encode(), _ptr(wav), wav.size, sampling_rate)
    if st != 0:
        raise ZvError(st, lib.zv_last_error().decode())
