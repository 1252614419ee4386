"""ctypes binding of libzerovox_amd.so (the C-ABI of include/zerovox_amd.h).

Used by the parity tests, bench.py and smoke(): the same entry points a C/C++ host would call.
There is NO CPU fallback: if the library is missing or no gfx950 device is present, loading fails.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Callable, NamedTuple, Optional

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
    "zv_set_graph_cache", "zv_graph_cache_stats",
    "zv_encode_batch", "zv_decode_batch", "zv_vocode_batch", "zv_vocode_batch_begin", "zv_vocode_batch_end",
    "zv_mel_wave", "zv_mel_wave_batch", "zv_mel_design",
    "zv_mel_align", "zv_mel_align_batch", "zv_align_durations",
    "zv_loudness_wave", "zv_loudness_wave_batch", "zv_loudness_design",
    "zv_limit_wave", "zv_limit_wave_batch", "zv_limit_design",
    "zv_resample_wave", "zv_resample_wave_batch", "zv_resample_design", "zv_resample_count", "zv_write_wav_pcm16",
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


class PitchC(C.Structure):
    """zv_pitch of include/zerovox_amd.h: the two tables' pointers, zv_pitch_frame [T] and zv_pitch_phoneme [n], each or NULL, and the
    parameters, 0 = default (a zeroed struct asks for nothing)"""
    _fields_ = [("frames", C.c_void_p), ("phonemes", C.c_void_p), ("min_lag", C.c_uint32), ("max_lag", C.c_uint32),
                ("window", C.c_uint32), ("voiced_threshold", C.c_float)]


class BandsC(C.Structure):
    """zv_bands of include/zerovox_amd.h: the two tables' pointers, float [T][n_bands] and [n][n_bands], each or NULL, the band count
    (0 = 16) and the edges' pointer, uint32 [n_bands + 1] or NULL = the default edges (a zeroed struct asks for nothing)"""
    _fields_ = [("frames", C.c_void_p), ("phonemes", C.c_void_p), ("n_bands", C.c_uint32), ("edges", C.c_void_p)]


class _Tables:
    """What Contour, Pitch and Bands share: .frames float32 [T, width] and .phonemes float32 [n, width] of the waveform the same call
    returned, None for a table that was not asked for; .struct is the subclass's C struct, which points into the arrays (kept alive
    here) and carries the subclass's parameters behind the two pointers.  dbfs() converts levels to dB re full scale (0 -> -inf)."""
    STRUCT = None

    def __init__(self, T: int, n: int, width: int, frames: bool, phonemes: bool):
        self.frames = np.zeros((T, width), np.float32) if frames else None
        self.phonemes = np.zeros((n, width), np.float32) if phonemes else None

    def _struct_params(self) -> tuple:
        return ()

    @property
    def struct(self):
        return self.STRUCT(None if self.frames is None else self.frames.ctypes.data,
                           None if self.phonemes is None else self.phonemes.ctypes.data, *self._struct_params())

    @staticmethod
    def dbfs(levels) -> np.ndarray:
        """20 * log10(level), full scale = 1.0; -inf for a level of 0"""
        a = np.asarray(levels, dtype=np.float64)
        with np.errstate(divide="ignore"):
            return 20.0 * np.log10(a)

    def __repr__(self):
        shape = lambda a: None if a is None else a.shape
        return f"{type(self).__name__}(frames={shape(self.frames)}, phonemes={shape(self.phonemes)})"


class Contour(_Tables):
    """An utterance's level contour (include/zerovox_amd.h "level contour"): the tables' columns are (rms, peak)"""
    STRUCT = ContourC
    CHOICES = (False, True, "frames", "phonemes")

    def __init__(self, T: int, n: int, frames: bool = True, phonemes: bool = True):
        super().__init__(T, n, 2, frames, phonemes)


class _BothTables:
    """what a contour is asked for: which tables, and no parameters"""

    def __init__(self, frames: bool = True, phonemes: bool = True):
        self.frames, self.phonemes = frames, phonemes


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


class Pitch(_Tables):
    """An utterance's pitch track: the columns of .frames are (f0_hz, strength), those of .phonemes (mean f0_hz of the voiced frames,
    share of voiced frames).  .params is the PitchTrack."""
    STRUCT = PitchC

    def __init__(self, T: int, n: int, params: PitchTrack):
        self.params = params
        super().__init__(T, n, 2, params.frames, params.phonemes)

    def _struct_params(self):
        p = self.params
        return p.min_lag, p.max_lag, p.window, p.voiced_threshold


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


class Bands(_Tables):
    """An utterance's band levels: a table's row holds the level (RMS re full scale) of each band.  .params is the BandLevels; .edges
    the bins in force (the struct points into the edges too, which .params keeps alive)."""
    STRUCT = BandsC

    def __init__(self, T: int, n: int, params: BandLevels):
        self.params = params
        super().__init__(T, n, params.width, params.frames, params.phonemes)

    @property
    def edges(self) -> np.ndarray:
        return np.asarray(BandLevels.DEFAULT_EDGES, np.uint32) if self.params.edges is None else self.params.edges

    def _struct_params(self):
        p = self.params
        return p.n_bands, None if p.edges is None else p.edges.ctypes.data


def _check_tables(keyword: str, params_cls, wish, where: str = ""):
    """a table request (the value of `keyword`) -> a params_cls or None (nothing asked for), checked before anything reaches the
    library: False, True (both tables, default parameters), "frames", "phonemes" or, unless params_cls is _BothTables, a params_cls"""
    kinds = "'frames' or 'phonemes'" if params_cls is _BothTables else f"'frames', 'phonemes' or a {params_cls.__name__}"
    if isinstance(wish, params_cls):
        return wish if wish.frames or wish.phonemes else None
    if isinstance(wish, (bool, np.bool_)):
        return params_cls() if wish else None
    if isinstance(wish, str):
        if wish in ("frames", "phonemes"):
            return params_cls(frames=wish == "frames", phonemes=wish == "phonemes")
        raise ValueError(f"{where}{keyword} = {wish!r}: expected False, True, {kinds}")
    raise TypeError(f"{where}{keyword} must be a bool, {kinds}, not {type(wish).__name__}")


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


class MelC(C.Structure):
    """zv_mel of include/zerovox_amd.h: the weights' pointer, float [num_mels * 513] or NULL = the design, and the scalars (a zeroed
    struct is Slaney 0 .. Nyquist, centre 0, zero padding, log10, floor 1e-10)"""
    _fields_ = [("weights", C.c_void_p), ("fmin_hz", C.c_float), ("fmax_hz", C.c_float), ("centre", C.c_uint32), ("pad", C.c_uint32),
                ("log", C.c_uint32), ("floor", C.c_float)]


class MelAnalysis:
    """The parameters of mel analysis (include/zerovox_amd.h "mel analysis"): .weights float32 [num_mels, 513] or None (the design
    from fmin_hz .. fmax_hz, 0 = Nyquist), centre (the sample of a hop a frame is centred on: 0 is librosa's center=True, hop // 2
    the band levels' spans), pad ("zero" or "reflect", or 0 / 1), log ("log10", "ln" or "linear", or 0 / 1 / 2), floor (0 = 1e-10).
    The library checks the values.  .struct is the zv_mel, which points into the weights (kept alive here)."""
    PADS = {"zero": 0, "reflect": 1}
    LOGS = {"log10": 0, "ln": 1, "linear": 2}
    BINS = 513

    def __init__(self, weights=None, fmin_hz: float = 0.0, fmax_hz: float = 0.0, centre: int = 0, pad=0, log=0, floor: float = 0.0):
        self.weights = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.ndim != 2 or w.shape[1] != self.BINS:
                raise ValueError(f"MelAnalysis weights must be [num_mels, {self.BINS}], got shape {w.shape}")
            self.weights = w
        if isinstance(pad, str) and pad not in self.PADS:
            raise ValueError(f"MelAnalysis pad = {pad!r}: expected 'zero' or 'reflect'")
        if isinstance(log, str) and log not in self.LOGS:
            raise ValueError(f"MelAnalysis log = {log!r}: expected 'log10', 'ln' or 'linear'")
        self.fmin_hz, self.fmax_hz, self.floor = float(fmin_hz), float(fmax_hz), float(floor)
        self.centre = int(centre)
        self.pad = self.PADS[pad] if isinstance(pad, str) else int(pad)
        self.log = self.LOGS[log] if isinstance(log, str) else int(log)

    @property
    def struct(self) -> MelC:
        return MelC(None if self.weights is None else self.weights.ctypes.data, self.fmin_hz, self.fmax_hz, self.centre, self.pad,
                    self.log, self.floor)

    def __repr__(self):
        return (f"MelAnalysis(weights={None if self.weights is None else self.weights.shape}, fmin_hz={self.fmin_hz}, fmax_hz={self.fmax_hz}, "
                f"centre={self.centre}, pad={self.pad}, log={self.log}, floor={self.floor})")


def _mel_params(who: str, params, num_mels: int) -> MelAnalysis:
    """params= of the mel calls -> a MelAnalysis, checked before anything reaches the library"""
    if params is None:
        return MelAnalysis()
    if not isinstance(params, MelAnalysis):
        raise TypeError(f"{who}: params must be a MelAnalysis or None, not {type(params).__name__}")
    if params.weights is not None and params.weights.shape[0] != num_mels:
        raise ValueError(f"{who}: the weights have {params.weights.shape[0]} rows, the model has {num_mels} mel channels")
    return params


def mel_design(sampling_rate: int, num_mels: int, fmin_hz: float = 0.0, fmax_hz: float = 0.0, lib=None) -> np.ndarray:
    """zv_mel_design: Slaney mel weights float32 [num_mels, 513] on the bins of the 1 024-point DFT; fmax_hz 0 = Nyquist.  Host only:
    no model, no device."""
    lib = lib or load_library()
    for name, v in (("sampling_rate", sampling_rate), ("num_mels", num_mels)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 0xffffffff:
            raise ValueError(f"mel_design: {name} = {v!r} must be an integer in [0, 4294967295]")
    w = np.zeros((min(max(int(num_mels), 1), 256), MelAnalysis.BINS), np.float32)
    st = lib.zv_mel_design(int(sampling_rate), int(num_mels), float(fmin_hz), float(fmax_hz), _ptr(w))
    if st != 0:
        raise ZvError(st, lib.zv_last_error().decode("utf-8", "replace"))
    return w


class AlignC(C.Structure):
    """zv_align of include/zerovox_amd.h (a zeroed struct is scale 64 without normalisation)"""
    _fields_ = [("scale", C.c_float), ("normalise", C.c_uint32)]


class AlignmentC(C.Structure):
    """zv_alignment of include/zerovox_amd.h"""
    _fields_ = [("total", C.c_uint64), ("distance", C.c_double), ("path_len", C.c_uint32), ("reserved", C.c_uint32)]


class AlignParams:
    """The parameters of mel alignment (include/zerovox_amd.h "mel alignment"): scale (the quantiser's steps per unit of the rows,
    0 = 64) and normalise (remove every channel's mean per sequence: a recording's gain and fixed channel response).  The library
    checks the values."""
    MAX_FRAMES = 4096

    def __init__(self, scale: float = 0.0, normalise=False):
        self.scale = float(scale)
        self.normalise = int(normalise)

    @property
    def struct(self) -> AlignC:
        return AlignC(self.scale, self.normalise & 0xffffffff)

    def __repr__(self):
        return f"AlignParams(scale={self.scale}, normalise={self.normalise})"


class Alignment:
    """What mel alignment returns: total (the path's summed integer cost), distance (the mean Euclidean distance per path cell, in the
    rows' own unit), path_len, map_a int32 [Ta] (the first frame of b on the path in each row of a) and map_b int32 [Tb]"""

    def __init__(self, total: int, distance: float, path_len: int, map_a, map_b):
        self.total, self.distance, self.path_len, self.map_a, self.map_b = int(total), float(distance), int(path_len), map_a, map_b

    def __repr__(self):
        return f"Alignment(total={self.total}, distance={self.distance!r}, path_len={self.path_len}, Ta={len(self.map_a)}, Tb={len(self.map_b)})"


def _align_params(who: str, params) -> AlignParams:
    if params is None:
        return AlignParams()
    if not isinstance(params, AlignParams):
        raise TypeError(f"{who}: params must be an AlignParams or None, not {type(params).__name__}")
    return params


def _mel_rows(who: str, rows) -> np.ndarray:
    r = np.ascontiguousarray(rows, dtype=np.float32)
    if r.ndim != 2:
        raise ValueError(f"{who}: the rows must be a 2-D array [frames, channels], got shape {r.shape}")
    return r


def align_durations(durations_a, map_a, Tb: int, lib=None) -> np.ndarray:
    """zv_align_durations, the timing transfer: the frames per phoneme of sequence a and the map of its alignment against a sequence
    of Tb frames -> the frames per phoneme on that sequence's clock, int32 [n], which sum to Tb.  Host only: no model, no device."""
    lib = lib or load_library()
    fn = _stage_symbol(lib, "zv_align_durations")
    da = np.ascontiguousarray(durations_a, dtype=np.int32)
    ma = np.ascontiguousarray(map_a, dtype=np.int32)
    if da.ndim != 1 or ma.ndim != 1:
        raise ValueError(f"align_durations: durations_a and map_a must be 1-D, got shapes {da.shape} and {ma.shape}")
    if isinstance(Tb, (bool, np.bool_)) or not isinstance(Tb, (int, np.integer)) or not 0 <= Tb <= 0xffffffff:
        raise ValueError(f"align_durations: Tb = {Tb!r} must be an integer in [0, 4294967295]")
    db = np.zeros(da.size, np.int32)
    st = fn(da.size, _ptr(da), ma.size, _ptr(ma), int(Tb), _ptr(db))
    if st != 0:
        raise ZvError(st, lib.zv_last_error().decode("utf-8", "replace"))
    return db


class LoudnessC(C.Structure):
    """zv_loudness of include/zerovox_amd.h (the identity is {1, 0, 0, 0})"""
    _fields_ = [("gain", C.c_float), ("target_lufs", C.c_float), ("true_peak_ceiling", C.c_float), ("flags", C.c_uint32)]


class LoudnessResultC(C.Structure):
    """zv_loudness_result of include/zerovox_amd.h"""
    _fields_ = [("integrated_ms", C.c_double), ("momentary_max_ms", C.c_double), ("short_term_max_ms", C.c_double), ("true_peak", C.c_double),
                ("blocks", C.c_uint32), ("blocks_absolute", C.c_uint32), ("blocks_gated", C.c_uint32), ("sample_peak", C.c_float),
                ("integrated_lufs", C.c_float), ("momentary_max_lufs", C.c_float), ("short_term_max_lufs", C.c_float),
                ("true_peak_dbtp", C.c_float), ("gain", C.c_float), ("reserved", C.c_uint32)]


class LoudnessFilterC(C.Structure):
    """zv_loudness_filter of include/zerovox_amd.h"""
    _fields_ = [("shelf_b", C.c_double * 3), ("shelf_a", C.c_double * 2), ("highpass_b", C.c_double * 3), ("highpass_a", C.c_double * 2),
                ("M", C.c_double * 16), ("interp", C.c_float * 49), ("step", C.c_uint32)]


class Loudness:
    """What a loudness call asks for (include/zerovox_amd.h "loudness"): a linear gain, a target in LUFS (None: none) and a true-peak
    ceiling, linear in (0, 1] (None: none).  from_lufs takes the ceiling in dBTP.  The library checks the values."""
    TARGET, CEILING = 1, 2

    def __init__(self, gain: float = 1.0, target_lufs=None, true_peak_ceiling=None):
        self.gain = float(gain)
        self.target_lufs = None if target_lufs is None else float(target_lufs)
        self.true_peak_ceiling = None if true_peak_ceiling is None else float(true_peak_ceiling)

    @classmethod
    def from_lufs(cls, target: float, true_peak_dbtp=None, gain: float = 1.0):
        """-16 LUFS under -1 dBTP: Loudness.from_lufs(-16.0, true_peak_dbtp=-1.0); the ceiling becomes float32(10^(dBTP / 20))"""
        return cls(gain, target, None if true_peak_dbtp is None else float(np.float32(10.0 ** (float(true_peak_dbtp) / 20.0))))

    @property
    def struct(self) -> LoudnessC:
        flags = (self.TARGET if self.target_lufs is not None else 0) | (self.CEILING if self.true_peak_ceiling is not None else 0)
        return LoudnessC(self.gain, self.target_lufs or 0.0, self.true_peak_ceiling or 0.0, flags)

    def __repr__(self):
        return f"Loudness(gain={self.gain}, target_lufs={self.target_lufs}, true_peak_ceiling={self.true_peak_ceiling})"


class LoudnessResult:
    """What a loudness call measured: the float64 mean squares (integrated_ms, momentary_max_ms, short_term_max_ms), true_peak (linear,
    float64), the block counts (blocks, blocks_absolute, blocks_gated), sample_peak and the four readings as float32
    (integrated_lufs, momentary_max_lufs, short_term_max_lufs, true_peak_dbtp), and the gain that was applied"""
    FIELDS = tuple(n for n, _ in LoudnessResultC._fields_ if n != "reserved")

    def __init__(self, c: LoudnessResultC):
        for n in self.FIELDS:
            v = getattr(c, n)
            setattr(self, n, np.float32(v) if dict(LoudnessResultC._fields_)[n] is C.c_float else v)

    def __repr__(self):
        return "LoudnessResult(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.FIELDS) + ")"


class LoudnessFilter:
    """zv_loudness_design's result: shelf_b, shelf_a, highpass_b, highpass_a and M (row major, 16) as lists of floats, c float32 [49]
    (the interpolator) and step"""

    def __init__(self, c: LoudnessFilterC):
        self.shelf_b, self.shelf_a, self.highpass_b, self.highpass_a, self.M = (list(getattr(c, n)) for n in
                                                                                 ("shelf_b", "shelf_a", "highpass_b", "highpass_a", "M"))
        self.c = np.array(list(c.interp), np.float32)
        self.step = int(c.step)


def loudness_design(sampling_rate: int, lib=None) -> LoudnessFilter:
    """zv_loudness_design: the K-weighting biquads, the gating step, M = A^256 and the true-peak interpolator for a sampling rate.
    Host only: no model, no device."""
    lib = lib or load_library()
    fn = _stage_symbol(lib, "zv_loudness_design")
    if isinstance(sampling_rate, (bool, np.bool_)) or not isinstance(sampling_rate, (int, np.integer)) or not 0 <= sampling_rate <= 0xffffffff:
        raise ValueError(f"loudness_design: sampling_rate = {sampling_rate!r} must be an integer in [0, 4294967295]")
    out = LoudnessFilterC()
    st = fn(int(sampling_rate), C.byref(out))
    if st != 0:
        raise ZvError(st, lib.zv_last_error().decode("utf-8", "replace"))
    return LoudnessFilter(out)


def _loudness_ask(who: str, ask):
    if ask is not None and not isinstance(ask, Loudness):
        raise TypeError(f"{who}: ask must be a Loudness or None, not {type(ask).__name__}")
    return ask


class LimiterC(C.Structure):
    """zv_limiter of include/zerovox_amd.h"""
    _fields_ = [("gain", C.c_float), ("ceiling", C.c_float), ("attack", C.c_uint32), ("release", C.c_uint32), ("flags", C.c_uint32)]


class LimitResultC(C.Structure):
    """zv_limit_result of include/zerovox_amd.h"""
    _fields_ = [("true_peak_before", C.c_double), ("true_peak_after", C.c_double), ("limited_samples", C.c_uint64),
                ("sample_peak_before", C.c_float), ("sample_peak_after", C.c_float), ("min_gain", C.c_float),
                ("true_peak_before_dbtp", C.c_float), ("true_peak_after_dbtp", C.c_float), ("reduction_db", C.c_float)]


def limit_design(sampling_rate: int, attack_ms: float = 0.0, release_ms: float = 0.0, lib=None):
    """zv_limit_design: (attack, release) in samples for milliseconds at a sampling rate; 0 ms means the default (1.5 ms, 60 ms).
    Host only: no model, no device."""
    lib = lib or load_library()
    fn = _stage_symbol(lib, "zv_limit_design")
    if isinstance(sampling_rate, (bool, np.bool_)) or not isinstance(sampling_rate, (int, np.integer)) or not 0 <= sampling_rate <= 0xffffffff:
        raise ValueError(f"limit_design: sampling_rate = {sampling_rate!r} must be an integer in [0, 4294967295]")
    a, r = C.c_uint32(), C.c_uint32()
    st = fn(int(sampling_rate), float(attack_ms), float(release_ms), C.byref(a), C.byref(r))
    if st != 0:
        raise ZvError(st, lib.zv_last_error().decode("utf-8", "replace"))
    return int(a.value), int(r.value)


class Limiter:
    """What a limiter call asks for (include/zerovox_amd.h "limiter"): a linear gain applied ahead of the limiter, a linear ceiling in
    (0, 1], and the attack and release in samples.  from_dbtp takes the ceiling in dBTP, the gain in dB and the windows in milliseconds
    at a sampling rate.  The library checks the values."""

    def __init__(self, gain: float, ceiling: float, attack: int, release: int):
        self.gain, self.ceiling, self.attack, self.release = float(gain), float(ceiling), int(attack), int(release)

    @classmethod
    def from_dbtp(cls, dbtp: float, gain_db: float = 0.0, attack_ms: float = 0.0, release_ms: float = 0.0, sampling_rate: int = 0, lib=None):
        """-1 dBTP behind +6 dB at 22 050 Hz: Limiter.from_dbtp(-1.0, gain_db=6.0, sampling_rate=22050); ceiling and gain become
        float32(10^(dB / 20)), the windows limit_design's counts (0 ms: the defaults)"""
        a, r = limit_design(sampling_rate, attack_ms, release_ms, lib)
        return cls(float(np.float32(10.0 ** (float(gain_db) / 20.0))), float(np.float32(10.0 ** (float(dbtp) / 20.0))), a, r)

    @property
    def struct(self) -> LimiterC:
        if not (0 <= self.attack <= 0xffffffff and 0 <= self.release <= 0xffffffff):
            raise ValueError(f"Limiter: attack = {self.attack} and release = {self.release} must fit 32 bits")
        return LimiterC(self.gain, self.ceiling, self.attack, self.release, 0)

    def __repr__(self):
        return f"Limiter(gain={self.gain}, ceiling={self.ceiling}, attack={self.attack}, release={self.release})"


class LimitResult:
    """What a limiter call reports: true_peak_before and true_peak_after (linear, float64), limited_samples, and as float32
    sample_peak_before, sample_peak_after, min_gain, true_peak_before_dbtp, true_peak_after_dbtp and reduction_db"""
    FIELDS = tuple(n for n, _ in LimitResultC._fields_)

    def __init__(self, c: LimitResultC):
        for n in self.FIELDS:
            v = getattr(c, n)
            setattr(self, n, np.float32(v) if dict(LimitResultC._fields_)[n] is C.c_float else v)

    def __repr__(self):
        return "LimitResult(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.FIELDS) + ")"


def _limit_ask(who: str, ask):
    if ask is not None and not isinstance(ask, Limiter):
        raise TypeError(f"{who}: ask must be a Limiter or None, not {type(ask).__name__}")
    return ask


class ResampleC(C.Structure):
    """zv_resample of include/zerovox_amd.h"""
    _fields_ = [("rate_in", C.c_uint32), ("rate_out", C.c_uint32), ("zeros", C.c_uint32), ("beta", C.c_float), ("cutoff", C.c_float),
                ("table", C.c_void_p), ("L", C.c_uint32), ("M", C.c_uint32), ("P", C.c_uint32), ("flags", C.c_uint32), ("seed", C.c_uint32)]


class ResampleResultC(C.Structure):
    """zv_resample_result of include/zerovox_amd.h"""
    _fields_ = [("n_out", C.c_uint64), ("clipped", C.c_uint64), ("sample_peak", C.c_float)]


def _u32_arg(who: str, name: str, v) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 0xffffffff:
        raise ValueError(f"{who}: {name} = {v!r} must be an integer in [0, 4294967295]")
    return int(v)


def resample_design(rate_in: int, rate_out: int, zeros: int = 0, beta: float = 0.0, cutoff: float = 0.0, lib=None):
    """zv_resample_design: (L, M, the table float32 [L, P]) of a Kaiser-windowed sinc for rate_in -> rate_out; 0 means the default
    (zeros 32, beta 9, cutoff 0.91).  Host only: no model, no device."""
    lib = lib or load_library()
    fn = _stage_symbol(lib, "zv_resample_design")
    args = [_u32_arg("resample_design", n, v) for n, v in (("rate_in", rate_in), ("rate_out", rate_out), ("zeros", zeros))] + [float(beta), float(cutoff)]
    L, M, P = C.c_uint32(), C.c_uint32(), C.c_uint32()
    for table in (None, True):
        if table:
            table = np.empty((L.value, P.value), np.float32)
        st = fn(*args, C.byref(L), C.byref(M), C.byref(P), _ptr(table))
        if st != 0:
            raise ZvError(st, lib.zv_last_error().decode("utf-8", "replace"))
    return int(L.value), int(M.value), table


def resample_count(S_in: int, L: int, M: int, lib=None) -> int:
    """zv_resample_count: the outputs of S_in input samples under the ratio L / M"""
    lib = lib or load_library()
    return int(_stage_symbol(lib, "zv_resample_count")(int(S_in), _u32_arg("resample_count", "L", L), _u32_arg("resample_count", "M", M)))


class Resample:
    """What a resampling call asks for (include/zerovox_amd.h "resampling"): either the design of (rate_in, rate_out, zeros, beta,
    cutoff; 0: the default), or a caller's table float32 [L, P] with its M; dither: TPDF dither of the PCM16 output under `seed`.  The
    library checks the values."""

    def __init__(self, rate_in: int = 0, rate_out: int = 0, zeros: int = 0, beta: float = 0.0, cutoff: float = 0.0, table=None, M: int = 0,
                 dither: bool = False, seed: int = 0, flags=None):
        self.rate_in, self.rate_out, self.zeros, self.beta, self.cutoff = rate_in, rate_out, zeros, float(beta), float(cutoff)
        self.table = None if table is None else np.ascontiguousarray(table, dtype=np.float32)
        if self.table is not None and self.table.ndim != 2:
            raise ValueError(f"Resample: the table must be [L, P], got shape {self.table.shape}")
        self.M, self.seed = M, seed
        self.flags = (1 if dither else 0) if flags is None else flags

    @property
    def ratio(self):
        """(L, M) of the ask: the table's, or the rates' in lowest terms"""
        if self.table is not None:
            return int(self.table.shape[0]), int(self.M)
        g = int(np.gcd(int(self.rate_in), int(self.rate_out))) or 1
        return int(self.rate_out) // g, int(self.rate_in) // g

    @property
    def struct(self) -> ResampleC:
        u = lambda n, v: _u32_arg("Resample", n, v)
        L, P = (0, 0) if self.table is None else self.table.shape
        return ResampleC(u("rate_in", self.rate_in), u("rate_out", self.rate_out), u("zeros", self.zeros), self.beta, self.cutoff,
                         None if self.table is None else self.table.ctypes.data, u("L", L), u("M", self.M), u("P", P), u("flags", self.flags),
                         u("seed", self.seed))

    def __repr__(self):
        what = f"{self.rate_in} -> {self.rate_out}, zeros={self.zeros}, beta={self.beta}, cutoff={self.cutoff}" if self.table is None else \
            f"table {self.table.shape}, M={self.M}"
        return f"Resample({what}, flags={self.flags}, seed={self.seed})"


class ResampleResult:
    """What a resampling call reports: n_out, clipped (0 where no PCM16 was asked for) and sample_peak (float32)"""
    FIELDS = ("n_out", "clipped", "sample_peak")

    def __init__(self, c: ResampleResultC):
        self.n_out, self.clipped, self.sample_peak = int(c.n_out), int(c.clipped), np.float32(c.sample_peak)

    def __repr__(self):
        return "ResampleResult(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.FIELDS) + ")"


def _resample_ask(who: str, ask):
    if not isinstance(ask, Resample):
        raise TypeError(f"{who}: ask must be a Resample, not {type(ask).__name__}")
    return ask


def _samples(who: str, wav):
    """a waveform of any length in samples, float32 [S]"""
    w = np.ascontiguousarray(wav, dtype=np.float32)
    if w.ndim != 1:
        raise ValueError(f"{who}: the waveform must be a 1-D array, got shape {w.shape}")
    return w


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


class GraphStats(C.Structure):
    """zv_graph_stats: the captured-graph cache since the model was loaded.  lookups = hits + captures, and captures = entries +
    evictions + stale_evictions + lane_drops + full_drops (the last two count graphs, not drops)."""
    _fields_ = [("capacity", C.c_uint32), ("entries", C.c_uint32), ("retired", C.c_uint32), ("reserved", C.c_uint32),
                ("lookups", C.c_uint64), ("hits", C.c_uint64), ("captures", C.c_uint64), ("evictions", C.c_uint64),
                ("stale_evictions", C.c_uint64), ("lane_drops", C.c_uint64), ("full_drops", C.c_uint64)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}

    def __repr__(self):
        return "GraphStats(" + ", ".join(f"{k}={v}" for k, v in self.as_dict().items()) + ")"


class ZvError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"zv_status {status}: {msg}")
        self.status = status


class Form(NamedTuple):
    suffix: str         # appended to the entry point's name
    args: tuple         # the arguments the rung adds: (keyword of _call_variant, ctype of the single call, ctype of the batch calls)
    selects: tuple      # the keywords that select the rung


# The ladder of entry-point forms, lowest rung first.  A form takes the arguments of every rung up to itself, NULL / 0 for what the
# call lacks, and the forms agree bit for bit on those.  A call goes to the highest rung one of whose selecting arguments is not
# None: _prosody with prosody controls; _phonemes with per-phoneme controls or a buffer for the phoneme timings; _target with a frame
# count the durations are fitted to (single call: a uint32, 0 = none; batches: uint32 [n_utt] or NULL), which is also where the
# `fitted` flag becomes an argument; _volume with volumes or a buffer for the levels; _envelope, _contour, _pitch, _bands and
# _filter each with its struct (batches: an array [n_utt]).  _fitted is the one irregular form: it adds nothing to the _phonemes list,
# and a call goes there when `fitted` is set and nothing from _target upward is present.
_P, _vp, _u32 = C.POINTER, C.c_void_p, C.c_uint32
FORMS = (
    Form("_prosody", (("prosody", _P(Prosody), _P(Prosody)),), ("prosody",)),
    Form("_phonemes", (("phonemes", _P(PhonemeControlsC), _P(PhonemeControlsC)), ("durations", _vp, _P(_vp))), ("phonemes", "durations")),
    Form("_fitted", (), ()),
    Form("_target", (("target", _u32, _P(_u32)), ("fitted", C.c_int, C.c_int)), ("target",)),
    Form("_volume", (("volume", _P(Volume), _P(Volume)), ("levels", _P(Level), _P(Level))), ("volume", "levels")),
    Form("_envelope", (("envelope", _P(EnvelopeC), _P(EnvelopeC)),), ("envelope",)),
    Form("_contour", (("contour", _P(ContourC), _P(ContourC)),), ("contour",)),
    Form("_pitch", (("pitch", _P(PitchC), _P(PitchC)),), ("pitch",)),
    Form("_bands", (("bands", _P(BandsC), _P(BandsC)),), ("bands",)),
    Form("_filter", (("filter", _P(FilterC), _P(FilterC)),), ("filter",)),
)
# entry point -> (the plain form's argtypes, the column of Form.args that holds its ctypes, its rungs).  zv_encode_taps has three
# rungs, and its _target adds the count alone
LADDERS = {
    "zv_synthesize": ([_vp, _vp, _vp, _vp, _u32, _u32, _vp, _P(_u32)], 1, FORMS),
    "zv_synthesize_batch": ([_vp, _u32, _P(_vp), _P(_vp), _P(_vp), _P(_u32), _P(_u32), _P(_vp), _P(_u32)], 2, FORMS),
    "zv_synthesize_batch_begin": ([_vp, _u32, _u32, _P(_vp), _P(_vp), _P(_vp), _P(_u32), _P(_u32), _P(_vp), _P(_u32)], 2, FORMS),
    "zv_encode_taps": ([_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _P(_u32), _vp, _vp, _vp, _vp, _vp, _vp], 1,
                       FORMS[:2] + (FORMS[3]._replace(args=FORMS[3].args[:1]),)),
}


def _select(forms, given: dict):
    """the walk of the ladder: (suffix, trailing arguments) of the form a call with the `given` arguments (keyword -> value) goes to"""
    for top in range(len(forms) - 1, -1, -1):
        form = forms[top]
        if given["fitted"] if form.suffix == "_fitted" else any(given[k] is not None for k in form.selects):
            return form.suffix, tuple(int(given[k]) if k == "fitted" else given[k] for f in forms[:top + 1] for k, *_ in f.args)
    return "", ()


_lib = None


def load_library(path: Optional[str] = None):
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ZvError(-1, f"{p} not found: build it with `make -C zerovox.cpp_amd/csrc` (no CPU fallback exists)")
    lib = C.CDLL(p)
    _bind(lib)
    if path is None:
        _lib = lib
    _forward_env_switches(lib)
    return lib


def _bind(lib):
    """argtypes / restype of every entry point `lib` carries (a CDLL, or any object with the symbols as attributes): every form of
    LADDERS from the table, the rest written out.  The suffixed forms and the entry points of the second loop are bound where
    present: an older build named by ZEROVOX_AMD_LIB for an A/B run may lack the upper ones, and a call that needs one then fails
    with AttributeError; build() checks SYMBOLS on the tree's own library."""
    vp, u32, i32p, fp = C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p
    pvp, pu32 = C.POINTER(vp), C.POINTER(u32)
    lib.zv_last_error.restype = C.c_char_p
    lib.zv_version.restype = C.c_char_p
    lib.zv_model_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    lib.zv_model_free.argtypes = [vp]
    lib.zv_model_free.restype = None
    lib.zv_model_get_hparams.argtypes = [vp, C.POINTER(HParams)]
    lib.zv_model_reserve.argtypes = [vp, u32, u32]
    lib.zv_encode.argtypes = [vp, i32p, i32p, fp, u32, u32, fp, C.POINTER(u32)]
    for name, (plain, column, forms) in LADDERS.items():
        getattr(lib, name).argtypes = argtypes = list(plain)
        for form in forms:
            argtypes = argtypes + [arg[column] for arg in form.args]
            if hasattr(lib, name + form.suffix):
                getattr(lib, name + form.suffix).argtypes = argtypes
    lib.zv_debug_layer.argtypes = [vp, C.c_int, C.c_int, fp, u32, fp, fp]
    lib.zv_debug_set.argtypes = [C.c_char_p, C.c_int]
    lib.zv_debug_get.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    lib.zv_batch_timeline.argtypes = [vp, u32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u32)]
    lib.zv_max_frames.argtypes = [vp]
    lib.zv_max_frames.restype = u32
    lib.zv_demo_utterance.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]
    lib.zv_demo_utterance.restype = None
    lib.zv_decode.argtypes = [vp, fp, fp, u32, fp]
    lib.zv_vocode.argtypes = [vp, fp, u32, fp]
    lib.zv_synthesize_batch_end.argtypes = [vp, u32]
    for name, argtypes in (("zv_debug_mfma_chain", [vp, C.c_int, vp, vp, fp, u32, fp]),
                           ("zv_debug_voc_runs", [vp, u32, vp, u32, C.POINTER(u32)]),
                           ("zv_debug_poison", [vp, u32, C.c_int, C.POINTER(C.c_size_t)]),
                           ("zv_pitch_track", [vp, vp, u32, C.POINTER(PitchC)]),
                           ("zv_band_levels", [vp, vp, u32, C.POINTER(BandsC)]),
                           ("zv_filter_wave", [vp, vp, u32, C.POINTER(FilterC), vp]),
                           ("zv_filter_design", [u32, vp, vp, u32, vp]),
                           ("zv_set_graph_cache", [vp, u32]),
                           ("zv_graph_cache_stats", [vp, C.POINTER(GraphStats)]),
                           ("zv_encode_batch", [vp, u32, pvp, pvp, pvp, pu32, pu32, pvp, pu32, C.POINTER(Prosody), C.POINTER(PhonemeControlsC),
                                                pvp, pu32]),
                           ("zv_decode_batch", [vp, u32, pvp, pvp, pu32, pvp]),
                           ("zv_vocode_batch", [vp, u32, pvp, pu32, pvp]),
                           ("zv_vocode_batch_begin", [vp, u32, u32, pvp, pu32, pvp]),
                           ("zv_vocode_batch_end", [vp, u32]),
                           ("zv_mel_wave", [vp, fp, u32, C.POINTER(MelC), fp]),
                           ("zv_mel_wave_batch", [vp, u32, pvp, pu32, C.POINTER(MelC), pvp]),
                           ("zv_mel_design", [u32, u32, C.c_float, C.c_float, fp]),
                           ("zv_mel_align", [vp, fp, u32, fp, u32, u32, C.POINTER(AlignC), C.POINTER(AlignmentC), vp, vp]),
                           ("zv_mel_align_batch", [vp, u32, pvp, pu32, pvp, pu32, u32, C.POINTER(AlignC), C.POINTER(AlignmentC), pvp, pvp]),
                           ("zv_align_durations", [u32, vp, u32, vp, u32, vp]),
                           ("zv_loudness_wave", [vp, fp, u32, u32, C.POINTER(LoudnessC), C.POINTER(LoudnessResultC), fp]),
                           ("zv_loudness_wave_batch", [vp, u32, pvp, pu32, pu32, C.POINTER(LoudnessC), C.POINTER(LoudnessResultC), pvp]),
                           ("zv_loudness_design", [u32, C.POINTER(LoudnessFilterC)]),
                           ("zv_limit_wave", [vp, fp, u32, u32, C.POINTER(LimiterC), C.POINTER(LimitResultC), fp]),
                           ("zv_limit_wave_batch", [vp, u32, pvp, pu32, pu32, C.POINTER(LimiterC), C.POINTER(LimitResultC), pvp]),
                           ("zv_limit_design", [u32, C.c_float, C.c_float, pu32, pu32]),
                           ("zv_resample_wave", [vp, fp, C.c_uint64, C.POINTER(ResampleC), C.POINTER(ResampleResultC), fp, vp]),
                           ("zv_resample_wave_batch", [vp, u32, pvp, C.POINTER(C.c_uint64), C.POINTER(ResampleC), C.POINTER(ResampleResultC), pvp, pvp]),
                           ("zv_resample_design", [u32, u32, u32, C.c_float, C.c_float, pu32, pu32, pu32, fp]),
                           ("zv_resample_count", [C.c_uint64, u32, u32]),
                           ("zv_write_wav_pcm16", [C.c_char_p, vp, C.c_size_t, u32])):
        if hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    if hasattr(lib, "zv_resample_count"):
        lib.zv_resample_count.restype = C.c_uint64
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
    """a struct, or a holder with one in .struct, by reference; None -> NULL"""
    return None if x is None else C.byref(getattr(x, "struct", x))


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
    """entry point `name` in the form the ladder gives for what the call has (its own rungs in LADDERS, else all of FORMS); its
    status"""
    given = dict(prosody=prosody, phonemes=phonemes, durations=durations, fitted=fitted, target=target, volume=volume, levels=levels,
                 envelope=envelope, contour=contour, pitch=pitch, bands=bands, filter=filter)
    suffix, tail = _select(LADDERS[name][2] if name in LADDERS else FORMS, given)
    return getattr(lib, name + suffix)(*args, *tail)


class Option(NamedTuple):
    """one per-utterance option of synthesize / BatchCall"""
    keyword: str            # the keyword that carries it (for the first three: the name of the utterance tuple's element)
    struct: type            # what the C call reads; struct() is "nothing asked for" / the identity
    check: Callable         # (wish, n phonemes, T, where) -> the checked wish, None: nothing asked for
    hold: Callable          # (checked wish, n phonemes, T) -> the holder: the struct itself, or an object whose .struct is it
    batch_wide: bool        # one wish may stand for the whole batch (else: a list with one per utterance)
    array: str              # BatchCall's attribute for the ctypes array, None: built without
    keep: Optional[str]     # BatchCall's attribute for the list of holders the array points into
    without: str = ""       # set_*: "this BatchCall was built without ..."

    def holder(self, wish, n: int, T: int, where: str = ""):
        checked = self.check(wish, n, T, where)
        return None if checked is None else self.hold(checked, n, T)

    def c(self, holder):
        """the struct of a holder, None: the zeroed one"""
        return self.struct() if holder is None else getattr(holder, "struct", holder)


_as_checked = lambda checked, n, T: checked
PROSODY = Option("prosody", Prosody, lambda w, n, T, where: _prosody(w), _as_checked, False, "prosody", None, "prosody controls")
PHONEMES = Option("phonemes", PhonemeControlsC, lambda w, n, T, where: _phoneme_controls(w, n), _as_checked, False, "phonemes", "pkeep",
                  "per-phoneme controls")
TARGET = Option("target_frames", C.c_uint32, lambda w, n, T, where: _check_target(w, T), _as_checked, False, "targets", None,
                "target frame counts")
VOLUME = Option("volume", Volume, lambda w, n, T, where: _volume(w, where), _as_checked, False, "volume", None, "volume controls")
ENVELOPE = Option("envelope", EnvelopeC, lambda w, n, T, where: _envelope(w, n, where), _as_checked, False, "envelope", "ekeep", "envelopes")
CONTOUR = Option("return_contour", ContourC, lambda w, n, T, where: _check_tables("return_contour", _BothTables, w, where),
                 lambda c, n, T: Contour(T, n, c.frames, c.phonemes), True, "contour", "contours")
PITCH = Option("return_pitch", PitchC, lambda w, n, T, where: _check_tables("return_pitch", PitchTrack, w, where),
               lambda c, n, T: Pitch(T, n, c), True, "pitch", "pitches", "a pitch track")
BANDS = Option("return_bands", BandsC, lambda w, n, T, where: _check_tables("return_bands", BandLevels, w, where),
               lambda c, n, T: Bands(T, n, c), True, "band", "bands", "band levels")
FILTER = Option("filter", FilterC, lambda w, n, T, where: _filter(w, where), _as_checked, False, "filter", "fkeep", "filters")


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


def _stage_symbol(lib, name: str):
    """a stage-batch entry point of `lib`; an older library without it fails that call alone, naming the symbol"""
    fn = getattr(lib, name, None)
    if fn is None:
        raise AttributeError(f"the library has no {name}: it is older than the stage-batch calls")
    return fn


def _waveform(hop: int, who: str, wav):
    """a waveform the caller brings, float32 [T * hop] at the model's rate and hop -> (the array, T)"""
    w = np.ascontiguousarray(wav, dtype=np.float32)
    if w.ndim != 1 or w.size == 0 or w.size % hop:
        raise ValueError(f"{who}: the waveform must be a non-empty 1-D array of a multiple of {hop} samples, got shape {w.shape}")
    return w, w.size // hop


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
        zv_encode_taps in the form FORMS gives for what the call has.  prosody: a Prosody, dict or 5-sequence.  phonemes (a
        PhonemeControls or dict of arrays [len(ids)]) or return_durations: the result gains "durations" (the phoneme timings, int32
        [len(ids)]).  target_frames (0 <= frames <= T): the durations are fitted to sum to exactly that many frames (0: the bits of
        the call without it)"""
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
        self._chk(_call_variant(self.lib, "zv_encode_taps", args, _ref(_prosody(prosody)), _ref(pc),
                                _ptr(out.get("durations")), target=target))
        out["n_frames"] = int(nf.value)
        return out

    def synthesize(self, ids, puncts, style, T: int, prosody=None, phonemes=None, return_durations: bool = False,
                   fitted: bool = False, target_frames: Optional[int] = None, *, volume=None, return_levels: bool = False,
                   envelope=None, return_contour=False, return_pitch=False, return_bands=False, filter=None):
        """zv_synthesize in the form FORMS gives for what the call has -> (wav, n_frames), then what the return_* arguments add.
        prosody: a Prosody, dict or 5-sequence.  phonemes: a PhonemeControls or dict of arrays [len(ids)].  return_durations adds the
        phoneme timings (int32 [len(ids)]) as a third element.  fitted: T is a capacity, the utterance is decoded and vocoded as the
        n_frames the length regulator fills; wav keeps the capacity shape [T * hop], zero behind n_frames * hop.
        target_frames (0 <= frames <= T): the durations are fitted to sum to exactly that many frames (0: the bits of the call
        without it).
        volume (Volume, dict or (gain, target_rms, peak_ceiling)): the waveform is measured and scaled on the device; return_levels
        adds the Level (rms and peak before the gain, the gain) as the last element.
        envelope (Envelope or dict of its fields): per-phoneme gains, cross-fades and fades, applied on the device ahead of the volume.
        return_contour (False, True, "frames" or "phonemes"), return_pitch (those, or a PitchTrack), return_bands (those, or a
        BandLevels): the level and peak, the fundamental frequency and voicing, the level per frequency band of every frame and / or
        every phoneme of the returned waveform, metered on the device; each adds its Contour, Pitch, Bands as the last element.
        filter (a Filter, a sequence of taps or None): a linear-phase FIR applied to the waveform on the device, ahead of envelope,
        volume and all meters"""
        # every argument is checked before T sizes a buffer or the model is touched; the tables are built behind the checks
        stages = (FILTER, CONTOUR, PITCH, BANDS)
        asked = [opt.check(wish, None, T, "") for opt, wish in zip(stages, (filter, return_contour, return_pitch, return_bands))]
        fitted = _check_fitted(fitted, [T])
        target = TARGET.check(target_frames, None, T, "")
        vol, return_levels = VOLUME.check(volume, None, T, ""), _check_levels(return_levels)
        env = ENVELOPE.check(envelope, len(ids), T, "")
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        puncts = np.ascontiguousarray(puncts, dtype=np.int32)
        style = np.ascontiguousarray(style, dtype=np.float32)
        wav = np.empty(T * self.hp.audio_hop_size, np.float32)
        nf = C.c_uint32(0)
        n = len(ids)
        args = (self.h, _ptr(ids), _ptr(puncts), _ptr(style), n, T, _ptr(wav), C.byref(nf))
        pc = PHONEMES.check(phonemes, n, T, "")
        dur = np.empty(n, np.int32) if return_durations else None
        level = Level() if vol is not None or return_levels else None
        flt, contour, pitch, bands = (None if a is None else opt.hold(a, n, T) for opt, a in zip(stages, asked))
        held = (vol, level, env, contour, pitch, bands, flt)
        if target is None and any(h is not None for h in held):
            target = 0                       # every form above _target takes the count, 0 = none
        self._chk(_call_variant(self.lib, "zv_synthesize", args, _ref(_prosody(prosody)), _ref(pc), _ptr(dur), fitted, target,
                                *map(_ref, held)))
        out = (wav, int(nf.value), dur) if return_durations else (wav, int(nf.value))
        out = out + (level,) if return_levels else out
        return out + tuple(h for h in (contour, pitch, bands) if h is not None)

    def filter_wave(self, wav, filter) -> np.ndarray:
        """zv_filter_wave: the waveform through the filter (a Filter or a sequence of taps) on the device; returns the filtered waveform"""
        flt = _filter(filter)
        if flt is None:
            raise TypeError("filter_wave: filter must be a Filter or a sequence of taps, not None")
        w, T = _waveform(self.hp.audio_hop_size, "filter_wave", wav)
        out = np.empty_like(w)
        st = flt.struct
        self._chk(self.lib.zv_filter_wave(self.h, _ptr(w), T, C.byref(st), _ptr(out)))
        return out

    def band_levels(self, wav, params=None) -> Bands:
        """zv_band_levels: the band levels of the waveform, frames only; params: a BandLevels or None (the default bands)"""
        if params is not None and not isinstance(params, BandLevels):
            raise TypeError(f"band_levels: params must be a BandLevels or None, not {type(params).__name__}")
        p = params or BandLevels()
        spec = BandLevels(p.n_bands if p.edges is None else 0, p.edges, True, False)      # a waveform has no timings
        w, T = _waveform(self.hp.audio_hop_size, "band_levels", wav)
        bands = Bands(T, 0, spec)
        st = bands.struct
        self._chk(self.lib.zv_band_levels(self.h, _ptr(w), T, C.byref(st)))
        return bands

    def mel_wave(self, wav, params=None) -> np.ndarray:
        """zv_mel_wave: the log-mel rows [T][num_mels] of the waveform (the vocoder's input domain); params: a MelAnalysis or None
        (Slaney weights 0 .. Nyquist, centre 0, zero padding, log10, floor 1e-10)"""
        fn = _stage_symbol(self.lib, "zv_mel_wave")
        p = _mel_params("mel_wave", params, self.hp.audio_num_mels)
        w, T = _waveform(self.hp.audio_hop_size, "mel_wave", wav)
        out = np.empty((T, self.hp.audio_num_mels), np.float32)
        st = p.struct
        self._chk(fn(self.h, _ptr(w), T, C.byref(st), _ptr(out)))
        return out

    def mel_wave_batch(self, wavs, params=None) -> list:
        """zv_mel_wave_batch: waveforms [T_u * hop], one per utterance, through ONE launch per kernel -> the list of rows
        [T_u][num_mels], each with the bits of its mel_wave; params serves the whole batch"""
        fn = _stage_symbol(self.lib, "zv_mel_wave_batch")
        p = _mel_params("mel_wave_batch", params, self.hp.audio_num_mels)
        ws = [_waveform(self.hp.audio_hop_size, f"mel_wave_batch: utterance {u}", w) for u, w in enumerate(wavs)]
        n = len(ws)
        outs = [np.empty((T, self.hp.audio_num_mels), np.float32) for _, T in ws]
        P = C.c_void_p * n
        st = p.struct
        self._chk(fn(self.h, n, P(*[w.ctypes.data for w, _ in ws]), (C.c_uint32 * n)(*[T for _, T in ws]), C.byref(st),
                     P(*[o.ctypes.data for o in outs])))
        return outs

    def loudness_wave(self, wav, ask=None, n_frames=None, apply=True):
        """zv_loudness_wave: the BS.1770 loudness and the true peak of the waveform's first n_frames frames (None: all of it) and the
        whole waveform scaled by one gain -> (LoudnessResult, float32 [T * hop]); ask: a Loudness or None (the identity);
        apply=False meters only -> (LoudnessResult, None)"""
        fn = _stage_symbol(self.lib, "zv_loudness_wave")
        q = _loudness_ask("loudness_wave", ask)
        w, T = _waveform(self.hp.audio_hop_size, "loudness_wave", wav)
        out = np.empty_like(w) if apply else None
        res = LoudnessResultC()
        st = q.struct if q is not None else None
        self._chk(fn(self.h, _ptr(w), T, T if n_frames is None else int(n_frames), C.byref(st) if q is not None else None, C.byref(res),
                     _ptr(out) if apply else None))
        return LoudnessResult(res), out

    def loudness_wave_batch(self, wavs, asks=None, n_frames=None, apply=True):
        """zv_loudness_wave_batch: waveforms [T_u * hop], one per utterance, through ONE launch per kernel per launch group -> the list
        of (LoudnessResult, waveform or None), each with the bits of its loudness_wave; asks: None or one Loudness (or None) per
        utterance; n_frames: None or one count per utterance; apply: a bool, or one per utterance"""
        fn = _stage_symbol(self.lib, "zv_loudness_wave_batch")
        ws = [_waveform(self.hp.audio_hop_size, f"loudness_wave_batch: utterance {u}", w) for u, w in enumerate(wavs)]
        n = len(ws)
        if asks is not None and len(asks) != n:
            raise ValueError(f"loudness_wave_batch: {len(asks)} asks for {n} utterances")
        if n_frames is not None and len(n_frames) != n:
            raise ValueError(f"loudness_wave_batch: {len(n_frames)} frame counts for {n} utterances")
        want = [bool(apply)] * n if isinstance(apply, (bool, np.bool_)) else [bool(a) for a in apply]
        if len(want) != n:
            raise ValueError(f"loudness_wave_batch: {len(want)} apply flags for {n} utterances")
        qs = None
        if asks is not None:
            qs = (LoudnessC * n)(*[(_loudness_ask(f"loudness_wave_batch: utterance {u}", a) or Loudness()).struct for u, a in enumerate(asks)])
        outs = [np.empty_like(w) if a else None for (w, _), a in zip(ws, want)]
        res = (LoudnessResultC * n)()
        P, U = C.c_void_p * n, C.c_uint32 * n
        self._chk(fn(self.h, n, P(*[w.ctypes.data for w, _ in ws]), U(*[T for _, T in ws]),
                     None if n_frames is None else U(*[int(f) for f in n_frames]), qs, res, P(*[None if o is None else o.ctypes.data for o in outs])))
        return [(LoudnessResult(r), o) for r, o in zip(res, outs)]

    def limit_wave(self, wav, ask=None, n_frames=None):
        """zv_limit_wave: the waveform behind the look-ahead peak limiter, its first n_frames frames (None: all of it) measured ->
        (LimitResult, float32 [T * hop]); ask: a Limiter or None (gain 1, ceiling 1, the default windows of the model's rate)"""
        fn = _stage_symbol(self.lib, "zv_limit_wave")
        q = _limit_ask("limit_wave", ask)
        w, T = _waveform(self.hp.audio_hop_size, "limit_wave", wav)
        out = np.empty_like(w)
        res = LimitResultC()
        st = q.struct if q is not None else None
        self._chk(fn(self.h, _ptr(w), T, T if n_frames is None else int(n_frames), C.byref(st) if q is not None else None, C.byref(res), _ptr(out)))
        return LimitResult(res), out

    def limit_wave_batch(self, wavs, asks=None, n_frames=None):
        """zv_limit_wave_batch: waveforms [T_u * hop], one per utterance, through ONE launch per kernel per launch group -> the list of
        (LimitResult, waveform), each with the bits of its limit_wave; asks: None or one Limiter per utterance; n_frames: None or one
        count per utterance"""
        fn = _stage_symbol(self.lib, "zv_limit_wave_batch")
        ws = [_waveform(self.hp.audio_hop_size, f"limit_wave_batch: utterance {u}", w) for u, w in enumerate(wavs)]
        n = len(ws)
        if asks is not None and len(asks) != n:
            raise ValueError(f"limit_wave_batch: {len(asks)} asks for {n} utterances")
        if n_frames is not None and len(n_frames) != n:
            raise ValueError(f"limit_wave_batch: {len(n_frames)} frame counts for {n} utterances")
        qs = None
        if asks is not None:
            if any(a is None for a in asks):
                raise TypeError("limit_wave_batch: asks holds None (give every utterance a Limiter, or asks=None for the identity)")
            qs = (LimiterC * n)(*[_limit_ask(f"limit_wave_batch: utterance {u}", a).struct for u, a in enumerate(asks)])
        outs = [np.empty_like(w) for w, _ in ws]
        res = (LimitResultC * n)()
        P, U = C.c_void_p * n, C.c_uint32 * n
        self._chk(fn(self.h, n, P(*[w.ctypes.data for w, _ in ws]), U(*[T for _, T in ws]),
                     None if n_frames is None else U(*[int(f) for f in n_frames]), qs, res, P(*[o.ctypes.data for o in outs])))
        return [(LimitResult(r), o) for r, o in zip(res, outs)]

    def resample_wave(self, wav, ask, out=True, pcm=False):
        """zv_resample_wave: a waveform of any length in samples at another rate -> (ResampleResult, float32 [n_out] or None, int16
        [n_out] or None); ask: a Resample; out, pcm: which of the two outputs to return (at least one)"""
        fn = _stage_symbol(self.lib, "zv_resample_wave")
        q = _resample_ask("resample_wave", ask)
        w = _samples("resample_wave", wav)
        n = resample_count(w.size, *q.ratio, lib=self.lib) if q.ratio[1] else 0
        o = np.empty(n, np.float32) if out else None
        p = np.empty(n, np.int16) if pcm else None
        res = ResampleResultC()
        self._chk(fn(self.h, _ptr(w), w.size, C.byref(q.struct), C.byref(res), _ptr(o), _ptr(p)))
        assert res.n_out == n, (res.n_out, n)
        return ResampleResult(res), o, p

    def resample_wave_batch(self, wavs, ask, out=True, pcm=False):
        """zv_resample_wave_batch: waveforms of any lengths under ONE ask, one launch per kernel per launch group -> the list of
        (ResampleResult, float32 or None, int16 or None), utterance u with the bits of its resample_wave under seed + u"""
        fn = _stage_symbol(self.lib, "zv_resample_wave_batch")
        q = _resample_ask("resample_wave_batch", ask)
        ws = [_samples(f"resample_wave_batch: utterance {u}", w) for u, w in enumerate(wavs)]
        n = len(ws)
        counts = [resample_count(w.size, *q.ratio, lib=self.lib) if q.ratio[1] else 0 for w in ws]
        outs = [np.empty(c, np.float32) for c in counts] if out else None
        pcms = [np.empty(c, np.int16) for c in counts] if pcm else None
        res = (ResampleResultC * n)()
        P = C.c_void_p * n
        self._chk(fn(self.h, n, P(*[w.ctypes.data for w in ws]), (C.c_uint64 * n)(*[w.size for w in ws]), C.byref(q.struct), res,
                     P(*[o.ctypes.data for o in outs]) if out else None, P(*[p.ctypes.data for p in pcms]) if pcm else None))
        return [(ResampleResult(r), outs[u] if out else None, pcms[u] if pcm else None) for u, r in enumerate(res)]

    def deliver(self, wav, lufs, dbtp, n_frames=None, rate=None, pcm16=False, dither=False):
        """A delivery chain for "lufs LUFS, dbtp dBTP": a target-only loudness meter, the limiter with that gain under the ceiling (the
        default windows), then the meter on the result -> (LoudnessResult before, LimitResult, LoudnessResult after, waveform).
        rate (Hz) and pcm16 add the last step, resample_wave over the limited waveform (the default design; dither: TPDF, seed 0),
        and the tuple gains (ResampleResult, the delivered samples: float32, or int16 where pcm16)"""
        before, _ = self.loudness_wave(wav, Loudness.from_lufs(lufs), n_frames, apply=False)
        a, r = limit_design(self.hp.audio_sampling_rate, lib=self.lib)
        lim, out = self.limit_wave(wav, Limiter(float(before.gain), float(np.float32(10.0 ** (float(dbtp) / 20.0))), a, r), n_frames)
        after, _ = self.loudness_wave(out, None, n_frames, apply=False)
        if rate is None and not pcm16:
            if dither:
                raise ValueError("deliver: dither belongs to pcm16=True")
            return before, lim, after, out
        sr = self.hp.audio_sampling_rate
        rs, f32, i16 = self.resample_wave(out, Resample(sr, sr if rate is None else rate, dither=dither), out=not pcm16, pcm=pcm16)
        return before, lim, after, out, rs, i16 if pcm16 else f32

    def resynthesize(self, wav, params=None) -> np.ndarray:
        """analysis-resynthesis: vocode(mel_wave(wav)), the acceptance check of a converted vocoder checkpoint.  params must keep the
        vocoder's domain (the natural logarithm is what the reference's checkpoints were trained on: pass MelAnalysis(log="ln", ...)
        with the training front end's fmin / fmax / floor where they differ from the defaults)"""
        return self.vocode(self.mel_wave(wav, params))

    def mel_align(self, a, b, params=None) -> Alignment:
        """zv_mel_align: the dynamic-time-warping path between the rows a [Ta][M] and b [Tb][M] (float32, 1 <= M <= 256, at most 4 096
        rows each) -> an Alignment; params: an AlignParams or None (scale 64, no normalisation)"""
        fn = _stage_symbol(self.lib, "zv_mel_align")
        p = _align_params("mel_align", params)
        ra, rb = _mel_rows("mel_align: a", a), _mel_rows("mel_align: b", b)
        if ra.shape[1] != rb.shape[1]:
            raise ValueError(f"mel_align: a has {ra.shape[1]} channels, b has {rb.shape[1]}")
        ma, mb = np.empty(ra.shape[0], np.int32), np.empty(rb.shape[0], np.int32)
        st, out = p.struct, AlignmentC()
        self._chk(fn(self.h, _ptr(ra), ra.shape[0], _ptr(rb), rb.shape[0], ra.shape[1], C.byref(st), C.byref(out), _ptr(ma), _ptr(mb)))
        return Alignment(out.total, out.distance, out.path_len, ma, mb)

    def mel_align_batch(self, pairs, params=None) -> list:
        """zv_mel_align_batch: pairs of rows (a [Ta][M], b [Tb][M]) of one width through ONE launch per kernel per launch group -> the
        list of Alignments, each with the bits of its mel_align; params serves the whole batch"""
        fn = _stage_symbol(self.lib, "zv_mel_align_batch")
        p = _align_params("mel_align_batch", params)
        rows = [(_mel_rows(f"mel_align_batch: pair {k}: a", a), _mel_rows(f"mel_align_batch: pair {k}: b", b)) for k, (a, b) in enumerate(pairs)]
        n = len(rows)
        widths = {r.shape[1] for ab in rows for r in ab}
        if len(widths) > 1:
            raise ValueError(f"mel_align_batch: the rows have different widths: {sorted(widths)}")
        M = widths.pop() if widths else 0
        mas, mbs = [np.empty(a.shape[0], np.int32) for a, _ in rows], [np.empty(b.shape[0], np.int32) for _, b in rows]
        P, U = C.c_void_p * n, C.c_uint32 * n
        st, out = p.struct, (AlignmentC * n)()
        self._chk(fn(self.h, n, P(*[a.ctypes.data for a, _ in rows]), U(*[a.shape[0] for a, _ in rows]), P(*[b.ctypes.data for _, b in rows]),
                     U(*[b.shape[0] for _, b in rows]), M, C.byref(st), out, P(*[x.ctypes.data for x in mas]), P(*[x.ctypes.data for x in mbs])))
        return [Alignment(o.total, o.distance, o.path_len, ma, mb) for o, ma, mb in zip(out, mas, mbs)]

    def synthesize_like(self, ids, puncts, style, T: int, ref_wav, mel=None, align=None, **controls):
        """"say this text with the timing of that take": a fitted synthesis at capacity T gives the model's own waveform and phoneme
        timings; its mel rows and those of ref_wav (cut to whole hops, Tb frames) come from ONE mel_wave_batch (mel: a MelAnalysis,
        default natural-log rows); mel_align (align: an AlignParams, default normalise on) maps the model's frames to the
        reference's; align_durations moves the phoneme boundaries onto the reference's clock; a second fitted synthesis at T = Tb
        with those duration_frames follows it.  controls: what synthesize takes besides return_*, fitted, target_frames and a
        phonemes duration (prosody, phonemes as a dict, volume, envelope, filter).
        -> (wav [Tb * hop], n_frames, durations_b, alignment)"""
        for k in controls:
            if k.startswith("return_") or k in ("fitted", "target_frames"):
                raise TypeError(f"synthesize_like: {k} is not a control of this call")
        ph = controls.pop("phonemes", None)
        if ph is not None and not isinstance(ph, dict):
            raise TypeError(f"synthesize_like: phonemes must be a dict of arrays or None, not {type(ph).__name__}")
        if ph and (ph.get("duration_frames") is not None or ph.get("duration_scale") is not None):
            raise ValueError("synthesize_like: phonemes carries a duration: the reference gives the timing")
        hop = self.hp.audio_hop_size
        ref = np.ascontiguousarray(ref_wav, dtype=np.float32)
        if ref.ndim != 1 or ref.size < hop:
            raise ValueError(f"synthesize_like: ref_wav must be a 1-D array of at least one hop ({hop} samples), got shape {ref.shape}")
        Tb = ref.size // hop
        mel = MelAnalysis(log="ln") if mel is None else mel
        align = AlignParams(normalise=True) if align is None else align
        wav, nf, dur_a = self.synthesize(ids, puncts, style, T, phonemes=ph, return_durations=True, fitted=True, **controls)
        if nf < 1:
            raise ValueError("synthesize_like: the model's own synthesis has no frames")
        rows_a, rows_b = self.mel_wave_batch([wav[:nf * hop], ref[:Tb * hop]], mel)
        alignment = self.mel_align(rows_a, rows_b, align)
        dur_b = align_durations(dur_a, alignment.map_a, Tb, lib=self.lib)
        wav2, nf2, _ = self.synthesize(ids, puncts, style, Tb, phonemes=dict(ph or {}, duration_frames=dur_b), return_durations=True,
                                       fitted=True, **controls)
        return wav2, nf2, dur_b, alignment

    def pitch_track(self, wav, params=None) -> Pitch:
        """zv_pitch_track: the pitch track of the waveform, frames only; params: a PitchTrack or None (the defaults)"""
        if params is not None and not isinstance(params, PitchTrack):
            raise TypeError(f"pitch_track: params must be a PitchTrack or None, not {type(params).__name__}")
        p = params or PitchTrack()
        track = PitchTrack(p.min_lag, p.max_lag, p.window, p.voiced_threshold, True, False)      # a waveform has no timings
        w, T = _waveform(self.hp.audio_hop_size, "pitch_track", wav)
        pitch = Pitch(T, 0, track)
        st = pitch.struct
        self._chk(self.lib.zv_pitch_track(self.h, _ptr(w), T, C.byref(st)))
        return pitch

    def prepare_batch(self, utterances, durations: bool = False, fitted: bool = False, *, volume=None,
                      return_levels: bool = False, envelope=None, return_contour=False, return_pitch=False,
                      return_bands=False, filter=None) -> "BatchCall":
        """argument arrays and output buffers of one zv_synthesize_batch call, built once (a C host would keep its
        buffers too): .run() is exactly one call of the C entry point, .results() the (wav, n_frames) list; the lane form is
        .begin(lane) / .end(lane).  The arguments are BatchCall's"""
        return BatchCall(self, utterances, durations, fitted, volume=volume, return_levels=return_levels, envelope=envelope,
                         return_contour=return_contour, return_pitch=return_pitch, return_bands=return_bands, filter=filter)

    def synthesize_batch(self, utterances, return_durations: bool = False, fitted: bool = False, *, volume=None,
                         return_levels: bool = False, envelope=None, return_contour=False, return_pitch=False, return_bands=False,
                         filter=None):
        """utterances: list of (ids, puncts, style, T[, prosody[, phonemes[, target_frames]]]) -> list of (wav, n_frames); each
        utterance keeps its own (N, T) and, with a fifth element, its own prosody controls (None: identity), with a sixth its
        per-phoneme controls (PhonemeControls, dict of arrays or None), with a seventh its target frame count (None / 0: none).
        return_durations: (wav, n_frames, durations) tuples.  fitted: every T is a capacity, wav keeps the capacity shape with zeros
        behind n_frames * hop.  volume, envelope, filter: a list with one value as synthesize takes it, or None, per utterance.
        return_levels: every tuple gains the utterance's Level as its last element.  return_contour, return_pitch, return_bands: a
        value as synthesize takes it for the whole batch, or a list with one per utterance; every tuple gains the utterance's
        Contour, Pitch, Bands (None where it asked for none) as its last element"""
        call = BatchCall(self, utterances, return_durations, fitted, volume=volume, return_levels=return_levels, envelope=envelope,
                         return_contour=return_contour, return_pitch=return_pitch, return_bands=return_bands, filter=filter)
        call.run()
        res = call.results()
        if return_durations:
            res = [r + (d,) for r, d in zip(res, call.durations)]
        if call.return_levels:
            res = [r + (Level.from_buffer_copy(lv),) for r, lv in zip(res, call.levels)]
        for opt in (CONTOUR, PITCH, BANDS):
            if getattr(call, opt.array) is not None:
                res = [r + (h,) for r, h in zip(res, getattr(call, opt.keep))]
        return res

    # ---- the stages in batches (zv_encode_batch, zv_decode_batch, zv_vocode_batch*) ----
    def encode_batch(self, utterances, return_hidden: bool = True, return_durations: bool = False) -> list:
        """zv_encode_batch: the encoder over a batch.  utterances: the tuples synthesize_batch takes, (ids, puncts, style, T[, prosody
        [, phonemes[, target_frames]]]) -> a list of dicts like encode's: "n_frames", "hidden" [T][E] unless return_hidden is False
        (the planning call: only the frame counts leave the device), "durations" (int32 [len(ids)]) with return_durations or where
        some utterance carries per-phoneme controls"""
        fn = _stage_symbol(self.lib, "zv_encode_batch")
        call = BatchCall(self, utterances, bool(return_durations))
        hidden = [np.empty((int(T), self.E), np.float32) for T in call.Ts] if return_hidden else None
        hid_p = (C.c_void_p * call.n)(*[h.ctypes.data for h in hidden]) if return_hidden else None
        self._chk(fn(self.h, call.n, call.ids_p, call.pun_p, call.sty_p, call.Ns, call.Ts, hid_p, call.nf, call.prosody, call.phonemes,
                     call.dur_p, call.targets))
        out = [dict(n_frames=int(call.nf[i])) for i in range(call.n)]
        for i, d in enumerate(out):
            if return_hidden:
                d["hidden"] = hidden[i]
            if call.durations is not None:
                d["durations"] = call.durations[i]
        return out

    def decode_batch(self, hiddens, styles) -> list:
        """zv_decode_batch: hiddens [T_u][E] and styles [E], one per utterance -> the list of mels [T_u][num_mels]"""
        fn = _stage_symbol(self.lib, "zv_decode_batch")
        hid = [np.ascontiguousarray(h, dtype=np.float32) for h in hiddens]
        sty = [np.ascontiguousarray(s, dtype=np.float32) for s in styles]
        if len(hid) != len(sty):
            raise ValueError(f"decode_batch: {len(hid)} hiddens, {len(sty)} styles")
        n = len(hid)
        mels = [np.empty((h.shape[0], self.hp.audio_num_mels), np.float32) for h in hid]
        P = C.c_void_p * n
        Ts = (C.c_uint32 * n)(*[h.shape[0] for h in hid])
        self._chk(fn(self.h, n, P(*[h.ctypes.data for h in hid]), P(*[s.ctypes.data for s in sty]), Ts, P(*[m.ctypes.data for m in mels])))
        return mels

    @staticmethod
    def _vocode_args(hop: int, mels):
        """(n, the mel pointers, the frame counts, the waveform pointers) of a vocode batch, the mels and the waveforms themselves"""
        mel = [np.ascontiguousarray(m, dtype=np.float32) for m in mels]
        n = len(mel)
        wavs = [np.empty(m.shape[0] * hop, np.float32) for m in mel]
        P = C.c_void_p * n
        return (n, P(*[m.ctypes.data for m in mel]), (C.c_uint32 * n)(*[m.shape[0] for m in mel]), P(*[w.ctypes.data for w in wavs])), mel, wavs

    def vocode_batch(self, mels) -> list:
        """zv_vocode_batch: mels [T_u][num_mels], one per utterance -> the list of waveforms [T_u * hop]"""
        fn = _stage_symbol(self.lib, "zv_vocode_batch")
        args, _mel, wavs = Model._vocode_args(self.hp.audio_hop_size, mels)
        self._chk(fn(self.h, *args))
        return wavs

    def vocode_batch_begin(self, lane: int, mels):
        """zv_vocode_batch_begin on `lane` (one launch group): returns once everything is enqueued; vocode_batch_end(lane) waits and
        returns the waveforms"""
        fn = _stage_symbol(self.lib, "zv_vocode_batch_begin")
        args, mel, wavs = Model._vocode_args(self.hp.audio_hop_size, mels)
        self._chk(fn(self.h, lane, args[0], *args[1:]))
        if not hasattr(self, "_vocode_lanes"):
            self._vocode_lanes = {}
        self._vocode_lanes[lane] = (args, mel, wavs)      # the arrays the library reads and writes until _end

    def vocode_batch_end(self, lane: int) -> list:
        fn = _stage_symbol(self.lib, "zv_vocode_batch_end")
        held = getattr(self, "_vocode_lanes", {})
        self._chk(fn(self.h, lane))
        return held.pop(lane)[2] if lane in held else None

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

    def set_graph_cache(self, capacity: int):
        """zv_set_graph_cache: how many captured graphs the model keeps (1 .. 1024, 16 by default); a smaller capacity evicts the
        least recently used, graphs of an older switch epoch first, and waits for no lane"""
        if not 0 <= int(capacity) <= 0xFFFFFFFF:
            raise ValueError(f"capacity {capacity} is no uint32")
        self._chk(self.lib.zv_set_graph_cache(self.h, int(capacity)))

    def graph_cache_stats(self) -> GraphStats:
        """zv_graph_cache_stats: a GraphStats of the counts since load; waits for nothing"""
        st = GraphStats()
        self._chk(self.lib.zv_graph_cache_stats(self.h, C.byref(st)))
        return st

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
    """The argument arrays and output buffers of one zv_synthesize_batch call.  utterances: (ids, puncts, style, T[, prosody[, phonemes
    [, target_frames]]]) tuples.  Every option (an Option each) has a ctypes array [n_utt] under the Option's .array name, which exists
    when an utterance carries the option (the others get the zeroed struct) and is None otherwise; the form of the entry point
    follows from which arrays exist (FORMS) and is settled here, once.  The set_* methods rewrite an entry in place: the next run() /
    begin() uses the new values with the same buffers (a captured graph replays with them).  An option given as a keyword is one
    wish for the whole batch (the return_* ones only) or a list with one per utterance, None for none.
    .durations[i] holds utterance i's phoneme timings after run() / end() (durations=True, or any per-phoneme controls); .levels every
    utterance's Level (volume or return_levels); .contours[i], .pitches[i] and .bands[i] utterance i's Contour, Pitch and Bands, None
    where it asked for none; .ekeep[i], .fkeep[i] and .pkeep[i] its checked Envelope, Filter and PhonemeControls, whose arrays the
    structs point into.  fitted: every T is a capacity."""

    def __init__(self, model: Model, utterances, durations: bool = False, fitted: bool = False, *, volume=None,
                 return_levels: bool = False, envelope=None, return_contour=False, return_pitch=False, return_bands=False, filter=None):
        element = lambda k: [u[k] if len(u) > k else None for u in utterances]
        self.fitted = _check_fitted(fitted, [u[3] for u in utterances])
        for opt, wish in ((FILTER, filter), (BANDS, return_bands), (PITCH, return_pitch), (CONTOUR, return_contour), (ENVELOPE, envelope)):
            self._build(opt, wish, utterances, wish is not None and not opt.batch_wide)
        self.return_levels = _check_levels(return_levels)
        self._build(VOLUME, volume, utterances, volume is not None)
        self.levels = (Level * len(utterances))() if self.volume is not None or self.return_levels else None
        self._build(TARGET, element(6), utterances)
        self.model = model
        n = self.n = len(utterances)
        self.keep, self.wavs = [], []
        P = C.c_void_p * n
        self.ids_p, self.pun_p, self.sty_p, self.wav_p = P(), P(), P(), P()
        self.Ns, self.Ts, self.nf = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_uint32 * n)()
        self._build(PROSODY, element(4), utterances)
        for i, (ids, puncts, style, T) in enumerate(u[:4] for u in utterances):
            a = np.ascontiguousarray(ids, dtype=np.int32)
            b = np.ascontiguousarray(puncts, dtype=np.int32)
            c = np.ascontiguousarray(style, dtype=np.float32)
            w = np.zeros(T * model.hp.audio_hop_size, np.float32)
            self.keep += [a, b, c]
            self.wavs.append(w)
            self.ids_p[i], self.pun_p[i], self.sty_p[i], self.wav_p[i] = a.ctypes.data, b.ctypes.data, c.ctypes.data, w.ctypes.data
            self.Ns[i], self.Ts[i] = len(a), T
        self._build(PHONEMES, element(5), utterances, durations)
        self.pkeep = self.pkeep or [None] * n
        self.durations = self.dur_p = None
        if self.phonemes is not None:
            self.durations = [np.zeros(int(self.Ns[i]), np.int32) for i in range(n)]
            self.dur_p = P(*[d.ctypes.data for d in self.durations])
        # the per-step path walks no table: the symbols and the argument tuple of run() and begin(), settled once
        suffix, tail = _select(FORMS, dict(prosody=self.prosody, phonemes=self.phonemes, durations=self.dur_p, fitted=self.fitted,
                                           target=self.targets, volume=self.volume, levels=self.levels, envelope=self.envelope,
                                           contour=self.contour, pitch=self.pitch, bands=self.band, filter=self.filter))
        self._run, self._begin = "zv_synthesize_batch" + suffix, "zv_synthesize_batch_begin" + suffix
        self._args = (self.ids_p, self.pun_p, self.sty_p, self.Ns, self.Ts, self.wav_p, self.nf) + tail

    def _build(self, opt: Option, wish, utterances, always: bool = False):
        """opt's array and holders: from one wish for the whole batch or a list with one per utterance, each checked; the array exists
        when an utterance asks for something, or `always`"""
        n, holders = len(utterances), None
        if isinstance(wish, (list, tuple)) if opt.batch_wide else wish is not None:
            wish = list(wish)
            if len(wish) != n:
                raise ValueError(f"{opt.keyword} has {len(wish)} entries, the batch has {n} utterances")
            holders = [opt.holder(w, len(u[0]), u[3], f"utterance {i}: ") for i, (w, u) in enumerate(zip(wish, utterances))]
        elif opt.batch_wide:
            checked = opt.check(wish, 0, 0, "")
            holders = [None if checked is None else opt.hold(checked, len(u[0]), u[3]) for u in utterances]
        exists = holders is not None and (always or any(h is not None for h in holders))
        setattr(self, opt.array, (opt.struct * n)(*[opt.c(h) for h in holders]) if exists else None)
        if opt.keep:
            setattr(self, opt.keep, holders if exists else None)

    def _set(self, opt: Option, i: int, wish):
        """utterance i's entry of opt's array, and its holder, for the following run() / begin()"""
        array = getattr(self, opt.array)
        if array is None:
            raise ValueError(f"this BatchCall was built without {opt.without}")
        holder = opt.holder(wish, int(self.Ns[i]), int(self.Ts[i]), f"utterance {i}: ")
        if opt.keep:
            getattr(self, opt.keep)[i] = holder
        array[i] = opt.c(holder)

    def set_phoneme_controls(self, i: int, controls):
        """utterance i's per-phoneme controls (PhonemeControls, dict of arrays or None); needs a call built with per-phoneme controls
        or durations=True"""
        self._set(PHONEMES, i, controls)

    def set_target_frames(self, i: int, frames):
        """utterance i's target frame count (0 / None: none); needs a call built with a target on some utterance"""
        self._set(TARGET, i, frames)

    def set_volume(self, i: int, volume):
        """utterance i's volume (None: the identity); needs a call built with volume="""
        self._set(VOLUME, i, volume)

    def set_envelope(self, i: int, envelope):
        """utterance i's envelope (None: the identity); needs a call built with envelope="""
        self._set(ENVELOPE, i, envelope)

    def set_pitch(self, i: int, return_pitch):
        """utterance i's pitch request (False / None: none); needs a call built with return_pitch=; .pitches[i] is replaced"""
        self._set(PITCH, i, False if return_pitch is None else return_pitch)

    def set_bands(self, i: int, return_bands):
        """utterance i's band request (False / None: none); needs a call built with return_bands=; .bands[i] is replaced"""
        self._set(BANDS, i, False if return_bands is None else return_bands)

    def set_filter(self, i: int, filter):
        """utterance i's filter (a Filter, a sequence of taps or None: none); needs a call built with filter="""
        self._set(FILTER, i, filter)

    def set_prosody(self, i: int, prosody):
        """utterance i's controls (None: the identity); needs a call built with controls"""
        self._set(PROSODY, i, prosody)

    def run(self):
        m = self.model
        m._chk(getattr(m.lib, self._run)(m.h, self.n, *self._args))

    def begin(self, lane: int):
        """zv_synthesize_batch_begin on `lane`: returns once everything is enqueued; results are valid after end(lane)"""
        m = self.model
        m._chk(getattr(m.lib, self._begin)(m.h, lane, self.n, *self._args))

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


def write_wav_pcm16(path: str, pcm: np.ndarray, sampling_rate: int):
    """zv_write_wav_pcm16: int16 samples as they are, a mono RIFF/WAVE file"""
    lib = load_library()
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    st = _stage_symbol(lib, "zv_write_wav_pcm16")(path.encode(), _ptr(pcm), pcm.size, sampling_rate)
    if st != 0:
        raise ZvError(st, lib.zv_last_error().decode())


def write_wav(path: str, wav: np.ndarray, sampling_rate: int):
    lib = load_library()
    wav = np.ascontiguousarray(wav, dtype=np.float32)
    st = lib.zv_write_wav(path.encode(), _ptr(wav), wav.size, sampling_rate)
    if st != 0:
        raise ZvError(st, lib.zv_last_error().decode())
