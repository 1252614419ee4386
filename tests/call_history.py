"""History independence over every entry point: the generator of a call history, its coverage counts and the runner.

history(seed, steps) is a pure function (numpy only): a list of steps, each a state change or a call key.  A call key is a hashable
tuple that determines the call completely (op, sizes, seeds, an index into MENU, the fixed menu of per-utterance asks); run() rebuilds
the inputs from it with synth.encoder_inputs / vocoder_mel / decoder_hidden and a seeded waveform.  A state change is one of
("graph", on), ("cache", capacity), ("reserve", N, T), ("poison", byte, lane).

The call keys:
  ("vocode", T, seed)  ("stream", T, seed, chunk)  ("decode", T, seed)  ("encode", N, T, seed)          the old single calls
  ("synth", N, T, seed, entry, fitted)                                                                  synthesize with MENU[entry]
  ("batch", form, lane, fitted, utts)     utts = ((N, T, seed, entry), ...); form "sync": synthesize_batch, "lane": begin / end on lane
  ("pair", order, fitted0, utts0, fitted1, utts1)     two batches in flight on lanes 0 and 1, ended in `order`
  ("encode_batch", hidden, utts)  ("decode_batch", ((T, seed), ...))  ("vocode_batch", ((T, seed), ...))
  ("vocode_batch_lane", ((T, seed), ...), inner)      vocode_batch_begin(1), the lane-0 call `inner`, vocode_batch_end(1)
  ("filter_wave", T, seed, taps)  ("band_levels", T, seed, custom)  ("pitch_track", T, seed, explicit)
  ("mel_wave", T, seed, variant)  ("mel_wave_batch", ((T, seed), ...), variant)  ("resynth", T, seed)
  ("vocode_device", T, seed)  ("decode_device", T, seed)

Collisions are made, not hoped for: after a synth, batch or pair step the next step is, with probability 1/3, the same shape with
other asks (same sizes, seeds, form, lane and fitted flag, every utterance another MENU entry), with probability 1/6 the identical key
once more, and with probability 1/6 an analysis call followed by the identical key (a "sandwich").  No state change falls inside such
a succession, so both of its steps run in one graph mode on one lane.  Ops, MENU entries, lanes and cache capacities are dealt from
shuffled decks (every card once per deal), the cache capacity changes at six set places, graph mode goes off for 4 to 9 steps at a
time, and three reserves that exceed everything before them are set early, so that the counts test_call_history_cpu.py asks for do
not hang on the luck of one seed.

parts(key) names what a call is compared with: the canonical keys of its parts, each the same work as ONE synchronous lane-0 call (a
batch begun on a lane is its synthesize_batch, a pair is its two batches, a vocode batch on lane 1 is its vocode_batch and the inner
call).  run_parts(model, key, ctx) makes the call and returns one flat list of arrays per part; the project promises their equality
bit for bit whatever the model has done before, which same() checks with no tolerance."""
import numpy as np

HOP, NUM_MELS, BINS = 300, 80, 513                 # the "small" synthetic checkpoint; 513: the samples a reflect pad needs
TS = (1, 7, 33, 64, 100, 160, 250)                 # frame capacities and phoneme counts: the pools of test_gpu_state_machine.py
NS = (1, 5, 24, 40, 77)
CACHES = (1, 2, 16)
STEPS = 400                                        # the length of the history test_gpu_call_history.py walks
RESERVES = tuple((n, t) for n, t in zip(NS, TS)) + ((77, 250), (256, 512))
MENU = ("nothing", "everything", "mixed", "volume", "filter1", "filter255", "prosody", "phonemes", "target")
ENCODER_ENTRIES = (0, 6, 7, 8)                     # what of MENU the encoder alone can be asked
STATE_OPS = ("graph", "cache", "reserve", "poison")
SYNTH_OPS = ("synth", "batch", "pair")
ANALYSIS_OPS = ("filter_wave", "band_levels", "pitch_track", "mel_wave", "mel_wave_batch", "resynth")
OPS = ("vocode", "stream", "decode", "encode", "synth", "batch_sync", "batch_lane", "pair", "encode_batch", "decode_batch", "vocode_batch",
       "vocode_batch_lane") + ANALYSIS_OPS + ("vocode_device", "decode_device")
_WEIGHTS = dict(vocode=2, stream=2, decode=2, encode=2, synth=9, batch_sync=1, batch_lane=3, pair=2, encode_batch=2, decode_batch=2,
                vocode_batch=2, vocode_batch_lane=2, filter_wave=2, band_levels=2, pitch_track=2, mel_wave=2, mel_wave_batch=2, resynth=2,
                vocode_device=2, decode_device=2)                 # how often an op comes up in one deal of the deck
ABSENT = np.zeros(0, np.uint32)                    # stands for an output the call did not hand out
F = np.float32


# ---- the generator ------------------------------------------------------------------------------------------------------------------

def op_of(key):
    """the op a call key counts under: its first element, a batch split by form"""
    return "batch_" + key[1] if key[0] == "batch" else key[0]


def _pick(rng, pool):
    return pool[int(rng.integers(0, len(pool)))]


class _Deck:
    """draws without replacement from a shuffled deck, dealt anew when it runs out: every card comes up once per deal, so a history of a
    given length holds every op and every MENU entry a known number of times, whatever the seed"""

    def __init__(self, cards):
        self.cards, self.left = list(cards), []

    def take(self, rng):
        if not self.left:
            self.left = [self.cards[i] for i in rng.permutation(len(self.cards))]
        return self.left.pop()


def _decks():
    return dict(op=_Deck([o for o in OPS for _ in range(_WEIGHTS[o])]), synth=_Deck(range(len(MENU))), batch=_Deck(range(len(MENU))),
                lane=_Deck((0, 1, 1)), cache=_Deck(CACHES), analysis=_Deck(ANALYSIS_OPS))


def _draw(rng, decks, small, lane0_only=False, op=None):
    """one random call key; small: sizes from the low end of the pools (the history's opening, so that later steps grow every block);
    lane0_only: a synchronous call on lane 0 (what may run beside a batch in flight on lane 1)"""
    Ts, Ns = (TS[:3], NS[:3]) if small else (TS, NS)
    T, N, seed = lambda: int(_pick(rng, Ts)), lambda: int(_pick(rng, Ns)), lambda: int(rng.integers(0, 3))
    utts = lambda: tuple((N(), T(), seed(), int(decks["batch"].take(rng))) for _ in range(int(rng.integers(1, 7))))
    rows = lambda lo, hi: tuple((T(), seed()) for _ in range(int(rng.integers(lo, hi + 1))))
    flag = lambda: bool(rng.integers(0, 2))
    op = op or decks["op"].take(rng)
    while lane0_only and op in ("batch_lane", "pair", "vocode_batch_lane", "stream"):
        op = _pick(rng, OPS)
    if op in ("vocode", "decode", "resynth", "vocode_device", "decode_device"):
        return (op, T(), seed())
    if op == "stream":
        return (op, T(), seed(), int(_pick(rng, (16, 50, 64))))
    if op == "encode":
        return (op, N(), T(), seed())
    if op == "synth":
        return (op, N(), T(), seed(), int(decks["synth"].take(rng)), flag())
    if op == "batch_sync":
        return ("batch", "sync", 0, flag(), utts())
    if op == "batch_lane":
        return ("batch", "lane", int(decks["lane"].take(rng)), flag(), utts())
    if op == "pair":
        return (op, (0, 1) if flag() else (1, 0), flag(), utts(), flag(), utts())
    if op == "encode_batch":
        return (op, flag(), tuple((n, t, s, int(_pick(rng, ENCODER_ENTRIES))) for n, t, s, _ in utts()))
    if op in ("decode_batch", "vocode_batch"):
        return (op, rows(1, 5))
    if op == "vocode_batch_lane":
        return (op, rows(1, 5), _draw(rng, decks, small, lane0_only=True))
    if op == "filter_wave":
        return (op, T(), seed(), int(_pick(rng, (1, 33, 255))))
    if op in ("band_levels", "pitch_track"):
        return (op, T(), seed(), flag())
    if op == "mel_wave":
        t = T()
        return (op, t, seed(), flag() and t * HOP >= BINS)
    if op == "mel_wave_batch":
        r = rows(2, 4)
        return (op, r, flag() and all(t * HOP >= BINS for t, _ in r))
    raise AssertionError(op)


def _other_asks(rng, decks, key):
    """the same shape with other asks: every utterance of the call another MENU entry, everything else as it is"""
    def other(e):
        deck = decks["synth" if key[0] == "synth" else "batch"]
        new = int(deck.take(rng))
        return new if new != e else int(deck.take(rng) if deck.left else (e + 1 + rng.integers(0, len(MENU) - 1)) % len(MENU))
    again = lambda utts: tuple((n, t, s, other(e)) for n, t, s, e in utts)
    if key[0] == "synth":
        return key[:4] + (other(key[4]), key[5])
    if key[0] == "batch":
        return key[:4] + (again(key[4]),)
    return key[:3] + (again(key[3]), key[4], again(key[5]))


def history(seed, steps):
    """the list of `steps` steps for `seed`: a pure function of its arguments"""
    rng = np.random.default_rng([int(seed), 0x5a17])
    decks = _decks()
    out = [("graph", True)]
    queued = []
    graph_off = 0                                  # free steps left with graph mode off: it comes back on by itself
    reserves_due = [steps // 18, steps // 9, steps // 4]
    caches_due = [steps * k // 7 for k in range(1, 7)]          # six changes of the cache capacity, two deals of the three
    nmax = tmax = 0
    while len(out) < steps:
        small = len(out) < steps // 6
        growing = [r for r in RESERVES if r[0] > nmax and r[1] > tmax]
        if queued:
            out.append(queued.pop(0))
        elif reserves_due and len(out) >= reserves_due[0]:
            reserves_due.pop(0)                    # three reserves that exceed everything before them: two in the opening, one behind it
            out.append(("reserve",) + growing[0])
        elif caches_due and len(out) >= caches_due[0]:
            caches_due.pop(0)
            out.append(("cache", int(decks["cache"].take(rng))))
        elif graph_off == 1:
            graph_off = 0
            out.append(("graph", True))
        else:
            graph_off = max(0, graph_off - 1)
            r = rng.random()
            if r < 0.04 and not graph_off:
                graph_off = int(rng.integers(4, 10))
                out.append(("graph", False))
            elif r < 0.07:
                # (small ones only while a scheduled reserve is still to come: those must find something left to exceed)
                grow = not reserves_due and growing and rng.random() < 0.5
                out.append(("reserve",) + tuple(int(v) for v in (growing[0] if grow else _pick(rng, RESERVES[:3] if reserves_due else RESERVES))))
            elif r < 0.19:
                out.append(("poison", int(_pick(rng, (0xFF, 0x3C, 0x00))), int(rng.integers(0, 2))))
            else:
                out.append(_draw(rng, decks, small))
        last = out[-1]
        n, t = sizes_of(last)
        nmax, tmax = max(nmax, n), max(tmax, t)
        if last[0] in SYNTH_OPS and not queued:
            r = rng.random()
            if r < 1 / 3:
                queued = [_other_asks(rng, decks, last)]
            elif r < 1 / 3 + 1 / 6:
                queued = [last]
            elif r < 1 / 3 + 1 / 6 + 1 / 6:
                queued = [_draw(rng, decks, small, op=decks["analysis"].take(rng)), last]
    return out[:steps]


# ---- what a history holds -------------------------------------------------------------------------------------------------------------

def shape_of(key):
    """a synth, batch or pair key without its MENU entries: what two calls share that differ in their asks alone"""
    strip = lambda utts: tuple(u[:3] for u in utts)
    if key[0] == "synth":
        return key[:4] + key[5:]
    if key[0] == "batch":
        return key[:4] + (strip(key[4]),)
    if key[0] == "pair":
        return key[:3] + (strip(key[3]), key[4], strip(key[5]))
    return None


def _uses_lane1(key):
    return key[0] == "pair" or (key[0] == "batch" and key[1] == "lane" and key[2] == 1)


def sizes_of(key):
    """(the largest phoneme count, the largest frame capacity) a step names, 0 where it names none"""
    if key[0] == "reserve":
        return key[1], key[2]
    if key[0] in STATE_OPS:
        return 0, 0
    n = t = 0
    for k in calls_of(key):
        if k[0] in ("synth", "encode"):
            rows = [(k[1], k[2])]
        elif k[0] == "batch":
            rows = [u[:2] for u in k[4]]
        elif k[0] == "pair":
            rows = [u[:2] for u in k[3] + k[5]]
        elif k[0] == "encode_batch":
            rows = [u[:2] for u in k[2]]
        elif k[0] in ("decode_batch", "vocode_batch", "mel_wave_batch", "vocode_batch_lane"):
            rows = [(0, r[0]) for r in k[1]]
        else:
            rows = [(0, k[1])]
        n, t = max([n] + [r[0] for r in rows]), max([t] + [r[1] for r in rows])
    return n, t


def calls_of(key):
    """the calls a call key makes: itself, and the inner call of a vocode batch on lane 1"""
    return [key] + (calls_of(key[2]) if key[0] == "vocode_batch_lane" else [])


def walk(steps):
    """(index, step, graph mode, cache capacity) of every step, the state as the step finds it"""
    graph, cache = False, 16
    for i, s in enumerate(steps):
        yield i, s, graph, cache
        if s[0] == "graph":
            graph = s[1]
        elif s[0] == "cache":
            cache = s[1]


def repeats(steps):
    """the indices i of identical back-to-back call keys (steps[i - 1] == steps[i]) that run with graph mode on"""
    return [i for i, s, graph, _ in walk(steps) if i and graph and s[0] not in STATE_OPS and steps[i - 1] == s]


def coverage(steps):
    """the counts the conditions of test_call_history_cpu.py are stated on"""
    c = dict(ops={o: 0 for o in OPS}, synth_entries=[0] * len(MENU), batch_entries=[0] * len(MENU), fitted_entries=[0] * len(MENU),
             successions=0, successions_lane1=0, repeats=len(repeats(steps)), sandwiches=0, cache_steps={k: 0 for k in CACHES}, pairs=0,
             growing_reserves=0, reserves=0, poisons=0, graph_changes=0, calls=0, distinct=0)
    state = list(walk(steps))
    graph_shapes = set()
    nmax = tmax = 0
    distinct = set()
    for i, s, graph, cache in state:
        n, t = sizes_of(s)
        if s[0] == "reserve":
            c["reserves"] += 1
            c["growing_reserves"] += n > nmax and t > tmax
        nmax, tmax = max(nmax, n), max(tmax, t)
        if s[0] in STATE_OPS:
            c["poisons"] += s[0] == "poison"
            c["graph_changes"] += s[0] == "graph"
            continue
        c["cache_steps"][cache] += 1
        for k in calls_of(s):
            c["calls"] += 1
            c["ops"][op_of(k)] += 1
            if k[0] == "synth":
                c["synth_entries"][k[4]] += 1
                c["fitted_entries"][k[4]] += k[5]
            for fitted, utts in ((k[3], k[4]),) if k[0] == "batch" else ((k[2], k[3]), (k[4], k[5])) if k[0] == "pair" else ():
                for u in utts:
                    c["batch_entries"][u[3]] += 1
                    c["fitted_entries"][u[3]] += fitted
        distinct.update(p for k in [s] for p in parts(k))
        c["pairs"] += s[0] == "pair"
        prev = steps[i - 1] if i else None
        if graph and s[0] in SYNTH_OPS and prev is not None and prev[0] == s[0] and prev != s and shape_of(prev) == shape_of(s):
            c["successions"] += 1
            c["successions_lane1"] += _uses_lane1(s)
        if (graph and s[0] in ANALYSIS_OPS and 0 < i < len(steps) - 1 and prev[0] in SYNTH_OPS and steps[i + 1][0] in SYNTH_OPS
                and state[i + 1][2] and shape_of(steps[i + 1]) in graph_shapes):
            c["sandwiches"] += 1
        if graph and s[0] in SYNTH_OPS:
            graph_shapes.add(shape_of(s))
    c["distinct"] = len(distinct)
    return c


def legal(steps):
    """every call of the history is one the library accepts: no reflect pad below 513 samples, no target above its capacity, every size
    from the pools; the first offender, or None"""
    for s in steps:
        if s[0] in STATE_OPS:
            continue
        for k in calls_of(s):
            if k[0] == "mel_wave" and k[3] and k[1] * HOP < BINS:
                return k
            if k[0] == "mel_wave_batch" and k[2] and any(t * HOP < BINS for t, _ in k[1]):
                return k
            utts = [k[1:5]] if k[0] == "synth" else k[4] if k[0] == "batch" else k[3] + k[5] if k[0] == "pair" else k[2] if k[0] == "encode_batch" else ()
            for n, t, _, e in utts:
                if n not in NS or t not in TS or not 0 <= e < len(MENU) or not 1 <= target_of(t) <= t or forced_frames(n, t).sum() > t:
                    return k
    return None


# ---- the inputs, rebuilt from a key ---------------------------------------------------------------------------------------------------

def target_of(T):
    """the frame count the "target" entry fits an utterance of capacity T to"""
    return max(1, (2 * T + 2) // 3)


def forced_frames(N, T):
    """the frames the "phonemes" entry forces per phoneme: about three quarters of the capacity dealt over the N phonemes, one at least"""
    total = max(1, 3 * T // 4)
    return (total // N + (np.arange(N) < total % N)).astype(np.int32)


def speech(rate, seed, T, amp=0.3):
    """a seeded waveform of T * HOP samples: harmonics plus noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(T * HOP)
    f0 = rng.uniform(80, 300) / rate
    x = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 6)) / h for h in range(1, 12))
    return ((x * 0.3 + rng.standard_normal(t.size) * 0.05) * amp).astype(F)


def taps(seed, L):
    return (np.random.default_rng(1000 + seed).standard_normal(L) / np.sqrt(L)).astype(F)


def gains(N, seed):
    g = np.random.default_rng(seed).random(N) * 4.0
    g[::5] = 0.0
    return g.astype(F)


def asks(entry, N, T, seed):
    """MENU[entry] for an utterance of N phonemes and capacity T: the keyword arguments of synthesize, and under "levels" and
    "durations" whether the Level and the phoneme timings are asked for"""
    from zerovox_cpp_amd import capi
    a = dict(prosody=None, phonemes=None, target_frames=None, volume=None, envelope=None, return_contour=False, return_pitch=False,
             return_bands=False, filter=None, levels=False, durations=False)
    name = MENU[entry]
    if name == "everything":
        a.update(volume=capi.Volume(0.8, 0.07, 0.5), envelope=capi.Envelope(gains(N, seed), 2, 450, 1000), return_contour=True, return_pitch=True,
                 return_bands=True, filter=taps(seed, 33), levels=True, durations=True)
    elif name == "mixed":
        a.update(return_contour="frames", return_pitch=capi.PitchTrack(frames=False), return_bands=capi.BandLevels(edges=[2, 9, 40, 200, 500]),
                 filter=np.array([0.5], F), levels=True)
    elif name == "volume":
        a.update(volume=capi.Volume(1.7, 0.05, 0.4), levels=True)
    elif name == "filter1":
        a.update(filter=np.array([-0.75], F))
    elif name == "filter255":
        a.update(filter=taps(seed + 7, 255))
    elif name == "prosody":
        a.update(prosody=(1.25, 1.0, 0.1, 1.0, -0.1))
    elif name == "phonemes":
        a.update(phonemes=dict(duration_frames=forced_frames(N, T)), durations=True)
    elif name == "target":
        a.update(target_frames=target_of(T))
    else:
        assert name == "nothing"
    return a


class Context:
    """what run() needs beside the model: the geometry, the checkpoint's tensors and the model's device buffers, allocated once at the
    largest size (mel, waveform, hidden rows, style)"""

    def __init__(self, model, g, tensors):
        assert g.hop_size == HOP and g.num_mels == NUM_MELS
        self.model, self.g, self.tensors = model, g, tensors
        t = max(TS)
        self.d_mel, self.d_wav = model.device_alloc(t * NUM_MELS * 4), model.device_alloc(t * HOP * 4)
        self.d_hid, self.d_sty = model.device_alloc(t * g.E * 4), model.device_alloc(g.E * 4)

    def close(self):
        for p in (self.d_mel, self.d_wav, self.d_hid, self.d_sty):
            self.model.device_free(p)


# ---- the runner -----------------------------------------------------------------------------------------------------------------------

def parts(key):
    """the canonical keys a call is compared with, in the order run_parts() returns their outputs"""
    if key[0] == "batch":
        return [("batch", "sync", 0) + key[3:]]
    if key[0] == "pair":
        return [("batch", "sync", 0, key[2], key[3]), ("batch", "sync", 0, key[4], key[5])]
    if key[0] == "vocode_batch_lane":
        return [("vocode_batch", key[1])] + parts(key[2])
    return [key]


def _tables(holders):
    out = []
    for h in holders:
        out += [ABSENT, ABSENT] if h is None else [ABSENT if t is None else t.copy() for t in (h.frames, h.phonemes)]
    return out


def _outputs(wav, nf, dur, level, contour, pitch, bands):
    """the ten arrays of one utterance: waveform, n_frames, durations, Level bits, then the six tables; ABSENT for what was not handed out"""
    import level_rule
    return [wav.copy(), np.array([nf], np.uint32), ABSENT if dur is None else dur.copy(),
            ABSENT if level is None else np.array(level_rule.level_bits(level), np.uint32)] + _tables((contour, pitch, bands))


def run_synth(model, ctx, N, T, seed, entry, fitted, levels=None):
    """one synthesize call with MENU[entry]; levels: overrides whether the Level is asked for"""
    from zerovox_cpp_amd import synth
    a = asks(entry, N, T, seed)
    want_levels, want_dur = a.pop("levels"), a.pop("durations")
    if levels is not None:
        want_levels = levels
    out = list(model.synthesize(*synth.encoder_inputs(ctx.g, seed, N), T, fitted=fitted, return_levels=want_levels, return_durations=want_dur, **a))
    wav, nf = out[:2]
    rest = out[2:]
    dur = rest.pop(0) if want_dur else None
    level = rest.pop(0) if want_levels else None
    contour, pitch, bands = (rest.pop(0) if a[k] else None for k in ("return_contour", "return_pitch", "return_bands"))
    assert not rest
    return _outputs(wav, nf, dur, level, contour, pitch, bands)


def batch_arguments(ctx, utts, levels=None):
    """(the utterance tuples, the keyword arguments but `fitted`, the asks per utterance) of a batch whose utterance u asks MENU[utts[u][3]];
    an option no utterance asks for is not passed at all, so the call goes to the lowest form that holds its asks"""
    from zerovox_cpp_amd import synth
    rows = [asks(e, n, t, s) for n, t, s, e in utts]
    if levels is not None:
        for r in rows:
            r["levels"] = levels
    tuples = [(*synth.encoder_inputs(ctx.g, s, n), t, r["prosody"], r["phonemes"], r["target_frames"]) for (n, t, s, _), r in zip(utts, rows)]
    col = lambda k, none: [r[k] for r in rows] if any(r[k] is not None and r[k] is not False for r in rows) else none
    kw = dict(volume=col("volume", None), envelope=col("envelope", None), filter=col("filter", None), return_contour=col("return_contour", False),
              return_pitch=col("return_pitch", False), return_bands=col("return_bands", False), return_levels=any(r["levels"] for r in rows))
    return tuples, kw, rows


def _snapshot(bc, rows):
    """what a finished BatchCall handed out, per utterance as _outputs orders it, in one flat list"""
    out = []
    for u, (w, nf) in enumerate(bc.results()):
        pick = lambda name: None if getattr(bc, name) is None else getattr(bc, name)[u]
        out += _outputs(w, nf, bc.durations[u] if rows[u]["durations"] else None, bc.levels[u] if rows[u]["levels"] else None,
                        pick("contours"), pick("pitches"), pick("bands"))
    return out


def prepare(model, ctx, fitted, utts, levels=None):
    """(the BatchCall, the asks per utterance) of a batch key's utterances"""
    tuples, kw, rows = batch_arguments(ctx, utts, levels)
    return model.prepare_batch(tuples, durations=any(r["durations"] for r in rows), fitted=fitted, **kw), rows


def run_batch_sync(model, ctx, fitted, utts, levels=None):
    """the batch through synthesize_batch"""
    tuples, kw, rows = batch_arguments(ctx, utts, levels)
    want_dur = any(r["durations"] for r in rows)
    out = []
    for r, res in zip(rows, model.synthesize_batch(tuples, return_durations=want_dur, fitted=fitted, **kw)):
        rest = list(res[2:])
        dur = rest.pop(0) if want_dur else None
        level = rest.pop(0) if kw["return_levels"] else None
        contour, pitch, bands = (rest.pop(0) if kw[k] is not False else None for k in ("return_contour", "return_pitch", "return_bands"))
        assert not rest
        out += _outputs(res[0], res[1], dur if r["durations"] else None, level if r["levels"] else None, contour, pitch, bands)
    return out


def _mels(ctx, rows):
    from zerovox_cpp_amd import synth
    return [synth.vocoder_mel(ctx.g, ctx.tensors, s, t) for t, s in rows]


def _mel_params(variant):
    from zerovox_cpp_amd import capi
    return capi.MelAnalysis(pad="reflect", log="ln", centre=7) if variant else None


def _run_one(model, key, ctx):
    """a call that is one part: its outputs as a flat list of arrays"""
    from zerovox_cpp_amd import capi, synth
    g, op = ctx.g, key[0]
    wave = lambda T, seed: speech(g.sampling_rate, 50 + seed, T)
    if op == "vocode":
        return [model.vocode(synth.vocoder_mel(g, ctx.tensors, key[2], key[1]))]
    if op == "stream":
        return [np.concatenate([c[1] for c in model.vocode_stream(synth.vocoder_mel(g, ctx.tensors, key[2], key[1]), key[3])])]
    if op == "decode":
        return [model.decode(synth.decoder_hidden(g, key[2], key[1], frames_per_phoneme=2, fill=0.9), synth.encoder_inputs(g, key[2], 4)[2])]
    if op == "encode":
        e = model.encode(*synth.encoder_inputs(g, key[3], key[1]), key[2])
        return [e["hidden"], e["logdur"], np.array([e["n_frames"]], np.uint32)]
    if op == "synth":
        return run_synth(model, ctx, *key[1:])
    if op == "batch":
        return run_batch_sync(model, ctx, key[3], key[4])
    if op == "encode_batch":
        rows = [asks(e, n, t, s) for n, t, s, e in key[2]]
        tuples = [(*synth.encoder_inputs(g, s, n), t, r["prosody"], r["phonemes"], r["target_frames"]) for (n, t, s, _), r in zip(key[2], rows)]
        out = []
        for e in model.encode_batch(tuples, return_hidden=key[1], return_durations=True):
            out += [e["hidden"] if key[1] else ABSENT, np.array([e["n_frames"]], np.uint32), e["durations"]]
        return out
    if op == "decode_batch":
        return model.decode_batch([synth.decoder_hidden(g, s, t, frames_per_phoneme=2, fill=0.9) for t, s in key[1]],
                                  [synth.encoder_inputs(g, s, 4)[2] for _, s in key[1]])
    if op == "vocode_batch":
        return model.vocode_batch(_mels(ctx, key[1]))
    if op == "filter_wave":
        return [model.filter_wave(wave(key[1], key[2]), taps(key[2], key[3]))]
    if op == "band_levels":
        return [model.band_levels(wave(key[1], key[2]), capi.BandLevels(edges=[2, 9, 40, 200, 500]) if key[3] else None).frames]
    if op == "pitch_track":
        return [model.pitch_track(wave(key[1], key[2]), capi.PitchTrack(min_lag=40, max_lag=300, window=512) if key[3] else None).frames]
    if op == "mel_wave":
        return [model.mel_wave(wave(key[1], key[2]), _mel_params(key[3]))]
    if op == "mel_wave_batch":
        return model.mel_wave_batch([wave(t, s) for t, s in key[1]], _mel_params(key[2]))
    if op == "resynth":
        return [model.resynthesize(wave(key[1], key[2]))]
    if op == "vocode_device":
        T = key[1]
        model.h2d(ctx.d_mel, synth.vocoder_mel(g, ctx.tensors, key[2], T))
        model.vocode_device(ctx.d_mel, T, ctx.d_wav)
        model.synchronize()
        wav = np.empty(T * HOP, F)
        model.d2h(wav, ctx.d_wav)
        return [wav]
    if op == "decode_device":
        T = key[1]
        model.h2d(ctx.d_hid, synth.decoder_hidden(g, key[2], T, frames_per_phoneme=2, fill=0.9))
        model.h2d(ctx.d_sty, synth.encoder_inputs(g, key[2], 4)[2])
        model.decode_device(ctx.d_hid, ctx.d_sty, T, ctx.d_mel)
        model.synchronize()
        mel = np.empty((T, NUM_MELS), F)
        model.d2h(mel, ctx.d_mel)
        return [mel]
    raise AssertionError(key)


def run_parts(model, key, ctx):
    """makes the call of `key` on `model`; one flat list of arrays per entry of parts(key)"""
    op = key[0]
    if op == "batch" and key[1] == "lane":
        bc, rows = prepare(model, ctx, key[3], key[4])
        bc.begin(key[2])
        bc.end(key[2])
        return [_snapshot(bc, rows)]
    if op == "pair":
        calls = [prepare(model, ctx, key[2], key[3]), prepare(model, ctx, key[4], key[5])]
        calls[0][0].begin(0)
        calls[1][0].begin(1)
        for lane in key[1]:
            calls[lane][0].end(lane)
        return [_snapshot(bc, rows) for bc, rows in calls]
    if op == "vocode_batch_lane":
        model.vocode_batch_begin(1, _mels(ctx, key[1]))
        inner = run_parts(model, key[2], ctx)
        return [[w.copy() for w in model.vocode_batch_end(1)]] + inner
    return [[np.array(x, copy=True) for x in _run_one(model, key, ctx)]]


def run(model, key, ctx):
    """makes the call and returns its outputs as one flat list of numpy arrays"""
    return [x for part in run_parts(model, key, ctx) for x in part]


def apply_state(model, step):
    """a state change on `model`"""
    if step[0] == "graph":
        model.set_graph_mode(step[1])
    elif step[0] == "cache":
        model.set_graph_cache(step[1])
    elif step[0] == "reserve":
        model.reserve(step[1], step[2])
    elif step[0] == "poison":
        model.poison(step[1], step[2])
    else:
        raise AssertionError(step)


def bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype.itemsize == 4, x.dtype
    return x.reshape(-1).view(np.uint32)


def same(got, want, key):
    """got and want, two flat lists of arrays, agree in length, shapes, dtypes and every bit; else the key, the output's index and the
    first element that differs"""
    assert len(got) == len(want), (key, "outputs", len(got), len(want))
    for i, (x, y) in enumerate(zip(got, want)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (key, "output", i, x.shape, x.dtype, y.shape, y.dtype)
        bad = np.flatnonzero(bits(x) != bits(y))
        assert bad.size == 0, (key, "output", i, "element", int(bad[0]), x.reshape(-1)[bad[0]], y.reshape(-1)[bad[0]], "of", int(bad.size), "differing")
