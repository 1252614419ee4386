"""-m gpu: the narrow convs of a batch on all eight XCDs (csrc/conv_xcd.h, launch_conv_from in csrc/conv.hip) give the bits of the
forms they replace.

A launch over several segments with fewer than 8 channel groups either leaves the loader-wave ("single-utterance") form of
conv1d_mfma_kernel for the ordinary one (more than a round of workgroups) or keeps it on the spread map (a channel group's row
tiles dealt over 8 / 4 / 2 / 1 XCDs).  Every output element is one accumulation chain whatever the form, the tile shape or the
workgroup order, so the default schedule must equal, as uint32 views of waveforms, frame counts and mel,

    * ZV_CONV_SINGLE=0: no launch takes the loader-wave form (the batch-form model of scripts/single_stress.py), and
    * ZV_CONV_XCD=0:    the loader-wave form on a plain (row tile, channel group) grid,

eagerly and under graph replay, with ZV_VOC_RUNS=2 and ZV_DEC_RUNS=2 in every arm.  The lane's buffers are poisoned before every
call (tests/test_gpu_poison.py): a row tile that no workgroup owns is a missing write and shows as 0xFF / 0x3C bytes.

(i)   3 utterances, capacities T = 40, 64, 96 with 9, 33, 70 phonemes: loader-wave launches with ny = 1 (asr0, to_out), 2 (the
      predictors' first conv), 5 and 9 (the 528- and 1 056-channel decoder convs, below the GEMM threshold).  A batch's capacities are
      the longest utterance's, rounded up to 32 phonemes and 64 frames: nx = 3 x 2 row tiles for asr0, 3 x 4 for to_out (p = 8) and
      3 x 3 for the predictors (p = 4) — no multiple of p.
(ii)  32 utterances of 32 .. 256 phonemes, one of exactly 256, T = 32: the predictors' first conv at the benchmark's own grid
      (8 row tiles x 32 utterances x 2 channel groups = 512 workgroups, on the loader-wave form's threshold), with a trivial vocoder.
(iii) one utterance, 128 phonemes, T = 512: the single-utterance schedule; besides the bits, the stages and launch counts
      zv_profile_end reports are those of the commit before the header existed, recorded below."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RUNS = dict(ZV_VOC_RUNS=2, ZV_DEC_RUNS=2)
ARMS = {"default": {}, "batch_form": {"ZV_CONV_SINGLE": 0}, "plain_grid": {"ZV_CONV_XCD": 0}}
FILLS = (0xFF, 0x3C)
_M = {}

# (stage, launches) of zv_synthesize(128 phonemes, T = 512), medium geometry, eager, ZV_VOC_RUNS = ZV_DEC_RUNS = 2, as the library
# reported them before conv_xcd.h existed
PARENT_PROFILE = [("enc_embed", 1), ("enc_linear", 8), ("enc_attention", 4), ("enc_layernorm", 14), ("enc_conv", 14), ("enc_length_regulator", 1),
                  ("enc_dec_runs", 1), ("dec_adain_fc", 1), ("dec_in_stats", 3), ("dec_norm_operand", 14), ("dec_conv", 17), ("dec_norm_apply", 1),
                  ("dec_run_expand", 1), ("voc_runs", 1), ("voc_input_conv", 1), ("voc_upsample", 4), ("voc_resblock_s0", 6),
                  ("voc_resblock_s1", 3), ("voc_resblock_s2", 3), ("voc_resblock_s3", 1), ("voc_output_conv", 1), ("voc_run_fill", 1)]


@pytest.fixture(scope="module")
def models(ckpt):
    """arm -> its model, built and used under the arm's switches"""
    from zerovox_cpp_amd import capi
    path, g, tensors = ckpt("medium")
    for arm, sw in ARMS.items():
        if arm not in _M:
            with capi.switches(**RUNS, **sw):
                _M[arm] = capi.Model(path, 0)
    return g, _M


def teardown_module(module):
    for m in _M.values():
        m.close()
    _M.clear()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype.itemsize == 4 else x


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        if isinstance(b, np.ndarray):
            a, b = _bits(a), _bits(b)
            assert a.shape == b.shape and np.array_equal(a, b), (what, i, int((a != b).sum()) if a.shape == b.shape else (a.shape, b.shape))
        else:
            assert a == b, (what, i, a, b)


def _all_arms(models, call, what):
    """call(model) -> flat list of arrays and integers.  The batch-form arm, eager, is the reference; every arm then runs eagerly and
    under graph replay (capture, replay, replay), its lane poisoned before every call."""
    from zerovox_cpp_amd import capi
    _, ms = models
    with capi.switches(**RUNS, **ARMS["batch_form"]):
        ms["batch_form"].set_graph_mode(False)
        want = call(ms["batch_form"])
    assert all(np.isfinite(w).all() for w in want if isinstance(w, np.ndarray) and w.dtype == np.float32), what
    for arm, sw in ARMS.items():
        m = ms[arm]
        with capi.switches(**RUNS, **sw):
            for graph in (False, True):
                m.set_graph_mode(graph)
                for fill in FILLS + FILLS[:1]:
                    m.poison(fill, 0)
                    _same(call(m), want, (what, arm, "graph" if graph else "eager", hex(fill)))
                assert m.poison(FILLS[0], 0)[0] > 0, (what, arm)             # the hook did fill what the calls used
            m.set_graph_mode(False)
    return want


def _batch_call(utts):
    calls = {}

    def call(m):
        if id(m) not in calls:
            calls[id(m)] = m.prepare_batch(utts)                    # one set of buffers per model: a captured graph replays
        bc = calls[id(m)]
        for w in bc.wavs:
            w[:] = np.nan
        bc.run()
        return [x for wav, nf in bc.results() for x in (wav.copy(), nf)]

    return call


def _mel(m, u):
    ids, puncts, style, T = u
    return m.decode(m.encode(ids, puncts, style, T)["hidden"], style)


def test_three_utterances_with_row_tiles_that_do_not_fill_the_xcds(models):
    from zerovox_cpp_amd import synth
    g, _ = models
    utts = [(*synth.encoder_inputs(g, 8100 + i, N), T) for i, (N, T) in enumerate(((9, 40), (33, 64), (70, 96)))]
    want = _all_arms(models, _batch_call(utts), "case (i)")
    assert all(0 < nf <= u[3] for nf, u in zip(want[1::2], utts)), want[1::2]
    # the mel of each utterance (the stand-alone stages: one segment, the group map)
    _all_arms(models, lambda m: [_mel(m, u) for u in utts], "case (i), mel")


def test_predictor_convs_at_the_benchmark_grid(models):
    from zerovox_cpp_amd import synth
    g, _ = models
    rng = np.random.default_rng(8200)
    Ns = [int(n) for n in rng.integers(32, 257, 32)]
    Ns[17] = 256
    assert max(Ns) == 256 and min(Ns) >= 32
    utts = [(*synth.encoder_inputs(g, 8200 + i, N), 32) for i, N in enumerate(Ns)]
    want = _all_arms(models, _batch_call(utts), "case (ii)")
    assert all(0 < nf <= 32 for nf in want[1::2]), want[1::2]


def test_one_utterance_keeps_its_schedule(models):
    from zerovox_cpp_amd import capi, synth
    g, ms = models
    u = (*synth.encoder_inputs(g, 8300, 128), 512)

    def call(m):
        wav, nf = m.synthesize(*u)
        return [wav, nf, _mel(m, u)]

    want = _all_arms(models, call, "case (iii)")
    assert 0 < want[1] <= 512
    m = ms["default"]
    with capi.switches(**RUNS):
        m.set_graph_mode(False)
        m.profile_begin()
        m.synthesize(*u)
        prof = [(s["name"], s["launches"]) for s in m.profile_end()]
    print("profile:", prof)
    assert prof == PARENT_PROFILE, prof
