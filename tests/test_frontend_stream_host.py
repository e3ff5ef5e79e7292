"""CPU checks of the online front-end: the running-normalisation oracle against
its direct definition, a NumPy model of the chunked front-end against the whole-signal oracle,
FrameSchedule against brute force, and what Python refuses before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from asr_study_amd import _lib
from asr_study_amd.preprocessing import audio
from tests import frontend_stream_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECES = (7, 159, 160, 161, 400, 401, 1000, None)


# ------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize('mean_norm,var_norm', [(True, True), (False, True), (True, False)])
def test_running_standardize_is_the_direct_definition(mean_norm, var_norm):
    rs = np.random.RandomState(3)
    x = rs.randn(40, 5) * np.array([1.0, 10.0, 0.1, 3.0, 1.0]) + np.array([0, 5, -2, 100, 0])
    x[:, 4] = -36.04365338911715            # a constant column (log of the float64 eps)
    got = FO.running_standardize(x, mean_norm, var_norm, 1e-8)
    for t in range(len(x)):
        mean = np.mean(x[:t + 1], axis=0) if mean_norm else 0.0
        den = (np.std(x[:t + 1], axis=0) + 1e-8) if var_norm else 1.0
        want = (x[t] - mean) / den
        # (near sd_t = 0 -- frame 0 -- both divide a rounding error by eps)
        np.testing.assert_allclose(got[t, :4], want[:4], rtol=1e-9, atol=1e-6)
    if mean_norm:
        assert np.all(got[0] == 0.0)
        assert np.all(got[:, 4] == 0.0)
    if mean_norm and var_norm:
        t = np.arange(len(x))[:, None]
        assert np.all(np.abs(got) <= np.sqrt(t + 1) * (1 + 1e-12))


def test_running_oracle_keeps_empty_filters_at_zero():
    x = FO.signal(1999, 5)
    got = FO.extract_running('logfbank', x, num_filt=80)
    assert got.shape == (11, 80)
    assert np.all(got[:, list(FO.EMPTY_FILTERS_80)] == 0.0)
    assert np.all(got[0] == 0.0)
    assert np.abs(got).max() > 0.5


# ------------------------------------------------------------------------------ the chunked model
@pytest.mark.parametrize('name', sorted(FO.CONFIGS))
def test_chunked_model_equals_the_whole_signal_oracle(name):
    kind, _, kw = FO.CONFIGS[name]
    for n in FO.LENGTHS:
        x = FO.signal(n, 100 + n)
        raw_rows, want = FO.extract_running_rowwise(kind, x, **kw)
        # (the row-at-a-time form of the oracle is the oracle, to the rounding of NumPy's
        # batched matrix product and log)
        np.testing.assert_allclose(raw_rows, FO.kept(kind, x, **kw), rtol=0, atol=1e-11)
        splits = PIECES + ((1,) if n == 561 else ())
        for piece in splits:
            m = FO.ChunkedModel(kind, **kw)
            rows = []
            for lo, hi in FO.pieces(n, piece):
                rows.append(m.feed(x[lo:hi], ended=n if hi == n else None))
            got = np.concatenate([r for r in rows if len(r)], 0)
            assert got.shape == want.shape, (name, n, piece)
            assert np.array_equal(got, want), (name, n, piece, np.abs(got - want).max())


def test_chunked_model_end_given_after_the_last_sample():
    """The length arrives with an empty feed (finish): the tail frame is computed then."""
    kind, _, kw = FO.CONFIGS['mfcc39']
    for n in (401, 561, 1041, 1999):
        x = FO.signal(n, 7 + n)
        m = FO.ChunkedModel(kind, **kw)
        rows = [m.feed(x[lo:hi]) for lo, hi in FO.pieces(n, 160)] + [m.feed(x[:0], ended=n)]
        got = np.concatenate([r for r in rows if len(r)], 0)
        assert np.array_equal(got, FO.extract_running_rowwise(kind, x, **kw)[1])


# ------------------------------------------------------------------------------ FrameSchedule
@pytest.mark.parametrize('la', [0, 2, 4])
@pytest.mark.parametrize('stride', [1, 2, 3])
def test_frame_schedule_against_brute_force(la, stride):
    L, S = 400, 160
    sc = audio.FrameSchedule(L, S, la, stride)
    for samples in range(0, 3 * L + 1):
        complete = sum(1 for f in range(samples) if f * S + L <= samples)
        assert sc.complete(samples) == complete
        final = [f for f in range(complete) if f + la < complete]
        assert sc.final(samples) == len(final)
        assert sc.rows(samples) == sum(1 for f in final if f % stride == 0)
        if samples >= 1:
            # ended: every frame that holds a sample, the first always
            frames = [f for f in range(samples) if f == 0 or (f - 1) * S + L < samples]
            assert sc.total(samples) == len(frames)
            assert sc.final(samples, ended=samples) == len(frames)
            assert sc.rows(samples, ended=samples) == sum(1 for f in frames if f % stride == 0)
            assert sc.final(samples, ended=samples + 1) == len(final)       # not reached yet
        # lock-step: running streams bound the window; all ended: the longest
        assert sc.window(samples, [None, 2]) == len(final)
        if samples >= 2:
            assert sc.window(samples, [samples, 2]) == sc.total(samples)


def test_frame_schedule_matches_the_frame_counts_of_the_issue():
    sc = audio.FrameSchedule(400, 160, 4, 1)
    assert [sc.total(n) for n in FO.LENGTHS] == [1, 1, 2, 2, 3, 3, 6, 11, 99]


# ------------------------------------------------------------------------------ refusals
def test_norm_is_validated():
    assert audio.MFCC(device='cpu').norm == 'utterance'
    assert audio.MFCC(norm='running', device='cpu')._cfg().norm_mode == 1
    assert audio.MFCC(device='cpu')._cfg().norm_mode == 0
    with pytest.raises(ValueError, match='norm'):
        audio.MFCC(norm='bogus', device='cpu')
    with pytest.raises(ValueError, match='num_context'):
        audio.LogFbank(norm='running', num_context=1, device='cpu')


def test_a_stream_refuses_utterance_normalisation():
    with pytest.raises(ValueError, match='whole-utterance'):
        audio.MFCC(device='cpu').stream()
    with pytest.raises(ValueError, match='whole-utterance'):
        audio.LogFbank(norm='utterance', device='cpu').stream(3)


def test_stream_audio_needs_stream():
    from asr_study_amd import cli
    with pytest.raises(ValueError, match='--stream_audio'):
        cli.predict_main(['--model', 'nowhere.h5', '--file', 'nowhere.wav', '--stream_audio'])


def test_norm_travels_through_the_plugin_parameters():
    from asr_study_amd.cli import utils
    f = utils.get_from_module('preprocessing.audio', 'mfcc', params=['norm', 'running',
                                                                      'device', 'cpu'])
    assert f.norm == 'running' and f._cfg().norm_mode == 1


# ------------------------------------------------------------------------------ the binding
def test_frontend_cfg_still_matches_the_header():
    header = open(os.path.join(ROOT, 'include', 'asr_hip.h')).read()
    body = re.search(r'typedef struct asr_frontend_cfg \{(.*?)\} asr_frontend_cfg;', header,
                     re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            kind, rest = decl.split(None, 1)
            names += [(n.strip(), kind) for n in rest.split(',')]
    want = [(n, {C.c_int: 'int', C.c_double: 'double'}[t]) for n, t in _lib.FrontendCfg._fields_]
    assert names == want
    assert ('norm_mode', 'int') in names and 'reserved' not in dict(names)
    F = _lib.FrontendCfg
    assert (C.sizeof(F), F.norm_mode.offset, F.pre_emph.offset, F.eps.offset) == (72, 52, 56, 64)
    assert re.search(r'#define ASR_HIP_ABI_VERSION 107\b', header)
    for name in ('asr_frontend_stream_state_bytes', 'asr_frontend_stream_host_ints',
                 'asr_frontend_stream_workspace_bytes', 'asr_frontend_stream_reset',
                 'asr_frontend_stream'):
        assert name in _lib.SIGNATURES and re.search(r'\b%s\s*\(' % name, header)


def test_stream_entry_point_refuses_utterance_mode_without_a_device():
    """norm_mode = 0 is refused before anything is touched (no GPU needed)."""
    lib = _lib.load()
    cfg = audio.MFCC(device='cpu')._cfg()
    buf = (C.c_char * 64)()
    host = (C.c_longlong * lib.asr_frontend_stream_host_ints(1))()
    rc = lib.asr_frontend_stream_reset(C.byref(cfg), C.cast(buf, C.c_void_p),
                                       C.cast(host, C.c_void_p), 1, C.cast(buf, C.c_void_p),
                                       C.cast(buf, C.c_void_p), None)
    assert rc == -1
    assert b'whole-utterance statistics need the end of the utterance' in lib.asr_last_error()
