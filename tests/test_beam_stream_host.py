"""Host checks of the streaming beam decoder (K27): the chunked model of the resumable kernel
(tests/beam_stream_model.py) against the whole-utterance model (tests/beam_device_model.py) on
tied logits, the stable prefix against a brute force over the beam's tree paths, the refusals and
the size functions of the library (no device is touched), the exported symbols, and what
Model.stream(beam=...) does before its first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from asr_study_amd import _lib as L
from tests.beam_device_model import beam_device_model
from tests.beam_stream_model import BeamStream, beam_stream_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1
NEW_SYMBOLS = ['asr_ctc_beam_stream_state_bytes', 'asr_ctc_beam_stream_workspace_bytes',
               'asr_ctc_beam_stream', 'asr_ctc_beam_lm_stream']
T = 23
SPLITS = {'ones': [1] * T, '3_7_13': [3, 7, 13], 'whole': [T]}


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def _tied(C_, W):
    rs = np.random.RandomState(C_ * 100 + W)
    x = np.round(rs.randn(T, C_) * 2).astype(np.float32) / 2
    x[5:8] = 0.0                                     # all-equal frames
    return x


def _common_prefix(paths):
    out = []
    for col in zip(*paths):
        if any(c != col[0] for c in col):
            break
        out.append(col[0])
    return out


# ----------------------------------------------------------------------------- the model
@pytest.mark.parametrize('merge', [True, False])
@pytest.mark.parametrize('W', [1, 4, 7, 40])
@pytest.mark.parametrize('C_', [2, 3, 5, 6])
def test_chunked_model_is_the_whole_utterance_model(C_, W, merge):
    x = _tied(C_, W)
    want, wscore = beam_device_model(x, W, merge)
    tables = []
    for name, splits in SPLITS.items():
        st, outs = beam_stream_model(x, W, splits, merge)
        labels, score, _ = outs[-1]
        assert labels == want and score == wscore, name         # the same float64, not close
        tables.append(st.table())
        # the stable prefix after every chunk
        st2, pos, last = BeamStream(C_, W, merge), 0, 0
        for s in splits:
            labels_s, _, stable = st2.feed(x[pos:pos + s])
            pos += s
            assert stable >= last, (name, pos)
            last = stable
            assert labels_s[:stable] == want[:stable], (name, pos)
            assert stable <= len(labels_s)
            # brute force: the common prefix of the UNMERGED tree paths of all beam entries
            brute = st2.merged(_common_prefix([st2.path(c) for c in st2.b_node]))
            assert stable == len(brute) and labels_s[:stable] == brute, (name, pos)
        assert last <= len(want)
    for t in tables[1:]:
        assert t == tables[0]                                   # the same table and tree


def test_stable_prefix_commits_something_before_the_end():
    """Peaked logits: the beam agrees on its past, so the stable prefix grows during the
    stream, and with width 1 it is the whole hypothesis."""
    rs = np.random.RandomState(3)
    x = rs.randn(T, 6).astype(np.float32)
    x[np.arange(T), rs.randint(0, 6, size=T)] += 8.0
    _, outs = beam_stream_model(x, 4, [1] * T)
    assert outs[T // 2][2] > 0
    _, outs = beam_stream_model(x, 1, [1] * T)
    assert all(stable == len(labels) for labels, _, stable in outs)


# ----------------------------------------------------------------------------- the library
def test_size_functions(lib):
    per = lambda W, lm: -(-(32 + W * (24 + (12 if lm else 8))) // 64) * 64
    for N, W, lm in ((1, 1, 0), (3, 100, 0), (3, 100, 1), (64, 1024, 1)):
        assert lib.asr_ctc_beam_stream_state_bytes(N, 28, W, lm) == N * per(W, lm)
    for bad in ((0, 28, 8, 0), (1, 1, 8, 0), (1, 65, 8, 0), (1, 28, 0, 0), (1, 28, 1025, 0)):
        assert lib.asr_ctc_beam_stream_state_bytes(*bad) == 0, bad
    # the sizing of the whole-utterance decoders at T = max_frames
    for mf, N, C_, W in ((3000, 1, 28, 100), (40, 3, 6, 129), (1, 2, 2, 1)):
        assert lib.asr_ctc_beam_stream_workspace_bytes(mf, N, C_, W, 0) == \
            lib.asr_ctc_beam_device_workspace_bytes(mf, N, C_, W)
        assert lib.asr_ctc_beam_stream_workspace_bytes(mf, N, C_, W, 1) == \
            lib.asr_ctc_beam_lm_device_workspace_bytes(mf, N, C_, W)
    blocks = 3000 * 100
    assert lib.asr_ctc_beam_stream_workspace_bytes(3000, 1, 28, 100, 0) == \
        -(-(64 + (1 + blocks * 27) * 8 + blocks * 4) // 256) * 256
    for bad in ((0, 1, 28, 8), (10, 0, 28, 8), (10, 1, 65, 8), (10, 1, 28, 1025), (10, 1, 1, 8)):
        assert lib.asr_ctc_beam_stream_workspace_bytes(*bad, 0) == 0, bad
    # node ids are int32: max_frames * width * (C - 1) must stay below 2^31
    assert lib.asr_ctc_beam_stream_workspace_bytes(33289, 1, 64, 1024, 0) == 0
    assert lib.asr_ctc_beam_stream_workspace_bytes(33288, 1, 64, 1024, 0) > 0
    assert 33289 * 1024 * 63 >= 2 ** 31 - 1 > 33288 * 1024 * 63


def test_bad_calls_are_refused_without_a_device(lib):
    """ASR_ERR_INVALID before any device call: the buffers are host memory no kernel could use."""
    buf = (C.c_char * 8192)()
    base = (C.addressof(buf) + 63) & ~63
    big = 1 << 40

    def call(lm=False, **kw):
        a = dict(logits=base, chunk_len=base, Tq=4, N=1, n_pad=16, C=5, W=8, merge=1, w=base,
                 order=2, max_frames=16, state=base, state_bytes=big, ws=base, ws_bytes=big,
                 dec=base, dlen=base, stable=base, score=base)
        a.update(kw)
        head = (a['logits'], a['chunk_len'], a['Tq'], a['N'], a['n_pad'], a['C'], a['W'],
                a['merge'])
        tail = (a['max_frames'], a['state'], a['state_bytes'], a['ws'], a['ws_bytes'], a['dec'],
                a['dlen'], a['stable'], a['score'], None)
        if lm:
            return lib.asr_ctc_beam_lm_stream(*(head + (a['w'], a['order']) + tail))
        return lib.asr_ctc_beam_stream(*(head + tail))

    for lm in (False, True):
        for name in ('logits', 'chunk_len', 'state', 'ws', 'dec', 'dlen', 'stable', 'score'):
            assert call(lm, **{name: None}) == ERR_INVALID, name
            assert b'null' in lib.asr_last_error()
        for kw in (dict(Tq=0), dict(Tq=17), dict(C=65), dict(C=1), dict(W=0), dict(W=1025),
                   dict(N=0), dict(n_pad=0), dict(max_frames=0, Tq=1)):
            assert call(lm, **kw) == ERR_INVALID, kw
        need_state = lib.asr_ctc_beam_stream_state_bytes(1, 5, 8, int(lm))
        need_ws = lib.asr_ctc_beam_stream_workspace_bytes(16, 1, 5, 8, int(lm))
        assert call(lm, state_bytes=need_state - 1) == ERR_INVALID
        assert b'state' in lib.asr_last_error()
        assert call(lm, ws_bytes=need_ws - 1) == ERR_INVALID
        assert b'workspace' in lib.asr_last_error()
        # ids past int32
        assert call(lm, C=64, W=1024, max_frames=33289) == ERR_INVALID
    for kw in (dict(w=None), dict(order=0), dict(order=6)):
        assert call(True, **kw) == ERR_INVALID, kw


def test_new_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(ROOT, 'include', 'asr_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in L.SIGNATURES, name
        assert name in design, name
    i, p, z = C.c_int, C.c_void_p, C.c_size_t
    assert L.SIGNATURES['asr_ctc_beam_stream_state_bytes'] == (z, [i] * 4)
    assert L.SIGNATURES['asr_ctc_beam_stream_workspace_bytes'] == (z, [i] * 5)
    assert L.SIGNATURES['asr_ctc_beam_stream'] == (
        i, [p, p] + [i] * 7 + [p, z, p, z] + [p] * 5)
    assert L.SIGNATURES['asr_ctc_beam_lm_stream'] == (
        i, [p, p] + [i] * 6 + [p, i, i] + [p, z, p, z] + [p] * 5)
    assert lib.asr_version() == L.ABI_VERSION == 107                # additions only
    from asr_study_amd import ops
    assert callable(ops.ctc_beam_stream) and callable(ops.BeamStreamState)


# ----------------------------------------------------------------------------- Model.stream
SMALL = dict(num_features=16, num_classes=7, d_model=32, num_heads=2, num_layers=2, d_ff=64,
             dropout=0, conv=False, device='cpu', kernel_size=7, conv_norm='layer',
             context=(4, 8, 0), causal_conv=True)


def test_model_stream_with_a_beam_up_to_the_first_device_call():
    from asr_study_amd.core import models
    from asr_study_amd.core.stream import BEAM_MAX_FRAMES
    model = models.conformer(**SMALL)
    model.decoder = dict(is_greedy=False, beam_width=8, merge_repeated=False)
    with pytest.raises(NotImplementedError) as e:            # as before, and it names the way out
        model.stream()
    assert 'beam=' in str(e.value)
    ss = model.stream(beam=True)
    assert ss.beam == dict(beam_width=8, merge_repeated=False, max_frames=BEAM_MAX_FRAMES,
                           lm=None) and BEAM_MAX_FRAMES == 3000
    assert ss.hypothesis() == [([], 0.0)]
    ss = model.stream(n_streams=2, step=4, beam=dict(beam_width=3, max_frames=8))
    assert ss.beam['beam_width'] == 3 and ss.beam['max_frames'] == 8
    assert ss.beam['merge_repeated'] is False and ss.step == 4
    # a step that would take a stream past max_frames: refused on the host, before any launch
    with pytest.raises(ValueError) as e:
        ss.feed(np.zeros((2, 12, 16), np.float32))
    assert 'max_frames' in str(e.value)
    assert ss.frames_in == 0 and ss._pend is None           # refused before the input was taken
    # what is refused
    for bad in (dict(beam_width=0), dict(beam_width=1025), dict(max_frames=0), dict(width=8),
                dict(max_frames=3)):                            # (less than one step of 16)
        with pytest.raises(ValueError):
            model.stream(beam=bad)
    model.decoder = dict(is_greedy=True)
    with pytest.raises(ValueError):
        model.stream(beam=True)                                 # no beam decoder to take it from
    assert model.stream(beam=dict(beam_width=5)).beam['beam_width'] == 5
    assert model.stream().beam is None
    with pytest.raises(RuntimeError):
        model.stream().hypothesis()
    model.decoder = None
    with pytest.raises(ValueError):
        model.stream(beam=True)
    # a model that cannot stream is refused for the reasons check gives, beam or not
    with pytest.raises(ValueError) as e:
        models.conformer(**dict(SMALL, causal_conv=False)).stream(beam=dict(beam_width=4))
    assert '(dwconv)' in str(e.value)
