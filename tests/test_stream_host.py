"""Host checks of cached chunk-by-chunk inference (K26): the chunked float64 oracle against the
whole-utterance oracle, the ring plan against a brute-force search, the refusals of Model.stream
and of the library (no device is touched), the emission schedule against the reach formula, the
exported symbols and the stage-kind table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from asr_study_amd import _lib as L
from tests import stream_oracle as SO
from tests import window_oracle as WO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1                    # ASR_ERR_INVALID of include/asr_hip.h
NEW_SYMBOLS = ['asr_ring_put', 'asr_attn_stream_plan', 'asr_attn_stream_fwd',
               'asr_relattn_stream_fwd', 'asr_dwconv1d_stream_fwd', 'asr_ctc_greedy_stream']
WINDOWS = [(4, 8, 0), (1, 5, 0), (7, 3, 0)]
PIECES = [1, 7, 13, 3, 17]


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


@pytest.fixture()
def on_cpu(monkeypatch):
    from asr_study_amd.core import engine
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')


def _model(build, context, **kw):
    """Model (a) and model (b) of tests/test_gpu_window.py."""
    from tests import test_gpu_window as TW
    model = TW._blocks(context) if build == 'blocks' else TW._conformer(context=context, **kw)
    TW._randomise(model, np.random.RandomState(5))
    return model


def _default_step(chunk):
    return -(-16 // chunk) * chunk


# ----------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize('build', ['blocks', 'conformer'])
@pytest.mark.parametrize('window', WINDOWS, ids=['%d_%d_%d' % w for w in WINDOWS])
def test_chunked_oracle_is_the_whole_utterance_oracle(on_cpu, build, window):
    rs = np.random.RandomState(11)
    T, N, F = 41, 3, 10
    assert sum(PIECES) == T
    stages = WO.stages_from_model(_model(build, window))
    lens = np.array([41, 33, 9])
    x = rs.randn(T, N, F)
    for n in range(N):
        x[lens[n]:, n] = 0.0
    want, _ = WO.model_forward(stages, x, lens, training=False)
    got = SO.model_stream(stages, x, lens, PIECES, _default_step(window[0]))
    assert got.shape == want.shape
    for n in range(N):
        err = np.abs(got[:lens[n], n] - want[:lens[n], n]).max()
        assert err < 1e-12 * max(1.0, np.abs(want).max()), (n, err)
    # the greedy decoder with a carried last label, on the same logits
    for step in (1, 3, 16):
        labels, last = [[] for _ in range(N)], [-1] * N
        for t0 in range(0, T, step):
            add, last = SO.greedy_chunk(want[t0:t0 + step], np.clip(lens - t0, 0, step), last)
            labels = [a + b for a, b in zip(labels, add)]
        assert labels == WO.greedy(want, lens)


# ----------------------------------------------------------------------------- the ring plan
def test_ring_plan_is_the_smallest_valid_ring():
    """asr_attn_stream_plan against a brute-force search over t0, for every left 0 .. 130, chunk
    1 .. 64 and count of new frames 1 .. 64; never above left + chunk - 1 + Tq + 63 rounded up."""
    from asr_study_amd import ops
    for left in range(131):
        for chunk in range(1, 65):
            span = SO.ring_span((chunk, left, 0))
            for tq in range(1, 65):
                want = -(-(span + tq) // 64) * 64
                got = ops.attn_stream_plan((chunk, left, 0), tq)
                assert got == want, (chunk, left, tq, got, want)
                assert got <= -(-(left + chunk - 1 + tq + 63) // 64) * 64
    # the brute force itself, frame by frame, on a few windows
    for window, tq in (((4, 8, 0), 16), ((64, 0, 0), 1), ((16, 64, 0), 16), ((7, 3, 0), 21)):
        chunk, left, _ = window
        need = max(t0 + tq - max(0, t0 // chunk * chunk - left) // 64 * 64 for t0 in range(5000))
        assert SO.ring_rows(window, tq) == -(-need // 64) * 64 == ops.attn_stream_plan(window, tq)


def test_bad_plans_and_calls_are_refused_without_a_device(lib):
    """ASR_ERR_INVALID before any device call: the buffers are host memory no kernel could use."""
    buf = (C.c_char * 8192)()
    base = (C.addressof(buf) + 63) & ~63
    rows = C.c_int(-7)
    for bad in ((0, 8, 0), (4, -1, 0), (4, 8, 1)):
        assert lib.asr_attn_stream_plan(C.byref(L.AttnWindow(*bad)), 16, C.byref(rows)) == ERR_INVALID
        assert rows.value == -7
    assert lib.asr_attn_stream_plan(None, 16, C.byref(rows)) == ERR_INVALID
    assert lib.asr_attn_stream_plan(C.byref(L.AttnWindow(4, 8, 0)), 0, C.byref(rows)) == ERR_INVALID

    def args(**kw):
        a = L.AttnStreamArgs()
        a.Tq, a.N, a.n_pad, a.heads, a.dh = 16, 1, 16, 2, 16
        a.ld, a.ld_kv, a.ld_out, a.R, a.t0, a.P, a.ld_pos, a.scale = 96, 64, 32, 128, 0, 12, 32, 0.25
        for k in ('q', 'ring', 'kv_len', 'pos', 'bias_u', 'bias_v'):
            setattr(a, k, base)
        a.out = base + 4096
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    good = L.AttnWindow(4, 8, 0)
    for fwd in (lib.asr_attn_stream_fwd, lib.asr_relattn_stream_fwd):
        for w in (L.AttnWindow(4, -1, 0), L.AttnWindow(4, 8, 1), L.AttnWindow(0, 8, 0)):
            assert fwd(C.byref(args()), C.byref(w), None) == ERR_INVALID
            assert b'window' in lib.asr_last_error()
        assert fwd(C.byref(args()), None, None) == ERR_INVALID
        for kw in (dict(Tq=0), dict(dh=24), dict(ld_kv=60), dict(t0=-1), dict(kv_len=None),
                   dict(q=base + 4)):
            assert fwd(C.byref(args(**kw)), C.byref(good), None) == ERR_INVALID, kw
        # the ring: not a multiple of 64, and too small for the call (t0 100, lo 88, tile 64)
        for kw in (dict(R=100), dict(R=64, t0=100, Tq=32)):
            assert fwd(C.byref(args(**kw)), C.byref(good), None) == ERR_INVALID, kw
            assert b'ring' in lib.asr_last_error()
    assert lib.asr_relattn_stream_fwd(C.byref(args(P=11)), C.byref(good), None) == ERR_INVALID
    assert b'table' in lib.asr_last_error()
    assert lib.asr_relattn_stream_fwd(C.byref(args(dh=80, ld=240, ld_kv=320, ld_out=160,
                                                   ld_pos=160)), C.byref(good), None) == ERR_INVALID
    # the convolution: T, N, n_pad, C, ld, k, ring rows, t0
    dw = lambda *geo: lib.asr_dwconv1d_stream_fwd(base, base, base, base, base + 4096, *geo, None)
    assert dw(8, 1, 16, 4, 4, 3, 9, 0) == ERR_INVALID and b'ring' in lib.asr_last_error()
    assert dw(8, 1, 16, 4, 4, 4, 16, 0) == ERR_INVALID
    assert dw(8, 1, 16, 4, 4, 3, 16, -1) == ERR_INVALID
    assert lib.asr_dwconv1d_stream_fwd(base, base, base, None, base + 4096, 8, 1, 16, 4, 4, 3, 16,
                                       0, None) == ERR_INVALID
    # ring_put: Tq, n_pad, ld_src, col0, cols, ld_ring, ring rows, t0
    put = lambda *geo: lib.asr_ring_put(base, base + 4096, *geo, None)
    for geo in ((0, 16, 8, 0, 8, 8, 4, 0), (5, 16, 8, 0, 8, 8, 4, 0), (4, 16, 8, 4, 8, 8, 4, 0),
                (4, 16, 8, 0, 6, 8, 4, 0), (4, 16, 8, 0, 8, 4, 4, 0), (4, 16, 8, 0, 8, 8, 4, -1)):
        assert put(*geo) == ERR_INVALID, geo
    assert lib.asr_ring_put(base, base, 4, 16, 8, 0, 8, 8, 4, 0, None) == ERR_INVALID
    assert lib.asr_ctc_greedy_stream(base, base, None, 4, 1, 16, 5, base, base, None) == ERR_INVALID
    assert lib.asr_ctc_greedy_stream(base, base, base, 0, 1, 16, 5, base, base, None) == ERR_INVALID


# ----------------------------------------------------------------------------- Model.stream
SMALL = dict(num_features=16, num_classes=7, d_model=32, num_heads=2, num_layers=2, d_ff=64,
             dropout=0, conv=False, device='cpu', kernel_size=7, conv_norm='layer')


@pytest.mark.parametrize('kw,stage,word', [
    (dict(context=None, causal_conv=True), 'mha', 'window'),
    (dict(context='causal', causal_conv=True), 'mha', 'left'),
    (dict(context=(4, 8, 1), causal_conv=True), 'mha', 'right'),
    (dict(context=(4, 8, 0), causal_conv=False), 'dwconv', 'causal'),
])
def test_models_that_cannot_stream_are_refused_before_a_device_call(kw, stage, word):
    from asr_study_amd.core import models
    model = models.conformer(**dict(SMALL, **kw))
    with pytest.raises(ValueError) as e:
        model.stream()
    assert '(%s)' % stage in str(e.value) and word in str(e.value), str(e.value)
    assert re.search(r'stage \d+', str(e.value))


def test_recurrent_models_and_beam_decoders_are_refused():
    from asr_study_amd.core import models
    with pytest.raises(ValueError) as e:
        models.brsmv1(num_features=16, num_hiddens=8, num_layers=1, device='cpu').stream()
    assert 'bilstm' in str(e.value)
    model = models.conformer(**dict(SMALL, context=(4, 8, 0), causal_conv=True))
    model.decoder = dict(is_greedy=False, beam_width=8)
    with pytest.raises(NotImplementedError):
        model.stream()
    model.decoder = dict(is_greedy=True)
    for step in (0, 6, -4):
        with pytest.raises(ValueError):
            model.stream(step=step)
    assert model.stream().step == 16 and model.stream(step=8).step == 8
    assert model.stream(n_streams=3).n_pad == 16
    one = models.transformer(**dict({k: v for k, v in SMALL.items() if k not in
                                     ('kernel_size', 'conv_norm')}, context=(1, 5, 0)))
    assert one.stream().step == 16          # 16 one-frame chunks per launch
    assert models.transformer(**dict({k: v for k, v in SMALL.items() if k not in
                                      ('kernel_size', 'conv_norm')},
                                     context=(7, 3, 0))).stream().step == 21
    # a front-end the session cannot window: one convolution only
    with pytest.raises(ValueError) as e:
        models.conformer(**dict(SMALL, conv=True, conv_filters=4, conv_kernels=((5, 7),),
                                context=(4, 8, 0), causal_conv=True)).stream()
    assert 'front-end' in str(e.value)


# ----------------------------------------------------------------------------- emission
def _reach(t, step, front):
    """The reach formula of the transformer factory's docstring: strided frame t waits for input frame 2 (c_end - 1 + (kt2 - 1) // 2)
    + kt1 - 1 - p1, p1 = (kt1 - 2) // 2, c_end the end of t's step; without a front-end for the
    last frame of its step."""
    c_end = (t // step + 1) * step
    if front is None:
        return c_end - 1
    kt1, kt2 = front
    return 2 * (c_end - 1 + (kt2 - 1) // 2) + kt1 - 1 - (kt1 - 2) // 2


@pytest.mark.parametrize('front', [None, (5, 3), (11, 11), (4, 1)])
@pytest.mark.parametrize('step', [1, 4, 16])
def test_emitted_frames_follow_the_reach_formula(front, step):
    from asr_study_amd.core.stream import Schedule
    sc = Schedule(step, front)
    for pieces in ([3, 22, 1, 30, 24], [1, 7, 13, 3, 16], [1] * 50, [80]):
        fed = emitted = 0
        for p in pieces:
            fed += p
            want = 0
            while _reach(want, step, front) < fed:      # every frame of the step has arrived
                want += 1
            want = want // step * step
            emitted = sc.ready(fed, emitted)
            assert emitted == want, (front, step, fed)
            assert all(sc.reach(t) == _reach(t, step, front) for t in range(want + step))
        assert sc.total(fed) == (fed if front is None else -(-fed // 2)) >= emitted
    if front is not None:       # the window: even start, the step's rows clear of both edges
        kt1, kt2 = front
        p1, l2 = (kt1 - 2) // 2, (kt2 - 1) // 2
        for c0 in (0, step, 5 * step):
            w0 = sc.window_start(c0)
            assert w0 % 2 == 0
            first, last = c0 - l2, c0 + step - 1 + (kt2 - 1 - l2)       # rows of convolution 1
            assert w0 <= 2 * first - p1
            assert 2 * last - p1 + kt1 - 1 <= w0 + 2 * sc.rows1 - 1
            assert first - w0 // 2 == sc.keep - l2 and sc.rows1 >= sc.keep + step


def test_the_session_uses_the_schedule_of_its_front_end(on_cpu):
    model = _model('conformer', (4, 8, 0), num_features=16, conv=True, conv_filters=4,
                   conv_kernels=((5, 7), (3, 5)))
    ss = model.stream()
    assert ss.schedule.front == (5, 3) and ss.step == 16 and ss.schedule.stride == 2
    assert [model.stages[i].kind for i in range(ss.enc0)][-1] == 'conv'
    assert ss.frames_in == ss.frames_out == 0
    plain = _model('conformer', (4, 8, 0)).stream(step=4)
    assert plain.schedule.front is None and plain.enc0 == 0


# ----------------------------------------------------------------------------- the surface
def test_new_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(ROOT, 'include', 'asr_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in L.SIGNATURES, name
        assert name in open(os.path.join(ROOT, 'DESIGN.md')).read(), name
    assert re.search(r'typedef struct asr_attn_stream_args \{', code)
    ints = ['Tq', 'N', 'n_pad', 'heads', 'dh', 'ld', 'ld_kv', 'ld_out', 'R', 't0', 'P', 'ld_pos']
    assert [f[0] for f in L.AttnStreamArgs._fields_] == ints + [
        'scale', 'q', 'ring', 'kv_len', 'out', 'pos', 'bias_u', 'bias_v']
    assert C.sizeof(L.AttnStreamArgs) == 4 * 13 + 4 + 8 * 7
    assert lib.asr_version() == L.ABI_VERSION == 107                # additions only
    from asr_study_amd import ops
    for name in ('ring_put', 'attn_stream_plan', 'attn_stream_fwd', 'relattn_stream_fwd',
                 'dwconv1d_stream_fwd', 'ctc_greedy_stream'):
        assert callable(getattr(ops, name))


def test_kind_table_keeps_every_entry():
    from asr_study_amd.core import stages as S
    old = ('build', 'forward', 'backward', 'mask_shape', 'needs_lens', 'attention', 'needs_in_len',
           'extra_timeout_flags')
    assert S.Kind._fields == old + ('stream',)
    assert S.Kind(1, 2, 3) == S.Kind(1, 2, 3, None, False, False, False, False, None)
    assert sorted(S.KINDS) == sorted(['noise', 'dropout', 'reshape', 'specaug', 'act', 'glu',
                                      'posenc', 'merge', 'dense', 'conv', 'dwconv', 'bn', 'ln',
                                      'mha', 'bilstm', 'birnn', 'bigru', 'birhn'])
    want = {'noise': (S._noise_build, S._noise_forward, S._pass_through),
            'dense': (S._dense_build, S._dense_forward, S._dense_backward),
            'posenc': (S._posenc_build, S._posenc_forward, S._pass_through),
            'dwconv': (S._dwconv_build, S._dwconv_forward, S._dwconv_backward),
            'mha': (S._mha_build, S._mha_forward, S._mha_backward),
            'bilstm': (S._bilstm_build, S._bilstm_forward, S._bilstm_backward)}
    for name, fns in want.items():
        assert S.KINDS[name][:3] == fns
    flags = {k: tuple(v[4:8]) for k, v in S.KINDS.items()}
    assert flags['mha'] == (True, True, False, False) and flags['dwconv'] == (True, False, False, False)
    assert flags['specaug'] == (False, False, True, False) and flags['birnn'] == (False, False, False, True)
    assert all(f == (False,) * 4 for k, f in flags.items()
               if k not in ('mha', 'dwconv', 'specaug', 'birnn'))
    assert sorted(k for k, v in S.KINDS.items() if v.stream is not None) == ['dwconv', 'mha', 'posenc']
    assert all(S.KINDS[k].stream is None for k in S.STREAM_AS_FORWARD)
