"""Time reduction by frame stacking (K33) without a GPU: the oracle is an exact adjoint pair, the
TimeReduction layer and its stage (the 'treduce' variant of the reshape kind), the six factories'
``time_reduction`` argument, the engine's time axes, the refusals, the C ABI's argument checks."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import time_reduction_oracle as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('asr_time_stack_fwd', 'asr_time_stack_bwd')


# ---------------------------------------------------------------- oracle
@pytest.mark.parametrize('T,k', [(1, 2), (2, 2), (3, 2), (7, 3), (9, 4), (17, 8), (16, 8)])
@pytest.mark.parametrize('with_lens', [False, True])
def test_oracle_is_an_exact_adjoint_pair(T, k, with_lens):
    """<y, S x> == <S^T y, x> on integer-valued data: every product and sum is exact."""
    rs = np.random.RandomState(100 * T + k)
    N, F = 5, 3
    lens = np.array([T, 1, 0, max(1, T - 1), (T // k) * k + 1 if (T // k) * k + 1 <= T else T])
    lens = lens if with_lens else None
    x = rs.randint(-9, 10, size=(T, N, F)).astype(np.float64)
    y = rs.randint(-9, 10, size=(TR.out_frames(T, k), N, k * F)).astype(np.float64)
    Sx, Sty = TR.stack(x, k, lens), TR.unstack(y, k, T, lens)
    assert Sx.shape == y.shape and Sty.shape == x.shape
    assert float((y * Sx).sum()) == float((Sty * x).sum())
    # S^T S is the projection onto the valid frames
    valid = TR._valid(T, N, lens)[:, :, None]
    assert np.array_equal(TR.unstack(Sx, k, T, lens), np.where(valid, x, 0))
    # element by element: y[to, n, j F + f] = x[to k + j, n, f]
    for to in range(Sx.shape[0]):
        for j in range(k):
            t = to * k + j
            for n in range(N):
                ok = t < T and (lens is None or t < lens[n])
                want = x[t, n] if ok else np.zeros(F)
                assert np.array_equal(Sx[to, n, j * F:(j + 1) * F], want)


def test_oracle_slab_form_writes_every_pad_as_zero():
    rs = np.random.RandomState(0)
    T, N, n_pad, F, ld_in, ld_out, k = 7, 3, 16, 5, 8, 16, 3
    x = rs.randn(T, n_pad, ld_in)
    x[:, :, F:] = np.nan                    # (never read)
    lens = [7, 4, 0]
    y = TR.stack_slab(x, lens, N, F, ld_out, k)
    assert y.shape == (3, n_pad, ld_out) and np.isfinite(y).all()
    assert not y[:, :, k * F:].any() and not y[:, 2].any()
    assert np.array_equal(y[1, 1, :F], x[3, 1, :F]) and not y[1, 1, F:].any()   # len 4: frame 3 only
    assert np.array_equal(y[2, 5, :F], x[6, 5, :F])         # a row n >= N: every frame
    dy = rs.randn(*y.shape)
    dy[:, :, k * F:] = np.nan
    dx = TR.unstack_slab(dy, lens, N, T, F, ld_in, k)
    assert dx.shape == x.shape and np.isfinite(dx).all()
    assert not dx[:, :, F:].any() and not dx[4:, 1].any() and not dx[:, 2].any()
    assert np.array_equal(dx[3, 1, :F], dy[1, 1, :F])


# ---------------------------------------------------------------- layer, stage, config
def test_layer_widths_and_refusals():
    from asr_study_amd.core import layers as L
    x = L.Input(name='inputs', shape=(None, 39))
    for k in range(2, 9):
        assert L.TimeReduction(k)(x).features == 39 * k
    for bad in (1, 9, 0, -2, 2.5, True):
        with pytest.raises(NotImplementedError, match='factor'):
            L.TimeReduction(bad)
    with pytest.raises(NotImplementedError, match='unknown arguments'):
        L.TimeReduction(2, mode='mean')
    assert 'concatenat' in L.TimeReduction.__doc__


def _chain(build, features=8, **kw):
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import ctc_model
    x = L.Input(name='inputs', shape=(None, features))
    return ctc_model(x, build(L, x), device='cpu', **kw)


def test_stage_is_the_treduce_variant_of_reshape():
    from asr_study_amd.core.stages import KINDS, time_factor
    m = _chain(lambda L, x: L.TimeDistributed(L.Dense(6))(L.TimeReduction(3)(x)), features=39)
    assert m.spec[0] == {'type': 'reshape', 'target': [-1, 117], 'time_factor': 3}
    s = m.stages[0]
    assert (s.kind, time_factor(s), s.f_in, s.f_in_pad, s.f_out, s.f_out_pad) == \
        ('reshape', 3, 39, 40, 117, 120)
    assert not s.tensors and s.first and m.stages[1].first
    assert m.stages[1].f_in_pad == 120 and m.time_strides == [3] and m._treduce
    assert KINDS['reshape'].forward is not None and 'treduce' not in KINDS
    # a plain Reshape carries no such attribute and is no stride
    m = _chain(lambda L, x: L.TimeDistributed(L.Dense(6))(L.Reshape((-1, 8))(x)))
    assert not hasattr(m.stages[0], 'time_factor') and m.time_strides == [] and not m._treduce


def test_build_time_refusals_name_their_reason():
    def spans(L, x):
        a = L.TimeDistributed(L.Dense(16))(x)
        b = L.TimeReduction(2)(a)
        c = L.TimeDistributed(L.Dense(16))(b)
        return L.Merge('sum', a)(c)
    with pytest.raises(ValueError, match='spans a TimeReduction.*different time axes'):
        _chain(spans)

    def conv_behind(L, x):
        o = L.TimeReduction(2)(x)
        o = L.Reshape((-1, 16, 1))(o)
        return L.Convolution2D(4, 3, 3, subsample=(1, 2))(o)
    with pytest.raises(ValueError, match='conv stage behind a TimeReduction'):
        _chain(conv_behind)

    def specaug_behind(L, x):
        return L.SpecAugment()(L.TimeReduction(2)(x))
    with pytest.raises(ValueError, match='SpecAugment behind a TimeReduction'):
        _chain(specaug_behind)

    def padded_apart(L, x):      # H = 10: the two directions sit at columns 0 and 12
        return L.TimeReduction(2)(L.Bidirectional(L.LSTM(10))(x))
    with pytest.raises(NotImplementedError, match='padded apart.*multiple of 4'):
        _chain(padded_apart)
    # a merge on one side of the stage is fine
    def one_side(L, x):
        a = L.TimeDistributed(L.Dense(16))(L.TimeReduction(2)(x))
        b = L.TimeDistributed(L.Dense(16))(a)
        return L.merge([b, a], mode='sum')
    assert [s.kind for s in _chain(one_side).stages] == ['reshape', 'dense', 'dense', 'merge']


def test_keras_config_round_trip(monkeypatch):
    from asr_study_amd.core import engine, models
    from asr_study_amd.utils import keras_config as K
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = models.brsmv1(num_features=13, num_classes=6, num_hiddens=8, num_layers=3,
                      time_reduction=[[0, 3], [2, 2]], residual='sum', device='cpu')
    text = K.model_config(m)
    layers = [l for l in json.loads(text)['config']['layers'] if l['class_name'] == 'TimeReduction']
    assert [(l['name'], l['config']['factor']) for l in layers] == \
        [('timereduction_1', 3), ('timereduction_2', 2)]
    m2 = K.topology_from_config(text)
    assert m2.spec == m.spec and m2.time_strides == [3, 2]
    assert [a.shape for a in m2.get_weights()] == [a.shape for a in m.get_weights()]
    assert K.model_config(m2) == text


# ---------------------------------------------------------------- factories
def _kinds(m):
    from asr_study_amd.core.stages import time_factor
    return [('treduce%d' % time_factor(s)) if time_factor(s) else s.kind for s in m.stages]


def test_brsmv1_and_deep_speech2_place_the_stage():
    from asr_study_amd.core import models
    kw = dict(num_features=39, num_classes=6, num_hiddens=16, num_layers=3, device='cpu')
    m = models.brsmv1(time_reduction=[[1, 2], [2, 2]], **kw)
    assert _kinds(m) == ['noise', 'bilstm', 'treduce2', 'bilstm', 'treduce2', 'bilstm', 'dense']
    assert [s.f_in for s in m.stages if s.kind == 'bilstm'] == [39, 64, 64]
    assert m.config['kwargs']['time_reduction'] == [[1, 2], [2, 2]]
    m = models.brsmv1(time_reduction=[[0, 3]], bidirectional=False, **kw)
    assert _kinds(m) == ['noise', 'treduce3', 'bilstm', 'bilstm', 'bilstm', 'dense']
    assert m.stages[2].f_in == 117 and m.stages[2].f_in_pad == 120
    m = models.brsmv1(time_reduction=[[1, 2]], residual='sum', **kw)
    assert _kinds(m) == ['noise', 'dense', 'bilstm', 'merge', 'treduce2', 'dense', 'bilstm', 'merge',
                         'bilstm', 'merge', 'dense']
    assert (m.stages[4].f_out, m.stages[5].n_out, m.stages[7].skip) == (64, 32, 5)
    assert 'time_reduction' not in models.brsmv1(**kw).config['kwargs']
    for rnn_type, bn, bi in (('lstm', False, True), ('gru', False, True), ('gru', 'recurrent', True),
                             ('gru', True, False), ('lstm', 'layer', True)):
        d = models.deep_speech2(num_features=16, num_classes=6, num_hiddens=8, num_layers=2,
                                conv_filters=4, rnn_type=rnn_type, batch_norm=bn,
                                bidirectional=bi, time_reduction=[[0, 2], [1, 3]], device='cpu')
        rec = 'bigru' if rnn_type == 'gru' else 'bilstm'
        k = [x for x in _kinds(d) if x in (rec, 'treduce2', 'treduce3')]
        assert k == ['treduce2', rec, 'treduce3', rec], (rnn_type, bn, bi, _kinds(d))
        assert d.time_strides == [2, 2, 3] and d.config['kwargs']['time_reduction'] == [[0, 2], [1, 3]]
        if bn in (True, 'layer'):       # the stage goes in front of the layer's normalisation
            i = _kinds(d).index('treduce2')
            assert d.stages[i + 1].kind in ('bn', 'ln') and d.stages[i + 2].kind == rec
    assert 'time_reduction' not in models.deep_speech2(
        num_features=16, num_classes=6, num_hiddens=8, num_layers=1, conv_filters=4,
        device='cpu').config['kwargs']


def test_transformer_and_conformer_place_the_stage():
    from asr_study_amd.core import models
    kw = dict(num_features=16, num_classes=6, d_model=32, num_heads=2, num_layers=1, device='cpu')
    for factory in (models.transformer, models.conformer):
        m = factory(time_reduction=2, **kw)
        i = _kinds(m).index('treduce2')
        assert m.stages[i - 1].kind == 'reshape' and m.stages[i + 1].kind == 'dense'
        assert m.stages[i + 1].n_out == 32 and m.stages[i].f_out == 2 * m.stages[i].f_in
        assert m.time_strides == [2, 2] and m.config['kwargs']['time_reduction'] == 2
        assert m._needs_lens
        m = factory(time_reduction=3, conv=False, **kw)
        assert _kinds(m)[:2] == ['treduce3', 'dense'] and m.time_strides == [3]
        assert 'time_reduction' not in factory(**kw).config['kwargs']
        assert 'REDUCED' in factory.__doc__
        with pytest.raises(ValueError, match='one integer factor'):
            factory(time_reduction=[[0, 2]], **kw)


def test_transducer_and_aed_forward_the_argument():
    from asr_study_amd.core import models
    t = models.transducer(num_features=8, num_classes=6, encoder='lstm', num_hiddens=8,
                          num_layers=2, joint_dim=8, pred_hiddens=8, time_reduction=[[1, 2]],
                          device='cpu')
    assert _kinds(t.encoder) == ['noise', 'bilstm', 'treduce2', 'bilstm', 'dense']
    assert t.encoder.time_strides == [2] and t.config['kwargs']['time_reduction'] == [[1, 2]]
    a = models.aed(num_features=8, num_classes=6, encoder='blstm', num_hiddens=8, num_layers=3,
                   d_att=16, num_heads=1, pred_hiddens=8, time_reduction=[[1, 2], [2, 2]],
                   device='cpu')
    assert _kinds(a.encoder) == ['noise', 'bilstm', 'treduce2', 'bilstm', 'treduce2', 'bilstm',
                                 'dense']
    assert a.encoder.out_frames(37) == 10 and a.config['kwargs']['time_reduction'] == [[1, 2], [2, 2]]
    c = models.aed(num_features=16, num_classes=6, encoder='conformer', num_layers=1, d_att=16,
                   num_heads=1, pred_hiddens=8, d_model=64, time_reduction=2, device='cpu')
    assert c.encoder.time_strides == [2, 2]
    assert 'time_reduction' in models.transducer.__doc__ and 'pyramid' in models.aed.__doc__


def test_time_axes_compose_as_ceil_divisions():
    import torch
    from asr_study_amd.core import models
    m = models.deep_speech2(num_features=16, num_classes=6, num_hiddens=8, num_layers=2,
                            conv_filters=4, time_reduction=[[0, 2], [1, 3]], device='cpu')
    assert m.time_strides == [2, 2, 3]
    assert m.out_frames(37) == 4                    # 37 -> 19 -> 10 -> 4
    lens = np.array([37, 36, 13, 12, 1])
    want = -(-(-(-(-(-lens // 2)) // 2)) // 3)
    assert m.out_lengths(lens).tolist() == want.tolist() == [4, 3, 2, 1, 1]
    assert m.out_lengths(torch.as_tensor(lens, dtype=torch.int32)).tolist() == want.tolist()
    assert int(np.prod(m.time_strides)) == 12       # what Model.align reports as time_stride
    axes = m._axis_lens(torch.as_tensor(lens, dtype=torch.int32), None)
    assert [a.tolist() for a in axes] == [lens.tolist(), [19, 18, 7, 6, 1], [10, 9, 4, 3, 1],
                                          want.tolist()]
    assert m._axis_lens(None, None) == [None] * 4
    with pytest.raises(ValueError, match='in_len.*cannot be inverted'):
        m._axis_lens(None, torch.as_tensor(want, dtype=torch.int32))
    # which axis every stage runs on: 0 up to the strided convolution, ... 3 behind the last
    kinds = _kinds(m)
    assert m._axis_of[kinds.index('conv')] == 0 and m._axis_of[kinds.index('treduce2')] == 1
    assert m._axis_of[kinds.index('treduce3')] == 2 and m._axis_of[-1] == 3
    assert m._input_lens(lens).dtype == torch.int32
    plain = models.brsmv1(num_features=8, num_classes=6, num_hiddens=8, num_layers=1, device='cpu')
    assert plain._input_lens(lens) is None and not plain._treduce


@pytest.mark.parametrize('bad', [[[3, 2]], [[1, 2], [1, 2]], [[2, 2], [1, 2]], [[-1, 2]], 5, [],
                                 [[1]], [[0, 2.5]], 'x'])
def test_bad_after_layer_lists_are_refused(bad):
    from asr_study_amd.core import models
    with pytest.raises(ValueError, match='time_reduction'):
        models.brsmv1(num_features=8, num_classes=6, num_hiddens=8, num_layers=3,
                      time_reduction=bad, device='cpu')


def test_factor_outside_the_kernels_limits_is_refused():
    from asr_study_amd.core import models
    for k in (1, 9):
        with pytest.raises(NotImplementedError, match='factor'):
            models.brsmv1(num_features=8, num_classes=6, num_hiddens=8, num_layers=3,
                          time_reduction=[[1, k]], device='cpu')


def test_stream_check_names_the_stage():
    from asr_study_amd.core import models, stream
    from asr_study_amd.core.stages import stream_check
    m = models.brsmv1(num_features=8, num_classes=6, num_hiddens=8, num_layers=2,
                      bidirectional=False, time_reduction=[[1, 2]], device='cpu')
    assert [stream_check(m, s, i) is None for i, s in enumerate(m.stages)] == \
        [True, True, False, True, True]
    assert 'one time axis' in stream_check(m, m.stages[2], 2)
    with pytest.raises(ValueError, match=r'stage 2 \(reshape\) cannot stream: it is a '
                                         r'TimeReduction stage.*one time axis'):
        stream.check(m, None)
    # the same stack without the stage streams
    stream.check(models.brsmv1(num_features=8, num_classes=6, num_hiddens=8, num_layers=2,
                               bidirectional=False, device='cpu'), None)


def test_command_line_value_parses_like_context():
    from asr_study_amd.utils.hparams import HParams
    got = HParams().parse(['encoder', 'blstm', 'time_reduction', '[[1, 2], [2, 2]]']).values()
    assert got == {'encoder': 'blstm', 'time_reduction': [[1, 2], [2, 2]]}


# ---------------------------------------------------------------- C ABI
def test_symbols_declared_exported_and_bound():
    from asr_study_amd import _lib, build, ops
    with open(os.path.join(ROOT, 'include', 'asr_hip.h')) as f:
        header = f.read()
    assert 'timestack.hip' in build.SOURCES
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r'\bint %s\(' % name, header), name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args) and len(args) == 11
    assert _lib.ABI_VERSION == 107 and lib.asr_version() == 107        # additions only
    assert callable(ops.time_stack_fwd) and callable(ops.time_stack_bwd)
    assert ops.TIME_STACK_FACTORS == (2, 8) and ops.time_stack_frames(37, 3) == 13


def test_c_abi_argument_checks_without_a_device():
    """Every refusal is decided on the host, before anything is launched."""
    from asr_study_amd import _lib
    lib = _lib.load()
    good = dict(T=7, N=3, n_pad=16, F=8, ld_in=8, ld_out=16, k=2)
    order = ('T', 'N', 'n_pad', 'F', 'ld_in', 'ld_out', 'k')
    a, b = C.c_void_p(16), C.c_void_p(32)      # aligned non-NULL pointers nothing dereferences
    for key, v in (('k', 1), ('k', 9), ('k', 0), ('k', -2), ('F', 0), ('F', -4), ('ld_in', 4),
                   ('ld_out', 12), ('ld_in', 10), ('ld_out', 18), ('n_pad', 8), ('n_pad', 24),
                   ('n_pad', 0), ('N', 0), ('N', 17), ('N', -1), ('T', 0)):
        args = [dict(good, **{key: v})[n] for n in order]
        for fn in (lib.asr_time_stack_fwd, lib.asr_time_stack_bwd):
            assert fn(a, None, b, *args, None) == -1, (key, v)
            assert 'time_stack' in lib.asr_last_error().decode()
    # F = 5 in ld_in = 8: ld_out must hold k F = 15 -> 16; 12 is too narrow
    args = [dict(good, F=5, ld_out=12, k=3)[n] for n in order]
    assert lib.asr_time_stack_fwd(a, None, b, *args, None) == -1
    args = [good[n] for n in order]
    for fn in (lib.asr_time_stack_fwd, lib.asr_time_stack_bwd):
        assert fn(None, None, b, *args, None) == -1         # NULL input
        assert fn(a, None, None, *args, None) == -1         # NULL output
        assert fn(a, None, a, *args, None) == -1            # aliased
        assert fn(C.c_void_p(20), None, b, *args, None) == -1       # alignment
        assert fn(a, None, C.c_void_p(36), *args, None) == -1
