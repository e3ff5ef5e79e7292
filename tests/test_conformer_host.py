"""CPU checks of the Conformer feature: the float64 oracle's gradients against central differences
and against torch float64 (which pins the tap direction on third-party code), the masking
properties, the layer validation, the ctc_model spec, parameter layout and Keras names, the Keras
config round trip, the unchanged existing models, and the C ABI's refusals without a device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conformer_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('asr_dwconv1d_workspace_bytes', 'asr_dwconv1d_plan', 'asr_dwconv1d_fwd',
               'asr_dwconv1d_bwd', 'asr_glu_fwd', 'asr_glu_bwd', 'asr_swish_fwd', 'asr_swish_bwd')


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _central(f, arrays, h=1e-5):
    """d f() / d a for every a of `arrays` (perturbed in place), by central differences."""
    out = []
    for a in arrays:
        num = np.zeros_like(a)
        flat, nf = a.reshape(-1), num.reshape(-1)
        for i in range(flat.size):
            old = flat[i]
            flat[i] = old + h
            up = f()
            flat[i] = old - h
            dn = f()
            flat[i] = old
            nf[i] = (up - dn) / (2 * h)
        out.append(num)
    return out


def _dw_case(seed=0, T=9, N=3, C=4, k=5, lens=(9, 1, 6)):
    rs = np.random.RandomState(seed)
    return (rs.randn(T, N, C), rs.randn(k, C) * 0.7, rs.randn(C) * 0.3, np.array(lens),
            rs.randn(T, N, C))


def test_oracle_gradients_match_central_differences():
    x, w, b, lens, R = _dw_case()
    y, c = CO.dwconv_forward(x, w, b, lens)
    got = CO.dwconv_backward(R, c)
    num = _central(lambda: float((CO.dwconv_forward(x, w, b, lens)[0] * R).sum()), [x, w, b])
    for name, g, n in zip(('dx', 'dw', 'db'), got, num):
        err = _rel(g, n)
        print('[conformer] dwconv %s vs central differences: %.2e' % (name, err))
        assert err <= 1e-6, (name, err)
    rs = np.random.RandomState(1)
    xg, Rg = rs.randn(5, 2, 8) * 2.0, rs.randn(5, 2, 4)
    num, = _central(lambda: float((CO.glu_forward(xg)[0] * Rg).sum()), [xg])
    assert _rel(CO.glu_backward(Rg, xg), num) <= 1e-6
    xs, Rs = rs.randn(6, 7) * 3.0, rs.randn(6, 7)
    num, = _central(lambda: float((CO.swish(xs) * Rs).sum()), [xs])
    assert _rel(CO.swish_backward(Rs, xs), num) <= 1e-6


@pytest.mark.parametrize('k', [1, 3, 5, 31])
def test_oracle_matches_torch_float64(k):
    """F.conv1d(groups=C, padding=p) on the masked input and its autograd: the tap direction
    (cross-correlation, tap j reads frame t + j - p) is torch's, not a convention of this
    repository."""
    x, w, b, lens, R = _dw_case(seed=k, T=12, N=3, C=8, k=k, lens=(12, 1, 7))
    y, c = CO.dwconv_forward(x, w, b, lens)
    dx, dw, db = CO.dwconv_backward(R, c)
    xt = torch.tensor(x, requires_grad=True)
    wt = torch.tensor(w, requires_grad=True)
    bt = torch.tensor(b, requires_grad=True)
    mask = torch.tensor(np.arange(12)[:, None] < lens[None, :])[:, :, None]
    xm = torch.where(mask, xt, torch.zeros_like(xt)).permute(1, 2, 0)           # (N, C, T)
    yt = F.conv1d(xm, wt.t().unsqueeze(1), bt, padding=(k - 1) // 2, groups=8).permute(2, 0, 1)
    (yt * torch.tensor(R)).sum().backward()
    for name, g, t in (('y', y, yt.detach()), ('dx', dx, xt.grad), ('dw', dw, wt.grad),
                       ('db', db, bt.grad)):
        err = _rel(g, t.numpy())
        print('[conformer] k=%d dwconv %s vs torch: %.2e' % (k, name, err))
        assert err <= 1e-12, (name, err)


def test_glu_and_swish_match_torch_float64():
    rs = np.random.RandomState(3)
    x = np.concatenate([rs.randn(4, 3, 16) * 4.0,
                        np.tile([100., -100., 20., -20., 0., -0., 1., -1.], (1, 3, 2))])
    R = rs.randn(5, 3, 8)
    xt = torch.tensor(x, requires_grad=True)
    yt = F.glu(xt, dim=-1)
    (yt * torch.tensor(R)).sum().backward()
    assert _rel(CO.glu_forward(x)[0], yt.detach().numpy()) <= 1e-12
    assert _rel(CO.glu_backward(R, x), xt.grad.numpy()) <= 1e-12
    R = rs.randn(*x.shape)
    xt = torch.tensor(x, requires_grad=True)
    yt = F.silu(xt)
    (yt * torch.tensor(R)).sum().backward()
    assert _rel(CO.swish(x), yt.detach().numpy()) <= 1e-12
    assert _rel(CO.swish_backward(R, x), xt.grad.numpy()) <= 1e-12
    assert np.isfinite(CO.swish(x)).all() and np.isfinite(CO.swish_backward(R, x)).all()


def test_masking_properties():
    x, w, b, lens, R = _dw_case(seed=2, T=11, N=3, C=4, k=7, lens=(11, 2, 6))
    y, c = CO.dwconv_forward(x, w, b, lens)
    dx, dw, db = CO.dwconv_backward(R, c)
    junk = x.copy()
    for n in range(3):
        junk[lens[n]:, n] = np.nan                      # a select: not even NaN gets through
    y2, c2 = CO.dwconv_forward(junk, w, b, lens)
    assert np.array_equal(y2, y)                        # (every frame, valid or not)
    dx2, dw2, db2 = CO.dwconv_backward(R, c2)
    assert np.array_equal(dw2, dw) and np.array_equal(dx2, dx)
    for n in range(3):
        assert not dx[lens[n]:, n].any()
        assert dx[:lens[n], n].all()
    # lens = T is lens = None
    assert np.array_equal(CO.dwconv_forward(x, w, b, np.full(3, 11))[0],
                          CO.dwconv_forward(x, w, b, None)[0])
    # an utterance's valid-frame outputs do not change when T grows by padding
    grown = np.concatenate([x, np.random.RandomState(5).randn(6, 3, 4)], axis=0)
    y3, _ = CO.dwconv_forward(grown, w, b, lens)
    for n in range(3):
        assert np.array_equal(y3[:lens[n], n], y[:lens[n], n])
    # ... which the unmasked convolution does not give
    y4, _ = CO.dwconv_forward(grown, w, b, None)
    assert np.abs(y4[:lens[1], 1] - y[:lens[1], 1]).max() > 1e-3


def test_layer_validation(monkeypatch):
    from asr_study_amd.core import engine, layers as L
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    x = L.Input(shape=(None, 48))
    d = L.DepthwiseConvolution1D(31, W_regularizer=L.l2(0.1))
    assert d(x).features == 48 and (d.kernel_size, d.l2) == (31, 0.1)
    assert L.GLU()(x).features == 24
    assert L.Activation('swish').activation == 'swish'
    for k in (0, 2, 30, 65, 3.5):
        with pytest.raises(NotImplementedError, match='kernel_size'):
            L.DepthwiseConvolution1D(k)
    with pytest.raises(NotImplementedError, match='multiple of 4'):
        L.DepthwiseConvolution1D(3)(L.Input(shape=(None, 10)))
    with pytest.raises(NotImplementedError, match='multiple of 8'):
        L.GLU()(L.Input(shape=(None, 12)))
    with pytest.raises(NotImplementedError):
        L.DepthwiseConvolution1D(3, dilation=2)
    # the same limits on a spec that did not come through the layer classes
    for spec, feats, match in (([{'type': 'dwconv', 'k': 4}], 8, 'kernel_size'),
                               ([{'type': 'dwconv', 'k': 65}], 8, 'kernel_size'),
                               ([{'type': 'dwconv', 'k': 3}], 10, 'multiple of 4'),
                               ([{'type': 'glu'}], 12, 'multiple of 8')):
        with pytest.raises(NotImplementedError, match=match):
            engine.Model(spec, feats, device='cpu')
    # swish stays an Activation: no recurrent layer takes it
    with pytest.raises(NotImplementedError):
        L.SimpleRNN(8, activation='swish')
    from asr_study_amd import ops
    assert 'swish' not in ops.RNN_ACTIVATIONS
    with pytest.raises(NotImplementedError):
        ops.rnn_activation_id('swish')
    a, b = L.Input(shape=(None, 8)), L.Input(shape=(None, 8))
    for mode in ('mul', 'concat', None):
        with pytest.raises(NotImplementedError, match='merge mode'):
            L.merge([a, b], mode=mode)
    with pytest.raises(NotImplementedError, match='scale'):
        L.merge([a, b], mode='ave', scale=0.5)
    assert L.merge([a, b], mode='sum', scale=0.5).producer.scale == 0.5
    assert L.merge([a, b], mode='sum').producer.scale == 1.0


def _small(conv_norm='batch', conv=True, device='cpu', **kw):
    from asr_study_amd.core.models import conformer
    return conformer(num_features=16, num_classes=7, d_model=32, num_heads=2, num_layers=2,
                     d_ff=64, kernel_size=7, conv_norm=conv_norm, dropout=0.1, conv=conv,
                     conv_filters=4, conv_kernels=((5, 7), (3, 5)), weight_decay=1e-4,
                     device=device, **kw)


@pytest.mark.parametrize('conv_norm', ['batch', 'layer'])
def test_conformer_spec_layout_and_names(monkeypatch, conv_norm):
    from asr_study_amd.core import engine
    from asr_study_amd.core.callbacks import keras_layers
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = _small(conv_norm)
    norm = 'bn' if conv_norm == 'batch' else 'ln'
    ffn = ['ln', 'dense', 'act', 'dense', 'dropout', 'merge']
    block = ffn + ['ln', 'mha', 'dropout', 'merge'] + \
        ['ln', 'dense', 'glu', 'dwconv', norm, 'act', 'dense', 'dropout', 'merge'] + ffn + ['ln']
    front = ['reshape', 'conv', 'conv', 'reshape']
    assert [s.kind for s in m.stages] == front + ['dense', 'posenc', 'dropout'] + 2 * block + \
        ['dense']
    b0 = len(front) + 3                                 # first stage of block 0
    assert m.spec[b0 + 5] == {'type': 'merge', 'mode': 'sum', 'skip': b0 - 1, 'scale': 0.5}
    assert m.spec[b0 + 9] == {'type': 'merge', 'mode': 'sum', 'skip': b0 + 5}
    assert m.spec[b0 + 12] == {'type': 'glu'}
    assert m.spec[b0 + 13] == {'type': 'dwconv', 'k': 7, 'l2': 1e-4}
    assert m.spec[b0 + 2] == {'type': 'act', 'activation': 'swish', 'wrapped': False}
    assert m.spec[b0 + 18] == {'type': 'merge', 'mode': 'sum', 'skip': b0 + 9}
    assert m.spec[b0 + 24] == {'type': 'merge', 'mode': 'sum', 'skip': b0 + 18, 'scale': 0.5}
    assert [s.scale for s in m.stages if s.kind == 'merge'] == [0.5, 1.0, 1.0, 0.5] * 2
    assert m._needs_lens and m._has_mha and m.time_strides == [2]
    s = m.stages[b0 + 13]
    assert (s.k, s.C, s.f_in, s.f_out, s.l2) == (7, 32, 32, 32, 1e-4)
    # in front of a BatchNormalization the bias gradient is identically 0 and is not produced
    assert s.bias_dead == (conv_norm == 'batch')
    assert (m.stages[b0 + 11].n_out, m.stages[b0 + 12].C, m.stages[b0 + 12].f_out) == (64, 32, 32)
    # the parameter table: W (k, C) then b (C), glorot with fan_in = fan_out = k, l2 on W only
    tensors = [t for st in m.stages for t in st.tensors]
    w = m.get_weights()
    iw = [i for i, t in enumerate(tensors) if t.layer == 'depthwiseconvolution1d']
    assert len(iw) == 4 and [tensors[i].name for i in iw] == ['W', 'b', 'W', 'b']
    assert w[iw[0]].shape == (7, 32) and w[iw[1]].shape == (32,)
    lim = np.sqrt(3.0 / 7)
    assert 0.9 * lim < np.abs(w[iw[0]]).max() <= lim and not w[iw[1]].any()
    assert (s.oW % 4, s.ob) == (0, s.oW + 7 * 32) and s.p_lo == s.oW and s.p_hi == s.ob + 32
    l2 = {off: c for off, n, c in m._segments}
    assert (l2[s.oW], l2[s.ob]) == (1e-4, 0.0)
    rs = np.random.RandomState(0)
    w2 = [rs.rand(*a.shape).astype(np.float32) + 0.5 for a in w]
    m.set_weights(w2)
    assert all(np.array_equal(a, b) for a, b in zip(w2, m.get_weights()))
    host = m.params.numpy()
    assert np.array_equal(host[s.oW:s.oW + 7 * 32].reshape(7, 32), w2[iw[0]])   # tap major
    assert np.array_equal(host[s.ob:s.ob + 32], w2[iw[1]])
    names = [n for n, _ in keras_layers(m, w2)]
    assert [n for n in names if n.startswith('depthwise')] == ['depthwiseconvolution1d_1',
                                                                'depthwiseconvolution1d_2']
    layers = dict(keras_layers(m, w2))
    assert [n for n, _ in layers['depthwiseconvolution1d_2']] == \
        ['depthwiseconvolution1d_2_W:0', 'depthwiseconvolution1d_2_b:0']
    assert names.count('batchnormalization_1') == (conv_norm == 'batch')
    assert len([n for n in names if n.startswith('layernormalization')]) == \
        (10 if conv_norm == 'batch' else 12)
    assert [a.shape for a in m.get_gradients()] == [a.shape for a in w]
    assert m.config['name'] == 'conformer' and m.config['kwargs']['conv_norm'] == conv_norm
    assert m.config['kwargs']['kernel_size'] == 7
    json.dumps(m.config)


def test_conformer_defaults_and_hparams(monkeypatch):
    from asr_study_amd.core import engine
    from asr_study_amd.core.models import conformer
    from asr_study_amd.utils.generic_utils import get_from_module
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    assert get_from_module('core.models', 'conformer') is conformer     # train.py --model
    d = conformer(device='cpu')
    assert [(s.k, s.C) for s in d.stages if s.kind == 'dwconv'] == [(31, 256)] * 6
    assert [s.kind for s in d.stages].count('bn') == 6
    assert [(s.heads, s.dh) for s in d.stages if s.kind == 'mha'] == [(4, 64)] * 6
    with pytest.raises(ValueError, match='conv_norm'):
        conformer(conv_norm='group', device='cpu')
    with pytest.raises(NotImplementedError, match='kernel_size'):
        conformer(kernel_size=32, device='cpu')
    assert 'relative positional' in conformer.__doc__


@pytest.mark.parametrize('conv_norm', ['batch', 'layer'])
def test_keras_config_round_trip(monkeypatch, conv_norm):
    from asr_study_amd.core import engine
    from asr_study_amd.utils import keras_config as K
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = _small(conv_norm)
    text = K.model_config(m)
    layers = {l['name']: l for l in json.loads(text)['config']['layers']}
    c = layers['depthwiseconvolution1d_1']
    assert c['class_name'] == 'DepthwiseConvolution1D'
    assert c['config']['kernel_size'] == 7 and c['config']['W_regularizer']['l2'] == 1e-4
    assert layers['glu_2']['class_name'] == 'GLU'
    assert layers['merge_1']['config']['scale'] == 0.5
    assert 'scale' not in layers['merge_2']['config']
    assert layers['activation_1']['config']['activation'] == 'swish'
    m2 = K.topology_from_config(text)
    assert m2.spec == m.spec
    assert [a.shape for a in m2.get_weights()] == [a.shape for a in m.get_weights()]
    assert K.model_config(m2) == text


def test_existing_models_unchanged(monkeypatch):
    """The spec and the Keras config text of brsmv1(), deep_speech2() and transformer() are what
    the commit before this feature wrote (tests/golden/conformer_parent_models.json, recorded
    there from that commit): no 'scale' key, nothing else either."""
    from asr_study_amd.core import engine, models
    from asr_study_amd.utils import keras_config as K
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    with open(os.path.join(ROOT, 'tests', 'golden', 'conformer_parent_models.json')) as f:
        golden = json.load(f)
    assert sorted(golden) == ['brsmv1', 'deep_speech2', 'transformer']
    for name in sorted(golden):
        m = getattr(models, name)(device='cpu')
        text = K.model_config(m)
        assert 'scale' not in json.dumps(m.spec) and '"scale"' not in text, name
        assert m.spec == golden[name]['spec'], name
        assert text == golden[name]['model_config'], name
        assert m._needs_lens == (name == 'transformer')
        assert all(s.scale == 1.0 for s in m.stages if s.kind == 'merge')


def test_new_symbols_declared_exported_and_mirrored():
    from asr_study_amd import _lib
    with open(os.path.join(ROOT, 'include', 'asr_hip.h')) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b(int|size_t) %s\(' % name, header), name
        assert name in _lib.SIGNATURES, name
        fn = getattr(lib, name)                         # exported
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        decl = header[header.index(name + '('):]
        assert len(decl[:decl.index(')')].split(',')) == len(args), name
    assert _lib.ABI_VERSION == 107
    assert re.search(r'#define ASR_HIP_ABI_VERSION 107\b', header)
    assert lib.asr_version() == 107


def test_c_abi_argument_checks_without_a_device():
    """Every refusal is decided on the host, before anything is launched."""
    from asr_study_amd import _lib, ops
    lib = _lib.load()
    good = dict(T=130, N=3, n_pad=16, C=8, ld=8, k=31)
    order = ('T', 'N', 'n_pad', 'C', 'ld', 'k')
    p = ops.dwconv1d_plan(130, 16, 8, 31, N=3)
    tiles = -(-130 // p['tile'])
    assert p['tile'] >= 16 and p['blocks'] % tiles == 0 and p['lds'] <= 64 * 1024
    pb = ops.dwconv1d_plan(130, 16, 8, 31, N=3, backward=True)
    assert pb['tile'] == p['tile'] and 0 < pb['blocks'] <= p['blocks'] and pb['lds'] <= 64 * 1024
    assert ops.dwconv1d_plan(500, 64, 256, 63, backward=True)['lds'] <= 64 * 1024
    assert lib.asr_dwconv1d_workspace_bytes(*[good[k] for k in order]) >= (31 + 1) * 16 * 8 * 4
    one = C.c_void_p(16)            # an aligned non-NULL pointer nothing dereferences
    for key, v in (('k', 0), ('k', 2), ('k', 30), ('k', 65), ('k', -1), ('C', 6), ('C', 0),
                   ('ld', 4), ('ld', 10), ('T', 0), ('N', 0), ('N', 17)):
        a = [dict(good, **{key: v})[k] for k in order]
        assert lib.asr_dwconv1d_workspace_bytes(*a) == 0, (key, v)
        assert lib.asr_dwconv1d_plan(*a, 0, None, None, None) == -1, (key, v)
        assert lib.asr_dwconv1d_fwd(one, one, one, None, C.c_void_p(32), *a, None) == -1, (key, v)
        assert lib.asr_dwconv1d_bwd(one, one, one, None, None, one, one, *a, one, 1 << 30,
                                    None) == -1, (key, v)
        assert 'dwconv1d' in lib.asr_last_error().decode()
    a = [good[k] for k in order]
    assert lib.asr_dwconv1d_fwd(None, None, None, None, None, *a, None) == -1   # NULL pointers
    assert lib.asr_dwconv1d_fwd(one, one, None, None, C.c_void_p(32), *a, None) == -1
    assert lib.asr_dwconv1d_fwd(one, one, one, None, one, *a, None) == -1       # y aliases x
    assert lib.asr_dwconv1d_bwd(one, one, one, None, None, None, one, *a, one, 1 << 30,
                                None) == -1                                     # no dw
    assert lib.asr_dwconv1d_fwd(C.c_void_p(20), one, one, None, C.c_void_p(32), *a,
                                None) == -1                                     # alignment
    # GLU: (x, y, rows, C, ld_in, ld_out); swish: (x, y, n)
    for Cc, ld_in, ld_out in ((6, 12, 8), (8, 12, 8), (8, 16, 4), (8, 18, 8), (8, 16, 10),
                              (0, 16, 8)):
        assert lib.asr_glu_fwd(one, C.c_void_p(32), 5, Cc, ld_in, ld_out, None) == -1
        assert lib.asr_glu_bwd(one, C.c_void_p(32), C.c_void_p(48), 5, Cc, ld_in, ld_out,
                               None) == -1
    assert lib.asr_glu_fwd(None, None, 5, 8, 16, 8, None) == -1
    assert lib.asr_glu_fwd(one, C.c_void_p(32), 0, 8, 16, 8, None) == -1
    assert lib.asr_glu_bwd(one, None, None, 5, 8, 16, 8, None) == -1
    assert lib.asr_swish_fwd(None, None, 8, None) == -1
    assert lib.asr_swish_fwd(one, C.c_void_p(32), 0, None) == -1
    assert lib.asr_swish_bwd(one, None, None, 8, None) == -1
    assert lib.asr_swish_bwd(one, C.c_void_p(36), C.c_void_p(48), 8, None) == -1


def test_lengths_are_checked_on_the_host(monkeypatch):
    """A model with a dwconv stage (and no attention) refuses utterance lengths outside 1 .. T
    while they are host arrays."""
    from asr_study_amd.core import engine, layers as L
    from asr_study_amd.core.models import ctc_model
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    x_in = L.Input(name='inputs', shape=(None, 8))
    o = L.DepthwiseConvolution1D(3)(x_in)
    o = L.TimeDistributed(L.Dense(5))(o)
    m = ctc_model(x_in, o, device='cpu')
    assert m._needs_lens and not m._has_mha
    assert m._key_lens([1, 10, 7], 10).tolist() == [1, 10, 7]
    for bad in ([0, 5], [5, 11]):
        with pytest.raises(ValueError, match='inputs_length'):
            m._key_lens(bad, 10)


def test_oracle_walk_scaled_merge_and_bn_bookkeeping(monkeypatch):
    """The oracle's model walk on a small conformer: its gradients against central differences
    of its own loss (through the scaled merge, GLU, dwconv, BN and swish), in training mode."""
    from asr_study_amd.core import engine
    from asr_study_amd.core.models import conformer
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = conformer(num_features=8, num_classes=5, d_model=16, num_heads=1, num_layers=1, d_ff=8,
                  kernel_size=3, conv_norm='batch', dropout=0, conv=False, device='cpu', seed=1)
    rs = np.random.RandomState(0)
    m.set_weights([(a + 0.1 * rs.randn(*a.shape)).astype(np.float32) for a in m.get_weights()])
    stages = CO.stages_from_model(m)
    x = rs.randn(6, 2, 8)
    lens, labels = np.array([6, 4]), [[1, 2], [3]]
    out = CO.loss_and_grads(stages, x, labels, lens)
    assert len(out['grads']) == len(m.get_weights()) == len(CO.weights(stages))
    tr = CO.trainable(stages)
    g = CO.grads_trainable(stages, out['grads'])
    assert len(tr) == len(g) == len(out['grads']) - 2
    f = lambda: float(np.mean(CO.loss_and_grads(stages, x, labels, lens)['ctc']))
    pick = [i for i, (st, k, _) in enumerate(tr) if st['type'] in ('dwconv', 'bn')] + [0, 1, 3]
    for i in pick:
        st, k, _ = tr[i]
        num, = _central(f, [st[k]], h=1e-6)
        assert np.abs(g[i] - num).max() <= 1e-6 * max(np.abs(num).max(), 1e-3), (i, st['type'], k)
