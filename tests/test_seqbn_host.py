"""CPU checks of the sequence-wise batch normalisation of the GRU input projection
(layers.GRU(batch_norm=True), deep_speech2(batch_norm='recurrent')): the float64 oracle
tests/seqbn_oracle.py against torch autograd, layer validation, the factory's stage list, weight
order, parameter count, config round trip, unchanged defaults, and the C ABI's prototypes."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from asr_study_amd.core.layers import GRU
from tests import seqbn_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- oracle against autograd
def _torch_seqbn(p, gamma, beta, V, eps):
    nv = V.sum()
    Vf = V[..., None].to(p.dtype)
    mu = (p * Vf).sum(dim=(0, 1)) / nv
    var = (((p - mu) ** 2) * Vf).sum(dim=(0, 1)) / nv
    return gamma * (p - mu) / torch.sqrt(var + eps) + beta


@pytest.mark.parametrize('lens', [list(range(30, 0, -1))[::3], [30] * 7, None, [1, 30, 17]],
                         ids=['ragged', 'full', 'none', 'len1'])
def test_oracle_matches_autograd(lens):
    rs = np.random.RandomState(0)
    T, W = 30, 12
    N = 5 if lens is None else len(lens)
    p = rs.randn(T, N, W) * rs.uniform(0.1, 3.0, W) + rs.randn(W) * 2
    gamma, beta = rs.randn(W), rs.randn(W)
    gamma[3] = 0.0                                  # xhat must not be recovered from zx
    da = rs.randn(T, N, W)                          # non-zero on padded frames too
    y, c = SO.seqbn_forward(p, gamma, beta, lens, eps=1e-3)
    dp, dg, db = SO.seqbn_backward(da, c)
    V = SO.valid_mask(T, N, lens)
    assert V.sum() == (T * N if lens is None else sum(min(l, T) for l in lens))
    tp, tg, tb = [torch.tensor(a, dtype=torch.float64, requires_grad=True)
                  for a in (p, gamma, beta)]
    ty = _torch_seqbn(tp, tg, tb, torch.tensor(V), 1e-3)
    ty.backward(torch.tensor(da))
    for got, want, what in ((y, ty.detach().numpy(), 'y'), (dp, tp.grad.numpy(), 'dp'),
                            (dg, tg.grad.numpy(), 'dgamma'), (db, tb.grad.numpy(), 'dbeta')):
        assert np.abs(got - want).max() < 1e-10, what
    # padded frames are normalised, and count for nothing in the statistics
    if lens is not None and min(lens) < T:
        p2 = p.copy()
        p2[~V] += rs.randn(*p2[~V].shape) * 5
        y2, c2 = SO.seqbn_forward(p2, gamma, beta, lens, eps=1e-3)
        assert np.array_equal(c2['mean'], c['mean']) and np.array_equal(c2['var'], c['var'])
        assert np.array_equal(y2[V], y[V]) and not np.array_equal(y2[~V], y[~V])
    # inference and the EMA
    rm, rv = rs.randn(W), rs.uniform(0.5, 2.0, W)
    want = gamma * (p - rm) / np.sqrt(rv + 1e-3) + beta
    assert np.abs(SO.seqbn_infer(p, gamma, beta, rm, rv, 1e-3) - want).max() < 1e-12
    assert np.allclose(SO.ema(rm, c['mean'], 0.99), 0.99 * rm + 0.01 * c['mean'], atol=1e-15)
    blk = SO.moments_block(p, lens, 1.0, rm)
    from tests import batchnorm_oracle as BO
    m2, v2 = BO.update_from_moments(rm, rv, blk, 0.99)
    assert np.abs(m2 - SO.ema(rm, c['mean'], 0.99)).max() < 1e-12
    assert np.abs(v2 - SO.ema(rv, c['var'], 0.99)).max() < 1e-12
    assert blk[0] == V.sum()


def test_oracle_model_chain_matches_autograd():
    """The batch-normalised Bidirectional(GRU) of the oracle, forward and every gradient, against
    autograd on a transcription of the equations (unequal lengths, masks, 'sum')."""
    from tests.test_gru_host import _torch_act, _torch_hs
    rs = np.random.RandomState(1)
    T, N, F, H = 9, 4, 5, 3
    lens = [9, 4, 1, 7]
    x = rs.randn(T, N, F)
    BW = (rs.rand(2, N, F) > 0.2) / 0.8
    BU = (rs.rand(2, N, H) > 0.2) / 0.8
    st = dict(act='tanh', merge='sum', eps=1e-3, p={
        d: dict(W=rs.randn(F, 3 * H), U=rs.randn(H, 3 * H) * 0.5, gamma=rs.randn(3 * H),
                beta=rs.randn(3 * H), rm=np.zeros(3 * H), rv=np.ones(3 * H))
        for d in ('fwd', 'bwd')})
    y, c = SO.bigru_bn_forward(x, st, lens, BW, BU)
    dy = rs.randn(*y.shape)
    dx, g = SO.bigru_bn_backward(dy, c)
    V = torch.tensor(SO.valid_mask(T, N, lens))
    tx = torch.tensor(x, requires_grad=True)
    leaves, ty = [], 0
    for d, key in enumerate(('fwd', 'bwd')):
        q = {k: torch.tensor(st['p'][key][k], requires_grad=True)
             for k in ('W', 'U', 'gamma', 'beta')}
        leaves += [q[k] for k in ('W', 'U', 'gamma', 'beta')]
        zx = _torch_seqbn((tx * torch.tensor(BW[d])) @ q['W'], q['gamma'], q['beta'], V, 1e-3)
        prev = torch.zeros(N, H, dtype=torch.float64)
        hs = [None] * T
        for t in (range(T - 1, -1, -1) if d else range(T)):
            m = prev * torch.tensor(BU[d])
            zr = _torch_hs(zx[t, :, :2 * H] + m @ q['U'][:, :2 * H])
            z, r = zr[:, :H], zr[:, H:]
            hh = _torch_act('tanh', zx[t, :, 2 * H:] + (r * m) @ q['U'][:, 2 * H:])
            prev = z * prev + (1 - z) * hh
            hs[t] = prev
        ty = ty + torch.stack(hs)
    assert np.abs(ty.detach().numpy() - y).max() < 1e-10
    ty.backward(torch.tensor(dy))
    assert np.abs(tx.grad.numpy() - dx).max() < 1e-10
    got = [g[i] for i in (0, 1, 2, 3, 6, 7, 8, 9)]
    for a, leaf in zip(got, leaves):
        assert np.abs(leaf.grad.numpy() - a).max() < 1e-10
    assert all(np.all(g[i] == 0) for i in (4, 5, 10, 11))


# ---------------------------------------------------------------- layer and factory
def test_layer_builds_and_validates():
    from asr_study_amd.core import layers as L
    g = GRU(8, batch_norm=True)
    assert (g.batch_norm, g.bn_epsilon, g.bn_momentum) == (True, 1e-3, 0.99)
    g = GRU(8, batch_norm=True, bn_epsilon=1e-5, bn_momentum=0.9)
    assert (g.bn_epsilon, g.bn_momentum) == (1e-5, 0.9)
    assert GRU(8).batch_norm is False
    for kw in (dict(batch_norm='yes'), dict(batch_norm=1), dict(batch_norm=True, bn_epsilon=0.0),
               dict(batch_norm=True, bn_momentum=1.5), dict(batch_norm=True, bn_momentum=-0.1)):
        with pytest.raises(NotImplementedError) as e:
            GRU(8, **kw)
        assert 'implemented' in str(e.value)
    x = L.Input(shape=(None, 5))
    assert L.Bidirectional(GRU(8, batch_norm=True))(x).features == 16
    assert L.Bidirectional(GRU(8, batch_norm=True), merge_mode='sum')(x).features == 8


def _ds2(**kw):
    from asr_study_amd.core.models import deep_speech2
    return deep_speech2(num_features=16, num_classes=12, num_hiddens=10, num_layers=2,
                        conv_filters=4, conv_kernels=((5, 7), (3, 5)), device='cpu', **kw)


def test_recurrent_needs_gru():
    for kw in (dict(), dict(rnn_type='lstm')):
        with pytest.raises(ValueError) as e:
            _ds2(batch_norm='recurrent', **kw)
        assert 'gru' in str(e.value) and 'recurrent' in str(e.value)
    with pytest.raises(ValueError):
        _ds2(batch_norm='sequence', rnn_type='gru')


def test_deep_speech2_recurrent_stages_weights_and_config():
    from asr_study_amd.core import engine
    from asr_study_amd.core.callbacks import keras_layers
    from asr_study_amd.utils import keras_config as K
    m = _ds2(batch_norm='recurrent', rnn_type='gru')
    kinds = [s.kind for s in m.stages if s.kind not in ('noise', 'reshape')]
    assert kinds == ['conv', 'bn', 'act', 'conv', 'bn', 'act', 'bigru', 'bigru', 'dense']
    for i, s in enumerate(m.stages):
        if s.kind == 'bigru':
            assert s.bn and (s.bn_eps, s.bn_momentum) == (1e-3, 0.99) and s.ob is None
            before = [p.kind for p in m.stages[:i] if p.kind not in ('reshape', 'dropout')]
            assert before[-1] != 'bn'
        if s.kind == 'conv':
            assert m.stages[i + 1].kind == 'bn' and s.clip == 0
    assert m.config['kwargs']['batch_norm'] == 'recurrent'
    assert m.config['kwargs']['rnn_type'] == 'gru'
    H = 10
    w = m.get_weights()
    named = keras_layers(m, w)
    groups = [ws for name, ws in named if name.startswith('bidirectional_')]
    for k, F in enumerate((16, 2 * H)):
        assert [a.shape for _, a in groups[k]] == [(F, 3 * H), (H, 3 * H)] + [(3 * H,)] * 4 \
            + [(F, 3 * H), (H, 3 * H)] + [(3 * H,)] * 4
        assert [n for n, _ in groups[k]] == [
            '%s_gru_%d_%s:0' % (d, k + 1, part) for d in ('forward', 'backward')
            for part in ('W', 'U', 'gamma', 'beta', 'running_mean', 'running_std')]
    # initial values: gamma 1, beta 0, running mean 0, running variance 1
    vals = [a for _, a in groups[0]][2:6]
    assert [float(v.min()) for v in vals] == [1.0, 0.0, 0.0, 1.0]
    assert [float(v.max()) for v in vals] == [1.0, 0.0, 0.0, 1.0]
    # trainable parameters per Bidirectional layer: 2 (F 3H + H 3H + 6H); gamma and beta get l2 0
    grads = m._unpack(m.params.numpy())            # trainable arrays only
    per_layer = {16: 0, 2 * H: 0}
    it = iter(grads)
    for s in m.stages:
        n = {'conv': 2, 'bn': 2, 'dense': 2, 'bigru': 8}.get(s.kind, 0)
        arrs = [next(it) for _ in range(n)]
        if s.kind == 'bigru':
            per_layer[s.f_in] = sum(a.size for a in arrs)
    assert per_layer == {F: 2 * (F * 3 * H + H * 3 * H + 6 * H) for F in (16, 2 * H)}
    for s in m.stages:
        if s.kind == 'bigru':
            seg = {o: l2 for o, _, l2 in m._segments}
            assert seg[s.og] == 0.0 and seg[s.obeta] == 0.0 and seg[s.oW] == 1e-4
    # round trip in Keras order with distinct values; pad columns stay zero (Hp = 12)
    rs = np.random.RandomState(0)
    new = [rs.randn(*a.shape).astype(np.float32) for a in w]
    m.set_weights(new)
    assert all(np.array_equal(a, b) for a, b in zip(new, m.get_weights()))
    s = [st for st in m.stages if st.kind == 'bigru'][1]
    flat = m.params.numpy()
    for o in (s.og, s.obeta):
        assert np.all(flat[o:o + 72].reshape(2, 3, 12)[..., H:] == 0)
    assert len(m.get_gradients()) == len(w)
    # config round trip
    text = K.model_config(m)
    cfg = json.loads(text)
    bi = [l for l in cfg['config']['layers'] if l['class_name'] == 'Bidirectional']
    c = bi[0]['config']['layer']['config']
    assert (c['batch_norm'], c['bn_epsilon'], c['bn_momentum']) == (True, 1e-3, 0.99)
    old = engine.DEFAULT_DEVICE
    engine.DEFAULT_DEVICE = 'cpu'
    try:
        m2 = K.topology_from_config(text)
    finally:
        engine.DEFAULT_DEVICE = old
    key = lambda mm: [(st.kind, getattr(st, 'H', None), getattr(st, 'bn', None),
                       getattr(st, 'bn_eps', None), getattr(st, 'bn_momentum', None))
                      for st in mm.stages]
    assert key(m2) == key(m) and K.model_config(m2) == text
    assert [a.shape for a in m2.get_weights()] == [a.shape for a in w]


def test_defaults_and_layer_input_bn_are_unchanged():
    """deep_speech2() and deep_speech2(batch_norm=True, rnn_type='gru') against the same
    topologies built by hand from the layer calls the factory made before the option existed."""
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import ctc_model
    from asr_study_amd.utils import keras_config as K

    def by_hand(bn, cell):
        x = L.Input(name='inputs', shape=(None, 16))
        o = L.GaussianNoise(.0)(x)
        o = L.Reshape((-1, 16, 1))(o)
        for (kt, kf), (st, sf) in zip(((5, 7), (3, 5)), ((2, 2), (1, 2))):
            o = L.Convolution2D(4, kt, kf, subsample=(st, sf), border_mode='same',
                                activation=None if bn else L.clipped_relu(20),
                                W_regularizer=L.l2(1e-4))(o)
            if bn:
                o = L.BatchNormalization()(o)
                o = L.Activation(L.clipped_relu(20))(o)
        o = L.Reshape((-1, o.features))(o)
        for _ in range(2):
            if bn:
                o = L.BatchNormalization()(o)
            o = L.Bidirectional(cell(10, return_sequences=True, W_regularizer=L.l2(1e-4),
                                     U_regularizer=L.l2(1e-4), dropout_W=0.2, dropout_U=0.2))(o)
        o = L.TimeDistributed(L.Dense(12, W_regularizer=L.l2(1e-4)))(o)
        return ctc_model(x, o, device='cpu')
    for kw, ref in ((dict(), by_hand(False, L.LSTM)),
                    (dict(batch_norm=True, rnn_type='gru'), by_hand(True, L.GRU))):
        m = _ds2(**kw)
        text = K.model_config(m)
        assert text == K.model_config(ref)
        assert 'bn_epsilon' not in text and '"batch_norm"' not in text
        assert [a.shape for a in m.get_weights()] == [a.shape for a in ref.get_weights()]
        assert all(np.array_equal(a, b) for a, b in zip(m.get_weights(), ref.get_weights()))
        assert m.n_params == ref.n_params and m._gbuf.numel() == ref._gbuf.numel()
        assert m.config['kwargs'].get('batch_norm', False) == kw.get('batch_norm', False)
        assert all(not getattr(s, 'bn', False) for s in m.stages if s.kind == 'bigru')


# ---------------------------------------------------------------- the C ABI
def test_prototypes_match_header():
    """Every asr_seqbn_* prototype of include/asr_hip.h against _lib.SIGNATURES, argument by
    argument; the additions leave the ABI number alone."""
    from asr_study_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'asr_hip.h')).read()
    protos = re.findall(r'^(size_t|int) (asr_seqbn_\w+)\(([^;]*)\);', text, re.M)
    assert sorted(n for _, n, _ in protos) == ['asr_seqbn_bwd', 'asr_seqbn_fwd_infer',
                                               'asr_seqbn_fwd_train', 'asr_seqbn_workspace_bytes']

    def ctype(arg):
        arg = ' '.join(arg.split())
        if '*' in arg or arg.startswith('asr_stream_t'):
            return C.c_void_p
        return {'int': C.c_int, 'float': C.c_float, 'size_t': C.c_size_t}[arg.split()[0]]
    for ret, name, args in protos:
        res, argtypes = _lib.SIGNATURES[name]
        assert res is (C.c_size_t if ret == 'size_t' else C.c_int), name
        assert [ctype(a) for a in args.split(',')] == list(argtypes), name
    assert _lib.ABI_VERSION == 107 and '#define ASR_HIP_ABI_VERSION 107' in text
