"""CPU checks of the RHN feature: the float64 oracle against torch.autograd on a direct
transcription of the reference's RHN.step, the ctypes mirror of asr_rhn_args against the header,
the layer-level validation, Keras-order weights, configs and checkpoint names of the ``rhn``
factory, the unchanged default models, and the two facts the GPU suite leans on (the saturation
sides of the parity inputs do not depend on the precision; the oracle's own learning step)."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from asr_study_amd.core.layers import RHN
from tests import rhn_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ['tanh', 'relu', 'linear', ('clipped_relu', 1.5)]


def _torch_act(act, z):
    if isinstance(act, tuple):
        return torch.clamp(z, 0.0, act[1])
    return {'tanh': torch.tanh, 'relu': torch.relu, 'linear': lambda v: v}[act](z)


def _torch_hs(a):
    return torch.clamp(0.2 * a + 0.5, 0.0, 1.0)


def _torch_birhn(x, p, act, coupling, merge, BW, BU):
    """The forward equations of RHN.step as an explicit time loop in torch (float64): the autograd
    reference."""
    T, N, _ = x.shape
    outs = []
    for d, key in enumerate(('fwd', 'bwd')):
        W, Us, bs = p[key]
        H = Us[0].shape[0]
        zx = (x if BW is None else x * BW[d]) @ W
        s = torch.zeros(N, H, dtype=x.dtype)
        ys = [None] * T
        for t in (range(T - 1, -1, -1) if d == 1 else range(T)):
            for l in range(len(Us)):
                m = s if BU is None else s * BU[d][l]
                a = m @ Us[l] + bs[l]
                if l == 0:
                    a = a + zx[t]
                hh, tg = _torch_act(act, a[:, :H]), _torch_hs(a[:, H:2 * H])
                cg = 1.0 - tg if coupling else _torch_hs(a[:, 2 * H:])
                s = hh * tg + s * cg
            ys[t] = s
        outs.append(torch.stack(ys))
    return torch.cat(outs, -1) if merge == 'concat' else outs[0] + outs[1]


def _random_stages(rs, F, H, Cn, depth, coupling, act, merge):
    """Dense, two stacked Bidirectional(RHN), Dense: weights spread so that the t / c gates
    saturate on a visible share of their entries."""
    Cb = RO.n_blocks(coupling)
    width = 2 * H if merge == 'concat' else H
    bias = np.concatenate([np.zeros(H)] + [np.full(H, -2.0)] * (Cb - 1))
    stages = [dict(type='dense', W=rs.randn(F, 6) * 0.5, b=rs.randn(6) * 0.1, l2=0.0)]
    for f_in in (6, width):
        p = {k: dict(W=rs.randn(f_in, Cb * H) * 0.6,
                     U=[rs.randn(H, Cb * H) * 0.4 for _ in range(depth)],
                     b=[bias + rs.randn(Cb * H) * 0.3 for _ in range(depth)])
             for k in ('fwd', 'bwd')}
        stages.append(dict(type='birhn', p=p, act=act, coupling=coupling, merge=merge, l2_W=0.0,
                           l2_U=0.0))
    stages.append(dict(type='dense', W=rs.randn(width, Cn) * 0.5, b=rs.randn(Cn) * 0.1, l2=0.0))
    return stages, width


@pytest.mark.parametrize('act', ACTS, ids=lambda a: a if isinstance(a, str) else a[0])
@pytest.mark.parametrize('merge', ['concat', 'sum'])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('H', [4, 5])
@pytest.mark.parametrize('coupling', [True, False])
@pytest.mark.parametrize('depth', [1, 2, 3])
def test_oracle_matches_autograd(depth, coupling, H, masked, merge, act):
    rs = np.random.RandomState(11 + H + 7 * depth)
    T, N, F, Cn = 7, 3, 5, 6
    x = rs.randn(T, N, F)
    stages, width = _random_stages(rs, F, H, Cn, depth, coupling, act, merge)
    masks = {}
    if masked:
        for i, f_in in ((1, 6), (2, width)):
            masks[i] = ((rs.rand(2, N, f_in) > 0.3) / 0.7, (rs.rand(2, depth, N, H) > 0.3) / 0.7)
    logits, caches = RO.model_forward(stages, x, masks)
    sat = np.mean([RO.saturated_share(c['gates'], H) for i in (1, 2) for c in caches[i]['cs']])
    assert 0.05 <= sat <= 0.8, sat
    G = rs.randn(*logits.shape)
    grads = RO.model_backward(stages, caches, G)

    tt = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tm = lambda a: torch.tensor(a)
    W1, b1 = tt(stages[0]['W']), tt(stages[0]['b'])
    P = [{k: (tt(stages[i]['p'][k]['W']), [tt(u) for u in stages[i]['p'][k]['U']],
              [tt(b) for b in stages[i]['p'][k]['b']]) for k in ('fwd', 'bwd')} for i in (1, 2)]
    W2, b2 = tt(stages[3]['W']), tt(stages[3]['b'])
    a = torch.tensor(x) @ W1 + b1
    for i in (1, 2):
        BW, BU = (tm(masks[i][0]), tm(masks[i][1])) if masked else (None, None)
        a = _torch_birhn(a, P[i - 1], act, coupling, merge, BW, BU)
    y = a @ W2 + b2
    (y * torch.tensor(G)).sum().backward()
    assert np.abs(y.detach().numpy() - logits).max() <= 1e-10 * max(1.0, np.abs(logits).max())
    want = [W1.grad, b1.grad]
    for Pi in P:
        for k in ('fwd', 'bwd'):
            W, Us, bs = Pi[k]
            want += [W.grad] + [u.grad for u in Us] + [b.grad for b in bs]
    want += [W2.grad, b2.grad]
    assert len(want) == len(grads)
    for g, w in zip(grads, want):
        w = w.numpy()
        assert g.shape == w.shape
        assert np.abs(g - w).max() <= 1e-10 * max(1.0, np.abs(w).max())


@pytest.mark.parametrize('coupling', [True, False])
def test_oracle_kernel_view_on_padded_slabs(coupling):
    """kernel_forward / kernel_backward are the per-direction recurrences stacked, and zero-padded
    slabs (H = 5 inside Hp = 8, pad bias 0) give the same real entries and exactly zero pads."""
    rs = np.random.RandomState(3)
    T, N, H, Hp, L = 5, 2, 5, 8, 2
    Cb = RO.n_blocks(coupling)
    zx = rs.randn(T, N, 2, Cb, H) * 2
    U = rs.randn(2, L, H, Cb, H) * 0.5
    b = np.zeros((2, L, Cb, H))
    b[:, :, 1:] = -2.0
    BU = (rs.rand(2, L, N, H) > 0.3) / 0.7
    dy = rs.randn(T, N, H)
    flat = lambda a: a.reshape(a.shape[:-2] + (-1,))
    h, gates = RO.kernel_forward(flat(zx), flat(U), flat(b), 'tanh', coupling, BU)
    assert h.shape == (L, T, N, 2, H) and gates.shape == (L, T, N, 2, Cb * H)
    for d in range(2):
        wh, wg = RO.recurrence_forward(flat(zx)[:, :, d], flat(U)[d], flat(b)[d], 'tanh', coupling,
                                       BU[d], reverse=d == 1)
        assert np.array_equal(h[:, :, :, d], wh) and np.array_equal(gates[:, :, :, d], wg)
    da = RO.kernel_backward(dy, flat(U), h, gates, 'tanh', coupling, BU, shared=True)
    assert da.shape == (L, T, N, 2, Cb * H)

    def pad(a, axes):
        for ax in axes:
            sh = list(a.shape)
            sh[ax] = Hp - H
            a = np.concatenate([a, np.zeros(sh)], axis=ax)
        return a
    zxp, Up, bp = pad(zx, [-1]), pad(U, [-1, 2]), pad(b, [-1])
    BUp = np.concatenate([BU, np.ones((2, L, N, Hp - H))], axis=-1)
    hp, gp = RO.kernel_forward(flat(zxp), flat(Up), flat(bp), 'tanh', coupling, BUp)
    assert np.all(hp[..., H:] == 0) and np.allclose(hp[..., :H], h, rtol=0, atol=1e-15)
    gp4 = gp.reshape(L, T, N, 2, Cb, Hp)
    assert np.allclose(flat(gp4[..., :H]), gates, rtol=0, atol=1e-15)
    dap = RO.kernel_backward(pad(dy, [-1]), flat(Up), hp, gp, 'tanh', coupling, BUp, shared=True)
    dap4 = dap.reshape(L, T, N, 2, Cb, Hp)
    assert np.all(dap4[..., H:] == 0)
    assert np.allclose(flat(dap4[..., :H]), da, rtol=0, atol=1e-14)


@pytest.mark.parametrize('coupling', [True, False])
def test_backward_reads_slopes_from_the_saved_gates(coupling):
    """A gate handed over as exactly 0 or 1 gets slope 0 whatever its pre-activation was, and the
    `sides` argument moves only the sides, not the values."""
    rs = np.random.RandomState(5)
    T, N, H, L = 4, 2, 3, 2
    Cb = RO.n_blocks(coupling)
    zx = rs.randn(T, N, Cb * H) * 0.5               # (nothing saturates by itself)
    Us = rs.randn(L, H, Cb * H) * 0.3
    bs = np.zeros((L, Cb * H))
    h, gates = RO.recurrence_forward(zx, Us, bs, 'tanh', coupling)
    assert RO.saturated_share(gates, H) == 0.0
    dy = rs.randn(T, N, H)
    base = RO.recurrence_backward(dy, Us, h, gates, 'tanh', coupling)
    for blk, value in [(1, 1.0), (1, 0.0)] + ([] if coupling else [(2, 0.0), (2, 1.0)]):
        cols = slice(blk * H, (blk + 1) * H)
        forced = gates.copy()
        forced[-1, -1, :, cols] = value            # the last level of the last frame, by hand
        da = RO.recurrence_backward(dy, Us, h, forced, 'tanh', coupling)
        assert np.all(da[-1, -1, :, cols] == 0.0) and np.any(base[-1, -1, :, cols] != 0.0)
        da2 = RO.recurrence_backward(dy, Us, h, gates, 'tanh', coupling, sides=forced)
        assert np.all(da2[-1, -1, :, cols] == 0.0)
        # values still the oracle's: the h block of that micro-step reads tg, not its slope
        assert np.array_equal(da2[-1, -1, :, :H], base[-1, -1, :, :H])
        assert RO.side_share(gates, forced, H) > 0


def test_rhn_args_layout_matches_header(tmp_path):
    from asr_study_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    fields = ['T', 'n_pad', 'H', 'depth', 'coupling', 'mode', 'activation', 'clip', 'U', 'b',
              'mask_u', 'zx', 'h', 'gates', 'y_sum', 'dy', 'dy_ld', 'dy_dir_stride', 'da',
              'db_part', 'dz_absmax']
    src = tmp_path / 'layout.c'
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "asr_hip.h"
int main(void) {
  printf("%%zu", sizeof(asr_rhn_args));
%s
  printf(" %%d\\n", ASR_HIP_ABI_VERSION);
  return 0;
}
''' % '\n'.join('  printf(" %%zu", offsetof(asr_rhn_args, %s));' % f for f in fields))
    exe = tmp_path / 'layout'
    subprocess.check_call([gcc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    R = _lib.RhnArgs
    assert [n for n, _ in R._fields_] == fields
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f in fields] + [_lib.ABI_VERSION]
    assert _lib.ABI_VERSION == 107
    for name in ('asr_rhn_workspace_bytes', 'asr_rhn_seq_fwd', 'asr_rhn_seq_bwd', 'asr_rhn_plan'):
        assert name in _lib.SIGNATURES


def test_library_exports_the_rhn_symbols():
    from asr_study_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):           # (as tests/test_capi_host.py's fixture)
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.asr_version() == _lib.ABI_VERSION == 107
    for name in ('asr_rhn_workspace_bytes', 'asr_rhn_seq_fwd', 'asr_rhn_seq_bwd', 'asr_rhn_plan'):
        assert hasattr(lib, name), name


def test_layer_validation():
    from asr_study_amd.core import layers as L
    r = RHN(8, depth=3, coupling=False, activation='relu', W_regularizer=L.l2(0.1),
            U_regularizer=L.l2(0.2), dropout_W=0.3, dropout_U=0.4, return_sequences=True)
    assert (r.output_dim, r.depth, r.coupling, r.activation, r.l2_W, r.l2_U, r.dropout_W,
            r.dropout_U) == (8, 3, False, 'relu', 0.1, 0.2, 0.3, 0.4)
    d = RHN(8)
    assert (d.depth, d.coupling, d.activation) == (1, True, 'tanh')
    RHN(8, activation='linear')
    RHN(8, activation=L.clipped_relu(20))
    RHN(8, bias_init=L.highway_bias_initializer)
    assert np.all(L.highway_bias_initializer((5,)) == -2.0)
    for kw, word in ((dict(activation='elu'), 'activation'),
                     (dict(inner_activation='sigmoid'), 'inner_activation'),
                     (dict(init='he_normal'), 'init'),
                     (dict(inner_init='glorot_uniform'), 'inner_init'),
                     (dict(bias_init='zero'), 'bias_init'),
                     (dict(return_sequences=False), 'return_sequences'),
                     (dict(b_regularizer=L.l2(0.1)), 'b_regularizer'),
                     (dict(stateful=True), 'stateful'),
                     (dict(layer_norm=True), 'layer_norm'),
                     (dict(mi=True), 'mi=True'),
                     (dict(depth=0), 'depth'),
                     (dict(go_backwards=True), 'go_backwards')):
        with pytest.raises(NotImplementedError) as e:
            RHN(8, **kw)
        msg = str(e.value)
        assert word in msg and 'implemented' in msg and 'hard_sigmoid' in msg \
            and 'highway_bias_initializer' in msg, msg
    x = L.Input(shape=(None, 5))
    assert L.Bidirectional(RHN(8))(x).features == 16
    assert L.Bidirectional(RHN(8), merge_mode='sum')(x).features == 8
    with pytest.raises(NotImplementedError):
        L.Bidirectional(RHN(8), merge_mode='mul')
    with pytest.raises(NotImplementedError) as e:
        L.recurrent(8, model='rhn')
    assert 'layers.RHN' in str(e.value)


def _rhn(**kw):
    from asr_study_amd.core.models import rhn
    return rhn(**dict(dict(num_features=16, num_classes=12, num_hiddens=10, num_layers=2, depth=2,
                           device='cpu'), **kw))


@pytest.mark.parametrize('coupling', [True, False])
def test_rhn_factory_builds_and_keeps_keras_order(coupling):
    from asr_study_amd.core.callbacks import keras_layers
    from asr_study_amd.utils import keras_config as K
    m = _rhn(coupling=coupling)
    assert [s.kind for s in m.stages] == ['noise', 'birhn', 'birhn', 'dense']
    H, Hp, Cb = 10, 12, (2 if coupling else 3)      # not a multiple of 4: padded to 12 inside
    st = [s for s in m.stages if s.kind == 'birhn']
    assert all((s.H, s.Hp, s.depth, s.coupling, s.nblk) == (H, Hp, 2, coupling, Cb) for s in st)
    assert all((s.l2_W, s.l2_U, s.dropout_W, s.dropout_U) == (1e-4, 1e-4, 0.2, 0.2) for s in st)
    w = m.get_weights()
    per_dir = lambda f: [(f, Cb * H)] + [(H, Cb * H)] * 2 + [(Cb * H,)] * 2
    assert [a.shape for a in w] == per_dir(16) * 2 + per_dir(2 * H) * 2 + [(2 * H, 12), (12,)]
    # initial values as the reference builds them
    bias = np.concatenate([np.zeros(H)] + [np.full(H, -2.0)] * (Cb - 1)).astype(np.float32)
    for k0 in (0, 5, 10, 15):
        W, Us, bs = w[k0], w[k0 + 1:k0 + 3], w[k0 + 3:k0 + 5]
        lim = math.sqrt(6.0 / (W.shape[0] + Cb * H))
        assert 0.8 * lim < np.abs(W).max() <= lim + 1e-7
        for U in Us:
            U = U.astype(np.float64)
            assert np.abs(U @ U.T - 1.21 * np.eye(H)).max() < 1e-5
        assert all(np.array_equal(b, bias) for b in bs)
    # ... and the pad entries of b_l are 0 in the flat parameters, not -2
    s = st[1]
    flat = m.params.numpy()
    bp = flat[s.ob:s.ob + 2 * 2 * Cb * Hp].reshape(2, 2, Cb, Hp)
    assert np.all(bp[..., H:] == 0) and np.all(bp[:, :, 1:, :H] == -2) and np.all(bp[:, :, 0] == 0)
    # checkpoint names in get_weights() order
    named = keras_layers(m, w)
    assert [n for n, _ in named] == ['bidirectional_1', 'bidirectional_2', 'timedistributed_1']
    want = []
    for d in ('forward', 'backward'):
        want += ['%s_rhn_2_W:0' % d] + ['%s_rhn_2_%d_U:0' % (d, l) for l in range(2)] + \
            ['%s_rhn_2_%d_b:0' % (d, l) for l in range(2)]
    assert [n for n, _ in named[1][1]] == want
    assert all(a is b for (_, a), b in zip(named[1][1], w[10:20]))
    # round trip in Keras order with distinct values everywhere
    rs = np.random.RandomState(0)
    new = [rs.randn(*a.shape).astype(np.float32) for a in w]
    m.set_weights(new)
    assert all(np.array_equal(a, b) for a, b in zip(new, m.get_weights()))
    flat = m.params.numpy()
    Up = flat[s.oU:s.oU + 2 * 2 * Hp * Cb * Hp].reshape(2, 2, Hp, Cb, Hp)
    assert np.all(Up[:, :, H:] == 0) and np.all(Up[..., H:] == 0)
    Wp = flat[s.oW:s.oW + s.f_in_pad * 2 * Cb * Hp].reshape(s.f_in_pad, 2, Cb, Hp)
    assert s.f_in_pad == 24 and np.all(Wp[[10, 11, 22, 23]] == 0) and np.all(Wp[..., H:] == 0)
    bp = flat[s.ob:s.ob + 2 * 2 * Cb * Hp].reshape(2, 2, Cb, Hp)
    assert np.all(bp[..., H:] == 0)
    # the Keras config names an RHN and rebuilds the same stage list
    text = K.model_config(m)
    bi = [l for l in json.loads(text)['config']['layers'] if l['class_name'] == 'Bidirectional']
    assert [l['config']['layer']['class_name'] for l in bi] == ['RHN', 'RHN']
    c = bi[0]['config']['layer']['config']
    assert c == {'name': 'rhn_1', 'trainable': True, 'return_sequences': True,
                 'go_backwards': False, 'stateful': False, 'unroll': False, 'consume_less': 'gpu',
                 'input_dim': 16, 'input_length': None, 'output_dim': H, 'depth': 2,
                 'init': 'glorot_uniform', 'inner_init': 'orthogonal',
                 'bias_init': 'highway_bias_initializer', 'activation': 'tanh',
                 'inner_activation': 'hard_sigmoid', 'coupling': coupling, 'layer_norm': False,
                 'ln_gain_init': 'one', 'ln_bias_init': 'zero', 'mi': False,
                 'W_regularizer': {'name': 'WeightRegularizer', 'l1': 0.0, 'l2': 1e-4},
                 'U_regularizer': {'name': 'WeightRegularizer', 'l1': 0.0, 'l2': 1e-4},
                 'b_regularizer': None, 'dropout_W': 0.2, 'dropout_U': 0.2}
    from asr_study_amd.core import engine
    old = engine.DEFAULT_DEVICE
    engine.DEFAULT_DEVICE = 'cpu'
    try:
        m2 = K.topology_from_config(text)
    finally:
        engine.DEFAULT_DEVICE = old
    key = lambda mm: [(s.kind, getattr(s, 'H', None), getattr(s, 'depth', None),
                       getattr(s, 'coupling', None), getattr(s, 'merge', None),
                       getattr(s, 'act', None), getattr(s, 'dropout_U', None),
                       getattr(s, 'l2_U', None), s.p_lo, s.p_hi) for s in mm.stages]
    assert key(m2) == key(m)
    assert m.config == {'name': 'rhn', 'kwargs': dict(
        num_features=16, num_classes=12, num_hiddens=10, num_layers=2, depth=2, coupling=coupling,
        dropout=0.2, input_dropout=False, input_std_noise=.0, weight_decay=1e-4,
        merge_mode='concat', activation='tanh')}


def test_rhn_factory_options_and_name_lookup():
    from asr_study_amd.core import models
    from asr_study_amd.utils import generic_utils as utils
    assert utils.get_from_module('core.models', 'rhn') is models.rhn
    m = _rhn(merge_mode='sum', activation='relu', input_dropout=True, depth=3)
    assert [s.kind for s in m.stages] == ['noise', 'dropout', 'birhn', 'birhn', 'dense']
    st = [s for s in m.stages if s.kind == 'birhn']
    assert [(s.merge, s.act, s.depth, s.f_in, s.f_out) for s in st] == \
        [('sum', 'relu', 3, 16, 10), ('sum', 'relu', 3, 10, 10)]
    with pytest.raises(ValueError):
        models.deep_speech2(num_features=16, conv_filters=4, device='cpu', rnn_type='rhn')


def test_default_models_are_unchanged():
    """brsmv1() and deep_speech2() as built by hand from the layer calls their factories make: the
    same Keras config text, stage kinds, parameter offsets and initial weights (the new stage
    kind draws nothing from another stage's random stream)."""
    from asr_study_amd.core import layers as L
    from asr_study_amd.core import models
    from asr_study_amd.core.models import ctc_model
    from asr_study_amd.utils import keras_config as K

    def same(m, by_hand):
        assert K.model_config(m) == K.model_config(by_hand)
        assert [(s.kind, s.p_lo, s.p_hi) for s in m.stages] == \
            [(s.kind, s.p_lo, s.p_hi) for s in by_hand.stages]
        a, b = m.get_weights(), by_hand.get_weights()
        assert len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))
        assert m._segments == by_hand._segments

    m = models.brsmv1(num_features=16, num_classes=12, num_hiddens=10, num_layers=2, device='cpu')
    x = L.Input(name='inputs', shape=(None, 16))
    o = L.GaussianNoise(.0)(x)
    for _ in range(2):
        o = L.Bidirectional(L.LSTM(10, return_sequences=True, W_regularizer=L.l2(1e-4),
                                   U_regularizer=L.l2(1e-4), dropout_W=0.2, dropout_U=0.2,
                                   zoneout_c=0., zoneout_h=0., mi=None, layer_norm=None,
                                   activation='tanh'))(o)
    o = L.TimeDistributed(L.Dense(12, W_regularizer=L.l2(1e-4)))(o)
    same(m, ctc_model(x, o, device='cpu'))
    assert m.config == {'name': 'brsmv1', 'kwargs': dict(
        num_features=16, num_classes=12, num_hiddens=10, num_layers=2, dropout=0.2, zoneout=0.,
        input_dropout=False, input_std_noise=.0, weight_decay=1e-4, residual=None,
        layer_norm=None, mi=None, activation='tanh')}
    # W of the first BiLSTM: glorot-uniform over (16, 40) from RandomState(0), the first draw
    lim = math.sqrt(6.0 / (16 + 40))
    want = np.random.RandomState(0).uniform(-lim, lim, size=(16, 40)).astype(np.float32)
    assert np.array_equal(m.get_weights()[0], want)

    m = models.deep_speech2(num_features=16, num_classes=12, num_hiddens=10, num_layers=2,
                            conv_filters=4, conv_kernels=((5, 7), (3, 5)), device='cpu')
    x = L.Input(name='inputs', shape=(None, 16))
    o = L.GaussianNoise(.0)(x)
    o = L.Reshape((-1, 16, 1))(o)
    for (kt, kf), (st, sf) in zip(((5, 7), (3, 5)), ((2, 2), (1, 2))):
        o = L.Convolution2D(4, kt, kf, subsample=(st, sf), border_mode='same',
                            activation=L.clipped_relu(20), W_regularizer=L.l2(1e-4))(o)
    o = L.Reshape((-1, o.features))(o)
    for _ in range(2):
        o = L.Bidirectional(L.LSTM(10, return_sequences=True, W_regularizer=L.l2(1e-4),
                                   U_regularizer=L.l2(1e-4), dropout_W=0.2, dropout_U=0.2))(o)
    o = L.TimeDistributed(L.Dense(12, W_regularizer=L.l2(1e-4)))(o)
    same(m, ctc_model(x, o, device='cpu'))
    assert 'rnn_type' not in m.config['kwargs'] and 'batch_norm' not in m.config['kwargs']
    assert json.loads(json.dumps(m.config))['kwargs']['conv_kernels'] == [[5, 7], [3, 5]]


@pytest.mark.parametrize('masks_on', [False, True], ids=['plain', 'masks'])
@pytest.mark.parametrize('case', [0, 1], ids=['stack', 'rhn'])
def test_parity_inputs_keep_their_sides_in_float32(case, masks_on):
    """The condition of the GPU model-parity test, on the reference alone: the oracle run in
    float32 lands on the same side of every hard-sigmoid kink as in float64, on the very models
    and batches the GPU test uses (share of differing t / c entries at most 1e-4 per stage)."""
    tag, build, batch, seed = RO.parity_cases()[case]
    rs = np.random.RandomState(seed)
    model = build(0.2 if masks_on else 0.0, device='cpu')
    x, lens, labels = batch(rs)
    N = x.shape[0]
    masks = RO.cut_masks(model, RO.draw_masks(model, 16, rs), N) if masks_on else None
    stages = RO.stages_from_model(model)
    x64 = np.ascontiguousarray(np.transpose(x, (1, 0, 2))).astype(np.float64)

    def cast(o):
        if isinstance(o, dict):
            return {k: cast(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)) and not (o and isinstance(o[0], str)):
            return type(o)(cast(v) for v in o)
        return o.astype(np.float32) if isinstance(o, np.ndarray) else o
    _, c64 = RO.model_forward(stages, x64, masks)
    _, c32 = RO.model_forward(cast(stages), x64.astype(np.float32), cast(masks))
    n = 0
    for si, s in enumerate(model.stages):
        if s.kind != 'birhn':
            continue
        for d in range(2):
            g64, g32 = c64[si]['cs'][d]['gates'], c32[si]['cs'][d]['gates']
            assert g32.dtype == np.float32
            share = RO.side_share(g64, g32.astype(np.float64), s.H)
            sat = RO.saturated_share(g64, s.H)
            print('[rhn] %s stage %d dir %d: %d t/c entries, %.3f saturated, share on another '
                  'side in float32 %.2e' % (tag, si, d, g64[..., s.H:].size, sat, share))
            assert share <= 1e-4, (tag, si, d, share)
            n += 1
    assert n == 4


def test_kernel_case_options_cover_the_grid():
    """The 60 kernel cases of the GPU suite: every (depth, coupling) pair meets a width below 64,
    H = 512 and H = 1024; masks on / off and both merge modes occur; every activation meets every
    shape (k runs over all of them for each shape)."""
    seen = {}
    for i, (H, _, _) in enumerate(RO.KERNEL_SHAPES):
        for k in range(4):
            depth, coupling, masked, merge = RO.case_options(i, k)
            seen.setdefault((depth, coupling), set()).add('small' if H < 64 else H)
            seen.setdefault('mask', set()).add(masked)
            seen.setdefault('merge', set()).add(merge)
    assert all({'small', 512, 1024} <= seen[p] for p in RO.PAIRS)
    assert seen['mask'] == {False, True} and seen['merge'] == {'sum', 'concat'}


def test_oracle_learning_step():
    """K_REF, the step at which the float64 oracle first decodes the learning task without error
    (the GPU test's budget is ceil(1.25 * K_REF))."""
    assert RO.K_REF is not None and RO.K_REF <= 400
    assert RO.learn_reference(max_steps=RO.K_REF) == RO.K_REF
