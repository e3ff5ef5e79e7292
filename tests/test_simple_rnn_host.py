"""CPU checks of the SimpleRNN feature: the float64 oracle against torch.autograd, the ctypes
mirror of asr_rnn_args against the header, and the layer-level validation."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import simple_rnn_oracle as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_act(act, z):
    if isinstance(act, tuple):
        return torch.clamp(z, 0.0, act[1])
    return {'tanh': torch.tanh, 'relu': torch.relu, 'linear': lambda v: v}[act](z)


def _torch_birnn(x, p, act, merge, BW, BU):
    """An explicit time loop in torch (float64), the autograd reference."""
    T, N, _ = x.shape
    outs = []
    for d, key in enumerate(('fwd', 'bwd')):
        W, U, b = p[key]
        xm = x if BW is None else x * BW[d]
        prev = torch.zeros(N, U.shape[0], dtype=x.dtype)
        hs = [None] * T
        for t in (range(T - 1, -1, -1) if d == 1 else range(T)):
            hp = prev if BU is None else prev * BU[d]
            hs[t] = _torch_act(act, xm[t] @ W + b + hp @ U)
            prev = hs[t]
        outs.append(torch.stack(hs))
    return torch.cat(outs, -1) if merge == 'concat' else outs[0] + outs[1]


@pytest.mark.parametrize('act', ['tanh', 'relu', 'linear', ('clipped_relu', 1.5)])
@pytest.mark.parametrize('merge', ['concat', 'sum'])
@pytest.mark.parametrize('masked', [False, True])
def test_oracle_matches_autograd(act, merge, masked):
    rs = np.random.RandomState(7)
    T, N, F, H, C = 6, 3, 5, 4, 7
    x = rs.randn(T, N, F)
    stages = [dict(type='dense', W=rs.randn(F, 6) * 0.5, b=rs.randn(6) * 0.1),
              dict(type='act', act=act), dict(type='dropout', p=0.5)]
    p = {k: dict(W=rs.randn(6, H) * 0.5, U=rs.randn(H, H) * 0.4, b=rs.randn(H) * 0.1)
         for k in ('fwd', 'bwd')}
    stages.append(dict(type='birnn', p=p, act=act, merge=merge))
    width = 2 * H if merge == 'concat' else H
    stages.append(dict(type='dense', W=rs.randn(width, C) * 0.5, b=rs.randn(C) * 0.1))
    masks = {}
    if masked:
        masks[2] = (rs.rand(T, N, 6) > 0.3) / 0.7
        masks[3] = ((rs.rand(2, N, 6) > 0.3) / 0.7, (rs.rand(2, N, H) > 0.3) / 0.7)
    logits, caches = SR.model_forward(stages, x, masks)
    G = rs.randn(*logits.shape)
    grads = SR.model_backward(stages, caches, G)

    tt = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    W1, b1 = tt(stages[0]['W']), tt(stages[0]['b'])
    P = {k: [tt(p[k][n]) for n in ('W', 'U', 'b')] for k in ('fwd', 'bwd')}
    W2, b2 = tt(stages[4]['W']), tt(stages[4]['b'])
    tm = lambda a: None if a is None else torch.tensor(a)
    a = _torch_act(act, torch.tensor(x) @ W1 + b1)
    if masked:
        a = a * tm(masks[2])
    BW, BU = (tm(masks[3][0]), tm(masks[3][1])) if masked else (None, None)
    y = _torch_birnn(a, P, act, merge, BW, BU) @ W2 + b2
    (y * torch.tensor(G)).sum().backward()
    assert np.abs(y.detach().numpy() - logits).max() <= 1e-10 * max(1.0, np.abs(logits).max())
    want = [W1.grad, b1.grad] + [t.grad for k in ('fwd', 'bwd') for t in P[k]] + [W2.grad, b2.grad]
    assert len(want) == len(grads)
    for g, w in zip(grads, want):
        w = w.numpy()
        assert g.shape == w.shape
        assert np.abs(g - w).max() <= 1e-10 * max(1.0, np.abs(w).max())


def test_oracle_kernel_view_matches_layers():
    rs = np.random.RandomState(3)
    T, N, H = 5, 2, 3
    zx = rs.randn(T, N, 2, H)
    U = rs.randn(2, H, H) * 0.5
    h = SR.kernel_forward(zx, U, 'tanh')
    for d in range(2):
        want = SR.recurrence_forward(zx[:, :, d], U[d], 'tanh', reverse=d == 1)
        assert np.array_equal(h[:, :, d], want)
    dz = SR.kernel_backward(rs.randn(T, N, H), U, h, 'tanh', shared=True)
    assert dz.shape == (T, N, 2, H)


def test_rnn_args_layout_matches_header(tmp_path):
    from asr_study_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    src = tmp_path / 'layout.c'
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "asr_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(asr_rnn_args), offsetof(asr_rnn_args, clip),
         offsetof(asr_rnn_args, U), offsetof(asr_rnn_args, y_sum), offsetof(asr_rnn_args, dy_ld),
         offsetof(asr_rnn_args, dz), offsetof(asr_rnn_args, dz_absmax), ASR_HIP_ABI_VERSION);
  return 0;
}
''')
    exe = tmp_path / 'layout'
    subprocess.check_call([gcc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    R = _lib.RnnArgs
    assert got == [C.sizeof(R), R.clip.offset, R.U.offset, R.y_sum.offset, R.dy_ld.offset,
                   R.dz.offset, R.dz_absmax.offset, _lib.ABI_VERSION]
    assert _lib.ABI_VERSION == 107
    for name in ('asr_rnn_workspace_bytes', 'asr_rnn_seq_fwd', 'asr_rnn_seq_bwd', 'asr_rnn_plan'):
        assert name in _lib.SIGNATURES


def test_layer_validation():
    from asr_study_amd.core import layers as L
    assert isinstance(L.recurrent(8, model='rnn'), L.SimpleRNN)
    assert isinstance(L.recurrent(8, model='lstm'), L.LSTM)
    assert isinstance(L.recurrent(8, model='keras_lstm'), L.LSTM)
    r = L.recurrent(8, model='rnn', activation='relu', regularizer=L.l2(0.1), dropout=0.2)
    assert (r.activation, r.l2_W, r.l2_U, r.dropout_W, r.dropout_U) == ('relu', 0.1, 0.1, 0.2, 0.2)
    for m in ('gru', 'rhn'):
        with pytest.raises(NotImplementedError):
            L.recurrent(8, model=m)
    with pytest.raises(NotImplementedError):
        L.SimpleRNN(8, activation='elu')
    with pytest.raises(NotImplementedError):
        L.Activation('softmax')
    with pytest.raises(NotImplementedError):
        L.Bidirectional(L.LSTM(8), merge_mode='sum')
    with pytest.raises(NotImplementedError):
        L.Bidirectional(L.SimpleRNN(8), merge_mode='mul')
    x = L.Input(shape=(None, 5))
    assert L.Bidirectional(L.SimpleRNN(8), merge_mode='sum')(x).features == 8
    assert L.Bidirectional(L.SimpleRNN(8))(x).features == 16
    assert L.TimeDistributed(L.Activation(L.clipped_relu(20)))(x).features == 5
    assert L.TimeDistributed(L.Dropout(0.1))(x).features == 5


def test_factories_build_and_keep_keras_order(monkeypatch):
    from asr_study_amd.core import engine
    from asr_study_amd.core.models import maas, deep_speech
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    from asr_study_amd.core.callbacks import keras_layers
    from asr_study_amd.utils import keras_config as K
    for f, n_dense in ((maas, 5), (deep_speech, 5)):
        m = f(num_features=26, num_hiddens=34, num_classes=29, device='cpu')
        assert [s.kind for s in m.stages].count('birnn') == 1
        assert [s.kind for s in m.stages].count('dense') == n_dense
        w = m.get_weights()
        m.set_weights(w)
        assert all(np.array_equal(a, b) for a, b in zip(w, m.get_weights()))
        names = [n for _, ws in keras_layers(m, w) for n, _ in ws]
        assert 'forward_simplernn_1_W:0' in names and 'backward_simplernn_1_b:0' in names
        m2 = K.topology_from_config(K.model_config(m))
        assert [(s.kind, getattr(s, 'merge', None)) for s in m2.stages] == \
            [(s.kind, getattr(s, 'merge', None)) for s in m.stages]
        assert m.config['name'] == f.__name__
