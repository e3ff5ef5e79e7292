"""CPU checks of the LayerNormalization feature: the float64 oracle against torch.autograd, the
layer validation, the ctc_model spec and factory stage lists, the parameter layout and Keras
names, the Keras config round trip, and the asr_ln_* C declarations and argument checks."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import layernorm_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_ln(x, gain, bias, eps):
    mu = x.mean(dim=-1, keepdim=True)
    var = x.var(dim=-1, unbiased=False, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gain + bias


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


# (H, Hp, segs): widths 1 and 3, and two segments of 29 padded apart to 32
@pytest.mark.parametrize('H,Hp,segs', [(1, 4, 1), (3, 4, 1), (29, 32, 2)])
def test_oracle_matches_autograd(H, Hp, segs):
    rs = np.random.RandomState(7 + H)
    T, N, eps = 6, 4, 1e-5
    cols = LO.real_columns(H, Hp, segs)
    F = len(cols)
    assert F == segs * H
    slab = rs.randn(T, N, segs * Hp) * 1.5 + 0.4          # junk in the pad columns
    slab[0, 0, cols] = 0.0                                # a zero row: y = bias
    slab[1, 2, cols] = 3.25                               # a constant row: var 0
    gain, bias = rs.rand(F) + 0.5, rs.randn(F) * 0.3
    G = rs.randn(T, N, F)
    y, c = LO.ln_forward(slab[..., cols], gain, bias, eps)
    dx, dg, db = LO.ln_backward(G, c)
    st = torch.tensor(slab, requires_grad=True)
    gt = torch.tensor(gain, requires_grad=True)
    bt = torch.tensor(bias, requires_grad=True)
    yt = _torch_ln(st[..., torch.as_tensor(cols)], gt, bt, eps)
    (yt * torch.tensor(G)).sum().backward()
    assert _rel(y, yt.detach().numpy()) < 1e-10
    full = st.grad.numpy()
    assert _rel(dx, full[..., cols]) < 1e-10
    pad = np.setdiff1d(np.arange(segs * Hp), cols)
    assert not full[..., pad].any()                       # the pad columns take no part
    assert _rel(dg, gt.grad.numpy()) < 1e-10
    assert _rel(db, bt.grad.numpy()) < 1e-10
    assert np.allclose(y[0, 0], bias, rtol=0, atol=1e-12)
    assert np.allclose(y[1, 2], bias, rtol=0, atol=1e-12) and c['var'][1, 2] == 0.0
    # biased variance, epsilon inside the square root
    x00 = slab[2, 1, cols]
    assert abs(c['var'][2, 1] - np.mean((x00 - x00.mean()) ** 2)) < 1e-12
    assert abs(c['r'][2, 1] - 1.0 / np.sqrt(c['var'][2, 1] + eps)) < 1e-12


def test_layer_validation():
    from asr_study_amd.core import layers as L
    for kw in (dict(weights=[np.ones(3), np.zeros(3)]), dict(gain_init='zero'),
               dict(bias_init='one'), dict(gain_init='glorot_uniform')):
        with pytest.raises(NotImplementedError):
            L.LayerNormalization(**kw)
    for eps in (0.0, -1e-3):
        with pytest.raises(ValueError):
            L.LayerNormalization(epsilon=eps)
    ln = L.LayerNormalization()
    assert ln.epsilon == 1e-5
    x = L.Input(shape=(None, 12))
    assert ln(x).features == 12
    img = L.Reshape((-1, 3, 4))(x)
    y = L.LayerNormalization(epsilon=1e-3)(img)
    assert y.features == 12 and y.fc == (3, 4)


def _chain(H, device='cpu', seed=2):
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import ctc_model
    x_in = L.Input(name='inputs', shape=(None, 10))
    o = L.TimeDistributed(L.Dense(20))(x_in)
    o = L.LayerNormalization()(o)
    o = L.Activation(L.clipped_relu(3.0))(o)
    o = L.Bidirectional(L.SimpleRNN(H, activation='tanh'), merge_mode='concat')(o)
    o = L.LayerNormalization(epsilon=1e-3)(o)
    o = L.TimeDistributed(L.Dense(8))(o)
    return ctc_model(x_in, o, seed=seed, device=device)


def test_ctc_model_spec_layout_and_names(monkeypatch):
    from asr_study_amd.core import engine
    from asr_study_amd.core.callbacks import keras_layers
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = _chain(13)
    assert [s['type'] for s in m.spec] == ['dense', 'ln', 'act', 'birnn', 'ln', 'dense']
    assert m.spec[1] == {'type': 'ln', 'epsilon': 1e-5}
    assert m.spec[4] == {'type': 'ln', 'epsilon': 1e-3}
    l1, l2 = [s for s in m.stages if s.kind == 'ln']
    assert (l1.ld, l1.segs, l1.seg_H, l1.seg_Hp) == (20, 1, 20, 20)
    assert (l2.ld, l2.segs, l2.seg_H, l2.seg_Hp) == (32, 2, 13, 16)     # H 13 -> Hp 16
    # the Dense behind the second LN looks through it to the recurrent layer's real columns
    assert np.array_equal(m._real_rows(m.stages[5]), LO.real_columns(13, 16, 2))
    w = m.get_weights()
    shapes = [a.shape for a in w]
    assert shapes[2:4] == [(20,), (20,)] and shapes[10:12] == [(26,), (26,)]
    assert np.all(w[2] == 1) and np.all(w[3] == 0) and np.all(w[10] == 1) and np.all(w[11] == 0)
    # gain / bias of pad columns are zero in the flat parameters, and a set / get round trip holds
    rs = np.random.RandomState(0)
    w2 = [rs.randn(*a.shape).astype(np.float32) for a in w]
    m.set_weights(w2)
    assert all(np.array_equal(a, b) for a, b in zip(w2, m.get_weights()))
    host = m.params.numpy()
    pad = np.setdiff1d(np.arange(32), LO.real_columns(13, 16, 2))
    assert np.all(host[l2.og + pad] == 0) and np.all(host[l2.obeta + pad] == 0)
    assert np.array_equal(host[l2.og + LO.real_columns(13, 16, 2)], w2[10])
    # no l2 on gain or bias
    for off, n, l2c in m._segments:
        if off in (l1.og, l1.obeta, l2.og, l2.obeta):
            assert l2c == 0.0
    layers = keras_layers(m, w2)
    assert [n for n, _ in layers] == ['timedistributed_1', 'layernormalization_1',
                                      'bidirectional_1', 'layernormalization_2',
                                      'timedistributed_2']
    assert [n for n, _ in layers[1][1]] == ['layernormalization_1_gain:0',
                                            'layernormalization_1_bias:0']
    assert [n for n, _ in layers[3][1]] == ['layernormalization_2_gain:0',
                                            'layernormalization_2_bias:0']
    assert [a.shape for a in m.get_gradients()] == shapes


def test_width_limits_are_refused_at_model_build(monkeypatch):
    from asr_study_amd import ops
    from asr_study_amd.core import engine, layers as L
    from asr_study_amd.core.models import ctc_model
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    x_in = L.Input(name='inputs', shape=(None, 8))
    o = L.LayerNormalization()(L.TimeDistributed(L.Dense(ops.LN_MAX_WIDTH + 4))(x_in))
    with pytest.raises(NotImplementedError, match=str(ops.LN_MAX_WIDTH)):
        ctc_model(x_in, L.TimeDistributed(L.Dense(5))(o), device='cpu')
    o = L.LayerNormalization()(L.TimeDistributed(L.Dense(30))(x_in))
    with pytest.raises(NotImplementedError, match='multiple of 4'):
        ctc_model(x_in, L.TimeDistributed(L.Dense(5))(o), device='cpu')


def test_deep_speech2_layer_norm_stage_lists(monkeypatch):
    from asr_study_amd.core import engine
    from asr_study_amd.core.models import deep_speech2
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    kw = dict(num_features=16, num_hiddens=8, num_layers=2, conv_filters=4, device='cpu')
    plain = deep_speech2(**kw)
    for rnn, kind in (('lstm', 'bilstm'), ('gru', 'bigru')):
        m = deep_speech2(batch_norm='layer', rnn_type=rnn, **kw)
        assert [s.kind for s in m.stages] == ['noise', 'reshape', 'conv', 'ln', 'act', 'conv', 'ln',
                                              'act', 'reshape', 'ln', kind, 'ln', kind, 'dense']
        assert m.config['kwargs']['batch_norm'] == 'layer'
        assert ('rnn_type' in m.config['kwargs']) == (rnn == 'gru')
        assert all(s.clip == 0.0 for s in m.stages if s.kind == 'conv')
        assert not any(getattr(s, 'fused', False) for s in m.stages if s.kind == 'act')
        lns = [s for s in m.stages if s.kind == 'ln']
        # the conv images: one group of F * C features per frame, no per-channel grouping
        assert [(s.ld, s.segs, s.seg_H) for s in lns] == [(32, 1, 32), (16, 1, 16), (16, 1, 16),
                                                          (16, 1, 16)]
        assert all(s.eps == 1e-5 for s in lns)
        if rnn == 'lstm':
            assert m.n_params == plain.n_params + sum(2 * s.ld for s in lns)
        assert m.bn_running.numel() == plain.bn_running.numel()        # no running state
    assert 'batch_norm' not in plain.config['kwargs']
    with pytest.raises(ValueError, match="'layer'"):
        deep_speech2(batch_norm='group', **kw)


def test_default_layouts_unchanged(monkeypatch):
    """No existing model's layout or names move: the golden layout file of the default models
    still describes them (its own test checks the bytes; this one that LN added no stage, tensor
    or name to a model without it)."""
    from asr_study_amd.core import engine, params as P
    from asr_study_amd.core.models import brsmv1, deep_speech2
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    for m in (brsmv1(num_hiddens=8, num_layers=2, device='cpu'),
              deep_speech2(num_features=16, num_hiddens=8, num_layers=2, conv_filters=4,
                           batch_norm=True, device='cpu')):
        assert not any(s.kind == 'ln' for s in m.stages)
        names = [n for _, ns in P.keras_names(m.stages) for n in ns]
        assert not any('layernormalization' in n for n in names)
    with open(os.path.join(ROOT, 'tests', 'golden', 'param_layout.json')) as f:
        assert 'layernormalization' not in f.read()


def test_keras_config_round_trip(monkeypatch):
    from asr_study_amd.core import engine
    from asr_study_amd.core.models import deep_speech2
    from asr_study_amd.utils import keras_config as K
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    for m in (_chain(13),
              deep_speech2(num_features=16, num_hiddens=6, num_layers=2, conv_filters=4,
                           batch_norm='layer', rnn_type='gru', device='cpu')):
        cfg = K.model_config(m)
        lns = [l for l in json.loads(cfg)['config']['layers']
               if l['class_name'] == 'LayerNormalization']
        assert len(lns) == len([s for s in m.stages if s.kind == 'ln'])
        assert lns[0]['name'] == 'layernormalization_1'
        assert lns[0]['config']['gain_init'] == 'one' and lns[0]['config']['bias_init'] == 'zero'
        assert [l['config']['epsilon'] for l in lns] == [s.eps for s in m.stages if s.kind == 'ln']
        m2 = K.topology_from_config(cfg)
        assert m2.spec == m.spec
        rs = np.random.RandomState(1)
        w = [rs.randn(*a.shape).astype(np.float32) for a in m.get_weights()]
        m.set_weights(w)
        m2.set_weights(m.get_weights())
        assert all(np.array_equal(a, b) for a, b in zip(m2.get_weights(), w))


def test_hparams_take_batch_norm_layer_from_the_command_line():
    from asr_study_amd.utils.hparams import HParams
    kw = HParams().parse(['batch_norm', 'layer', 'rnn_type', 'lstm', 'num_hiddens', '8']).values()
    assert kw == {'batch_norm': 'layer', 'rnn_type': 'lstm', 'num_hiddens': 8}


def _c_type(ct):
    return {C.c_int: 'int', C.c_float: 'float', C.c_size_t: 'size_t', C.c_int64: 'int64_t',
            C.c_double: 'double'}[ct]


def test_ln_declarations_match_signatures(tmp_path):
    """gcc checks every asr_ln_* declaration of the header against a prototype generated from
    _lib.SIGNATURES (scalars from the ctypes types, pointers where ctypes passes void*)."""
    gcc = shutil.which('gcc') or shutil.which('cc')
    if gcc is None:
        pytest.fail('no C compiler on this machine')
    from asr_study_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'asr_hip.h')).read()
    names = sorted(n for n in _lib.SIGNATURES if n.startswith('asr_ln_'))
    assert names == ['asr_ln_bwd', 'asr_ln_fwd', 'asr_ln_max_width', 'asr_ln_workspace_bytes']
    checks = []
    for n in names:
        m = re.search(r'^(\w+)\s+%s\(([^;]*)\);' % n, hdr, re.S | re.M)
        assert m, n
        params = [p.strip() for p in m.group(2).split(',')]
        res, args = _lib.SIGNATURES[n]
        if params == ['void']:
            params = []
        assert len(params) == len(args), n
        proto = []
        for p, a in zip(params, args):
            if a is C.c_void_p:
                assert '*' in p or p.startswith('asr_stream_t '), (n, p)
                proto.append(re.sub(r'\s*\w+$', '', p))       # the header's pointer type
            else:
                assert '*' not in p, (n, p)
                proto.append(_c_type(a))
        checks.append('_Static_assert(__builtin_types_compatible_p(__typeof__(&%s), %s (*)(%s)), '
                      '"%s");' % (n, _c_type(res), ', '.join(proto) or 'void', n))
    src = tmp_path / 'ln_decl.c'
    src.write_text('#include <stdio.h>\n#include "asr_hip.h"\n' + '\n'.join(checks) +
                   '\nint main(void) { printf("%d\\n", ASR_HIP_ABI_VERSION); return 0; }\n')
    exe = tmp_path / 'ln_decl'
    subprocess.check_call([gcc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    assert int(subprocess.check_output([str(exe)]).decode()) == _lib.ABI_VERSION


def test_c_abi_argument_checks_without_a_device():
    """Every refusal is decided on the host, before anything is launched: the negative codes
    come back on a machine without a GPU."""
    from asr_study_amd import _lib, ops
    lib = _lib.load()
    assert lib.asr_ln_max_width() == ops.LN_MAX_WIDTH >= 4096
    ws = lib.asr_ln_workspace_bytes
    assert ws(500, 64, 64, 1280, 1280, 1280, 1) > 0
    assert ws(5, 3, 16, 3648, 1824, 1824, 2) > 0
    assert ws(5, 3, 16, 4096, 4096, 4096, 1) > 0
    for bad in ((0, 1, 16, 4, 1, 4, 1),             # T
                (1, 0, 16, 4, 1, 4, 1),             # N
                (1, 17, 16, 4, 1, 4, 1),            # N > n_pad
                (1, 1, 16, 6, 3, 6, 1),             # ld % 4
                (1, 1, 16, 4100, 8, 8, 1),          # ld over the limit
                (1, 1, 16, 8, 5, 4, 1),             # H > Hp
                (1, 1, 16, 8, 3, 6, 1),             # Hp % 4
                (1, 1, 16, 8, 3, 4, 3),             # segs * Hp > ld
                (1, 1, 16, 8, 0, 4, 1),             # H
                (1, 1, 16, 8, 3, 4, 0)):            # segs
        assert ws(*bad) == 0, bad
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += (-base) % 16                            # a 16-byte aligned host address: never read
    p = [C.c_void_p(base + 64 * k) for k in range(3)]
    geo = (1, 1, 16, 4, 1, 4, 1)
    fwd, bwd = lib.asr_ln_fwd, lib.asr_ln_bwd
    assert fwd(None, p[1], p[2], p[2], None, *geo, 1e-5, None) == -1
    assert fwd(p[0], p[0], p[2], p[2], None, *geo, 1e-5, None) == -1          # y aliases x
    assert fwd(p[0], p[1], p[2], p[2], None, *geo, 0.0, None) == -1           # eps
    assert fwd(C.c_void_p(base + 4), p[1], p[2], p[2], None, *geo, 1e-5, None) == -1   # alignment
    assert fwd(p[0], p[1], p[2], p[2], None, 1, 1, 16, 4100, 8, 8, 1, 1e-5, None) == -1
    assert b'4096' in lib.asr_last_error()
    assert bwd(p[0], p[1], p[2], None, None, p[2], p[2], *geo, p[0], 1 << 20, None) == -1   # stats
    assert bwd(p[0], p[1], p[2], p[2], p[1], p[2], p[2], *geo, p[0], 1 << 20, None) == -1   # alias
    assert bwd(p[0], p[1], p[2], p[2], None, p[2], p[2], *geo, p[0], 8, None) == -2         # workspace
    assert bwd(p[0], p[1], p[2], p[2], None, p[2], p[2], *geo, None, 0, None) == -2
