"""CPU checks of the self-attention feature: the float64 oracle's gradients against central
differences, the masking properties, the layer validation, the ctc_model spec, the parameter
layout and Keras names, the Keras config round trip, the transformer factory's stage lists, the
ctypes mirror of asr_attn_args against the header, and the unchanged existing models."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import attention_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _tiny(seed=0, T=7, N=3, F=5, heads=2, dh=3, n_out=4):
    rs = np.random.RandomState(seed)
    D = heads * dh
    p = dict(x=rs.randn(T, N, F), W_qkv=rs.randn(F, 3 * D) * 0.7, b_qkv=rs.randn(3 * D) * 0.3,
             W_o=rs.randn(D, n_out) * 0.7, b_o=rs.randn(n_out) * 0.3)
    return p, heads, np.array([T, 1, 4]), rs.randn(T, N, n_out)


def _y(p, heads, lens):
    return AO.mha_forward(p['x'], p['W_qkv'], p['b_qkv'], p['W_o'], p['b_o'], heads, lens)


def test_oracle_gradients_match_central_differences():
    """dx, dW_qkv, db_qkv, dW_o, db_o (so dQ, dK, dV through the projection) of the loss
    sum(y * R) on a ragged case (lengths 7, 1, 4 of T = 7): <= 1e-6 relative."""
    p, heads, lens, R = _tiny()
    y, c = _y(p, heads, lens)
    dx, (dWq, dbq, dWo, dbo) = AO.mha_backward(R, c)
    got = dict(x=dx, W_qkv=dWq, b_qkv=dbq, W_o=dWo, b_o=dbo)
    h = 1e-5
    for k in got:
        num = np.zeros_like(p[k])
        flat, nf = p[k].reshape(-1), num.reshape(-1)
        for i in range(flat.size):
            old = flat[i]
            flat[i] = old + h
            up = float((_y(p, heads, lens)[0] * R).sum())
            flat[i] = old - h
            dn = float((_y(p, heads, lens)[0] * R).sum())
            flat[i] = old
            nf[i] = (up - dn) / (2 * h)
        err = _rel(got[k], num)
        print('[attn] d%s vs central differences: %.2e' % (k, err))
        assert err <= 1e-6, (k, err)


def test_masking_properties():
    p, heads, lens, R = _tiny(1)
    T, N = p['x'].shape[:2]
    y, c = _y(p, heads, lens)
    for n in range(N):
        assert not c['p'][n, :, :, lens[n]:].any()              # masked keys: p = 0
        assert np.allclose(c['p'][n].sum(axis=-1), 1.0, atol=1e-14)
    D = heads * 3
    dqkv = AO.attn_backward(R @ p['W_o'].T, c)
    for n in range(N):
        assert not dqkv[lens[n]:, n, D:].any()                  # ... and dK = dV = 0
        # padding frames are queries like any other (one key alone: p = 1, dS = 0, dQ = 0)
        assert dqkv[lens[n]:, n, :D].any() or lens[n] in (1, T)
    # the utterance of length 1: every query returns v_0
    v0 = (p['x'][0, 1] @ p['W_qkv'] + p['b_qkv'])[2 * D:]
    assert np.allclose(c['ctx'][:, 1], v0[None, :], atol=1e-14)
    # lens = T is lens = None
    full, _ = _y(p, heads, np.full(N, T))
    none, _ = _y(p, heads, None)
    assert np.array_equal(full, none)
    # an utterance's valid-frame outputs do not change when T grows by padding
    grown = dict(p, x=np.concatenate([p['x'], np.random.RandomState(2).randn(5, N, 5)], axis=0))
    y2, _ = _y(grown, heads, lens)
    for n in range(N):
        assert _rel(y2[:lens[n], n], y[:lens[n], n]) < 1e-13
    # the positional table
    pe = AO.posenc(9, 6)
    assert np.array_equal(pe[0], [0, 1, 0, 1, 0, 1])
    assert abs(pe[3, 0] - np.sin(3.0)) < 1e-7 and abs(pe[3, 3] - np.cos(3 / 10000 ** (2 / 6))) < 1e-7
    from asr_study_amd import ops
    assert np.array_equal(ops.posenc_table(9, 6).astype(np.float32).astype(np.float64), pe)


def test_layer_validation():
    from asr_study_amd.core import layers as L
    x = L.Input(shape=(None, 48))
    a = L.MultiHeadAttention(3, W_regularizer=L.l2(0.1))
    assert a(x).features == 48 and (a.num_heads, a.head_dim, a.output_dim, a.l2) == (3, 16, 48, 0.1)
    b = L.MultiHeadAttention(2, head_dim=32, output_dim=20)
    assert b(x).features == 20 and b.head_dim == 32
    assert L.PositionalEncoding()(x).features == 48
    with pytest.raises(NotImplementedError, match='divide'):
        L.MultiHeadAttention(5)(x)                              # heads do not divide the width
    with pytest.raises(NotImplementedError, match='multiple of 16'):
        L.MultiHeadAttention(4)(x)                              # dh 12
    for dh in (8, 24, 144):
        with pytest.raises(NotImplementedError, match='multiple of 16'):
            L.MultiHeadAttention(2, head_dim=dh)
    with pytest.raises(NotImplementedError, match='attention_dropout'):
        L.MultiHeadAttention(3, attention_dropout=0.1)
    with pytest.raises(NotImplementedError):
        L.MultiHeadAttention(3, causal=True)
    with pytest.raises(NotImplementedError):
        L.MultiHeadAttention(0)


def _block(device='cpu', seed=2):
    """Dense(32) -> PositionalEncoding -> one pre-LN attention block -> LN -> Dense(8)."""
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import ctc_model
    x_in = L.Input(name='inputs', shape=(None, 10))
    o = L.TimeDistributed(L.Dense(32))(x_in)
    o = L.PositionalEncoding()(o)
    y = L.LayerNormalization()(o)
    y = L.MultiHeadAttention(2, W_regularizer=L.l2(1e-3))(y)
    o = L.merge([L.Dropout(0.0)(y), o], mode='sum')
    o = L.LayerNormalization()(o)
    o = L.TimeDistributed(L.Dense(8))(o)
    return ctc_model(x_in, o, seed=seed, device=device)


def test_ctc_model_spec_layout_and_names(monkeypatch):
    from asr_study_amd.core import engine
    from asr_study_amd.core.callbacks import keras_layers
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = _block()
    assert [s['type'] for s in m.spec] == ['dense', 'posenc', 'ln', 'mha', 'dropout', 'merge',
                                           'ln', 'dense']
    assert m.spec[1] == {'type': 'posenc'}
    assert m.spec[3] == {'type': 'mha', 'heads': 2, 'dh': 16, 'n_out': 32, 'l2': 1e-3}
    assert m.spec[5] == {'type': 'merge', 'mode': 'sum', 'skip': 1}
    s = m.stages[3]
    assert (s.heads, s.dh, s.D, s.n_out, s.f_in_pad) == (2, 16, 32, 32, 32)
    w = m.get_weights()
    shapes = [a.shape for a in w]
    assert shapes[4:8] == [(32, 96), (96,), (32, 32), (32,)]
    lim = np.sqrt(6.0 / (32 + 32))                      # glorot per Q / K / V block
    for blk in np.split(w[4], 3, axis=1):
        assert 0.8 * lim < np.abs(blk).max() <= lim
    assert not w[5].any() and not w[7].any() and np.abs(w[6]).max() <= np.sqrt(6.0 / 64)
    rs = np.random.RandomState(0)
    w2 = [rs.randn(*a.shape).astype(np.float32) for a in w]
    m.set_weights(w2)
    assert all(np.array_equal(a, b) for a, b in zip(w2, m.get_weights()))
    host = m.params.numpy()
    assert np.array_equal(host[s.oW:s.oW + 32 * 96].reshape(32, 96), w2[4])
    assert np.array_equal(host[s.oWo:s.oWo + 32 * 32].reshape(32, 32), w2[6])
    l2 = {off: c for off, n, c in m._segments}
    assert (l2[s.oW], l2[s.ob], l2[s.oWo], l2[s.obo]) == (1e-3, 0.0, 1e-3, 0.0)
    layers = keras_layers(m, w2)
    assert [n for n, _ in layers] == ['timedistributed_1', 'layernormalization_1',
                                      'multiheadattention_1', 'layernormalization_2',
                                      'timedistributed_2']
    assert [n for n, _ in layers[2][1]] == ['multiheadattention_1_W_qkv:0',
                                            'multiheadattention_1_b_qkv:0',
                                            'multiheadattention_1_W_o:0',
                                            'multiheadattention_1_b_o:0']
    assert [a.shape for a in m.get_gradients()] == shapes
    # a head width the kernels do not have is refused when the model is built
    with pytest.raises(NotImplementedError, match='multiple of 16'):
        engine.Model([{'type': 'mha', 'heads': 2, 'dh': 20, 'n_out': 40, 'l2': 0.0}], 40,
                     device='cpu')


def test_keras_config_round_trip(monkeypatch):
    from asr_study_amd.core import engine
    from asr_study_amd.utils import keras_config as K
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = _block()
    text = K.model_config(m)
    layers = {l['name']: l for l in json.loads(text)['config']['layers']}
    c = layers['multiheadattention_1']
    assert c['class_name'] == 'MultiHeadAttention'
    assert (c['config']['num_heads'], c['config']['head_dim'], c['config']['output_dim']) == \
        (2, 16, 32)
    assert c['config']['W_regularizer']['l2'] == 1e-3 and c['config']['attention_dropout'] == 0.0
    assert layers['positionalencoding_1']['class_name'] == 'PositionalEncoding'
    assert [n[0] for n in layers['merge_1']['inbound_nodes'][0]] == ['dropout_1',
                                                                    'positionalencoding_1']
    m2 = K.topology_from_config(text)
    assert m2.spec == m.spec
    assert [a.shape for a in m2.get_weights()] == [a.shape for a in m.get_weights()]
    assert K.model_config(m2) == text


@pytest.mark.parametrize('conv', [True, False])
def test_transformer_stage_kinds(monkeypatch, conv):
    from asr_study_amd.core import engine
    from asr_study_amd.core.models import transformer
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = transformer(num_features=16, num_classes=7, d_model=32, num_heads=2, num_layers=2,
                    d_ff=64, dropout=0.1, conv=conv, conv_filters=4,
                    conv_kernels=((5, 7), (3, 5)), weight_decay=1e-4, device='cpu')
    front = ['reshape', 'conv', 'conv', 'reshape'] if conv else []
    block = ['ln', 'mha', 'dropout', 'merge', 'ln', 'dense', 'act', 'dense', 'dropout', 'merge']
    assert [s.kind for s in m.stages] == front + ['dense', 'posenc', 'dropout'] + 2 * block + \
        ['ln', 'dense']
    assert m.time_strides == ([2] if conv else [])
    if conv:
        assert [(s.st, s.sf, s.clip) for s in m.stages if s.kind == 'conv'] == [(2, 2, 20.0),
                                                                                (1, 2, 20.0)]
    mha = [s for s in m.stages if s.kind == 'mha']
    assert [(s.heads, s.dh, s.n_out, s.l2) for s in mha] == [(2, 16, 32, 1e-4)] * 2
    dense = [s.n_out for s in m.stages if s.kind == 'dense']
    assert dense == [32, 64, 32, 64, 32, 7]
    merges = [(i, s.skip) for i, s in enumerate(m.stages) if s.kind == 'merge']
    base = len(front) + 2                                   # the first Dropout's stage index
    assert merges == [(base + 4, base), (base + 10, base + 4), (base + 14, base + 10),
                      (base + 20, base + 14)]
    assert m.config['name'] == 'transformer' and m.config['kwargs']['conv'] is conv
    assert m.config['kwargs']['conv_kernels'] == [[5, 7], [3, 5]]
    assert m.num_classes == 7
    from asr_study_amd.utils.hparams import HParams
    kw = HParams().parse(['d_model', '32', 'num_heads', '2', 'conv', 'False']).values()
    assert kw == {'d_model': 32, 'num_heads': 2, 'conv': False}
    d = transformer(device='cpu')                           # the defaults: 6 blocks of 4 x 64
    assert [(s.heads, s.dh) for s in d.stages if s.kind == 'mha'] == [(4, 64)] * 6


def test_attn_args_layout_matches_header(tmp_path):
    from asr_study_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    fields = [n for n, _ in _lib.AttnArgs._fields_]
    assert fields == ['T', 'N', 'n_pad', 'heads', 'dh', 'ld', 'ld_out', 'scale', 'qkv', 'lens',
                      'out', 'lse', 'dout', 'dqkv']
    src = tmp_path / 'layout.c'
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "asr_hip.h"
int main(void) {
  printf("%%zu", sizeof(asr_attn_args));
%s
  printf(" %%d\\n", ASR_HIP_ABI_VERSION);
  return 0;
}
''' % '\n'.join('  printf(" %%zu", offsetof(asr_attn_args, %s));' % f for f in fields))
    exe = tmp_path / 'layout'
    subprocess.check_call([gcc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    A = _lib.AttnArgs
    assert got == [C.sizeof(A)] + [getattr(A, f).offset for f in fields] + [_lib.ABI_VERSION]
    assert _lib.ABI_VERSION == 107
    for name in ('asr_attn_workspace_bytes', 'asr_attn_fwd', 'asr_attn_bwd', 'asr_attn_plan',
                 'asr_posenc_add'):
        assert name in _lib.SIGNATURES


def test_c_abi_argument_checks_without_a_device():
    """Every refusal is decided on the host, before anything is launched."""
    from asr_study_amd import _lib, ops
    lib = _lib.load()
    plan = ops.attn_plan(130, 16, 2, 32)
    assert plan['bq'] >= 16 and plan['bk'] >= 16 and plan['lds'] <= 160 * 1024
    assert plan['blocks'] == -(-130 // plan['bq']) * 2 * 16
    assert ops.attn_plan(130, 16, 1, 128, backward=True)['lds'] <= 160 * 1024
    a = _lib.AttnArgs()
    a.T, a.N, a.n_pad, a.heads, a.dh, a.ld, a.ld_out, a.scale = 8, 2, 16, 2, 32, 192, 64, 0.25
    assert lib.asr_attn_workspace_bytes(C.byref(a)) >= 8 * 16 * 2 * 4
    for k, v in (('dh', 24), ('dh', 144), ('dh', 8), ('heads', 0), ('T', 0), ('N', 17),
                 ('ld', 188), ('ld_out', 60), ('ld', 194)):
        b = _lib.AttnArgs.from_buffer_copy(a)
        setattr(b, k, v)
        assert lib.asr_attn_workspace_bytes(C.byref(b)) == 0, (k, v)
        assert lib.asr_attn_fwd(C.byref(b), None) == -1, (k, v)
        assert lib.asr_attn_bwd(C.byref(b), None, 0, None) == -1, (k, v)
        assert lib.asr_attn_plan(C.byref(b), 0, None, None, None, None) == -1, (k, v)
    assert lib.asr_attn_fwd(C.byref(a), None) == -1         # no pointers
    assert lib.asr_posenc_add(None, None, None, 4, 2, 16, 8, 8, None) == -1
    assert ops.attn_lse_len(8, 16, 2) == 256


def test_existing_models_unchanged(monkeypatch):
    """Every model of the golden layout file (offsets, l2 segments, Keras names and shapes,
    recorded before this feature) is rebuilt and compared with it key by key, as
    tests/test_param_layout_host.py does; none of them has an mha or posenc stage."""
    import importlib.util
    from asr_study_amd.core import engine
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    golden = os.path.join(ROOT, 'tests', 'golden')
    spec = importlib.util.spec_from_file_location('gen_param_layout',
                                                  os.path.join(golden, 'gen_param_layout.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(golden, 'param_layout.json')) as f:
        layout = json.load(f)
    assert sorted(layout) == sorted(name for name, _, _ in gen.CASES)
    for name, factory, kwargs in gen.CASES:
        m = gen.build(factory, kwargs)
        assert not any(st['type'] in ('mha', 'posenc') for st in m.spec), name
        assert not m._has_mha
        got, _ = gen.record(m)
        assert sorted(got) == sorted(layout[name]), name
        for key in sorted(layout[name]):
            assert got[key] == layout[name][key], (name, key)


def test_key_lengths_are_checked_on_the_host(monkeypatch):
    """A model with an mha stage refuses utterance lengths outside 1 .. T where they are still
    host arrays (the kernel would clamp them silently); other models take what they took."""
    from asr_study_amd.core import engine
    from asr_study_amd.core.models import brsmv1
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = _block()
    assert m._key_lens([1, 10, 7], 10).tolist() == [1, 10, 7]
    for bad in ([0, 5], [5, 11]):
        with pytest.raises(ValueError, match='inputs_length'):
            m._key_lens(bad, 10)
    with pytest.raises(ValueError, match='inputs_length'):
        m._prep_labels([[1], [2]], [10, 12], 10)
    plain = brsmv1(num_hiddens=8, num_layers=1, device='cpu')
    assert plain._key_lens([0, 99], 10).tolist() == [0, 99]
