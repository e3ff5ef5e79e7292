"""CPU checks of relative positional self-attention: the float64 oracle against central
differences, its reduction to plain attention, the shift property that pins the sign and origin of
the relative index, the layer validation and head_dim limit, the spec / parameter layout / Keras
names, the Keras config round trip, the ctypes mirror of asr_relattn_args against the header, the
C ABI's refusals and LDS plan, the host check of the lengths, and the unchanged existing models."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import attention_oracle as AO
from tests import relattention_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('x', 'W_qkv', 'b_qkv', 'W_pos', 'bias_u', 'bias_v', 'W_o', 'b_o')


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _tiny(seed=0, T=7, N=3, F=5, heads=2, dh=3, n_out=4):
    rs = np.random.RandomState(seed)
    D = heads * dh
    p = dict(x=rs.randn(T, N, F), W_qkv=rs.randn(F, 3 * D) * 0.7, b_qkv=rs.randn(3 * D) * 0.3,
             W_pos=rs.randn(D, D) * 0.7, bias_u=rs.randn(heads, dh) * 0.5,
             bias_v=rs.randn(heads, dh) * 0.5, W_o=rs.randn(D, n_out) * 0.7,
             b_o=rs.randn(n_out) * 0.3)
    return p, heads, np.array([T, 1, 4]), rs.randn(T, N, n_out)


def _y(p, heads, lens):
    return RO.relmha_forward(*[p[k] for k in KEYS], heads=heads, lens=lens)


def test_oracle_gradients_match_central_differences():
    """dx, dW_qkv, db_qkv, dW_pos, dbias_u, dbias_v, dW_o, db_o of the loss sum(y * R) on a ragged
    case (lengths 7, 1, 4 of T = 7, two heads): <= 1e-6 relative, step 1e-5."""
    p, heads, lens, R = _tiny()
    y, c = _y(p, heads, lens)
    dx, g = RO.relmha_backward(R, c)
    got = dict(zip(KEYS, [dx] + g))
    h = 1e-5
    for k in KEYS:
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
        print('[relattn] d%s vs central differences: %.2e' % (k, err))
        assert err <= 1e-6, (k, err)
    # the key bias: a shift of all keys of a head adds (q_t + b_u) . c to a whole row
    D = heads * 3
    assert np.abs(got['b_qkv'][D:2 * D]).max() <= 1e-12 * np.abs(got['b_qkv']).max()


def test_reduces_to_plain_attention():
    """W_pos = 0 and both position biases 0: attention_oracle.attn_forward / backward to 1e-14."""
    p, heads, lens, R = _tiny(3)
    T, D = p['x'].shape[0], heads * 3
    qkv = p['x'] @ p['W_qkv'] + p['b_qkv']
    zero = np.zeros(D)
    for ln in (lens, None):
        out, c = RO.relattn_forward(qkv, np.zeros((2 * T - 1, D)), zero, zero, heads, ln)
        want, cw = AO.attn_forward(qkv.copy(), heads, ln)
        assert _rel(out, want) <= 1e-14 and _rel(c['lse'], cw['lse']) <= 1e-14
        dout = R @ p['W_o'].T
        dqkv = RO.relattn_backward(dout, c)[0]
        assert _rel(dqkv, AO.attn_backward(dout, cw)) <= 1e-13
    y, _ = _y(dict(p, W_pos=0 * p['W_pos'], bias_u=0 * p['bias_u'], bias_v=0 * p['bias_v']),
              heads, lens)
    want, _ = AO.mha_forward(p['x'], p['W_qkv'], p['b_qkv'], p['W_o'], p['b_o'], heads, lens)
    assert _rel(y, want) <= 1e-14


def shift_case(T, N, heads, dh, r_star, lens, seed=0):
    """Q = K = 0, b_u = 0, and pos / b_v with b_v . pos_r = 40 dh^.5 at r = r_star, 0 elsewhere
    (scale 1 / dh^.5: the score is 40 there): column 0 of every head's pos block is the indicator
    of r_star, b_v is 40 dh^.5 in that column.  -> qkv, pos, bias_u, bias_v."""
    rs = np.random.RandomState(seed)
    D = heads * dh
    qkv = np.zeros((T, N, 3 * D))
    qkv[:, :, 2 * D:] = rs.randn(T, N, D)
    pos = np.zeros((2 * T - 1, D))
    pos[r_star + T - 1, ::dh] = 1.0
    bias_v = np.zeros(D)
    bias_v[::dh] = 40.0 * np.sqrt(dh)
    return qkv, pos, np.zeros(D), bias_v


def test_shift_property_pins_the_relative_index():
    """out_t = v_{t - r*} for every t with 0 <= t - r* < len: r = t - u, query minus key.  The
    other keys carry e^-40 each against 1: the error is at most T e^-40 max|v| (relative)."""
    T, N, heads, dh = 12, 2, 2, 4
    lens = np.array([12, 7])
    for r_star in (3, -5, 0, 11, -6):
        qkv, pos, bu, bv = shift_case(T, N, heads, dh, r_star, lens)
        out, _ = RO.relattn_forward(qkv, pos, bu, bv, heads, lens)
        v = qkv[:, :, 2 * heads * dh:]
        seen = 0
        for n in range(N):
            for t in range(T):
                if 0 <= t - r_star < lens[n]:
                    assert np.abs(out[t, n] - v[t - r_star, n]).max() <= \
                        T * np.exp(-40.0) * 2 * np.abs(v).max()
                    seen += 1
        assert seen > 0


def test_relative_table():
    from asr_study_amd import ops
    pe = RO.relpos(5, 6)
    assert pe.shape == (9, 6) and np.array_equal(pe[4], [0, 1, 0, 1, 0, 1])     # r = 0
    assert abs(pe[4 + 3, 0] - np.sin(3.0)) < 1e-7 and abs(pe[4 - 3, 0] + np.sin(3.0)) < 1e-7
    assert abs(pe[4 - 2, 3] - np.cos(2 / 10000 ** (2 / 6))) < 1e-7
    assert np.array_equal(ops.relpos_table(5, 6).astype(np.float32).astype(np.float64), pe)
    # the non-negative half is the absolute table
    assert np.array_equal(pe[4:], AO.posenc(5, 6))
    # the table of the weight gradient: 1 off the ROUNDED cosine columns, exactly where they are
    # slow (cos x >= 1 / 2): the gradient of what the forward pass computes
    g, full = ops.relpos_grad_table(50, 64), ops.relpos_table(50, 64).astype(np.float32)
    assert g.dtype == np.float32 and np.array_equal(g[:, 0::2], full[:, 0::2])
    slow = full[:, 1::2] >= 0.5
    assert slow[:, -8:].all()
    assert np.array_equal(g[:, 1::2].astype(np.float64)[slow],
                          full[:, 1::2].astype(np.float64)[slow] - 1.0)
    assert np.abs(g[:, 1::2].astype(np.float64) - (full[:, 1::2].astype(np.float64) - 1.0)).max() \
        <= 2.0 ** -24
    # ... which changes nothing, because the rows of dS sum to zero: sum_r dpos_r = 0
    p, heads, lens, R = _tiny(5)
    _, c = _y(p, heads, lens)
    dpos = RO.relattn_backward(R @ p['W_o'].T, c)[1]
    assert np.abs(dpos.sum(axis=0)).max() < 1e-13 * np.abs(dpos).max()


def test_layer_validation_and_head_dim_limit():
    from asr_study_amd.core import layers as L
    x = L.Input(shape=(None, 48))
    a = L.RelativeMultiHeadAttention(3, W_regularizer=L.l2(0.1))
    assert a(x).features == 48 and (a.num_heads, a.head_dim, a.output_dim, a.l2) == (3, 16, 48, 0.1)
    b = L.RelativeMultiHeadAttention(2, head_dim=64, output_dim=20)
    assert b(x).features == 20 and b.head_dim == 64
    with pytest.raises(NotImplementedError, match='divide'):
        L.RelativeMultiHeadAttention(5)(x)
    with pytest.raises(NotImplementedError, match='16 .. 64'):
        L.RelativeMultiHeadAttention(4)(x)                      # dh 12
    for dh in (8, 24, 80, 128):
        with pytest.raises(NotImplementedError, match='16 .. 64'):
            L.RelativeMultiHeadAttention(2, head_dim=dh)
    with pytest.raises(NotImplementedError, match='16 .. 64'):
        L.RelativeMultiHeadAttention(2)(L.Input(shape=(None, 256)))     # dh 128
    for kw in (dict(attention_dropout=0.1), dict(causal=True)):
        with pytest.raises(NotImplementedError):
            L.RelativeMultiHeadAttention(3, **kw)
    with pytest.raises(NotImplementedError):
        L.RelativeMultiHeadAttention(0)
    assert L.MultiHeadAttention(2, head_dim=128).head_dim == 128        # (the plain layer's stays)


def _block(device='cpu', seed=2):
    """Dense(32) -> one pre-LN relative attention block -> LN -> Dense(8)."""
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import ctc_model
    x_in = L.Input(name='inputs', shape=(None, 10))
    o = L.TimeDistributed(L.Dense(32))(x_in)
    y = L.LayerNormalization()(o)
    y = L.RelativeMultiHeadAttention(2, W_regularizer=L.l2(1e-3))(y)
    o = L.merge([L.Dropout(0.0)(y), o], mode='sum')
    o = L.LayerNormalization()(o)
    o = L.TimeDistributed(L.Dense(8))(o)
    return ctc_model(x_in, o, seed=seed, device=device)


def test_ctc_model_spec_layout_and_names(monkeypatch):
    from asr_study_amd.core import engine
    from asr_study_amd.core.callbacks import keras_layers
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = _block()
    assert [s['type'] for s in m.spec] == ['dense', 'ln', 'mha', 'dropout', 'merge', 'ln', 'dense']
    assert m.spec[2] == {'type': 'mha', 'heads': 2, 'dh': 16, 'n_out': 32, 'l2': 1e-3,
                         'relative': True}
    s = m.stages[2]
    assert s.relative and (s.heads, s.dh, s.D, s.n_out, s.f_in_pad) == (2, 16, 32, 32, 32)
    assert m._has_mha and m._needs_lens
    w = m.get_weights()
    shapes = [a.shape for a in w]
    assert shapes[4:11] == [(32, 96), (96,), (32, 32), (2, 16), (2, 16), (32, 32), (32,)]
    lim = np.sqrt(6.0 / (32 + 32))
    for blk in np.split(w[4], 3, axis=1) + [w[6], w[9]]:
        assert 0.8 * lim < np.abs(blk).max() <= lim
    blim = np.sqrt(6.0 / (2 + 16))                      # glorot over (heads, dh)
    for b in (w[7], w[8]):
        assert 0.7 * blim < np.abs(b).max() <= blim
    assert not w[5].any() and not w[10].any() and not np.array_equal(w[7], w[8])
    rs = np.random.RandomState(0)
    w2 = [rs.randn(*a.shape).astype(np.float32) for a in w]
    m.set_weights(w2)
    assert all(np.array_equal(a, b) for a, b in zip(w2, m.get_weights()))
    host = m.params.numpy()
    assert np.array_equal(host[s.oWp:s.oWp + 32 * 32].reshape(32, 32), w2[6])
    assert np.array_equal(host[s.obu:s.obu + 32].reshape(2, 16), w2[7])
    assert np.array_equal(host[s.obv:s.obv + 32].reshape(2, 16), w2[8])
    l2 = {off: c for off, n, c in m._segments}
    assert [l2[o] for o in (s.oW, s.ob, s.oWp, s.obu, s.obv, s.oWo, s.obo)] == \
        [1e-3, 0.0, 1e-3, 0.0, 0.0, 1e-3, 0.0]
    layers = keras_layers(m, w2)
    assert [n for n, _ in layers] == ['timedistributed_1', 'layernormalization_1',
                                      'relativemultiheadattention_1', 'layernormalization_2',
                                      'timedistributed_2']
    assert [n for n, _ in layers[2][1]] == [
        'relativemultiheadattention_1_%s:0' % k
        for k in ('W_qkv', 'b_qkv', 'W_pos', 'pos_bias_u', 'pos_bias_v', 'W_o', 'b_o')]
    assert [a.shape for a in m.get_gradients()] == shapes
    # the head_dim limit is refused when the model is built, by name
    for dh in (20, 80, 128):
        with pytest.raises(NotImplementedError, match='16 .. 64'):
            engine.Model([{'type': 'mha', 'heads': 2, 'dh': dh, 'n_out': 40, 'l2': 0.0,
                           'relative': True}], 2 * dh, device='cpu')


def test_keras_config_round_trip(monkeypatch):
    from asr_study_amd.core import engine
    from asr_study_amd.utils import keras_config as K
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = _block()
    text = K.model_config(m)
    layers = {l['name']: l for l in json.loads(text)['config']['layers']}
    c = layers['relativemultiheadattention_1']
    assert c['class_name'] == 'RelativeMultiHeadAttention'
    assert (c['config']['num_heads'], c['config']['head_dim'], c['config']['output_dim']) == \
        (2, 16, 32)
    assert c['config']['W_regularizer']['l2'] == 1e-3
    assert not any(l['class_name'] == 'PositionalEncoding' for l in layers.values())
    m2 = K.topology_from_config(text)
    assert m2.spec == m.spec and m2.stages[2].relative
    assert [a.shape for a in m2.get_weights()] == [a.shape for a in m.get_weights()]
    assert K.model_config(m2) == text


@pytest.mark.parametrize('factory', ['transformer', 'conformer'])
def test_factories_take_positions(monkeypatch, factory):
    from asr_study_amd.core import engine, models
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    kw = dict(num_features=16, num_classes=7, d_model=32, num_heads=2, num_layers=2, d_ff=64,
              conv=False, device='cpu')
    f = getattr(models, factory)
    rel, plain = f(positions='relative', **kw), f(**kw)
    assert [s.kind for s in rel.stages] == [s.kind for s in plain.stages if s.kind != 'posenc']
    assert [getattr(s, 'relative', False) for s in rel.stages if s.kind == 'mha'] == [True, True]
    assert not any(hasattr(s, 'relative') for s in plain.stages)
    assert 'posenc' in [s.kind for s in plain.stages]
    assert rel.config['kwargs']['positions'] == 'relative'
    assert 'positions' not in plain.config['kwargs']
    assert 'positions' not in f(positions='absolute', **kw).config['kwargs']
    for bad in ('rel', None, True):
        with pytest.raises(ValueError, match='positions'):
            f(positions=bad, **kw)
    with pytest.raises(NotImplementedError, match='16 .. 64'):
        f(positions='relative', **dict(kw, d_model=256))          # dh 128
    from asr_study_amd.utils.hparams import HParams
    assert HParams().parse(['positions', 'relative']).values() == {'positions': 'relative'}
    rebuilt = getattr(models, rel.config['name'])(device='cpu', **rel.config['kwargs'])
    assert rebuilt.spec == rel.spec


def test_relattn_args_layout_matches_header(tmp_path):
    from asr_study_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    fields = [n for n, _ in _lib.RelAttnArgs._fields_]
    assert fields == ['T', 'N', 'n_pad', 'heads', 'dh', 'ld', 'ld_out', 'ld_pos', 'scale', 'qkv',
                      'lens', 'out', 'lse', 'dout', 'dqkv', 'pos', 'bias_u', 'bias_v', 'dpos',
                      'dbias_u', 'dbias_v']
    src = tmp_path / 'layout.c'
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "asr_hip.h"
int main(void) {
  printf("%%zu", sizeof(asr_relattn_args));
%s
  printf(" %%d\\n", ASR_HIP_ABI_VERSION);
  return 0;
}
''' % '\n'.join('  printf(" %%zu", offsetof(asr_relattn_args, %s));' % f for f in fields))
    exe = tmp_path / 'layout'
    subprocess.check_call([gcc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    A = _lib.RelAttnArgs
    assert got == [C.sizeof(A)] + [getattr(A, f).offset for f in fields] + [_lib.ABI_VERSION]
    assert _lib.ABI_VERSION == 107
    for name in ('asr_relattn_workspace_bytes', 'asr_relattn_fwd', 'asr_relattn_bwd',
                 'asr_relattn_plan'):
        assert name in _lib.SIGNATURES
    from asr_study_amd import build
    assert 'rel_attention.hip' in build.SOURCES
    assert any(d.endswith('attn_tile.h') for d in build._deps())


def test_c_abi_argument_checks_and_lds_without_a_device():
    """Every refusal is decided on the host, before anything is launched; the ABI number stays;
    every supported head_dim fits the 160 KB of a CU in both directions."""
    from asr_study_amd import _lib, ops
    lib = _lib.load()
    assert lib.asr_version() == 107
    for dh in (16, 32, 48, 64):
        for backward in (False, True):
            plan = ops.relattn_plan(130, 16, 2, dh, backward=backward)
            assert plan['bq'] == plan['bk'] == 64 and 0 < plan['lds'] <= 163840, (dh, plan)
            assert plan['blocks'] == 3 * 2 * 16
    assert ops.relattn_plan(130, 16, 2, 64, True)['lds'] > ops.relattn_plan(130, 16, 2, 64)['lds']
    a = _lib.RelAttnArgs()
    a.T, a.N, a.n_pad, a.heads, a.dh, a.ld, a.ld_out, a.ld_pos, a.scale = \
        8, 2, 16, 2, 32, 192, 64, 64, 0.25
    # D of every row, the two dQ slabs, the per-sample dpos partials
    assert lib.asr_relattn_workspace_bytes(C.byref(a)) >= \
        4 * (8 * 16 * 2 + 2 * 8 * 16 * 64 + 2 * 15 * 64)
    for k, v in (('dh', 24), ('dh', 80), ('dh', 128), ('dh', 8), ('heads', 0), ('T', 0),
                 ('N', 17), ('ld', 188), ('ld_out', 60), ('ld', 194), ('ld_pos', 60),
                 ('ld_pos', 66), ('scale', 0.0)):
        b = _lib.RelAttnArgs.from_buffer_copy(a)
        setattr(b, k, v)
        assert lib.asr_relattn_workspace_bytes(C.byref(b)) == 0, (k, v)
        assert lib.asr_relattn_fwd(C.byref(b), None) == -1, (k, v)
        assert lib.asr_relattn_bwd(C.byref(b), None, 0, None) == -1, (k, v)
        assert lib.asr_relattn_plan(C.byref(b), 0, None, None, None, None) == -1, (k, v)
        if k == 'dh' and v > 64:
            assert b'16..64' in lib.asr_last_error()            # the limit is named
    assert lib.asr_relattn_fwd(C.byref(a), None) == -1          # no pointers
    assert lib.asr_relattn_bwd(C.byref(a), None, 0, None) == -1
    assert lib.asr_relattn_fwd(None, None) == -1
    assert ops.RELATTN_MAX_HEAD_DIM == 64


def test_key_lengths_are_checked_on_the_host(monkeypatch):
    """A model with a relative attention stage refuses utterance lengths outside 1 .. T where they
    are still host arrays, as one with a plain mha stage does."""
    from asr_study_amd.core import engine
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = _block()
    assert m._key_lens([1, 10, 7], 10).tolist() == [1, 10, 7]
    for bad in ([0, 5], [5, 11]):
        with pytest.raises(ValueError, match='inputs_length'):
            m._key_lens(bad, 10)
    with pytest.raises(ValueError, match='inputs_length'):
        m._prep_labels([[1], [2]], [10, 12], 10)


def test_existing_models_unchanged(monkeypatch):
    """Spec, Keras config text and factory record of brsmv1(), deep_speech2(), transformer() and
    conformer() equal tests/golden/relattention_parent_models.json, recorded from the commit
    before this feature by tests/golden/gen_relattention_parent_models.py."""
    import importlib.util
    from asr_study_amd.core import engine
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    golden = os.path.join(ROOT, 'tests', 'golden')
    spec = importlib.util.spec_from_file_location(
        'gen_relattention_parent_models',
        os.path.join(golden, 'gen_relattention_parent_models.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(golden, 'relattention_parent_models.json')) as f:
        want = json.load(f)
    got = gen.record()
    assert sorted(got) == sorted(want) == sorted(gen.NAMES)
    for name in gen.NAMES:
        for key in ('spec', 'model_config', 'kwargs'):
            assert got[name][key] == want[name][key], (name, key)
        assert 'relative' not in json.dumps(want[name]['spec'])
        assert 'positions' not in want[name]['kwargs']
