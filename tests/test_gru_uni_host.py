"""Host-only checks of the unidirectional GRU (K28): the oracle's carried state, the bare
``layers.GRU`` as a one-direction variant of the 'bigru' stage kind (spec, parameters, Keras names,
config, checkpoint), deep_speech2(bidirectional=False), what ``stream.check`` accepts, the ctypes
mirror of asr_gru_uni_args and every argument error of the four asr_gru_uni_* entry points, which
the library refuses before any device call."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gru_oracle as GO
from tests import gru_uni_oracle as GU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ['tanh', 'relu', 'linear', ('clipped_relu', 20.0)]


def _case(rs, T, N, H, masked):
    zx = rs.randn(T, N, 3 * H) * 2.0
    U = rs.randn(H, 3 * H) * (0.8 / np.sqrt(H))
    BU = ((rs.rand(N, H) > 0.25) / 0.75) if masked else None
    return zx, U, BU


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize('act', ACTS, ids=['tanh', 'relu', 'linear', 'clipped'])
@pytest.mark.parametrize('masked', [False, True])
def test_oracle_split_run_is_the_whole_run_exactly(act, masked):
    rs = np.random.RandomState(7)
    T, N, H = 9, 5, 6
    zx, U, BU = _case(rs, T, N, H, masked)
    h0 = 0.5 * rs.randn(N, H)
    for start in (None, h0):
        h, g = GU.recurrence_forward(zx, U, act, BU, start)
        for k in (1, 4, T - 1):
            ha, ga = GU.recurrence_forward(zx[:k], U, act, BU, start)
            hb, gb = GU.recurrence_forward(zx[k:], U, act, BU, ha[-1])
            assert np.array_equal(np.concatenate([ha, hb]), h)
            assert np.array_equal(np.concatenate([ga, gb]), g)


@pytest.mark.parametrize('act', ACTS, ids=['tanh', 'relu', 'linear', 'clipped'])
def test_oracle_zero_state_is_the_bidirectional_oracles_direction_0(act):
    rs = np.random.RandomState(8)
    zx, U, BU = _case(rs, 7, 4, 5, True)
    want_h, want_g = GO.recurrence_forward(zx, U, act, BU, reverse=False)
    for start in (None, np.zeros((4, 5))):
        h, g = GU.recurrence_forward(zx, U, act, BU, start)
        assert np.array_equal(h, want_h) and np.array_equal(g, want_g)
    # rm: r (.) h_prev (.) B_U, with h0 in front of frame 0
    h0 = rs.randn(4, 5)
    h, g = GU.recurrence_forward(zx, U, act, BU, h0)
    rm = GU.rm_of(h, g, BU, h0)
    assert np.array_equal(rm[0], g[0, :, 5:10] * (h0 * BU))
    assert np.array_equal(rm[3], g[3, :, 5:10] * (h[2] * BU))


def test_oracle_chunked_model_is_the_whole_model():
    m = _stack()
    stages = GU.stages_from_model(m)
    rs = np.random.RandomState(9)
    x = rs.randn(23, 3, 10)
    want, _ = GU.model_forward(stages, x)
    got = GU.model_stream(stages, x, [23, 23, 23], [1, 7, 3, 12])
    assert np.abs(got - want).max() < 1e-12


# ---------------------------------------------------------------- layer, spec, parameters
def _stack(mixed=False):
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import ctc_model
    x = L.Input(name='inputs', shape=(None, 10))
    o = x
    if mixed:
        o = L.TimeDistributed(L.Dense(12))(o)
        o = L.DepthwiseConvolution1D(3, causal=True)(o)
    o = L.GRU(10, activation='tanh', W_regularizer=L.l2(1e-4))(o)
    o = L.GRU(14, activation='relu', U_regularizer=L.l2(1e-4))(o)
    o = L.TimeDistributed(L.Dense(8))(o)
    return ctc_model(x, o, device='cpu')


def _ds2(**kw):
    from asr_study_amd.core.models import deep_speech2
    return deep_speech2(num_features=16, num_classes=7, num_hiddens=18, num_layers=2,
                        conv_filters=4, conv_kernels=((5, 7), (3, 5)), device='cpu', **kw)


def test_bare_gru_is_a_one_direction_bigru_stage():
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.callbacks import keras_layers
    x = L.Input(name='inputs', shape=(None, 10))
    assert L.GRU(10)(x).features == 10
    m = _stack()
    assert [s.kind for s in m.stages] == ['bigru', 'bigru', 'dense']
    assert m.spec[0]['directions'] == 1 and 'merge_mode' not in m.spec[0]
    s0, s1 = m.stages[:2]
    assert s0.directions == 1 and (s0.f_out, s0.f_out_pad) == (10, 12)
    assert (s1.f_in, s1.f_in_pad, s1.f_out, s1.f_out_pad) == (10, 12, 14, 16)
    assert not hasattr(s0, 'merge') and s0.bn is False
    assert [(t.layer, t.name, t.shape, t.block) for t in s0.tensors] == [
        ('gru', 'W', (10, 30), (12, 36)), ('gru', 'U', (10, 30), (12, 36)),
        ('gru', 'b', (30,), (36,))]
    assert [t.l2 for t in s0.tensors] == [1e-4, 0.0, 0.0]
    assert [t.l2 for t in s1.tensors] == [0.0, 1e-4, 0.0]
    assert [t.init[0] for t in s0.tensors] == ['uniform', 'orthogonal', 'blocks']
    assert s0.tensors[0].init[1] == np.sqrt(6.0 / (10 + 30))
    # the second layer reads the 10 real columns of the first's 12
    assert list(m._real_rows(s1)) == list(range(10))
    named = keras_layers(m, m.get_weights())
    assert [n for n, _ in named] == ['gru_1', 'gru_2', 'timedistributed_1']
    assert [n for n, _ in named[1][1]] == ['gru_2_W:0', 'gru_2_U:0', 'gru_2_b:0']
    # Keras-order round trip; pads stay zero
    rs = np.random.RandomState(0)
    new = [rs.randn(*a.shape).astype(np.float32) for a in m.get_weights()]
    m.set_weights(new)
    assert all(np.array_equal(a, b) for a, b in zip(new, m.get_weights()))
    flat = m.params.numpy()
    Up = flat[s0.oU:s0.oU + 12 * 36].reshape(12, 3, 12)
    assert np.all(Up[10:] == 0) and np.all(Up[..., 10:] == 0) and np.all(Up[:10, :, :10] != 0)
    # a wrapped and a bare GRU in one model: each counts its own kind
    o = L.Bidirectional(L.GRU(6))(x)
    o = L.GRU(6)(o)
    o = L.TimeDistributed(L.Dense(8))(o)
    from asr_study_amd.core.models import ctc_model
    m2 = ctc_model(x, o, device='cpu')
    assert [getattr(s, 'directions', 2) for s in m2.stages] == [2, 1, 2]
    assert [n for n, _ in keras_layers(m2, m2.get_weights())] == [
        'bidirectional_1', 'gru_1', 'timedistributed_1']
    assert list(m2._real_rows(m2.stages[1])) == list(range(6)) + list(range(8, 14))


def test_bare_gru_with_batch_norm_is_refused():
    from asr_study_amd.core import layers as L
    x = L.Input(name='inputs', shape=(None, 10))
    with pytest.raises(NotImplementedError) as e:
        L.GRU(10, batch_norm=True)(x)
    assert 'both directions' in str(e.value)
    L.Bidirectional(L.GRU(10, batch_norm=True))(x)         # inside the wrapper: as before


def test_deep_speech2_unidirectional():
    with pytest.raises(ValueError) as e:
        _ds2(bidirectional=False)
    assert 'unidirectional LSTM' in str(e.value)
    with pytest.raises(NotImplementedError):
        _ds2(bidirectional=False, rnn_type='gru', batch_norm='recurrent')
    assert 'bidirectional' not in _ds2(rnn_type='gru').config['kwargs']
    assert 'bidirectional' not in _ds2(rnn_type='gru', bidirectional=True).config['kwargs']
    for bn, extra in ((False, []), (True, ['bn']), ('layer', ['ln'])):
        m = _ds2(bidirectional=False, rnn_type='gru', batch_norm=bn)
        assert m.config['kwargs']['bidirectional'] is False
        rec = [s for s in m.stages if s.kind == 'bigru']
        assert len(rec) == 2 and all(s.directions == 1 and s.H == 18 for s in rec)
        dense = m.stages[-1]
        assert dense.kind == 'dense' and dense.f_in == 18
        assert all(k in [s.kind for s in m.stages] for k in extra)
        assert [s.dropout_W for s in rec] == [0.2, 0.2] and [s.l2_U for s in rec] == [1e-4] * 2


def test_keras_config_and_checkpoint_round_trip(tmp_path):
    from asr_study_amd.core import callbacks, engine
    from asr_study_amd.datasets import h5lite
    from asr_study_amd.utils import core_utils, keras_config as K
    m = _ds2(bidirectional=False, rnn_type='gru')
    rs = np.random.RandomState(1)
    m.set_weights([rs.randn(*a.shape).astype(np.float32) for a in m.get_weights()])
    cfg = json.loads(K.model_config(m))
    gru = [l for l in cfg['config']['layers'] if l['class_name'] == 'GRU']
    assert [l['name'] for l in gru] == ['gru_1', 'gru_2']
    assert not [l for l in cfg['config']['layers'] if l['class_name'] == 'Bidirectional']
    assert gru[0]['config']['output_dim'] == 18 and gru[0]['config']['consume_less'] == 'gpu'
    old = engine.DEFAULT_DEVICE
    engine.DEFAULT_DEVICE = 'cpu'
    try:
        m2 = K.topology_from_config(K.model_config(m))
        key = lambda mm: [(s.kind, getattr(s, 'directions', 2), getattr(s, 'H', None),
                           getattr(s, 'act', None), getattr(s, 'l2_U', None)) for s in mm.stages]
        assert key(m2) == key(m)
        fname = str(tmp_path / ('uni.' + ('h5' if h5lite.available() else 'npz')))
        callbacks.save_model(m, fname)
        m3 = core_utils.load_model(fname, mode='predict', decoder=False)
    finally:
        engine.DEFAULT_DEVICE = old
    assert m3.config == m.config and m3.config['kwargs']['bidirectional'] is False
    assert key(m3) == key(m)
    assert all(np.array_equal(a, b) for a, b in zip(m.get_weights(), m3.get_weights()))


def test_stream_check():
    from asr_study_amd.core import stream
    from asr_study_amd.core.stages import KINDS, stream_variant
    assert KINDS['bigru'].stream is None            # (the kind as such does not stream)
    m = _stack()
    assert stream.check(m, None) == (16, 0, None)
    assert callable(stream_variant(m.stages[0])) and stream_variant(m.stages[2]) is None
    assert stream.check(_stack(mixed=True), 3)[0] == 3
    # LayerNormalization and Dense around bare GRUs: per-frame stages, so the stack streams
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import ctc_model
    x = L.Input(name='inputs', shape=(None, 10))
    o = L.GRU(12)(L.LayerNormalization()(L.TimeDistributed(L.Dense(12))(x)))
    o = L.TimeDistributed(L.Dense(8))(L.LayerNormalization()(o))
    assert stream.check(ctc_model(x, o, device='cpu'), 4) == (4, 0, None)
    step, enc0, front = stream.check(_ds2(bidirectional=False, rnn_type='gru'), None)
    assert (step, front) == (16, (5, 3))
    bi = _ds2(rnn_type='gru')
    assert stream_variant([s for s in bi.stages if s.kind == 'bigru'][0]) is None
    with pytest.raises(ValueError) as e:
        stream.check(bi, None)
    assert 'a bigru stage reads the whole utterance' in str(e.value)
    # the normalisation between the two convolutions is the front-end's refusal, as before
    with pytest.raises(ValueError) as e:
        stream.check(_ds2(bidirectional=False, rnn_type='gru', batch_norm='layer'), None)
    assert 'lies before the convolution' in str(e.value)


# ---------------------------------------------------------------- the C ABI
FIELDS = ['clip', 'U', 'mask_u', 'zx', 'h', 'gates', 'rm', 'h0', 'h_last', 'dy', 'dy_ld', 'da',
          'db_part', 'dz_absmax']


def test_gru_uni_args_layout_matches_header(tmp_path):
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
  printf("%%zu", sizeof(asr_gru_uni_args));
%s
  printf(" %%d\\n", ASR_HIP_ABI_VERSION);
  return 0;
}
''' % '\n'.join('  printf(" %%zu", offsetof(asr_gru_uni_args, %s));' % f for f in FIELDS))
    exe = tmp_path / 'layout'
    subprocess.check_call([gcc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    G = _lib.GruUniArgs
    assert got == [C.sizeof(G)] + [getattr(G, f).offset for f in FIELDS] + [_lib.ABI_VERSION]
    assert [n for n, _ in G._fields_][:6] == ['T', 'n_pad', 'H', 'mode', 'activation', 'clip']
    assert _lib.ABI_VERSION == 107                  # additions only: the version stays


def _args(T=3, n_pad=16, H=8, **over):
    """A well-formed forward + BPTT argument block over host arrays no call ever reads (every
    call below is refused before the first device call), and what keeps them alive."""
    from asr_study_amd import _lib
    bufs = {n: np.zeros(T * n_pad * 3 * H, np.float32)
            for n in ('U', 'zx', 'h', 'gates', 'rm', 'h0', 'h_last', 'dy', 'da')}
    a = _lib.GruUniArgs()
    a.T, a.n_pad, a.H, a.mode, a.activation, a.clip = T, n_pad, H, 0, 0, 0.0
    for n, b in bufs.items():
        setattr(a, n, b.ctypes.data)
    a.h_last = None                 # (a forward-only field: the cases that need it set it)
    a.h0 = None
    a.dy_ld = H
    for k, v in over.items():
        setattr(a, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
    return a, bufs


def _refused(fn, a, *rest):
    from asr_study_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, fn)(C.byref(a), *rest)
    msg = lib.asr_last_error().decode()
    return rc, msg


BAD_SHAPES = [dict(H=6), dict(H=0), dict(n_pad=24), dict(n_pad=0), dict(T=0), dict(mode=2),
              dict(activation=3), dict(activation=7, clip=0.0)]


@pytest.mark.parametrize('bad', BAD_SHAPES, ids=[str(sorted(b.items())) for b in BAD_SHAPES])
def test_every_entry_point_refuses_a_bad_shape(bad):
    a, keep = _args(**bad)
    ws = np.zeros(1 << 16, np.uint8)
    none = (None, None, None, None)
    for backward in (0, 1):
        rc, msg = _refused('asr_gru_uni_plan', a, backward, *none)
        assert rc == -1 and msg.startswith('gru_uni:'), (rc, msg)
        from asr_study_amd import _lib
        assert _lib.load().asr_gru_uni_workspace_bytes(C.byref(a), backward) == 0
    for fn in ('asr_gru_uni_seq_fwd', 'asr_gru_uni_seq_bwd'):
        rc, msg = _refused(fn, a, ws.ctypes.data, ws.size, None)
        assert rc == -1 and msg.startswith('gru_uni:'), (fn, rc, msg)
    if 'mode' in bad:
        assert 'stepwise' in msg


def test_plan_is_the_bidirectional_plan_with_half_the_workgroups():
    from asr_study_amd import _lib
    lib = _lib.load()
    for n_pad, H in ((16, 4), (32, 36), (48, 132), (64, 100), (64, 512)):
        for backward in (0, 1):
            got, want = [], []
            for args, fn, out in ((_lib.GruUniArgs(), lib.asr_gru_uni_plan, got),
                                  (_lib.GruArgs(), lib.asr_gru_plan, want)):
                args.T, args.n_pad, args.H = 5, n_pad, H
                v = [C.c_int() for _ in range(4)]
                assert fn(C.byref(args), backward, *[C.byref(x) for x in v]) == 0
                out += [x.value for x in v]
            assert got[:3] == want[:3] and got[0] == 0 and 2 * got[3] == want[3]


def test_missing_pointers_alias_and_short_workspace_are_refused():
    from asr_study_amd import _lib
    lib = _lib.load()
    ws = np.zeros(1 << 20, np.uint8)
    a, keep = _args()
    need_f = lib.asr_gru_uni_workspace_bytes(C.byref(a), 0)
    need_b = lib.asr_gru_uni_workspace_bytes(C.byref(a), 1)
    assert 0 < need_f < need_b <= ws.size
    for fn, need in (('asr_gru_uni_seq_fwd', need_f), ('asr_gru_uni_seq_bwd', need_b)):
        rc, msg = _refused(fn, a, ws.ctypes.data, need - 1, None)
        assert rc == -1 and 'workspace' in msg, (fn, rc, msg)
        rc, msg = _refused(fn, a, None, need, None)
        assert rc == -1 and 'workspace' in msg, (fn, rc, msg)
    missing = {'asr_gru_uni_seq_fwd': ('U', 'h', 'gates', 'zx', 'rm'),
               'asr_gru_uni_seq_bwd': ('U', 'h', 'gates', 'dy', 'da')}
    for fn, names in missing.items():
        for n in names:
            a, keep = _args(**{n: None})
            rc, msg = _refused(fn, a, ws.ctypes.data, ws.size, None)
            assert rc == -1 and msg.startswith('gru_uni:'), (fn, n, rc, msg)
    for bad_ld in (4, 10):                      # below H; not a multiple of 4
        a, keep = _args(dy_ld=bad_ld)
        rc, msg = _refused('asr_gru_uni_seq_bwd', a, ws.ctypes.data, ws.size, None)
        assert rc == -1 and 'dy_ld' in msg
    # h_last == h0: the session ping-pongs two buffers
    state = np.zeros(16 * 8, np.float32)
    a, keep = _args(h0=state, h_last=state)
    rc, msg = _refused('asr_gru_uni_seq_fwd', a, ws.ctypes.data, ws.size, None)
    assert rc == -1 and 'h_last' in msg and 'h0' in msg
    # BPTT starts from the zero state
    a, keep = _args(h0=state)
    rc, msg = _refused('asr_gru_uni_seq_bwd', a, ws.ctypes.data, ws.size, None)
    assert rc == -1 and 'zero state' in msg
    assert lib.asr_gru_uni_plan(None, 0, None, None, None, None) == -1
    assert 'null' in lib.asr_last_error().decode()
