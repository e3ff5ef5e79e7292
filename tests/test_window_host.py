"""Host checks of limited-context attention and the causal depthwise convolution (K25): the
oracle's mask against the definition, the library's refusals and tile counts (no device is
touched), the layers' argument checks, specs, configs and the exported symbols."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from asr_study_amd import _lib as L
from tests import window_oracle as WO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1                    # ASR_ERR_INVALID of include/asr_hip.h

WINDOWS = [(1, -1, 0), (1, 0, 0), (16, 64, 0), (48, 100, 5), (64, 0, 0), (200, -1, 0)]
LENGTHS = [63, 64, 65, 130, 500]
NEW_SYMBOLS = ['asr_attn_win_fwd', 'asr_attn_win_bwd', 'asr_attn_win_plan', 'asr_relattn_win_fwd',
               'asr_relattn_win_bwd', 'asr_relattn_win_plan', 'asr_dwconv1d_pad_fwd',
               'asr_dwconv1d_pad_bwd']


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def _brute_mask(T, window):
    """The definition, frame by frame."""
    chunk, left, right = window
    m = np.zeros((T, T), bool)
    for t in range(T):
        c0 = (t // chunk) * chunk
        hi = c0 + chunk + right
        lo = 0 if left < 0 else max(0, c0 - left)
        for u in range(T):
            m[t, u] = lo <= u < hi
    return m


@pytest.mark.parametrize('window', WINDOWS + [(3, 2, 1), (1, 5, 5), (16, 16, 0), (7, 0, 3)])
def test_oracle_mask_is_the_definition(window):
    for T in (1, 7, 65, 130):
        m = _brute_mask(T, window)
        assert np.array_equal(WO.window_mask(T, window), m)
        lo, hi = WO.window_lo_hi(T, window)
        assert (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all()      # both monotone
        lens = np.array([T, 1, (T + 1) // 2])
        vis = WO.visible(T, window, lens, 3)
        for n in range(3):
            want = m.copy()
            want[:, lens[n]:] = False
            assert np.array_equal(vis[n], want)
    assert WO.window_mask(9, (1, -1, 0)).tolist() == np.tril(np.ones((9, 9), bool)).tolist()


def test_oracle_empty_rows_and_full_window():
    """A row with no visible key: out = lse = 0 and no gradient; (1, T, T) is the plain oracle."""
    from tests import attention_oracle as AO
    rs = np.random.RandomState(0)
    T, N, heads, dh = 70, 2, 2, 4
    qkv, dout = rs.randn(T, N, 3 * heads * dh), rs.randn(T, N, heads * dh)
    lens = np.array([70, 20])
    out, c = WO.attn_forward(qkv, heads, (16, 16, 0), lens)
    assert not out[48:, 1].any() and not c['lse'][48:, 1].any() and out[47, 1].any()
    dqkv = WO.attn_backward(dout, c)
    assert np.isfinite(dqkv).all() and not dqkv[48:, 1, :heads * dh].any()
    assert not dqkv[20:, 1, heads * dh:].any()
    full, cf = WO.attn_forward(qkv, heads, (1, T, T), lens)
    want, cw = AO.attn_forward(qkv, heads, lens)
    assert np.allclose(full, want, rtol=1e-12, atol=0) and np.allclose(cf['lse'], cw['lse'])


def _attn_args(T, heads=2, dh=32, n_pad=16):
    a = L.AttnArgs()
    a.T, a.N, a.n_pad, a.heads, a.dh = T, 1, n_pad, heads, dh
    a.ld, a.ld_out, a.scale = 3 * heads * dh, heads * dh, 1.0
    return a


def _relattn_args(T, heads=2, dh=32, n_pad=16):
    a = L.RelAttnArgs()
    a.T, a.N, a.n_pad, a.heads, a.dh = T, 1, n_pad, heads, dh
    a.ld, a.ld_out, a.ld_pos, a.scale = 3 * heads * dh, heads * dh, heads * dh, 1.0
    return a


@pytest.mark.parametrize('bad', [(0, -1, 0), (-3, 0, 0), (1, -2, 0), (1, 0, -1), None])
def test_invalid_windows_are_refused_without_a_device(lib, bad):
    """ASR_ERR_INVALID before any device call: the buffers are host memory no kernel could use."""
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 63) & ~63
    w = None if bad is None else C.byref(L.AttnWindow(*bad))
    pairs = C.c_longlong(-7)
    for args, stem in ((_attn_args(64), 'attn'), (_relattn_args(64), 'relattn')):
        for k in ('qkv', 'out', 'lse', 'dout', 'dqkv'):
            setattr(args, k, base)
        fwd, bwd = getattr(lib, 'asr_%s_win_fwd' % stem), getattr(lib, 'asr_%s_win_bwd' % stem)
        plan = getattr(lib, 'asr_%s_win_plan' % stem)
        assert fwd(C.byref(args), w, None) == ERR_INVALID
        assert b'window' in lib.asr_last_error()
        assert bwd(C.byref(args), w, base, 1 << 30, None) == ERR_INVALID
        assert b'window' in lib.asr_last_error()
        assert plan(C.byref(args), w, 0, None, None, None, None, C.byref(pairs)) == ERR_INVALID
        assert pairs.value == -7
    # a good window with a refused geometry is refused as before (dh 80 under K24)
    good = L.AttnWindow(16, 64, 0)
    assert lib.asr_relattn_win_plan(C.byref(_relattn_args(64, dh=80)), C.byref(good), 0, None,
                                    None, None, None, None) == ERR_INVALID
    assert lib.asr_attn_win_plan(C.byref(_attn_args(64, dh=80)), C.byref(good), 0, None, None,
                                 None, None, None) == 0


@pytest.mark.parametrize('k,pad_left', [(3, -1), (3, 3), (31, 31), (1, 1), (63, 100)])
def test_invalid_pad_left_is_refused_without_a_device(lib, k, pad_left):
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 63) & ~63
    geo = (8, 1, 16, 4, 4, k)                   # T, N, n_pad, C, ld, k
    assert lib.asr_dwconv1d_pad_fwd(base, base, base, None, base + 1024, *geo, pad_left,
                                    None) == ERR_INVALID
    assert b'pad_left' in lib.asr_last_error()
    assert lib.asr_dwconv1d_pad_bwd(base, base, base, None, base + 1024, base, base, *geo,
                                    pad_left, base, 1 << 30, None) == ERR_INVALID
    assert b'pad_left' in lib.asr_last_error()


@pytest.mark.parametrize('T', LENGTHS)
def test_tile_pairs_is_the_count_of_tiles_with_a_visible_pair(T):
    from asr_study_amd import ops
    tiles = (T + WO.TILE - 1) // WO.TILE
    for window in WINDOWS:
        want = WO.tile_pairs(T, window)
        for plan in (ops.attn_win_plan, ops.relattn_win_plan):
            for backward in (False, True):
                got = plan(T, 16, 2, 32, window, backward=backward)
                assert got['tile_pairs'] == want, (T, window, got)
                assert got['bq'] == got['bk'] == WO.TILE
    for plan, plain in ((ops.attn_win_plan, ops.attn_plan),
                        (ops.relattn_win_plan, ops.relattn_plan)):
        got = plan(T, 16, 2, 32, (1, T, T))
        assert got['tile_pairs'] == tiles * tiles                    # a window that hides nothing
        want = plain(T, 16, 2, 32)
        assert {k: got[k] for k in want} == want                     # LDS and blocks do not grow
        assert plan(T, 16, 2, 32, (1, T, T), backward=True)['lds'] == \
            plain(T, 16, 2, 32, backward=True)['lds']
    if T == 500:        # the cfg3-slab shape: about three quarters of the pairs are skipped
        assert ops.attn_win_plan(T, 64, 4, 64, (16, 64, 0))['tile_pairs'] == 15
        assert tiles * tiles == 64


def test_layer_argument_validation():
    from asr_study_amd.core import layers as Ly
    for cls in (Ly.MultiHeadAttention, Ly.RelativeMultiHeadAttention):
        assert cls(2).context is None
        assert cls(2, context='causal').context == (1, -1, 0)
        assert cls(2, context=[16, 64, 0]).context == (16, 64, 0)
        assert cls(2, context=(4, -1, 3)).context == (4, -1, 3)
        for bad in ('future', (1, 2), (1, 2, 3, 4), 5, (1.5, 0, 0), ('a', 0, 0), (True, 0, 0)):
            with pytest.raises(NotImplementedError):
                cls(2, context=bad)
        for bad in ((0, 0, 0), (1, -2, 0), (1, 0, -1)):
            with pytest.raises(ValueError):
                cls(2, context=bad)
    assert Ly.DepthwiseConvolution1D(7).causal is False
    assert Ly.DepthwiseConvolution1D(7, causal=True).causal is True
    with pytest.raises(NotImplementedError):
        Ly.DepthwiseConvolution1D(7, causal='left')
    with pytest.raises(NotImplementedError):
        Ly.DepthwiseConvolution1D(7, padding='causal')


SMALL = dict(num_features=16, num_classes=7, d_model=32, num_heads=2, num_layers=2, d_ff=64,
             dropout=0, conv=False, device='cpu')


@pytest.mark.parametrize('positions', ['absolute', 'relative'])
def test_specs_and_configs_of_default_models_are_unchanged(positions):
    """The new arguments add keys to the mha / dwconv specs only when set; without them the spec,
    the stage attributes and the factory record are what they were."""
    from asr_study_amd.core import models
    for factory, extra, new in ((models.transformer, {}, dict(context=[4, 8, 0])),
                                (models.conformer, dict(kernel_size=7, conv_norm='layer'),
                                 dict(context='causal', causal_conv=True))):
        kw = dict(SMALL, positions=positions, **extra)
        plain = factory(**kw)
        same = factory(**dict(kw, **{k: None if k == 'context' else False for k in new}))
        assert same.spec == plain.spec and same.config == plain.config
        assert 'context' not in plain.config['kwargs'] and 'causal_conv' not in plain.config['kwargs']
        for st in plain.spec:
            assert 'context' not in st and 'causal' not in st
        for s in plain.stages:
            assert not hasattr(s, 'window') and not hasattr(s, 'pad_left')
        windowed = factory(**dict(kw, **new))
        want = [4, 8, 0] if factory is models.transformer else [1, -1, 0]
        assert len(windowed.spec) == len(plain.spec)
        for a, b in zip(windowed.spec, plain.spec):                 # key by key
            added = {k: a[k] for k in a if k not in b}
            assert {k: a[k] for k in b} == b
            if a['type'] == 'mha':
                assert added == {'context': want}
            elif a['type'] == 'dwconv':
                assert added == {'causal': True}
            else:
                assert added == {}
        assert windowed.n_params == plain.n_params                  # no new parameters
        assert [t.name for s in windowed.stages for t in s.tensors] == \
            [t.name for s in plain.stages for t in s.tensors]
        assert [s.window for s in windowed.stages if s.kind == 'mha'] == [tuple(want)] * 2
        if factory is models.conformer:
            assert [s.pad_left for s in windowed.stages if s.kind == 'dwconv'] == [6, 6]
            assert windowed.config['kwargs']['causal_conv'] is True
        assert windowed.config['kwargs']['context'] == want


def test_config_round_trip_keeps_the_window(monkeypatch):
    """Both ways a saved model comes back: the factory record (callbacks.save_model writes
    model.config) and the layer graph of keras_config.model_config."""
    from asr_study_amd.core import engine, models
    from asr_study_amd.utils import keras_config as K
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    m = models.conformer(kernel_size=7, conv_norm='layer', positions='relative',
                         context=[4, 8, 0], causal_conv=True, **SMALL)
    record = json.loads(json.dumps(m.config))                       # as stored: JSON / YAML text
    rebuilt = getattr(models, record['name'])(device='cpu', **record['kwargs'])
    assert rebuilt.spec == m.spec
    text = K.model_config(m)
    graph = json.loads(text)['config']['layers']
    att = [l['config'] for l in graph if l['class_name'] == 'RelativeMultiHeadAttention']
    dwc = [l['config'] for l in graph if l['class_name'] == 'DepthwiseConvolution1D']
    assert [c['context'] for c in att] == [[4, 8, 0]] * 2 and [c['causal'] for c in dwc] == [True] * 2
    m2 = K.topology_from_config(text)
    assert m2.spec == m.spec
    assert [s.window for s in m2.stages if s.kind == 'mha'] == [(4, 8, 0)] * 2
    # without the arguments the config text has neither key
    plain = models.conformer(kernel_size=7, conv_norm='layer', **SMALL)
    assert '"context"' not in K.model_config(plain) and '"causal"' not in K.model_config(plain)
    # the command line hands the factory a list, 'causal' and True
    from asr_study_amd.utils.hparams import HParams
    kw = HParams().parse(['context', '[16, 64, 0]', 'causal_conv', 'True']).values()
    assert kw == {'context': [16, 64, 0], 'causal_conv': True}
    kw = HParams().parse(['context', 'causal', 'causal_conv', 'True']).values()
    m3 = models.conformer(kernel_size=7, conv_norm='layer', **dict(SMALL, **kw))
    assert m3.config['kwargs']['context'] == [1, -1, 0]


def test_new_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(ROOT, 'include', 'asr_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert re.search(r'typedef struct asr_attn_window \{ int chunk, left, right; \}', code)
    assert C.sizeof(L.AttnWindow) == 12
    assert [f[0] for f in L.AttnWindow._fields_] == ['chunk', 'left', 'right']
    assert lib.asr_version() == L.ABI_VERSION == 107                # additions only
    for doc in ('DESIGN.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        for name in NEW_SYMBOLS:
            assert name in text, (doc, name)
