"""-m gpu: limited-context attention (K25: the window of csrc/attn_tile.h on the kernels of
csrc/attention.hip and csrc/rel_attention.hip), the depthwise convolution with a chosen left
padding (csrc/dwconv.hip) and the models that use them, against the float64 oracle
(tests/window_oracle.py).  Kernel bound: 1e-5 max-norm relative; model bounds: 1e-4, as
tests/test_gpu_attention.py."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import window_oracle as WO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-5
NAMES = ('out', 'lse', 'dQ', 'dK', 'dV', 'dpos', 'dbias_u', 'dbias_v')


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


# ----------------------------------------------------------------------------- the attention kernels
def _make(rs, T, N, n_pad, heads, dh, lens, pad_cols=4):
    """Data at scale 1 in the real rows and columns (the biases at 0.5); junk at 3x the scale in
    the pad sample rows, the pad columns (of pos too) and the masked key frames of K and V."""
    D = heads * dh
    qkv = (rs.randn(T, n_pad, 3 * D + pad_cols) * 3.0).astype(np.float32)
    qkv[:, :N, :3 * D] = rs.randn(T, N, 3 * D).astype(np.float32)
    if lens is not None:
        for n in range(N):
            qkv[lens[n]:, n, D:3 * D] = (rs.randn(T - lens[n], 2 * D) * 3.0).astype(np.float32)
    dout = (rs.randn(T, n_pad, D + pad_cols) * 3.0).astype(np.float32)
    dout[:, :N, :D] = rs.randn(T, N, D).astype(np.float32)
    pos = (rs.randn(2 * T - 1, D + pad_cols) * 3.0).astype(np.float32)
    pos[:, :D] = rs.randn(2 * T - 1, D).astype(np.float32)
    return dict(qkv=qkv, dout=dout, pos=pos, bias_u=(rs.randn(D) * 0.5).astype(np.float32),
                bias_v=(rs.randn(D) * 0.5).astype(np.float32))


def _run(kind, d, N, heads, dh, lens, window):
    """kind 'attn' (K21) or 'rel' (K24); d: host float32 arrays of _make -> dict of host arrays.
    Outputs start from the sentinel 7.0: what is not written shows.  window None: the unwindowed
    entry points."""
    from asr_study_amd import ops
    T, n_pad, _ = d['qkv'].shape
    D = heads * dh
    q, do = _dev(d['qkv']), _dev(d['dout'])
    ld = None if lens is None else torch.tensor(np.asarray(lens, np.int32), device='cuda:0')
    out, out2 = torch.full_like(do, 7.0), torch.full_like(do, 7.0)
    lse = torch.full((ops.attn_lse_len(T, n_pad, heads),), 7.0, device='cuda:0')
    res = dict(out=out, lse=lse.view(T, n_pad, heads), out2=out2, dqkv=torch.full_like(q, 7.0))
    if kind == 'attn':
        ops.attn_fwd(q, out, N, heads, dh, lens=ld, lse=lse, window=window)
        ops.attn_fwd(q, out2, N, heads, dh, lens=ld, window=window)     # inference: nothing kept
        ops.attn_bwd(q, out, lse, do, res['dqkv'], N, heads, dh, lens=ld, window=window)
    else:
        pos, bu, bv = _dev(d['pos']), _dev(d['bias_u']), _dev(d['bias_v'])
        res.update(dpos=torch.full_like(pos, 7.0), dbias_u=torch.full((D,), 7.0, device='cuda:0'),
                   dbias_v=torch.full((D,), 7.0, device='cuda:0'))
        ops.relattn_fwd(q, pos, bu, bv, out, N, heads, dh, lens=ld, lse=lse, window=window)
        ops.relattn_fwd(q, pos, bu, bv, out2, N, heads, dh, lens=ld, window=window)
        ops.relattn_bwd(q, pos, bu, bv, out, lse, do, res['dqkv'], res['dpos'], res['dbias_u'],
                        res['dbias_v'], N, heads, dh, lens=ld, window=window)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in res.items()}


def _oracle(kind, d, N, heads, dh, lens, window):
    """Sample by sample -> dict over the real rows and columns, the largest |score| and the
    (N, T, T) visibility."""
    T, D = d['qkv'].shape[0], heads * dh
    out, lse, dqkv = np.zeros((T, N, D)), np.zeros((T, N, heads)), np.zeros((T, N, 3 * D))
    dpos, dbu, dbv, smax = np.zeros((2 * T - 1, D)), np.zeros(D), np.zeros(D), 0.0
    pos = d['pos'][:, :D].astype(np.float64)
    bu, bv = d['bias_u'].astype(np.float64), d['bias_v'].astype(np.float64)
    for n in range(N):
        x = d['qkv'][:, n:n + 1, :3 * D].astype(np.float64)
        ln = None if lens is None else lens[n:n + 1]
        do = d['dout'][:, n:n + 1, :D].astype(np.float64)
        if kind == 'attn':
            o, c = WO.attn_forward(x, heads, window, ln)
            dqkv[:, n:n + 1] = WO.attn_backward(do, c)
        else:
            o, c = WO.relattn_forward(x, pos, bu, bv, heads, window, ln)
            g = WO.relattn_backward(do, c)
            dqkv[:, n:n + 1] = g[0]
            dpos, dbu, dbv = dpos + g[1], dbu + g[2], dbv + g[3]
        out[:, n:n + 1], lse[:, n:n + 1] = o, c['lse']
        smax = max(smax, float(c['smax']))
    return dict(out=out, lse=lse, dqkv=dqkv, dpos=dpos, dbias_u=dbu, dbias_v=dbv, smax=smax,
                vis=WO.visible(T, window, lens, N))


def _parts(kind, r, N, D):
    p = (r['out'][:, :N, :D], r['lse'][:, :N], r['dqkv'][:, :N, :D], r['dqkv'][:, :N, D:2 * D],
         r['dqkv'][:, :N, 2 * D:3 * D])
    return p if kind == 'attn' else p + (r['dpos'][:, :D], r['dbias_u'], r['dbias_v'])


def _check(kind, tag, d, N, heads, dh, lens, window, zero_scale=None):
    """zero_scale: the size against which the gradients through dS are measured where the
    oracle's are exactly zero (every row sees a single key: p = 1, dS = 0); the sums over all
    (sample, frame) pairs (dpos, the biases) against T N times that.  window None: the unwindowed
    entry points, against the oracle under a window that hides nothing."""
    T, D = d['qkv'].shape[0], heads * dh
    got_all = _run(kind, d, N, heads, dh, lens, window)
    if window is None:
        window = (1, -1, T)
    want_all = _oracle(kind, d, N, heads, dh, lens, window)
    got, want = _parts(kind, got_all, N, D), _parts(kind, want_all, N, D)
    errs = [_rel(g, w) for g, w in zip(got, want)]
    if zero_scale is not None:
        for k in (2, 3, 5, 6, 7)[:2 if kind == 'attn' else 5]:
            assert not want[k].any()
            errs[k] = float(np.abs(got[k]).max() / (zero_scale * (T * N if k >= 5 else 1)))
    print('[window] %s %s %s: %s (bound %.1e, largest |s| %.1f)'
          % (kind, tag, window, ' '.join('%s %.2e' % kv for kv in zip(NAMES, errs)), BOUND,
             want_all['smax']))
    for k, a in got_all.items():            # (what is not written keeps the finite sentinel)
        assert np.isfinite(a).all(), (tag, k)
    for name, e in zip(NAMES, errs):
        assert e < BOUND, (kind, tag, window, name, e)
    assert np.array_equal(got_all['out'], got_all['out2']), tag     # with and without lse
    # padding rows and columns are written as exact zeros
    out, dqkv, vis = got_all['out'], got_all['dqkv'], want_all['vis']
    assert not out[:, N:].any() and not out[:, :, D:].any(), tag
    assert not dqkv[:, N:].any() and not dqkv[:, :, 3 * D:].any(), tag
    for n in range(N):
        if lens is not None:                                    # masked keys: dK = dV = 0
            assert not dqkv[lens[n]:, n, D:3 * D].any(), (tag, n)
        unseen = ~vis[n].any(axis=0)                            # keys no query sees: dK = dV = 0
        assert not dqkv[unseen, n, D:3 * D].any(), (tag, n)
        empty = ~vis[n].any(axis=1)                             # rows with no visible key
        assert not out[empty, n].any() and not got_all['lse'][empty, n].any(), (tag, n)
        assert not dqkv[empty, n, :D].any(), (tag, n)
    if kind == 'rel':
        dpos = got_all['dpos']
        assert not dpos[:, D:].any(), tag
        r = np.arange(T)[:, None] - np.arange(T)[None, :] + T - 1
        reached = np.zeros(2 * T - 1, bool)
        reached[np.unique(r[vis.any(axis=0)])] = True
        assert not dpos[~reached].any(), tag                    # table rows no visible pair reaches
        chunk, left, right = window
        rr = np.arange(-(T - 1), T)
        outside = (rr < -(chunk - 1 + right)) | ((rr > left + chunk - 1) if left >= 0 else False)
        assert not reached[outside].any() and not dpos[outside].any(), tag
    return got_all, want_all


def _ragged(T):
    """T, 1, a tile edge, one past it and 20, where T has room."""
    return np.array([T, 1, min(64, T), min(65, T), min(20, T)])


# (T, window) around the 64-frame tile; 2 heads of 32, n_pad 16
KERNEL_CASES = [(130, (1, -1, 0)), (130, (16, 16, 0)), (130, (48, 100, 5)), (130, (64, 0, 0)),
                (130, (64, 64, 0)), (130, (1, 5, 5)), (65, (16, 16, 0)), (63, (16, 16, 0)),
                (7, (3, 2, 1))]


@pytest.mark.parametrize('kind', ['attn', 'rel'])
@pytest.mark.parametrize('T,window', KERNEL_CASES, ids=['T%d-%d_%d_%d' % ((T,) + w)
                                                        for T, w in KERNEL_CASES])
def test_kernel_parity(kind, T, window):
    rs = np.random.RandomState(T + sum(window))
    lens = _ragged(T)
    d = _make(rs, T, 5, 16, 2, 32, lens)
    got, want = _check(kind, 'T=%d' % T, d, 5, 2, 32, lens, window)
    if (T, window) == (130, (16, 16, 0)):
        # len 20: the queries t >= 48 have lo(t) = 32 >= 20, rows with no visible key
        assert lens[4] == 20 and not want['vis'][4, 48:].any() and want['vis'][4, 47].any()
        assert not got['out'][48:, 4].any() and not got['lse'][48:, 4].any()
        assert got['out'][47, 4, :64].any()


@pytest.mark.parametrize('kind', ['attn', 'rel'])
@pytest.mark.parametrize('heads,dh', [(1, 16), (1, 64)])
def test_kernel_parity_other_head_sizes(kind, heads, dh):
    rs = np.random.RandomState(dh)
    lens = _ragged(130)
    d = _make(rs, 130, 5, 16, heads, dh, lens)
    _check(kind, 'dh=%d' % dh, d, 5, heads, dh, lens, (16, 16, 0))
    _check(kind, 'dh=%d null lens' % dh, d, 5, heads, dh, None, (48, 100, 5))


# every head size the dispatch knows (the relative family refuses dh > 64), so that each reaches
# its own instantiation: a kernel of another DH reads another pitch and misses by orders of magnitude
HEAD_SIZES = [('attn', dh) for dh in range(16, 129, 16)] + [('rel', dh) for dh in range(16, 65, 16)]


@pytest.mark.parametrize('window', [None, (16, 16, 0)], ids=['plain', '16_16_0'])
@pytest.mark.parametrize('kind,dh', HEAD_SIZES, ids=['%s-%d' % c for c in HEAD_SIZES])
def test_every_head_size_reaches_its_own_kernel(kind, dh, window):
    """T = 70: two tiles; one length inside the second tile, one inside the first.  Data differ
    per dh."""
    rs = np.random.RandomState(1000 + dh)
    lens = np.array([70, 41])
    d = _make(rs, 70, 2, 16, 1, dh, lens)
    _check(kind, 'dh=%d' % dh, d, 2, 1, dh, lens, window)


@pytest.mark.parametrize('kind', ['attn', 'rel'])
def test_each_query_sees_itself_only(kind):
    """(1, 0, 0): p = 1 on the diagonal, out = v bit for bit on the valid frames and 0 past them.
    dS = p (dO . v - D) is exactly 0 in the oracle, so what comes through it is measured against
    the size of the terms that cancel: scale |dO . v| max(|q| + |b|, |k|, |pos|)."""
    rs = np.random.RandomState(5)
    T, N, heads, dh = 130, 5, 2, 32
    D = heads * dh
    lens = _ragged(T)
    d = _make(rs, T, N, 16, heads, dh, lens)
    terms = np.abs(d['dout'][:, :N, :D].astype(np.float64) * d['qkv'][:, :N, 2 * D:3 * D])
    size = terms.reshape(T, N, heads, dh).sum(axis=-1).max() / np.sqrt(dh) * \
        max(np.abs(d['qkv'][:, :N, :D]).max() + 2.0, np.abs(d['qkv'][:, :N, D:2 * D]).max(),
            np.abs(d['pos'][:, :D]).max())
    got, _ = _check(kind, 'self', d, N, heads, dh, lens, (1, 0, 0), zero_scale=float(size))
    for n in range(N):
        assert np.array_equal(got['out'][:lens[n], n, :D], d['qkv'][:lens[n], n, 2 * D:3 * D])
        assert not got['out'][lens[n]:, n].any()


@pytest.mark.parametrize('kind', ['attn', 'rel'])
@pytest.mark.parametrize('T', [65, 130])
def test_a_window_that_hides_nothing_gives_the_unwindowed_bits(kind, T):
    rs = np.random.RandomState(T)
    lens = _ragged(T)
    d = _make(rs, T, 5, 16, 2, 32, lens)
    a = _run(kind, d, 5, 2, 32, lens, None)
    b = _run(kind, d, 5, 2, 32, lens, (1, T, T))
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k][:, :5] if a[k].ndim == 3 else a[k],
                              b[k][:, :5] if b[k].ndim == 3 else b[k]), k


@pytest.mark.parametrize('kind', ['attn', 'rel'])
def test_future_blindness_is_bit_exact(kind):
    """(16, 32, 0), T = 130: frame 80 is a chunk boundary, so no frame < 80 sees a frame >= 80.
    Replacing Q, K and V of all frames >= 80 (100x the scale) leaves out and lse at frames < 80
    bit-equal; with dout zero at frames >= 80 the keys >= 80 get dK = dV = exactly 0.  The mask is
    a select: an exact condition, which fails for an implementation that forgets one pass."""
    rs = np.random.RandomState(12)
    T, N, heads, dh, window = 130, 3, 2, 32, (16, 32, 0)
    D = heads * dh
    lens = np.array([130, 97, 81])
    d = _make(rs, T, N, 16, heads, dh, lens)
    d['dout'][80:] = 0
    a = _run(kind, d, N, heads, dh, lens, window)
    e = dict(d, qkv=d['qkv'].copy())
    e['qkv'][80:] = (rs.randn(T - 80, 16, e['qkv'].shape[2]) * 100.0).astype(np.float32)
    b = _run(kind, e, N, heads, dh, lens, window)
    for r in (a, b):
        assert all(np.isfinite(v[:, :N] if v.ndim == 3 else v).all() for v in r.values())
        assert not r['dqkv'][80:, :N, D:3 * D].any()
    assert np.abs(a['dqkv'][:80, :N, D:3 * D]).max() > 0
    assert np.array_equal(a['out'][:80], b['out'][:80])
    assert np.array_equal(a['lse'][:80, :N], b['lse'][:80, :N])
    assert not np.array_equal(a['out'][80:, :N], b['out'][80:, :N])
    # everything a frame < 80 contributes to or receives is unchanged as well
    assert np.array_equal(a['dqkv'][:80], b['dqkv'][:80])
    # ... and the unwindowed call does look ahead: the test sees what it is meant to see
    c, f = _run(kind, d, N, heads, dh, lens, None), _run(kind, e, N, heads, dh, lens, None)
    assert not np.array_equal(c['out'][:80, :N], f['out'][:80, :N])


@pytest.mark.parametrize('kind', ['attn', 'rel'])
def test_windowed_kernels_are_deterministic(kind):
    rs = np.random.RandomState(1)
    T, N = 200, 7
    lens = rs.randint(1, T + 1, size=N)
    d = _make(rs, T, N, 16, 2, 32, lens)
    a = _run(kind, d, N, 2, 32, lens, (16, 64, 0))
    b = _run(kind, d, N, 2, 32, lens, (16, 64, 0))
    for k in a:
        assert np.array_equal(a[k][:, :N] if a[k].ndim == 3 else a[k],
                              b[k][:, :N] if b[k].ndim == 3 else b[k]), k


# ----------------------------------------------------------------------------- dwconv, pad_left
DW_NAMES = ('y', 'dx', 'dw', 'db')


def _dw_make(rs, T, N, n_pad, C, ld, k, lens):
    x = (rs.randn(T, n_pad, ld) * 3.0).astype(np.float32)
    x[:, :N, :C] = rs.randn(T, N, C).astype(np.float32)
    for n in range(N):
        x[lens[n]:, n] = (rs.randn(T - lens[n], ld) * 3.0).astype(np.float32)
    dy = (rs.randn(T, n_pad, ld) * 3.0).astype(np.float32)
    dy[:, :N, :C] = rs.randn(T, N, C).astype(np.float32)
    return x, (rs.randn(k, C) * 0.5).astype(np.float32), (rs.randn(C) * 0.3).astype(np.float32), dy


def _dw_run(x, w, b, dy, N, C, k, lens, pad_left):
    from asr_study_amd import ops
    xd, wd, bd, dyd = _dev(x), _dev(w), _dev(b), _dev(dy)
    ld = torch.tensor(np.asarray(lens, np.int32), device='cuda:0')
    y, dx = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
    dw, db = torch.full_like(wd, 7.0), torch.full_like(bd, 7.0)
    ops.dwconv1d_fwd(xd, wd, bd, y, N, k, lens=ld, C_=C, pad_left=pad_left)
    ops.dwconv1d_bwd(xd, wd, dyd, dx, dw, db, N, k, lens=ld, C_=C, pad_left=pad_left)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (y, dx, dw, db)]


@pytest.mark.parametrize('k', [1, 3, 31, 63])
@pytest.mark.parametrize('T', [5, 64, 65, 130])
def test_dwconv_pad_left_parity(T, k):
    """Forward, dx, dw, db at the 1e-5 of tests/test_gpu_conformer.py's kernel test (T N <= 2100
    there as here: a single missing term shows), for the left paddings 0, (k - 1) / 2 and k - 1."""
    N, n_pad, C, ld = 5, 16, 8, 12
    lens = np.array([T, 0, 1, (T + 1) // 2, min(64, T)])
    rs = np.random.RandomState(T + k)
    x, w, b, dy = _dw_make(rs, T, N, n_pad, C, ld, k, lens)
    plain = _dw_run(x, w, b, dy, N, C, k, lens, None)
    for pad_left in sorted({0, (k - 1) // 2, k - 1}):
        got = _dw_run(x, w, b, dy, N, C, k, lens, pad_left)
        y, dx, dw, db = got
        wy, c = WO.dwconv_forward(x[:, :N, :C].astype(np.float64), w.astype(np.float64),
                                  b.astype(np.float64), pad_left, lens)
        wdx, wdw, wdb = WO.dwconv_backward(dy[:, :N, :C].astype(np.float64), c)
        errs = [_rel(y[:, :N, :C], wy), _rel(dx[:, :N, :C], wdx), _rel(dw, wdw), _rel(db, wdb)]
        print('[window] dwconv T=%d k=%d pad_left=%d: %s' % (
            T, k, pad_left, ' '.join('%s %.2e' % kv for kv in zip(DW_NAMES, errs))))
        for a in got:
            assert np.isfinite(a).all()
        for name, e in zip(DW_NAMES, errs):
            assert e < BOUND, (T, k, pad_left, name, e)
        assert not y[:, N:].any() and not y[:, :, C:].any()
        assert not dx[:, N:].any() and not dx[:, :, C:].any()
        for n in range(N):
            assert not dx[lens[n]:, n].any()
        if pad_left == (k - 1) // 2:                    # the existing entry points are this call
            assert all(np.array_equal(u, v) for u, v in zip(got, plain))


@pytest.mark.parametrize('k', [3, 31, 63])
def test_causal_dwconv_reads_no_later_frame(k):
    """pad_left = k - 1: changing the frames >= t0 leaves the outputs < t0 bit-equal; with
    (k - 1) / 2 it does not."""
    T, N, n_pad, C, ld, t0 = 130, 3, 16, 8, 8, 70
    lens = np.array([130, 100, 71])
    rs = np.random.RandomState(k)
    x, w, b, dy = _dw_make(rs, T, N, n_pad, C, ld, k, lens)
    x2 = x.copy()
    x2[t0:] = (rs.randn(T - t0, n_pad, ld) * 100.0).astype(np.float32)
    a = _dw_run(x, w, b, dy, N, C, k, lens, k - 1)
    c = _dw_run(x2, w, b, dy, N, C, k, lens, k - 1)
    assert np.array_equal(a[0][:t0], c[0][:t0]) and not np.array_equal(a[0][t0:], c[0][t0:])
    a = _dw_run(x, w, b, dy, N, C, k, lens, (k - 1) // 2)
    c = _dw_run(x2, w, b, dy, N, C, k, lens, (k - 1) // 2)
    assert not np.array_equal(a[0][:t0], c[0][:t0])


# ----------------------------------------------------------------------------- models
def _randomise(model, rs):
    """LN gain / bias and the depthwise bias away from their start values."""
    w = model.get_weights()
    k = 0
    for s in model.stages:
        if s.kind == 'ln':
            n = w[k].size
            w[k] = (rs.rand(n) + 0.5).astype(np.float32)
            w[k + 1] = (rs.randn(n) * 0.2).astype(np.float32)
        elif s.kind == 'dwconv':
            w[k + 1] = (rs.randn(w[k + 1].size) * 0.2).astype(np.float32)
        k += len(s.tensors)
    model.set_weights(w)


def _parity(model, x, lens, labels, tag):
    """The scheme and bounds of tests/test_gpu_attention.py: logits, per-sample CTC, every
    gradient, predict, three Adam steps."""
    N = x.shape[0]
    slab = model.to_slab(x)
    stages = WO.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    ctc, logits, sl = model.loss_and_grads(slab, labels, lens, training=True)
    torch.cuda.synchronize()
    want = WO.loss_and_grads(stages, x64, labels, lens)
    e = _rel(logits[:, :N].cpu().numpy(), want['logits'])
    print('[window] %s logits rel err %.3e' % (tag, e))
    assert e < 1e-4, tag
    assert _rel(ctc.cpu().numpy()[:N], want['ctc']) < 1e-4, tag
    got = model.get_gradients()
    assert len(got) == len(want['grads'])
    for k, (g, gw) in enumerate(zip(got, want['grads'])):
        err = np.abs(g - gw).max()
        print('[window] %s grad %d %s err %.3e of %.3e' % (tag, k, g.shape, err, np.abs(gw).max()))
        assert err < 1e-4 * np.abs(gw).max() + 1e-7, (tag, k, err)
    model.decoder = None
    want_i, _ = WO.model_forward(stages, x64, lens, training=False)
    got_i = model.predict(x, lens)
    model.decoder = {'is_greedy': True}
    assert _rel(got_i.transpose(1, 0, 2), want_i) < 1e-4, tag
    from oracle import optim as OO
    opt = OO.Adam(lr=1e-3, clipnorm=400.0)
    for _ in range(3):
        m = model.train_on_batch([('slab', slab), labels, lens])
        out = WO.train_step(stages, x64, labels, lens, opt)
    assert abs(m[1] - float(np.mean(out['ctc']))) < 1e-4 * abs(m[1])
    for k, (a, b) in enumerate(zip(WO.weights(stages), model.get_weights())):
        err = np.abs(b - a).max()
        assert err < 5e-5 * max(1.0, np.abs(a).max()), (tag, 'w', k, err)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def _blocks(context, seed=2):
    """Dense(32) -> PositionalEncoding -> two pre-LN blocks (2 heads of 16, d_ff 48) -> LN ->
    Dense(8), the blocks of tests/test_gpu_attention.py with a window."""
    from asr_study_amd.core import layers as L, optimizers
    from asr_study_amd.core.models import ctc_model
    x_in = L.Input(name='inputs', shape=(None, 10))
    o = L.TimeDistributed(L.Dense(32))(x_in)
    o = L.PositionalEncoding()(o)
    for _ in range(2):
        y = L.MultiHeadAttention(2, context=context)(L.LayerNormalization()(o))
        o = L.merge([L.Dropout(0.0)(y), o], mode='sum')
        y = L.TimeDistributed(L.Dense(48))(L.LayerNormalization()(o))
        y = L.TimeDistributed(L.Dense(32))(L.Activation('relu')(y))
        o = L.merge([L.Dropout(0.0)(y), o], mode='sum')
    o = L.TimeDistributed(L.Dense(8))(L.LayerNormalization()(o))
    model = ctc_model(x_in, o, seed=seed)
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    return model


def _conformer(context=(4, 8, 0), causal_conv=True, seed=1, **kw):
    """Model (b): a small streaming conformer with relative positions."""
    from asr_study_amd.core import models, optimizers
    args = dict(num_features=10, num_classes=8, d_model=32, num_heads=2, num_layers=2, d_ff=64,
                kernel_size=7, conv_norm='layer', conv=False, dropout=0, context=context,
                causal_conv=causal_conv, positions='relative', seed=seed)
    args.update(kw)
    m = models.conformer(**args)
    m.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    return m


def _batch(rs, N, T, F, lens):
    x = rs.randn(N, T, F).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    return x


@pytest.mark.parametrize('build', ['blocks', 'conformer'])
def test_windowed_models_vs_oracle(build):
    rs = np.random.RandomState(4)
    N, T, F, C = 6, 21, 10, 8
    model = _blocks((4, 8, 0)) if build == 'blocks' else _conformer()
    _randomise(model, rs)
    assert [s.window for s in model.stages if s.kind == 'mha'] == [(4, 8, 0)] * 2
    lens = np.array([21, 15, 21, 8, 12, 21])
    x = _batch(rs, N, T, F, lens)
    labels = [rs.randint(0, C - 1, size=k).tolist() for k in (3, 2, 4, 1, 2, 3)]
    _parity(model, x, lens, labels, build)


def test_model_look_ahead_is_bounded():
    """Model (b) in predict mode, T = 40, one utterance: frame 20 is a boundary of chunk 4, right
    is 0 and the convolutions are causal, so the look-ahead past the chunk is 0 frames: the
    logits at frames < 20 are bit-equal between the utterance and a copy whose frames >= 20 are
    replaced.  With context=None they differ (that guards the test)."""
    rs = np.random.RandomState(9)
    x = rs.randn(1, 40, 10).astype(np.float32)
    x2 = x.copy()
    x2[:, 20:] = rs.randn(1, 20, 10).astype(np.float32) * 3.0
    for context, same in (((4, 8, 0), True), (None, False)):
        model = _conformer(context=context)
        _randomise(model, rs)
        model.decoder = None
        a, b = model.predict(x, [40]), model.predict(x2, [40])
        assert np.isfinite(a).all() and np.isfinite(b).all() and np.abs(a).max() > 0
        assert np.array_equal(a[:, :20], b[:, :20]) == same, context
        assert not np.array_equal(a[:, 20:], b[:, 20:])
    # a causal window with the 'same' convolution looks (k - 1) / 2 frames ahead per module
    model = _conformer(context=(4, 8, 0), causal_conv=False)
    model.decoder = None
    a, b = model.predict(x, [40]), model.predict(x2, [40])
    assert not np.array_equal(a[:, :20], b[:, :20])


def test_model_look_ahead_with_the_front_end():
    """conv=True with the small front-end of tests/test_gpu_attention.py's _small_transformer,
    kernels (5, 7) and (3, 5): the formula of the factory docstrings.  The encoder's look-ahead
    A is chunk - 1 = 3 strided frames past the first frame c0 of a chunk; the frames of that
    chunk read the input frames up to 2 (c0 + A + (kt2 - 1) // 2) + kt1 - 1 - p1 with
    p1 = (kt1 - 2) // 2 = 1 for the even T = 80: 2 (c0 + 3 + 1) + 3 = 2 c0 + 11.  The input
    changes from frame 60 on: the chunks up to c0 = 24 (2 * 24 + 11 = 59) read nothing from
    there, the chunk at 28 does.  Equality is asserted for the strided frames < 28 only."""
    rs = np.random.RandomState(10)
    kt1, kt2, chunk, T, change = 5, 3, 4, 80, 60
    p1 = (kt1 - 2) // 2
    reach = lambda t: 2 * (t // chunk * chunk + chunk - 1 + (kt2 - 1) // 2) + kt1 - 1 - p1
    safe = max(t for t in range(T // 2) if reach(t) < change) + 1
    assert safe == 28 and reach(safe) >= change
    x = rs.randn(1, T, 16).astype(np.float32)
    x2 = x.copy()
    x2[:, change:] = rs.randn(1, T - change, 16).astype(np.float32) * 3.0
    for context, same in (((chunk, 8, 0), True), (None, False)):
        model = _conformer(context=context, num_features=16, conv=True, conv_filters=4,
                           conv_kernels=((kt1, 7), (kt2, 5)))
        _randomise(model, rs)
        model.decoder = None
        a, b = model.predict(x, [T]), model.predict(x2, [T])
        assert a.shape[1] == T // 2 and np.isfinite(a).all()
        assert np.array_equal(a[:, :safe], b[:, :safe]) == same, context
        assert not np.array_equal(a[:, safe:], b[:, safe:])


def test_truncation_independence():
    """lens = [40] against lens = [20] on the same slab: the logits at frames < 20 agree to 1e-6
    relative, the bound of test_time_padding_independence (different key-loop ends reorder
    nothing but may skip tiles)."""
    rs = np.random.RandomState(13)
    model = _conformer()
    _randomise(model, rs)
    model.decoder = None
    x = rs.randn(1, 40, 10).astype(np.float32)
    a, b = model.predict(x, [40]), model.predict(x, [20])
    e = _rel(b[:, :20], a[:, :20])
    print('[window] truncation 40 vs 20: rel %.2e' % e)
    assert e < 1e-6


def learn_setup(device=None, context=(4, 8, 0)):
    """learn_setup of tests/test_gpu_attention.py with a window on every block (the factory
    argument is the only difference, so that function cannot be called as it is)."""
    from asr_study_amd.core import models, optimizers
    kw = {} if device is None else {'device': device}
    model = models.transformer(conv=False, num_features=16, num_classes=12, d_model=32,
                               num_heads=2, num_layers=2, d_ff=64, dropout=0, seed=3,
                               context=context, **kw)
    model.compile(optimizer=optimizers.Adam(lr=3e-3, clipnorm=400))
    rs = np.random.RandomState(0)
    x = rs.randn(4, 60, 16).astype(np.float32)
    lab = [list(rs.randint(1, 11, size=5)) for _ in range(4)]
    return model, x, lab


# the oracle's greedy LER is 0 first at this step: `python tools/window_learn_oracle.py` (host)
# runs WO.train_step on learn_setup() and prints it
ORACLE_LER0_STEP = 180


def test_windowed_transformer_learns_a_fixed_batch():
    """Overfits the 4 utterances of tests/test_gpu_attention.py's learning test under the window
    (4, 8, 0) to greedy LER 0; the float64 oracle's train_step, run on the host from the same
    initial weights, reaches it at ORACLE_LER0_STEP; the test allows twice that."""
    model, x, lab = learn_setup()
    slab = model.to_slab(x)
    cap = 2 * ORACLE_LER0_STEP
    ler = None
    for step in range(1, cap + 1):
        m = model.train_on_batch([('slab', slab), lab, np.full(4, 60)])
        ler = m[3]
        if ler == 0.0:
            break
    print('[learn] windowed transformer greedy LER 0 at step %d (oracle %d, cap %d)'
          % (step, ORACLE_LER0_STEP, cap))
    assert ler == 0.0, (step, m)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def test_cli_roundtrip_streaming_conformer(tmp_path):
    sys.path.insert(0, ROOT)
    import train
    import predict as predict_cli
    from asr_study_amd import cli
    from asr_study_amd.datasets import h5lite
    from asr_study_amd.utils import core_utils
    fmt = 'h5' if h5lite.available() else 'npz'
    fname = str(tmp_path / ('dummy.' + fmt))
    cli.make_dataset_main(['--parser', 'dummy', '--parser_params', 'num_speakers', '4',
                           'num_utterances_per_speaker', '6', 'max_duration', '1.2',
                           'min_duration', '0.6', 'max_label_length', '8', 'split',
                           '[0.5, 0.25]', 'seed', '3', '--input_parser', 'logfbank',
                           '--input_parser_params', 'num_filt', '16', '--output_file', fname])
    out = str(tmp_path / 'run')
    train.main(['--dataset', fname, '--model', 'conformer', '--model_params', 'num_features',
                '16', 'd_model', '32', 'num_heads', '2', 'num_layers', '2', 'd_ff', '64',
                'kernel_size', '7', 'num_classes', '28', 'conv_filters', '4', 'conv_kernels',
                '[[5,7],[3,5]]', 'positions', 'relative', 'context', '[4, 8, 0]', 'causal_conv',
                'True', '--num_epochs', '1', '--batch_size', '4', '--save', out, '--seed', '1',
                '--lr', '0.001'])
    best = os.path.join(out, 'best.h5')
    assert os.path.exists(best)
    model = core_utils.load_model(best, mode='predict', decoder=False)
    assert model.config['name'] == 'conformer'
    assert model.config['kwargs']['context'] == [4, 8, 0]
    assert model.config['kwargs']['causal_conv'] is True
    assert [s.window for s in model.stages if s.kind == 'mha'] == [(4, 8, 0)] * 2
    assert [s.pad_left for s in model.stages if s.kind == 'dwconv'] == [6, 6]
    rs = np.random.RandomState(2)
    x = rs.randn(2, 30, 16).astype(np.float32)
    want = model.predict(x, [30, 25])
    from asr_study_amd.utils import keras_config as K
    m2 = K.topology_from_config(K.model_config(model))
    m2.set_weights(model.get_weights())
    m2.decoder = None
    assert [s.window for s in m2.stages if s.kind == 'mha'] == [(4, 8, 0)] * 2
    assert np.array_equal(m2.predict(x, [30, 25]), want)
    res = predict_cli.main(['--model', best, '--dataset', fname, '--no_decoder'])
    assert all(np.isfinite(r['best']).all() for r in res)
