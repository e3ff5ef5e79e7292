"""-m gpu: the relative positional attention kernels (csrc/rel_attention.hip) and the models that
use them against the float64 oracle (tests/relattention_oracle.py).  Kernel bound: 1e-5 max-norm
relative; model bounds: DESIGN.md 7."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import relattention_oracle as RO
from tests.test_relattention_host import shift_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('out', 'lse', 'dQ', 'dK', 'dV', 'dpos', 'dbias_u', 'dbias_v')


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _run_kernels(d, N, heads, dh, lens, backward=True):
    """d: host float32 qkv (T, n_pad, ld), pos (2T - 1, ld_pos), bias_u, bias_v (D), dout
    (T, n_pad, ld_out) -> dict of host arrays.  Outputs start from the sentinel 7.0."""
    from asr_study_amd import ops
    T, n_pad, _ = d['qkv'].shape
    D = heads * dh
    q, do, pos = _dev(d['qkv']), _dev(d['dout']), _dev(d['pos'])
    bu, bv = _dev(d['bias_u']), _dev(d['bias_v'])
    ld = None if lens is None else torch.tensor(np.asarray(lens, np.int32), device='cuda:0')
    out, out2 = torch.full_like(do, 7.0), torch.full_like(do, 7.0)
    lse = torch.full((ops.attn_lse_len(T, n_pad, heads),), 7.0, device='cuda:0')
    ops.relattn_fwd(q, pos, bu, bv, out, N, heads, dh, lens=ld, lse=lse)
    ops.relattn_fwd(q, pos, bu, bv, out2, N, heads, dh, lens=ld)    # inference: nothing kept
    res = dict(out=out, lse=lse.view(T, n_pad, heads), out2=out2)
    if backward:
        res.update(dqkv=torch.full_like(q, 7.0), dpos=torch.full_like(pos, 7.0),
                   dbias_u=torch.full((D,), 7.0, device='cuda:0'),
                   dbias_v=torch.full((D,), 7.0, device='cuda:0'))
        ops.relattn_bwd(q, pos, bu, bv, out, lse, do, res['dqkv'], res['dpos'], res['dbias_u'],
                        res['dbias_v'], N, heads, dh, lens=ld)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in res.items()}


def _oracle(d, N, heads, dh, lens):
    """Sample by sample -> out, lse, dqkv, dpos, dbias_u, dbias_v over the real rows and columns,
    and the largest |score|."""
    T, D = d['qkv'].shape[0], heads * dh
    out, lse, dqkv = np.zeros((T, N, D)), np.zeros((T, N, heads)), np.zeros((T, N, 3 * D))
    dpos, dbu, dbv, smax = np.zeros((2 * T - 1, D)), np.zeros(D), np.zeros(D), 0.0
    pos = d['pos'][:, :D].astype(np.float64)
    bu, bv = d['bias_u'].astype(np.float64), d['bias_v'].astype(np.float64)
    for n in range(N):
        o, c = RO.relattn_forward(d['qkv'][:, n:n + 1, :3 * D].astype(np.float64), pos, bu, bv,
                                  heads, None if lens is None else lens[n:n + 1])
        out[:, n:n + 1], lse[:, n:n + 1] = o, c['lse']
        g = RO.relattn_backward(d['dout'][:, n:n + 1, :D].astype(np.float64), c)
        dqkv[:, n:n + 1] = g[0]
        dpos, dbu, dbv = dpos + g[1], dbu + g[2], dbv + g[3]
        smax = max(smax, float(c['smax']))
    return dict(out=out, lse=lse, dqkv=dqkv, dpos=dpos, dbias_u=dbu, dbias_v=dbv, smax=smax)


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


def _parts(r, N, D):
    return (r['out'][:, :N, :D], r['lse'][:, :N], r['dqkv'][:, :N, :D], r['dqkv'][:, :N, D:2 * D],
            r['dqkv'][:, :N, 2 * D:3 * D], r['dpos'][:, :D], r['dbias_u'], r['dbias_v'])


def _check(tag, d, N, heads, dh, lens, bound=1e-5, zero_scale=None):
    """zero_scale: the size against which the gradients through dS are measured where the
    oracle's are exactly zero (a single key: p = 1, dS = 0)."""
    D = heads * dh
    got_all = _run_kernels(d, N, heads, dh, lens)
    want_all = _oracle(d, N, heads, dh, lens)
    got, want = _parts(got_all, N, D), _parts(want_all, N, D)
    errs = [_rel(g, w) for g, w in zip(got, want)]
    if zero_scale is not None:
        for k in (2, 3, 5, 6, 7):
            assert not want[k].any()
            errs[k] = float(np.abs(got[k]).max() / zero_scale)
    print('[relattn] %s: %s (bound %.3e, largest |s| %.1f)'
          % (tag, ' '.join('%s %.2e' % kv for kv in zip(NAMES, errs)), bound, want_all['smax']))
    for a in got + (got_all['out'], got_all['dqkv'], got_all['dpos']):
        assert np.isfinite(a).all(), tag
    for name, e in zip(NAMES, errs):
        assert e < bound, (tag, name, e)
    assert np.array_equal(got_all['out'], got_all['out2']), tag     # with and without lse
    # padding rows and columns are written as exact zeros
    out, dqkv = got_all['out'], got_all['dqkv']
    assert not out[:, N:].any() and not out[:, :, D:].any(), tag
    assert not dqkv[:, N:].any() and not dqkv[:, :, 3 * D:].any(), tag
    assert not got_all['dpos'][:, D:].any(), tag
    if lens is not None:                                        # masked keys: dK = dV = 0
        for n in range(N):
            assert not dqkv[lens[n]:, n, D:3 * D].any(), (tag, n)
    return got_all


def test_single_frame_returns_v_exactly():
    """T = 1: p = 1, out = v bit for bit.  dS is exactly 0 in the oracle, so what comes through it
    is measured against the size of the terms that cancel, scale |dO . v| max(|k|, |q|, |pos|)."""
    rs = np.random.RandomState(0)
    d = _make(rs, 1, 3, 16, 2, 16, None)
    terms = np.abs(d['dout'][0, :3, :32].astype(np.float64) * d['qkv'][0, :3, 64:96])
    size = 0.25 * terms.reshape(3, 2, 16).sum(axis=-1).max() * \
        max(np.abs(d['qkv'][0, :3, :64]).max() + 2.0, np.abs(d['pos'][:, :32]).max())
    r = _check('T=1', d, 3, 2, 16, None, zero_scale=float(size))
    assert np.array_equal(r['out'][0, :3, :32], d['qkv'][0, :3, 64:96])


# (T, N, n_pad, heads, dh, lens): lens None = the NULL pointer
CASES = {
    'ragged-131-dh64': (131, 5, 16, 2, 64, [131, 1, 77, 64, 65]),
    'null-lens-dh16': (65, 3, 16, 4, 16, None),
    'one-head-dh32': (64, 9, 16, 1, 32, [64, 1, 33, 63, 17, 64, 2, 50, 31]),
    'long-200-dh64': (200, 4, 16, 2, 64, [200, 70, 129, 192]),
    'dh48': (70, 2, 16, 1, 48, [70, 41]),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_kernel_parity(case):
    T, N, n_pad, heads, dh, lens = CASES[case]
    rs = np.random.RandomState(T + dh)
    lens = None if lens is None else np.asarray(lens)
    d = _make(rs, T, N, n_pad, heads, dh, lens)
    _check(case, d, N, heads, dh, lens)
    if lens is None:                                            # lens = T is lens = NULL
        a = _run_kernels(d, N, heads, dh, None)
        b = _run_kernels(d, N, heads, dh, np.full(N, T))
        assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('side', ['bq', 'bk'])
@pytest.mark.parametrize('edge', ['B-1', 'B', 'B+1', '2B+3'])
def test_tile_edges(side, edge):
    """T around the query and key tile lengths the library reports (63, 64, 65, 131), ragged
    lengths with one exactly on a tile edge and one one past it wherever T has room."""
    from asr_study_amd import ops
    heads, dh = 2, 32
    B = ops.relattn_plan(100, 16, heads, dh)[side]
    assert B == 64 and ops.relattn_plan(100, 16, heads, dh, backward=True)[side] == B
    T = {'B-1': B - 1, 'B': B, 'B+1': B + 1, '2B+3': 2 * B + 3}[edge]
    lens = np.array(sorted(set(v for v in (T, B, B + 1, 2 * B, 2 * B + 1, 1, T // 2 + 1, B - 1)
                               if 1 <= v <= T)))
    N = len(lens)
    rs = np.random.RandomState(T)
    d = _make(rs, T, N, 16, heads, dh, lens)
    _check('%s %s T=%d lens=%s' % (side, edge, T, lens.tolist()), d, N, heads, dh, lens)


def test_unreached_dpos_rows_are_exact_zeros():
    """T = 131, every length <= 70: no valid pair has t - u < -69, those rows of dpos are 0."""
    rs = np.random.RandomState(5)
    T, N, heads, dh = 131, 3, 2, 16
    lens = np.array([70, 64, 9])
    d = _make(rs, T, N, 16, heads, dh, lens)
    r = _check('short keys', d, N, heads, dh, lens)
    rows = np.arange(-(T - 1), T)
    assert not r['dpos'][rows < -69].any()
    assert r['dpos'][rows == -69, :heads * dh].any()


@pytest.mark.parametrize('r_star', [3, -5, 63, 64, 65, -63, -64, -65])
def test_shift_on_the_device(r_star):
    """The host test's shift case at T = 150: out_t = v_{t - r*} wherever 0 <= t - r* < len, on
    each side of the band-tile borders (|r*| = 63, 64, 65).  Within the kernel bound of max|v|
    (the other keys' e^-40 each is far below it)."""
    T, N, heads, dh = 150, 2, 2, 16
    lens = np.array([150, 100])
    qkv, pos, bu, bv = shift_case(T, N, heads, dh, r_star, lens, seed=r_star % 7)
    D = heads * dh
    d = dict(qkv=np.zeros((T, 16, 3 * D), np.float32), pos=pos.astype(np.float32),
             bias_u=bu.astype(np.float32), bias_v=bv.astype(np.float32),
             dout=np.zeros((T, 16, D), np.float32))
    d['qkv'][:, :N] = qkv
    out = _run_kernels(d, N, heads, dh, lens, backward=False)['out']
    v = d['qkv'][:, :N, 2 * D:]
    seen = 0
    for n in range(N):
        t = np.arange(max(r_star, 0), min(T, lens[n] + r_star))
        assert len(t) > 0
        err = np.abs(out[t, n, :D].astype(np.float64) - v[t - r_star, n]).max()
        assert err <= 1e-5 * np.abs(v).max(), (r_star, n, err)
        seen += len(t)
    print('[relattn] shift r* = %d: %d frames' % (r_star, seen))


def test_reduces_to_plain_attention_on_the_device():
    """pos = 0 and zero position biases: asr_attn_fwd / asr_attn_bwd on the same qkv, within the
    kernel bound (bit-equality is not required)."""
    from asr_study_amd import ops
    rs = np.random.RandomState(9)
    T, N, n_pad, heads, dh = 131, 4, 16, 2, 32
    D = heads * dh
    lens = np.array([131, 64, 65, 3])
    d = _make(rs, T, N, n_pad, heads, dh, lens, pad_cols=0)
    d['pos'][:] = 0
    d['bias_u'][:] = 0
    d['bias_v'][:] = 0
    r = _run_kernels(d, N, heads, dh, lens)
    q, do = _dev(d['qkv']), _dev(d['dout'])
    ld = torch.tensor(lens.astype(np.int32), device='cuda:0')
    out = torch.full_like(do, 7.0)
    lse = torch.full((ops.attn_lse_len(T, n_pad, heads),), 7.0, device='cuda:0')
    dqkv = torch.full_like(q, 7.0)
    ops.attn_fwd(q, out, N, heads, dh, lens=ld, lse=lse)
    ops.attn_bwd(q, out, lse, do, dqkv, N, heads, dh, lens=ld)
    torch.cuda.synchronize()
    assert _rel(r['out'], out.cpu().numpy()) < 1e-5
    assert _rel(r['lse'][:, :N], lse.view(T, n_pad, heads)[:, :N].cpu().numpy()) < 1e-5
    for k in range(3):
        assert _rel(r['dqkv'][..., k * D:(k + 1) * D],
                    dqkv[..., k * D:(k + 1) * D].cpu().numpy()) < 1e-5, k


def test_large_scores():
    """tests/test_gpu_attention.py::test_large_scores' data (a query whose best key wins by far, a
    sample of identical keys) with K and pos rescaled so that the content term and the relative
    term each reach about 150: the relative term carries half of the score.  A relative product
    error of 2^-22 on a term of size s is an absolute score error of s 2^-22; the two terms' errors
    add, and the sum is the relative error of p, which enters through the row maximum and the
    entry: bound 1e-5 + 8 (smax_content + smax_position) 2^-22."""
    rs = np.random.RandomState(11)
    T, N, n_pad, heads, dh = 70, 2, 16, 1, 16
    lens = np.array([70, 41])
    d = _make(rs, T, N, n_pad, heads, dh, lens)
    D = dh
    qkv = d['qkv']
    qkv[:lens[1], 1, D:2 * D] = qkv[0, 1, D:2 * D]              # sample 1: identical keys
    qkv[0, 0, :D] = 3.0 * qkv[5, 0, D:2 * D]                    # sample 0, query 0: key 5 wins

    def terms():
        q = qkv[:, :N, :D].astype(np.float64)
        k = qkv[:, :N, D:2 * D].astype(np.float64)
        c = np.einsum('tnd,und->ntu', q + d['bias_u'], k) / 4.0
        p = np.einsum('tnd,rd->ntr', q + d['bias_v'], d['pos'][:, :D].astype(np.float64)) / 4.0
        mask = np.arange(T)[None, :] < lens[:, None]
        return (np.abs(c) * mask[:, None, :]).max(), np.abs(p).max()
    sc, sp = terms()
    qkv[:, :N, D:2 * D] *= np.float32(150.0 / sc)
    d['pos'][:, :D] *= np.float32(150.0 / sp)
    sc, sp = terms()
    assert 140 < sc < 160 and 140 < sp < 160
    bound = 1e-5 + 8 * (sc + sp) * 2.0 ** -22
    print('[relattn] large scores: content %.2f position %.2f bound %.3e' % (sc, sp, bound))
    _check('large-scores', d, N, heads, dh, lens, bound=bound)


def test_kernels_are_deterministic():
    rs = np.random.RandomState(1)
    T, N, n_pad, heads, dh = 200, 12, 16, 4, 64
    lens = rs.randint(70, T + 1, size=N)
    d = _make(rs, T, N, n_pad, heads, dh, lens, pad_cols=0)
    a = _run_kernels(d, N, heads, dh, lens)
    b = _run_kernels(d, N, heads, dh, lens)
    for k in a:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k


def test_relpos_table_is_cached():
    from asr_study_amd import ops
    pe = ops.relpos_get(9, 32, 'cuda:0')
    assert pe is ops.relpos_get(9, 32, 'cuda:0') and tuple(pe.shape) == (17, 32)
    assert np.array_equal(pe.cpu().numpy(), RO.relpos(9, 32).astype(np.float32))


# ---------------------------------------------------------------- models
def _randomise_ln(model, rs):
    """gain / bias away from their 1 / 0 start."""
    w = model.get_weights()
    k = 0
    for s in model.stages:
        if s.kind == 'ln':
            n = w[k].size
            w[k] = (rs.rand(n) + 0.5).astype(np.float32)
            w[k + 1] = (rs.randn(n) * 0.2).astype(np.float32)
        k += len(s.tensors or ())
    model.set_weights(w)


def _parity(model, x, lens, labels, tag):
    """The scheme and bounds of tests/test_gpu_conformer.py: logits, per-sample CTC,
    every gradient, predict, three Adam steps."""
    N = x.shape[0]
    slab = model.to_slab(x)
    stages = RO.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    ctc, logits, sl = model.loss_and_grads(slab, labels, lens, training=True)
    torch.cuda.synchronize()
    want = RO.loss_and_grads(stages, x64, labels, lens)
    e = _rel(logits[:, :N].cpu().numpy(), want['logits'])
    print('[relattn] %s logits rel err %.3e' % (tag, e))
    assert e < 1e-4, tag
    assert _rel(ctc.cpu().numpy()[:N], want['ctc']) < 1e-4, tag
    got = model.get_gradients()
    assert len(got) == len(want['grads'])
    worst = 0.0
    for k, (g, gw) in enumerate(zip(got, want['grads'])):
        err = np.abs(g - gw).max()
        worst = max(worst, err / (1e-4 * np.abs(gw).max() + 1e-7))
        assert err < 1e-4 * np.abs(gw).max() + 1e-7, (tag, k, g.shape, err, np.abs(gw).max())
    print('[relattn] %s %d gradients, worst at %.3f of its bound' % (tag, len(got), worst))
    model.decoder = None
    want_i, _ = RO.model_forward(stages, x64, lens, training=False)
    got_i = model.predict(x, lens)
    model.decoder = {'is_greedy': True}
    assert _rel(got_i.transpose(1, 0, 2), want_i) < 1e-4, tag
    from oracle import optim as OO
    opt = OO.Adam(lr=1e-3, clipnorm=400.0)
    for _ in range(3):
        m = model.train_on_batch([('slab', slab), labels, lens])
        out = RO.train_step(stages, x64, labels, lens, opt)
    assert abs(m[1] - float(np.mean(out['ctc']))) < 1e-4 * abs(m[1])
    for k, (a, b) in enumerate(zip(RO.weights(stages), model.get_weights())):
        err = np.abs(b - a).max()
        assert err < 5e-5 * max(1.0, np.abs(a).max()), (tag, 'w', k, err)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def _blocks(seed=2):
    """Dense(32) -> two pre-LN relative blocks (2 heads of 16, d_ff 48) -> LN -> Dense(8)."""
    from asr_study_amd.core import layers as L, optimizers
    from asr_study_amd.core.models import ctc_model
    x_in = L.Input(name='inputs', shape=(None, 10))
    o = L.TimeDistributed(L.Dense(32))(x_in)
    for _ in range(2):
        y = L.RelativeMultiHeadAttention(2)(L.LayerNormalization()(o))
        o = L.merge([L.Dropout(0.0)(y), o], mode='sum')
        y = L.TimeDistributed(L.Dense(48))(L.LayerNormalization()(o))
        y = L.TimeDistributed(L.Dense(32))(L.Activation('relu')(y))
        o = L.merge([L.Dropout(0.0)(y), o], mode='sum')
    o = L.TimeDistributed(L.Dense(8))(L.LayerNormalization()(o))
    model = ctc_model(x_in, o, seed=seed)
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    assert [getattr(s, 'relative', False) for s in model.stages].count(True) == 2
    return model


def _small_conformer(seed=1, F=10):
    from asr_study_amd.core import models, optimizers
    m = models.conformer(positions='relative', num_layers=2, d_model=32, num_heads=2, conv=False,
                         num_features=F, num_classes=8, d_ff=48, kernel_size=7, dropout=0,
                         seed=seed)
    m.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    assert 'posenc' not in [s.kind for s in m.stages]
    return m


def _batch(rs, N, T, F, C, lens, label_lens):
    x = rs.randn(N, T, F).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    return x, [rs.randint(0, C - 1, size=k).tolist() for k in label_lens]


def test_relative_blocks_vs_oracle():
    rs = np.random.RandomState(4)
    model = _blocks()
    _randomise_ln(model, rs)
    lens = np.array([21, 15, 21, 8, 12, 21])
    x, labels = _batch(rs, 6, 21, 10, 8, lens, (3, 2, 4, 1, 2, 3))
    _parity(model, x, lens, labels, 'blocks')


def test_relative_conformer_vs_oracle():
    rs = np.random.RandomState(3)
    model = _small_conformer()
    _randomise_ln(model, rs)
    lens = np.array([25, 14, 25, 9, 20])
    x, labels = _batch(rs, 5, 25, 10, 8, lens, (3, 2, 4, 1, 2))
    _parity(model, x, lens, labels, 'conformer')


def test_time_padding_independence():
    """The valid-frame logits of a batch padded to T = 40 and to T = 56 agree within 1e-6
    relative: the relative index of a pair of valid frames does not depend on T."""
    rs = np.random.RandomState(8)
    model = _blocks()
    _randomise_ln(model, rs)
    model.decoder = None
    lens = np.array([40, 17, 33, 8])
    x = np.zeros((4, 56, 10), np.float32)
    for n in range(4):
        x[n, :lens[n]] = rs.randn(lens[n], 10)
    short = model.predict(x[:, :40], lens)
    long_ = model.predict(x, lens)
    for n in range(4):
        e = _rel(long_[n, :lens[n]], short[n, :lens[n]])
        print('[relattn] utterance %d (len %d): T 40 vs T 56 rel %.2e' % (n, lens[n], e))
        assert e < 1e-6, (n, e)


@pytest.mark.parametrize('build', ['blocks', 'conformer-layer'])
def test_batch_independence(build):
    """The same 3 utterances alone and inside a batch of 6, the same T and n_pad: bit-equal."""
    rs = np.random.RandomState(6)
    if build == 'blocks':
        model = _blocks()
    else:
        from asr_study_amd.core import models
        model = models.conformer(positions='relative', num_layers=2, d_model=32, num_heads=2,
                                 conv=False, num_features=10, num_classes=8, d_ff=48,
                                 kernel_size=7, conv_norm='layer', dropout=0, seed=1)
    _randomise_ln(model, rs)
    model.decoder = None
    T = 40
    lens6 = np.array([40, 33, 25, 40, 12, 29])
    x6 = rs.randn(6, T, 10).astype(np.float32)
    for n in range(6):
        x6[n, lens6[n]:] = 0
    pick = [4, 0, 2]
    alone = model.predict(x6[pick], lens6[pick])
    among = model.predict(x6, lens6)
    assert np.isfinite(alone).all() and np.abs(alone).max() > 0
    assert np.array_equal(alone, among[pick])


def learn_setup(device=None):
    """The model, batch and labels of the learning test (also run by the float64 oracle on the
    host to find the step at which it reaches LER 0)."""
    from asr_study_amd.core import models, optimizers
    kw = {} if device is None else {'device': device}
    model = models.conformer(positions='relative', conv=False, num_features=16, num_classes=12,
                             d_model=32, num_heads=2, num_layers=2, d_ff=64, kernel_size=7,
                             conv_norm='layer', dropout=0, seed=3, **kw)
    model.compile(optimizer=optimizers.Adam(lr=3e-3, clipnorm=400))
    rs = np.random.RandomState(0)
    x = rs.randn(4, 60, 16).astype(np.float32)
    lab = [list(rs.randint(1, 11, size=5)) for _ in range(4)]
    return model, x, lab


# the oracle's greedy LER is 0 first at its step 116: `python tools/relattn_learn_oracle.py`
# (host, a few seconds) runs RO.train_step on learn_setup() and prints that step
ORACLE_LER0_STEP = 116


def test_relative_conformer_learns_a_fixed_batch():
    """Overfits 4 utterances (T = 60, 5 labels each) to greedy LER 0.  The float64 oracle's
    train_step, run on the host from the same initial weights, batch and Adam(lr=3e-3,
    clipnorm=400), reaches LER 0 at step 116 (counted from 1, ORACLE_LER0_STEP); the test allows
    twice that, 232."""
    model, x, lab = learn_setup()
    slab = model.to_slab(x)
    cap = 2 * ORACLE_LER0_STEP
    ler = step = m = None
    for step in range(1, cap + 1):
        m = model.train_on_batch([('slab', slab), lab, np.full(4, 60)])
        ler = m[3]
        if ler == 0.0:
            break
    print('[learn] relative conformer greedy LER 0 at step %s (oracle %d, cap %d)'
          % (step, ORACLE_LER0_STEP, cap))
    assert ler == 0.0, (step, m)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def test_cli_roundtrip_relative_conformer(tmp_path):
    sys.path.insert(0, ROOT)
    import train
    import eval as eval_cli
    import predict as predict_cli
    import align as align_cli
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
                '[[5,7],[3,5]]', 'positions', 'relative', '--num_epochs', '1', '--batch_size',
                '4', '--save', out, '--seed', '1', '--lr', '0.001'])
    best = os.path.join(out, 'best.h5')
    assert os.path.exists(best)
    model = core_utils.load_model(best, mode='predict', decoder=False)
    assert [getattr(s, 'relative', False) for s in model.stages].count(True) == 2
    assert 'posenc' not in [s.kind for s in model.stages]
    assert model.config['name'] == 'conformer'
    assert model.config['kwargs']['positions'] == 'relative'
    saved = []
    with h5lite.File(best, 'r') as f:
        g = f['model_weights']
        names = g.attrs.get_strings('layer_names')
        assert [n for n in names if 'multiheadattention' in n] == \
            ['relativemultiheadattention_1', 'relativemultiheadattention_2']
        for lname in names:
            wn = g[lname].attrs.get_strings('weight_names')
            if lname.startswith('relativemultiheadattention'):
                assert wn == ['%s_%s:0' % (lname, k) for k in
                              ('W_qkv', 'b_qkv', 'W_pos', 'pos_bias_u', 'pos_bias_v', 'W_o',
                               'b_o')]
            saved += [g[lname][w].read_array() for w in wn]
    w = model.get_weights()
    assert len(saved) == len(w) and all(np.array_equal(a, b) for a, b in zip(saved, w))
    for mode in ('train', 'eval'):
        assert core_utils.load_model(best, mode=mode).n_params == model.n_params
    rs = np.random.RandomState(2)
    x = rs.randn(2, 30, 16).astype(np.float32)
    want = model.predict(x, [30, 25])
    from asr_study_amd.utils import keras_config as K
    m2 = K.topology_from_config(K.model_config(model))
    m2.set_weights(model.get_weights())
    m2.decoder = None
    assert np.array_equal(m2.predict(x, [30, 25]), want)
    m = eval_cli.main(['--model', best, '--dataset', fname, '--beam_width', '10'])
    assert len(m) == 4 and np.isfinite(m[1]) and m[3] >= 0
    res = predict_cli.main(['--model', best, '--dataset', fname, '--no_decoder'])
    assert all(np.isfinite(r['best']).all() for r in res)
    res = align_cli.main(['--model', best, '--dataset', fname, '--save',
                          str(tmp_path / 'align.jsonl')])
    assert os.path.exists(str(tmp_path / 'align.jsonl'))
    assert len(res) > 0 and all(np.isfinite(r['score']) for r in res)
