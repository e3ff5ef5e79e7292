"""-m gpu: the depthwise convolution, GLU and Swish kernels (csrc/dwconv.hip) and the conformer
models against the float64 oracle (tests/conformer_oracle.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import conformer_oracle as CO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('y', 'dx', 'dw', 'db')
BOUND = 1e-5        # max-norm relative: the project's bound for its exact-fp32 kernels


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _make(rs, T, N, n_pad, C, ld, k, lens):
    """Data at scale 1 in the real rows and columns; finite junk at 3x the scale in the pad sample
    rows, the pad columns and the frames at or past an utterance's length (x only: dy there is
    real, those frames are outputs)."""
    x = (rs.randn(T, n_pad, ld) * 3.0).astype(np.float32)
    x[:, :N, :C] = rs.randn(T, N, C).astype(np.float32)
    if lens is not None:
        for n in range(N):
            x[lens[n]:, n] = (rs.randn(T - lens[n], ld) * 3.0).astype(np.float32)
    dy = (rs.randn(T, n_pad, ld) * 3.0).astype(np.float32)
    dy[:, :N, :C] = rs.randn(T, N, C).astype(np.float32)
    w = (rs.randn(k, C) * 0.5).astype(np.float32)
    b = (rs.randn(C) * 0.3).astype(np.float32)
    return x, w, b, dy


def _run_kernels(x, w, b, dy, N, C, k, lens, want_dx=True):
    """-> y, dx, dw, db (host arrays).  Outputs start from the sentinel 7.0: what is not written
    shows."""
    from asr_study_amd import ops
    xd, wd, bd, dyd = _dev(x), _dev(w), _dev(b), _dev(dy)
    ld = None if lens is None else torch.tensor(np.asarray(lens, np.int32), device='cuda:0')
    y, dx = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
    dw, db = torch.full_like(wd, 7.0), torch.full_like(bd, 7.0)
    ops.dwconv1d_fwd(xd, wd, bd, y, N, k, lens=ld, C_=C)
    ops.dwconv1d_bwd(xd, wd, dyd, dx if want_dx else None, dw, db, N, k, lens=ld, C_=C)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (y, dx, dw, db)]


def _oracle(x, w, b, dy, N, C, lens):
    y, c = CO.dwconv_forward(x[:, :N, :C].astype(np.float64), w.astype(np.float64),
                             b.astype(np.float64), lens)
    d = dy[:, :N, :C].astype(np.float64)
    return (y,) + CO.dwconv_backward(d, c) + (CO.dwconv_abs_terms(d, c),)


def _check(tag, x, w, b, dy, N, C, k, lens, against_terms=False):
    """against_terms: dw and db are measured against the largest sum of |terms| (a long fp32 sum
    has no useful worst-case bound relative to its own value)."""
    T = x.shape[0]
    got = _run_kernels(x, w, b, dy, N, C, k, lens)
    y, dx, dw, db = got
    wy, wdx, wdw, wdb, (aw, ab) = _oracle(x, w, b, dy, N, C, lens)
    errs = [_rel(y[:, :N, :C], wy), _rel(dx[:, :N, :C], wdx), _rel(dw, wdw), _rel(db, wdb)]
    if against_terms:
        errs[2] = float(np.abs(dw - wdw).max() / aw.max())
        errs[3] = float(np.abs(db - wdb).max() / ab.max())
    print('[conformer] %s: %s (bound %.1e%s)'
          % (tag, ' '.join('%s %.2e' % kv for kv in zip(NAMES, errs)), BOUND,
             ', dw db against sum |terms|' if against_terms else ''))
    for a in got:
        assert np.isfinite(a).all(), tag
    for name, e in zip(NAMES, errs):
        assert e < BOUND, (tag, name, e)
    # padding rows and columns are written as exact zeros, in every frame
    assert not y[:, N:].any() and not y[:, :, C:].any(), tag
    assert not dx[:, N:].any() and not dx[:, :, C:].any(), tag
    if lens is not None:                                # dx = 0 at every frame >= len
        for n in range(N):
            assert not dx[lens[n]:, n].any(), (tag, n)
    # without an input gradient: the same dw, db bit for bit
    _, dx2, dw2, db2 = _run_kernels(x, w, b, dy, N, C, k, lens, want_dx=False)
    assert np.array_equal(dw2, dw) and np.array_equal(db2, db) and (dx2 == 7.0).all(), tag
    return got


def _masked(x, N, C, lens):
    xm = x[:, :N, :C].copy()
    for n in range(N):
        xm[lens[n]:, n] = 0
    return xm


def test_identity_filter_is_exact():
    """k = 1, w = 1, b = 0: y == the masked input, bit for bit."""
    rs = np.random.RandomState(0)
    T, N, n_pad, C, ld = 70, 5, 16, 12, 16
    lens = np.array([70, 1, 33, 64, 65])
    x, w, b, dy = _make(rs, T, N, n_pad, C, ld, 1, lens)
    w[:], b[:] = 1.0, 0.0
    y, dx, dw, db = _check('k=1', x, w, b, dy, N, C, 1, lens)
    assert np.array_equal(y[:, :N, :C], _masked(x, N, C, lens))
    assert np.array_equal(dx[:, :N, :C], _masked(dy, N, C, lens))


@pytest.mark.parametrize('j', [0, 3, 6])
def test_one_hot_filter_shifts_exactly(j):
    """w[j] = 1 alone, k = 7 (p = 3): y[t] == xm[t + j - p] bit for bit: a flipped kernel or a halo
    off by one shows here."""
    rs = np.random.RandomState(j)
    T, N, n_pad, C, ld, k, p = 131, 4, 16, 8, 8, 7, 3
    lens = np.array([131, 2, 64, 67])
    x, w, b, dy = _make(rs, T, N, n_pad, C, ld, k, lens)
    w[:], b[:] = 0.0, 0.0
    w[j] = 1.0
    y, dx, dw, db = _check('one-hot j=%d' % j, x, w, b, dy, N, C, k, lens)
    xm = np.zeros((T + 2 * p, N, C), np.float32)
    xm[p:p + T] = _masked(x, N, C, lens)
    assert np.array_equal(y[:, :N, :C], xm[j:j + T])
    dyp = np.zeros((T + 2 * p, N, C), np.float32)
    dyp[p:p + T] = dy[:, :N, :C]
    want = dyp[2 * p - j:2 * p - j + T].copy()          # dx[u] = dy[u - j + p] below len
    for n in range(N):
        want[lens[n]:, n] = 0
    assert np.array_equal(dx[:, :N, :C], want)


# (T, N, n_pad, C, ld, k, lens): lens None = the NULL pointer
CASES = {
    'window-wider-than-T': (1, 1, 16, 4, 4, 31, [1]),
    'tiny-ragged': (5, 3, 16, 4, 8, 31, [5, 1, 3]),
    'pad-columns': (40, 5, 16, 36, 40, 7, [40, 1, 17, 33, 8]),
    'null-lens': (130, 3, 16, 64, 64, 3, None),
    'k31-256': (67, 20, 32, 256, 256, 31, 'ragged'),
}


def _lens(rs, kind, T, N, lo=1):
    if kind is None or isinstance(kind, list):
        return None if kind is None else np.asarray(kind)
    lens = rs.randint(lo, T + 1, size=N)
    lens[0], lens[-1] = T, lo
    return lens


@pytest.mark.parametrize('case', sorted(CASES))
def test_kernel_parity(case):
    T, N, n_pad, C, ld, k, kind = CASES[case]
    assert T * N <= 2100                # a single missing term shows against the bound
    rs = np.random.RandomState(T + k)
    lens = _lens(rs, kind, T, N)
    x, w, b, dy = _make(rs, T, N, n_pad, C, ld, k, lens)
    _check(case, x, w, b, dy, N, C, k, lens)
    if case == 'null-lens':                                     # lens = T is lens = NULL
        a = _run_kernels(x, w, b, dy, N, C, k, None)
        c = _run_kernels(x, w, b, dy, N, C, k, np.full(N, T))
        assert all(np.array_equal(u, v) for u, v in zip(a, c))


@pytest.mark.parametrize('edge', ['Tt-1', 'Tt', 'Tt+1', '2Tt+3'])
def test_tile_edges(edge):
    """T around the time tile the library reports (asr_dwconv1d_plan); for every tile boundary B
    inside T one length on each side of it, one on it and one within p frames on each side."""
    from asr_study_amd import ops
    C, ld, k, p = 8, 12, 7, 3
    Tt = ops.dwconv1d_plan(100, 16, C, k, ld=ld)['tile']
    assert ops.dwconv1d_plan(100, 16, C, k, ld=ld, backward=True)['tile'] == Tt
    T = {'Tt-1': Tt - 1, 'Tt': Tt, 'Tt+1': Tt + 1, '2Tt+3': 2 * Tt + 3}[edge]
    want = [T, 1]
    for B in range(Tt, T + 1, Tt):
        want += [B - 1, B, B + 1, B - p + 1, B + p - 1]
    lens = np.array(sorted(set(v for v in want if 1 <= v <= T)))
    N = len(lens)
    assert N <= 16 and T * N <= 2100
    if T > Tt:
        assert Tt - 1 in lens and Tt + 1 in lens
    rs = np.random.RandomState(T)
    x, w, b, dy = _make(rs, T, N, 16, C, ld, k, lens)
    _check('%s T=%d lens=%s' % (edge, T, lens.tolist()), x, w, b, dy, N, C, k, lens)


def _cfg3(seed=1):
    rs = np.random.RandomState(seed)
    T, N, C, k = 500, 64, 256, 31
    lens = rs.randint(200, T + 1, size=N)
    lens[0], lens[-1] = T, 200
    return _make(rs, T, N, 64, C, C, k, lens) + (N, C, k, lens)


def test_cfg3_slab_parity():
    x, w, b, dy, N, C, k, lens = _cfg3()
    _check('cfg3-slab', x, w, b, dy, N, C, k, lens, against_terms=True)


def test_kernels_are_deterministic():
    x, w, b, dy, N, C, k, lens = _cfg3(2)
    a = _run_kernels(x, w, b, dy, N, C, k, lens)
    c = _run_kernels(x, w, b, dy, N, C, k, lens)
    for u, v in zip(a, c):
        assert np.isfinite(u).all() and np.array_equal(u, v)


SPECIAL = np.array([100., -100., 20., -20., 0., -0., 88., -88., 1e-20, -1e-20, 5., -5.], np.float32)


@pytest.mark.parametrize('rows,C,ld_in,ld_out', [(1, 4, 8, 4), (37, 12, 28, 16),
                                                 (1030, 32, 64, 32)])
def test_glu_vs_oracle(rows, C, ld_in, ld_out):
    from asr_study_amd import ops
    rs = np.random.RandomState(rows)
    x = (rs.randn(rows, ld_in) * 3.0).astype(np.float32)
    x[-1, :2 * C] = np.resize(SPECIAL, 2 * C)
    x[0, C:2 * C] = np.resize(SPECIAL, C)
    dy = (rs.randn(rows, ld_out) * 3.0).astype(np.float32)
    dy[:, :C] = rs.randn(rows, C)
    y, dx = torch.full((rows, ld_out), 7.0, device='cuda:0'), \
        torch.full((rows, ld_in), 7.0, device='cuda:0')
    ops.glu_fwd(_dev(x), y, C_=C)
    ops.glu_bwd(_dev(x), _dev(dy), dx, C_=C)
    y, dx = y.cpu().numpy(), dx.cpu().numpy()
    x64 = x[:, :2 * C].astype(np.float64)
    ey = _rel(y[:, :C], CO.glu_forward(x64)[0])
    edx = _rel(dx[:, :2 * C], CO.glu_backward(dy[:, :C].astype(np.float64), x64))
    print('[conformer] glu rows %d C %d ld %d/%d: y %.2e dx %.2e' % (rows, C, ld_in, ld_out, ey,
                                                                    edx))
    assert np.isfinite(y).all() and np.isfinite(dx).all()
    assert ey < BOUND and edx < BOUND
    assert not y[:, C:].any() and not dx[:, 2 * C:].any()


@pytest.mark.parametrize('n', [1, 7, 1024, 4 * 256 * 3 + 5, 300001])
def test_swish_vs_oracle(n):
    from asr_study_amd import ops
    rs = np.random.RandomState(n)
    x = (rs.randn(n) * 4.0).astype(np.float32)
    x[:min(n, SPECIAL.size)] = SPECIAL[:n]
    x[-min(n, SPECIAL.size):] = SPECIAL[:n][::-1]
    dy = rs.randn(n).astype(np.float32)
    y, dx = torch.full((n,), 7.0, device='cuda:0'), torch.full((n,), 7.0, device='cuda:0')
    ops.swish_fwd(_dev(x), y)
    ops.swish_bwd(_dev(x), _dev(dy), dx)
    y, dx = y.cpu().numpy(), dx.cpu().numpy()
    x64 = x.astype(np.float64)
    ey, edx = _rel(y, CO.swish(x64)), _rel(dx, CO.swish_backward(dy.astype(np.float64), x64))
    print('[conformer] swish n %d: y %.2e dx %.2e' % (n, ey, edx))
    assert np.isfinite(y).all() and np.isfinite(dx).all()
    assert ey < BOUND and edx < BOUND
    # element by element where the values are small (a max-norm hides them behind 100)
    small = np.abs(x64) <= 20
    assert np.abs(y - CO.swish(x64))[small].max(initial=0.0) <= 1e-5 * 20


# ---------------------------------------------------------------- models
def _randomise(model, rs):
    """LN gain / bias, BN gamma / beta and the depthwise bias away from their start values."""
    w = model.get_weights()
    k = 0
    for s in model.stages:
        if s.kind in ('ln', 'bn'):
            n = w[k].size
            w[k] = (rs.rand(n) + 0.5).astype(np.float32)
            w[k + 1] = (rs.randn(n) * 0.2).astype(np.float32)
        elif s.kind == 'dwconv':
            w[k + 1] = (rs.randn(w[k + 1].size) * 0.2).astype(np.float32)
        k += len(s.tensors)
    model.set_weights(w)


def _parity(model, x, lens, labels, tag):
    """The scheme and bounds of tests/test_gpu_attention.py: logits, per-sample
    CTC, every gradient, predict, three Adam steps."""
    N = x.shape[0]
    slab = model.to_slab(x)
    stages = CO.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    ctc, logits, sl = model.loss_and_grads(slab, labels, lens, training=True)
    torch.cuda.synchronize()
    want = CO.loss_and_grads(stages, x64, labels, lens)
    e = _rel(logits[:, :N].cpu().numpy(), want['logits'])
    print('[conformer] %s logits rel err %.3e' % (tag, e))
    assert e < 1e-4, tag
    assert _rel(ctc.cpu().numpy()[:N], want['ctc']) < 1e-4, tag
    got = model.get_gradients()
    assert len(got) == len(want['grads'])
    worst = 0.0
    for k, (g, gw) in enumerate(zip(got, want['grads'])):
        err = np.abs(g - gw).max()
        worst = max(worst, err / (1e-4 * np.abs(gw).max() + 1e-7))
        assert err < 1e-4 * np.abs(gw).max() + 1e-7, (tag, k, g.shape, err, np.abs(gw).max())
    print('[conformer] %s %d gradients, worst at %.3f of its bound' % (tag, len(got), worst))
    model.decoder = None
    want_i, _ = CO.model_forward(stages, x64, lens, training=False)
    got_i = model.predict(x, lens)
    model.decoder = {'is_greedy': True}
    assert _rel(got_i.transpose(1, 0, 2), want_i) < 1e-4, tag
    from oracle import optim as OO
    opt = OO.Adam(lr=1e-3, clipnorm=400.0)
    for _ in range(3):
        m = model.train_on_batch([('slab', slab), labels, lens])
        out = CO.train_step(stages, x64, labels, lens, opt)
    assert abs(m[1] - float(np.mean(out['ctc']))) < 1e-4 * abs(m[1])
    for k, (a, b) in enumerate(zip(CO.weights(stages), model.get_weights())):
        err = np.abs(b - a).max()
        assert err < 5e-5 * max(1.0, np.abs(a).max()), (tag, 'w', k, err)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def _blocks(conv_norm, seed=2, F=10):
    """Two conformer blocks without front-end: Dense(32) -> PositionalEncoding -> the blocks
    (2 heads of 16, d_ff 48, k 7) -> Dense(8)."""
    from asr_study_amd.core import models, optimizers
    m = models.conformer(num_features=F, num_classes=8, d_model=32, num_heads=2, num_layers=2,
                         d_ff=48, kernel_size=7, conv_norm=conv_norm, dropout=0, conv=False,
                         seed=seed)
    m.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    assert [s.kind for s in m.stages].count('dwconv') == 2
    return m


def _small_conformer(conv_norm, seed=1):
    from asr_study_amd.core import models, optimizers
    m = models.conformer(num_features=16, num_classes=7, d_model=32, num_heads=2, num_layers=2,
                         d_ff=64, kernel_size=7, conv_norm=conv_norm, conv_filters=4,
                         conv_kernels=((5, 7), (3, 5)), dropout=0, weight_decay=1e-4, seed=seed)
    m.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    return m


@pytest.mark.parametrize('conv_norm', ['batch', 'layer'])
def test_conformer_blocks_vs_oracle(conv_norm):
    rs = np.random.RandomState(4)
    N, T, F, C = 6, 21, 10, 8
    model = _blocks(conv_norm)
    _randomise(model, rs)
    lens = np.array([21, 15, 21, 8, 12, 21])
    x = rs.randn(N, T, F).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    labels = [rs.randint(0, C - 1, size=k).tolist() for k in (3, 2, 4, 1, 2, 3)]
    _parity(model, x, lens, labels, 'blocks-' + conv_norm)


@pytest.mark.parametrize('conv_norm', ['batch', 'layer'])
def test_conformer_with_front_end_vs_oracle(conv_norm):
    """The length mask follows the strided lengths (ceil(len / 2) behind the front-end)."""
    rs = np.random.RandomState(3)
    N, T, F, C = 5, 37, 16, 7
    model = _small_conformer(conv_norm)
    _randomise(model, rs)
    lens = np.array([37, 20, 37, 9, 30])
    x = (rs.randn(N, T, F) * 2.0 + 1.0).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    labels = [rs.randint(0, C - 1, size=k).tolist() for k in (3, 2, 4, 1, 2)]
    _parity(model, x, lens, labels, 'conformer-conv-' + conv_norm)


@pytest.mark.parametrize('conv_norm', ['batch', 'layer'])
def test_time_padding_independence(conv_norm):
    """The logits on an utterance's valid frames do not depend on how far the batch is padded in
    time: T = 40 against T = 56, one length within p = 3 frames of 40.  (predict: BN uses its
    running moments.)  Fails without the length mask of the depthwise convolution: the frames
    40 .. 55 are not zeros behind the positional encoding."""
    rs = np.random.RandomState(8)
    model = _blocks(conv_norm)
    _randomise(model, rs)
    model.decoder = None
    lens = np.array([40, 17, 38, 8])
    x = np.zeros((4, 56, 10), np.float32)
    for n in range(4):
        x[n, :lens[n]] = rs.randn(lens[n], 10)
    short = model.predict(x[:, :40], lens)
    long_ = model.predict(x, lens)
    for n in range(4):
        e = _rel(long_[n, :lens[n]], short[n, :lens[n]])
        print('[conformer] %s utterance %d (len %d): T 40 vs T 56 rel %.2e'
              % (conv_norm, n, lens[n], e))
        assert e < 1e-6, (n, e)


@pytest.mark.parametrize('build', ['blocks', 'conformer'])
def test_batch_independence(build):
    """The same 3 utterances alone and inside a batch of 6 (predict, same T and n_pad):
    bit-equal."""
    rs = np.random.RandomState(6)
    model = _blocks('batch') if build == 'blocks' else _small_conformer('layer')
    F = model.num_features
    _randomise(model, rs)
    model.decoder = None
    T = 40
    lens6 = np.array([40, 33, 25, 40, 12, 29])
    x6 = rs.randn(6, T, F).astype(np.float32)
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
    model = models.conformer(conv=False, num_features=16, num_classes=12, d_model=32,
                             num_heads=2, num_layers=2, d_ff=64, kernel_size=7,
                             conv_norm='layer', dropout=0, seed=3, **kw)
    model.compile(optimizer=optimizers.Adam(lr=3e-3, clipnorm=400))
    rs = np.random.RandomState(0)
    x = rs.randn(4, 60, 16).astype(np.float32)
    lab = [list(rs.randint(1, 11, size=5)) for _ in range(4)]
    return model, x, lab


# the oracle's greedy LER is 0 first at its step 138: `python tools/conformer_learn_oracle.py`
# (host, a few seconds) runs CO.train_step on learn_setup() and prints that step
ORACLE_LER0_STEP = 138


def test_conformer_learns_a_fixed_batch():
    """Overfits 4 utterances (T = 60, 5 labels each) to greedy LER 0.  The float64 oracle's
    train_step, run on the host from the same initial weights, batch and Adam(lr=3e-3,
    clipnorm=400), reaches LER 0 at step 138 (counted from 1, ORACLE_LER0_STEP); the test allows
    twice that, 276 (the margin of the transformer's test for fp32-vs-float64 trajectory
    drift)."""
    model, x, lab = learn_setup()
    slab = model.to_slab(x)
    cap = 2 * ORACLE_LER0_STEP
    ler = None
    for step in range(1, cap + 1):
        m = model.train_on_batch([('slab', slab), lab, np.full(4, 60)])
        ler = m[3]
        if ler == 0.0:
            break
    print('[learn] conformer greedy LER 0 at step %d (oracle %d, cap %d)'
          % (step, ORACLE_LER0_STEP, cap))
    assert ler == 0.0, (step, m)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def test_full_size_conformer_steps():
    """conformer() defaults at the cfg3 input (64 x 10 s, log-mel-80): 5 steps give finite losses
    and weights, every depthwise W and every W_qkv moves, no fallback."""
    from asr_study_amd.core import models, optimizers
    model = models.conformer(seed=0)
    model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
    assert [(s.k, s.C) for s in model.stages if s.kind == 'dwconv'] == [(31, 256)] * 6
    rs = np.random.RandomState(5)
    x = rs.randn(64, 1000, 80).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=60)) for _ in range(64)]
    slab = model.to_slab(x)
    w0 = model.get_weights()
    for _ in range(5):
        m = model.train_on_batch([('slab', slab), lab, np.full(64, 1000)])
        assert np.all(np.isfinite(m))
    assert model.fallbacks == 0 and model.vetoed_steps == 0
    w = model.get_weights()
    assert all(np.isfinite(a).all() for a in w)
    moved = [np.abs(a - b).max() > 0 for (a, b, t) in
             zip(w, w0, (t for s in model.stages for t in s.tensors))
             if t.name == 'W_qkv' or (t.layer == 'depthwiseconvolution1d' and t.name == 'W')]
    assert len(moved) == 12 and all(moved)


def test_cli_roundtrip_conformer(tmp_path):
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
                '[[5,7],[3,5]]', '--num_epochs', '1', '--batch_size', '4', '--save', out,
                '--seed', '1', '--lr', '0.001'])
    best = os.path.join(out, 'best.h5')
    assert os.path.exists(best)
    model = core_utils.load_model(best, mode='predict', decoder=False)
    kinds = [s.kind for s in model.stages]
    assert (kinds.count('dwconv'), kinds.count('glu'), kinds.count('bn')) == (2, 2, 2)
    assert [s.scale for s in model.stages if s.kind == 'merge'] == [0.5, 1.0, 1.0, 0.5] * 2
    assert model.config['name'] == 'conformer'
    saved = []
    with h5lite.File(best, 'r') as f:
        g = f['model_weights']
        names = g.attrs.get_strings('layer_names')
        assert [n for n in names if n.startswith('depthwise')] == \
            ['depthwiseconvolution1d_1', 'depthwiseconvolution1d_2']
        for lname in names:
            wn = g[lname].attrs.get_strings('weight_names')
            if lname.startswith('depthwise'):
                assert wn == ['%s_%s:0' % (lname, k) for k in ('W', 'b')]
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
