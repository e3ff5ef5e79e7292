"""-m gpu: the self-attention kernels (csrc/attention.hip), the positional-encoding add and the
transformer models against the float64 oracle (tests/attention_oracle.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import attention_oracle as AO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('out', 'lse', 'dQ', 'dK', 'dV')


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _run_kernels(qkv, dout, N, heads, dh, lens):
    """qkv (T, n_pad, ld), dout (T, n_pad, ld_out) host float32 -> out, lse, dqkv, out without lse
    (host arrays).  Outputs start from the sentinel 7.0: what is not written shows."""
    from asr_study_amd import ops
    T, n_pad, _ = qkv.shape
    q, do = _dev(qkv), _dev(dout)
    ld = None if lens is None else torch.tensor(np.asarray(lens, np.int32), device='cuda:0')
    out, out2 = torch.full_like(do, 7.0), torch.full_like(do, 7.0)
    lse = torch.full((ops.attn_lse_len(T, n_pad, heads),), 7.0, device='cuda:0')
    ops.attn_fwd(q, out, N, heads, dh, lens=ld, lse=lse)
    ops.attn_fwd(q, out2, N, heads, dh, lens=ld)                # inference: nothing kept
    dqkv = torch.full_like(q, 7.0)
    ops.attn_bwd(q, out, lse, do, dqkv, N, heads, dh, lens=ld)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (out, lse.view(T, n_pad, heads), dqkv, out2)]


def _oracle(qkv, dout, N, heads, dh, lens):
    """Sample by sample (the (T, T) probabilities of one sample at a time) -> out, lse, dqkv over
    the real rows and columns, and the largest |score|."""
    T, D = qkv.shape[0], heads * dh
    out, lse, dqkv = np.zeros((T, N, D)), np.zeros((T, N, heads)), np.zeros((T, N, 3 * D))
    smax = 0.0
    for n in range(N):
        o, c = AO.attn_forward(qkv[:, n:n + 1, :3 * D].astype(np.float64), heads,
                               None if lens is None else lens[n:n + 1])
        out[:, n:n + 1], lse[:, n:n + 1] = o, c['lse']
        dqkv[:, n:n + 1] = AO.attn_backward(dout[:, n:n + 1, :D].astype(np.float64), c)
        smax = max(smax, float(c['smax']))
    return out, lse, dqkv, smax


def _make(rs, T, N, n_pad, heads, dh, lens, pad_cols=4):
    """Data at scale 1 in the real rows and columns; junk at 3x the scale in the pad sample rows,
    the pad columns and the masked key frames of K and V (finite, of ordinary magnitude)."""
    D = heads * dh
    qkv = (rs.randn(T, n_pad, 3 * D + pad_cols) * 3.0).astype(np.float32)
    qkv[:, :N, :3 * D] = rs.randn(T, N, 3 * D).astype(np.float32)
    if lens is not None:
        for n in range(N):
            qkv[lens[n]:, n, D:3 * D] = (rs.randn(T - lens[n], 2 * D) * 3.0).astype(np.float32)
    dout = (rs.randn(T, n_pad, D + pad_cols) * 3.0).astype(np.float32)
    dout[:, :N, :D] = rs.randn(T, N, D).astype(np.float32)
    return qkv, dout


def _check(tag, qkv, dout, N, heads, dh, lens, bound=1e-5, zero_scale=None):
    """zero_scale: the size against which dQ and dK are measured where the oracle's are exactly
    zero (a single key: p = 1, dS = 0), so that a relative error does not exist."""
    T, D = qkv.shape[0], heads * dh
    out, lse, dqkv, out2 = _run_kernels(qkv, dout, N, heads, dh, lens)
    wo, wl, wd, smax = _oracle(qkv, dout, N, heads, dh, lens)
    got = (out[:, :N, :D], lse[:, :N], dqkv[:, :N, :D], dqkv[:, :N, D:2 * D],
           dqkv[:, :N, 2 * D:3 * D])
    want = (wo, wl, wd[..., :D], wd[..., D:2 * D], wd[..., 2 * D:])
    errs = [_rel(g, w) for g, w in zip(got, want)]
    if zero_scale is not None:
        assert not want[2].any() and not want[3].any()
        errs[2:4] = [float(np.abs(got[k]).max() / zero_scale) for k in (2, 3)]
    print('[attn] %s: %s (bound %.3e, largest |s| %.1f)'
          % (tag, ' '.join('%s %.2e' % kv for kv in zip(NAMES, errs)), bound, smax))
    for a in (out, lse[:, :N], dqkv):
        assert np.isfinite(a).all(), tag
    for name, e in zip(NAMES, errs):
        assert e < bound, (tag, name, e)
    assert np.array_equal(out, out2), tag                       # with and without lse
    # padding rows and columns are written as exact zeros
    assert not out[:, N:].any() and not out[:, :, D:].any(), tag
    assert not dqkv[:, N:].any() and not dqkv[:, :, 3 * D:].any(), tag
    if lens is not None:                                        # masked keys: dK = dV = 0
        for n in range(N):
            assert not dqkv[lens[n]:, n, D:3 * D].any(), (tag, n)
    return out, lse, dqkv


def test_single_frame_returns_v_exactly():
    """T = 1: p = 1, out = v bit for bit.  dS = p (dO . v - D) is exactly 0 in the oracle, so dQ
    and dK are measured against the size of the terms that cancel, scale |dO . v| max |k|, |q|."""
    rs = np.random.RandomState(0)
    qkv, dout = _make(rs, 1, 3, 16, 2, 16, None)
    terms = np.abs(dout[0, :3, :32].astype(np.float64) * qkv[0, :3, 64:96]).reshape(3, 2, 16)
    size = 0.25 * terms.sum(axis=-1).max() * np.abs(qkv[0, :3, :64]).max()
    out, _, _ = _check('T=1', qkv, dout, 3, 2, 16, None, zero_scale=float(size))
    assert np.array_equal(out[0, :3, :32], qkv[0, :3, 64:96])


# (T, N, n_pad, heads, dh, lens): lens None = the NULL pointer
CASES = {
    'tiny-ragged': (7, 5, 16, 1, 16, [7, 1, 4, 6, 3]),
    'null-lens': (130, 3, 16, 2, 32, None),
    'four-heads-64': (257, 20, 32, 4, 64, 'ragged'),
    'one-head-128': (64, 9, 16, 1, 128, 'ragged'),
    'cfg3-slab': (500, 64, 64, 4, 64, 'ragged-200'),
}


def _lens(rs, kind, T, N):
    if kind is None or isinstance(kind, list):
        return None if kind is None else np.asarray(kind)
    lo = 200 if kind == 'ragged-200' else 1
    lens = rs.randint(lo, T + 1, size=N)
    lens[0], lens[-1] = T, lo
    return lens


@pytest.mark.parametrize('case', sorted(CASES))
def test_kernel_parity(case):
    T, N, n_pad, heads, dh, kind = CASES[case]
    rs = np.random.RandomState(T + dh)
    lens = _lens(rs, kind, T, N)
    qkv, dout = _make(rs, T, N, n_pad, heads, dh, lens)
    _check(case, qkv, dout, N, heads, dh, lens)
    if case == 'null-lens':                                     # lens = T is lens = NULL
        a = _run_kernels(qkv, dout, N, heads, dh, None)
        b = _run_kernels(qkv, dout, N, heads, dh, np.full(N, T))
        assert all(np.array_equal(u[:, :N], v[:, :N]) for u, v in zip(a, b))


@pytest.mark.parametrize('side', ['bq', 'bk'])
@pytest.mark.parametrize('edge', ['B-1', 'B', 'B+1', '2B+3'])
def test_tile_edges(side, edge):
    """T around the query and the key tile lengths the library reports (asr_attn_plan), ragged
    lengths with one exactly on a tile edge and one one past it wherever T has room."""
    from asr_study_amd import ops
    heads, dh = 2, 32
    B = ops.attn_plan(100, 16, heads, dh)[side]
    assert ops.attn_plan(100, 16, heads, dh, backward=True)[side] == B
    T = {'B-1': B - 1, 'B': B, 'B+1': B + 1, '2B+3': 2 * B + 3}[edge]
    lens = np.array(sorted(set(v for v in (T, B, B + 1, 2 * B, 2 * B + 1, 1, T // 2 + 1, B - 1)
                               if 1 <= v <= T)))
    if T > B:
        assert B in lens and B + 1 in lens
    N = len(lens)
    rs = np.random.RandomState(T)
    qkv, dout = _make(rs, T, N, 16, heads, dh, lens)
    _check('%s %s T=%d lens=%s' % (side, edge, T, lens.tolist()), qkv, dout, N, heads, dh, lens)


def test_large_scores():
    """Scores up to about 300 in size: one query row whose keys are all identical (uniform p) and
    one whose best key wins by more than 100 (p one-hot).  A relative product error of 2^-22 on
    a score of size smax is an absolute score error of smax 2^-22, which is the relative error
    of p and enters through both the row maximum and the entry: bound 1e-5 + 8 smax 2^-22."""
    rs = np.random.RandomState(11)
    T, N, n_pad, heads, dh = 70, 2, 16, 1, 16
    lens = np.array([70, 41])
    qkv, dout = _make(rs, T, N, n_pad, heads, dh, lens)
    D = dh
    qkv[:lens[1], 1, D:2 * D] = qkv[0, 1, D:2 * D]              # sample 1: identical keys
    k5 = qkv[5, 0, D:2 * D]
    qkv[0, 0, :D] = 3.0 * k5                                    # sample 0, query 0: key 5 wins
    _, c = AO.attn_forward(qkv[:, :N, :3 * D].astype(np.float64), heads, lens)
    qkv[:, :N, :D] *= np.float32(300.0 / c['smax'])
    _, c = AO.attn_forward(qkv[:, :N, :3 * D].astype(np.float64), heads, lens)
    smax = float(c['smax'])
    s0 = np.sort(np.log(np.maximum(c['p'][0, 0, 0], 1e-300)))
    assert 250 < smax < 350 and s0[-1] - s0[-2] > 100           # one-hot row
    p1 = c['p'][1, 0, 3, :lens[1]]
    assert np.allclose(p1, 1.0 / lens[1], rtol=1e-9)            # uniform row
    bound = 1e-5 + 8 * smax * 2.0 ** -22
    print('[attn] large scores: smax %.2f bound %.3e' % (smax, bound))
    _check('large-scores', qkv, dout, N, heads, dh, lens, bound=bound)


def test_kernels_are_deterministic():
    rs = np.random.RandomState(1)
    T, N, n_pad, heads, dh = 500, 64, 64, 4, 64
    lens = rs.randint(200, T + 1, size=N)
    qkv, dout = _make(rs, T, N, n_pad, heads, dh, lens, pad_cols=0)
    a = _run_kernels(qkv, dout, N, heads, dh, lens)
    b = _run_kernels(qkv, dout, N, heads, dh, lens)
    for u, v in zip(a, b):
        assert np.isfinite(u[:, :N]).all() and np.array_equal(u[:, :N], v[:, :N])


@pytest.mark.parametrize('T,N,n_pad,D,ld', [(1, 1, 16, 16, 16), (33, 5, 16, 48, 64),
                                            (1000, 64, 64, 256, 256)])
def test_posenc_add(T, N, n_pad, D, ld):
    """float32(x + pe) bit for bit on the real entries, zeros elsewhere."""
    from asr_study_amd import ops
    rs = np.random.RandomState(T)
    x = rs.randn(T, n_pad, ld).astype(np.float32)
    y = torch.full((T, n_pad, ld), 7.0, device='cuda:0')
    ops.posenc_add(_dev(x), y, N, D)
    y = y.cpu().numpy()
    pe = AO.posenc(T, D).astype(np.float32)
    assert np.array_equal(y[:, :N, :D], x[:, :N, :D] + pe[:, None, :])
    assert not y[:, N:].any() and not y[:, :, D:].any()
    assert ops.posenc_get(T, D, 'cuda:0') is ops.posenc_get(T, D, 'cuda:0')     # cached


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
        k += len(s.tensors)
    model.set_weights(w)


def _parity(model, x, lens, labels, tag):
    """The scheme and bounds of tests/test_gpu_layernorm.py: logits, per-sample CTC, every
    gradient, predict, three Adam steps."""
    N = x.shape[0]
    slab = model.to_slab(x)
    stages = AO.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    ctc, logits, sl = model.loss_and_grads(slab, labels, lens, training=True)
    torch.cuda.synchronize()
    want = AO.loss_and_grads(stages, x64, labels, lens)
    e = _rel(logits[:, :N].cpu().numpy(), want['logits'])
    print('[attn] %s logits rel err %.3e' % (tag, e))
    assert e < 1e-4, tag
    assert _rel(ctc.cpu().numpy()[:N], want['ctc']) < 1e-4, tag
    got = model.get_gradients()
    assert len(got) == len(want['grads'])
    for k, (g, gw) in enumerate(zip(got, want['grads'])):
        err = np.abs(g - gw).max()
        print('[attn] %s grad %d %s err %.3e of %.3e' % (tag, k, g.shape, err, np.abs(gw).max()))
        assert err < 1e-4 * np.abs(gw).max() + 1e-7, (tag, k, err)
    model.decoder = None
    want_i, _ = AO.model_forward(stages, x64, lens)
    got_i = model.predict(x, lens)
    model.decoder = {'is_greedy': True}
    assert _rel(got_i.transpose(1, 0, 2), want_i) < 1e-4, tag
    from oracle import optim as OO
    opt = OO.Adam(lr=1e-3, clipnorm=400.0)
    for _ in range(3):
        m = model.train_on_batch([('slab', slab), labels, lens])
        out = AO.train_step(stages, x64, labels, lens, opt)
    assert abs(m[1] - float(np.mean(out['ctc']))) < 1e-4 * abs(m[1])
    for k, (a, b) in enumerate(zip(AO.weights(stages), model.get_weights())):
        err = np.abs(b - a).max()
        assert err < 5e-5 * max(1.0, np.abs(a).max()), (tag, 'w', k, err)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def _blocks(seed=2):
    """(a): Dense(32) -> PositionalEncoding -> two pre-LN blocks (2 heads of 16, d_ff 48) -> LN ->
    Dense(8)."""
    from asr_study_amd.core import layers as L, optimizers
    from asr_study_amd.core.models import ctc_model
    x_in = L.Input(name='inputs', shape=(None, 10))
    o = L.TimeDistributed(L.Dense(32))(x_in)
    o = L.PositionalEncoding()(o)
    for _ in range(2):
        y = L.MultiHeadAttention(2)(L.LayerNormalization()(o))
        o = L.merge([L.Dropout(0.0)(y), o], mode='sum')
        y = L.TimeDistributed(L.Dense(48))(L.LayerNormalization()(o))
        y = L.TimeDistributed(L.Dense(32))(L.Activation('relu')(y))
        o = L.merge([L.Dropout(0.0)(y), o], mode='sum')
    o = L.TimeDistributed(L.Dense(8))(L.LayerNormalization()(o))
    model = ctc_model(x_in, o, seed=seed)
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    assert [s.kind for s in model.stages].count('mha') == 2
    return model


def _small_transformer(seed=1):
    from asr_study_amd.core import models, optimizers
    m = models.transformer(num_features=16, num_classes=7, d_model=32, num_heads=2, num_layers=2,
                           d_ff=64, dropout=0, conv=True, conv_filters=4,
                           conv_kernels=((5, 7), (3, 5)), weight_decay=1e-4, seed=seed)
    m.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    return m


def test_attention_blocks_vs_oracle():
    rs = np.random.RandomState(4)
    N, T, F, C = 6, 21, 10, 8
    model = _blocks()
    _randomise_ln(model, rs)
    lens = np.array([21, 15, 21, 8, 12, 21])
    x = rs.randn(N, T, F).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    labels = [rs.randint(0, C - 1, size=k).tolist() for k in (3, 2, 4, 1, 2, 3)]
    _parity(model, x, lens, labels, 'blocks')


def test_transformer_with_front_end_vs_oracle():
    """The key mask follows the strided lengths (ceil(len / 2) behind the front-end)."""
    rs = np.random.RandomState(3)
    N, T, F, C = 5, 37, 16, 7
    model = _small_transformer()
    _randomise_ln(model, rs)
    lens = np.array([37, 20, 37, 9, 30])
    x = (rs.randn(N, T, F) * 2.0 + 1.0).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    labels = [rs.randint(0, C - 1, size=k).tolist() for k in (3, 2, 4, 1, 2)]
    _parity(model, x, lens, labels, 'transformer-conv')


def test_time_padding_independence():
    """New with this layer: the logits on an utterance's valid frames do not depend on how far
    the batch is padded in time (the keys past its length carry probability 0)."""
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
        print('[attn] utterance %d (len %d): T 40 vs T 56 rel %.2e' % (n, lens[n], e))
        assert e < 1e-6, (n, e)


@pytest.mark.parametrize('build', ['blocks', 'transformer'])
def test_padding_independence(build):
    """tests/test_gpu_layernorm.py::test_padding_independence on the attention models: the same 3
    utterances alone and inside a batch of 6, the same T and n_pad: bit-equal."""
    rs = np.random.RandomState(6)
    model = _blocks() if build == 'blocks' else _small_transformer()
    F = model.num_features
    _randomise_ln(model, rs)
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
    model = models.transformer(conv=False, num_features=16, num_classes=12, d_model=32,
                               num_heads=2, num_layers=2, d_ff=64, dropout=0, seed=3, **kw)
    model.compile(optimizer=optimizers.Adam(lr=3e-3, clipnorm=400))
    rs = np.random.RandomState(0)
    x = rs.randn(4, 60, 16).astype(np.float32)
    lab = [list(rs.randint(1, 11, size=5)) for _ in range(4)]
    return model, x, lab


# the oracle's greedy LER is 0 first at its step 160: `python tools/attn_learn_oracle.py` (host,
# about a minute) runs AO.train_step on learn_setup() and prints that step
ORACLE_LER0_STEP = 160


def test_transformer_learns_a_fixed_batch():
    """Overfits 4 utterances (T = 60, 5 labels each) to greedy LER 0.  The float64 oracle's
    train_step, run on the host from the same initial weights, batch and Adam(lr=3e-3,
    clipnorm=400), reaches LER 0 at step 160 (counted from 1, ORACLE_LER0_STEP); the test allows
    twice that, 320."""
    model, x, lab = learn_setup()
    slab = model.to_slab(x)
    cap = 2 * ORACLE_LER0_STEP
    ler = None
    for step in range(1, cap + 1):
        m = model.train_on_batch([('slab', slab), lab, np.full(4, 60)])
        ler = m[3]
        if ler == 0.0:
            break
    print('[learn] transformer greedy LER 0 at step %d (oracle %d, cap %d)'
          % (step, ORACLE_LER0_STEP, cap))
    assert ler == 0.0, (step, m)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def test_full_size_transformer_steps():
    """transformer() defaults at the cfg3 input (64 x 10 s, log-mel-80): 5 steps give finite
    losses and weights, every W_qkv and W_o moves, no fallback."""
    from asr_study_amd.core import models, optimizers
    model = models.transformer(seed=0)
    model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
    assert [(s.heads, s.dh) for s in model.stages if s.kind == 'mha'] == [(4, 64)] * 6
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
             if t.name in ('W_qkv', 'W_o')]
    assert len(moved) == 12 and all(moved)


def test_cli_roundtrip_transformer(tmp_path):
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
    train.main(['--dataset', fname, '--model', 'transformer', '--model_params', 'num_features',
                '16', 'd_model', '32', 'num_heads', '2', 'num_layers', '2', 'd_ff', '64',
                'num_classes', '28', 'conv_filters', '4', 'conv_kernels', '[[5,7],[3,5]]',
                '--num_epochs', '1', '--batch_size', '4', '--save', out, '--seed', '1',
                '--lr', '0.001'])
    best = os.path.join(out, 'best.h5')
    assert os.path.exists(best)
    model = core_utils.load_model(best, mode='predict', decoder=False)
    assert [s.kind for s in model.stages].count('mha') == 2
    assert model.config['name'] == 'transformer'
    saved = []
    with h5lite.File(best, 'r') as f:
        g = f['model_weights']
        names = g.attrs.get_strings('layer_names')
        assert [n for n in names if n.startswith('multiheadattention')] == \
            ['multiheadattention_1', 'multiheadattention_2']
        for lname in names:
            wn = g[lname].attrs.get_strings('weight_names')
            if lname.startswith('multiheadattention'):
                assert wn == ['%s_%s:0' % (lname, k) for k in ('W_qkv', 'b_qkv', 'W_o', 'b_o')]
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
