"""-m gpu: the LayerNormalization kernels (csrc/layernorm.hip) and the layer-normalised models
against the float64 oracle (tests/layernorm_oracle.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import gru_oracle as GO
from tests import layernorm_oracle as LO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _run_kernels(x, dy, gain, bias, N, H, Hp, segs, want_dx=True):
    """x, dy (T, n_pad, ld), gain, bias (ld) host float32 -> y, stats, dx, dgain, dbias, y without
    stats (host arrays).  Outputs start from a sentinel: what is not written shows."""
    from asr_study_amd import ops
    T, n_pad, ld = x.shape
    xd, dyd, g, b = _dev(x), _dev(dy), _dev(gain), _dev(bias)
    y, y2 = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
    stats = torch.full((ops.ln_stats_len(T, n_pad),), 7.0, device='cuda:0')
    ops.ln_fwd(xd, y, g, b, N, H, Hp, segs, EPS, stats=stats)
    ops.ln_fwd(xd, y2, g, b, N, H, Hp, segs, EPS)              # inference: no stats kept
    dx = torch.full_like(xd, 7.0) if want_dx else None
    dg, db = torch.full((ld,), 7.0, device='cuda:0'), torch.full((ld,), 7.0, device='cuda:0')
    ops.ln_bwd(xd, dyd, g, stats, dx, dg, db, N, H, Hp, segs)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in (y, stats, dx, dg, db, y2)]


# (T, N, n_pad, ld, H, Hp, segs): width 1 (var 0, y = bias), 3, 28, two segments with pads
# between, 1026 of 1028, the 1280 conv image, 2 x 1024, maas' 2 x 1824, and 64 000 rows
CASES = [(1, 1, 16, 4, 1, 4, 1), (7, 5, 16, 4, 3, 4, 1), (9, 4, 16, 28, 28, 28, 1),
         (50, 13, 16, 32, 13, 16, 2), (33, 20, 32, 1028, 1026, 1028, 1),
         (20, 9, 16, 1280, 1280, 1280, 1), (12, 50, 64, 2048, 1024, 1024, 2),
         (5, 3, 16, 3648, 1824, 1824, 2), (1000, 64, 64, 32, 32, 32, 1)]


@pytest.mark.parametrize('T,N,n_pad,ld,H,Hp,segs', CASES)
def test_kernel_parity(T, N, n_pad, ld, H, Hp, segs):
    """y, stats, dx, dgain, dbias against the oracle on the real rows and columns, junk everywhere
    else.  Three special rows where the case has room for them (at least 3 real rows of at least
    3 features): all zeros, a constant (var 0), and mean 100 with std 1."""
    rs = np.random.RandomState(T + ld)
    cols = LO.real_columns(H, Hp, segs)
    F = len(cols)
    pad = np.setdiff1d(np.arange(ld), cols)
    x = (rs.randn(T, n_pad, ld) * 3.0).astype(np.float32)      # junk in pad rows / columns
    x[:, :N, cols] = (rs.randn(T, N, F) * 1.5 + rs.randn(T, N, 1)).astype(np.float32)
    special = T * N >= 3 and F >= 3
    if special:
        rows = [(0, 0), (T - 1, N - 1), (T // 2, N // 2)]
        assert len(set(rows)) == 3
        x[rows[0][0], rows[0][1], cols] = 0.0
        x[rows[1][0], rows[1][1], cols] = 0.25
        off = rs.randn(F)
        off = (off - off.mean()) / off.std() + 100.0
        x[rows[2][0], rows[2][1], cols] = off.astype(np.float32)
    gain = np.zeros(ld, np.float32)
    bias = np.zeros(ld, np.float32)
    gain[cols], bias[cols] = rs.rand(F) + 0.5, rs.randn(F) * 0.3
    gain[pad], bias[pad] = 5.0, 5.0                            # never read into an output
    dy = rs.randn(T, n_pad, ld).astype(np.float32)
    y, stats, dx, dg, db, y2 = _run_kernels(x, dy, gain, bias, N, H, Hp, segs)
    xr = x[:, :N][:, :, cols].astype(np.float64)
    yw, c = LO.ln_forward(xr, gain[cols].astype(np.float64), bias[cols].astype(np.float64), EPS)
    dxw, dgw, dbw = LO.ln_backward(dy[:, :N][:, :, cols].astype(np.float64), c)
    yg, dxg = y[:, :N][:, :, cols], dx[:, :N][:, :, cols]
    st = stats.reshape(T, n_pad, 2)[:, :N]
    errs = dict(dx=_rel(dxg, dxw), dgain=_rel(dg[cols], dgw), dbias=_rel(db[cols], dbw),
                mu=_rel(st[..., 0], c['mean']), r=_rel(st[..., 1], c['r']))
    if special:
        t, n = rows[2]
        mu, sigma = abs(c['mean'][t, n]), np.sqrt(c['var'][t, n])
        bound = 1e-5 + 2.0 * mu * 2.0 ** -24 / sigma
        errs['y_offset_row'] = _rel(yg[t, n], yw[t, n])
        keep = np.ones((T, N), bool)
        keep[t, n] = False
        errs['y'] = _rel(yg[keep], yw[keep])
        print('[ln] offset row: mu %.3f sigma %.3f bound %.3e' % (mu, sigma, bound))
    else:
        errs['y'] = _rel(yg, yw)
    print('[ln] %s: %s' % ((T, N, n_pad, ld, H, Hp, segs),
                           ' '.join('%s %.2e' % kv for kv in sorted(errs.items()))))
    assert errs['y'] < 1e-5
    if special:
        assert errs['y_offset_row'] < bound
        assert np.array_equal(yg[0, 0], bias[cols])             # the zero row: y = bias
    if F == 1:
        assert np.array_equal(yg[..., 0], np.full((T, N), bias[cols][0]))
    assert errs['dx'] < 1e-5 and errs['dgain'] < 1e-5 and errs['dbias'] < 1e-5
    assert errs['mu'] < 1e-6 and errs['r'] < 1e-5
    assert np.array_equal(y, y2)                                # with and without stats
    for a in (y, dx):           # padding rows and columns are written as exact zeros
        assert not a[:, N:].any() and not a[:, :, pad].any()
    assert not dg[pad].any() and not db[pad].any()


def test_backward_without_input_gradient():
    """dx = NULL (the first trainable stage): dgain / dbias are the same bits."""
    rs = np.random.RandomState(5)
    T, N, n_pad, ld = 9, 5, 16, 40
    x = rs.randn(T, n_pad, ld).astype(np.float32)
    dy = rs.randn(T, n_pad, ld).astype(np.float32)
    gain, bias = (rs.rand(ld) + 0.5).astype(np.float32), rs.randn(ld).astype(np.float32)
    a = _run_kernels(x, dy, gain, bias, N, ld, ld, 1)
    b = _run_kernels(x, dy, gain, bias, N, ld, ld, 1, want_dx=False)
    assert b[2] is None and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


def test_kernels_are_deterministic():
    rs = np.random.RandomState(1)
    T, N, n_pad, ld = 500, 64, 64, 1280
    x = rs.randn(T, n_pad, ld).astype(np.float32)
    dy = rs.randn(T, n_pad, ld).astype(np.float32)
    gain, bias = (rs.rand(ld) + 0.5).astype(np.float32), rs.randn(ld).astype(np.float32)
    a = _run_kernels(x, dy, gain, bias, N, ld, ld, 1)
    b = _run_kernels(x, dy, gain, bias, N, ld, ld, 1)
    for u, v in zip(a, b):
        assert np.isfinite(u).all() and np.array_equal(u, v)


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


def _gpu_gates(model, si, N):
    s = model.stages[si]
    g = model._acts[si]['gates'][:, :N].cpu().numpy().astype(np.float64)
    T = g.shape[0]
    return np.ascontiguousarray(g.reshape(T, N, 2, 3, s.Hp)[..., :s.H]).reshape(T, N, 2, 3 * s.H)


def _gru_sides(model, stages, x64, N):
    """GRU stages only (tests/test_gpu_gru.py): the oracle's backward takes the saturation side
    of every hard-sigmoid gate entry from the GPU's saved gates, after checking that the oracle's
    own forward lands on another side for at most 1e-4 of each stage's entries."""
    gru = [si for si, s in enumerate(model.stages) if s.kind == 'bigru']
    if not gru:
        return None
    _, caches = LO.model_forward(stages, x64)
    sides = {}
    for si in gru:
        sides[si] = _gpu_gates(model, si, N)
        own = np.stack([c['gates'] for c in caches[si]['cs']], axis=2)
        share = GO.side_share(own, sides[si], model.stages[si].H)
        print('[ln] stage %d: share of gate entries on another side than the oracle %.2e'
              % (si, share))
        assert share <= 1e-4, (si, share)
    return sides


def _parity(model, x, lens, labels, tag):
    """The scheme and bounds of tests/test_gpu_batchnorm.py: logits, per-sample CTC, every
    gradient, predict, three Adam steps."""
    N = x.shape[0]
    slab = model.to_slab(x)
    stages = LO.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    ctc, logits, sl = model.loss_and_grads(slab, labels, lens, training=True)
    torch.cuda.synchronize()
    want = LO.loss_and_grads(stages, x64, labels, lens, sides=_gru_sides(model, stages, x64, N))
    e = _rel(logits[:, :N].cpu().numpy(), want['logits'])
    print('[ln] %s logits rel err %.3e' % (tag, e))
    assert e < 1e-4, tag
    assert _rel(ctc.cpu().numpy()[:N], want['ctc']) < 1e-4, tag
    got = model.get_gradients()
    assert len(got) == len(want['grads'])
    for k, (g, gw) in enumerate(zip(got, want['grads'])):
        err = np.abs(g - gw).max()
        print('[ln] %s grad %d %s err %.3e of %.3e' % (tag, k, g.shape, err, np.abs(gw).max()))
        assert err < 1e-4 * max(np.abs(gw).max(), 1e-3) + 1e-7, (tag, k, err)
    # inference: the same computation
    model.decoder = None
    want_i, _ = LO.model_forward(stages, x64, training=False)
    got_i = model.predict(x, lens)
    model.decoder = {'is_greedy': True}
    assert _rel(got_i.transpose(1, 0, 2), want_i) < 1e-4, tag
    assert np.abs(want_i - want['logits']).max() == 0.0         # no phase in the oracle either
    from oracle import optim as OO
    opt = OO.Adam(lr=1e-3, clipnorm=400.0)
    for _ in range(3):
        m = model.train_on_batch([('slab', slab), labels, lens])
        sides = {si: _gpu_gates(model, si, N) for si, s in enumerate(model.stages)
                 if s.kind == 'bigru'}
        out = LO.train_step(stages, x64, labels, lens, opt, sides or None)
    assert abs(m[1] - float(np.mean(out['ctc']))) < 1e-4 * abs(m[1])
    for k, (a, b) in enumerate(zip(LO.weights(stages), model.get_weights())):
        err = np.abs(b - a).max()
        assert err < 5e-5 * max(1.0, np.abs(a).max()), (tag, 'w', k, err)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def _chain(H, seed=2):
    from asr_study_amd.core import layers as L, optimizers
    from asr_study_amd.core.models import ctc_model
    x_in = L.Input(name='inputs', shape=(None, 10))
    o = L.TimeDistributed(L.Dense(20))(x_in)
    o = L.LayerNormalization()(o)
    o = L.Activation(L.clipped_relu(3.0))(o)
    o = L.Bidirectional(L.SimpleRNN(H, activation='tanh'), merge_mode='concat')(o)
    o = L.LayerNormalization()(o)
    o = L.TimeDistributed(L.Dense(8))(o)
    model = ctc_model(x_in, o, seed=seed)
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    assert [s.kind for s in model.stages] == ['dense', 'ln', 'act', 'birnn', 'ln', 'dense']
    return model


@pytest.mark.parametrize('H', [12, 13], ids=['H12-no-pad-gap', 'H13-two-segments'])
def test_dense_ln_simple_rnn_chain_vs_oracle(H):
    """Dense -> LayerNormalization -> Activation -> Bidirectional(SimpleRNN) -> LayerNormalization
    -> Dense; H 13 pads the two directions apart (Hp 16): the second LN runs on two segments."""
    rs = np.random.RandomState(4)
    N, T, F, C = 6, 21, 10, 8
    model = _chain(H)
    assert model.stages[4].segs == (2 if H == 13 else 1)
    _randomise_ln(model, rs)
    lens = np.array([21, 15, 21, 8, 12, 21])
    x = rs.randn(N, T, F).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    labels = [rs.randint(0, C - 1, size=k).tolist() for k in (3, 2, 4, 1, 2, 3)]
    _parity(model, x, lens, labels, 'dense-ln-rnn-H%d' % H)


def _ds2_ln(rnn_type, F=16, C=7, H=16, L=2, seed=1):
    from asr_study_amd.core import models, optimizers
    m = models.deep_speech2(num_features=F, num_classes=C, num_hiddens=H, num_layers=L,
                            conv_filters=4, conv_kernels=((5, 7), (3, 5)), dropout=0.0,
                            weight_decay=1e-4, seed=seed, batch_norm='layer', rnn_type=rnn_type)
    m.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    return m


@pytest.mark.parametrize('rnn_type', ['lstm', 'gru'])
def test_deep_speech2_layer_norm_vs_oracle(rnn_type):
    """deep_speech2(batch_norm='layer'), dropout 0: logits, per-sample CTC, every gradient (gain
    and bias included), predict, and three Adam steps.  The zeroed time-padding frames are
    frames like any other."""
    rs = np.random.RandomState(3)
    N, T, F, C = 5, 37, 16, 7
    model = _ds2_ln(rnn_type, F, C, 16, 2)
    _randomise_ln(model, rs)
    lens = np.array([37, 20, 37, 9, 30])
    x = (rs.randn(N, T, F) * 2.0 + 1.0).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    labels = [rs.randint(0, C - 1, size=k).tolist() for k in (3, 2, 4, 1, 2)]
    _parity(model, x, lens, labels, 'ds2-ln-' + rnn_type)


@pytest.mark.parametrize('build', ['chain', 'ds2'])
def test_padding_independence(build):
    """The property BatchNormalization lacks: an utterance's logits do not depend on what else is
    in the batch.  The same 3 utterances alone and inside a batch of 6, both padded to the same T.
    BIT-equal: both batches pad to the same 16 sample rows, so every kernel runs the same
    geometry (the same GEMM tiles, the same batch tile of the recurrences), each sample row is
    computed from that row alone, and LayerNormalization takes its statistics from the row."""
    rs = np.random.RandomState(6)
    model = _chain(13) if build == 'chain' else _ds2_ln('lstm')
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


def test_deep_speech2_layer_norm_learns_a_fixed_batch():
    """Overfits 4 utterances to greedy LER 0 within 300 Adam steps, with no fallback or veto."""
    from asr_study_amd.core import models, optimizers
    model = models.deep_speech2(num_features=16, num_classes=12, num_hiddens=32, num_layers=2,
                                conv_filters=8, conv_kernels=((5, 7), (3, 5)), dropout=0.0,
                                seed=3, batch_norm='layer')
    model.compile(optimizer=optimizers.Adam(lr=3e-3, clipnorm=400))
    rs = np.random.RandomState(0)
    x = rs.randn(4, 60, 16).astype(np.float32)
    lab = [list(rs.randint(1, 11, size=5)) for _ in range(4)]
    slab = model.to_slab(x)
    ler = None
    for step in range(300):
        m = model.train_on_batch([('slab', slab), lab, np.full(4, 60)])
        ler = m[3]
        if ler == 0.0:
            break
    print('[learn] ds2-ln greedy LER 0 at step %d' % step)
    assert ler == 0.0, (step, m)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def test_full_size_deep_speech2_layer_norm_steps():
    """cfg3 geometry (64 x 10 s, log-mel-80), rnn_type 'lstm': 5 steps give finite losses and
    weights, no fallback."""
    from asr_study_amd.core import models, optimizers
    model = models.deep_speech2(seed=0, batch_norm='layer', rnn_type='lstm')
    model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
    assert [(s.ld, s.segs) for s in model.stages if s.kind == 'ln'] == \
        [(1280, 1), (640, 1), (640, 1)] + [(1024, 1)] * 4
    rs = np.random.RandomState(5)
    x = rs.randn(64, 1000, 80).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=60)) for _ in range(64)]
    slab = model.to_slab(x)
    for _ in range(5):
        m = model.train_on_batch([('slab', slab), lab, np.full(64, 1000)])
        assert np.all(np.isfinite(m))
    assert model.fallbacks == 0 and model.vetoed_steps == 0
    w = model.get_weights()
    assert all(np.isfinite(a).all() for a in w)
    # gain and bias moved off their 1 / 0 start
    k = 0
    for s in model.stages:
        if s.kind == 'ln':
            assert np.abs(w[k] - 1).max() > 0 and np.abs(w[k + 1]).max() > 0
        k += len(s.tensors)


def test_cli_roundtrip_deep_speech2_layer_norm(tmp_path):
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
    train.main(['--dataset', fname, '--model', 'deep_speech2', '--model_params', 'num_features',
                '16', 'num_hiddens', '16', 'num_layers', '2', 'num_classes', '28',
                'conv_filters', '4', 'conv_kernels', '[[5,7],[3,5]]', 'batch_norm', 'layer',
                '--num_epochs', '1', '--batch_size', '4', '--save', out, '--seed', '1',
                '--lr', '0.001'])
    best = os.path.join(out, 'best.h5')
    assert os.path.exists(best)
    model = core_utils.load_model(best, mode='predict', decoder=False)
    assert [s.kind for s in model.stages].count('ln') == 4
    assert model.config['kwargs']['batch_norm'] == 'layer'
    # the reloaded weights are the saved ones: the file's arrays, group by group
    saved = []
    with h5lite.File(best, 'r') as f:
        g = f['model_weights']
        names = g.attrs.get_strings('layer_names')
        assert [n for n in names if n.startswith('layernormalization')] == \
            ['layernormalization_%d' % k for k in (1, 2, 3, 4)]
        for lname in names:
            wn = g[lname].attrs.get_strings('weight_names')
            if lname.startswith('layernormalization'):
                assert wn == ['%s_gain:0' % lname, '%s_bias:0' % lname]
            saved += [g[lname][w].read_array() for w in wn]
    w = model.get_weights()
    assert len(saved) == len(w) and all(np.array_equal(a, b) for a, b in zip(saved, w))
    gains = [w[k] for k, t in enumerate(t for s in model.stages for t in s.tensors)
             if t.name == 'gain']
    assert len(gains) == 4 and all(np.abs(a - 1).max() > 0 for a in gains)   # trained
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
    assert os.path.exists(str(tmp_path / 'align.jsonl')) and res is not None
