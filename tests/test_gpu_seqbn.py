"""GPU checks of K18, the sequence-wise batch normalisation of the GRU input projection
(csrc/batchnorm.hip asr_seqbn_*; layers.GRU(batch_norm=True); deep_speech2(batch_norm=
'recurrent', rnn_type='gru')) against the float64 oracle tests/seqbn_oracle.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import seqbn_oracle as SO
from tests.bn_cases import (SEQBN_CASES as CASES, ragged as _ragged, seqbn_inputs,
                            run_seqbn_kernels as _run_kernels)
from tests.test_gpu_gru import _gpu_gates, _gpu_masks, _labels, ds2_batch, stack_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


@pytest.mark.parametrize('ragged', [True, False], ids=['ragged', 'full'])
@pytest.mark.parametrize('T,N,n_pad,ld,W,Hp,H', CASES)
def test_kernel_parity(T, N, n_pad, ld, W, Hp, H, ragged):
    p, gamma, beta, da, lens, rm, rv, pad = seqbn_inputs(T, N, n_pad, ld, W, Hp, H, ragged)
    y, stats, dp, dg, db, yi, mom, mx = _run_kernels(p, N, W, lens, gamma, beta, da, rm, rv)
    pr = p[:, :N, :W].astype(np.float64)
    yw, c = SO.seqbn_forward(pr, gamma, beta, lens, 1e-3)
    dpw, dgw, dbw = SO.seqbn_backward(da[:, :N, :W].astype(np.float64), c)
    errs = dict(y=_rel(y[:, :N, :W], yw), dp=_rel(dp[:, :N, :W], dpw), dgamma=_rel(dg, dgw),
                dbeta=_rel(db, dbw),
                mean=_rel(stats[:W].astype(np.float64) + stats[W:2 * W], c['mean']),
                var=float(np.abs(stats[3 * W:4 * W] - c['var']).max()
                          / max(c['var'].max(), 1e-3)),
                infer=_rel(yi[:, :N, :W], SO.seqbn_infer(pr, gamma, beta, rm, rv, 1e-3)))
    print('[seqbn] %s %s' % ((T, N, n_pad, ld, W, ragged),
                             ' '.join('%s %.2e' % kv for kv in sorted(errs.items()))))
    for k in ('y', 'dp', 'dgamma', 'dbeta', 'infer'):
        assert errs[k] < 1e-5, (k, errs[k])
    assert errs['mean'] < 1e-6 and errs['var'] < 1e-5, errs
    assert stats[4 * W] == c['nv'] and not stats[4 * W + 1:].any()
    for a in (y, dp, yi):       # padding rows and columns are written as exact zeros
        assert not a[:, N:].any() and not a[:, :, W:].any()
    if pad.any():               # ... and so are the pad columns inside a GRU slab; their var is 0
        assert not y[:, :N, :W][..., pad].any() and not dp[:, :N, :W][..., pad].any()
        assert not stats[3 * W:4 * W][pad].any()
    assert mx[0] == np.abs(dp).max()
    assert mom[0] == c['nv'] and np.abs(mom[4:4 + W]).max() < 1e-3 * c['nv']


def test_padded_frames_are_out_of_the_statistics():
    """Changing p at rows t >= len_n leaves stats and the moments block bit-identical and changes
    y only at those rows."""
    rs = np.random.RandomState(3)
    T, N, n_pad, W = 40, 9, 16, 72
    lens = _ragged(rs, T, N)
    p = (rs.randn(T, n_pad, W) * 2 + 1).astype(np.float32)
    da = rs.randn(T, n_pad, W).astype(np.float32)
    gamma, beta = rs.rand(W) + 0.5, rs.randn(W)
    rm = rs.randn(W)
    a = _run_kernels(p, N, W, lens, gamma, beta, da, shift=rm)
    V = np.zeros((T, n_pad), bool)
    V[:, :N] = SO.valid_mask(T, N, lens)
    p2 = p.copy()
    p2[:, :N][~V[:, :N]] += (rs.randn(int((~V[:, :N]).sum()), W) * 3 + 1).astype(np.float32)
    b = _run_kernels(p2, N, W, lens, gamma, beta, da, shift=rm)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[6], b[6])      # stats, moments
    assert np.array_equal(a[0][V], b[0][V])
    assert not np.array_equal(a[0][:, :N][~V[:, :N]], b[0][:, :N][~V[:, :N]])
    assert a[6][0] == V.sum()
    # without lengths every frame counts: the statistics move
    c = _run_kernels(p2, N, W, None, gamma, beta, da, shift=rm)
    assert not np.array_equal(a[1][:W], c[1][:W]) and c[6][0] == T * N


def test_kernels_are_deterministic():
    rs = np.random.RandomState(1)
    T, N, n_pad, W = 200, 64, 64, 3072
    p = rs.randn(T, n_pad, W).astype(np.float32)
    da = rs.randn(T, n_pad, W).astype(np.float32)
    gamma, beta = rs.rand(W) + 0.5, rs.randn(W)
    lens = rs.randint(T // 2, T + 1, size=N)
    a = _run_kernels(p, N, W, lens, gamma, beta, da, np.zeros(W), np.ones(W))
    b = _run_kernels(p, N, W, lens, gamma, beta, da, np.zeros(W), np.ones(W))
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_running_update_and_guard():
    """The EMA from a moments block of weight |V|; with a non-zero flag word (a plain input here)
    the update leaves the statistics bit for bit as they were; a zero-weight block does too."""
    from asr_study_amd import ops
    rs = np.random.RandomState(2)
    T, N, n_pad, W = 9, 5, 16, 12
    lens = np.array([9, 4, 1, 7, 9])
    p = rs.randn(T, n_pad, W).astype(np.float32) * 2 + 1
    da = np.zeros_like(p)
    rm0, rv0 = rs.randn(W), rs.rand(W) + 0.5
    _, c = SO.seqbn_forward(p[:, :N].astype(np.float64), np.ones(W), np.zeros(W), lens)
    for shift in (None, rm0):       # single process (the batch mean) / data parallel (running mean)
        out = _run_kernels(p, N, W, lens, np.ones(W), np.zeros(W), da, shift=shift)
        stats, mom = _dev(out[1]), _dev(out[6])
        assert out[6][0] == lens.sum() == c['nv']
        want = SO.moments_block(p[:, :N].astype(np.float64), lens, 1.0,
                                c['mean'] if shift is None else shift)
        assert np.abs(out[6] - want).max() < 1e-5 * np.abs(want).max()
        rm, rv = _dev(rm0), _dev(rv0)
        sh = stats[:W] if shift is None else rm.clone()
        flags = torch.tensor([0, 3, 0, 0], dtype=torch.int32, device='cuda:0')
        ops.bn_update_running(rm, rv, mom, W, 0.9, shift=sh, flags=flags)
        assert np.array_equal(rm.cpu().numpy(), rm0.astype(np.float32))
        assert np.array_equal(rv.cpu().numpy(), rv0.astype(np.float32))
        flags.zero_()
        ops.bn_update_running(rm, rv, mom, W, 0.9, shift=sh, flags=flags)
        assert _rel(rm.cpu().numpy(), SO.ema(rm0, c['mean'], 0.9)) < 1e-5
        assert _rel(rv.cpu().numpy(), SO.ema(rv0, c['var'], 0.9)) < 1e-5
    # a zero-weight dummy rank: w = 0, an all-zero block, no update from it alone
    out = _run_kernels(p, N, W, lens, np.ones(W), np.zeros(W), da, shift=rm0, weight=0.0)
    assert not out[6].any()
    rm, rv = _dev(rm0), _dev(rv0)
    ops.bn_update_running(rm, rv, _dev(out[6]), W, 0.9, shift=rm.clone(),
                          flags=torch.zeros(4, dtype=torch.int32, device='cuda:0'))
    assert np.array_equal(rm.cpu().numpy(), rm0.astype(np.float32))


def test_two_rank_moments_pool_to_the_union_batch():
    """Data parallel bookkeeping on one device: the blocks of two shards (shift = the common
    running mean, w = each shard's |V|) summed, as the gradient all-reduce sums them, give the EMA
    of the union batch's moments."""
    from asr_study_amd import ops
    rs = np.random.RandomState(5)
    T, n_pad, W = 12, 16, 20
    shards = [(4, np.array([12, 5, 9, 1])), (7, np.array([3, 12, 12, 8, 2, 6, 11]))]
    rm0, rv0 = rs.randn(W) * 0.3, rs.rand(W) + 0.5
    total, ps = np.zeros(4 + 2 * W, np.float32), []
    for N, lens in shards:
        p = (rs.randn(T, n_pad, W) * 1.5 + rs.randn(W)).astype(np.float32)
        total += _run_kernels(p, N, W, lens, np.ones(W), np.zeros(W), np.zeros_like(p),
                              shift=rm0)[6]
        ps.append(p[:, :N].astype(np.float64))
    V = np.concatenate([SO.valid_mask(T, N, lens) for N, lens in shards], axis=1)
    rows = np.concatenate(ps, axis=1)[V]
    rm, rv = _dev(rm0), _dev(rv0)
    ops.bn_update_running(rm, rv, _dev(total), W, 0.9, shift=rm.clone(),
                          flags=torch.zeros(4, dtype=torch.int32, device='cuda:0'))
    assert total[0] == V.sum()
    assert _rel(rm.cpu().numpy(), SO.ema(rm0, rows.mean(axis=0), 0.9)) < 1e-5
    assert _rel(rv.cpu().numpy(), SO.ema(rv0, rows.var(axis=0), 0.9)) < 1e-5


# ---------------------------------------------------------------- models
def _randomise_bn(model, rs):
    """gamma / beta / running moments of every BN stage and batch-normalised GRU away from their
    1 / 0 / 0 / 1 start."""
    w = model.get_weights()
    k = 0
    for s in model.stages:
        if s.kind in ('conv', 'dense'):
            k += 2
        elif s.kind == 'bn' or (s.kind == 'bigru' and s.bn):
            for _ in range(1 if s.kind == 'bn' else 2):
                k += 0 if s.kind == 'bn' else 2
                n = w[k].size
                w[k] = (rs.rand(n) + 0.5).astype(np.float32)
                w[k + 1] = (rs.randn(n) * 0.2).astype(np.float32)
                w[k + 2] = (rs.randn(n) * 0.3).astype(np.float32)
                w[k + 3] = (rs.rand(n) + 0.5).astype(np.float32)
                k += 4
        elif s.kind == 'bigru':
            k += 6
    assert k == len(w)
    model.set_weights(w)


def _bias_before_bn(model):
    """get_weights() indices of the biases of conv / dense stages a BN stage follows."""
    out, k = set(), 0
    st = [s for s in model.stages if s.kind not in ('noise', 'reshape')]
    for i, s in enumerate(st):
        if s.kind in ('conv', 'dense') and i + 1 < len(st) and st[i + 1].kind == 'bn':
            out.add(k + 1)
        k += {'conv': 2, 'dense': 2, 'bn': 4}.get(s.kind, 0)
        if s.kind == 'bigru':
            k += 12 if s.bn else 6
    return out


def _sides(model, stages, x64, masks, N, lens):
    """test_gpu_gru._sides with the lengths handed to the oracle's forward pass."""
    _, caches = SO.model_forward(stages, x64, masks, seq_len=lens)
    sides = {}
    for si, s in enumerate(model.stages):
        if s.kind != 'bigru':
            continue
        sides[si] = _gpu_gates(model, si, N)
        own = np.stack([c['gates'] for c in caches[si]['cs']], axis=2)
        share = SO.GO.side_share(own, sides[si], s.H)
        print('[seqbn] stage %d: share of gate entries on another side than the oracle %.2e'
              % (si, share))
        assert share <= 1e-4, (si, share)
    return sides


def _model_parity(model, x, lens, labels, masks_on, tag, rs):
    """The method and tolerances of test_gpu_gru._model_parity on the batch-normalised oracle:
    logits and CTC to rtol 1e-4, every gradient entry within 2e-4 max|ref| + 1e-6 (none left
    out), then three Adam steps: weights -- the running moments among them, i.e. the oracle's EMA
    -- within 5e-5 max(1, max|w|).  The saturation sides come from the GPU's saved gates."""
    from asr_study_amd.core import optimizers
    from oracle import optim as OO
    N = x.shape[0]
    slab = model.to_slab(x)
    n_pad = slab.shape[1]
    stages = SO.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    masks_g = None
    if masks_on:
        masks_g = {}
        for si, s in enumerate(model.stages):
            if s.kind == 'bigru':
                BW = ((rs.rand(2, n_pad, s.f_in_pad) > 0.2) / 0.8).astype(np.float32)
                BU = ((rs.rand(2, n_pad, s.Hp) > 0.2) / 0.8).astype(np.float32)
                masks_g[si] = (_dev(BW), _dev(BU))
    # inference on the running moments, before anything moves them
    model.decoder = None
    want_i, _ = SO.model_forward(stages, x64, training=False)
    got_i = model.predict(x, lens)
    assert _rel(got_i.transpose(1, 0, 2), want_i) < 1e-4, tag
    ctc, logits, _ = model.loss_and_grads(slab, labels, lens, training=True, masks=masks_g)
    torch.cuda.synchronize()
    masks_o = _gpu_masks(model, N)
    assert bool(masks_o) == masks_on
    sides = _sides(model, stages, x64, masks_o, N, lens)
    want = SO.loss_and_grads(stages, x64, labels, lens, masks_o, sides)
    got_l = logits[:, :N].cpu().numpy()
    e = np.abs(got_l - want['logits']).max()
    print('[seqbn] %s logits err %.3e of %.3e' % (tag, e, np.abs(want['logits']).max()))
    assert e <= 1e-4 * max(1.0, np.abs(want['logits']).max()), (tag, 'logits', e)
    got_ctc = ctc.cpu().numpy()[:N]
    assert np.allclose(got_ctc, want['ctc'], rtol=1e-4, atol=1e-4), (got_ctc, want['ctc'])
    got = model.get_gradients()
    assert len(got) == len(want['grads'])
    for i, (g, w) in enumerate(zip(got, want['grads'])):
        err = np.abs(g - w).max()
        print('[seqbn] %s grad %d %s err %.3e of %.3e' % (tag, i, g.shape, err, np.abs(w).max()))
        assert err <= 2e-4 * np.abs(w).max() + 1e-6, (tag, i, g.shape, err, np.abs(w).max())
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    opt = OO.Adam(lr=1e-3, clipnorm=400.0)
    for _ in range(3):
        m = model.train_on_batch([('slab', slab), labels, lens], masks=masks_g)
        masks_o = _gpu_masks(model, N)
        sides = {si: _gpu_gates(model, si, N) for si, s in enumerate(model.stages)
                 if s.kind == 'bigru'}
        out = SO.train_step(stages, x64, labels, lens, opt, masks_o, sides)
    assert abs(m[1] - float(np.mean(out['ctc']))) < 1e-4 * abs(m[1])
    # (the bias in front of a BN has an exactly zero gradient in exact arithmetic: Adam turns the
    # rounding noise of either side into steps of up to lr, tests/test_gpu_batchnorm.py)
    free = _bias_before_bn(model)
    ws = SO.weights(stages)
    assert len(ws) == len(model.get_weights())
    for k, (a, b) in enumerate(zip(ws, model.get_weights())):
        if k in free:
            assert np.abs(b - a).max() <= 3 * 1e-3 * 1.01, (tag, 'w', k)
            continue
        err = np.abs(b - a).max()
        assert err < 5e-5 * max(1.0, np.abs(a).max()), (tag, 'w', k, err)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def gru_bn_stack(F, C, seed=2, dropout=0.0):
    """Bidirectional(GRU(batch_norm=True)) x 2 built by hand: 'concat' into 'sum', H not a
    multiple of 4, its own epsilon and momentum in the second."""
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import ctc_model
    x_in = L.Input(name='inputs', shape=(None, F))
    o = L.Bidirectional(L.GRU(10, activation='tanh', dropout_W=dropout, dropout_U=dropout,
                              W_regularizer=L.l2(1e-4), batch_norm=True),
                        merge_mode='concat')(x_in)
    o = L.Bidirectional(L.GRU(14, activation='relu', dropout_W=dropout, dropout_U=dropout,
                              U_regularizer=L.l2(1e-4), batch_norm=True, bn_epsilon=1e-2,
                              bn_momentum=0.9), merge_mode='sum')(o)
    o = L.TimeDistributed(L.Dense(C))(o)
    return ctc_model(x_in, o, seed=seed)


def ds2_recurrent(dropout, seed=1, H=18, C=7):
    from asr_study_amd.core import models
    return models.deep_speech2(num_features=16, num_classes=C, num_hiddens=H, num_layers=2,
                               conv_filters=4, conv_kernels=((5, 7), (3, 5)), seed=seed,
                               dropout=dropout, rnn_type='gru', batch_norm='recurrent')


@pytest.mark.parametrize('masks_on', [False, True], ids=['plain', 'masks'])
def test_gru_bn_stack_vs_oracle(masks_on):
    rs = np.random.RandomState(4)
    model = gru_bn_stack(10, 8, dropout=0.2 if masks_on else 0.0)
    assert [s.kind for s in model.stages] == ['bigru', 'bigru', 'dense']
    assert all(s.bn for s in model.stages[:2])
    _randomise_bn(model, rs)
    x, lens, labels = stack_batch(rs)
    assert len(set(lens)) > 2 and lens.min() < x.shape[1]
    _model_parity(model, x, lens, labels, masks_on, 'bn-stack', rs)


@pytest.mark.parametrize('masks_on', [False, True], ids=['plain', 'masks'])
def test_deep_speech2_recurrent_vs_oracle(masks_on):
    rs = np.random.RandomState(3)
    model = ds2_recurrent(0.2 if masks_on else 0.0)
    assert [s.kind for s in model.stages].count('bigru') == 2
    _randomise_bn(model, rs)
    x, lens, labels = ds2_batch(rs)
    _model_parity(model, x, lens, labels, masks_on, 'ds2-recurrent', rs)


def test_running_moments_follow_the_oracle_ema_and_predict_uses_them():
    """One step: the running moments equal the oracle's EMA of the valid-frame batch moments.
    predict then runs on them: an utterance's output does not depend on the rest of the batch,
    and it changes when the running moments change."""
    from asr_study_amd.core import optimizers
    rs = np.random.RandomState(7)
    model = ds2_recurrent(0.0)
    _randomise_bn(model, rs)
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    x, lens, labels = ds2_batch(rs)
    N = x.shape[0]
    slab = model.to_slab(x)
    stages = SO.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    _, caches = SO.model_forward(stages, x64, seq_len=lens)
    model.train_on_batch([('slab', slab), labels, lens])
    w = model.get_weights()
    k = 0
    for st, c in zip(stages, caches):
        if st['type'] == 'bigru_bn':
            for d, key in enumerate(('fwd', 'bwd')):
                q, bn = st['p'][key], c['cs'][d]['bn']
                assert bn['nv'] == sum(-(-l // 2) for l in lens)
                assert _rel(w[k + 4], SO.ema(q['rm'], bn['mean'], 0.99)) < 1e-5
                assert _rel(w[k + 5], SO.ema(q['rv'], bn['var'], 0.99)) < 1e-5
                k += 6
        else:
            k += len(SO.GO.weights([st]))
    model.decoder = None
    both = model.predict(x[:2], lens[:2])
    alone = model.predict(x[:1], lens[:1])
    other = model.predict(np.stack([x[0], x[3] * 3 + 1]), [lens[0], lens[3]])
    assert np.abs(both[0] - alone[0]).max() < 1e-5 * max(1.0, np.abs(alone).max())
    assert np.abs(other[0] - alone[0]).max() < 1e-5 * max(1.0, np.abs(alone).max())
    w2 = list(w)
    i = [j for j, a in enumerate(w2) if a.shape == (54,)][2]       # a GRU's running mean
    w2[i] = w2[i] + 0.5
    model.set_weights(w2)
    assert np.abs(model.predict(x[:1], lens[:1]) - alone).max() > 1e-3


def test_a_vetoed_step_leaves_the_running_moments_alone():
    """One step with a planted flag word (what a timed-out recurrent kernel leaves behind): the
    update and the running-moment EMA are both skipped on the device."""
    from asr_study_amd import ops
    from asr_study_amd.core import optimizers
    rs = np.random.RandomState(8)
    model = ds2_recurrent(0.0)
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    x, lens, labels = ds2_batch(rs)
    batch = [x, labels, lens]
    model.train_on_batch(batch)
    run0, par0 = model.bn_running.clone(), model.params.clone()
    word = ops.WS.get('lstm_bwd', 0, model.device)[:4].view(torch.int32)
    word[0] = 1
    try:
        model.train_on_batch(batch, sync=False)
        torch.cuda.synchronize()
        assert torch.equal(model.bn_running, run0) and torch.equal(model.params, par0)
    finally:
        word[0] = 0
    torch.cuda.synchronize()
    model.train_on_batch(batch, sync=False)
    torch.cuda.synchronize()
    assert not torch.equal(model.bn_running, run0) and not torch.equal(model.params, par0)


def test_deep_speech2_recurrent_learns_a_fixed_batch():
    """The criterion of test_gpu_gru.test_deep_speech2_gru_learns_a_fixed_batch: 4 utterances,
    greedy LER 0 within 200 Adam steps (here with unequal lengths)."""
    from asr_study_amd.core import models, optimizers
    model = models.deep_speech2(num_features=16, num_classes=12, num_hiddens=32, num_layers=2,
                                conv_filters=8, conv_kernels=((5, 7), (3, 5)), dropout=0.0,
                                seed=3, rnn_type='gru', batch_norm='recurrent')
    model.compile(optimizer=optimizers.Adam(lr=3e-3, clipnorm=400))
    rs = np.random.RandomState(0)
    x = rs.randn(4, 60, 16).astype(np.float32)
    lens = np.array([60, 44, 52, 60])
    for n in range(4):
        x[n, lens[n]:] = 0
    lab = [list(rs.randint(1, 11, size=5)) for _ in range(4)]
    slab = model.to_slab(x)
    ler = None
    for step in range(200):
        m = model.train_on_batch([('slab', slab), lab, lens])
        ler = m[3]
        if ler == 0.0:
            break
    print('[learn] ds2-recurrent greedy LER %r at step %d' % (ler, step))
    assert ler == 0.0, (step, m)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


_CLI = r'''
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import train
import eval as eval_cli
import predict as predict_cli
from asr_study_amd import cli
from asr_study_amd.datasets import h5lite
from asr_study_amd.utils import core_utils, keras_config as K
tmp = %(tmp)r
fmt = 'h5' if h5lite.available() else 'npz'
fname = os.path.join(tmp, 'dummy.' + fmt)
cli.make_dataset_main(['--parser', 'dummy', '--parser_params', 'num_speakers', '4',
                       'num_utterances_per_speaker', '6', 'max_duration', '1.2',
                       'min_duration', '0.6', 'max_label_length', '8', 'split',
                       '[0.5, 0.25]', 'seed', '3', '--input_parser', 'logfbank',
                       '--input_parser_params', 'num_filt', '16', '--output_file', fname])
out = os.path.join(tmp, 'run')
train.main(['--dataset', fname, '--model', 'deep_speech2', '--model_params', 'num_features',
            '16', 'num_hiddens', '18', 'num_layers', '2', 'num_classes', '28',
            'conv_filters', '4', 'conv_kernels', '[[5,7],[3,5]]', 'batch_norm', 'recurrent',
            'rnn_type', 'gru', '--num_epochs', '1', '--batch_size', '4', '--save', out,
            '--seed', '1', '--lr', '0.001'])
best = os.path.join(out, 'best.h5')
assert os.path.exists(best)
model = core_utils.load_model(best, mode='predict', decoder=False)
gru = [s for s in model.stages if s.kind == 'bigru']
assert len(gru) == 2 and all(s.bn for s in gru)
assert [s.kind for s in model.stages].count('bn') == 2
assert model.config['kwargs']['batch_norm'] == 'recurrent'
# the running moments were trained and travelled through the file
w = model.get_weights()
rm = [a for a in w if a.shape == (54,)][2]
assert np.abs(rm).max() > 0
rs = np.random.RandomState(2)
x = rs.randn(2, 30, 16).astype(np.float32)
want = model.predict(x, [30, 25])
m2 = K.topology_from_config(K.model_config(model))
m2.set_weights(model.get_weights())
m2.decoder = None
assert np.abs(m2.predict(x, [30, 25]) - want).max() < 1e-5
m = eval_cli.main(['--model', best, '--dataset', fname, '--beam_width', '10'])
assert len(m) == 4 and np.isfinite(m[1]) and m[3] >= 0
res = predict_cli.main(['--model', best, '--dataset', fname, '--no_decoder'])
assert res[0]['best'].ndim == 2 and res[0]['best'].shape[1] == 28
assert all(np.isfinite(r['best']).all() for r in res)
print('CLI-OK')
'''


def test_cli_roundtrip_deep_speech2_recurrent(tmp_path):
    """train.py --model deep_speech2 --model_params batch_norm recurrent rnn_type gru, then the
    checkpoint through load_model, topology_from_config, eval.py and predict.py, in a child
    process."""
    script = tmp_path / 'cli_seqbn.py'
    script.write_text(_CLI % dict(root=ROOT, tmp=str(tmp_path)))
    p = subprocess.run([sys.executable, str(script)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    text = p.stdout.decode(errors='replace')
    assert p.returncode == 0 and 'CLI-OK' in text, text[-4000:]


# ---------------------------------------------------------------- data parallel
def _run_worker(world, port):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', ASR_FORCE_ALLREDUCE='1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node',
           str(world), '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(ROOT, 'tests', 'seqbn_dp_worker.py')]
    out = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=560, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    line = [ln for ln in out.stdout.decode().splitlines() if ln.startswith('RESULT ')][0]
    return json.loads(line[7:])


def _check_worker(res, world):
    assert res['world'] == world and res['stages'] == 2
    assert res['w_pooled'] == res['valid_frames_all_ranks']
    assert res['running_mean_err'] < 1e-5 and res['running_var_err'] < 1e-5
    assert res['ranks_agree']


@pytest.mark.timeout(600)
def test_moments_pooling_through_the_allreduce_at_world_one():
    """The data-parallel path (moments about the running mean, pooled by the gradient all-reduce)
    on the single GPU: the collective is an identity, the bookkeeping is the real one."""
    _check_worker(_run_worker(1, 29591), 1)


@pytest.mark.timeout(600)
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs a second GPU')
def test_moments_pooling_through_the_allreduce_at_world_two():
    _check_worker(_run_worker(2, 29593), 2)
