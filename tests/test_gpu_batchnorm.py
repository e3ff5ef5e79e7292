"""-m gpu: the BatchNormalization kernels (csrc/batchnorm.hip) and the batch-normalised models
against the float64 oracle (tests/batchnorm_oracle.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import batchnorm_oracle as BO
from tests.bn_cases import BN_CASES as CASES, bn_inputs, run_bn_kernels as _run_kernels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


@pytest.mark.parametrize('clip', [0.0, 2.0], ids=['plain', 'clip'])
@pytest.mark.parametrize('T,N,n_pad,ld,W,C', CASES)
def test_kernel_parity(T, N, n_pad, ld, W, C, clip):
    Cn = W if C is None else C
    x, gamma, beta, dy, rm, rv = bn_inputs(T, N, n_pad, ld, W, C)
    y, stats, dx, dg, db, yi, mom = _run_kernels(x, N, W, Cn, gamma, beta, dy, clip, rm, rv)
    xr = x[:, :N, :W].astype(np.float64)
    yw, c = BO.bn_forward(xr, gamma, beta, 1e-3, C, clip)
    dxw, dgw, dbw = BO.bn_backward(dy[:, :N, :W].astype(np.float64), c)
    assert _rel(y[:, :N, :W], yw) < 1e-5
    assert _rel(stats[:Cn].astype(np.float64) + stats[Cn:2 * Cn], c['mean']) < 1e-6
    assert np.abs(stats[3 * Cn:] - c['var']).max() < 1e-5 * max(c['var'].max(), 1e-3)
    assert _rel(dx[:, :N, :W], dxw) < 1e-5
    assert _rel(dg, dgw) < 1e-5 and _rel(db, dbw) < 1e-5
    yiw = BO.bn_infer(xr, gamma, beta, rm, rv, 1e-3, C, clip)
    assert _rel(yi[:, :N, :W], yiw) < 1e-5
    for a in (y, dx, yi):       # padding rows and columns are written as exact zeros
        assert not a[:, N:].any() and not a[:, :, W:].any()
    assert mom[0] == N and np.abs(mom[4:4 + Cn]).max() < 1e-3 * N


def test_kernels_are_deterministic():
    rs = np.random.RandomState(1)
    T, N, n_pad, ld = 500, 64, 64, 1280
    x = rs.randn(T, n_pad, ld).astype(np.float32)
    dy = rs.randn(T, n_pad, ld).astype(np.float32)
    for C in (32, 1280):
        gamma, beta = rs.rand(C) + 0.5, rs.randn(C)
        a = _run_kernels(x, N, ld, C, gamma, beta, dy, 20.0, np.zeros(C), np.ones(C))
        b = _run_kernels(x, N, ld, C, gamma, beta, dy, 20.0, np.zeros(C), np.ones(C))
        for u, v in zip(a, b):
            assert np.array_equal(u, v)


def test_running_update_and_guard():
    """The EMA from a moments block; with a non-zero flag word (a plain input here) the update
    leaves the statistics bit for bit as they were."""
    from asr_study_amd import ops
    rs = np.random.RandomState(2)
    T, N, n_pad, C = 9, 5, 16, 12
    x = rs.randn(T, n_pad, C).astype(np.float32) * 2 + 1
    xd = _dev(x)
    stats = torch.empty(ops.bn_stats_len(C), device='cuda:0')
    mom = torch.empty(ops.bn_moments_len(C), device='cuda:0')
    y = torch.empty_like(xd)
    ops.bn_fwd_train(xd, y, _dev(np.ones(C)), _dev(np.zeros(C)), stats, N, C, C, moments=mom,
                     weight=float(N * T))
    rm0, rv0 = rs.randn(C), rs.rand(C) + 0.5
    rm, rv = _dev(rm0), _dev(rv0)
    flags = torch.tensor([0, 3, 0, 0], dtype=torch.int32, device='cuda:0')
    ops.bn_update_running(rm, rv, mom, C, 0.9, shift=stats[:C], flags=flags)
    assert np.array_equal(rm.cpu().numpy(), rm0.astype(np.float32))
    assert np.array_equal(rv.cpu().numpy(), rv0.astype(np.float32))
    flags.zero_()
    ops.bn_update_running(rm, rv, mom, C, 0.9, shift=stats[:C], flags=flags)
    _, c = BO.bn_forward(x[:, :N].astype(np.float64), np.ones(C), np.zeros(C))
    assert _rel(rm.cpu().numpy(), BO.ema(rm0, c['mean'], 0.9)) < 1e-5
    assert _rel(rv.cpu().numpy(), BO.ema(rv0, c['var'], 0.9)) < 1e-5


def _ds2_bn(F=16, C=7, H=16, L=2, seed=1):
    from asr_study_amd.core import models, optimizers
    m = models.deep_speech2(num_features=F, num_classes=C, num_hiddens=H, num_layers=L,
                            conv_filters=4, conv_kernels=((5, 7), (3, 5)), dropout=0.0,
                            weight_decay=1e-4, seed=seed, batch_norm=True)
    m.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    return m


def _randomise_bn(model, rs):
    """gamma / beta / running moments away from their 1 / 0 / 0 / 1 start."""
    w = model.get_weights()
    it = iter(range(len(w)))
    for s in model.stages:
        if s.kind in ('conv', 'dense'):
            next(it), next(it)
        elif s.kind in ('bilstm', 'birnn'):
            [next(it) for _ in range(6)]
        elif s.kind == 'bn':
            i = [next(it) for _ in range(4)]
            n = w[i[0]].size
            w[i[0]] = (rs.rand(n) + 0.5).astype(np.float32)
            w[i[1]] = (rs.randn(n) * 0.2).astype(np.float32)
            w[i[2]] = (rs.randn(n) * 0.3).astype(np.float32)
            w[i[3]] = (rs.rand(n) + 0.5).astype(np.float32)
    model.set_weights(w)


def _bias_before_bn(model):
    """get_weights() indices of the biases of conv / dense stages a BN stage follows."""
    out, k = set(), 0
    counts = {'conv': 2, 'dense': 2, 'bn': 4, 'bilstm': 6, 'birnn': 6}
    st = [s for s in model.stages if s.kind not in ('noise', 'reshape')]
    for i, s in enumerate(st):
        if s.kind in ('conv', 'dense') and i + 1 < len(st) and st[i + 1].kind == 'bn':
            out.add(k + 1)
        k += counts.get(s.kind, 0)
    return out


def _parity(model, x, lens, labels, tag, check_steps=True):
    N = x.shape[0]
    slab = model.to_slab(x)
    stages = BO.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    want = BO.loss_and_grads(stages, x64, labels, lens)
    ctc, logits, sl = model.loss_and_grads(slab, labels, lens, training=True)
    assert _rel(logits[:, :N].cpu().numpy(), want['logits']) < 1e-4, tag
    assert _rel(ctc.cpu().numpy(), want['ctc']) < 1e-4, tag
    got = model.get_gradients()
    assert len(got) == len(want['grads'])
    for k, (g, gw) in enumerate(zip(got, want['grads'])):
        err = np.abs(g - gw).max()
        assert err < 1e-4 * max(np.abs(gw).max(), 1e-3) + 1e-7, (tag, k, err)
    # inference on the running moments
    model.decoder = None
    want_i, _ = BO.model_forward(stages, x64, training=False)
    got_i = model.predict(x, lens)
    model.decoder = {'is_greedy': True}
    assert _rel(got_i.transpose(1, 0, 2), want_i) < 1e-4, tag
    if not check_steps:
        return
    from oracle import optim as OO
    opt = OO.Adam(lr=1e-3, clipnorm=400.0)
    for _ in range(3):
        out = BO.train_step(stages, x64, labels, lens, opt)
        m = model.train_on_batch([('slab', slab), labels, lens])
    assert abs(m[1] - float(np.mean(out['ctc']))) < 1e-4 * abs(m[1])
    # the bias of a layer right in front of a BN has a gradient of exactly zero in exact
    # arithmetic (the BN removes any per-channel shift): Adam normalises the rounding noise of
    # both sides into steps of up to lr each, so those biases are only held to that bound
    free = _bias_before_bn(model)
    for k, (a, b) in enumerate(zip(BO.weights(stages), model.get_weights())):
        if k in free:
            assert np.abs(b - a).max() <= 3 * 1e-3 * 1.01, (tag, 'w', k)
            continue
        assert np.abs(b - a).max() < 5e-5 * max(1.0, np.abs(a).max()), (tag, 'w', k)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def test_deep_speech2_batch_norm_vs_oracle():
    """deep_speech2(batch_norm=True), dropout 0, training phase: logits, per-sample CTC, every
    gradient (gamma / beta included), inference on the running moments, and three Adam steps
    with the running moments."""
    rs = np.random.RandomState(3)
    N, T, F, C = 5, 37, 16, 7
    model = _ds2_bn(F, C, 16, 2)
    _randomise_bn(model, rs)
    lens = np.array([37, 20, 37, 9, 30])
    x = (rs.randn(N, T, F) * 2.0 + 1.0).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    labels = [rs.randint(0, C - 1, size=k).tolist() for k in (3, 2, 4, 1, 2)]
    _parity(model, x, lens, labels, 'ds2-bn')


def test_dense_bn_simple_rnn_chain_vs_oracle():
    """Dense -> BatchNormalization -> Activation -> Bidirectional(SimpleRNN) -> Dense."""
    from asr_study_amd.core import layers as L, optimizers
    from asr_study_amd.core.models import ctc_model
    rs = np.random.RandomState(4)
    N, T, F, C, H = 6, 21, 10, 8, 12
    x_in = L.Input(name='inputs', shape=(None, F))
    o = L.TimeDistributed(L.Dense(20))(x_in)
    o = L.BatchNormalization(momentum=0.9)(o)
    o = L.Activation(L.clipped_relu(3.0))(o)
    o = L.Bidirectional(L.SimpleRNN(H, activation='tanh'), merge_mode='concat')(o)
    o = L.TimeDistributed(L.Dense(C))(o)
    model = ctc_model(x_in, o, seed=2)
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    assert [s.kind for s in model.stages] == ['dense', 'bn', 'act', 'birnn', 'dense']
    _randomise_bn(model, rs)
    lens = np.array([21, 15, 21, 8, 12, 21])
    x = rs.randn(N, T, F).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    labels = [rs.randint(0, C - 1, size=k).tolist() for k in (3, 2, 4, 1, 2, 3)]
    _parity(model, x, lens, labels, 'dense-bn-rnn')


def test_deep_speech2_batch_norm_learns_a_fixed_batch():
    """Overfits 4 utterances to greedy LER 0 within 300 Adam steps, with no fallback or veto."""
    from asr_study_amd.core import models, optimizers
    model = models.deep_speech2(num_features=16, num_classes=12, num_hiddens=32, num_layers=2,
                                conv_filters=8, conv_kernels=((5, 7), (3, 5)), dropout=0.0,
                                seed=3, batch_norm=True)
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
    print('[learn] ds2-bn greedy LER 0 at step %d' % step)
    assert ler == 0.0, (step, m)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def test_full_size_deep_speech2_batch_norm_steps():
    """cfg3 geometry (64 x 10 s, log-mel-80): 5 steps give finite losses and weights."""
    from asr_study_amd.core import models, optimizers
    model = models.deep_speech2(seed=0, batch_norm=True)
    model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
    rs = np.random.RandomState(5)
    x = rs.randn(64, 1000, 80).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=60)) for _ in range(64)]
    slab = model.to_slab(x)
    for _ in range(5):
        m = model.train_on_batch([('slab', slab), lab, np.full(64, 1000)])
        assert np.all(np.isfinite(m))
    assert model.fallbacks == 0
    assert all(np.isfinite(w).all() for w in model.get_weights())
    # the running moments moved off their 0 / 1 start
    rm = model.bn_running.cpu().numpy()
    assert np.isfinite(rm).all() and np.abs(rm).max() > 0


def test_cli_roundtrip_deep_speech2_batch_norm(tmp_path):
    sys.path.insert(0, ROOT)
    import train
    import eval as eval_cli
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
    train.main(['--dataset', fname, '--model', 'deep_speech2', '--model_params', 'num_features',
                '16', 'num_hiddens', '16', 'num_layers', '2', 'num_classes', '28',
                'conv_filters', '4', 'conv_kernels', '[[5,7],[3,5]]', 'batch_norm', 'True',
                '--num_epochs', '1', '--batch_size', '4', '--save', out, '--seed', '1',
                '--lr', '0.001'])
    best = os.path.join(out, 'best.h5')
    assert os.path.exists(best)
    model = core_utils.load_model(best, mode='predict', decoder=False)
    assert [s.kind for s in model.stages].count('bn') == 4
    assert np.abs(model.bn_running.cpu().numpy()).max() > 0      # trained moments reloaded
    rs = np.random.RandomState(2)
    x = rs.randn(2, 30, 16).astype(np.float32)
    want = model.predict(x, [30, 25])
    from asr_study_amd.utils import keras_config as K
    m2 = K.topology_from_config(K.model_config(model))
    m2.set_weights(model.get_weights())
    m2.decoder = None
    assert np.abs(m2.predict(x, [30, 25]) - want).max() < 1e-5
    m = eval_cli.main(['--model', best, '--dataset', fname, '--beam_width', '10'])
    assert len(m) == 4 and np.isfinite(m[1]) and m[3] >= 0
    res = predict_cli.main(['--model', best, '--dataset', fname, '--no_decoder'])
    assert all(np.isfinite(r['best']).all() for r in res)
