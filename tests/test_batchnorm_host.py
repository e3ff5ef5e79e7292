"""CPU checks of the BatchNormalization feature: the float64 oracle against torch.autograd, the
layer validation and factory stage lists, the Keras config / weight round trip, the C
declarations against the ctypes signatures, and the data-parallel pooling of the running
moments over gloo."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import batchnorm_oracle as BO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_bn(x, gamma, beta, eps, C, clip):
    T, N, W = x.shape
    xr = x.reshape(T, N, W // C, C)
    mu = xr.mean(dim=(0, 1, 2))
    var = xr.var(dim=(0, 1, 2), unbiased=False)
    z = gamma * (xr - mu) / torch.sqrt(var + eps) + beta
    if clip > 0:
        z = torch.clamp(z, 0.0, clip)
    return z.reshape(T, N, W), mu, var


@pytest.mark.parametrize('W,C', [(7, None), (24, 4), (1, None)])
@pytest.mark.parametrize('clip', [0.0, 1.2])
def test_oracle_matches_autograd(W, C, clip):
    rs = np.random.RandomState(3)
    T, N, eps = 5, 3, 1e-3
    Cn = W if C is None else C
    x = rs.randn(T, N, W) * 2.0 + 0.7
    gamma, beta = rs.rand(Cn) + 0.5, rs.randn(Cn) * 0.3
    G = rs.randn(T, N, W)
    y, c = BO.bn_forward(x, gamma, beta, eps, C, clip)
    dx, dg, db = BO.bn_backward(G, c)
    xt = torch.tensor(x, requires_grad=True)
    gt = torch.tensor(gamma, requires_grad=True)
    bt = torch.tensor(beta, requires_grad=True)
    yt, mu, var = _torch_bn(xt, gt, bt, eps, Cn, clip)
    (yt * torch.tensor(G)).sum().backward()
    assert np.abs(y - yt.detach().numpy()).max() < 1e-10
    assert np.abs(c['mean'] - mu.detach().numpy()).max() < 1e-10
    assert np.abs(c['var'] - var.detach().numpy()).max() < 1e-10       # biased
    assert np.abs(dx - xt.grad.numpy()).max() < 1e-10
    assert np.abs(dg - gt.grad.numpy()).max() < 1e-10
    assert np.abs(db - bt.grad.numpy()).max() < 1e-10
    # inference on given running moments
    rm, rv = rs.randn(Cn), rs.rand(Cn) + 0.1
    yi = BO.bn_infer(x, gamma, beta, rm, rv, eps, C, clip)
    xr = torch.tensor(x).reshape(T, N, W // Cn, Cn)
    zi = torch.tensor(gamma) * (xr - torch.tensor(rm)) / torch.sqrt(torch.tensor(rv) + eps) + \
        torch.tensor(beta)
    if clip > 0:
        zi = torch.clamp(zi, 0.0, clip)
    assert np.abs(yi - zi.reshape(T, N, W).numpy()).max() < 1e-10


def test_running_update_by_hand():
    """The EMA (biased batch variance, no debias), written out; torch's running_var would be
    the unbiased one, so it is not the reference here."""
    x = np.array([[[1.0, 10.0]], [[3.0, 10.0]], [[8.0, 10.0]]])      # T 3, N 1, W 2
    _, c = BO.bn_forward(x, np.ones(2), np.zeros(2))
    assert np.allclose(c['mean'], [4.0, 10.0]) and np.allclose(c['var'], [26.0 / 3.0, 0.0])
    rm, rv = np.zeros(2), np.ones(2)
    rm, rv = BO.ema(rm, c['mean'], 0.99), BO.ema(rv, c['var'], 0.99)
    assert np.allclose(rm, [0.04, 0.1]) and np.allclose(rv, [0.99 + 0.01 * 26.0 / 3.0, 0.99])
    # the moments-block route (one rank, shift = the batch mean) gives the same numbers
    blk = BO.moments_block(x, 3.0, c['mean'])
    rm2, rv2 = BO.update_from_moments(np.zeros(2), np.ones(2), blk, 0.99, shift=c['mean'])
    assert np.allclose(rm2, rm) and np.allclose(rv2, rv)


def test_layer_validation_and_stage_lists(monkeypatch):
    from asr_study_amd.core import engine
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import deep_speech2
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    for kw in (dict(mode=1), dict(axis=1), dict(gamma_regularizer=L.l2(0.1)),
               dict(beta_regularizer=L.l2(0.1))):
        with pytest.raises(NotImplementedError):
            L.BatchNormalization(**kw)
    x = L.Input(shape=(None, 12))
    assert L.BatchNormalization()(x).features == 12
    img = L.Reshape((-1, 3, 4))(x)
    y = L.BatchNormalization()(img)
    assert y.features == 12 and y.fc == (3, 4)
    plain = deep_speech2(num_features=16, num_hiddens=8, num_layers=2, conv_filters=4,
                         device='cpu')
    assert [s.kind for s in plain.stages] == ['noise', 'reshape', 'conv', 'conv', 'reshape',
                                              'bilstm', 'bilstm', 'dense']
    assert 'batch_norm' not in plain.config['kwargs']
    bn = deep_speech2(num_features=16, num_hiddens=8, num_layers=2, conv_filters=4,
                      batch_norm=True, device='cpu')
    assert [s.kind for s in bn.stages] == ['noise', 'reshape', 'conv', 'bn', 'act', 'conv', 'bn',
                                           'act', 'reshape', 'bn', 'bilstm', 'bn', 'bilstm', 'dense']
    assert bn.config['kwargs']['batch_norm'] is True
    convs = [s for s in bn.stages if s.kind == 'conv']
    assert all(s.clip == 0.0 for s in convs)
    bns = [s for s in bn.stages if s.kind == 'bn']
    assert [(s.grouped, s.C) for s in bns] == [(True, 4), (True, 4), (False, 16), (False, 16)]
    # the parameters grow by gamma + beta only; the running moments live outside them
    assert bn.n_params == plain.n_params + sum(2 * s.C for s in bns)
    assert bn.count_params() == plain.count_params() + sum(4 * s.C for s in bns)


def test_keras_config_and_weight_round_trip(monkeypatch):
    from asr_study_amd.core import engine
    from asr_study_amd.core.callbacks import keras_layers
    from asr_study_amd.core.models import deep_speech2
    from asr_study_amd.utils import keras_config as K
    monkeypatch.setattr(engine, 'DEFAULT_DEVICE', 'cpu')
    # num_hiddens 6: Hp 8, so the second BN sees pad columns behind the first BiLSTM
    m = deep_speech2(num_features=16, num_hiddens=6, num_layers=2, conv_filters=4,
                     batch_norm=True, device='cpu')
    w = m.get_weights()
    rs = np.random.RandomState(0)
    w2 = [rs.randn(*a.shape).astype(np.float32) for a in w]
    m.set_weights(w2)
    assert all(np.array_equal(a, b) for a, b in zip(w2, m.get_weights()))
    layers = keras_layers(m, w2)
    names = [n for _, ws in layers for n, _ in ws]
    for k in (1, 2, 3, 4):
        for part in ('gamma', 'beta', 'running_mean', 'running_std'):
            assert 'batchnormalization_%d_%s:0' % (k, part) in names
    assert [n for n, _ in layers][:4] == ['convolution2d_1', 'batchnormalization_1',
                                          'convolution2d_2', 'batchnormalization_2']
    # BN gamma / beta of pad columns stay zero (the pads stay exactly zero through the layer)
    s = [s for s in m.stages if s.kind == 'bn'][3]
    assert s.C == 16 and s.n_real == 12
    pad = np.setdiff1d(np.arange(16), m._bn_cols(s))
    host = m.params.numpy()
    assert np.all(host[s.og + pad] == 0) and np.all(host[s.obeta + pad] == 0)
    g = m.get_gradients()
    assert [a.shape for a in g] == [a.shape for a in w]
    cfg = K.model_config(m)
    assert '"BatchNormalization"' in cfg
    m2 = K.topology_from_config(cfg)
    assert [s.kind for s in m2.stages] == [s.kind for s in m.stages]
    assert [(s.C, s.grouped, s.eps, s.momentum) for s in m2.stages if s.kind == 'bn'] == \
        [(s.C, s.grouped, s.eps, s.momentum) for s in m.stages if s.kind == 'bn']
    m2.set_weights(m.get_weights())
    assert all(np.array_equal(a, b) for a, b in zip(m2.get_weights(), w2))
    # optimiser slots cover the trainable weights only (gamma, beta; not the running moments)
    from asr_study_amd.core import optimizers
    m.compile(optimizer=optimizers.Adam())
    ow = K.optimizer_weights(m)
    n_tr = len(w) - 2 * len([s for s in m.stages if s.kind == 'bn'])
    assert len(ow) == 1 + 2 * n_tr


def _c_type(ct):
    import ctypes as C
    return {C.c_int: 'int', C.c_float: 'float', C.c_size_t: 'size_t', C.c_int64: 'int64_t',
            C.c_double: 'double'}[ct]


def test_bn_declarations_match_signatures(tmp_path):
    """gcc checks every asr_bn_* declaration of the header against a prototype generated from
    _lib.SIGNATURES (scalars from the ctypes types, pointers where ctypes passes void*)."""
    gcc = shutil.which('gcc') or shutil.which('cc')
    if gcc is None:
        pytest.fail('no C compiler on this machine')
    import ctypes as C
    from asr_study_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'asr_hip.h')).read()
    names = sorted(n for n in _lib.SIGNATURES if n.startswith('asr_bn_'))
    assert names == ['asr_bn_bwd', 'asr_bn_fwd_infer', 'asr_bn_fwd_train',
                     'asr_bn_update_running', 'asr_bn_workspace_bytes']
    checks = []
    for n in names:
        m = re.search(r'\b(\w+)\s+%s\(([^;]*)\);' % n, hdr, re.S)
        assert m, n
        params = [p.strip() for p in m.group(2).split(',')]
        res, args = _lib.SIGNATURES[n]
        assert len(params) == len(args), n
        proto = []
        for p, a in zip(params, args):
            if a is C.c_void_p:
                assert '*' in p or p.startswith('asr_stream_t '), (n, p)
                proto.append(re.sub(r'\s*\w+$', '', p))       # the header's pointer type
            else:
                assert '*' not in p, (n, p)
                proto.append(_c_type(a))
        ret = _c_type(res)
        checks.append('_Static_assert(__builtin_types_compatible_p(__typeof__(&%s), %s (*)(%s)), '
                      '"%s");' % (n, ret, ', '.join(proto), n))
    src = tmp_path / 'bn_decl.c'
    src.write_text('#include <stdio.h>\n#include "asr_hip.h"\n' + '\n'.join(checks) +
                   '\nint main(void) { printf("%d %zu\\n", ASR_HIP_ABI_VERSION, sizeof(size_t)); '
                   'return 0; }\n')
    exe = tmp_path / 'bn_decl'
    subprocess.check_call([gcc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    abi, szt = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert abi == _lib.ABI_VERSION == 107 and szt == C.sizeof(C.c_size_t)


def _dp_worker(rank, world, port, shards, momentum, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    C = shards[0][0].shape[-1]
    rm, rv = np.zeros(C), np.ones(C)
    for batch in shards:
        x, w = batch[rank], (0.0 if batch[rank] is None else None)
        if x is None:           # a zero-weight dummy: normalises a copy of sample 0, weight 0
            x, w = batch[1 - rank][:, :1], 0.0
        T, N = x.shape[:2]
        blk = BO.moments_block(x, N * T if w is None else w, rm).astype(np.float32)
        t = torch.from_numpy(blk)
        dist.all_reduce(t)      # as the gradient all-reduce carries the blocks
        rm, rv = BO.update_from_moments(rm, rv, t.numpy().astype(np.float64), momentum)
    q.put((rank, rm, rv))
    dist.destroy_process_group()


def test_dp_pooled_running_moments_gloo():
    """World 2, uneven shards and a dummy rank: the all-reduced moments blocks give the running
    moments of the union batch, and both ranks hold the same ones."""
    import socket
    import torch.multiprocessing as mp
    rs = np.random.RandomState(11)
    T, C, mom = 6, 5, 0.9
    b1 = rs.randn(T, 5, C) * 3.0 + 2.0          # 3 + 2 samples
    b2 = rs.randn(T, 1, C) * 0.5 - 1.0          # 1 sample: rank 1 is a dummy
    shards = [[b1[:, :3], b1[:, 3:]], [b2, None]]
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    ps = [ctx.Process(target=_dp_worker, args=(r, 2, port, shards, mom, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = dict((r, (a, b)) for r, a, b in [q.get(timeout=120) for _ in ps])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    rm, rv = np.zeros(C), np.ones(C)
    for x in (b1, b2):
        _, c = BO.bn_forward(x, np.ones(C), np.zeros(C))
        rm, rv = BO.ema(rm, c['mean'], mom), BO.ema(rv, c['var'], mom)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.abs(res[0][0] - rm).max() < 1e-5 * max(1.0, np.abs(rm).max())
    assert np.abs(res[0][1] - rv).max() < 1e-5 * max(1.0, np.abs(rv).max())
