"""-m gpu: the GRU kernels (csrc/gru.hip), Bidirectional(GRU) stacks and
deep_speech2(rnn_type='gru') against the float64 oracle (tests/gru_oracle.py), determinism,
full-size steps, a learning run and the command line round trip."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import gru_oracle as GO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ['tanh', 'relu', 'linear', ('clipped_relu', 20.0)]

# (H, n_pad, T): every width of the issue, both batch paddings, T capped so that the float64
# oracle stays well under a minute per case
SHAPES = [(4, 16, 1), (4, 64, 50), (36, 16, 200), (36, 64, 7), (100, 16, 50), (100, 64, 200),
          (256, 16, 50), (256, 64, 50), (512, 16, 20), (512, 64, 20), (1024, 16, 7),
          (1024, 64, 7),
          # NR = 32 (part-filled last column tile; two reduction chunks) and n_pad = 48 -> NR = 16
          # with BPTT phase B's K = 2 * 132 crossing a chunk edge on a part-filled tile
          (36, 32, 7), (260, 32, 5), (132, 48, 3)]


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def kernel_case(H, n_pad, T, k):
    """Inputs of activation k of a shape: zx is scaled so that a visible share of z and r
    saturates at 0 and at 1 (|pre-activation| >= 2.5), the recurrent term is kept O(1)."""
    act = ACTS[k]
    Hp = (H + 3) // 4 * 4
    rs = np.random.RandomState(1000 * k + H + n_pad + T)
    masked, merge = bool(k % 2), ('sum', 'concat')[(k // 2 + H) % 2]
    U = np.zeros((2, Hp, 3, Hp))
    U[:, :H, :, :H] = rs.randn(2, H, 3, H) * (0.8 / np.sqrt(H))
    U = U.reshape(2, Hp, 3 * Hp)
    zx = np.zeros((T, n_pad, 2, 3, Hp))
    zx[..., :2, :H] = rs.randn(T, n_pad, 2, 2, H) * 2.0
    zx[..., 2, :H] = rs.randn(T, n_pad, 2, H) * (2.0 if act != 'tanh' else 1.0)
    zx = zx.reshape(T, n_pad, 2, 3 * Hp)
    BU = ((rs.rand(2, n_pad, Hp) > 0.25) / 0.75) if masked else None
    dy = rs.randn(T, n_pad, Hp) if merge == 'sum' else rs.randn(T, n_pad, 2 * Hp)
    # (float32-representable inputs: both sides start from the same numbers)
    return dict(act=act, Hp=Hp, merge=merge, U=_f32(U), zx=_f32(zx),
                BU=None if BU is None else _f32(BU), dy=_f32(dy))


def saturated_share(gates, H, Hp):
    g = gates.reshape(gates.shape[:-1] + (3, Hp))[..., :2, :H]
    return float(np.mean((g <= 0.0) | (g >= 1.0)))


def _close(got, want, what):
    bound = 1e-4 * max(1e-3, np.abs(want).max())
    err = np.abs(got - want).max()
    print('[gru] %s: max err %.3e (bound %.3e)' % (what, err, bound))
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize('mode', [1], ids=['stepwise'])
@pytest.mark.parametrize('H,n_pad,T', SHAPES)
def test_kernel_parity(H, n_pad, T, mode):
    """The stepwise form is the only one built (mode 2 is an argument error)."""
    from asr_study_amd import ops
    for k in range(len(ACTS)):
        c = kernel_case(H, n_pad, T, k)
        act, Hp, merge, U, zx, BU, dy = (c[n] for n in ('act', 'Hp', 'merge', 'U', 'zx', 'BU',
                                                        'dy'))
        want_h, want_g = GO.kernel_forward(zx, U, act, BU)
        share = saturated_share(want_g, H, Hp)
        print('[gru] H=%d n_pad=%d T=%d %s: saturated share %.3f' % (H, n_pad, T, act, share))
        assert 0.05 <= share <= 0.5, share
        h = torch.zeros(T, n_pad, 2, Hp, device='cuda:0')
        gates = torch.zeros(T, n_pad, 2, 3 * Hp, device='cuda:0')
        rm = torch.zeros(T, n_pad, 2, Hp, device='cuda:0')
        ysum = torch.zeros(T, n_pad, Hp, device='cuda:0') if merge == 'sum' else None
        Ud, BUd = _dev(U), (None if BU is None else _dev(BU))
        ops.gru_seq_fwd(_dev(zx), Ud, h, gates, rm, T, n_pad, Hp, act=act, mask_u=BUd,
                        y_sum=ysum, mode=mode)
        tag = 'H=%d n_pad=%d %s ' % (H, n_pad, act)
        _close(h.cpu().numpy(), want_h, tag + 'h')
        _close(gates.cpu().numpy(), want_g, tag + 'gates')
        for d in range(2):
            m = GO._prev(want_h[:, :, d], d == 1)
            if BU is not None:
                m = m * BU[d][None]
            _close(rm[:, :, d].cpu().numpy(), want_g[:, :, d, Hp:2 * Hp] * m, tag + 'rm%d' % d)
        if ysum is not None:
            _close(ysum.cpu().numpy(), want_h[:, :, 0] + want_h[:, :, 1], tag + 'y_sum')
        # BPTT reads the oracle's h and gates, rounded to float32 first; the oracle's backward is
        # fed the same rounded values (a gate that rounds to exactly 0 or 1 has slope 0 on both
        # sides)
        h32, g32 = _f32(want_h), _f32(want_g)
        dy4 = dy if merge == 'sum' else dy.reshape(T, n_pad, 2, Hp)
        want_da = GO.kernel_backward(dy4, U, h32, g32, act, BU, shared=merge == 'sum')
        da = torch.zeros(T, n_pad, 2, 3 * Hp, device='cuda:0')
        dbp = torch.zeros(n_pad // 16, 2, 3 * Hp, device='cuda:0')
        zmx = torch.zeros(1, device='cuda:0')
        ops.gru_seq_bwd(_dev(dy), Ud, _dev(h32), _dev(g32), da, T, n_pad, Hp, act=act,
                        mask_u=BUd, shared_dy=merge == 'sum', mode=mode, db_part=dbp,
                        dz_absmax=zmx)
        _close(da.cpu().numpy(), want_da, tag + 'da')
        ref = max(1e-3, np.abs(want_da).max())
        want_db = want_da.reshape(T, n_pad // 16, 16, 2, 3 * Hp).sum(axis=(0, 2))
        _close(dbp.cpu().numpy(), want_db, tag + 'db_part')
        assert abs(float(zmx.item()) - np.abs(want_da).max()) <= 1e-4 * ref


def test_plan_and_argument_errors():
    from asr_study_amd import ops
    for H in (512, 1024):
        p = ops.gru_plan(500, 64, H)
        assert p == {'persistent': False, 'rows': 64, 'units': 16, 'blocks': 2 * (2 * H // 16)}
        assert ops.gru_plan(500, 64, H, backward=True)['blocks'] == 2 * (H // 16)
    assert ops.gru_plan(100, 16, 256)['rows'] == 16
    with pytest.raises(Exception) as e:
        ops.gru_plan(100, 64, 512, mode=2)              # no persistent form
    assert 'stepwise' in str(e.value)
    with pytest.raises(Exception):
        ops.gru_plan(100, 64, 510)                      # H must be padded to a multiple of 4


def test_kernels_are_deterministic():
    """The same asr_gru_seq_fwd / _bwd call twice: bit-identical h, gates, da and db_part."""
    from asr_study_amd import ops
    for (H, n_pad, T, k) in ((100, 64, 40, 1), (512, 64, 12, 0), (36, 16, 60, 3)):
        c = kernel_case(H, n_pad, T, k)
        Hp, merge = c['Hp'], c['merge']
        Ud, zxd, dyd = _dev(c['U']), _dev(c['zx']), _dev(c['dy'])
        BUd = None if c['BU'] is None else _dev(c['BU'])
        outs = []
        for _ in range(2):
            h = torch.zeros(T, n_pad, 2, Hp, device='cuda:0')
            gates = torch.zeros(T, n_pad, 2, 3 * Hp, device='cuda:0')
            rm = torch.zeros(T, n_pad, 2, Hp, device='cuda:0')
            ops.gru_seq_fwd(zxd, Ud, h, gates, rm, T, n_pad, Hp, act=c['act'], mask_u=BUd)
            da = torch.full((T, n_pad, 2, 3 * Hp), float('nan'), device='cuda:0')
            dbp = torch.zeros(n_pad // 16, 2, 3 * Hp, device='cuda:0')
            zmx = torch.zeros(1, device='cuda:0')
            ops.gru_seq_bwd(dyd, Ud, h, gates, da, T, n_pad, Hp, act=c['act'], mask_u=BUd,
                            shared_dy=merge == 'sum', db_part=dbp, dz_absmax=zmx)
            outs.append([t.cpu().numpy() for t in (h, gates, rm, da, dbp, zmx)])
        for a, b in zip(*outs):
            assert np.isfinite(a).all() and np.array_equal(a, b)


# ---------------------------------------------------------------- models
def _gpu_gates(model, si, N):
    s = model.stages[si]
    g = model._acts[si]['gates'][:, :N].cpu().numpy().astype(np.float64)
    T = g.shape[0]
    return np.ascontiguousarray(g.reshape(T, N, 2, 3, s.Hp)[..., :s.H]).reshape(T, N, 2, 3 * s.H)


def _gpu_masks(model, N):
    """The variational masks of the last forward pass, cut to the real rows and columns."""
    out = {}
    for si, s in enumerate(model.stages):
        if s.kind == 'bigru' and model._acts[si].get('BW') is not None:
            BW = model._acts[si]['BW'].cpu().numpy().astype(np.float64)
            BU = model._acts[si]['BU'].cpu().numpy().astype(np.float64)
            out[si] = (BW[:, :N][:, :, model._real_rows(s)], BU[:, :N, :s.H])
    return out


def _sides(model, stages, x64, masks, N):
    """The GPU's saved gates per GRU stage, after checking that the oracle's OWN forward lands on
    the same side of the hard-sigmoid kinks for all but at most 1e-4 of each stage's entries."""
    _, caches = GO.model_forward(stages, x64, masks)
    sides = {}
    for si, s in enumerate(model.stages):
        if s.kind != 'bigru':
            continue
        sides[si] = _gpu_gates(model, si, N)
        own = np.stack([c['gates'] for c in caches[si]['cs']], axis=2)
        share = GO.side_share(own, sides[si], s.H)
        print('[gru] stage %d: share of gate entries on another side than the oracle %.2e'
              % (si, share))
        assert share <= 1e-4, (si, share)
    return sides


def _bias_before_bn(model):
    out, k = set(), 0
    counts = {'conv': 2, 'dense': 2, 'bn': 4, 'bigru': 6}
    st = [s for s in model.stages if s.kind not in ('noise', 'reshape')]
    for i, s in enumerate(st):
        if s.kind in ('conv', 'dense') and i + 1 < len(st) and st[i + 1].kind == 'bn':
            out.add(k + 1)
        k += counts.get(s.kind, 0)
    return out


def _model_parity(model, x, lens, labels, masks_on, tag, rs):
    """Logits and CTC to rtol 1e-4, every gradient to 2e-4 max|ref| + 1e-6 (no entry left out),
    then three Adam steps against the oracle's.  Each side runs its own forward; the oracle's
    backward takes the saturation side of every gate entry from the GPU's saved gates
    (GO._slopes), under the 1e-4 cap on the share that differs.  The oracle run in float32
    against itself in float64 on these models' inputs (CPU, before the first GPU run) differed on
    a share of 0 in every stage of every case (6840 to 11088 z and r entries per stage, 0 to 34 %
    of them saturated)."""
    from asr_study_amd.core import optimizers
    from oracle import optim as OO
    N = x.shape[0]
    slab = model.to_slab(x)
    n_pad = slab.shape[1]
    stages = GO.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    masks_g = None
    if masks_on:
        masks_g = {}
        for si, s in enumerate(model.stages):
            if s.kind == 'bigru':
                BW = ((rs.rand(2, n_pad, s.f_in_pad) > 0.2) / 0.8).astype(np.float32)
                BU = ((rs.rand(2, n_pad, s.Hp) > 0.2) / 0.8).astype(np.float32)
                masks_g[si] = (_dev(BW), _dev(BU))
    ctc, logits, _ = model.loss_and_grads(slab, labels, lens, training=True, masks=masks_g)
    torch.cuda.synchronize()
    masks_o = _gpu_masks(model, N)
    assert bool(masks_o) == masks_on
    sides = _sides(model, stages, x64, masks_o, N)
    want = GO.loss_and_grads(stages, x64, labels, lens, masks_o, sides)
    got_l = logits[:, :N].cpu().numpy()
    e = np.abs(got_l - want['logits']).max()
    print('[gru] %s logits err %.3e of %.3e' % (tag, e, np.abs(want['logits']).max()))
    assert e <= 1e-4 * max(1.0, np.abs(want['logits']).max()), (tag, 'logits', e)
    got_ctc = ctc.cpu().numpy()[:N]
    assert np.allclose(got_ctc, want['ctc'], rtol=1e-4, atol=1e-4), (got_ctc, want['ctc'])
    got = model.get_gradients()
    assert len(got) == len(want['grads'])
    for i, (g, w) in enumerate(zip(got, want['grads'])):
        err = np.abs(g - w).max()
        print('[gru] %s grad %d %s err %.3e of %.3e' % (tag, i, g.shape, err, np.abs(w).max()))
        assert err <= 2e-4 * np.abs(w).max() + 1e-6, (tag, i, g.shape, err, np.abs(w).max())
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    opt = OO.Adam(lr=1e-3, clipnorm=400.0)
    for _ in range(3):
        m = model.train_on_batch([('slab', slab), labels, lens], masks=masks_g)
        masks_o = _gpu_masks(model, N)
        sides = {si: _gpu_gates(model, si, N) for si, s in enumerate(model.stages)
                 if s.kind == 'bigru'}
        out = GO.train_step(stages, x64, labels, lens, opt, masks_o, sides)
    assert abs(m[1] - float(np.mean(out['ctc']))) < 1e-4 * abs(m[1])
    # (the bias in front of a BN has an exactly zero gradient in exact arithmetic: Adam turns the
    # rounding noise of either side into steps of up to lr, tests/test_gpu_batchnorm.py)
    free = _bias_before_bn(model)
    for k, (a, b) in enumerate(zip(GO.weights(stages), model.get_weights())):
        if k in free:
            assert np.abs(b - a).max() <= 3 * 1e-3 * 1.01, (tag, 'w', k)
            continue
        err = np.abs(b - a).max()
        assert err < 5e-5 * max(1.0, np.abs(a).max()), (tag, 'w', k, err)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


def _labels(rs, C, sizes):
    return [rs.randint(0, C - 1, size=k).tolist() for k in sizes]


def gru_stack(F, C, seed=2, dropout=0.0, device=None):
    """Bidirectional(GRU) x 2 built by hand: 'concat' into 'sum', H not a multiple of 4."""
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import ctc_model
    x_in = L.Input(name='inputs', shape=(None, F))
    o = L.Bidirectional(L.GRU(10, activation='tanh', dropout_W=dropout, dropout_U=dropout,
                              W_regularizer=L.l2(1e-4)), merge_mode='concat')(x_in)
    o = L.Bidirectional(L.GRU(14, activation='relu', dropout_W=dropout, dropout_U=dropout,
                              U_regularizer=L.l2(1e-4)), merge_mode='sum')(o)
    o = L.TimeDistributed(L.Dense(C))(o)
    kw = {} if device is None else {'device': device}
    return ctc_model(x_in, o, seed=seed, **kw)


def stack_batch(rs):
    N, T, F, C = 6, 33, 10, 8
    lens = np.array([33, 15, 33, 8, 12, 33])
    x = (rs.randn(N, T, F) * 2.0).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    return x, lens, _labels(rs, C, (3, 2, 4, 1, 2, 3))


def ds2_gru(batch_norm, dropout, device=None, seed=1):
    from asr_study_amd.core import models
    kw = {} if device is None else {'device': device}
    return models.deep_speech2(num_features=16, num_classes=7, num_hiddens=18, num_layers=2,
                               conv_filters=4, conv_kernels=((5, 7), (3, 5)), seed=seed,
                               dropout=dropout, rnn_type='gru', batch_norm=batch_norm, **kw)


def ds2_batch(rs):
    N, T, F, C = 5, 37, 16, 7
    lens = np.array([37, 20, 37, 9, 30])
    x = (rs.randn(N, T, F) * 2.0 + 1.0).astype(np.float32)
    for n in range(N):
        x[n, lens[n]:] = 0
    return x, lens, _labels(rs, C, (3, 2, 4, 1, 2))


@pytest.mark.parametrize('masks_on', [False, True], ids=['plain', 'masks'])
def test_gru_stack_vs_oracle(masks_on):
    rs = np.random.RandomState(4)
    model = gru_stack(10, 8, dropout=0.2 if masks_on else 0.0)
    assert [s.kind for s in model.stages] == ['bigru', 'bigru', 'dense']
    # spread the gate pre-activations so that both slope branches occur in the model too
    w = model.get_weights()
    model.set_weights([a * 2.5 if a.ndim == 2 and a.shape[1] in (30, 42) else a for a in w])
    x, lens, labels = stack_batch(rs)
    _model_parity(model, x, lens, labels, masks_on, 'stack', rs)


@pytest.mark.parametrize('masks_on', [False, True], ids=['plain', 'masks'])
@pytest.mark.parametrize('batch_norm', [False, True], ids=['nobn', 'bn'])
def test_deep_speech2_gru_vs_oracle(batch_norm, masks_on):
    rs = np.random.RandomState(3)
    model = ds2_gru(batch_norm, 0.2 if masks_on else 0.0)
    assert [s.kind for s in model.stages].count('bigru') == 2
    x, lens, labels = ds2_batch(rs)
    _model_parity(model, x, lens, labels, masks_on, 'ds2-gru%s' % ('-bn' if batch_norm else ''),
                  rs)


def test_full_size_deep_speech2_gru_steps():
    """cfg3 geometry (64 x 10 s, log-mel-80, 5 x 512): five steps with finite losses and weights,
    no fallback, no veto, status words 0."""
    from asr_study_amd import ops
    from asr_study_amd.core import models, optimizers
    model = models.deep_speech2(seed=0, rnn_type='gru')
    assert [s.kind for s in model.stages].count('bigru') == 5
    model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
    rs = np.random.RandomState(5)
    x = rs.randn(64, 1000, 80).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=60)) for _ in range(64)]
    slab = model.to_slab(x)
    for _ in range(5):
        m = model.train_on_batch([('slab', slab), lab, np.full(64, 1000)])
        assert np.all(np.isfinite(m))
    assert model.fallbacks == 0 and model.vetoed_steps == 0
    assert float(ops.lstm_timeout_flags(model.device).abs().sum().item()) == 0
    assert all(np.isfinite(w).all() for w in model.get_weights())


def test_deep_speech2_gru_learns_a_fixed_batch():
    """Overfits 4 utterances: greedy LER reaches 0 within the 200 Adam steps of the SimpleRNN
    test."""
    from asr_study_amd.core import models, optimizers
    model = models.deep_speech2(num_features=16, num_classes=12, num_hiddens=32, num_layers=2,
                                conv_filters=8, conv_kernels=((5, 7), (3, 5)), dropout=0.0,
                                seed=3, rnn_type='gru')
    model.compile(optimizer=optimizers.Adam(lr=3e-3, clipnorm=400))
    rs = np.random.RandomState(0)
    x = rs.randn(4, 60, 16).astype(np.float32)
    lab = [list(rs.randint(1, 11, size=5)) for _ in range(4)]
    slab = model.to_slab(x)
    ler = None
    for step in range(200):
        m = model.train_on_batch([('slab', slab), lab, np.full(4, 60)])
        ler = m[3]
        if ler == 0.0:
            break
    print('[learn] ds2-gru greedy LER %r at step %d' % (ler, step))
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
            'conv_filters', '4', 'conv_kernels', '[[5,7],[3,5]]', 'rnn_type', 'gru',
            '--num_epochs', '1', '--batch_size', '4', '--save', out, '--seed', '1',
            '--lr', '0.001'])
best = os.path.join(out, 'best.h5')
assert os.path.exists(best)
model = core_utils.load_model(best, mode='predict', decoder=False)
assert [s.kind for s in model.stages].count('bigru') == 2
assert model.config['kwargs']['rnn_type'] == 'gru'
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


def test_cli_roundtrip_deep_speech2_gru(tmp_path):
    """train.py --model deep_speech2 --model_params rnn_type gru, then the checkpoint through
    load_model, topology_from_config, eval.py and predict.py, in a child process."""
    import subprocess
    script = tmp_path / 'cli_gru.py'
    script.write_text(_CLI % dict(root=ROOT, tmp=str(tmp_path)))
    p = subprocess.run([sys.executable, str(script)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    text = p.stdout.decode(errors='replace')
    assert p.returncode == 0 and 'CLI-OK' in text, text[-4000:]
