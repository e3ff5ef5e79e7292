"""-m gpu: the RHN kernels (csrc/rhn.hip), Bidirectional(RHN) stacks and the ``rhn`` factory
against the float64 oracle (tests/rhn_oracle.py), determinism, full-size steps, a learning run
and the command line round trip."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests import rhn_oracle as RO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ['tanh', 'relu', 'linear', ('clipped_relu', 20.0)]
SHAPES, case_options = RO.KERNEL_SHAPES, RO.case_options


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def kernel_case(i, k):
    """Inputs as the issue sets them: zx ~ 2 N(0, 1) on the real columns, U_l ~ (0.8 / sqrt(H))
    N(0, 1), b_l = [0 | -2 | -2]; float32-representable, so both sides start from the same
    numbers."""
    H, n_pad, T = SHAPES[i]
    act = ACTS[k]
    depth, coupling, masked, merge = case_options(i, k)
    if depth == 4:
        T = max(1, T // 2)
    Cb = RO.n_blocks(coupling)
    Hp = (H + 3) // 4 * 4
    rs = np.random.RandomState(1000 * k + H + n_pad + T)
    U = np.zeros((2, depth, Hp, Cb, Hp))
    U[:, :, :H, :, :H] = rs.randn(2, depth, H, Cb, H) * (0.8 / np.sqrt(H))
    b = np.zeros((2, depth, Cb, Hp))
    b[:, :, 1:, :H] = -2.0
    zx = np.zeros((T, n_pad, 2, Cb, Hp))
    zx[..., :H] = rs.randn(T, n_pad, 2, Cb, H) * 2.0
    BU = ((rs.rand(2, depth, n_pad, Hp) > 0.25) / 0.75) if masked else None
    dy = rs.randn(T, n_pad, Hp) if merge == 'sum' else rs.randn(T, n_pad, 2 * Hp)
    return dict(act=act, H=H, Hp=Hp, n_pad=n_pad, T=T, depth=depth, coupling=coupling, Cb=Cb,
                merge=merge, U=_f32(U.reshape(2, depth, Hp, Cb * Hp)),
                b=_f32(b.reshape(2, depth, Cb * Hp)), zx=_f32(zx.reshape(T, n_pad, 2, Cb * Hp)),
                BU=None if BU is None else _f32(BU), dy=_f32(dy))


def _close(got, want, what):
    bound = 1e-4 * max(1e-3, np.abs(want).max())
    err = np.abs(got - want).max()
    print('[rhn] %s: max err %.3e (bound %.3e)' % (what, err, bound))
    assert got.shape == want.shape and err <= bound, (what, err, bound)


@pytest.mark.parametrize('i', range(len(SHAPES)), ids=['H%d-n%d-T%d' % s for s in SHAPES])
def test_kernel_parity(i):
    """mode = 1, the stepwise form: the only one built (mode 2 is an argument error)."""
    mode = 1
    from asr_study_amd import ops
    for k in range(len(ACTS)):
        c = kernel_case(i, k)
        act, H, Hp, n_pad, T, L, coupling, Cb, merge = (c[n] for n in (
            'act', 'H', 'Hp', 'n_pad', 'T', 'depth', 'coupling', 'Cb', 'merge'))
        U, b, zx, BU, dy = (c[n] for n in ('U', 'b', 'zx', 'BU', 'dy'))
        W = Cb * Hp
        want_h, want_g = RO.kernel_forward(zx, U, b, act, coupling, BU)
        share = RO.saturated_share(want_g.reshape(L, T, n_pad, 2, Cb, Hp)[..., :H]
                                   .reshape(L, T, n_pad, 2, Cb * H), H)
        tag = 'H=%d n_pad=%d T=%d L=%d %s %s %s%s ' % (
            H, n_pad, T, L, 'coupled' if coupling else 'uncoupled', act, merge,
            ' masked' if BU is not None else '')
        print('[rhn] %s: saturated share of t / c %.3f' % (tag, share))
        assert 0.05 <= share <= 0.5, share
        h = torch.zeros(L, T, n_pad, 2, Hp, device='cuda:0')
        gates = torch.zeros(L, T, n_pad, 2, W, device='cuda:0')
        ysum = torch.zeros(T, n_pad, Hp, device='cuda:0') if merge == 'sum' else None
        Ud, BUd = _dev(U), (None if BU is None else _dev(BU))
        ops.rhn_seq_fwd(_dev(zx), Ud, _dev(b), h, gates, T, n_pad, Hp, L, coupling=coupling,
                        act=act, mask_u=BUd, y_sum=ysum, mode=mode)
        _close(h.cpu().numpy(), want_h, tag + 'states')
        _close(gates.cpu().numpy(), want_g, tag + 'gates')
        if ysum is not None:
            _close(ysum.cpu().numpy(), want_h[-1, :, :, 0] + want_h[-1, :, :, 1], tag + 'y_sum')
        # BPTT reads the oracle's states and gates, rounded to float32 first; the oracle's backward
        # is fed the same rounded values (a gate that rounds to exactly 0 or 1 has slope 0 on both
        # sides)
        h32, g32 = _f32(want_h), _f32(want_g)
        dy4 = dy if merge == 'sum' else dy.reshape(T, n_pad, 2, Hp)
        want_da = RO.kernel_backward(dy4, U, h32, g32, act, coupling, BU, shared=merge == 'sum')
        da = torch.full((L, T, n_pad, 2, W), float('nan'), device='cuda:0')
        dbp = torch.zeros(n_pad // 16, 2, L, W, device='cuda:0')
        zmx = torch.zeros(1, device='cuda:0')
        ops.rhn_seq_bwd(_dev(dy), Ud, _dev(h32), _dev(g32), da, T, n_pad, Hp, L,
                        coupling=coupling, act=act, mask_u=BUd, shared_dy=merge == 'sum',
                        mode=mode, db_part=dbp, dz_absmax=zmx)
        _close(da.cpu().numpy(), want_da, tag + 'da')
        ref = max(1e-3, np.abs(want_da).max())
        want_db = want_da.reshape(L, T, n_pad // 16, 16, 2, W).sum(axis=(1, 3))
        _close(dbp.cpu().numpy(), np.transpose(want_db, (1, 2, 0, 3)), tag + 'db_part')
        assert abs(float(zmx.item()) - np.abs(want_da).max()) <= 1e-4 * ref


def test_plan_and_argument_errors():
    from asr_study_amd import ops
    for H in (512, 1024):
        assert ops.rhn_plan(500, 64, H, depth=2) == \
            {'persistent': False, 'rows': 64, 'units': 8, 'blocks': 2 * (H // 8)}
        assert ops.rhn_plan(500, 64, H, depth=2, coupling=False) == \
            {'persistent': False, 'rows': 64, 'units': 4, 'blocks': 2 * (H // 4)}
        assert ops.rhn_plan(500, 64, H, depth=2, backward=True) == \
            {'persistent': False, 'rows': 64, 'units': 16, 'blocks': 2 * (H // 16)}
    assert ops.rhn_plan(100, 16, 256)['rows'] == 16
    with pytest.raises(Exception) as e:
        ops.rhn_plan(100, 64, 512, mode=2)              # no persistent form
    assert 'stepwise' in str(e.value)
    with pytest.raises(Exception):
        ops.rhn_plan(100, 64, 510)                      # H must be padded to a multiple of 4
    with pytest.raises(Exception) as e:
        ops.rhn_plan(100, 64, 512, depth=0)
    assert 'depth' in str(e.value)


def test_kernels_are_deterministic():
    """The same asr_rhn_seq_fwd / _bwd call twice: every output bit-identical."""
    from asr_study_amd import ops
    for (i, k) in ((5, 1), (9, 0), (2, 3), (7, 2)):
        c = kernel_case(i, k)
        Hp, n_pad, T, L, coupling, merge = (c[n] for n in ('Hp', 'n_pad', 'T', 'depth',
                                                           'coupling', 'merge'))
        T = min(T, 40)
        W = c['Cb'] * Hp
        Ud, bd, zxd, dyd = _dev(c['U']), _dev(c['b']), _dev(c['zx'][:T]), _dev(c['dy'][:T])
        BUd = None if c['BU'] is None else _dev(c['BU'])
        outs = []
        for _ in range(2):
            h = torch.zeros(L, T, n_pad, 2, Hp, device='cuda:0')
            gates = torch.zeros(L, T, n_pad, 2, W, device='cuda:0')
            ysum = torch.zeros(T, n_pad, Hp, device='cuda:0')
            ops.rhn_seq_fwd(zxd, Ud, bd, h, gates, T, n_pad, Hp, L, coupling=coupling,
                            act=c['act'], mask_u=BUd, y_sum=ysum)
            da = torch.full((L, T, n_pad, 2, W), float('nan'), device='cuda:0')
            dbp = torch.zeros(n_pad // 16, 2, L, W, device='cuda:0')
            zmx = torch.zeros(1, device='cuda:0')
            ops.rhn_seq_bwd(dyd, Ud, h, gates, da, T, n_pad, Hp, L, coupling=coupling,
                            act=c['act'], mask_u=BUd, shared_dy=merge == 'sum', db_part=dbp,
                            dz_absmax=zmx)
            outs.append([t.cpu().numpy() for t in (h, gates, ysum, da, dbp, zmx)])
        for a, b in zip(*outs):
            assert np.isfinite(a).all() and np.array_equal(a, b)


# ---------------------------------------------------------------- models
def _gpu_gates(model, si, N):
    s = model.stages[si]
    g = model._acts[si]['gates'][:, :, :N].cpu().numpy().astype(np.float64)
    L, T = g.shape[:2]
    return np.ascontiguousarray(g.reshape(L, T, N, 2, s.nblk, s.Hp)[..., :s.H]).reshape(
        L, T, N, 2, s.nblk * s.H)


def _gpu_masks(model, N):
    """The variational masks of the last forward pass, cut to the real rows and columns."""
    return RO.cut_masks(model, {si: (model._acts[si]['BW'].cpu().numpy(),
                                     model._acts[si]['BU'].cpu().numpy())
                                for si, s in enumerate(model.stages)
                                if s.kind == 'birhn' and model._acts[si].get('BW') is not None}, N)


def _sides(model, stages, x64, masks, N):
    """The GPU's saved gates per RHN stage, after checking that the oracle's OWN forward lands on
    the same side of the hard-sigmoid kinks for all but at most 1e-4 of each stage's entries."""
    _, caches = RO.model_forward(stages, x64, masks)
    sides = {}
    for si, s in enumerate(model.stages):
        if s.kind != 'birhn':
            continue
        sides[si] = _gpu_gates(model, si, N)
        own = np.stack([c['gates'] for c in caches[si]['cs']], axis=3)
        share = RO.side_share(own, sides[si], s.H)
        print('[rhn] stage %d: share of gate entries on another side than the oracle %.2e'
              % (si, share))
        assert share <= 1e-4, (si, share)
    return sides


def _pads_are_zero(model):
    """Pad columns (H <= j < Hp) stay exactly 0 in the states and in da."""
    for si, s in enumerate(model.stages):
        if s.kind == 'birhn' and s.Hp != s.H:
            h = model._acts[si]['h']
            assert float(h[..., s.H:].abs().max().item()) == 0.0
            da = model._bufs[('hda%d' % si, tuple(h.shape[:4]) + (s.nblk * s.Hp,))]
            da = da.view(tuple(h.shape[:4]) + (s.nblk, s.Hp))
            assert float(da[..., s.H:].abs().max().item()) == 0.0


def _model_parity(model, x, lens, labels, masks_on, tag, rs):
    """Logits and CTC to rtol 1e-4, every gradient to 2e-4 max|ref| + 1e-6 (no entry left out),
    then three Adam steps against the oracle's.  Each side runs its own forward; the oracle's
    backward takes the saturation side of every gate entry from the GPU's saved gates
    (RO._slopes), under the 1e-4 cap on the share that differs
    (tests/test_rhn_host.py::test_parity_inputs_keep_their_sides_in_float32 is the same condition
    on the oracle alone)."""
    from asr_study_amd.core import optimizers
    from oracle import optim as OO
    N = x.shape[0]
    slab = model.to_slab(x)
    n_pad = slab.shape[1]
    stages = RO.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    masks_g = None
    if masks_on:
        masks_g = {si: (_dev(BW), _dev(BU))
                   for si, (BW, BU) in RO.draw_masks(model, n_pad, rs).items()}
    ctc, logits, _ = model.loss_and_grads(slab, labels, lens, training=True, masks=masks_g)
    torch.cuda.synchronize()
    masks_o = _gpu_masks(model, N)
    assert bool(masks_o) == masks_on
    sides = _sides(model, stages, x64, masks_o, N)
    _pads_are_zero(model)
    want = RO.loss_and_grads(stages, x64, labels, lens, masks_o, sides)
    got_l = logits[:, :N].cpu().numpy()
    e = np.abs(got_l - want['logits']).max()
    print('[rhn] %s logits err %.3e of %.3e' % (tag, e, np.abs(want['logits']).max()))
    assert e <= 1e-4 * max(1.0, np.abs(want['logits']).max()), (tag, 'logits', e)
    got_ctc = ctc.cpu().numpy()[:N]
    e = np.abs(got_ctc - want['ctc']).max()
    assert e <= 2e-4 * np.abs(want['ctc']).max() + 1e-6, (tag, 'ctc', got_ctc, want['ctc'])
    got = model.get_gradients()
    assert len(got) == len(want['grads'])
    for i, (g, w) in enumerate(zip(got, want['grads'])):
        err = np.abs(g - w).max()
        print('[rhn] %s grad %d %s err %.3e of %.3e' % (tag, i, g.shape, err, np.abs(w).max()))
        assert err <= 2e-4 * np.abs(w).max() + 1e-6, (tag, i, g.shape, err, np.abs(w).max())
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    opt = OO.Adam(lr=1e-3, clipnorm=400.0)
    for _ in range(3):
        m = model.train_on_batch([('slab', slab), labels, lens], masks=masks_g)
        masks_o = _gpu_masks(model, N)
        sides = {si: _gpu_gates(model, si, N) for si, s in enumerate(model.stages)
                 if s.kind == 'birhn'}
        out = RO.train_step(stages, x64, labels, lens, opt, masks_o, sides)
    assert abs(m[1] - float(np.mean(out['ctc']))) <= 2e-4 * abs(m[1]) + 1e-6
    for k, (a, b) in enumerate(zip(RO.weights(stages), model.get_weights())):
        err = np.abs(b - a).max()
        assert err <= 5e-5 * max(1.0, np.abs(a).max()), (tag, 'w', k, err)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


@pytest.mark.parametrize('masks_on', [False, True], ids=['plain', 'masks'])
@pytest.mark.parametrize('case', [0, 1], ids=['stack', 'rhn'])
def test_models_vs_oracle(case, masks_on):
    tag, build, batch, seed = RO.parity_cases()[case]
    rs = np.random.RandomState(seed)
    model = build(0.2 if masks_on else 0.0)
    assert [s.kind for s in model.stages].count('birhn') == 2
    x, lens, labels = batch(rs)
    _model_parity(model, x, lens, labels, masks_on, tag, rs)


@pytest.mark.parametrize('geometry', ['cfg2', 'H512'])
def test_full_size_rhn_steps(geometry):
    """rhn() at brsmv1's cfg2 geometry (32 x 10 s, MFCC-39, 5 x 256, depth 2) and at H = 512
    (64 x 10 s, log-mel-80): five steps with finite losses, gradients and weights, no fallback,
    no veto."""
    from asr_study_amd import ops
    from asr_study_amd.core import models, optimizers
    F, H, N = (39, 256, 32) if geometry == 'cfg2' else (80, 512, 64)
    model = models.rhn(num_features=F, num_hiddens=H, depth=2, seed=0)
    assert [s.kind for s in model.stages].count('birhn') == 5
    model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
    rs = np.random.RandomState(5)
    x = rs.randn(N, 1000, F).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=60)) for _ in range(N)]
    slab = model.to_slab(x)
    for _ in range(5):
        m = model.train_on_batch([('slab', slab), lab, np.full(N, 1000)])
        assert np.all(np.isfinite(m))
        assert all(np.isfinite(g).all() for g in model.get_gradients())
    assert model.fallbacks == 0 and model.vetoed_steps == 0
    assert float(ops.lstm_timeout_flags(model.device).abs().sum().item()) == 0
    assert all(np.isfinite(w).all() for w in model.get_weights())


def test_rhn_learns_a_fixed_batch():
    """Overfits 4 utterances: greedy LER reaches 0 within ceil(1.25 * K_REF) Adam steps, K_REF the
    step at which the float64 oracle gets there from the same initial weights
    (tests/rhn_oracle.py; checked by tests/test_rhn_host.py::test_oracle_learning_step)."""
    from asr_study_amd.core import models, optimizers
    model = models.rhn(**RO.LEARN)
    model.compile(optimizer=optimizers.Adam(lr=RO.LEARN_LR, clipnorm=RO.LEARN_CLIPNORM))
    x, lab, lens = RO.learn_batch()
    slab = model.to_slab(x)
    budget = int(math.ceil(1.25 * RO.K_REF))
    ler = None
    for step in range(1, budget + 1):
        m = model.train_on_batch([('slab', slab), lab, lens])
        ler = m[3]
        if ler == 0.0:
            break
    print('[learn] rhn greedy LER %r at step %d (oracle: %d, budget %d)'
          % (ler, step, RO.K_REF, budget))
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
train.main(['--dataset', fname, '--model', 'rhn', '--model_params', 'num_features', '16',
            'num_hiddens', '18', 'num_layers', '2', 'num_classes', '28', 'depth', '2',
            'coupling', 'False', '--num_epochs', '1', '--batch_size', '4', '--save', out,
            '--seed', '1', '--lr', '0.001'])
best = os.path.join(out, 'best.h5')
assert os.path.exists(best)
model = core_utils.load_model(best, mode='predict', decoder=False)
st = [s for s in model.stages if s.kind == 'birhn']
assert len(st) == 2 and all((s.depth, s.coupling, s.H) == (2, False, 18) for s in st)
assert model.config['name'] == 'rhn' and model.config['kwargs']['depth'] == 2
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


def test_cli_roundtrip_rhn(tmp_path):
    """train.py --model rhn --model_params depth 2 ..., then the checkpoint through load_model,
    topology_from_config, eval.py and predict.py, in a child process."""
    import subprocess
    script = tmp_path / 'cli_rhn.py'
    script.write_text(_CLI % dict(root=ROOT, tmp=str(tmp_path)))
    p = subprocess.run([sys.executable, str(script)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    text = p.stdout.decode(errors='replace')
    assert p.returncode == 0 and 'CLI-OK' in text, text[-4000:]
