"""-m gpu: the SimpleRNN kernels (csrc/rnn.hip) and the maas / deep_speech models against the
float64 oracle (tests/simple_rnn_oracle.py), full-size steps, a learning run and the command
line round trip."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import simple_rnn_oracle as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ['tanh', 'relu', 'linear', ('clipped_relu', 20.0)]


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def _status_ok(ws):
    from asr_study_amd import ops
    ops.lstm_status(ws)         # raises on a set timeout word


def _num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# (H, n_pad, T): every width of the issue, both batch paddings, capped so that the float64
# oracle stays well under a minute per case
SHAPES = [(4, 16, 1), (4, 64, 50), (36, 16, 200), (36, 64, 7), (100, 16, 50), (100, 64, 200),
          (256, 16, 50), (256, 64, 50), (1824, 64, 7), (1824, 16, 7), (2048, 64, 7),
          (2048, 16, 7)]


@pytest.mark.parametrize('mode', [1, 2], ids=['stepwise', 'persistent'])
@pytest.mark.parametrize('H,n_pad,T', SHAPES)
def test_kernel_parity(H, n_pad, T, mode):
    from asr_study_amd import ops
    Hp = (H + 3) // 4 * 4
    if mode == 2 and not ops.rnn_plan(max(T, 2), n_pad, Hp, mode=2)['persistent']:
        pytest.skip('persistent form not resident here')
    if mode == 2 and T == 1:
        T = 2                   # (a one-step sequence has no hand-off)
    rs = np.random.RandomState(H + n_pad + T)
    for k, act in enumerate(ACTS):
        masked, merge = bool(k % 2), ('sum', 'concat')[(k // 2 + H) % 2]
        scale = 1.0 / np.sqrt(Hp)
        U = np.zeros((2, Hp, Hp))
        U[:, :H, :H] = rs.randn(2, H, H) * scale * (0.9 if act == 'tanh' else 0.6)
        zx = np.zeros((T, n_pad, 2, Hp))
        zx[..., :H] = rs.randn(T, n_pad, 2, H) * (3.0 if act != 'tanh' else 1.0)
        BU = ((rs.rand(2, n_pad, Hp) > 0.25) / 0.75) if masked else None
        want_h = SR.kernel_forward(zx, U, act, BU)
        dy = rs.randn(T, n_pad, Hp) if merge == 'sum' else rs.randn(T, n_pad, 2 * Hp)
        want_dz = SR.kernel_backward(dy if merge == 'sum' else dy.reshape(T, n_pad, 2, Hp), U,
                                     want_h, act, BU, shared=merge == 'sum')
        h = torch.zeros(T, n_pad, 2, Hp, device='cuda:0')
        ysum = torch.zeros(T, n_pad, Hp, device='cuda:0') if merge == 'sum' else None
        Ud, BUd = _dev(U), (None if BU is None else _dev(BU))
        ws = ops.rnn_seq_fwd(_dev(zx), Ud, h, T, n_pad, Hp, act=act, mask_u=BUd, y_sum=ysum,
                             mode=mode)
        _status_ok(ws)
        got_h = h.cpu().numpy()
        assert np.abs(got_h - want_h).max() <= 1e-4 * max(1e-3, np.abs(want_h).max()), (act, 'h')
        if ysum is not None:
            ws_ = want_h[:, :, 0] + want_h[:, :, 1]
            assert np.abs(ysum.cpu().numpy() - ws_).max() <= 1e-4 * max(1e-3, np.abs(ws_).max())
        # BPTT reads the oracle's h: the backward pass is tested on its own
        dz = torch.zeros(T, n_pad, 2, Hp, device='cuda:0')
        dbp = torch.zeros(n_pad // 16, 2, Hp, device='cuda:0')
        zmx = torch.zeros(1, device='cuda:0')
        ws = ops.rnn_seq_bwd(_dev(dy), Ud, _dev(want_h), dz, T, n_pad, Hp, act=act, mask_u=BUd,
                             shared_dy=merge == 'sum', mode=mode, db_part=dbp, dz_absmax=zmx)
        _status_ok(ws)
        got_dz = dz.cpu().numpy()
        ref = max(1e-3, np.abs(want_dz).max())
        assert np.abs(got_dz - want_dz).max() <= 1e-4 * ref, (act, 'dz')
        want_db = want_dz.reshape(T, n_pad // 16, 16, 2, Hp).sum(axis=(0, 2))
        assert np.abs(dbp.cpu().numpy() - want_db).max() <= 1e-4 * max(1e-3, np.abs(want_db).max())
        assert abs(float(zmx.item()) - np.abs(want_dz).max()) <= 1e-4 * ref


def test_plan_reports_a_form():
    from asr_study_amd import ops
    for H in (1824, 2048):
        for bwd in (False, True):
            p = ops.rnn_plan(1000, 64, H, backward=bwd)
            assert p['rows'] == 64 and p['units'] == 16
            assert p['blocks'] == 2 * ((H + 15) // 16)
    assert ops.rnn_plan(100, 16, 256)['rows'] == 16
    assert not ops.rnn_plan(100, 64, 2048, mode=1)['persistent']


# ---------------------------------------------------------------- models
def _model_case(factory, H, N, T, masks_on, seed=0, gpu_kinks=False):
    from asr_study_amd.core import models
    F, C = 26, 29
    model = getattr(models, factory)(num_features=F, num_classes=C, num_hiddens=H, dropout=0.1,
                                     seed=seed)
    rs = np.random.RandomState(seed + 1)
    x = rs.randn(N, T, F).astype(np.float32)
    lens = np.array([T - (i % 4) * (T // 8) for i in range(N)])
    labels = [list(rs.randint(1, C - 1, size=max(1, int(l) // 6))) for l in lens]
    slab = model.to_slab(x)
    n_pad = slab.shape[1]
    stages = SR.stages_from_model(model)
    masks_g = masks_o = None
    if masks_on:
        masks_g, masks_o = {}, {}
        for si, s in enumerate(model.stages):
            if s.kind == 'birnn':
                BW = ((rs.rand(2, n_pad, s.f_in_pad) > 0.1) / 0.9).astype(np.float32)
                BU = ((rs.rand(2, n_pad, s.Hp) > 0.1) / 0.9).astype(np.float32)
                masks_g[si] = (_dev(BW), _dev(BU))
                masks_o[si] = (BW[:, :N, :s.f_in].astype(np.float64),
                               BU[:, :N, :s.H].astype(np.float64))
    ctc, logits, _ = model.loss_and_grads(slab, labels, lens, training=masks_on, masks=masks_g)
    torch.cuda.synchronize()
    if masks_on:        # the Dropout stages drew their own keep masks: hand them to the oracle
        for si, s in enumerate(model.stages):
            if s.kind == 'dropout' and 'mask' in model._acts[si]:
                masks_o[si] = model._acts[si]['mask'][:, :N].cpu().numpy().astype(np.float64)
    kinks = None
    if gpu_kinks:
        # the derivative masks of the clipped ReLUs from the GPU's forward outputs (SR.model_forward)
        kinks = {}
        for si, s in enumerate(model.stages):
            if s.kind == 'act':
                kinks[si] = model._acts[si]['out'][:, :N, :s.f_out].cpu().numpy().astype(np.float64)
            elif s.kind == 'birnn':
                kinks[si] = model._acts[si]['h'][:, :N, :, :s.H].cpu().numpy().astype(np.float64)
    want = SR.loss_and_grads(stages, x.transpose(1, 0, 2).astype(np.float64), labels, lens,
                             masks_o, kinks)
    e = np.abs(logits[:, :N].cpu().numpy() - want['logits']).max()
    assert e <= 1e-4 * max(1.0, np.abs(want['logits']).max()), ('logits', e)
    got_ctc = ctc.cpu().numpy()[:N]
    assert np.allclose(got_ctc, want['ctc'], rtol=1e-4, atol=1e-4), (got_ctc, want['ctc'])
    for i, (g, w) in enumerate(zip(model.get_gradients(), want['grads'])):
        err = np.abs(g - w).max()
        assert err <= 2e-4 * np.abs(w).max() + 1e-6, (i, g.shape, err, np.abs(w).max())
    return model


@pytest.mark.parametrize('masks_on', [False, True], ids=['plain', 'masks'])
@pytest.mark.parametrize('factory,H', [('maas', 32), ('deep_speech', 64), ('maas', 50)])
def test_model_parity_small(factory, H, masks_on):
    _model_case(factory, H, 16, 60, masks_on)


@pytest.mark.parametrize('factory,H', [('maas', 1824), ('deep_speech', 2048)])
def test_model_parity_reference_width(factory, H):
    """At 1824 / 2048 units, 3.3 M pre-activations per layer: some lie within rounding distance
    of a clipped-ReLU kink, so the oracle's backward takes the kinks' sides from the GPU's
    forward outputs (the arithmetic is still the oracle's, in float64)."""
    _model_case(factory, H, 16, 100, False, gpu_kinks=True)


def _batch(model, N, T, C, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(N, T, model.num_features).astype(np.float32)
    lab = [list(rs.randint(1, C - 1, size=T // 12)) for _ in range(N)]
    return x, lab, np.full(N, T)


def test_full_size_deep_speech_steps():
    from asr_study_amd.core import models, optimizers
    model = models.deep_speech(seed=0)
    model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
    x, lab, lens = _batch(model, 64, 1000, 29, 5)
    slab = model.to_slab(x)
    for _ in range(5):
        m = model.train_on_batch([('slab', slab), lab, lens])
        assert np.all(np.isfinite(m))
    assert model.fallbacks == 0 and model.vetoed_steps == 0
    assert all(np.isfinite(w).all() for w in model.get_weights())


def test_deep_speech_learns_a_fixed_batch():
    """Overfits 4 utterances: greedy LER reaches 0 (first run on an MI355X: at step 44; the
    bound is 200 Adam steps)."""
    from asr_study_amd.core import models, optimizers
    model = models.deep_speech(num_features=26, num_hiddens=64, dropout=0.0, seed=3)
    model.compile(optimizer=optimizers.Adam(lr=3e-3, clipnorm=400))
    rs = np.random.RandomState(0)
    x = rs.randn(4, 40, 26).astype(np.float32)
    lab = [list(rs.randint(1, 28, size=5)) for _ in range(4)]
    slab = model.to_slab(x)
    ler = None
    for step in range(200):
        m = model.train_on_batch([('slab', slab), lab, np.full(4, 40)])
        ler = m[3]
        if ler == 0.0:
            break
    assert ler == 0.0, (step, m)


def test_cli_roundtrip_deep_speech(tmp_path):
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
                           '[0.5, 0.25]', 'seed', '3', '--input_parser', 'mfcc',
                           '--input_parser_params', 'dd', 'False', '--output_file', fname])
    out = str(tmp_path / 'run')
    train.main(['--dataset', fname, '--model', 'deep_speech', '--model_params', 'num_features',
                '26', 'num_hiddens', '24', 'num_classes', '28', '--num_epochs', '1',
                '--batch_size', '4', '--save', out, '--seed', '1', '--lr', '0.001'])
    best = os.path.join(out, 'best.h5')
    assert os.path.exists(best)
    model = core_utils.load_model(best, mode='predict', decoder=False)
    assert [s.kind for s in model.stages].count('birnn') == 1
    rs = np.random.RandomState(2)
    x = rs.randn(2, 30, 26).astype(np.float32)
    want = model.predict(x, [30, 25])
    from asr_study_amd.utils import keras_config as K
    # the functional-graph route (a bare Keras file) rebuilds the same network
    m2 = K.topology_from_config(K.model_config(model))
    m2.set_weights(model.get_weights())
    m2.decoder = None
    assert np.abs(m2.predict(x, [30, 25]) - want).max() < 1e-5
    m = eval_cli.main(['--model', best, '--dataset', fname, '--beam_width', '10'])
    assert len(m) == 4 and np.isfinite(m[1]) and m[3] >= 0
    res = predict_cli.main(['--model', best, '--dataset', fname, '--no_decoder'])
    assert res[0]['best'].ndim == 2 and res[0]['best'].shape[1] == 28
    assert all(np.isfinite(r['best']).all() for r in res)
