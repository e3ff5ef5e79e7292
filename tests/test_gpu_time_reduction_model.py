"""-m gpu: models with a TimeReduction stage (K33) against the float64 oracle compositions of
tests/time_reduction_oracle.py.  Tiny shapes, an odd number of frames in front of every reduction
(so that a partial group exists), ragged lengths, dropout 0.

The reduction adds no arithmetic, so every comparison uses the bound of the existing test of the
same stack without the stage; each test names that test beside its bound."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import aed_oracle as AO
from tests import lstm_uni_oracle as LU
from tests import rnnt_oracle as RO
from tests import time_reduction_oracle as TR
from tests import test_gpu_gru as TG
from tests import test_gpu_lstm_uni as TLU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lstm_stages(model):
    return [si for si, s in enumerate(model.stages) if s.kind == 'bilstm']


def _treduce(model):
    return [si for si, s in enumerate(model.stages) if getattr(s, 'time_factor', 0)]


# ---------------------------------------------------------------- LSTM stacks, CTC
def _lstm_sides(model, stages, x64, lens, N):
    """The GPU's saved gates as the oracle's saturation sides (tests/test_gpu_lstm_uni.py), under
    the 1e-4 cap on the share of gate entries on another side than the oracle's own."""
    _, caches, _ = TR.model_forward(stages, x64, lens)
    own = LU.stage_gates(stages, caches)
    sides = {}
    for si in _lstm_stages(model):
        sides[si] = TLU._gpu_gates(model, si, N)
        assert sides[si].shape == own[si].shape         # (each stage on its own time axis)
        share = LU.side_share(own[si], sides[si])
        assert share <= 1e-4, (si, share)
    return sides


def _ctc_parity(model, tag, uni):
    """uni: procedure and bounds of tests/test_gpu_lstm_uni.py::test_models_vs_oracle
    (_model_parity, _three_adam_steps): logits 1e-4 max(1, |logits|), CTC rtol = atol = 1e-4,
    every gradient 2e-4 max|ref| + 1e-6, the weights after three Adam(1e-3, clipnorm 400) steps
    5e-5 max(1, |w|); saturation sides from the GPU's gates.
    not uni: those of tests/test_gpu_model.py::test_brsmv1_small_forward_backward_adam and
    ::test_brsmv1_residual_connections: logits 1e-4, CTC rtol 1e-4, every gradient 1e-4
    max(1e-3, |ref|) + 1e-6, the weights after three Adam(1e-2, clipnorm 0.5) steps 5e-5; the
    oracle on its own sides, as there."""
    from asr_study_amd.core import optimizers
    from oracle import optim as OO
    rs = np.random.RandomState(4)
    x, lens, labels = TG.stack_batch(rs)
    N, T = x.shape[:2]
    assert T % 2 == 1 and len(set(lens)) > 2
    slab = model.to_slab(x)
    stages = TR.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    ctc, logits, sl = model.loss_and_grads(slab, labels, lens, training=True)
    torch.cuda.synchronize()
    sides = _lstm_sides(model, stages, x64, lens, N) if uni else None
    want = TR.loss_and_grads(stages, x64, labels, lens, sides)
    k = int(np.prod(model.time_strides))
    assert logits.shape[0] == want['logits'].shape[0] == -(-T // k)
    assert sl.cpu().numpy().tolist() == want['seq_len'].tolist() == (-(-lens // k)).tolist()
    got_l = logits[:, :N].cpu().numpy()
    e = np.abs(got_l - want['logits']).max()
    print('[treduce] %s logits err %.3e of %.3e' % (tag, e, np.abs(want['logits']).max()))
    assert e <= 1e-4 * (max(1.0, np.abs(want['logits']).max()) if uni else 1.0), (tag, e)
    got_ctc = ctc.cpu().numpy()[:N]
    print('[treduce] %s ctc' % tag, got_ctc, want['ctc'])
    assert np.allclose(got_ctc, want['ctc'], rtol=1e-4, atol=1e-4 if uni else 0.0)
    got = model.get_gradients()
    assert len(got) == len(want['grads']) == len(model.get_weights())
    for i, (g, w) in enumerate(zip(got, want['grads'])):
        err, ref = np.abs(g - w).max(), np.abs(w).max()
        print('[treduce] %s grad %d %s err %.3e of %.3e' % (tag, i, g.shape, err, ref))
        assert ref > 0
        assert err <= (2e-4 * ref if uni else 1e-4 * max(1e-3, ref)) + 1e-6, (tag, i, err, ref)
    lr, clip = (1e-3, 400.0) if uni else (1e-2, 0.5)
    model.compile(optimizer=optimizers.Adam(lr=lr, clipnorm=clip))
    opt = OO.Adam(lr=lr, clipnorm=clip)
    for _ in range(3):
        m = model.train_on_batch([('slab', slab), labels, lens])
        sides = {si: TLU._gpu_gates(model, si, N) for si in _lstm_stages(model)} if uni else None
        out = TR.train_step(stages, x64, labels, lens, opt, sides)
    assert abs(m[1] - float(np.mean(out['ctc']))) < 1e-4 * max(1.0, abs(m[1]))
    for i, (a, b) in enumerate(zip(LU.weights(stages), model.get_weights())):
        err = np.abs(b - a).max()
        assert err < 5e-5 * (max(1.0, np.abs(a).max()) if uni else 1.0), (tag, 'w', i, err)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


@pytest.mark.parametrize('tr', [[[1, 2]], [[0, 3]]], ids=['after1_x2', 'input_x3'])
def test_unidirectional_lstm_vs_oracle(tr):
    from asr_study_amd.core import models
    # (H = 18: one direction's 18 real columns of 20, so the stage runs its scalar path too)
    m = models.brsmv1(num_features=10, num_classes=8, num_hiddens=18, num_layers=2, seed=1,
                      dropout=0.0, bidirectional=False, time_reduction=tr)
    TLU._scale_input_projections(m, (72, 72))
    assert [getattr(m.stages[si], 'directions', 2) for si in _lstm_stages(m)] == [1, 1]
    _ctc_parity(m, 'uni %r' % tr, uni=True)


@pytest.mark.parametrize('residual', [None, 'sum'])
def test_persistent_bilstm_vs_oracle(residual):
    from asr_study_amd.core import models
    m = models.brsmv1(num_features=10, num_classes=8, num_hiddens=16, num_layers=2, seed=2,
                      dropout=0.0, weight_decay=1e-2, residual=residual, time_reduction=[[1, 2]])
    assert all(m._is_bilstm(m.stages[si]) for si in _lstm_stages(m)) and len(_treduce(m)) == 1
    _ctc_parity(m, 'bi residual=%s' % residual, uni=False)


# ---------------------------------------------------------------- GRU, sequence-wise BN
@pytest.mark.parametrize('batch_norm', [False, 'recurrent'], ids=['plain', 'seqbn'])
def test_deep_speech2_gru_vs_oracle(batch_norm):
    """Bounds of tests/test_gpu_gru.py::test_deep_speech2_gru_vs_oracle and
    tests/test_gpu_seqbn.py::test_deep_speech2_recurrent_vs_oracle (_model_parity): logits 1e-4
    max(1, |logits|), CTC rtol = atol = 1e-4, every gradient 2e-4 max|ref| + 1e-6.  With
    batch_norm='recurrent' the second GRU's statistics run over the valid frames of the REDUCED
    axis (ceil(ceil(len / 2) / 2)), the first's over those of the convolutions' axis."""
    from asr_study_amd.core import models
    from tests.test_gpu_seqbn import _randomise_bn
    rs = np.random.RandomState(3)
    # (H = 20: the two concatenated directions must not be padded apart in front of the stage)
    model = models.deep_speech2(num_features=16, num_classes=7, num_hiddens=20, num_layers=2,
                                conv_filters=4, conv_kernels=((5, 7), (3, 5)), seed=1, dropout=0.0,
                                rnn_type='gru', batch_norm=batch_norm, time_reduction=[[1, 2]])
    if batch_norm:
        _randomise_bn(model, rs)
    x, lens, labels = TG.ds2_batch(rs)
    N, T = x.shape[:2]
    assert model.time_strides == [2, 2] and model.out_frames(T) == 10 and (-(-T // 2)) % 2 == 1
    slab = model.to_slab(x)
    stages = TR.ds2_stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    ctc, logits, sl = model.loss_and_grads(slab, labels, lens, training=True)
    torch.cuda.synchronize()
    gru = [si for si, s in enumerate(model.stages) if s.kind == 'bigru']
    if batch_norm:      # the statistics saw the lengths of their own axis
        seen = [model._acts[si]['lens'].cpu().numpy().tolist() for si in gru]
        assert seen == [(-(-lens // 2)).tolist(), (-(-lens // 4)).tolist()]
    _, caches, _ = TR.ds2_forward(stages, x64, lens)
    sides = {}
    for si in gru:
        sides[si] = TG._gpu_gates(model, si, N)
        own = np.stack([c['gates'] for c in caches[si]['cs']], axis=2)
        assert TR_share(own, sides[si], model.stages[si].H) <= 1e-4, si
    want = TR.ds2_loss_and_grads(stages, x64, labels, lens, sides)
    assert logits.shape[0] == 10 and sl.cpu().numpy().tolist() == want['seq_len'].tolist()
    e = np.abs(logits[:, :N].cpu().numpy() - want['logits']).max()
    print('[treduce] ds2 %s logits err %.3e of %.3e' % (batch_norm, e, np.abs(want['logits']).max()))
    assert e <= 1e-4 * max(1.0, np.abs(want['logits']).max())
    assert np.allclose(ctc.cpu().numpy()[:N], want['ctc'], rtol=1e-4, atol=1e-4)
    got = model.get_gradients()
    assert len(got) == len(want['grads'])
    for i, (g, w) in enumerate(zip(got, want['grads'])):
        err = np.abs(g - w).max()
        print('[treduce] ds2 %s grad %d %s err %.3e of %.3e' % (batch_norm, i, g.shape, err,
                                                                np.abs(w).max()))
        assert err <= 2e-4 * np.abs(w).max() + 1e-6, (i, g.shape, err)


def TR_share(own, other, H):
    from tests import gru_oracle as GO
    return GO.side_share(own, other, H)


# ---------------------------------------------------------------- conformer
def test_conformer_utterance_alone_and_among_longer_neighbours():
    """The criterion of tests/test_gpu_conformer.py::test_time_padding_independence: relative
    error below 1e-6 on the utterance's valid logit frames (predict: running moments).  Alone the
    slab has the utterance's 21 frames; in the batch of 3 it has 37, and the frames behind every
    length hold noise: without the stage's own lengths frame 21 would fill the second half of the
    partial group [frame 20 | frame 21], and without the reduced lengths (11 of 19) the attention
    keys and the depthwise convolution would read the groups behind it.
    conv=False, as the model of that test: the front-end's second convolution reads one strided
    frame past an utterance's end, which is not a zero in a longer slab (the first convolution's
    bias and its taps on the last valid frames), so behind the front-end the last frames depend
    on the padding with or without this stage."""
    from asr_study_amd.core import models
    from tests.test_gpu_conformer import _randomise, _rel
    rs = np.random.RandomState(8)
    model = models.conformer(num_features=16, num_classes=7, d_model=32, num_heads=2,
                             num_layers=1, d_ff=64, kernel_size=7, conv_norm='batch', conv=False,
                             dropout=0, seed=3, time_reduction=2, positions='relative')
    _randomise(model, rs)
    model.decoder = None
    assert model.time_strides == [2] and model._needs_lens
    lens = np.array([37, 21, 30])
    x = (100.0 * rs.randn(3, 37, 16)).astype(np.float32)        # noise behind every length
    for n in range(3):
        x[n, :lens[n]] = rs.randn(lens[n], 16) * 2.0 + 1.0
    among = model.predict(x, lens)
    alone = model.predict(x[1:2, :21], lens[1:2])
    assert among.shape == (3, 19, 7) and alone.shape == (1, 11, 7)
    e = _rel(among[1, :11], alone[0])
    print('[treduce] conformer: alone vs among longer neighbours rel %.2e' % e)
    assert np.isfinite(among).all() and np.abs(alone).max() > 0 and e < 1e-6


# ---------------------------------------------------------------- two towers
F, H, D, HEADS, J, C, N, T = 8, 12, 16, 1, 16, 6, 3, 21
LENS = np.array([21, 13, 17])
LABELS = [[0, 3, 3, 1, 4], [2], [4, 0, 1]]
MAX_LABELS = 12


def tiny(kind, seed=0, device=None, **kw):
    from asr_study_amd.core import models
    dev = {} if device is None else {'device': device}
    if kind == 'aed':
        return models.aed(num_features=F, num_classes=C, encoder='blstm', num_hiddens=H,
                          num_layers=2, d_att=D, num_heads=HEADS, pred_hiddens=H, pred_layers=1,
                          dropout=0.0, seed=seed, max_labels=MAX_LABELS, time_reduction=[[1, 2]],
                          **dict(dev, **kw))
    return models.transducer(num_features=F, num_classes=C, encoder='lstm', num_hiddens=H,
                             num_layers=2, joint_dim=J, pred_hiddens=H, pred_layers=1, dropout=0.0,
                             seed=seed, time_reduction=[[1, 2]], **dict(dev, **kw))


def batch(seed=5):
    rs = np.random.RandomState(seed)
    x = (rs.randn(N, T, F) * 1.5).astype(np.float32)
    for n in range(N):
        x[n, LENS[n]:] = 0
    return x


class Oracle(object):
    """The Oracle of tests/test_gpu_aed.py / test_gpu_transducer.py with the encoder tower from
    tests/time_reduction_oracle.py: its output, and the lengths the attention / the lattice take,
    are on the reduced axis."""

    def __init__(self, model, kind):
        self.kind = kind
        self.enc = TR.stages_from_model(model.encoder)
        full = LU.stages_from_model(model.predictor)
        self.pred, self.joint = full[:-1], full[-1]
        self.all = self.enc + full
        self.eps = getattr(model, 'label_smoothing', 0.0)

    def loss_and_grads(self, x64, sides_e=None, sides_p=None):
        labels = np.zeros((N, max(len(l) for l in LABELS)), np.int64)
        for n, l in enumerate(LABELS):
            labels[n, :len(l)] = l
        ll = np.array([len(l) for l in LABELS])
        onehot = RO.onehot_rows(labels, ll, N, N, C - 1).astype(np.float64)
        f, ce, sl = TR.model_forward(self.enc, x64, LENS, sides_e)
        assert f.shape[0] == 11 and sl.tolist() == [11, 7, 9]
        q, cp = LU.model_forward(self.pred, onehot, sides=sides_p)
        W, b = self.joint['W'], self.joint['b']
        if self.kind == 'aed':
            ctx, ca = AO.cross_forward(q, f, HEADS, ll + 1, sl)
            loss, d_pre, dW, db = AO.loss_and_grads(ctx, q, W, b, labels, ll, N, eps=self.eps,
                                                    grad_scale=1.0 / N)
            dq_att, d_enc = AO.cross_backward(d_pre, ca)
            d_pred = d_pre + dq_att
        else:
            loss, d_enc, d_pred, dW, db = RO.loss_and_grads(f, q, W, b, labels, ll, sl, N,
                                                            grad_scale=1.0 / N)
        grads = (TR.model_backward(self.enc, ce, d_enc) +
                 LU.model_backward(self.pred, cp, d_pred) + [dW, db])
        return loss, grads, (ce, cp)

    def gates(self, caches):
        return LU.stage_gates(self.enc, caches[0]), LU.stage_gates(self.pred, caches[1])

    def greedy(self, x64, margins=None):
        f, _, sl = TR.model_forward(self.enc, x64, LENS)
        lstms = [st for st in self.pred if st['type'] == 'lstm']
        dense = [st for st in self.pred if st['type'] == 'dense'][0]
        W, b = self.joint['W'], self.joint['b']

        def run(state, x):
            a, new = np.float64(x)[None], []
            for st, (h0, c0) in zip(lstms, state):
                a, c = LU.lstm_forward(a, st['W'], st['U'], st['b'], act=st['act'], h0=h0, c0=c0)
                new.append((a[0], c['cs'][0]))
            return new, (a @ dense['W'] + dense['b'])[0]

        def init(n):
            zero = [(np.zeros((n, st['U'].shape[0])),) * 2 for st in lstms]
            return run(zero, np.zeros((n, C - 1)))
        if self.kind == 'aed':
            return [AO.greedy_naive(f[:sl[n], n], W, b, HEADS, init, run, MAX_LABELS,
                                    margins=margins) for n in range(N)]
        return [RO.greedy_naive(f[:, n], W, b, int(sl[n]), init, run, 10) for n in range(N)]


def _sides(model, orc, x64):
    _, _, caches = orc.loss_and_grads(x64)
    out = []
    for tower, own in zip((model.encoder, model.predictor), orc.gates(caches)):
        sides = {}
        for si in _lstm_stages(tower):
            sides[si] = TLU._gpu_gates(tower, si, N)
            assert sides[si].shape == own[si].shape
            share = LU.side_share(own[si], sides[si])
            assert share <= 1e-4, (si, share)
        out.append(sides)
    return out


def _x64(model, x):
    return model.to_slab(x)[:, :N].cpu().numpy().astype(np.float64)


@pytest.mark.parametrize('kind', ['aed', 'transducer'])
def test_two_tower_gradient_parity(kind):
    """Bounds of tests/test_gpu_aed.py / tests/test_gpu_transducer.py
    ::test_gradient_parity_with_the_oracle_composition: loss rtol = atol = 1e-4, every gradient
    2e-4 max|ref| + 1e-6.  The encoder output -- the [K | V] slab, the lattice's T -- has
    ceil(21 / 2) frames, and the lengths the loss takes are ceil(len / 2)."""
    model = tiny(kind)
    x = batch()
    slab = model.to_slab(x)
    loss, f, sl = model.loss_and_grads(slab, LABELS, LENS, training=True)
    torch.cuda.synchronize()
    assert f.shape[0] == 11 and f.shape[2] == (2 * D if kind == 'aed' else J)
    assert sl.cpu().numpy().tolist() == [11, 7, 9]
    orc = Oracle(model, kind)
    x64 = _x64(model, x)
    sides_e, sides_p = _sides(model, orc, x64)
    want_loss, want, _ = orc.loss_and_grads(x64, sides_e, sides_p)
    got_loss = loss.cpu().numpy()
    print('[treduce] %s loss' % kind, got_loss, want_loss)
    assert np.allclose(got_loss, want_loss, rtol=1e-4, atol=1e-4)
    got = model.get_gradients()
    assert len(got) == len(want) == len(model.get_weights())
    for i, (g, w) in enumerate(zip(got, want)):
        err = np.abs(g - w).max()
        print('[treduce] %s grad %d %s err %.3e of %.3e' % (kind, i, g.shape, err, np.abs(w).max()))
        assert np.abs(w).max() > 0
        assert err <= 2e-4 * np.abs(w).max() + 1e-6, (i, g.shape, err)


# (chosen on the ORACLE alone: aed seed 10 decodes 12 / 4 / 12 labels of three kinds with a
# smallest margin of 3e-2; transducer seed 3 is tests/test_gpu_transducer.py's)
GREEDY_SEED = {'aed': 10, 'transducer': 3}


def greedy_model(kind, device=None):
    """Weights scaled up as tests/test_gpu_transducer.py does (a fresh model's outputs are flat)."""
    model = tiny(kind, seed=GREEDY_SEED[kind], device=device)
    rs = np.random.RandomState(9 + GREEDY_SEED[kind])
    model.set_weights([w * 3.0 if w.ndim == 2 else (rs.randn(*w.shape) * 0.5).astype(np.float32)
                       for w in model.get_weights()])
    return model


@pytest.mark.parametrize('kind', ['aed', 'transducer'])
def test_two_tower_greedy_decode_equals_the_oracle(kind):
    model = greedy_model(kind)
    x = batch(6)
    margins = []
    want = Oracle(model, kind).greedy(_x64(model, x), margins)
    print('[treduce] %s greedy oracle' % kind, want, margins and min(margins))
    assert sum(len(h) for h in want) >= 3           # (asserted on the ORACLE alone)
    if kind == 'aed':
        assert min(margins) > 1e-3 and any(len(h) < MAX_LABELS for h in want)
    got = model.predict(x, LENS)
    assert got == want
    assert model.predict(x, LENS) == got
    assert model.predict(x[1:2], LENS[1:2]) == got[1:2]     # alone == in the batch


# Measured once on an MI355X with the settings below (tests/test_gpu_aed.py's and
# tests/test_gpu_transducer.py's learning tests on the reduced encoders): greedy predict first
# reproduces all three transcripts after LEARN_STEPS steps; the test allows twice that.
LEARN_STEPS = {'aed': 30, 'transducer': 60}


def learn(kind, limit, seed=1, lr=1e-2):
    from asr_study_amd.core import optimizers
    model = tiny(kind, seed=seed)
    model.compile(optimizer=optimizers.Adam(lr=lr, clipnorm=5.0))
    slab = model.to_slab(batch(7))
    first = last = done = None
    for step in range(limit):
        m = model.train_on_batch([('slab', slab), LABELS, LENS])
        first = m[1] if first is None else first
        last = m[1]
        if step % 5 == 4 and model.predict(('slab', slab), LENS) == LABELS:
            done = step + 1
            break
    return model, slab, done, first, last


@pytest.mark.parametrize('kind', ['aed', 'transducer'])
def test_two_tower_learns_three_utterances(kind):
    limit = 2 * LEARN_STEPS[kind]
    model, slab, done, first, last = learn(kind, limit)
    print('[treduce] %s learned after %s steps, loss %.3f -> %.3f' % (kind, done, first, last))
    assert done is not None, 'not learned within %d steps' % limit
    m = model.test_on_batch([('slab', slab), LABELS, LENS])
    assert m[3] == 0.0 and m[1] < first


# ---------------------------------------------------------------- align, stream
def test_align_reports_the_product_and_stream_refuses():
    from asr_study_amd.core import models
    m = models.deep_speech2(num_features=16, num_classes=7, num_hiddens=16, num_layers=2,
                            conv_filters=4, conv_kernels=((5, 7), (3, 5)), seed=1, dropout=0.0,
                            time_reduction=[[0, 2], [1, 3]])
    rs = np.random.RandomState(2)
    x, lens, _ = TG.ds2_batch(rs)
    labels = [[1], [2], [3, 1], [0], [4]]
    res = m.align(x, labels, lens)
    assert res['time_stride'] == 12 == int(np.prod(m.time_strides))
    red = -(-(-(-(-(-lens // 2)) // 2)) // 3)
    assert red.tolist() == [4, 2, 4, 1, 3]
    for n, a in enumerate(res['alignments']):
        assert len(a['path']) == red[n] and np.isfinite(a['score'])
        assert [s[1] for s in a['segments']] == labels[n]
        assert all(0 <= s[2] < s[3] <= red[n] for s in a['segments']), (n, a['segments'])
    uni = models.brsmv1(num_features=10, num_classes=8, num_hiddens=16, num_layers=2,
                        bidirectional=False, time_reduction=[[1, 2]])
    with pytest.raises(ValueError, match='TimeReduction stage.*one time axis'):
        uni.stream()


# ---------------------------------------------------------------- the command line
def test_cli_train_load_predict(tmp_path):
    """train.py --model brsmv1 --model_params time_reduction "[[1, 2]]" for two epochs on the dummy
    dataset (tests/test_gpu_cli.py), then load_model: the model is rebuilt with the stage, and
    predict.py gives the outputs of Model.predict."""
    sys.path.insert(0, ROOT)
    import train
    import predict as predict_cli
    from asr_study_amd import cli
    from asr_study_amd.datasets import h5lite
    from asr_study_amd.datasets.dataset_generator import DatasetGenerator
    from asr_study_amd.utils import core_utils, generic_utils
    from tests.test_gpu_conformer import _rel
    fname = str(tmp_path / ('dummy.' + ('h5' if h5lite.available() else 'npz')))
    cli.make_dataset_main(['--parser', 'dummy', '--parser_params', 'num_speakers', '4',
                           'num_utterances_per_speaker', '6', 'max_duration', '1.2',
                           'min_duration', '0.6', 'max_label_length', '8', 'split',
                           '[0.5, 0.25]', 'seed', '3', '--input_parser', 'logfbank',
                           '--input_parser_params', 'num_filt', '16', '--output_file', fname])
    out = str(tmp_path / 'run')
    train.main(['--dataset', fname, '--model', 'brsmv1', '--model_params', 'num_features', '16',
                'num_hiddens', '16', 'num_layers', '2', 'num_classes', '28', 'time_reduction',
                '[[1, 2]]', '--num_epochs', '2', '--batch_size', '4', '--save', out, '--seed', '1',
                '--lr', '0.001'])
    best = os.path.join(out, 'best.h5')
    model = core_utils.load_model(best, mode='predict', decoder=False)
    assert model.config['kwargs']['time_reduction'] == [[1, 2]]
    assert [s.time_factor for s in model.stages if hasattr(s, 'time_factor')] == [2]
    assert model.time_strides == [2]
    raw = predict_cli.main(['--model', best, '--dataset', fname, '--no_decoder'])
    decoded = predict_cli.main(['--model', best, '--dataset', fname])
    parser = generic_utils.get_from_module('preprocessing.text', 'simple_char_parser', params=[])
    flow = DatasetGenerator(None, parser, batch_size=1, seed=0, mode='predict',
                            shuffle=False).flow_from_fname(fname, datasets='test')
    assert flow.len == len(raw) == len(decoded) > 0
    for r, d in zip(raw, decoded):
        x, lens = flow.next()
        Tn = int(np.asarray(lens).reshape(-1)[0])
        x = np.asarray(x, np.float32)[:, :Tn]
        want = model.predict(x, [Tn])[0]
        assert want.shape[0] == -(-Tn // 2)
        assert r['best'].shape == want.shape and _rel(r['best'], want) < 1e-4, Tn
        assert isinstance(d['best'], str)
