"""-m gpu: the unidirectional GRU (K28: the one-direction form of csrc/gru.hip with a carried
state) against the float64 oracle (tests/gru_uni_oracle.py), bit for bit against direction 0 of
the bidirectional kernels and against itself cut in two calls, then bare-GRU models in training
and in streaming sessions, and the command line round trip."""
import numpy as np
import pytest
import torch

from tests import gru_oracle as GO
from tests import gru_uni_oracle as GU
from tests import test_gpu_gru as TG

pytestmark = pytest.mark.gpu
ACTS, _dev, _f32, _close = TG.ACTS, TG._dev, TG._f32, TG._close

# (H, n_pad, T): T = 1 and 2 (prologue only, no frame two back), NR = 16 / 32 / 64, part-filled
# last column tiles (36, 100, 132, 260), BPTT phase B's K = 2 * 132 across the 256 chunk edge, two
# forward chunks (260, 512)
SHAPES = [(4, 16, 1), (4, 16, 2), (36, 16, 9), (36, 32, 7), (132, 48, 3), (260, 32, 5),
          (100, 64, 6), (512, 16, 4)]
BIT_SHAPES = [(36, 32, 7), (132, 48, 3), (100, 64, 6)]


def uni_case(H, n_pad, T, k, state):
    """Direction 0 of tests/test_gpu_gru.kernel_case (four activations, masks on odd k), and the
    initial state: None, or 0.5 randn on the real columns (float32-representable)."""
    c = TG.kernel_case(H, n_pad, T, k)
    Hp = c['Hp']
    dy = c['dy'] if c['merge'] == 'sum' else c['dy'].reshape(T, n_pad, 2, Hp)[:, :, 0]
    h0 = None
    if state:
        rs = np.random.RandomState(77 + 1000 * k + H + n_pad + T)
        h0 = np.zeros((n_pad, Hp))
        h0[:, :H] = 0.5 * rs.randn(n_pad, H)
        h0 = _f32(h0)
    return dict(act=c['act'], Hp=Hp, U=np.ascontiguousarray(c['U'][0]),
                zx=np.ascontiguousarray(c['zx'][:, :, 0]),
                BU=None if c['BU'] is None else np.ascontiguousarray(c['BU'][0]),
                dy=np.ascontiguousarray(dy), h0=h0, full=c)


def _zeros(*shape):
    return torch.zeros(*shape, device='cuda:0')


def _fwd(c, T, n_pad, zx=None, h0=None, want_last=True):
    """One asr_gru_uni_seq_fwd call on device copies -> h, gates, rm, h_last (numpy)."""
    from asr_study_amd import ops
    Hp = c['Hp']
    zx = c['zx'] if zx is None else zx
    h, gates, rm = _zeros(T, n_pad, Hp), _zeros(T, n_pad, 3 * Hp), _zeros(T, n_pad, Hp)
    last = torch.full((n_pad, Hp), float('nan'), device='cuda:0') if want_last else None
    ops.gru_uni_seq_fwd(_dev(zx), _dev(c['U']), h, gates, rm, T, n_pad, Hp, act=c['act'],
                        mask_u=None if c['BU'] is None else _dev(c['BU']),
                        h0=None if h0 is None else _dev(h0), h_last=last)
    return [t.cpu().numpy() for t in (h, gates, rm)] + [None if last is None else
                                                        last.cpu().numpy()]


@pytest.mark.parametrize('state', [False, True], ids=['zero', 'state'])
@pytest.mark.parametrize('H,n_pad,T', SHAPES)
def test_kernel_parity(H, n_pad, T, state):
    """h, gates, rm, h_last, then da, db_part, dz_absmax against the oracle, to the bound of
    tests/test_gpu_gru.py (_close: 1e-4 max(1e-3, max |want|); the same arithmetic and tile)."""
    from asr_study_amd import ops
    for k in range(len(ACTS)):
        c = uni_case(H, n_pad, T, k, state)
        act, Hp, U, zx, BU, dy, h0 = (c[n] for n in ('act', 'Hp', 'U', 'zx', 'BU', 'dy', 'h0'))
        want_h, want_g = GU.recurrence_forward(zx, U, act, BU, h0)
        share = TG.saturated_share(want_g, H, Hp)
        print('[gru_uni] H=%d n_pad=%d T=%d %s: saturated share %.3f' % (H, n_pad, T, act, share))
        assert 0.05 <= share <= 0.5, share
        h, gates, rm, last = _fwd(c, T, n_pad, h0=h0)
        tag = 'H=%d n_pad=%d %s ' % (H, n_pad, act)
        _close(h, want_h, tag + 'h')
        _close(gates, want_g, tag + 'gates')
        _close(rm, GU.rm_of(want_h, want_g, BU, h0), tag + 'rm')
        _close(last, want_h[-1], tag + 'h_last')
        # BPTT (from the zero state) reads the oracle's h and gates rounded to float32, and so
        # does the oracle's backward, as in tests/test_gpu_gru.py
        h32, g32 = _f32(want_h), _f32(want_g)
        want_da = GU.recurrence_backward(dy, U, h32, g32, act, BU)
        da = _zeros(T, n_pad, 3 * Hp)
        dbp, zmx = _zeros(n_pad // 16, 3 * Hp), _zeros(1)
        ops.gru_uni_seq_bwd(_dev(dy), _dev(U), _dev(h32), _dev(g32), da, T, n_pad, Hp, act=act,
                            mask_u=None if BU is None else _dev(BU), db_part=dbp, dz_absmax=zmx)
        _close(da.cpu().numpy(), want_da, tag + 'da')
        ref = max(1e-3, np.abs(want_da).max())
        want_db = want_da.reshape(T, n_pad // 16, 16, 3 * Hp).sum(axis=(0, 2))
        _close(dbp.cpu().numpy(), want_db, tag + 'db_part')
        assert abs(float(zmx.item()) - np.abs(want_da).max()) <= 1e-4 * ref


@pytest.mark.parametrize('H,n_pad,T', BIT_SHAPES)
def test_zero_state_is_direction_0_of_the_bidirectional_kernels_bit_for_bit(H, n_pad, T):
    """h0 = null: every output equals direction 0 of asr_gru_seq_fwd / _bwd on operands whose
    direction 1 is random (the same tile plan, chunk order and cross-wave sum)."""
    from asr_study_amd import ops
    for k in range(len(ACTS)):
        c = uni_case(H, n_pad, T, k, False)
        f, Hp, act = c['full'], c['Hp'], c['act']
        shared = f['merge'] == 'sum'
        Ud2, BUd2 = _dev(f['U']), (None if f['BU'] is None else _dev(f['BU']))
        h2, g2 = _zeros(T, n_pad, 2, Hp), _zeros(T, n_pad, 2, 3 * Hp)
        rm2 = _zeros(T, n_pad, 2, Hp)
        ops.gru_seq_fwd(_dev(f['zx']), Ud2, h2, g2, rm2, T, n_pad, Hp, act=act, mask_u=BUd2)
        da2, dbp2 = _zeros(T, n_pad, 2, 3 * Hp), _zeros(n_pad // 16, 2, 3 * Hp)
        dyd = _dev(f['dy'])
        ops.gru_seq_bwd(dyd, Ud2, h2, g2, da2, T, n_pad, Hp, act=act, mask_u=BUd2,
                        shared_dy=shared, db_part=dbp2, dz_absmax=_zeros(1))
        h, gates, rm, last = _fwd(c, T, n_pad)
        assert np.array_equal(h, h2[:, :, 0].cpu().numpy())
        assert np.array_equal(gates, g2[:, :, 0].cpu().numpy())
        assert np.array_equal(rm, rm2[:, :, 0].cpu().numpy())
        assert np.array_equal(last, h[-1])
        # BPTT on the kernels' own h and gates; dy is the bidirectional call's tensor, read at
        # its row stride (direction 0 lies first in a 'concat' row)
        BUd = None if c['BU'] is None else _dev(c['BU'])
        da, dbp, zmx = _zeros(T, n_pad, 3 * Hp), _zeros(n_pad // 16, 3 * Hp), _zeros(1)
        ops.gru_uni_seq_bwd(dyd, _dev(c['U']), _dev(h), _dev(gates), da, T, n_pad, Hp, act=act,
                            mask_u=BUd, dy_ld=Hp if shared else 2 * Hp, db_part=dbp,
                            dz_absmax=zmx)
        want_da = da2[:, :, 0].cpu().numpy()
        assert np.isfinite(want_da).all() and np.abs(want_da).max() > 0
        assert np.array_equal(da.cpu().numpy(), want_da)
        assert np.array_equal(dbp.cpu().numpy(), dbp2[:, 0].cpu().numpy())
        assert float(zmx.item()) == float(np.abs(want_da).max())


@pytest.mark.parametrize('state', [False, True], ids=['zero', 'state'])
@pytest.mark.parametrize('H,n_pad,T', [s for s in SHAPES if s[2] >= 2])
def test_a_sequence_cut_in_two_calls_is_the_one_call_bit_for_bit(H, n_pad, T, state):
    """[0, k) then [k, T) with h0 = the first call's h_last, k = 1, a middle value and T - 1: the
    h, gates and rm of the one call over T frames; a repeated call gives the same bits."""
    for ki in range(len(ACTS)):
        c = uni_case(H, n_pad, T, ki, state)
        whole = _fwd(c, T, n_pad, h0=c['h0'])
        again = _fwd(c, T, n_pad, h0=c['h0'])
        assert all(np.isfinite(a).all() and np.array_equal(a, b) for a, b in zip(whole, again))
        for cut in sorted({1, T // 2, T - 1} - {0}):
            a = _fwd(c, cut, n_pad, zx=c['zx'][:cut], h0=c['h0'])
            b = _fwd(c, T - cut, n_pad, zx=c['zx'][cut:], h0=a[3])
            assert np.array_equal(a[3], whole[0][cut - 1])
            for i, what in enumerate(('h', 'gates', 'rm')):
                assert np.array_equal(np.concatenate([a[i], b[i]]), whole[i]), (what, cut)
            assert np.array_equal(b[3], whole[3])
        # without h_last nothing else changes
        assert np.array_equal(_fwd(c, T, n_pad, h0=c['h0'], want_last=False)[0], whole[0])


# ---------------------------------------------------------------- models
def uni_stack(seed=2, dropout=0.0, device=None, mixed=False):
    """GRU(10, tanh) -> GRU(14, relu) -> Dense(8) built by hand (H not a multiple of 4); mixed: a
    Dense(12) and a causal DepthwiseConvolution1D(3) in front."""
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import ctc_model
    x_in = L.Input(name='inputs', shape=(None, 10))
    o = x_in
    if mixed:
        o = L.TimeDistributed(L.Dense(12))(o)
        o = L.DepthwiseConvolution1D(3, causal=True)(o)
    o = L.GRU(10, activation='tanh', dropout_W=dropout, dropout_U=dropout,
              W_regularizer=L.l2(1e-4))(o)
    o = L.GRU(14, activation='relu', dropout_W=dropout, dropout_U=dropout,
              U_regularizer=L.l2(1e-4))(o)
    o = L.TimeDistributed(L.Dense(8))(o)
    model = ctc_model(x_in, o, seed=seed, **({} if device is None else {'device': device}))
    # spread the gate pre-activations so that both slope branches occur, as tests/test_gpu_gru.py
    # does -- but through the two input projections W alone.  Scaling U as well (orthogonal x
    # 1.1 x 2.5) makes the relu layer, which here has no second direction summed to it, grow over
    # the 33 frames until the test measures conditioning: with the masks of the parity case the
    # float64 oracle's own loss after three Adam steps moves by 1.6e-4 (relative) when nothing
    # but its weights are rounded to float32 after each step (max |gradient| 1.9e4), more than
    # the bound any float32 model is held to.  With W alone that figure is 4.6e-8 / 6.2e-8
    # (plain / masks, max |gradient| 4.0 / 6.4).
    w = model.get_weights()
    scaled = [i for i, a in enumerate(w) if a.ndim == 2 and a.shape[1] in (30, 42)][::2]
    assert [w[i].shape for i in scaled] == [(w[scaled[0]].shape[0], 30), (10, 42)]
    model.set_weights([a * 2.5 if i in scaled else a for i, a in enumerate(w)])
    return model


def uni_ds2(dropout=0.0, device=None, seed=1):
    from asr_study_amd.core import models
    kw = {} if device is None else {'device': device}
    return models.deep_speech2(num_features=16, num_classes=7, num_hiddens=18, num_layers=2,
                               conv_filters=4, conv_kernels=((5, 7), (3, 5)), seed=seed,
                               dropout=dropout, rnn_type='gru', bidirectional=False, **kw)


def model_case(name, masks_on, device=None):
    """(model, x, lens, labels, rs) of a parity case: the batches of tests/test_gpu_gru.py."""
    dropout = 0.2 if masks_on else 0.0
    if name == 'stack':
        rs = np.random.RandomState(4)
        return (uni_stack(dropout=dropout, device=device),) + TG.stack_batch(rs) + (rs,)
    rs = np.random.RandomState(3)
    return (uni_ds2(dropout, device=device),) + TG.ds2_batch(rs) + (rs,)


def draw_masks(model, n_pad, rs):
    """The pair of masks a 'bigru' stage is given, per GRU stage; the one-direction stage reads
    direction 0 of each."""
    out = {}
    for si, s in enumerate(model.stages):
        if s.kind == 'bigru':
            BW = ((rs.rand(2, n_pad, s.f_in_pad) > 0.2) / 0.8).astype(np.float32)
            BU = ((rs.rand(2, n_pad, s.Hp) > 0.2) / 0.8).astype(np.float32)
            out[si] = (BW, BU)
    return out


def oracle_masks(model, masks, N):
    """... cut to direction 0, the real rows and columns."""
    return {si: (BW[0, :N][:, model._real_rows(model.stages[si])].astype(np.float64),
                 BU[0, :N, :model.stages[si].H].astype(np.float64))
            for si, (BW, BU) in masks.items()}


def _gpu_gates(model, si, N):
    s = model.stages[si]
    g = model._acts[si]['gates'][:, :N].cpu().numpy().astype(np.float64)
    T = g.shape[0]
    return np.ascontiguousarray(g.reshape(T, N, 3, s.Hp)[..., :s.H]).reshape(T, N, 3 * s.H)


def _gru_stages(model):
    return [si for si, s in enumerate(model.stages) if s.kind == 'bigru']


@pytest.mark.parametrize('masks_on', [False, True], ids=['plain', 'masks'])
@pytest.mark.parametrize('name', ['stack', 'ds2'])
def test_models_vs_oracle(name, masks_on):
    """The procedure and bounds of tests/test_gpu_gru.py's _model_parity: logits to 1e-4 max(1,
    |logits|), CTC to rtol = atol = 1e-4, every gradient to 2e-4 max|ref| + 1e-6 (no entry left
    out), the weights after three Adam steps to 5e-5 max(1, |w|).  Each side runs its own forward;
    the oracle's backward takes the saturation side of every gate entry from the GPU's saved
    gates, under the 1e-4 cap on the share that differs.  That cap is a condition on the inputs:
    the oracle run in float32 against itself in float64 on these four cases (CPU, before the
    first GPU run) differed on a share of 0 in every stage -- stack: 3960 and 5544 z and r
    entries per stage (plain: 29.8 % and 1.5 % of them saturated; masks: 30.9 % and 2.6 %);
    deep_speech2: 3420 entries per stage (0.1 % and 0.0 % saturated, plain and with masks)."""
    from asr_study_amd.core import optimizers
    from oracle import optim as OO
    model, x, lens, labels, rs = model_case(name, masks_on)
    assert [getattr(model.stages[si], 'directions', 2) for si in _gru_stages(model)] == [1, 1]
    N = x.shape[0]
    slab = model.to_slab(x)
    n_pad = slab.shape[1]
    stages = GU.stages_from_model(model)
    x64 = slab[:, :N].cpu().numpy().astype(np.float64)
    masks = draw_masks(model, n_pad, rs) if masks_on else {}
    masks_g = {si: (_dev(BW), _dev(BU)) for si, (BW, BU) in masks.items()} or None
    masks_o = oracle_masks(model, masks, N)
    ctc, logits, _ = model.loss_and_grads(slab, labels, lens, training=True, masks=masks_g)
    torch.cuda.synchronize()
    for si in _gru_stages(model):       # the stage ran under the masks it was given
        assert (model._acts[si].get('BW') is not None) == masks_on
    _, caches = GU.model_forward(stages, x64, masks_o)
    sides = {}
    for si in _gru_stages(model):
        sides[si] = _gpu_gates(model, si, N)
        share = GO.side_share(caches[si]['gates'], sides[si], model.stages[si].H)
        print('[gru_uni] %s stage %d: share of gate entries on another side than the oracle %.2e'
              % (name, si, share))
        assert share <= 1e-4, (si, share)
    want = GU.loss_and_grads(stages, x64, labels, lens, masks_o, sides)
    got_l = logits[:, :N].cpu().numpy()
    e = np.abs(got_l - want['logits']).max()
    print('[gru_uni] %s logits err %.3e of %.3e' % (name, e, np.abs(want['logits']).max()))
    assert e <= 1e-4 * max(1.0, np.abs(want['logits']).max()), (name, 'logits', e)
    got_ctc = ctc.cpu().numpy()[:N]
    assert np.allclose(got_ctc, want['ctc'], rtol=1e-4, atol=1e-4), (got_ctc, want['ctc'])
    got = model.get_gradients()
    assert len(got) == len(want['grads'])
    for i, (g, w) in enumerate(zip(got, want['grads'])):
        err = np.abs(g - w).max()
        print('[gru_uni] %s grad %d %s err %.3e of %.3e' % (name, i, g.shape, err,
                                                            np.abs(w).max()))
        assert err <= 2e-4 * np.abs(w).max() + 1e-6, (name, i, g.shape, err, np.abs(w).max())
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    opt = OO.Adam(lr=1e-3, clipnorm=400.0)
    for _ in range(3):
        m = model.train_on_batch([('slab', slab), labels, lens], masks=masks_g)
        sides = {si: _gpu_gates(model, si, N) for si in _gru_stages(model)}
        out = GU.train_step(stages, x64, labels, lens, opt, masks_o, sides)
    assert abs(m[1] - float(np.mean(out['ctc']))) < 1e-4 * abs(m[1])
    for k, (a, b) in enumerate(zip(GU.weights(stages), model.get_weights())):
        err = np.abs(b - a).max()
        assert err < 5e-5 * max(1.0, np.abs(a).max()), (name, 'w', k, err)
    assert model.fallbacks == 0 and model.vetoed_steps == 0


# ---------------------------------------------------------------- sessions
LENS = np.array([37, 20, 9])
PIECES = [1, 7, 13, 3, 13]
_REF = {}


def _rel(got, want):
    """max |got - want| in units of the model bound's scale, max(1, |want|)."""
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def session_case(name):
    """(model, x (3, 37, F), the slab the session equals, float64 logits of that slab, strided
    lengths), made once per model: 3 streams of 37, 20 and 9 frames.  Under the front-end the odd
    37 frames get the one zero frame finish() appends."""
    if name not in _REF:
        rs = np.random.RandomState({'stack': 31, 'ds2': 32, 'mixed': 33}[name])
        model = uni_ds2() if name == 'ds2' else uni_stack(mixed=name == 'mixed')
        F = model.num_features
        x = (rs.randn(3, 37, F) * 2.0 + (1.0 if name == 'ds2' else 0.0)).astype(np.float32)
        for n in range(3):
            x[n, LENS[n]:] = 0
        whole = x if name != 'ds2' else np.concatenate([x, np.zeros((3, 1, F), np.float32)], 1)
        x64 = model.to_slab(whole)[:, :3].cpu().numpy().astype(np.float64)
        out_lens = model.out_lengths(LENS)
        want, _ = GU.model_forward(GU.stages_from_model(model), x64, lens=out_lens)
        model.decoder = None
        _REF[name] = (model, x, whole, want, out_lens)
    return _REF[name]


def _feed_all(ss, x, pieces=PIECES):
    """x (N, T, F) in ragged pieces; a stream's length is told with the piece that carries its
    last frame.  -> the results of every feed and of finish."""
    outs, pos = [], 0
    for p in pieces:
        ended = [int(l) if pos < l <= pos + p else None for l in LENS]
        outs.append(ss.feed(x[:, pos:pos + p], ended))
        pos += p
    outs.append(ss.finish())
    return outs


@pytest.mark.parametrize('step', [1, 3, 16])
@pytest.mark.parametrize('name', ['stack', 'ds2', 'mixed'])
def test_sessions_vs_oracle(name, step):
    """Streamed logits of every valid frame against the float64 oracle of the whole utterance,
    and Model.predict's on the same input, both to 1e-4 max(1, |logits|) (the model bound of
    tests/test_gpu_stream.py); reset() and the same stream again: the bits of a fresh session."""
    model, x, whole, want, out_lens = session_case(name)
    model.decoder = None
    pred = model.predict(whole, LENS)
    ss = model.stream(n_streams=3, step=step)
    assert ss.step == step and (ss.schedule.front is not None) == (name == 'ds2')
    got = np.concatenate(_feed_all(ss, x), 1)
    assert got.shape == pred.shape == (3,) + want.shape[::2], (got.shape, pred.shape, want.shape)
    assert ss.frames_in == 37 and ss.frames_out == got.shape[1]
    e = max(_rel(got[n, :out_lens[n]], want[:out_lens[n], n]) for n in range(3))
    ep = max(_rel(pred[n, :out_lens[n]], want[:out_lens[n], n]) for n in range(3))
    print('[gru_uni] %s step %d: streamed logits vs float64 oracle %.3e, Model.predict %.3e'
          % (name, step, e, ep))
    assert e < 1e-4 and ep < 1e-4, (name, step, e, ep)
    state = [st['h'] for st in ss.state.values() if 'h' in st]
    assert len(state) == 2 and all(len(pair) == 2 for pair in state)
    ss.reset()
    assert ss.frames_in == ss.frames_out == 0
    assert all(float(t.abs().max()) == 0.0 for pair in state for t in pair)
    again = np.concatenate(_feed_all(ss, x), 1)
    assert np.array_equal(again, got)
    fresh = np.concatenate(_feed_all(model.stream(n_streams=3, step=step), x), 1)
    assert np.array_equal(fresh, got)


@pytest.mark.parametrize('name', ['stack', 'ds2'])
def test_session_with_a_greedy_decoder_returns_the_labels_of_predict(name):
    model, x, whole, want, out_lens = session_case(name)
    try:
        model.decoder = {'is_greedy': True}
        labels = model.predict(whole, LENS)
        outs = _feed_all(model.stream(n_streams=3, step=3), x)
        assert [sum((o[n] for o in outs), []) for n in range(3)] == labels
        assert all(isinstance(l, list) for l in labels) and any(labels)
    finally:
        model.decoder = None


def test_a_bidirectional_model_is_still_refused():
    with pytest.raises(ValueError) as e:
        TG.ds2_gru(False, 0.0).stream()
    assert 'a bigru stage reads the whole utterance' in str(e.value)


# ---------------------------------------------------------------- the command line
def test_cli_train_then_predict_stream(tmp_path):
    """train.py --model deep_speech2 --model_params rnn_type gru bidirectional False, then
    predict.py --stream 80 on the checkpoint with no further option: every streamed output against
    Model.predict on the utterance's even slab (the model bound), and greedy strings."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import train
    import predict as predict_cli
    from asr_study_amd import cli
    from asr_study_amd.datasets import h5lite
    from asr_study_amd.datasets.dataset_generator import DatasetGenerator
    from asr_study_amd.utils import core_utils, generic_utils
    fname = str(tmp_path / ('dummy.' + ('h5' if h5lite.available() else 'npz')))
    cli.make_dataset_main(['--parser', 'dummy', '--parser_params', 'num_speakers', '4',
                           'num_utterances_per_speaker', '6', 'max_duration', '1.2',
                           'min_duration', '0.6', 'max_label_length', '8', 'split',
                           '[0.5, 0.25]', 'seed', '3', '--input_parser', 'logfbank',
                           '--input_parser_params', 'num_filt', '16', '--output_file', fname])
    out = str(tmp_path / 'run')
    train.main(['--dataset', fname, '--model', 'deep_speech2', '--model_params', 'num_features',
                '16', 'num_hiddens', '18', 'num_layers', '2', 'num_classes', '28',
                'conv_filters', '4', 'conv_kernels', '[[5,7],[3,5]]', 'rnn_type', 'gru',
                'bidirectional', 'False', '--num_epochs', '1', '--batch_size', '4', '--save', out,
                '--seed', '1', '--lr', '0.001'])
    best = os.path.join(out, 'best.h5')
    model = core_utils.load_model(best, mode='predict', decoder=False)
    assert model.config['kwargs']['bidirectional'] is False
    assert [getattr(s, 'directions', 2) for s in model.stages if s.kind == 'bigru'] == [1, 1]
    raw = predict_cli.main(['--model', best, '--dataset', fname, '--no_decoder', '--stream', '80'])
    streamed = predict_cli.main(['--model', best, '--dataset', fname, '--stream', '80'])
    parser = generic_utils.get_from_module('preprocessing.text', 'simple_char_parser', params=[])
    flow = DatasetGenerator(None, parser, batch_size=1, seed=0, mode='predict',
                            shuffle=False).flow_from_fname(fname, datasets='test')
    assert flow.len == len(raw) == len(streamed) > 0
    for r, s in zip(raw, streamed):
        x, lens = flow.next()
        T = int(np.asarray(lens).reshape(-1)[0])
        x = np.asarray(x, np.float32)[:, :T]
        if T % 2:       # the session appends one zero frame under the front-end
            x = np.concatenate([x, np.zeros((1, 1, x.shape[2]), np.float32)], 1)
        want = model.predict(x, [T])[0]
        assert r['best'].shape == want.shape and _rel(r['best'], want) < 1e-4, T
        assert isinstance(s['best'], str)
