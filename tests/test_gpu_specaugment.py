"""GPU checks of SpecAugment (csrc/specaug.hip) against tests/specaugment_oracle.py:
the masks bit for bit and the draws as integers, the warp within 1e-6 max|x| of float64, select
semantics under non-finite input, what must be copied bit for bit, determinism, the engine's
stage (training against the oracle-augmented slab, inference as the identity, ragged input
lengths) and the command line."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import specaugment_oracle as SO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _slab(rs, T, n_pad, ld):
    return rs.randn(T, n_pad, ld).astype(np.float32)


def _run(x, N, F, lens, seed, stream_id, step, pol, params=True):
    """The kernel on the host slab x -> (out, params_out) as NumPy arrays; out starts from a
    sentinel, so an element the kernel does not write shows."""
    from asr_study_amd import ops
    xd = torch.from_numpy(x).cuda()
    out = torch.full_like(xd, SENTINEL)
    ld = None if lens is None else torch.tensor(list(lens), dtype=torch.int32, device='cuda')
    po = None
    if params:
        po = torch.full((max(N, 1), ops.specaug_params_len(pol['freq_masks'], pol['time_masks'])),
                        -7, dtype=torch.int32, device='cuda')
    ops.specaug_apply(xd, out, N, F, seed, stream_id, step, lens=ld, params_out=po, **pol)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))      # in untouched
    return out.cpu().numpy(), None if po is None else po.cpu().numpy()[:N]


def _check(x, N, F, lens, seed, stream_id, step, pol, tag):
    """out against the oracle: masked elements bit-equal mask_value, warped ones within
    1e-6 max|x| of float64, everything else bit-equal to x; params_out exact."""
    got, par = _run(x, N, F, lens, seed, stream_id, step, pol)
    want, masked, rows, warped = SO.apply(x, N, F, lens, seed, stream_id, step, **pol)
    assert np.array_equal(par, rows), tag
    mv = np.float32(pol['mask_value'])
    assert np.array_equal(_bits(got[masked]), _bits(np.full(int(masked.sum()), mv))), tag
    plain = ~masked & ~warped
    assert np.array_equal(_bits(got[plain]), _bits(x[plain])), tag
    w = warped & ~masked
    err = 0.0
    if w.any():
        scale = np.abs(x[:, :N, :F][np.isfinite(x[:, :N, :F])]).max()
        err = np.abs(got[w].astype(np.float64) - want[w]).max() / scale
        print('[specaug] %s warp: %d elements, max err %.3e of max|x|' % (tag, int(w.sum()), err))
        assert err <= 1e-6, tag
    return got, rows, masked, warped


MASK_CASES = {
    # (T, N, n_pad, F, ld), lens, policy
    'ragged': ((40, 5, 16, 36, 40), [1, 40, 17, 33, 8], dict(time_ratio=0.2)),
    'nolens': ((131, 3, 16, 80, 80), None, dict()),                 # the layer's defaults
    'tiny': ((1, 1, 16, 4, 4), [1], dict(time_ratio=1.0)),
    'T63': ((63, 3, 16, 8, 8), [63, 62, 9], dict(time_ratio=0.3, freq_width=3)),
    'T64': ((64, 3, 16, 8, 8), [64, 63, 9], dict(time_ratio=0.3, freq_width=3)),
    'T65': ((65, 3, 16, 8, 8), [65, 64, 9], dict(time_ratio=0.3, freq_width=3)),
    'odd_count': ((40, 5, 16, 36, 40), [40, 1, 17, 33, 8],
                  dict(freq_masks=1, time_masks=2, time_ratio=0.4)),
    'Fw_gt_F': ((40, 5, 16, 36, 40), [40, 1, 17, 33, 8], dict(freq_width=100, time_ratio=0.2)),
    'Tw_gt_len': ((40, 5, 16, 36, 40), [40, 1, 17, 33, 8], dict(time_width=1000, time_ratio=1.0)),
    'max_masks': ((40, 5, 16, 36, 40), [40, 1, 17, 33, 8],
                  dict(freq_masks=31, freq_width=2, time_masks=33, time_width=2, time_ratio=1.0)),
    # the other paths: F and ld no multiples of 4 (scalar accesses), F < ld with a straddled
    # 16-byte group, a row count that is no multiple of the tile, lengths 0 and beyond T
    'scalar_ld': ((20, 3, 16, 13, 13), [20, 7, 13], dict(freq_width=5, time_ratio=0.3)),
    'F39_ld40': ((20, 9, 16, 39, 40), [20, 7, 13, 1, 2, 20, 19, 3, 11],
                 dict(freq_width=8, time_ratio=0.3)),
    'n_pad5': ((9, 3, 5, 6, 7), [9, 0, 15], dict(freq_width=3, time_ratio=0.5)),
    'N0': ((9, 0, 16, 8, 8), [], dict(time_ratio=0.5)),
    # the frequency masks are a bitmap of the columns up to F = 1024 and walked per element beyond
    'F1024': ((9, 3, 16, 1024, 1024), [9, 4, 1], dict(freq_masks=5, freq_width=700)),
    'F1028': ((9, 3, 16, 1028, 1032), [9, 4, 1], dict(freq_masks=5, freq_width=700)),
    'F33_scalar': ((9, 3, 16, 33, 35), [9, 4, 1], dict(freq_masks=3, freq_width=33)),
    'N_eq_n_pad': ((17, 16, 16, 8, 8), list(range(2, 18)), dict(freq_width=4, time_ratio=0.5)),
}


@pytest.mark.parametrize('case', sorted(MASK_CASES))
def test_masks_only_are_bit_exact(case):
    (T, N, n_pad, F, ld), lens, pol = MASK_CASES[case]
    pol = SO.policy(time_warp=0, **pol)
    rs = np.random.RandomState(len(case))
    x = _slab(rs, T, n_pad, ld)
    got, rows, masked, warped = _check(x, N, F, lens, 1234567890123, 8, 5, pol, case)
    assert not warped.any() and (N == 0 or (rows[:, :2] == -1).all())
    want = x.copy()
    want[masked] = np.float32(pol['mask_value'])
    assert np.array_equal(_bits(got), _bits(want))                  # the whole slab, bit for bit
    if case in ('ragged', 'nolens', 'Tw_gt_len', 'max_masks'):
        assert masked.any()                                         # the policy bites


WARP_LENS = [50, 11, 2, 1, 30, 11]


@pytest.mark.parametrize('seed,pol,draws', [
    (80, dict(), [[10, 6], [5, 0], [-1, -1], [-1, -1], [11, 12], [5, 10]]),
    (274, dict(freq_masks=0, time_masks=0), [[6, 6], [5, 0], [-1, -1], [-1, -1], [19, 17], [5, 10]]),
], ids=['with_masks', 'warp_alone'])
def test_warp_against_float64(seed, pol, draws):
    """W = 5: utterances of len = 2 W + 1 (one possible centre) and len <= 2 (never warped).  The
    seeds were found with the oracle (the block layout depends on the mask count, so each policy
    has its own): they draw c' = 0 for sample 1 and c' = len - 1 for sample 5."""
    pol = SO.policy(**dict(dict(time_warp=5, freq_masks=2, freq_width=9, time_masks=3,
                                time_ratio=0.3), **pol))
    rs = np.random.RandomState(7)
    x = _slab(rs, 50, 16, 40) * 3.0
    got, rows, masked, warped = _check(x, 6, 36, WARP_LENS, seed, 8, 3, pol, 'warp')
    assert rows[:, :2].tolist() == draws
    assert warped[:, 0].any() and not warped[:, 2:4].any()
    if not pol['freq_masks']:
        # c' = 0: frame 0 reads frame c; c' = len - 1: the last frame reads frame c; c' = c (no
        # displacement): the identity, still through the interpolation
        assert np.array_equal(_bits(got[0, 1, :36]), _bits(x[5, 1, :36]))
        assert np.array_equal(_bits(got[10, 5, :36]), _bits(x[5, 5, :36]))
        assert np.array_equal(_bits(got[17, 4, :36]), _bits(x[19, 4, :36]))  # frame c' = frame c
        assert np.array_equal(got[:50, 0, :36], x[:50, 0, :36])


def test_warp_wider_than_every_utterance_and_a_long_slab():
    """W far above the lengths (Wn = (len - 1) / 2) at T = 300, several time tiles, NULL lens."""
    rs = np.random.RandomState(9)
    x = _slab(rs, 300, 16, 8)
    pol = SO.policy(time_warp=100000, freq_masks=1, freq_width=3, time_masks=2, time_ratio=0.1)
    _, rows, _, warped = _check(x, 10, 8, None, 99, 0, 1, pol, 'wide-null')
    assert (rows[:, 0] >= 0).all() and warped.any()
    _check(x, 10, 8, [300, 3, 4, 5, 299, 150, 2, 77, 1, 0], 99, 0, 1, pol, 'wide-ragged')


@pytest.mark.parametrize('W', [0, 4])
def test_a_mask_is_a_select_and_the_rest_is_copied(W):
    """NaN and +-inf under every mask come out as mask_value; out beyond len, in rows n >= N and
    in columns >= F equals in bit for bit, junk included."""
    T, N, n_pad, F, ld = 40, 5, 16, 36, 40
    lens = [40, 1, 17, 33, 8]
    pol = SO.policy(time_warp=W, freq_masks=2, freq_width=9, time_masks=3, time_ratio=0.3,
                    mask_value=-1.5)
    rs = np.random.RandomState(3)
    x = _slab(rs, T, n_pad, ld)
    _, masked, _, _ = SO.apply(x, N, F, lens, 31, 4, 2, **pol)
    assert masked.sum() > 100
    junk = np.array([np.nan, np.inf, -np.inf, 3e38, -0.0], np.float32)
    if W == 0:
        x[masked] = junk[np.arange(int(masked.sum())) % 3]          # under every mask
    else:       # the warp mixes neighbouring frames: every real element of the slab is non-finite
        x[:, :N, :F] = junk[rs.randint(0, 3, size=(T, N, F))]
    outside = np.ones(x.shape, bool)
    for n in range(N):
        outside[:lens[n], n, :F] = False
    x[outside] = junk[rs.randint(0, 5, size=int(outside.sum()))]
    got, _ = _run(x, N, F, lens, 31, 4, 2, pol)
    assert np.array_equal(_bits(got[masked]), _bits(np.full(int(masked.sum()), np.float32(-1.5))))
    assert np.array_equal(_bits(got[outside]), _bits(x[outside]))
    if W == 0:
        plain = ~masked
        assert np.array_equal(_bits(got[plain]), _bits(x[plain]))
        assert np.isfinite(got[~outside]).all()


def test_determinism_and_independence_of_the_padding():
    T, N, F, ld = 70, 6, 20, 20
    lens = [70, 69, 8, 33, 1, 50]
    pol = SO.policy(time_warp=6, freq_masks=2, freq_width=7, time_masks=4, time_ratio=0.2)
    rs = np.random.RandomState(5)
    x32 = _slab(rs, T, 32, ld)
    x16 = np.ascontiguousarray(x32[:, :16])
    a, pa = _run(x16, N, F, lens, 42, 8, 3, pol)
    b, pb = _run(x16, N, F, lens, 42, 8, 3, pol)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(pa, pb)
    c, pc = _run(x32, N, F, lens, 42, 8, 3, pol)
    assert np.array_equal(_bits(c[:, :16]), _bits(a)) and np.array_equal(pc, pa)
    # without params_out: the same slab
    d, _ = _run(x16, N, F, lens, 42, 8, 3, pol, params=False)
    assert np.array_equal(_bits(d), _bits(a))
    for other in ((42, 8, 4), (42, 12, 3), (43, 8, 3), (42 + (1 << 40), 8, 3)):
        e, pe = _run(x16, N, F, lens, *other, pol)
        assert not np.array_equal(pe, pa) and not np.array_equal(_bits(e), _bits(a))


# ---------------------------------------------------------------- the engine's stage
POLICY = dict(time_warp=4, freq_masks=2, freq_width=4, time_masks=3, time_width=0, time_ratio=0.3)
LENS = np.array([40, 25, 33, 12])
LABELS = [[1, 2, 3], [4, 1], [2, 2, 5], [3]]


def _models(seed=1, F=10, **kw):
    """A small conformer without front-end (F = 10: two pad columns in the slab) with and
    without the layer; dropout 0, so the two differ in the SpecAugment stage alone (the stage
    index keys the dropout streams)."""
    from asr_study_amd.core import models, optimizers
    out = []
    for sa in (dict(POLICY), False):
        m = models.conformer(num_features=F, num_classes=8, d_model=32, num_heads=2,
                             num_layers=1, d_ff=48, kernel_size=7, dropout=0, conv=False,
                             seed=seed, spec_augment=sa, **kw)
        m.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
        out.append(m)
    assert [s.kind for s in out[0].stages][1:] == [s.kind for s in out[1].stages]
    assert all(np.array_equal(a, b) for a, b in zip(out[0].get_weights(), out[1].get_weights()))
    return out


def _batch(F=10, seed=2):
    rs = np.random.RandomState(seed)
    x = rs.randn(4, 40, F).astype(np.float32)
    for n in range(4):
        x[n, LENS[n]:] = 0
    return x


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def test_training_equals_the_model_without_the_layer_on_the_oracle_slab():
    """Logits, loss and every gradient (DESIGN.md 7's model bounds)."""
    m1, m0 = _models()
    x = _batch()
    slab = m1.to_slab(x)
    keep = slab.clone()
    ctc1, logits1, _ = m1.loss_and_grads(slab, LABELS, LENS, training=True)
    torch.cuda.synchronize()
    assert torch.equal(slab, keep)                      # the caller's slab is never overwritten
    g1 = m1.get_gradients()
    logits1, ctc1 = logits1.cpu().numpy(), ctc1.cpu().numpy()
    aug, masked, rows, warped = SO.apply(slab.cpu().numpy(), 4, 10, LENS, m1.rng_seed, 0, 0,
                                         **POLICY)
    assert masked.any() and warped.any() and (rows[:, 0] >= 0).all()
    stage_out = m1._acts[0]['out'].cpu().numpy()
    assert stage_out.shape == (40, 16, 12) and not stage_out[:, :, 10:].any()   # pad columns: 0
    assert np.abs(stage_out[:, :, :10] - aug).max() <= 1e-6 * np.abs(x).max()
    ctc0, logits0, _ = m0.loss_and_grads(m0.to_slab(aug.transpose(1, 0, 2)[:4].astype(np.float32)),
                                         LABELS, LENS, training=True)
    torch.cuda.synchronize()
    e = _rel(logits1[:, :4], logits0.cpu().numpy()[:, :4])
    print('[specaug] model logits rel err %.3e' % e)
    assert e < 1e-4
    assert _rel(ctc1[:4], ctc0.cpu().numpy()[:4]) < 1e-4
    worst = 0.0
    for k, (g, gw) in enumerate(zip(g1, m0.get_gradients())):
        err = np.abs(g - gw).max()
        worst = max(worst, err / (1e-4 * np.abs(gw).max() + 1e-7))
        assert err < 1e-4 * np.abs(gw).max() + 1e-7, (k, g.shape, err)
    print('[specaug] model %d gradients, worst at %.3f of its bound' % (len(g1), worst))
    # and the augmentation changes the result: the same model on the raw slab differs
    _, raw, _ = m0.loss_and_grads(slab, LABELS, LENS, training=True)
    assert _rel(raw.cpu().numpy()[:, :4], logits1[:, :4]) > 1e-3


def test_inference_is_the_identity():
    m1, m0 = _models()
    x = _batch()
    a = m1.test_on_batch([x, LABELS, LENS])
    b = m0.test_on_batch([x, LABELS, LENS])
    assert a == b
    assert not any(k.startswith('specaug') for k, _ in m1._bufs)    # nothing launched, no buffer
    m1.decoder = m0.decoder = None
    assert np.array_equal(_bits(m1.predict(x, LENS)), _bits(m0.predict(x, LENS)))
    res1 = m1.align(x, LABELS, LENS)
    res0 = m0.align(x, LABELS, LENS)
    assert [r['path'] for r in res1['alignments']] == [r['path'] for r in res0['alignments']]


def test_training_steps_repeat_bit_for_bit():
    x = _batch()
    runs = []
    for _ in range(2):
        m, _ = _models(seed=3)
        for _ in range(2):
            m.train_on_batch([x, LABELS, LENS])
        runs.append(m.get_weights())
        assert m.fallbacks == 0 and m.vetoed_steps == 0 and m._step == 2
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(*runs))
    # the step keys the stream: the second step drew other parameters than the first
    a = SO.apply(np.zeros((40, 16, 10), np.float32), 4, 10, LENS, m.rng_seed, 0, 0, **POLICY)[2]
    b = SO.apply(np.zeros((40, 16, 10), np.float32), 4, 10, LENS, m.rng_seed, 0, 1, **POLICY)[2]
    assert not np.array_equal(a, b)


@pytest.mark.parametrize('F', [10, 12])
def test_ragged_input_lengths_bound_the_augmentation(F):
    """With in_len, nothing is masked or warped past an utterance's length (junk there stays);
    without it every frame counts.  Checked on the stage's output buffer."""
    m1, _ = _models(F=F)
    rs = np.random.RandomState(8)
    x = rs.randn(4, 40, F).astype(np.float32) + 5.0     # no zero anywhere: a mask shows
    slab = m1.to_slab(x)
    ld = slab.shape[2]
    in_len = torch.tensor(LENS, dtype=torch.int32, device='cuda')
    hit_past = 0
    for step in range(3):
        m1._step = step
        m1.forward(slab, training=True, n_real=4, in_len=in_len,
                   seq_len=in_len if m1._needs_lens else None)
        out = m1._acts[0]['out'].cpu().numpy()
        ref = m1._acts[0]['in'].cpu().numpy()
        assert out.shape[2] == m1.f_in_pad0
        want, masked, _, _ = SO.apply(ref, 4, F, LENS, m1.rng_seed, 0, step, **POLICY)
        assert masked.any()
        for n in range(4):
            assert np.array_equal(_bits(out[LENS[n]:, n]), _bits(ref[LENS[n]:, n]))
            assert (out[:LENS[n], n, :F][masked[:LENS[n], n, :F]] == 0).all()
        assert np.array_equal(_bits(out[:, 4:]), _bits(ref[:, 4:]))
        assert np.abs(out - want).max() <= 1e-6 * np.abs(x).max()
        # in_len = None: every frame is valid, so masks may fall past the lengths above
        m1.forward(slab, training=True, n_real=4, seq_len=in_len if m1._needs_lens else None)
        full = m1._acts[0]['out'].cpu().numpy()
        want_full = SO.apply(ref, 4, F, None, m1.rng_seed, 0, step, **POLICY)[0]
        assert np.abs(full - want_full).max() <= 1e-6 * np.abs(x).max()
        hit_past += sum(int((full[LENS[n]:, n, :F] == 0).any()) for n in range(4))
    assert hit_past > 0
    torch.cuda.synchronize()


def test_cli_train_and_eval_with_spec_augment(tmp_path):
    sys.path.insert(0, ROOT)
    import train
    import eval as eval_cli
    from asr_study_amd import cli
    from asr_study_amd.datasets import h5lite
    from asr_study_amd.utils import core_utils
    fmt = 'h5' if h5lite.available() else 'npz'
    fname = str(tmp_path / ('dummy.' + fmt))
    cli.make_dataset_main(['--parser', 'dummy', '--parser_params', 'num_speakers', '4',
                           'num_utterances_per_speaker', '4', 'max_duration', '1.2',
                           'min_duration', '0.6', 'max_label_length', '8', 'split',
                           '[0.5, 0.25]', 'seed', '3', '--input_parser', 'logfbank',
                           '--input_parser_params', 'num_filt', '16', '--output_file', fname])
    out = str(tmp_path / 'run')
    train.main(['--dataset', fname, '--model', 'conformer', '--model_params', 'num_features',
                '16', 'd_model', '32', 'num_heads', '2', 'num_layers', '1', 'd_ff', '64',
                'kernel_size', '7', 'num_classes', '28', 'conv_filters', '4', 'conv_kernels',
                '[[5,7],[3,5]]', 'spec_augment', 'True', '--num_epochs', '1', '--batch_size',
                '4', '--save', out, '--seed', '1', '--lr', '0.001'])
    best = os.path.join(out, 'best.h5')
    assert os.path.exists(best)
    for mode in ('train', 'eval', 'predict'):
        model = core_utils.load_model(best, mode=mode)
        assert model.stages[0].kind == 'specaug' and model.stages[0].policy == SO.DEFAULT
        assert model.config['kwargs']['spec_augment'] is True
    m = eval_cli.main(['--model', best, '--dataset', fname])
    assert len(m) == 4 and np.isfinite(m[1]) and m[3] >= 0
