"""-m gpu: CTC loss/grad and greedy decode through the C ABI vs the float64 oracle.

Tolerances (BASELINE.json north_star: "CTC loss ... within 1e-4 fp32"): loss rtol
1e-4, gradient atol 1e-4 (entries are in [-1, 1]) at every size including T=999 --
the kernel re-centres its log-space rows (float64 offsets), so it does not inherit
the ~1e-3 posterior noise of a plain float32 log-space recursion
(tests/test_oracle_ctc.py::test_float32_close_to_float64); decode indices exact.

The second half runs the input families of tests/ctc_cases.py: every pairs-per-lane
instantiation at both ends of its label-width range, every sequence length against the
16-frame checkpoints, class counts past one wave's width, repeats across lanes, a tight and an
infeasible utterance, confident logits, grad_scale 0, a dirty workspace.  Measured on an MI355X
(gradient max-abs error; loss relative error <= 2.3e-7 everywhere):

    l_max 63 / 64 / 127 / 128 / 255 / 256 / 511     3.4e-6 5.8e-6 5.6e-6 4.3e-6 2.7e-5 1.4e-5 3.8e-5
    seq_len 1..50 at 1 / 2 / 8 pairs per lane       3.7e-6 3.0e-6 4.5e-5
    C = 2 / 64 / 65 / 100 / 128                     8.4e-7 6.4e-6 3.9e-6 7.6e-6 1.1e-5
    [3]*70 / [3]*130 / pairs of length 70           4.4e-6 1.7e-5 3.7e-6
    tight (vs oracle and vs the closed form)        1.1e-7
    peaked scale 12 / 25                            1.3e-6 3.8e-6

The two figures near 4e-5 are utterances of 511 and 260 labels in little more than min_time
frames: the states that carry the posterior then lie hundreds (log2) below the row maximum the
rows are re-centred on, where a float32 ulp is 3e-5 .. 6e-5; the float32 restatement shows the
same (tests/ctc_cases.py: lmax_boundary), so the headroom to 1e-4 is small there by design."""
import numpy as np
import pytest
import torch

from oracle import ctc as OC
from oracle import decode as OD
from tests import ctc_cases as CC
from tests.gpu_util import dev, to_dev, pad_batch, report
from tests.test_oracle_ctc import TF_PROBS_0, TF_PROBS_1

pytestmark = pytest.mark.gpu


def _run(logits, labels, seq_len, want_grad=True, scale=1.0):
    from asr_study_amd import ops
    T, N, C = logits.shape
    n_pad = ops.pad16(N)
    lmax = max([len(l) for l in labels] + [1])
    lab = np.zeros((N, lmax), np.int32)
    for n, l in enumerate(labels):
        lab[n, :len(l)] = l
    lg = to_dev(pad_batch(logits.astype(np.float32), n_pad))
    grad = torch.full_like(lg, 7.0) if want_grad else None
    loss = ops.ctc_loss_grad(lg, to_dev(lab), to_dev(np.array([len(l) for l in labels], np.int32)),
                             to_dev(np.asarray(seq_len, np.int32)), N, grad=grad,
                             grad_scale=scale)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), (grad.cpu().numpy() if want_grad else None), lg


def test_tf_known_answers():
    logits = np.log(np.stack([TF_PROBS_0, TF_PROBS_1], axis=1))
    loss, grad, _ = _run(logits, [[0, 1, 2, 1, 0], [0, 1, 1, 0]], [5, 5])
    assert abs(loss[0] - 3.34211) < 1e-4 and abs(loss[1] - 5.42262) < 1e-4
    _, g64 = OC.ctc_loss_grad(logits, [[0, 1, 2, 1, 0], [0, 1, 1, 0]], [5, 5])
    assert report('ctc tf-vectors grad', grad[:, :2], g64) < 1e-5
    assert np.all(grad[:, 2:] == 0)            # batch padding rows


@pytest.mark.parametrize('seed', [0, 1])
def test_small_ragged(seed):
    rs = np.random.RandomState(seed)
    T, N, C = 41, 7, 11
    logits = rs.randn(T, N, C) * 2
    labels = [rs.randint(0, C - 1, size=rs.randint(1, 9)).tolist() for _ in range(N)]
    labels[1] = [3, 3, 3, 2, 2]
    labels[2] = []
    labels[3] = [5]
    seq_len = [T, 20, 5, T, 11, 30, 1]
    labels[6] = [4]
    l64, g64 = OC.ctc_loss_grad(logits.astype(np.float32), labels, seq_len)
    loss, grad, _ = _run(logits, labels, seq_len, scale=0.5)
    np.testing.assert_allclose(loss, l64, rtol=1e-4)
    assert report('ctc small grad', grad[:, :N], 0.5 * g64) < 1e-4
    for n in range(N):
        assert np.all(grad[seq_len[n]:, n] == 0)
    loss_only, _, _ = _run(logits, labels, seq_len, want_grad=False)
    np.testing.assert_allclose(loss_only, l64, rtol=1e-4)


def test_long_labels_multi_pair_per_lane():
    rs = np.random.RandomState(3)
    T, N, C = 450, 3, 28
    logits = rs.randn(T, N, C)
    labels = [rs.randint(0, 25, size=L).tolist() for L in (200, 70, 1)]
    l64, g64 = OC.ctc_loss_grad(logits.astype(np.float32), labels, [T] * N)
    loss, grad, _ = _run(logits, labels, [T] * N)
    np.testing.assert_allclose(loss, l64, rtol=1e-4)
    assert report('ctc long-label grad', grad[:, :N], g64) < 1e-4


def test_infeasible_gives_inf_loss_zero_grad():
    logits = np.zeros((3, 1, 4))
    loss, grad, _ = _run(logits, [[1, 1, 1]], [3])
    assert np.isinf(loss[0]) and loss[0] > 0 and np.all(grad == 0)


def test_full_size_cfg3_slab():
    """T=999, N=64, C=28 (BASELINE cfg3 CTC slab), labels 2..49 symbols a-y."""
    rs = np.random.RandomState(11)
    T, N, C = 999, 64, 28
    logits = rs.randn(T, N, C).astype(np.float32)
    labels = [rs.randint(0, 25, size=rs.randint(2, 50)).tolist() for _ in range(N)]
    seq_len = [T] * N
    seq_len[5] = 700
    l64, g64 = OC.ctc_loss_grad(logits, labels, seq_len)
    loss, grad, _ = _run(logits, labels, seq_len)
    np.testing.assert_allclose(loss, l64, rtol=1e-4)
    assert report('ctc cfg3 grad', grad, g64) < 1e-4
    # size-independent properties: rows sum to 0 inside, exactly 0 outside
    assert np.abs(grad[:700].sum(-1)).max() < 1e-3
    assert np.all(grad[700:, 5] == 0)


def test_greedy_exact():
    from asr_study_amd import ops
    rs = np.random.RandomState(2)
    T, N, C = 600, 9, 28
    logits = rs.randn(T, N, C).astype(np.float32)
    logits[:, :, C - 1] += 1.5                       # plenty of blanks
    logits[10:20, 0, 3] += 9.0                       # a long repeat
    logits[0, 1, :] = 0.0                            # exact tie -> first index
    seq_len = np.array([T, 599, 257, 256, 255, 1, 2, 300, T], np.int32)
    n_pad = ops.pad16(N)
    lg = to_dev(pad_batch(logits, n_pad))
    dec, dlen = ops.ctc_greedy(lg, to_dev(seq_len), N)
    torch.cuda.synchronize()
    dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
    want = OD.greedy_decode(logits, seq_len)
    for n in range(N):
        assert dec[n, :dlen[n]].tolist() == want[n], n
        assert np.all(dec[n, dlen[n]:] == -1)


# --------------------------------------------------------------------------- every lane layout
# The families of tests/ctc_cases.py: the float32 restatement of the kernels reaches half of the
# tolerances below on each of them without a GPU (tests/test_ctc_loss_model_host.py).
def _check(name, logits, labels, seq_len, l64, g64, scale=1.0):
    """One call with the gradient (prefilled with 7.0, batch padded to 16) and one without."""
    T, N, C = logits.shape
    loss, grad, _ = _run(logits, labels, seq_len, scale=scale)
    ok = np.isfinite(l64)
    assert np.array_equal(np.isposinf(loss), ~ok), (loss, l64)
    rel = report('ctc %s loss/|loss|' % name, loss[ok] / np.abs(l64[ok]), np.sign(l64[ok]))
    gerr = report('ctc %s grad' % name, grad[:, :N], scale * g64)
    assert rel <= 1e-4
    assert gerr < 1e-4
    assert np.isfinite(grad).all()
    for n in range(N):
        assert np.all(grad[seq_len[n]:, n] == 0), n       # past the utterance: exactly 0
        if not ok[n]:
            assert np.all(grad[:, n] == 0), n               # infeasible: exactly 0
    assert np.all(grad[:, N:] == 0)                         # batch padding: exactly 0
    assert np.abs(grad.sum(-1)).max() < 1e-3                # softmax - posterior sums to 0
    loss_only, _, _ = _run(logits, labels, seq_len, want_grad=False)     # the do_beta = 0 launch
    assert np.array_equal(loss_only, loss)
    return loss, grad


def _check_family(name, scale=1.0):
    return _check(name, *(CC.case(name) + CC.reference(name)), scale=scale)


@pytest.mark.parametrize('l_max', CC.LMAX_BOUNDARIES)
def test_l_max_boundaries(l_max):
    """Labels of l_max, l_max - 1, 1 and 0 symbols at the last width of each pairs-per-lane
    instantiation and the first of the next; at L = l_max the final blank is the last pair of
    lane 63."""
    _, labels, seq_len = CC.case('lmax%d' % l_max)
    assert [len(l) for l in labels] == [l_max, l_max - 1, 1, 0]
    assert all(s % 16 for s in seq_len[2:])
    _check_family('lmax%d' % l_max)


def test_l_max_512_is_an_argument_error_and_launches_nothing():
    from asr_study_amd import _lib, ops
    logits = torch.zeros((4, 16, 5), device=dev())
    lab = torch.zeros((1, 512), dtype=torch.int32, device=dev())
    grad = torch.full_like(logits, 7.0)
    loss = torch.full((1,), -3.0, device=dev())
    with pytest.raises(_lib.AsrHipError, match='l_max=512'):
        ops.ctc_loss_grad(logits, lab, to_dev(np.array([1], np.int32)),
                          to_dev(np.array([4], np.int32)), 1, grad=grad, loss=loss)
    torch.cuda.synchronize()
    assert torch.all(grad == 7.0) and loss.item() == -3.0


@pytest.mark.parametrize('name', ['sweep1', 'sweep2', 'sweep8'])
def test_every_sequence_length_against_the_checkpoints(name):
    """seq_len = 1 .. 50 in one batch, at one, two and eight state pairs per lane (prefetch groups
    of 16, 8 and 4 frames against the 16-frame checkpoints); N = 50 or 51 pads to 64."""
    from asr_study_amd import ops
    logits, labels, seq_len = CC.case(name)
    assert seq_len[:50] == list(range(1, 51)) and ops.pad16(len(labels)) == 64
    _check_family(name)


@pytest.mark.parametrize('C', CC.CLASS_COUNTS)
def test_class_counts(C):
    """One class beside the blank, a full 64-class trip of the lse / gradient loops, a second trip
    with one class and partially / completely filled."""
    logits, labels, _ = CC.case('classes%d' % C)
    assert logits.shape[2] == C
    if C > 2:
        assert max(max(l) for l in labels) > C - 2 - 8      # drawn from all C - 1 symbols
    _check_family('classes%d' % C)


@pytest.mark.parametrize('kind', ['run70', 'run130', 'pairs70'])
def test_repeats_across_lanes(kind):
    _check_family(kind)


def test_tight_and_infeasible_in_one_batch():
    """seq_len == min_time leaves a single path: the answer is closed-form (loss = -sum log p
    along the path, gradient = softmax - onehot); one frame fewer is infeasible: +inf loss and a
    zero gradient, the neighbours untouched."""
    logits, labels, seq_len = CC.case('tight')
    loss, grad = _check_family('tight')
    assert np.isposinf(loss[2]) and np.all(grad[:, 2] == 0)
    for n in (0, 1):
        want_l, want_g = CC.tight_closed_form(logits[:, n], labels[n], logits.shape[2] - 1)
        assert abs(loss[n] - want_l) <= 1e-4 * abs(want_l)
        assert report('ctc tight closed form %d' % n, grad[:seq_len[n], n], want_g) < 1e-4


@pytest.mark.parametrize('which', [12, 25])
def test_confident_logits(which):
    _check_family('peaked%d' % which)


def test_grad_scale_zero_and_fractional():
    """grad_scale = 0.0 is the zero-weight dummy shard of loss_and_grads_device: a gradient that
    is exactly 0 (and finite) everywhere with the loss still right."""
    logits, labels, seq_len = CC.case('sweep2')
    l64, _ = CC.reference('sweep2')
    loss, grad, _ = _run(logits, labels, seq_len, scale=0.0)
    np.testing.assert_allclose(loss, l64, rtol=1e-4)
    assert np.isfinite(grad).all() and np.all(grad == 0)
    _check_family('sweep2', scale=0.37)


def test_dirty_reused_workspace():
    """A small call after a larger one on the process-wide 'ctc' workspace, and after the
    workspace was filled with 0xFF bytes: every byte that is read has been written by the call
    itself, so the loss (no atomics on its path) is bitwise the same."""
    from asr_study_amd import ops
    small = CC.case('sweep1')
    first, _, _ = _run(*small)
    big = CC.case('peaked12')
    assert big[0].shape[0] == 300 and max(len(l) for l in big[1]) == 100
    _run(*big)
    again, _ = _check_family('sweep1')
    assert np.array_equal(again.view(np.int32), first.view(np.int32))
    ops.WS.bufs[('ctc', str(dev()))].fill_(255)
    again, _ = _check_family('sweep1')
    assert np.array_equal(again.view(np.int32), first.view(np.int32))


@pytest.mark.parametrize('T,C', [(T, C) for T in (1, 255, 256, 257, 513) for C in (2, 100)])
def test_greedy_chunk_boundary(T, C):
    """Repeats and blanks around the 256-frame chunk of the kernel: the previous chunk's last
    argmax is carried over, so a run across frames 255 | 256 emits once."""
    from asr_study_amd import ops
    rs = np.random.RandomState(T + C)
    blank, k = C - 1, 0
    N = 8
    logits = rs.randn(T, N, C).astype(np.float32)
    logits[:, 1:, blank] += 50.0                     # rows 1.. are blank wherever not set below

    def put(n, t, c):
        if t < T:
            logits[t, n, c] += 100.0
    logits[:, 0, blank] += 1.5                       # 0: random with plenty of blanks
    for t in range(250, 262):                        # 2: one run over the chunk boundary
        put(2, t, k)
    put(3, 255, k), put(3, 256, k)                   # 3: the class on both sides, nothing between
    put(4, 256, k)                                   # 4: blank at 255, the class at 256
    put(5, 255, k), put(5, 256, C - 2)               # 5: another class behind it (C = 2: the same)
    put(6, 255, k), put(6, 256, k)                   # 6: as 3, the utterance ends at the boundary
    put(7, 0, k), put(7, T - 1, k)                   # 7: first and last frame
    seq_len = np.array([T] * N, np.int32)
    seq_len[6] = min(T, 256)
    n_pad = ops.pad16(N)
    dec, dlen = ops.ctc_greedy(to_dev(pad_batch(logits, n_pad)), to_dev(seq_len), N)
    torch.cuda.synchronize()
    dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
    want = OD.greedy_decode(logits, seq_len)
    assert want[1] == [] and want[2] == ([k] if T > 250 else [])
    assert want[3] == want[6] == ([k] if T > 255 else [])
    assert want[4] == ([k] if T > 256 else [])
    assert want[5] == ([k, C - 2] if T > 256 and C > 2 else [k] if T > 255 else [])
    assert want[7] == ([k, k] if T > 2 else [k])
    for n in range(N):
        assert dec[n, :dlen[n]].tolist() == want[n], n
        assert np.all(dec[n, dlen[n]:] == -1)
    assert dlen[1] == 0 and np.all(dec[1] == -1)
