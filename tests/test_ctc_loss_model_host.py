"""The float32 restatement of the CTC loss/gradient kernels (tests/ctc_loss_kernel_model.py)
against the float64 oracle on every input family of tests/ctc_cases.py, without a GPU.

tests/test_gpu_ctc.py asks the kernels for loss rtol 1e-4 and gradient max-abs error 1e-4 on
these inputs.  Here the same arithmetic, restated independently of the kernel, has to reach HALF
of that (loss rtol 5e-5, gradient 5e-5) at each family's own pairs-per-lane / prefetch-group
size: the tolerance is then reachable in float32 with headroom, and a kernel that misses it is
wrong rather than unlucky.  A family that misses the bound here gets other inputs, never a wider
bound.  Also: the oracle against torch's float64 CTC at two wide lattices (two and eight state
pairs per lane on the device), which have no other independent pin."""
import numpy as np
import pytest

from oracle import ctc as OC
from tests import ctc_cases as CC
from tests import ctc_loss_kernel_model as KM
from tests.ctc_align_kernel_model import pick_ppl
from tests.test_oracle_ctc import _torch_ref

HALF_TOL = 5e-5


def test_builders_are_deterministic_and_cover_every_lane_layout():
    ppl = {}
    for name in sorted(CC.FAMILIES):
        a, b = CC.FAMILIES[name](), CC.FAMILIES[name]()
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and list(a[2]) == list(b[2])
        logits, labels, seq_len = a
        T, N, C = logits.shape
        assert all(1 <= t <= T for t in seq_len)
        assert all(0 <= s <= C - 2 for l in labels for s in l)
        ppl.setdefault(pick_ppl(max([len(l) for l in labels] + [1])), []).append(name)
        if name != 'tight':
            assert all(CC.feasible(labels, seq_len)), name
    assert sorted(ppl) == [1, 2, 4, 8]
    assert [pick_ppl(l) for l in CC.LMAX_BOUNDARIES] == [1, 2, 2, 4, 4, 8, 8]
    assert CC.feasible(*CC.case('tight')[1:]) == [True, True, False]
    # the sweeps put a sequence end at every position against the 16-frame checkpoints
    assert CC.case('sweep1')[2] == list(range(1, 51))
    assert CC.case('sweep2')[2] == list(range(1, 51)) + [160]
    assert CC.case('sweep8')[2] == list(range(1, 51)) + [300]


def test_peaked_builder_follows_the_label():
    """Without wrong frames and noise-dominating scale the greedy path collapses to the label."""
    from oracle import decode as OD
    rs = np.random.RandomState(0)
    labels = [CC.random_label(rs, 30, 9), [2, 2, 2], []]
    logits, _, seq_len = CC.peaked(1, 80, 9, labels, 30.0, 0.0, [80, 7, 5])
    assert OD.greedy_decode(logits, np.array(seq_len)) == labels


@pytest.mark.parametrize('name', sorted(CC.FAMILIES))
def test_restatement_reaches_half_the_gpu_tolerance(name):
    logits, labels, seq_len = CC.case(name)
    l64, g64 = CC.reference(name)
    loss, grad = KM.loss_grad(logits, labels, seq_len)
    ok = np.isfinite(l64)
    assert np.array_equal(np.isposinf(loss), ~ok)
    rel = np.abs(loss[ok] - l64[ok]) / np.abs(l64[ok])
    err = np.abs(grad - g64).max()
    print('[restatement] %-12s PPL %d loss rel %.2e grad max|err| %.2e'
          % (name, pick_ppl(max([len(l) for l in labels] + [1])), rel.max(), err))
    assert rel.max() <= HALF_TOL
    assert err <= HALF_TOL
    assert np.all(grad[:, ~ok] == 0)


def test_tight_case_is_the_closed_form():
    """seq_len == min_time leaves one path: loss = -sum log p along it, grad = softmax - onehot."""
    logits, labels, seq_len = CC.case('tight')
    l64, g64 = CC.reference('tight')
    for n in (0, 1):
        loss, grad = CC.tight_closed_form(logits[:, n], labels[n], logits.shape[2] - 1)
        assert abs(loss - l64[n]) <= 1e-10 * abs(loss)
        assert np.abs(grad - g64[:seq_len[n], n]).max() <= 1e-10


@pytest.mark.parametrize('L,T', [(70, 120), (260, 330)])
def test_oracle_matches_torch_ctc_at_wide_lattices(L, T):
    rs = np.random.RandomState(L)
    N, C = 3, 9
    logits = rs.randn(T, N, C) * 2.0
    labels = [np.array(CC.random_label(rs, L, C, T)), np.array(CC.random_label(rs, L // 2, C)),
              np.array([4] * (L // 4))]
    seq_len = [T, T - 11, T - 40]
    loss, grad = OC.ctc_loss_grad(logits, labels, seq_len)
    rl, rg = _torch_ref(logits, labels, seq_len)
    np.testing.assert_allclose(loss, rl, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(grad, rg, rtol=0, atol=1e-10)
