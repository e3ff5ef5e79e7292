"""CPU checks of the transducer (K31): the float64 oracle against a brute-force sum
over every alignment and against torch autograd through an independent alpha recursion, the
Python model of the greedy loop against the textbook per-utterance decode, and the argument
checks of the C ABI, which precede any launch.  No device is touched.

Everything above the section "the C ABI" validates tests/rnnt_oracle.py, NOT csrc/rnnt.hip: those
tests pass whatever the library does and are no coverage of the kernels.  The kernels are compared
with the oracle they validate in tests/test_gpu_rnnt.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import rnnt_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lp(rs, T, U1, Cc, scale=1.5):
    return RO.log_softmax(rs.randn(T, U1, Cc) * scale)


@pytest.mark.parametrize('T', [1, 2, 3, 4])
@pytest.mark.parametrize('U', [0, 1, 2, 3])
def test_oracle_loss_is_the_sum_over_all_alignments(T, U):
    rs = np.random.RandomState(10 * T + U)
    lp = _lp(rs, T, U + 1, 3)
    y = list(rs.randint(0, 2, U))
    loss, alpha, beta, _ = RO.lattice(lp, y)
    assert abs(loss - RO.brute_force_loss(lp, y)) < 1e-13
    assert abs(beta[0, 0] + loss) < 1e-13                   # beta(0, 0) = logZ as well


def test_oracle_gradient_is_the_derivative_of_the_brute_force_sum():
    """T = 3, U = 2, C = 3: dz against central differences of the enumeration, on the LOGITS
    (the gradient formula includes the softmax)."""
    rs = np.random.RandomState(0)
    z = rs.randn(3, 3, 3)
    y = [1, 0]
    _, _, _, dz = RO.lattice(RO.log_softmax(z), y)
    num = np.zeros_like(z)
    eps = 1e-6
    for i in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[i] += eps
        zm[i] -= eps
        num[i] = (RO.brute_force_loss(RO.log_softmax(zp), y) -
                  RO.brute_force_loss(RO.log_softmax(zm), y)) / (2 * eps)
    assert np.abs(num - dz).max() < 1e-9


def _torch_loss(enc, pred, W, b, labels, label_len, seq_len, N):
    """An independent statement: plain torch ops, torch.logsumexp, float64, autograd."""
    total, losses = 0.0, []
    J = W.shape[0]
    for n in range(N):
        t_n, u_n = int(seq_len[n]), int(label_len[n])
        z = torch.tanh(enc[:t_n, n, None, :J] + pred[None, :u_n + 1, n, :J]) @ W + b
        lp = torch.log_softmax(z, dim=-1)
        blank = lp.shape[-1] - 1
        alpha = [[None] * (u_n + 1) for _ in range(t_n)]
        alpha[0][0] = torch.zeros((), dtype=torch.float64)
        for t in range(t_n):
            for u in range(u_n + 1):
                terms = []
                if t > 0:
                    terms.append(alpha[t - 1][u] + lp[t - 1, u, blank])
                if u > 0:
                    terms.append(alpha[t][u - 1] + lp[t, u - 1, int(labels[n][u - 1])])
                if terms:
                    alpha[t][u] = torch.logsumexp(torch.stack(terms), dim=0)
        ln = -(alpha[t_n - 1][u_n] + lp[t_n - 1, u_n, blank])
        losses.append(ln)
        total = total + ln
    return total, losses


def _case(rs, T, l_max, N, n_pad, J, Cc, seq_len, label_len, scale=1.0):
    Jp = (J + 3) // 4 * 4
    enc = rs.randn(T, n_pad, Jp) * scale
    pred = rs.randn(l_max + 1, n_pad, Jp) * scale
    W = rs.randn(J, Cc) * scale
    b = rs.randn(Cc) * 0.5
    labels = rs.randint(0, Cc - 1, (N, max(l_max, 1)))[:, :l_max]
    return enc, pred, W, b, labels, np.asarray(label_len), np.asarray(seq_len)


def test_oracle_gradients_equal_torch_autograd():
    rs = np.random.RandomState(3)
    N = 3
    enc, pred, W, b, labels, ll, sl = _case(rs, 6, 4, N, 16, 5, 4, (6, 1, 4), (4, 0, 2))
    loss, d_enc, d_pred, dW, db = RO.loss_and_grads(enc, pred, W, b, labels, ll, sl, N,
                                                    grad_scale=0.5)
    te = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (enc, pred, W, b)]
    total, losses = _torch_loss(te[0], te[1], te[2], te[3], labels, ll, sl, N)
    (0.5 * total).backward()
    assert np.abs(loss - np.array([float(v.detach()) for v in losses])).max() < 1e-12
    for got, t in zip((d_enc, d_pred, dW, db), te):
        assert np.abs(got - t.grad.numpy()).max() < 1e-12
    # the regions the kernel must leave zero
    assert not d_enc[1:, 1].any() and not d_enc[4:, 2].any() and not d_enc[:, N:].any()
    assert not d_pred[1:, 1].any() and not d_pred[3:, 2].any() and not d_pred[:, N:].any()


def test_every_cell_gradient_sums_to_zero_over_the_classes():
    rs = np.random.RandomState(4)
    lp = _lp(rs, 7, 5, 6, scale=3.0)
    _, _, _, dz = RO.lattice(lp, [0, 3, 3, 1])
    assert np.abs(dz.sum(axis=-1)).max() < 1e-14
    assert np.abs(dz).max() > 1e-2


def _toy_predictor(rs, Cc, J, S=5):
    """A small recurrent predictor in NumPy: state (N, S), g = tanh(state A + x E + c)."""
    A, E, c = rs.randn(S, S) * 0.8, rs.randn(Cc - 1, S) * 1.5, rs.randn(S) * 0.3
    P = rs.randn(S, J)

    def init(N):
        s = np.tanh(np.zeros((N, S)) @ A + c)
        return [s], s @ P

    def step(state, x):
        s = np.tanh(state[0] @ A + np.float64(x) @ E + c)
        return [s], s @ P
    return init, step


@pytest.mark.parametrize('max_symbols', [1, 2, 10])
def test_batched_greedy_loop_equals_the_per_utterance_decode(max_symbols):
    rs = np.random.RandomState(5 + max_symbols)
    T, N, n_pad, J, Cc = 12, 5, 16, 6, 5
    enc = rs.randn(T, n_pad, 8) * 1.5
    W, b = rs.randn(J, Cc) * 1.5, rs.randn(Cc) * 0.3
    b[Cc - 1] -= 0.5                                        # fewer blanks: frames with several labels
    seq_len = np.array([12, 0, 7, 1, 12])
    init, step = _toy_predictor(rs, Cc, J)
    got = RO.greedy_batched(enc, W, b, seq_len, N, init, step, max_symbols)
    want = [RO.greedy_naive(enc[:, n], W, b, int(seq_len[n]), init, step, max_symbols)
            for n in range(N)]
    assert got == want
    assert got[1] == [] and max(len(g) for g in got) > 3
    assert max(len(g) for g in got) <= T * max_symbols


def test_onehot_rows_and_rows_select_models():
    labels = np.array([[2, 0, 1], [1, 1, 1]])
    out = RO.onehot_rows(labels, [3, 1], 2, 16, 3, ld=4)
    assert out.shape == (4, 16, 4) and out.sum() == 4
    assert out[1, 0, 2] == out[2, 0, 0] == out[3, 0, 1] == out[1, 1, 1] == 1
    a, b = np.ones((16, 2)), np.zeros((16, 2))
    sel = RO.rows_select([0, 1, 1], a, b, 3)
    assert sel[:, 0].tolist() == [0, 1, 1] + [0] * 13


# ---------------------------------------------------------------- the C ABI
@pytest.fixture(scope='module')
def lib():
    from asr_study_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


NEW = ('asr_rnnt_workspace_bytes', 'asr_rnnt_loss_grad', 'asr_rnnt_greedy_step',
       'asr_onehot_rows', 'asr_rows_select')


def test_new_symbols_declared_exported_and_mirrored(lib):
    from asr_study_amd import _lib, build
    with open(os.path.join(ROOT, 'include', 'asr_hip.h')) as f:
        header = f.read()
    for name, nargs in zip(NEW, (6, 23, 21, 10, 8)):
        assert re.search(r'\b%s\(' % name, header)
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args) and len(args) == nargs
    assert _lib.SIGNATURES[NEW[0]][0] is C.c_size_t
    assert _lib.ABI_VERSION == 107 and lib.asr_version() == 107      # additions only
    assert 'rnnt.hip' in build.SOURCES


def test_workspace_has_no_joint_sized_term(lib):
    """O(N T U1) floats and slabs without the product T U1: tens of megabytes at the bench shape
    (the joint's hidden tensor alone would be 6.6 GB), and J enters through the slabs only."""
    ws = lib.asr_rnnt_workspace_bytes
    T, U1, N = 500, 101, 64
    bench = ws(T, U1, N, 64, 512, 29)
    cells = N * (T + U1 - 1) * U1 * 4
    assert 4 * cells < bench < 100e6
    slabs = bench - ws(T, U1, N, 64, 4, 29)
    assert 0 < slabs <= 256 * 513 * 32 * 4
    assert ws(2 * T, U1, N, 64, 512, 29) - bench < 4.5 * N * T * U1 * 4   # linear in T
    assert ws(T, U1, N, 64, 512, 64) - bench == 256 * 513 * 32 * 4        # C: the slabs only
    for bad in ((0, U1, N, 64, 512, 29), (T, 0, N, 64, 512, 29), (T, 257, N, 64, 512, 29),
                (T, U1, 0, 64, 512, 29), (T, U1, 65, 64, 512, 29), (T, U1, N, 64, 513, 29),
                (T, U1, N, 64, 0, 29), (T, U1, N, 64, 512, 1), (T, U1, N, 64, 512, 65)):
        assert ws(*bad) == 0, bad


def test_loss_grad_argument_checks_without_a_device(lib):
    p = [C.c_void_p(4096 * (i + 1)) for i in range(13)]      # non-NULL, nothing dereferences them
    good = dict(T=9, U1=7, N=3, n_pad=16, J=36, C=29, l_max=6)
    order = ('T', 'U1', 'N', 'n_pad', 'J', 'C', 'l_max')

    def call(ptrs=None, grads=4, ws_bytes=1 << 30, **kw):
        v = dict(good, **kw)
        q = list(ptrs or p)
        g = q[8:12] if grads == 4 else [None] * (4 - grads) + q[8:8 + grads]
        return lib.asr_rnnt_loss_grad(q[0], q[1], q[2], q[3], q[4], q[5], q[6],
                                      *[v[k] for k in order], 1.0, q[7], g[0], g[1], g[2], g[3],
                                      q[12], ws_bytes, None)
    for key, val in (('T', 1000001), ('J', 0), ('J', 513), ('C', 1), ('C', 65), ('l_max', 256), ('l_max', -1),
                     ('U1', 8), ('U1', 6), ('T', 0), ('N', 0), ('N', 17), ('n_pad', 8),
                     ('n_pad', 20)):
        kw = {key: val}
        if key == 'l_max' and val >= 0:
            kw['U1'] = val + 1
        assert call(**kw) == -1, (key, val)
        assert 'rnnt_loss_grad' in lib.asr_last_error().decode()
    for i in (0, 1, 2, 3, 4, 5, 6, 7):                       # a NULL input, length or loss
        q = list(p)
        q[i] = None
        assert call(ptrs=q) == -1, i
    for grads in (1, 2, 3):                                  # some gradient pointers, not all
        assert call(grads=grads) == -1
        assert 'gradient pointers' in lib.asr_last_error().decode()
    assert call(ws_bytes=1024) == -2 and b'workspace' in lib.asr_last_error()
    q = list(p)
    q[12] = None
    assert call(ptrs=q) == -2


def test_helper_argument_checks_without_a_device(lib):
    a, b, c = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(12288)
    assert lib.asr_onehot_rows(a, b, 7, 3, 16, 5, 28, 28, c, None) == -1     # U1 != l_max + 1
    assert lib.asr_onehot_rows(a, b, 7, 3, 16, 6, 28, 27, c, None) == -1     # ld < width
    assert lib.asr_onehot_rows(a, None, 7, 3, 16, 6, 28, 28, c, None) == -1
    assert lib.asr_onehot_rows(None, b, 7, 3, 16, 6, 28, 28, c, None) == -1
    assert b'onehot_rows' in lib.asr_last_error()
    assert lib.asr_rows_select(a, b, c, None, 3, 16, 8, None) == -1
    assert lib.asr_rows_select(a, b, c, c, 17, 16, 8, None) == -1
    assert lib.asr_rows_select(a, b, c, c, 3, 16, 0, None) == -1
    assert b'rows_select' in lib.asr_last_error()
    p = [C.c_void_p(4096 * (i + 1)) for i in range(12)]

    def greedy(J=36, Cc=29, max_symbols=10, cap=50, ld_next=28, n_pad=16, null=None):
        q = list(p)
        if null is not None:
            q[null] = None
        return lib.asr_rnnt_greedy_step(q[0], q[1], q[2], q[3], q[4], 9, 3, n_pad, J, Cc,
                                        max_symbols, cap, ld_next, q[5], q[6], q[7], q[8], q[9],
                                        q[10], q[11], None)
    for kw in (dict(J=513), dict(J=0), dict(Cc=65), dict(Cc=1), dict(max_symbols=0), dict(cap=0),
               dict(ld_next=27), dict(n_pad=8), dict(null=0), dict(null=5), dict(null=11)):
        assert greedy(**kw) == -1, kw
        assert b'rnnt_greedy_step' in lib.asr_last_error()
