"""CPU: tests/aed_oracle.py against independent statements of the same mathematics (central
differences in float64, tests/attention_oracle.py), and the ABI surface of K32 as the binding
derives it from the header.  No device."""
import numpy as np
import pytest

from tests import aed_oracle as AO
from tests import attention_oracle as ATO


def _case(seed=0, U1=4, N=2, J=8, C=5):
    rng = np.random.RandomState(seed)
    ctx, q = rng.randn(U1, N, J) * 0.7, rng.randn(U1, N, J) * 0.7
    W, b = rng.randn(J, C) * 0.5, rng.randn(C) * 0.3
    labels = rng.randint(0, C - 1, size=(N, U1 - 1))
    label_len = np.array([U1 - 1, 1])[:N]
    return ctx, q, W, b, labels, label_len


def _central(f, x, h=1e-6):
    g = np.zeros_like(x)
    it = np.nditer(x, flags=['multi_index'])
    for _ in it:
        i = it.multi_index
        old = x[i]
        x[i] = old + h
        up = f()
        x[i] = old - h
        dn = f()
        x[i] = old
        g[i] = (up - dn) / (2 * h)
    return g


@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_loss_gradients_match_central_differences(eps):
    ctx, q, W, b, labels, ll = _case()
    N = 2
    _, d_pre, dW, db = AO.loss_and_grads(ctx, q, W, b, labels, ll, N, eps=eps, grad_scale=0.5)

    def f():
        return 0.5 * AO.loss_and_grads(ctx, q, W, b, labels, ll, N, eps=eps)[0].sum()
    for got, x in ((d_pre, ctx), (d_pre, q), (dW, W), (db, b)):
        want = _central(f, x)
        assert np.abs(got - want).max() <= 1e-8 * max(1.0, np.abs(want).max())
    # rows past U_n: never read, gradient exactly 0
    assert not d_pre[2:, 1].any()


def test_cross_attention_gradients_match_central_differences():
    rng = np.random.RandomState(1)
    Tq, Tk, N, heads, dh = 3, 5, 2, 2, 4
    D = heads * dh
    q, kv = rng.randn(Tq, N, D), rng.randn(Tk, N, 2 * D)
    ql, kl = [3, 2], [5, 3]
    g = rng.randn(Tq, N, D)
    out, c = AO.cross_forward(q, kv, heads, ql, kl)
    dq, dkv = AO.cross_backward(g, c)

    def f():
        return (AO.cross_forward(q, kv, heads, ql, kl)[0] * g).sum()
    for got, x in ((dq, q), (dkv, kv)):
        want = _central(f, x)
        assert np.abs(got - want).max() <= 1e-8 * max(1.0, np.abs(want).max())
    # the masked query row and the masked keys
    assert not out[2, 1].any() and not c['lse'][2, 1].any() and not dq[2, 1].any()
    assert not dkv[3:, 1].any()


@pytest.mark.parametrize('ragged', [False, True])
def test_equal_lengths_is_self_attention(ragged):
    rng = np.random.RandomState(2)
    T, N, heads, dh = 7, 3, 2, 4
    D = heads * dh
    qkv = rng.randn(T, N, 3 * D)
    lens = [7, 4, 1] if ragged else None
    g = rng.randn(T, N, D)
    want, cs = ATO.attn_forward(qkv, heads, lens)
    dqkv = ATO.attn_backward(g, cs)
    out, c = AO.cross_forward(qkv[..., :D], qkv[..., D:], heads, None, lens)
    dq, dkv = AO.cross_backward(g, c)
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-13)
    np.testing.assert_allclose(c['lse'], cs['lse'], rtol=0, atol=1e-13)
    np.testing.assert_allclose(dq, dqkv[..., :D], rtol=0, atol=1e-13)
    np.testing.assert_allclose(dkv, dqkv[..., D:], rtol=0, atol=1e-13)


def test_eps_zero_is_plain_nll():
    ctx, q, W, b, labels, ll = _case(seed=3)
    loss = AO.loss_and_grads(ctx, q, W, b, labels, ll, 2)[0]
    C = len(b)
    for n in range(2):
        lp = AO.log_softmax(np.tanh(ctx[:, n] + q[:, n]) @ W + b)
        y = list(labels[n, :ll[n]]) + [C - 1]
        assert abs(loss[n] + sum(lp[u, k] for u, k in enumerate(y))) <= 1e-12


def test_eos_row_is_counted_exactly_once():
    """loss_n is the sum over exactly U_n + 1 rows, the last one scored against EOS: with a W
    of zeros every row costs log C, whatever the labels."""
    ctx, q, W, b, labels, ll = _case(seed=4)
    C = len(b)
    loss = AO.loss_and_grads(ctx, q, np.zeros_like(W), np.zeros_like(b), labels, ll, 2)[0]
    np.testing.assert_allclose(loss, (ll + 1) * np.log(C), rtol=1e-13)
    # and the EOS row alone (no labels): one row, its target C - 1
    one = AO.loss_and_grads(ctx, q, W, b, labels, [0, 0], 2)[0]
    for n in range(2):
        lp = AO.log_softmax(np.tanh(ctx[0, n] + q[0, n]) @ W + b)
        assert abs(one[n] + lp[C - 1]) <= 1e-12
    assert list(AO.targets(labels[0], 3, C)[-1:]) == [C - 1]


def test_greedy_naive_stops_on_eos_and_at_the_cap():
    rng = np.random.RandomState(5)
    D, C, heads = 8, 4, 2
    kv = rng.randn(6, 2 * D)
    W = np.zeros((D, C))

    def init(n):
        return None, np.zeros((n, D))

    def step(state, x):
        return state, np.zeros((1, D))
    b = np.array([0.0, 1.0, 0.0, 0.5])                  # always label 1: runs into the cap
    assert AO.greedy_naive(kv, W, b, heads, init, step, max_labels=5) == [1] * 5
    b = np.array([0.0, 1.0, 0.0, 1.5])                  # EOS at once
    m = []
    assert AO.greedy_naive(kv, W, b, heads, init, step, margins=m) == []
    assert m == [0.5]


def test_abi_surface():
    """The header declares K32 and the binding derives it: the struct's fields in the order the
    issue states, the entry points, the build list."""
    from asr_study_amd import _lib as L
    from asr_study_amd import build, ops
    assert [f for f, _ in L.AttnCrossArgs._fields_] == [
        'Tq', 'Tk', 'N', 'n_pad', 'heads', 'dh', 'ld_q', 'ld_kv', 'ld_out', 'scale', 'q', 'kv',
        'q_lens', 'k_lens', 'out', 'lse', 'dout', 'dq', 'dkv']
    for name in ('asr_attn_cross_workspace_bytes', 'asr_attn_cross_fwd', 'asr_attn_cross_bwd',
                 'asr_aed_workspace_bytes', 'asr_aed_loss_grad', 'asr_aed_greedy_step'):
        assert name in L.SIGNATURES
    assert L.ABI_VERSION == 107                          # additions only
    assert 'cross_attention.hip' in build.SOURCES and 'aed.hip' in build.SOURCES
    for name in ('attn_cross_fwd', 'attn_cross_bwd', 'aed_loss_grad', 'aed_greedy_step'):
        assert callable(getattr(ops, name))
