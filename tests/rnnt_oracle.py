"""Oracle: the RNN-Transducer (Graves, arXiv 1211.3711) as csrc/rnnt.hip defines it (include/asr_hip.h
K31), restated in float64 NumPy: the joint, the lattice loss, all five gradients, and Python
models of asr_rnnt_greedy_step, asr_onehot_rows and asr_rows_select.  Test infrastructure only.

No third-party transducer implementation (warp-transducer, torchaudio's rnnt_loss, ...) is
installed where these tests run, so the oracle cannot be pinned to one.  It is checked instead
(tests/test_rnnt_host.py) against two independent statements of the same mathematics: a brute-force
sum over every monotonic alignment, and torch float64 autograd through a plain torch.logsumexp
alpha recursion.

  z(t, u, :) = tanh(f(t, :) + g(u, :)) W + b,   lp = log_softmax(z),   blank = C - 1
  alpha(0, 0) = 0,  alpha(t, u) = lse(alpha(t-1, u) + lp_blank(t-1, u), alpha(t, u-1) + lp_{y_u}(t, u-1))
  loss = -(alpha(T-1, U) + lp_blank(T-1, U))
  dz(t, u, k) = e^{alpha + beta - logZ} softmax_k - [k = blank] e^{alpha + lp_blank + beta(t+1, u) - logZ}
                - [k = y_{u+1}] e^{alpha + lp_y + beta(t, u+1) - logZ},   beta(T, U) = 0
"""
import itertools

import numpy as np


def log_softmax(z):
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def joint(f, g, W, b):
    """f (T, J), g (U1, J) -> h (T, U1, J), z (T, U1, C)"""
    h = np.tanh(f[:, None, :] + g[None, :, :])
    return h, h @ W + b


def _lse(a, b):
    m = max(a, b)
    if m == -np.inf:
        return m
    return m + np.log(np.exp(a - m) + np.exp(b - m))


def lattice(lp, y):
    """lp (T, U1, C) log-probabilities, y (U) labels, U1 = U + 1.  Returns loss, alpha, beta, dz
    (= d loss / d logits, (T, U1, C))."""
    T, U1, C = lp.shape
    U = len(y)
    assert U1 == U + 1
    blank = C - 1
    alpha = np.full((T, U1), -np.inf)
    alpha[0, 0] = 0.0
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                continue
            a = alpha[t - 1, u] + lp[t - 1, u, blank] if t > 0 else -np.inf
            b = alpha[t, u - 1] + lp[t, u - 1, y[u - 1]] if u > 0 else -np.inf
            alpha[t, u] = _lse(a, b)
    logz = alpha[T - 1, U] + lp[T - 1, U, blank]
    beta = np.full((T + 1, U1 + 1), -np.inf)
    beta[T, U] = 0.0
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            a = beta[t + 1, u] + lp[t, u, blank]
            b = beta[t, u + 1] + lp[t, u, y[u]] if u < U else -np.inf
            beta[t, u] = _lse(a, b)
    dz = np.zeros_like(lp)
    for t in range(T):
        for u in range(U1):
            occ = np.exp(alpha[t, u] + beta[t, u] - logz)
            dz[t, u] = occ * np.exp(lp[t, u])
            dz[t, u, blank] -= np.exp(alpha[t, u] + lp[t, u, blank] + beta[t + 1, u] - logz)
            if u < U:
                dz[t, u, y[u]] -= np.exp(alpha[t, u] + lp[t, u, y[u]] + beta[t, u + 1] - logz)
    return -logz, alpha, beta[:T, :U1], dz


def brute_force_loss(lp, y):
    """-log of the sum over EVERY alignment: the U label emissions are placed at frames
    t_1 <= ... <= t_U, each frame ends in a blank."""
    T, U1, C = lp.shape
    U = len(y)
    blank = C - 1
    total = 0.0
    for frames in itertools.combinations_with_replacement(range(T), U):
        lg, u = 0.0, 0
        for t in range(T):
            while u < U and frames[u] == t:
                lg += lp[t, u, y[u]]
                u += 1
            lg += lp[t, u, blank]
        total += np.exp(lg)
    return -np.log(total)


def clamp_lens(seq_len, label_len, T, l_max):
    return (np.clip(np.asarray(seq_len), 1, T).astype(int),
            np.clip(np.asarray(label_len), 0, l_max).astype(int))


def loss_and_grads(enc, pred, W, b, labels, label_len, seq_len, N, grad_scale=1.0):
    """The slabs of the C ABI: enc (T, n_pad, Jp), pred (U1, n_pad, Jp), W (J, C), b (C), labels
    (N, U1 - 1).  Returns loss (N) and d_enc, d_pred, dW, db = grad_scale * d sum(loss) / d(.)
    in float64; rows n >= N are never read."""
    enc, pred = np.asarray(enc, np.float64), np.asarray(pred, np.float64)
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    T, U1, J = enc.shape[0], pred.shape[0], W.shape[0]
    Tn, Un = clamp_lens(seq_len, label_len, T, U1 - 1)
    loss = np.zeros(N)
    d_enc, d_pred = np.zeros_like(enc), np.zeros_like(pred)
    dW, db = np.zeros_like(W), np.zeros_like(b)
    for n in range(N):
        t_n, u_n = Tn[n], Un[n]
        f, g = enc[:t_n, n, :J], pred[:u_n + 1, n, :J]
        h, z = joint(f, g, W, b)
        loss[n], _, _, dz = lattice(log_softmax(z), [int(v) for v in labels[n][:u_n]])
        dz *= grad_scale
        dpre = (dz @ W.T) * (1.0 - h * h)
        d_enc[:t_n, n, :J] = dpre.sum(axis=1)
        d_pred[:u_n + 1, n, :J] = dpre.sum(axis=0)
        dW += np.einsum('tuj,tuc->jc', h, dz)
        db += dz.sum(axis=(0, 1))
    return loss, d_enc, d_pred, dW, db


# ------------------------------------------------------------------ the row helpers
def onehot_rows(labels, label_len, N, n_pad, width, ld=None):
    labels = np.asarray(labels)
    l_max = labels.shape[1] if labels.ndim == 2 else 0
    ld = width if ld is None else ld
    out = np.zeros((l_max + 1, n_pad, ld), np.float32)
    for n in range(N):
        for u in range(1, min(int(label_len[n]), l_max) + 1):
            if 0 <= labels[n, u - 1] < width:
                out[u, n, labels[n, u - 1]] = 1.0
    return out


def rows_select(mask, a, b, N):
    out = np.array(b, copy=True)
    for n in range(N):
        if mask[n]:
            out[n] = a[n]
    return out


# ------------------------------------------------------------------ greedy decoding
def first_argmax(z):
    return int(np.argmax(z))          # NumPy returns the FIRST maximum


def greedy_step(enc, g_cur, W, b, seq_len, N, st, max_symbols, cap):
    """Python model of asr_rnnt_greedy_step.  st: dict of t_ptr, n_sym, decoded_len (N) int and
    decoded (N, cap), updated in place.  Returns advance (N), x_next (N, C - 1), active."""
    T, C = enc.shape[0], len(b)
    J = W.shape[0]
    advance = np.zeros(N, np.int32)
    x_next = np.zeros((N, C - 1), np.float32)
    active = 0
    for n in range(N):
        t_n = int(np.clip(seq_len[n], 0, T))
        t = int(st['t_ptr'][n])
        if t >= t_n:
            continue
        z = np.tanh(np.float64(enc[t, n, :J]) + np.float64(g_cur[n, :J])) @ np.float64(W) + b
        k = first_argmax(z)
        if k != C - 1 and st['n_sym'][n] < max_symbols:
            if st['decoded_len'][n] < cap:
                st['decoded'][n, st['decoded_len'][n]] = k
                st['decoded_len'][n] += 1
            st['n_sym'][n] += 1
            advance[n] = 1
            x_next[n, k] = 1.0
            active += 1
        else:
            st['t_ptr'][n] = t + 1
            st['n_sym'][n] = 0
            active += int(t + 1 < t_n)
    return advance, x_next, active


def greedy_batched(enc, W, b, seq_len, N, pred_init, pred_step, max_symbols=10):
    """The batched loop the model runs: greedy_step, one predictor step for every row, the new
    predictor state kept only for the rows that emitted.  pred_init(N) -> (state, g) for the
    start-of-sequence input; pred_step(state, x (N, C - 1)) -> (state', g'); state is a list of
    (N, .) arrays.  Returns the label lists."""
    T, C = enc.shape[0], len(b)
    cap = T * max_symbols
    st = dict(t_ptr=np.zeros(N, int), n_sym=np.zeros(N, int), decoded_len=np.zeros(N, int),
              decoded=np.full((N, cap), -1, int))
    state, g = pred_init(N)
    for _ in range(T * (max_symbols + 1)):
        advance, x_next, active = greedy_step(enc, g, W, b, seq_len, N, st, max_symbols, cap)
        new_state, new_g = pred_step(state, x_next)
        state = [rows_select(advance, a, s, N) for a, s in zip(new_state, state)]
        g = rows_select(advance, new_g, g, N)
        if active == 0:
            break
    return [list(st['decoded'][n, :st['decoded_len'][n]]) for n in range(N)]


def greedy_naive(enc_n, W, b, t_n, pred_init, pred_step, max_symbols=10):
    """One utterance, the textbook loop: for every frame emit labels until blank (or max_symbols),
    feeding each label to the predictor."""
    C = len(b)
    J = W.shape[0]
    state, g = pred_init(1)
    out = []
    for t in range(t_n):
        for _ in range(max_symbols):
            z = np.tanh(np.float64(enc_n[t, :J]) + np.float64(g[0, :J])) @ np.float64(W) + b
            k = first_argmax(z)
            if k == C - 1:
                break
            out.append(k)
            x = np.zeros((1, C - 1), np.float32)
            x[0, k] = 1.0
            state, g = pred_step(state, x)
    return out
