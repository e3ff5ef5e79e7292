"""Oracle: the attention encoder-decoder's kernels as include/asr_hip.h K32 defines them, restated
in float64 NumPy: cross-attention forward and backward (csrc/cross_attention.hip), the decoder's
joint + label-smoothed cross-entropy with all its gradients and a Python model of the greedy
decode (csrc/aed.hip).  Test infrastructure only; tests/test_aed_host.py checks it against central
differences and against tests/attention_oracle.py.

  cross-attention, per sample n and head h:  q (Tq, N, D), kv (Tk, N, 2D) = [K | V]
    s[t, u] = scale q_t . k_u  for u < k_lens[n];  p = softmax_u(s), 0 for u >= k_lens[n]
    out_t = sum_u p[t, u] v_u,  lse_t = log sum_u exp s[t, u]      for t < q_lens[n]
    out_t = lse_t = 0, and no contribution to any gradient        for t >= q_lens[n]
  joint + cross-entropy, per row (u, n), 0 <= u <= U_n:
    h = tanh(ctx + q),  z = h W + b,  lp = log_softmax(z)
    target = y_{u+1} for u < U_n, EOS = C - 1 for u = U_n
    loss_n = sum_u -((1 - eps) lp[target] + eps mean_c lp[c])
"""
import numpy as np


def log_softmax(z):
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def clamp_lens(q_lens, k_lens, N, Tq, Tk):
    ql = np.full(N, Tq) if q_lens is None else np.clip(np.asarray(q_lens).reshape(-1)[:N], 0, Tq)
    kl = np.full(N, Tk) if k_lens is None else np.clip(np.asarray(k_lens).reshape(-1)[:N], 1, Tk)
    return ql.astype(int), kl.astype(int)


# ----------------------------------------------------------------------------- cross-attention
def cross_forward(q, kv, heads, q_lens=None, k_lens=None, scale=None):
    """q (Tq, N, D), kv (Tk, N, 2D) -> out (Tq, N, D), cache (lse (Tq, N, heads) in it)."""
    q, kv = np.asarray(q, np.float64), np.asarray(kv, np.float64)
    Tq, N, D = q.shape
    Tk = kv.shape[0]
    dh = D // heads
    scale = 1.0 / np.sqrt(dh) if scale is None else scale
    ql, kl = clamp_lens(q_lens, k_lens, N, Tq, Tk)
    out = np.zeros((Tq, N, D))
    lse = np.zeros((Tq, N, heads))
    ps = {}
    for n in range(N):
        for h in range(heads):
            cols = slice(h * dh, (h + 1) * dh)
            qh = q[:ql[n], n, cols]
            kh, vh = kv[:kl[n], n, cols], kv[:kl[n], n, D + h * dh:D + (h + 1) * dh]
            s = scale * (qh @ kh.T)
            m = s.max(axis=-1, keepdims=True) if s.size else np.zeros((0, 1))
            e = np.exp(s - m)
            l = e.sum(axis=-1, keepdims=True)
            p = e / l
            out[:ql[n], n, cols] = p @ vh
            lse[:ql[n], n, h] = (m + np.log(l))[:, 0]
            ps[n, h] = p
    return out, dict(q=q, kv=kv, heads=heads, scale=scale, ql=ql, kl=kl, p=ps, lse=lse, out=out)


def cross_backward(dout, c):
    """-> dq (Tq, N, D), dkv (Tk, N, 2D)."""
    q, kv, heads, scale = c['q'], c['kv'], c['heads'], c['scale']
    dout = np.asarray(dout, np.float64)
    Tq, N, D = q.shape
    dh = D // heads
    dq, dkv = np.zeros_like(q), np.zeros_like(kv)
    for n in range(N):
        a, k = c['ql'][n], c['kl'][n]
        for h in range(heads):
            cols = slice(h * dh, (h + 1) * dh)
            vcols = slice(D + h * dh, D + (h + 1) * dh)
            p, do = c['p'][n, h], dout[:a, n, cols]
            dp = do @ kv[:k, n, vcols].T
            ds = p * (dp - (dp * p).sum(axis=-1, keepdims=True))
            dq[:a, n, cols] = scale * (ds @ kv[:k, n, cols])
            dkv[:k, n, cols] = scale * (ds.T @ q[:a, n, cols])
            dkv[:k, n, vcols] = p.T @ do
    return dq, dkv


# ----------------------------------------------------------------------------- joint + loss
def targets(labels_n, u_n, C):
    """The u_n + 1 targets of one utterance: its labels (one outside 0 .. C - 2 counts as C - 1,
    as the kernel reads it), then EOS = C - 1."""
    y = [int(v) if 0 <= int(v) < C else C - 1 for v in labels_n[:u_n]]
    return np.asarray(y + [C - 1], int)


def loss_and_grads(ctx, q, W, b, labels, label_len, N, eps=0.0, grad_scale=1.0):
    """The slabs of the C ABI: ctx, q (U1, n_pad, J), W (J, C), b (C), labels (N, U1 - 1).
    Returns loss (N) and d_pre (= d_ctx = d_q), dW, db = grad_scale * d sum(loss) / d(.) in
    float64; rows n >= N and u > U_n are never read and stay 0."""
    ctx, q = np.asarray(ctx, np.float64), np.asarray(q, np.float64)
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    U1, C = ctx.shape[0], len(b)
    Un = np.clip(np.asarray(label_len), 0, U1 - 1).astype(int)
    loss = np.zeros(N)
    d_pre = np.zeros_like(ctx)
    dW, db = np.zeros_like(W), np.zeros_like(b)
    for n in range(N):
        u_n = Un[n]
        h = np.tanh(ctx[:u_n + 1, n] + q[:u_n + 1, n])
        lp = log_softmax(h @ W + b)
        tgt = targets(labels[n] if u_n else [], u_n, C)
        rows = np.arange(u_n + 1)
        loss[n] = -((1.0 - eps) * lp[rows, tgt] + eps * lp.mean(axis=-1)).sum()
        dz = np.exp(lp) - eps / C
        dz[rows, tgt] -= 1.0 - eps
        dz *= grad_scale
        d_pre[:u_n + 1, n] = (dz @ W.T) * (1.0 - h * h)
        dW += h.T @ dz
        db += dz.sum(axis=0)
    return loss, d_pre, dW, db


# ----------------------------------------------------------------------------- greedy decoding
def first_argmax(z):
    return int(np.argmax(z))          # NumPy returns the FIRST maximum


def greedy_naive(kv_n, W, b, heads, pred_init, pred_step, max_labels=255, scale=None,
                 margins=None):
    """One utterance, the textbook loop.  kv_n (T_n, 2D): the encoder's [K | V] rows of the valid
    frames.  pred_init(1) -> (state, q) for the start-of-sequence input, pred_step(state, x (1,
    C - 1)) -> (state', q'), q (1, D).  Per label: attend with the current query, score the joint,
    stop on EOS (C - 1) or after max_labels labels.  margins: a list that receives every step's
    gap between the two largest logits."""
    C = len(b)
    W, b = np.float64(W), np.float64(b)
    state, qv = pred_init(1)
    out = []
    while True:
        ctx, _ = cross_forward(np.float64(qv).reshape(1, 1, -1), np.float64(kv_n)[:, None, :],
                               heads, scale=scale)
        z = np.tanh(ctx[0, 0] + np.float64(qv)[0]) @ W + b
        if margins is not None:
            top = np.sort(z)
            margins.append(float(top[-1] - top[-2]))
        k = first_argmax(z)
        if k == C - 1 or len(out) >= max_labels:
            return out
        out.append(k)
        if len(out) >= max_labels:
            return out
        x = np.zeros((1, C - 1), np.float32)
        x[0, k] = 1.0
        state, qv = pred_step(state, x)
