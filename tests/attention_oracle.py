"""float64 NumPy restatement of multi-head self-attention (arXiv 1706.03762) with a key mask by
utterance length, of the sinusoidal positional encoding, and of the model chains that use them
(dense / ln / act / dropout(0) / merge / mha / posenc / conv), built on tests/layernorm_oracle,
oracle.conv and oracle.ctc.  Test infrastructure only.

The attention core, per sample n and head h of [Q | K | V] (T, N, 3D), D = heads * dh:
    s[t, u] = scale q_t . k_u  for u < lens[n];  p = softmax_u(s), p = 0 for u >= lens[n];
    out_t = sum_u p[t, u] v_u;  lse_t = log sum_u exp s[t, u]
Every frame t < T is a query, time-padding frames included; only keys are masked.
"""
import numpy as np

from oracle import conv as _conv
from oracle import ctc as _ctc
from tests import layernorm_oracle as LO
from tests import simple_rnn_oracle as SR


# ----------------------------------------------------------------------------- the core
def attn_forward(qkv, heads, lens=None, scale=None):
    """qkv (T, N, 3D) -> out (T, N, D), cache (with p (N, heads, T, T) and lse (T, N, heads))."""
    T, N, D3 = qkv.shape
    D = D3 // 3
    dh = D // heads
    scale = 1.0 / np.sqrt(dh) if scale is None else scale
    lens = np.full(N, T) if lens is None else np.asarray(lens).reshape(-1)
    # (N, heads, T, dh) each: the products are batched matrix products
    q, k, v = [np.ascontiguousarray(qkv[:, :, i * D:(i + 1) * D].reshape(T, N, heads, dh)
                                    .transpose(1, 2, 0, 3)) for i in range(3)]
    s = q @ k.transpose(0, 1, 3, 2)
    s *= scale
    mask = (np.arange(T)[None, :] < lens[:N, None])[:, None, None, :]      # valid keys
    smax = np.abs(s).max(initial=0.0, where=mask)
    if not mask.all():
        s[np.broadcast_to(~mask, s.shape)] = -np.inf
    m = s.max(axis=-1, keepdims=True)
    s -= m
    p = np.exp(s, out=s)                        # (in place: the scores are not needed again)
    l = p.sum(axis=-1, keepdims=True)
    p /= l
    out = (p @ v).transpose(2, 0, 1, 3).reshape(T, N, D)
    lse = (m + np.log(l))[..., 0].transpose(2, 0, 1)
    return out, dict(q=q, k=k, v=v, p=p, lse=lse, scale=scale, out=out, smax=smax)


def attn_backward(dout, c):
    """-> dqkv (T, N, 3D)."""
    q, k, v, p, scale = c['q'], c['k'], c['v'], c['p'], c['scale']
    N, heads, T, dh = q.shape
    do = np.ascontiguousarray(dout.reshape(T, N, heads, dh).transpose(1, 2, 0, 3))
    pT = p.transpose(0, 1, 3, 2)
    dv = pT @ do
    dp = do @ v.transpose(0, 1, 3, 2)
    dp -= (dp * p).sum(axis=-1, keepdims=True)
    ds = np.multiply(dp, p, out=dp)
    dq = scale * (ds @ k)
    dk = scale * (ds.transpose(0, 1, 3, 2) @ q)
    return np.concatenate([a.transpose(2, 0, 1, 3).reshape(T, N, heads * dh)
                           for a in (dq, dk, dv)], axis=-1)


# ----------------------------------------------------------------------------- the layer
def mha_forward(x, W_qkv, b_qkv, W_o, b_o, heads, lens=None):
    """x (T, N, F) -> y (T, N, n_out), cache."""
    qkv = x @ W_qkv + b_qkv
    ctx, c = attn_forward(qkv, heads, lens)
    c.update(x=x, ctx=ctx, W_qkv=W_qkv, W_o=W_o)
    return ctx @ W_o + b_o, c


def mha_backward(dy, c):
    """-> dx, [dW_qkv, db_qkv, dW_o, db_o]."""
    dW_o = np.einsum('tnd,tno->do', c['ctx'], dy)
    db_o = dy.sum(axis=(0, 1))
    dqkv = attn_backward(dy @ c['W_o'].T, c)
    dW_qkv = np.einsum('tnf,tnd->fd', c['x'], dqkv)
    db_qkv = dqkv.sum(axis=(0, 1))
    return dqkv @ c['W_qkv'].T, [dW_qkv, db_qkv, dW_o, db_o]


def posenc(T, D):
    """The (T, D) table, computed in float64 and rounded to fp32 as the library uploads it:
    pe[t, 2i] = sin(t / 10000^(2i / D)), pe[t, 2i + 1] = cos(t / 10000^(2i / D))."""
    pe = np.zeros((T, D))
    t = np.arange(T, dtype=np.float64)
    for f in range(D):
        ang = t / 10000.0 ** (2.0 * (f // 2) / D)
        pe[:, f] = np.sin(ang) if f % 2 == 0 else np.cos(ang)
    return pe.astype(np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- model chains
_COUNT = {'conv': 2, 'dense': 2, 'ln': 2, 'mha': 4}


def stages_from_model(model):
    """Oracle stage list (float64 weights), index-aligned with model.stages."""
    it = iter([w.astype(np.float64) for w in model.get_weights()])
    out = []
    for s in model.stages:
        if s.kind in ('noise', 'reshape', 'dropout'):
            out.append(dict(type='pass'))
        elif s.kind == 'conv':
            out.append(dict(type='conv', W=next(it), b=next(it), stride=(s.st, s.sf),
                            clip=s.clip, l2=s.l2))
        elif s.kind == 'ln':
            out.append(dict(type='ln', gain=next(it), bias=next(it), eps=s.eps))
        elif s.kind == 'act':
            out.append(dict(type='act', act=s.act))
        elif s.kind == 'dense':
            out.append(dict(type='dense', W=next(it), b=next(it), l2=s.l2))
        elif s.kind == 'mha':
            out.append(dict(type='mha', W_qkv=next(it), b_qkv=next(it), W_o=next(it),
                            b_o=next(it), heads=s.heads, l2=s.l2))
        elif s.kind == 'posenc':
            out.append(dict(type='posenc'))
        elif s.kind == 'merge':
            out.append(dict(type='merge', skip=s.skip, coef=s.coef))
        else:
            raise NotImplementedError(s.kind)
    return out


def model_forward(stages, x, lens=None):
    """x (T, N, F) real rows, lens: INPUT lengths (strided by the conv stages on the way; None:
    every frame is a key) -> logits, caches.  No phase: training and inference are one map."""
    a, caches, outs = x, [], []
    lens = None if lens is None else np.asarray(lens).reshape(-1)
    for st in stages:
        t, c = st['type'], None
        if t == 'conv':
            a, c = _conv.conv2d_forward(a, st['W'], st['b'], st['stride'], st['clip'])
            if lens is not None:
                lens = _conv.out_lengths(lens, st['stride'][0])
        elif t == 'ln':
            a, c = LO.ln_forward(a, st['gain'], st['bias'], st['eps'])
        elif t == 'act':
            a = SR.act_apply(st['act'], a)
            c = a
        elif t == 'dense':
            c = a
            a = a @ st['W'] + st['b']
        elif t == 'mha':
            a, c = mha_forward(a, st['W_qkv'], st['b_qkv'], st['W_o'], st['b_o'], st['heads'],
                               lens)
        elif t == 'posenc':
            a = a + posenc(a.shape[0], a.shape[2])[:, None, :]
        elif t == 'merge':
            a = st['coef'] * (a + outs[st['skip']])
        caches.append(c)
        outs.append(a)
    return a, caches


def model_backward(stages, caches, dlogits):
    """-> gradients in get_weights() order, input gradient."""
    da, out, skip = dlogits, [], {}
    for i in range(len(stages) - 1, -1, -1):
        st, c = stages[i], caches[i]
        t = st['type']
        if i in skip:                   # the residual branch rejoins at this stage's output
            da = da + skip.pop(i)
        if t == 'merge':
            da = st['coef'] * da
            skip[st['skip']] = da
        elif t == 'conv':
            da, dW, db = _conv.conv2d_backward(da, c)
            out = [dW, db] + out
        elif t == 'ln':
            da, dg, db = LO.ln_backward(da, c)
            out = [dg, db] + out
        elif t == 'act':
            da = da * SR.act_slope(st['act'], c)
        elif t == 'dense':
            out = [np.einsum('tnf,tnc->fc', c, da), da.sum(axis=(0, 1))] + out
            da = da @ st['W'].T
        elif t == 'mha':
            da, g = mha_backward(da, c)
            out = g + out
    return out, da


def loss_and_grads(stages, x, labels, seq_len):
    """Mean CTC over the batch (no l2) and its gradients: dict(ctc, logits, grads, caches)."""
    logits, caches = model_forward(stages, x, seq_len)
    for st in stages:
        if st['type'] == 'conv':
            seq_len = _conv.out_lengths(seq_len, st['stride'][0])
    N = logits.shape[1]
    ctc_n, dlog = _ctc.ctc_loss_grad(logits, labels, seq_len, dtype=np.float64)
    grads, _ = model_backward(stages, caches, dlog / N)
    return dict(ctc=ctc_n, logits=logits, grads=grads, caches=caches)


def trainable(stages):
    """The arrays Adam updates, get_weights() order, with the l2 factor of each."""
    out = []
    for st in stages:
        t = st['type']
        if t in ('conv', 'dense'):
            out += [(st, 'W', st['l2']), (st, 'b', 0.0)]
        elif t == 'ln':
            out += [(st, 'gain', 0.0), (st, 'bias', 0.0)]
        elif t == 'mha':
            out += [(st, 'W_qkv', st['l2']), (st, 'b_qkv', 0.0), (st, 'W_o', st['l2']),
                    (st, 'b_o', 0.0)]
    return out


def weights(stages):
    """get_weights() order."""
    return [holder[k] for holder, k, _ in trainable(stages)]


def train_step(stages, x, labels, seq_len, opt):
    """One optimisation step of the oracle: gradients + l2, then the optimiser (oracle.optim, on
    the trainable arrays in place).  Returns the step's loss_and_grads dict."""
    out = loss_and_grads(stages, x, labels, seq_len)
    tr = trainable(stages)
    g = [gi + 2.0 * l2 * holder[k] if l2 else gi
         for gi, (holder, k, l2) in zip(out['grads'], tr)]
    opt.step([holder[k] for holder, k, _ in tr], g)
    return out


def greedy(logits, seq_len):
    """Best-path CTC decoding (blank = C - 1, repeats merged) of (T, N, C) logits."""
    C = logits.shape[2]
    hyps = []
    for n in range(logits.shape[1]):
        path = logits[:int(seq_len[n]), n].argmax(axis=-1)
        hyps.append([int(k) for i, k in enumerate(path)
                     if k != C - 1 and (i == 0 or k != path[i - 1])])
    return hyps
