"""float64 NumPy restatement of the Conformer pieces (arXiv 2005.08100): the masked depthwise
convolution over time, the gated linear unit, Swish, the scaled residual, and the model chains
that use them (dense / ln / bn / act / dropout(0) / merge / mha / posenc / conv / dwconv / glu),
built on tests/attention_oracle, layernorm_oracle, batchnorm_oracle, oracle.conv and oracle.ctc.
Test infrastructure only.

The convolution, k odd, p = (k - 1) / 2, w (k, C), x (T, N, C):
    xm[u, n, c] = x[u, n, c] if 0 <= u < lens[n] else 0
    y[t, n, c]  = b[c] + sum_j w[j, c] xm[t + j - p, n, c]       (cross-correlation, 'same')
Every frame t < T is an output; frames at or past an utterance's length count as padding.
"""
import numpy as np

from oracle import conv as _conv
from oracle import ctc as _ctc
from tests import attention_oracle as AO
from tests import batchnorm_oracle as BO
from tests import layernorm_oracle as LO
from tests import simple_rnn_oracle as SR


# ----------------------------------------------------------------------------- the pieces
def _mask(T, N, lens):
    lens = np.full(N, T) if lens is None else np.clip(np.asarray(lens).reshape(-1)[:N], 0, T)
    return np.arange(T)[:, None] < lens[None, :]                  # (T, N)


def dwconv_forward(x, w, b, lens=None):
    """x (T, N, C), w (k, C), b (C) -> y (T, N, C), cache."""
    T, N, C = x.shape
    k = w.shape[0]
    p = (k - 1) // 2
    m = _mask(T, N, lens)
    xp = np.zeros((T + 2 * p, N, C))
    xp[p:p + T] = np.where(m[:, :, None], x, 0.0)       # a select: junk past len cannot leak
    y = np.zeros((T, N, C)) + b
    for j in range(k):
        y += w[j] * xp[j:j + T]
    return y, dict(xp=xp, w=w, mask=m, p=p)


def dwconv_backward(dy, c):
    """-> dx, dw, db."""
    xp, w, m, p = c['xp'], c['w'], c['mask'], c['p']
    T, k = dy.shape[0], w.shape[0]
    dyp = np.zeros((T + 2 * p,) + dy.shape[1:])
    dyp[p:p + T] = dy
    dx = np.zeros_like(dy)
    dw = np.zeros_like(w)
    for j in range(k):
        dw[j] = (dy * xp[j:j + T]).sum(axis=(0, 1))
        dx += w[j] * dyp[2 * p - j:2 * p - j + T]       # dy[u - j + p]
    return np.where(m[:, :, None], dx, 0.0), dw, dy.sum(axis=(0, 1))


def dwconv_abs_terms(dy, c):
    """sum |terms| of dw and db: the size a long fp32 sum's error is measured against."""
    xp, w = c['xp'], c['w']
    T = dy.shape[0]
    aw = np.stack([(np.abs(dy) * np.abs(xp[j:j + T])).sum(axis=(0, 1))
                   for j in range(w.shape[0])])
    return aw, np.abs(dy).sum(axis=(0, 1))


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def glu_forward(x):
    C = x.shape[-1] // 2
    a, g = x[..., :C], x[..., C:2 * C]
    return a * sigmoid(g), x


def glu_backward(dy, x):
    C = x.shape[-1] // 2
    a, s = x[..., :C], sigmoid(x[..., C:2 * C])
    return np.concatenate([dy * s, dy * a * s * (1.0 - s)], axis=-1)


def swish(x):
    return x * sigmoid(x)


def swish_backward(dy, x):
    s = sigmoid(x)
    return dy * s * (1.0 + x * (1.0 - s))


# ----------------------------------------------------------------------------- model chains
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
        elif s.kind == 'bn':
            out.append(dict(type='bn', gamma=next(it), beta=next(it), rm=next(it), rv=next(it),
                            eps=s.eps, momentum=s.momentum, C=s.C if s.grouped else None))
        elif s.kind == 'act':
            out.append(dict(type='act', act=s.act))
        elif s.kind == 'dense':
            out.append(dict(type='dense', W=next(it), b=next(it), l2=s.l2))
        elif s.kind == 'mha':
            out.append(dict(type='mha', W_qkv=next(it), b_qkv=next(it), W_o=next(it),
                            b_o=next(it), heads=s.heads, l2=s.l2))
        elif s.kind == 'posenc':
            out.append(dict(type='posenc'))
        elif s.kind == 'dwconv':
            out.append(dict(type='dwconv', W=next(it), b=next(it), l2=s.l2))
        elif s.kind == 'glu':
            out.append(dict(type='glu'))
        elif s.kind == 'merge':
            out.append(dict(type='merge', skip=s.skip, coef=s.coef, scale=s.scale))
        else:
            raise NotImplementedError(s.kind)
    return out


def model_forward(stages, x, lens=None, training=True):
    """x (T, N, F) real rows, lens: INPUT lengths (strided by the conv stages on the way; None:
    every frame) -> logits, caches.  training: BN takes batch statistics (else running)."""
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
        elif t == 'bn':
            if training:
                a, c = BO.bn_forward(a, st['gamma'], st['beta'], st['eps'], st['C'])
            else:
                a = BO.bn_infer(a, st['gamma'], st['beta'], st['rm'], st['rv'], st['eps'],
                                st['C'])
        elif t == 'act' and st['act'] == 'swish':
            c = a
            a = swish(a)
        elif t == 'act':
            a = SR.act_apply(st['act'], a)
            c = a
        elif t == 'dense':
            c = a
            a = a @ st['W'] + st['b']
        elif t == 'mha':
            a, c = AO.mha_forward(a, st['W_qkv'], st['b_qkv'], st['W_o'], st['b_o'],
                                  st['heads'], lens)
        elif t == 'posenc':
            a = a + AO.posenc(a.shape[0], a.shape[2])[:, None, :]
        elif t == 'dwconv':
            a, c = dwconv_forward(a, st['W'], st['b'], lens)
        elif t == 'glu':
            a, c = glu_forward(a)
        elif t == 'merge':
            a = st['coef'] * (st['scale'] * a + outs[st['skip']])
        caches.append(c)
        outs.append(a)
    return a, caches


def model_backward(stages, caches, dlogits):
    """-> gradients in get_weights() order (zeros at the running moments), input gradient."""
    da, out, skip = dlogits, [], {}
    for i in range(len(stages) - 1, -1, -1):
        st, c = stages[i], caches[i]
        t = st['type']
        if i in skip:                   # the residual branch rejoins at this stage's output
            da = da + skip.pop(i)
        if t == 'merge':
            da = st['coef'] * da
            skip[st['skip']] = da
            da = st['scale'] * da       # the branch gets scale * d, the skip d
        elif t == 'conv':
            da, dW, db = _conv.conv2d_backward(da, c)
            out = [dW, db] + out
        elif t == 'ln':
            da, dg, db = LO.ln_backward(da, c)
            out = [dg, db] + out
        elif t == 'bn':
            da, dg, dbeta = BO.bn_backward(da, c)
            out = [dg, dbeta, np.zeros_like(dg), np.zeros_like(dg)] + out
        elif t == 'act' and st['act'] == 'swish':
            da = swish_backward(da, c)
        elif t == 'act':
            da = da * SR.act_slope(st['act'], c)
        elif t == 'dense':
            out = [np.einsum('tnf,tnc->fc', c, da), da.sum(axis=(0, 1))] + out
            da = da @ st['W'].T
        elif t == 'mha':
            da, g = AO.mha_backward(da, c)
            out = g + out
        elif t == 'dwconv':
            da, dw, db = dwconv_backward(da, c)
            out = [dw, db] + out
        elif t == 'glu':
            da = glu_backward(da, c)
    return out, da


def loss_and_grads(stages, x, labels, seq_len, training=True):
    """Mean CTC over the batch (no l2) and its gradients: dict(ctc, logits, grads, caches)."""
    logits, caches = model_forward(stages, x, seq_len, training)
    for st in stages:
        if st['type'] == 'conv':
            seq_len = _conv.out_lengths(seq_len, st['stride'][0])
    N = logits.shape[1]
    ctc_n, dlog = _ctc.ctc_loss_grad(logits, labels, seq_len, dtype=np.float64)
    grads, _ = model_backward(stages, caches, dlog / N)
    return dict(ctc=ctc_n, logits=logits, grads=grads, caches=caches)


_KEYS = {'conv': ('W', 'b'), 'dense': ('W', 'b'), 'dwconv': ('W', 'b'), 'ln': ('gain', 'bias'),
         'bn': ('gamma', 'beta', 'rm', 'rv'), 'mha': ('W_qkv', 'b_qkv', 'W_o', 'b_o')}
_L2 = ('W', 'W_qkv', 'W_o')


def trainable(stages):
    """The arrays Adam updates, get_weights() order (the running moments left out), with the l2
    factor of each."""
    return [(st, k, st['l2'] if k in _L2 else 0.0) for st in stages
            for k in _KEYS.get(st['type'], ()) if k not in ('rm', 'rv')]


def grads_trainable(stages, grads):
    """get_weights()-order gradients -> the trainable ones (running-moment zeros dropped)."""
    keys = [k for st in stages for k in _KEYS.get(st['type'], ())]
    return [g for g, k in zip(grads, keys) if k not in ('rm', 'rv')]


def weights(stages):
    """get_weights() order, running moments included."""
    return [st[k] for st in stages for k in _KEYS.get(st['type'], ())]


def train_step(stages, x, labels, seq_len, opt):
    """One optimisation step of the oracle: gradients + l2, the optimiser (oracle.optim, on the
    trainable arrays in place), then the running-moment EMA of every BN stage.  Returns the
    step's loss_and_grads dict."""
    out = loss_and_grads(stages, x, labels, seq_len, training=True)
    tr = trainable(stages)
    g = [gi + 2.0 * l2 * holder[k] if l2 else gi
         for gi, (holder, k, l2) in zip(grads_trainable(stages, out['grads']), tr)]
    opt.step([holder[k] for holder, k, _ in tr], g)
    for st, c in zip(stages, out['caches']):
        if st['type'] == 'bn':
            st['rm'] = BO.ema(st['rm'], c['mean'], st['momentum'])
            st['rv'] = BO.ema(st['rv'], c['var'], st['momentum'])
    return out


greedy = AO.greedy
