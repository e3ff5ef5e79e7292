"""float64 NumPy restatement of the LayerNormalization layer (per frame, over the feature axis;
arXiv 1607.06450) and of the model chains that use it, composed with oracle.conv, oracle.lstm,
oracle.ctc, tests/batchnorm_oracle, tests/simple_rnn_oracle and tests/gru_oracle.  Test
infrastructure only.

The layer, for every frame (n, t) of a (T, N, F) tensor:
    y = (x - mu) / sqrt(var + eps) * gain + bias
mu and the BIASED variance over the F features of that one frame, eps inside the square root.
No mask (a zero frame gives y = bias), no phase: training and inference are the same map.
On the (N, T, F, C) conv image the F * C features of a frame are one group.
"""
import numpy as np

from oracle import conv as _conv
from oracle import ctc as _ctc
from oracle import lstm as _lstm
from tests import batchnorm_oracle as BO
from tests import gru_oracle as GO
from tests import simple_rnn_oracle as SR


# ----------------------------------------------------------------------------- the layer
def ln_forward(x, gain, bias, eps=1e-5):
    """x (..., F) -> y, cache (mean, var, r = 1 / sqrt(var + eps), xhat)."""
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    r = 1.0 / np.sqrt(var + eps)
    xhat = (x - mu) * r
    return xhat * gain + bias, dict(mean=mu[..., 0], var=var[..., 0], r=r[..., 0], xhat=xhat,
                                    gain=gain)


def ln_backward(dy, c):
    """-> dx, dgain, dbias."""
    xhat, r, gain = c['xhat'], c['r'][..., None], c['gain']
    g = dy * gain
    dx = r * (g - g.mean(axis=-1, keepdims=True)
              - xhat * (g * xhat).mean(axis=-1, keepdims=True))
    axes = tuple(range(dy.ndim - 1))
    return dx, (dy * xhat).sum(axis=axes), dy.sum(axis=axes)


def real_columns(H, Hp, segs=1):
    """Physical columns of a slab row that carry features: segs blocks of H at a stride of Hp."""
    return np.concatenate([k * Hp + np.arange(H) for k in range(segs)])


# ----------------------------------------------------------------------------- model chains
_COUNT = {'conv': 2, 'dense': 2, 'bn': 4, 'ln': 2, 'bilstm': 6, 'birnn': 6, 'bigru': 6}


def stages_from_model(model):
    """Oracle stage list (float64 weights), index-aligned with model.stages: noise (0) and
    reshape pass through; conv, bn, ln, act, dropout (p = 0), dense, bilstm (plain cell),
    birnn, bigru (no batch_norm)."""
    it = iter([w.astype(np.float64) for w in model.get_weights()])
    out = []
    for s in model.stages:
        if s.kind in ('noise', 'reshape', 'dropout'):
            out.append(dict(type='pass'))
        elif s.kind == 'conv':
            out.append(dict(type='conv', W=next(it), b=next(it), stride=(s.st, s.sf),
                            clip=s.clip, l2=s.l2))
        elif s.kind == 'bn':
            out.append(dict(type='bn', gamma=next(it), beta=next(it), rm=next(it), rv=next(it),
                            eps=s.eps, momentum=s.momentum, C=s.C if s.grouped else None))
        elif s.kind == 'ln':
            out.append(dict(type='ln', gain=next(it), bias=next(it), eps=s.eps))
        elif s.kind == 'act':
            out.append(dict(type='act', act=s.act))
        elif s.kind == 'dense':
            out.append(dict(type='dense', W=next(it), b=next(it), l2=s.l2))
        elif s.kind in ('bilstm', 'birnn', 'bigru'):
            p = {d: dict(W=next(it), U=next(it), b=next(it)) for d in ('fwd', 'bwd')}
            out.append(dict(type=s.kind, p=p, act=getattr(s, 'act', 'tanh'),
                            merge=getattr(s, 'merge', 'concat'), l2_W=s.l2_W, l2_U=s.l2_U))
        else:
            raise NotImplementedError(s.kind)
    return out


def model_forward(stages, x, training=True, sides=None):
    """x (T, N, F) real rows -> logits, caches.  training matters to 'bn' stages only.  sides:
    {stage index: gates} of bigru stages (tests/gru_oracle.model_forward)."""
    sides = sides or {}
    a, caches = x, []
    for i, st in enumerate(stages):
        t, c = st['type'], None
        if t == 'conv':
            a, c = _conv.conv2d_forward(a, st['W'], st['b'], st['stride'], st['clip'])
        elif t == 'bn':
            if training:
                a, c = BO.bn_forward(a, st['gamma'], st['beta'], st['eps'], st['C'])
            else:
                a = BO.bn_infer(a, st['gamma'], st['beta'], st['rm'], st['rv'], st['eps'], st['C'])
        elif t == 'ln':
            a, c = ln_forward(a, st['gain'], st['bias'], st['eps'])
        elif t == 'act':
            a = SR.act_apply(st['act'], a)
            c = a
        elif t == 'dense':
            c = a
            a = a @ st['W'] + st['b']
        elif t == 'bilstm':
            outs, c = [], {}
            for d, rev in (('fwd', False), ('bwd', True)):
                p = st['p'][d]
                hs, c[d] = _lstm.lstm_forward(a, p['W'], p['U'], p['b'], rev)
                outs.append(hs)
            a = np.concatenate(outs, axis=-1)
        elif t == 'birnn':
            a, c = SR.birnn_forward(a, st['p'], st['act'], st['merge'])
        elif t == 'bigru':
            a, c = GO.bigru_forward(a, st['p'], st['act'], st['merge'])
            if i in sides:
                for d in range(2):
                    c['cs'][d]['sides'] = sides[i][:, :, d]
        caches.append(c)
    return a, caches


def model_backward(stages, caches, dlogits):
    """-> gradients in get_weights() order (zeros at BN running moments), input gradient."""
    da, out = dlogits, []
    for st, c in zip(reversed(stages), reversed(caches)):
        t = st['type']
        if t == 'conv':
            da, dW, db = _conv.conv2d_backward(da, c)
            out = [dW, db] + out
        elif t == 'bn':
            da, dg, dbeta = BO.bn_backward(da, c)
            out = [dg, dbeta, np.zeros_like(dg), np.zeros_like(dg)] + out
        elif t == 'ln':
            da, dg, db = ln_backward(da, c)
            out = [dg, db] + out
        elif t == 'act':
            da = da * SR.act_slope(st['act'], c)
        elif t == 'dense':
            out = [np.einsum('tnf,tnc->fc', c, da), da.sum(axis=(0, 1))] + out
            da = da @ st['W'].T
        elif t == 'bilstm':
            H = st['p']['fwd']['U'].shape[0]
            dx, g = None, []
            for d, sl in (('fwd', slice(0, H)), ('bwd', slice(H, 2 * H))):
                ddx, dW, dU, db = _lstm.lstm_backward(np.ascontiguousarray(da[..., sl]), c[d])
                g += [dW, dU, db]
                dx = ddx if dx is None else dx + ddx
            out = g + out
            da = dx
        elif t == 'birnn':
            da, g = SR.birnn_backward(da, c)
            out = [g[k][n] for k in ('fwd', 'bwd') for n in ('W', 'U', 'b')] + out
        elif t == 'bigru':
            da, g = GO.bigru_backward(da, c)
            out = [g[k][n] for k in ('fwd', 'bwd') for n in ('W', 'U', 'b')] + out
    return out, da


def loss_and_grads(stages, x, labels, seq_len, training=True, sides=None):
    """Mean CTC over the batch (no l2) and its gradients: dict(ctc, logits, grads, caches)."""
    logits, caches = model_forward(stages, x, training, sides)
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
        elif t == 'bn':
            out += [(st, 'gamma', 0.0), (st, 'beta', 0.0)]
        elif t == 'ln':
            out += [(st, 'gain', 0.0), (st, 'bias', 0.0)]
        elif t in ('bilstm', 'birnn', 'bigru'):
            for d in ('fwd', 'bwd'):
                out += [(st['p'][d], 'W', st['l2_W']), (st['p'][d], 'U', st['l2_U']),
                        (st['p'][d], 'b', 0.0)]
    return out


def grads_trainable(stages, grads):
    out, it = [], iter(grads)
    for st in stages:
        g = [next(it) for _ in range(_COUNT.get(st['type'], 0))]
        out += g[:2] if st['type'] == 'bn' else g
    return out


def weights(stages):
    """get_weights() order."""
    out = []
    for st in stages:
        t = st['type']
        if t in ('conv', 'dense'):
            out += [st['W'], st['b']]
        elif t == 'bn':
            out += [st['gamma'], st['beta'], st['rm'], st['rv']]
        elif t == 'ln':
            out += [st['gain'], st['bias']]
        elif t in ('bilstm', 'birnn', 'bigru'):
            out += [st['p'][d][k] for d in ('fwd', 'bwd') for k in ('W', 'U', 'b')]
    return out


def train_step(stages, x, labels, seq_len, opt, sides=None):
    """One optimisation step of the oracle: gradients + l2, then the optimiser (oracle.optim, on
    the trainable arrays in place) and the running-moment EMA of any BN stage.  Returns the
    step's loss_and_grads dict."""
    out = loss_and_grads(stages, x, labels, seq_len, True, sides)
    g = grads_trainable(stages, out['grads'])
    tr = trainable(stages)
    g = [gi + 2.0 * l2 * holder[k] if l2 else gi for gi, (holder, k, l2) in zip(g, tr)]
    opt.step([holder[k] for holder, k, _ in tr], g)
    for st, c in zip(stages, out['caches']):
        if st['type'] == 'bn':
            st['rm'] = BO.ema(st['rm'], c['mean'], st['momentum'])
            st['rv'] = BO.ema(st['rv'], c['var'], st['momentum'])
    return out
