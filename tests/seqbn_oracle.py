"""float64 NumPy restatement of sequence-wise batch normalisation of a recurrent layer's input
projection (Laurent et al., "Batch normalized recurrent neural networks", arXiv 1510.01378; the
form Deep Speech 2 publishes), as ``layers.GRU(batch_norm=True)`` computes it, and of the model
chains that use it, composed with tests/gru_oracle and tests/batchnorm_oracle.  Test
infrastructure only.

One channel per column of the projection p = (x (.) B_W) W.  R is the set of real rows (every
frame of every real sample), V the valid ones (t < min(len_n, T)):

    mu = mean_V p, var = mean_V (p - mu)^2 (biased), xhat = (p - mu) / sqrt(var + eps) on R,
    zx = gamma xhat + beta on R (beta takes the place of the layer's bias).

Backward, da the gradient of zx (non-zero on padded frames too):

    dbeta = sum_R da, dgamma = sum_R da xhat,
    dp = gamma istd da                                          on R \\ V
    dp = gamma istd (da - dbeta / |V| - xhat dgamma / |V|)      on V

(the sums that reach mu and var run over V, but every row of R feeds them its gradient).
Inference is the affine map with the running moments; those follow Keras' EMA
(batchnorm_oracle.ema) of the batch moments over V.
"""
import numpy as np

from oracle import conv as _conv
from oracle import ctc as _ctc
from tests import batchnorm_oracle as BO
from tests import gru_oracle as GO

ema = BO.ema


# ----------------------------------------------------------------------------- the layer
def valid_mask(T, N, lens=None):
    """(T, N) bool: frame t of sample n is valid (lens None: every frame)."""
    if lens is None:
        return np.ones((T, N), bool)
    lens = np.minimum(np.maximum(np.asarray(lens).reshape(-1)[:N], 0), T)
    return np.arange(T)[:, None] < lens[None, :]


def seqbn_forward(p, gamma, beta, lens=None, eps=1e-3):
    """Training phase.  p (T, N, W) real rows -> zx (T, N, W), cache."""
    T, N, _ = p.shape
    V = valid_mask(T, N, lens)
    nv = float(V.sum())
    mu = p[V].sum(axis=0) / nv
    var = ((p[V] - mu) ** 2).sum(axis=0) / nv
    istd = 1.0 / np.sqrt(var + eps)
    xhat = (p - mu) * istd
    return gamma * xhat + beta, dict(mean=mu, var=var, istd=istd, xhat=xhat, gamma=gamma, V=V,
                                     nv=nv)


def seqbn_backward(da, c):
    """-> dp, dgamma, dbeta."""
    xhat, istd, gamma, V, nv = c['xhat'], c['istd'], c['gamma'], c['V'], c['nv']
    dbeta = da.sum(axis=(0, 1))
    dgamma = (da * xhat).sum(axis=(0, 1))
    dp = gamma * istd * (da - V[..., None] * (dbeta / nv + xhat * (dgamma / nv)))
    return dp, dgamma, dbeta


def seqbn_infer(p, gamma, beta, running_mean, running_var, eps=1e-3):
    return gamma * (p - running_mean) / np.sqrt(running_var + eps) + beta


def moments_block(p, lens, weight, shift):
    """What asr_seqbn_fwd_train writes for the running update: [w, 0, 0, 0 | w d | w (var +
    d^2)], w = weight * |V|, d = mean - shift."""
    c = seqbn_forward(p, 1.0, 0.0, lens)[1]
    w = weight * c['nv']
    d = c['mean'] - shift
    return np.concatenate([[w, 0.0, 0.0, 0.0], w * d, w * (c['var'] + d * d)])


# ----------------------------------------------------------------------------- the GRU layer
def gru_bn_forward(x, q, act, lens, eps, BW=None, BU=None, reverse=False, training=True):
    """q: {W, U, gamma, beta, rm, rv} of one direction."""
    xm = x if BW is None else x * BW[None]
    p = xm @ q['W']
    if training:
        zx, bn = seqbn_forward(p, q['gamma'], q['beta'], lens, eps)
    else:
        zx, bn = seqbn_infer(p, q['gamma'], q['beta'], q['rm'], q['rv'], eps), None
    h, gates = GO.recurrence_forward(zx, q['U'], act, BU, reverse)
    return h, dict(x=x, W=q['W'], U=q['U'], act=act, BW=BW, BU=BU, reverse=reverse, h=h,
                   gates=gates, sides=None, bn=bn)


def gru_bn_backward(dh, c):
    """-> dx, dW, dU, dgamma, dbeta."""
    x, W, U, h, gates, BW, BU = c['x'], c['W'], c['U'], c['h'], c['gates'], c['BW'], c['BU']
    H = h.shape[-1]
    da = GO.recurrence_backward(dh, U, h, gates, c['act'], BU, c['reverse'], c['sides'])
    m = GO._prev(h, c['reverse'])
    if BU is not None:
        m = m * BU[None]
    dU = np.concatenate([np.einsum('tni,tnj->ij', m, da[..., :2 * H]),
                         np.einsum('tni,tnj->ij', gates[..., H:2 * H] * m, da[..., 2 * H:])],
                        axis=1)
    dp, dgamma, dbeta = seqbn_backward(da, c['bn'])
    xm = x if BW is None else x * BW[None]
    dW = np.einsum('tnf,tnh->fh', xm, dp)
    dx = dp @ W.T
    if BW is not None:
        dx = dx * BW[None]
    return dx, dW, dU, dgamma, dbeta


def bigru_bn_forward(x, st, lens, BW=None, BU=None, training=True):
    hs, cs = [], []
    for d, key in enumerate(('fwd', 'bwd')):
        h, c = gru_bn_forward(x, st['p'][key], st['act'], lens, st['eps'],
                              None if BW is None else BW[d], None if BU is None else BU[d],
                              reverse=d == 1, training=training)
        hs.append(h)
        cs.append(c)
    y = np.concatenate(hs, axis=-1) if st['merge'] == 'concat' else hs[0] + hs[1]
    return y, dict(cs=cs, merge=st['merge'], H=hs[0].shape[-1])


def bigru_bn_backward(dy, c):
    H = c['H']
    dx, out = 0.0, []
    for d in range(2):
        dh = dy[..., d * H:(d + 1) * H] if c['merge'] == 'concat' else dy
        dxd, dW, dU, dg, db = gru_bn_backward(dh, c['cs'][d])
        dx = dx + dxd
        out += [dW, dU, dg, db, np.zeros_like(dg), np.zeros_like(dg)]
    return dx, out


# ----------------------------------------------------------------------------- model chains
BN_KEYS = ('W', 'U', 'gamma', 'beta', 'rm', 'rv')


def stages_from_model(model):
    """gru_oracle.stages_from_model, with the bigru stages of GRU(batch_norm=True) as
    dict(type='bigru_bn', p={'fwd' / 'bwd': {W, U, gamma, beta, rm, rv}}, ...).  Index-aligned
    with model.stages."""
    it = iter([w.astype(np.float64) for w in model.get_weights()])
    out = []
    for s in model.stages:
        if s.kind in ('noise', 'reshape'):
            out.append(dict(type='pass'))
        elif s.kind == 'dropout':
            out.append(dict(type='dropout', p=s.value))
        elif s.kind == 'conv':
            out.append(dict(type='conv', W=next(it), b=next(it), stride=(s.st, s.sf),
                            clip=s.clip, l2=s.l2))
        elif s.kind == 'bn':
            out.append(dict(type='bn', gamma=next(it), beta=next(it), rm=next(it), rv=next(it),
                            eps=s.eps, momentum=s.momentum, C=s.C if s.grouped else None))
        elif s.kind == 'act':
            out.append(dict(type='act', act=s.act))
        elif s.kind == 'dense':
            out.append(dict(type='dense', W=next(it), b=next(it), l2=s.l2))
        elif s.kind == 'bigru' and s.bn:
            p = {d: {k: next(it) for k in BN_KEYS} for d in ('fwd', 'bwd')}
            out.append(dict(type='bigru_bn', p=p, act=s.act, merge=s.merge, l2_W=s.l2_W,
                            l2_U=s.l2_U, eps=s.bn_eps, momentum=s.bn_momentum))
        elif s.kind == 'bigru':
            p = {d: dict(W=next(it), U=next(it), b=next(it)) for d in ('fwd', 'bwd')}
            out.append(dict(type='bigru', p=p, act=s.act, merge=s.merge, l2_W=s.l2_W,
                            l2_U=s.l2_U))
        else:
            raise NotImplementedError(s.kind)
    return out


def rec_lengths(stages, seq_len):
    """Input lengths -> lengths on the recurrent stack's time axis (None stays None)."""
    if seq_len is None:
        return None
    for st in stages:
        if st['type'] == 'conv':
            seq_len = _conv.out_lengths(seq_len, st['stride'][0])
    return np.asarray(seq_len)


def model_forward(stages, x, masks=None, sides=None, training=True, seq_len=None):
    """gru_oracle.model_forward with seq_len, the INPUT lengths (None: every frame is valid)."""
    masks, sides = masks or {}, sides or {}
    lens = rec_lengths(stages, seq_len)
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
        elif t == 'act':
            a = GO.act_apply(st['act'], a)
            c = a
        elif t == 'dense':
            c = a
            a = a @ st['W'] + st['b']
        elif t in ('bigru', 'bigru_bn'):
            BW, BU = masks.get(i, (None, None))
            if t == 'bigru':
                a, c = GO.bigru_forward(a, st['p'], st['act'], st['merge'], BW, BU)
            else:
                a, c = bigru_bn_forward(a, st, lens, BW, BU, training)
            if i in sides:
                for d in range(2):
                    c['cs'][d]['sides'] = sides[i][:, :, d]
        caches.append(c)
    return a, caches


def model_backward(stages, caches, dlogits):
    """-> gradients in get_weights() order (zeros at the running moments)."""
    da, out = dlogits, []
    for st, c in zip(reversed(stages), reversed(caches)):
        t = st['type']
        if t == 'conv':
            da, dW, db = _conv.conv2d_backward(da, c)
            out = [dW, db] + out
        elif t == 'bn':
            da, dg, dbeta = BO.bn_backward(da, c)
            out = [dg, dbeta, np.zeros_like(dg), np.zeros_like(dg)] + out
        elif t == 'act':
            da = da * GO.act_slope(st['act'], c)
        elif t == 'dense':
            out = [np.einsum('tnf,tnc->fc', c, da), da.sum(axis=(0, 1))] + out
            da = da @ st['W'].T
        elif t == 'bigru':
            da, g = GO.bigru_backward(da, c)
            out = [g[k][n] for k in ('fwd', 'bwd') for n in ('W', 'U', 'b')] + out
        elif t == 'bigru_bn':
            da, g = bigru_bn_backward(da, c)
            out = g + out
    return out


def loss_and_grads(stages, x, labels, seq_len, masks=None, sides=None):
    """Mean CTC over the batch (no l2) and its gradients: dict(ctc (N,), logits, grads, caches)."""
    logits, caches = model_forward(stages, x, masks, sides, True, seq_len)
    N = logits.shape[1]
    ctc_n, dlog = _ctc.ctc_loss_grad(logits, labels, rec_lengths(stages, seq_len),
                                     dtype=np.float64)
    grads = model_backward(stages, caches, dlog / N)
    return dict(ctc=ctc_n, logits=logits, grads=grads, caches=caches)


def trainable(stages):
    out = []
    for st in stages:
        if st['type'] == 'bigru_bn':
            for d in ('fwd', 'bwd'):
                out += [(st['p'][d], 'W', st['l2_W']), (st['p'][d], 'U', st['l2_U']),
                        (st['p'][d], 'gamma', 0.0), (st['p'][d], 'beta', 0.0)]
        else:
            out += GO.trainable([st])
    return out


def grads_trainable(stages, grads):
    out, it = [], iter(grads)
    for st in stages:
        t = st['type']
        n = {'conv': 2, 'dense': 2, 'bn': 4, 'bigru': 6, 'bigru_bn': 12}.get(t, 0)
        g = [next(it) for _ in range(n)]
        if t == 'bn':
            g = g[:2]
        elif t == 'bigru_bn':
            g = g[0:4] + g[6:10]
        out += g
    return out


def weights(stages):
    """get_weights() order, running moments included."""
    out = []
    for st in stages:
        if st['type'] == 'bigru_bn':
            out += [st['p'][d][k] for d in ('fwd', 'bwd') for k in BN_KEYS]
        else:
            out += GO.weights([st])
    return out


def train_step(stages, x, labels, seq_len, opt, masks=None, sides=None):
    """One optimisation step of the oracle: gradients + l2, the optimiser (oracle.optim, in place),
    then the running-moment EMA of every BN stage and every batch-normalised GRU direction."""
    out = loss_and_grads(stages, x, labels, seq_len, masks, sides)
    g = grads_trainable(stages, out['grads'])
    tr = trainable(stages)
    g = [gi + 2.0 * l2 * holder[k] if l2 else gi for gi, (holder, k, l2) in zip(g, tr)]
    opt.step([holder[k] for holder, k, _ in tr], g)
    for st, c in zip(stages, out['caches']):
        if st['type'] == 'bn':
            st['rm'] = ema(st['rm'], c['mean'], st['momentum'])
            st['rv'] = ema(st['rv'], c['var'], st['momentum'])
        elif st['type'] == 'bigru_bn':
            for d, key in enumerate(('fwd', 'bwd')):
                q, bn = st['p'][key], c['cs'][d]['bn']
                q['rm'] = ema(q['rm'], bn['mean'], st['momentum'])
                q['rv'] = ema(q['rv'], bn['var'], st['momentum'])
    return out
