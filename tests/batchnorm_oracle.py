"""float64 NumPy restatement of BatchNormalization (Keras 1.2.2, mode 0, axis -1) and of the
model chains that use it (deep_speech2(batch_norm=True), Dense -> BN -> Activation ->
Bidirectional(SimpleRNN)), composed with oracle.conv, oracle.lstm, oracle.ctc and
tests/simple_rnn_oracle.  Test infrastructure only.

Rules recalled from Keras 1.2.2 and TensorFlow 1.x (neither can run here, so these are unpinned):
* [recalled: keras/layers/normalization.py BatchNormalization.call, mode 0] training phase:
  K.normalize_batch_in_training over every axis but the last -> tf.nn.moments, i.e. the batch
  mean and the BIASED variance; y = gamma (x - mean) / sqrt(var + epsilon) + beta.
* [recalled: same, inference phase] K.batch_normalization with running_mean / running_std, where
  running_std holds the variance despite its name.
* [recalled: keras/backend/tensorflow_backend.py moving_average_update] r <- r momentum + value
  (1 - momentum), no zero-debias; running_mean starts at 0, running_std at 1.
* [recalled: BatchNormalization.build] weights gamma ('one'), beta ('zero'), running_mean,
  running_std; the last two are not trainable.
The rows a model feeds are its real samples (batch padding excluded); time-padding frames of
the zero-padded batch are included, as Keras sees them.
"""
import numpy as np

from oracle import conv as _conv
from oracle import ctc as _ctc
from oracle import lstm as _lstm
from tests import simple_rnn_oracle as SR


# ----------------------------------------------------------------------------- the layer
def _groups(x, C):
    T, N, W = x.shape
    C = W if C is None else int(C)
    return x.reshape(T, N, W // C, C), C


def bn_forward(x, gamma, beta, eps=1e-3, C=None, clip=0.0):
    """Training phase.  x (T, N, W) real rows; channel = column % C (C None: W).
    -> y (T, N, W), cache (mean, var, invstd, xhat, ...)."""
    xr, C = _groups(x, C)
    mu = xr.mean(axis=(0, 1, 2))
    var = ((xr - mu) ** 2).mean(axis=(0, 1, 2))
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = (xr - mu) * invstd
    z = gamma * xhat + beta
    y = np.minimum(np.maximum(z, 0.0), clip) if clip > 0 else z
    return y.reshape(x.shape), dict(mean=mu, var=var, invstd=invstd, xhat=xhat, z=z,
                                    gamma=gamma, clip=clip, shape=x.shape)


def bn_backward(dy, c):
    """-> dx, dgamma, dbeta."""
    xhat, invstd, gamma = c['xhat'], c['invstd'], c['gamma']
    g = dy.reshape(xhat.shape)
    if c['clip'] > 0:
        g = g * ((c['z'] > 0.0) & (c['z'] < c['clip']))
    dbeta = g.sum(axis=(0, 1, 2))
    dgamma = (g * xhat).sum(axis=(0, 1, 2))
    dx = gamma * invstd * (g - g.mean(axis=(0, 1, 2)) - xhat * (g * xhat).mean(axis=(0, 1, 2)))
    return dx.reshape(c['shape']), dgamma, dbeta


def bn_infer(x, gamma, beta, running_mean, running_var, eps=1e-3, C=None, clip=0.0):
    xr, C = _groups(x, C)
    z = gamma * (xr - running_mean) / np.sqrt(running_var + eps) + beta
    y = np.minimum(np.maximum(z, 0.0), clip) if clip > 0 else z
    return y.reshape(x.shape)


def ema(running, batch, momentum):
    return momentum * running + (1.0 - momentum) * batch


# ----------------------------------------------------- the data-parallel running-update bookkeeping
def moments_block(x, weight, shift, C=None):
    """What asr_bn_fwd_train writes for the running update: [w, 0, 0, 0 | w d | w (var + d^2)],
    d = mean - shift, from this rank's real rows x (T, N, W) (float64 here)."""
    xr, C = _groups(x, C)
    mu = xr.mean(axis=(0, 1, 2))
    var = ((xr - mu) ** 2).mean(axis=(0, 1, 2))
    d = mu - shift
    return np.concatenate([[weight, 0.0, 0.0, 0.0], weight * d, weight * (var + d * d)])


def update_from_moments(running_mean, running_var, block, momentum, shift=None):
    """What asr_bn_update_running does with a (summed) moments block."""
    C = running_mean.size
    w = block[0]
    if not w > 0:
        return running_mean.copy(), running_var.copy()
    d = block[4:4 + C] / w
    r = running_mean if shift is None else shift
    var = np.maximum(block[4 + C:4 + 2 * C] / w - d * d, 0.0)
    return ema(running_mean, r + d, momentum), ema(running_var, var, momentum)


# ----------------------------------------------------------------------------- model chains
def stages_from_model(model):
    """Oracle stage list (float64 weights) from an engine.Model whose stages are noise (0),
    reshape, conv, bn, act, dropout (p = 0), dense, bilstm (plain cell) or birnn."""
    it = iter([w.astype(np.float64) for w in model.get_weights()])
    out = []
    for s in model.stages:
        if s.kind in ('noise', 'reshape'):
            continue
        if s.kind == 'dropout':
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
        elif s.kind == 'bilstm':
            p = {d: dict(W=next(it), U=next(it), b=next(it)) for d in ('fwd', 'bwd')}
            out.append(dict(type='bilstm', p=p, l2_W=s.l2_W, l2_U=s.l2_U))
        elif s.kind == 'birnn':
            p = {d: dict(W=next(it), U=next(it), b=next(it)) for d in ('fwd', 'bwd')}
            out.append(dict(type='birnn', p=p, act=s.act, merge=s.merge, l2_W=s.l2_W,
                            l2_U=s.l2_U))
        else:
            raise NotImplementedError(s.kind)
    return out


def model_forward(stages, x, training=True):
    """x (T, N, F) real rows -> logits, caches.  training: batch statistics (else running)."""
    a, caches = x, []
    for st in stages:
        t = st['type']
        if t == 'conv':
            a, c = _conv.conv2d_forward(a, st['W'], st['b'], st['stride'], st['clip'])
        elif t == 'bn':
            if training:
                a, c = bn_forward(a, st['gamma'], st['beta'], st['eps'], st['C'])
            else:
                a, c = bn_infer(a, st['gamma'], st['beta'], st['rm'], st['rv'], st['eps'],
                                st['C']), None
        elif t == 'act':
            a = SR.act_apply(st['act'], a)
            c = a
        elif t == 'dropout':
            c = None
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
        caches.append(c)
    return a, caches


def model_backward(stages, caches, dlogits):
    """-> gradients in get_weights() order (zeros at the running moments), input gradient."""
    da, out = dlogits, []
    for st, c in zip(reversed(stages), reversed(caches)):
        t = st['type']
        if t == 'conv':
            da, dW, db = _conv.conv2d_backward(da, c)
            out = [dW, db] + out
        elif t == 'bn':
            da, dg, dbeta = bn_backward(da, c)
            out = [dg, dbeta, np.zeros_like(dg), np.zeros_like(dg)] + out
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
    return out, da


def trainable(stages):
    """The arrays Adam updates, get_weights() order (the running moments left out), with the
    l2 factor of each."""
    out = []
    for st in stages:
        t = st['type']
        if t in ('conv', 'dense'):
            out += [(st, 'W', st['l2']), (st, 'b', 0.0)]
        elif t == 'bn':
            out += [(st, 'gamma', 0.0), (st, 'beta', 0.0)]
        elif t in ('bilstm', 'birnn'):
            for d in ('fwd', 'bwd'):
                out += [(st['p'][d], 'W', st['l2_W']), (st['p'][d], 'U', st['l2_U']),
                        (st['p'][d], 'b', 0.0)]
    return out


def grads_trainable(stages, grads):
    """get_weights()-order gradients -> the trainable ones (running-moment zeros dropped)."""
    out, it = [], iter(grads)
    for st in stages:
        t = st['type']
        n = {'conv': 2, 'dense': 2, 'bn': 4, 'bilstm': 6, 'birnn': 6}.get(t, 0)
        g = [next(it) for _ in range(n)]
        out += g[:2] if t == 'bn' else g
    return out


def loss_and_grads(stages, x, labels, seq_len, training=True):
    """Mean CTC over the batch (no l2) and its gradients: dict(ctc, logits, grads)."""
    logits, caches = model_forward(stages, x, training)
    for st in stages:
        if st['type'] == 'conv':
            seq_len = _conv.out_lengths(seq_len, st['stride'][0])
    N = logits.shape[1]
    ctc_n, dlog = _ctc.ctc_loss_grad(logits, labels, seq_len, dtype=np.float64)
    grads, _ = model_backward(stages, caches, dlog / N)
    return dict(ctc=ctc_n, logits=logits, grads=grads, caches=caches)


def weights(stages):
    """get_weights() order, running moments included."""
    out = []
    for st in stages:
        t = st['type']
        if t in ('conv', 'dense'):
            out += [st['W'], st['b']]
        elif t == 'bn':
            out += [st['gamma'], st['beta'], st['rm'], st['rv']]
        elif t in ('bilstm', 'birnn'):
            out += [st['p'][d][k] for d in ('fwd', 'bwd') for k in ('W', 'U', 'b')]
    return out


def train_step(stages, x, labels, seq_len, opt):
    """One optimisation step of the oracle: gradients + l2, the optimiser (oracle.optim, on the
    trainable arrays in place), then the running-moment EMA of every BN stage from the batch
    moments of this step's forward pass.  Returns the step's loss_and_grads dict."""
    out = loss_and_grads(stages, x, labels, seq_len, training=True)
    g = grads_trainable(stages, out['grads'])
    tr = trainable(stages)
    g = [gi + 2.0 * l2 * holder[k] if l2 else gi for gi, (holder, k, l2) in zip(g, tr)]
    arrays = [holder[k] for holder, k, _ in tr]
    opt.step(arrays, g)
    for st, c in zip(stages, out['caches']):
        if st['type'] == 'bn':
            st['rm'] = ema(st['rm'], c['mean'], st['momentum'])
            st['rv'] = ema(st['rv'], c['var'], st['momentum'])
    return out
