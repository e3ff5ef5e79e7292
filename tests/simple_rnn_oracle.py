"""float64 NumPy restatement of the SimpleRNN models (core/models.py maas / deep_speech): the
Keras-1.2.2 SimpleRNN step, Bidirectional('concat' / 'sum'), Dense, Activation and Dropout,
forward and backward, composed with oracle.ctc for the CTC objective.  Test infrastructure
only.

Rules recalled from Keras 1.2.2 (it cannot run here, so these are unpinned):
* [recalled: keras/layers/recurrent.py SimpleRNN.step] h_t = act(x_t W + b + (h_{t-1} B_U) U),
  h_0 = 0; with consume_less='cpu' (the factories' default) dropout_W is applied to x inside
  time_distributed_dense with ONE mask per (sample, feature) repeated over time, which equals
  the per-step (x_t B_W) form used here.
* [recalled: keras/layers/wrappers.py Bidirectional] the backward copy runs on the reversed
  sequence (go_backwards) and its output is reversed back; merge 'concat' = [h_f | h_b],
  'sum' = h_f + h_b.
* [recalled: keras/activations.py relu(x, max_value)] clipped ReLU min(max(x, 0), max_value);
  its derivative is taken as 1 on 0 < h < max_value (the end points count as clipped).
"""
import numpy as np

from oracle import ctc as _ctc


def act_apply(act, z):
    if isinstance(act, (tuple, list)) and act[0] == 'clipped_relu':
        return np.minimum(np.maximum(z, 0.0), float(act[1]))
    if act == 'tanh':
        return np.tanh(z)
    if act == 'relu':
        return np.maximum(z, 0.0)
    if act == 'linear':
        return z
    raise NotImplementedError(act)


def act_slope(act, h):
    """act'(z) written in terms of h = act(z)."""
    if isinstance(act, (tuple, list)) and act[0] == 'clipped_relu':
        return ((h > 0.0) & (h < float(act[1]))).astype(h.dtype)
    if act == 'tanh':
        return 1.0 - h * h
    if act == 'relu':
        return (h > 0.0).astype(h.dtype)
    if act == 'linear':
        return np.ones_like(h)
    raise NotImplementedError(act)


def _order(T, reverse):
    return list(range(T - 1, -1, -1)) if reverse else list(range(T))


# ---------------------------------------------------------------- the recurrence alone
def recurrence_forward(zx, U, act, BU=None, reverse=False):
    """zx (T, N, H) = x W + b -> h (T, N, H) in frame order."""
    T, N, H = zx.shape
    h = np.zeros_like(zx)
    prev = np.zeros((N, H), zx.dtype)
    for t in _order(T, reverse):
        hp = prev if BU is None else prev * BU
        h[t] = act_apply(act, zx[t] + hp @ U)
        prev = h[t]
    return h


def recurrence_backward(dy, U, h, act, BU=None, reverse=False):
    """dy (T, N, H) gradient of h -> dz (T, N, H) gradient of the pre-activation."""
    T, N, H = dy.shape
    dz = np.zeros_like(dy)
    carry = np.zeros((N, H), dy.dtype)
    for t in reversed(_order(T, reverse)):
        dz[t] = (dy[t] + carry) * act_slope(act, h[t])
        carry = dz[t] @ U.T
        if BU is not None:
            carry = carry * BU
    return dz


def kernel_forward(zx2, U2, act, BU2=None):
    """The C ABI's view: zx (T, N, 2, H), U (2, H, H), B_U (2, N, H) -> h (T, N, 2, H)."""
    return np.stack([recurrence_forward(zx2[:, :, d], U2[d], act,
                                        None if BU2 is None else BU2[d], reverse=d == 1)
                     for d in range(2)], axis=2)


def kernel_backward(dy, U2, h2, act, BU2=None, shared=False):
    """dy (T, N, H) shared by both directions ('sum') or (T, N, 2, H) -> dz (T, N, 2, H)."""
    return np.stack([recurrence_backward(dy if shared else dy[:, :, d], U2[d], h2[:, :, d], act,
                                         None if BU2 is None else BU2[d], reverse=d == 1)
                     for d in range(2)], axis=2)


# ---------------------------------------------------------------- layers
def rnn_forward(x, W, U, b, act, BW=None, BU=None, reverse=False):
    xm = x if BW is None else x * BW[None]
    zx = xm @ W + b
    h = recurrence_forward(zx, U, act, BU, reverse)
    return h, dict(x=x, W=W, U=U, act=act, BW=BW, BU=BU, reverse=reverse, h=h)


def rnn_backward(dh, c):
    x, W, U, h, BW, BU = c['x'], c['W'], c['U'], c['h'], c['BW'], c['BU']
    T, N, H = h.shape
    dz = recurrence_backward(dh, U, h, c['act'], BU, c['reverse'])
    xm = x if BW is None else x * BW[None]
    dW = np.einsum('tnf,tnh->fh', xm, dz)
    db = dz.sum(axis=(0, 1))
    dx = dz @ W.T
    if BW is not None:
        dx = dx * BW[None]
    # h_prev of frame t: h one frame earlier in the processing order
    hp = np.zeros_like(h)
    if c['reverse']:
        hp[:-1] = h[1:]
    else:
        hp[1:] = h[:-1]
    if BU is not None:
        hp = hp * BU[None]
    dU = np.einsum('tni,tnj->ij', hp, dz)
    return dx, dW, dU, db, dz


def birnn_forward(x, p, act, merge, BW=None, BU=None):
    """p: {'fwd': {W, U, b}, 'bwd': {...}}; BW (2, N, F), BU (2, N, H)."""
    hs, cs = [], []
    for d, key in enumerate(('fwd', 'bwd')):
        h, c = rnn_forward(x, p[key]['W'], p[key]['U'], p[key]['b'], act,
                           None if BW is None else BW[d], None if BU is None else BU[d],
                           reverse=d == 1)
        hs.append(h)
        cs.append(c)
    y = np.concatenate(hs, axis=-1) if merge == 'concat' else hs[0] + hs[1]
    return y, dict(cs=cs, merge=merge, H=hs[0].shape[-1])


def birnn_backward(dy, c):
    H = c['H']
    dx, grads = 0.0, {}
    for d, key in enumerate(('fwd', 'bwd')):
        dh = (dy[..., d * H:(d + 1) * H] if c['merge'] == 'concat' else dy)
        dxd, dW, dU, db, _ = rnn_backward(dh, c['cs'][d])
        dx = dx + dxd
        grads[key] = dict(W=dW, U=dU, b=db)
    return dx, grads


# ---------------------------------------------------------------- models
def stages_from_model(model):
    """The oracle's stage list (float64 weights) from an engine.Model of SimpleRNN / Dense /
    Activation / Dropout stages."""
    it = iter([w.astype(np.float64) for w in model.get_weights()])
    out = []
    for s in model.stages:
        if s.kind == 'dense':
            out.append(dict(type='dense', W=next(it), b=next(it)))
        elif s.kind == 'act':
            out.append(dict(type='act', act=s.act))
        elif s.kind == 'dropout':
            out.append(dict(type='dropout', p=s.value))
        elif s.kind == 'birnn':
            p = {}
            for key in ('fwd', 'bwd'):
                p[key] = dict(W=next(it), U=next(it), b=next(it))
            out.append(dict(type='birnn', p=p, act=s.act, merge=s.merge))
        else:
            raise NotImplementedError(s.kind)
    return out


def model_forward(stages, x, masks=None, kinks=None):
    """x (T, N, F) -> logits (T, N, C).  masks: {stage index: array} -- Dropout: the keep mask
    (T, N, F) with the inverted scale folded in; birnn: (B_W (2, N, F), B_U (2, N, H)).
    kinks: {stage index: array} -- the outputs (Activation: y, birnn: h (T, N, 2, H)) the
    backward pass takes its activation derivatives from instead of the oracle's own (at wide
    layers some pre-activations sit within rounding distance of a ReLU kink, where two correct
    computations may pick different sides)."""
    masks, kinks = masks or {}, kinks or {}
    a, caches = x, []
    for i, st in enumerate(stages):
        if st['type'] == 'dense':
            caches.append(a)
            a = a @ st['W'] + st['b']
        elif st['type'] == 'act':
            a = act_apply(st['act'], a)
            caches.append(kinks.get(i, a))
        elif st['type'] == 'dropout':
            m = masks.get(i)
            caches.append(m)
            if m is not None:
                a = a * m
        elif st['type'] == 'birnn':
            BW, BU = masks.get(i, (None, None))
            a, c = birnn_forward(a, st['p'], st['act'], st['merge'], BW, BU)
            if i in kinks:
                for d in range(2):
                    c['cs'][d]['h'] = kinks[i][:, :, d]
            caches.append(c)
    return a, caches


def model_backward(stages, caches, dlogits):
    """-> gradients in get_weights() (Keras) order."""
    da, out = dlogits, []
    for st, c in zip(reversed(stages), reversed(caches)):
        if st['type'] == 'dense':
            out = [np.einsum('tnf,tnc->fc', c, da), da.sum(axis=(0, 1))] + out
            da = da @ st['W'].T
        elif st['type'] == 'act':
            da = da * act_slope(st['act'], c)
        elif st['type'] == 'dropout':
            if c is not None:
                da = da * c
        elif st['type'] == 'birnn':
            da, g = birnn_backward(da, c)
            out = [g[k][n] for k in ('fwd', 'bwd') for n in ('W', 'U', 'b')] + out
    return out


def loss_and_grads(stages, x, labels, seq_len, masks=None, kinks=None):
    """Mean CTC over the batch and its gradients: dict(ctc (N,), logits, grads)."""
    logits, caches = model_forward(stages, x, masks, kinks)
    N = logits.shape[1]
    ctc_n, dlog = _ctc.ctc_loss_grad(logits, labels, seq_len, dtype=np.float64)
    grads = model_backward(stages, caches, dlog / N)
    return dict(ctc=ctc_n, logits=logits, grads=grads)
