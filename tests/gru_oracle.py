"""float64 NumPy restatement of the Keras-1.2.2 GRU (consume_less='gpu',
inner_activation='hard_sigmoid') inside Bidirectional('concat' / 'sum'), forward and backward, and
of the model chains that use it (Bidirectional(GRU) stacks, deep_speech2(rnn_type='gru') with and
without batch normalisation), composed with oracle.conv, oracle.ctc, tests/simple_rnn_oracle and
tests/batchnorm_oracle.  Test infrastructure only.

Rules recalled from Keras 1.2.2 (it cannot run here, so these are unpinned):
* [recalled: keras/layers/recurrent.py GRU.step, consume_less='gpu'] with m = h_prev B_U[0],
  matrix_x = (x B_W[0]) W + b, matrix_inner = m U[:, :2H]: z = hs(x_z + inner_z),
  r = hs(x_r + inner_r), hh = act(x_h + (r m) U[:, 2H:]), h = z h_prev + (1 - z) hh.  The
  reset gate multiplies the state BEFORE the product; the fused W, U, b hold the blocks z, r, h.
* [recalled: keras/activations.py hard_sigmoid, TensorFlow backend] clip(0.2 x + 0.5, 0, 1).
* [recalled: keras/layers/wrappers.py Bidirectional] the backward copy runs on the reversed
  sequence and its output is reversed back; 'concat' = [h_f | h_b], 'sum' = h_f + h_b.

The backward pass takes every activation slope from the SAVED gate values it is handed (hs' = 0.2
where 0 < gate < 1, else 0; act' from hh alone), never from a recomputed pre-activation.
"""
import numpy as np

from oracle import conv as _conv
from oracle import ctc as _ctc
from tests import batchnorm_oracle as BO
from tests import simple_rnn_oracle as SR

act_apply, act_slope = SR.act_apply, SR.act_slope


def hard_sigmoid(a):
    return np.clip(0.2 * a + 0.5, 0.0, 1.0)


def hs_slope(g):
    """hard_sigmoid'(a) read from the gate g = hs(a): 0.2 strictly inside (0, 1), else 0."""
    return 0.2 * ((g > 0.0) & (g < 1.0))


def _order(T, reverse):
    return list(range(T - 1, -1, -1)) if reverse else list(range(T))


def _prev(h, reverse):
    """h_prev of every frame: h one frame earlier in the processing order, 0 at the first."""
    hp = np.zeros_like(h)
    if reverse:
        hp[:-1] = h[1:]
    else:
        hp[1:] = h[:-1]
    return hp


# ---------------------------------------------------------------- the recurrence alone
def recurrence_forward(zx, U, act, BU=None, reverse=False):
    """zx (T, N, 3H) = x W + b (blocks z, r, h), U (H, 3H) -> h (T, N, H), gates (T, N, 3H) =
    z | r | hh, both in frame order."""
    T, N, H3 = zx.shape
    H = H3 // 3
    h = np.zeros((T, N, H), zx.dtype)
    gates = np.zeros_like(zx)
    prev = np.zeros((N, H), zx.dtype)
    for t in _order(T, reverse):
        m = prev if BU is None else prev * BU
        zr = hard_sigmoid(zx[t, :, :2 * H] + m @ U[:, :2 * H])
        z, r = zr[:, :H], zr[:, H:]
        hh = act_apply(act, zx[t, :, 2 * H:] + (r * m) @ U[:, 2 * H:])
        h[t] = z * prev + (1.0 - z) * hh
        gates[t, :, :2 * H] = zr
        gates[t, :, 2 * H:] = hh
        prev = h[t]
    return h, gates


def _slopes(gates, act, H, sides=None):
    """(hs'(z), hs'(r), act'(hh)) from the saved gates; with `sides` (another computation's gates)
    the saturation SIDE of every entry is read from there: the hard-sigmoid slopes wholly, the
    activation's where it is piecewise linear (the values stay this computation's)."""
    src = gates if sides is None else sides
    sz, sr = hs_slope(src[..., :H]), hs_slope(src[..., H:2 * H])
    piecewise = act == 'relu' or isinstance(act, (tuple, list))
    sh = act_slope(act, (src if piecewise else gates)[..., 2 * H:])
    return sz, sr, sh


def recurrence_backward(dy, U, h, gates, act, BU=None, reverse=False, sides=None):
    """dy (T, N, H) gradient of h -> da (T, N, 3H) = da_z | da_r | da_h."""
    T, N, H = dy.shape
    sz, sr, sh = _slopes(gates, act, H, sides)
    hp = _prev(h, reverse)
    da = np.zeros((T, N, 3 * H), dy.dtype)
    carry = np.zeros((N, H), dy.dtype)
    for t in reversed(_order(T, reverse)):
        z, r, hh = gates[t, :, :H], gates[t, :, H:2 * H], gates[t, :, 2 * H:]
        m = hp[t] if BU is None else hp[t] * BU
        g = dy[t] + carry
        da_h = g * (1.0 - z) * sh[t]
        da_z = g * (hp[t] - hh) * sz[t]
        q = da_h @ U[:, 2 * H:].T
        da_r = q * m * sr[t]
        dm = q * r + np.concatenate([da_z, da_r], axis=1) @ U[:, :2 * H].T
        carry = g * z + (dm if BU is None else dm * BU)
        da[t] = np.concatenate([da_z, da_r, da_h], axis=1)
    return da


def kernel_forward(zx2, U2, act, BU2=None):
    """The C ABI's view: zx (T, N, 2, 3H), U (2, H, 3H), B_U (2, N, H) -> h (T, N, 2, H), gates
    (T, N, 2, 3H)."""
    outs = [recurrence_forward(zx2[:, :, d], U2[d], act, None if BU2 is None else BU2[d],
                               reverse=d == 1) for d in range(2)]
    return np.stack([o[0] for o in outs], axis=2), np.stack([o[1] for o in outs], axis=2)


def kernel_backward(dy, U2, h2, gates2, act, BU2=None, shared=False):
    """dy (T, N, H) shared by both directions ('sum') or (T, N, 2, H) -> da (T, N, 2, 3H)."""
    return np.stack([recurrence_backward(dy if shared else dy[:, :, d], U2[d], h2[:, :, d],
                                         gates2[:, :, d], act, None if BU2 is None else BU2[d],
                                         reverse=d == 1) for d in range(2)], axis=2)


# ---------------------------------------------------------------- layers
def gru_forward(x, W, U, b, act, BW=None, BU=None, reverse=False):
    xm = x if BW is None else x * BW[None]
    h, gates = recurrence_forward(xm @ W + b, U, act, BU, reverse)
    return h, dict(x=x, W=W, U=U, act=act, BW=BW, BU=BU, reverse=reverse, h=h, gates=gates,
                   sides=None)


def gru_backward(dh, c):
    x, W, U, h, gates, BW, BU = c['x'], c['W'], c['U'], c['h'], c['gates'], c['BW'], c['BU']
    H = h.shape[-1]
    da = recurrence_backward(dh, U, h, gates, c['act'], BU, c['reverse'], c['sides'])
    xm = x if BW is None else x * BW[None]
    dW = np.einsum('tnf,tnh->fh', xm, da)
    db = da.sum(axis=(0, 1))
    dx = da @ W.T
    if BW is not None:
        dx = dx * BW[None]
    m = _prev(h, c['reverse'])
    if BU is not None:
        m = m * BU[None]
    dU = np.concatenate([np.einsum('tni,tnj->ij', m, da[..., :2 * H]),
                         np.einsum('tni,tnj->ij', gates[..., H:2 * H] * m, da[..., 2 * H:])],
                        axis=1)
    return dx, dW, dU, db, da


def bigru_forward(x, p, act, merge, BW=None, BU=None):
    """p: {'fwd': {W, U, b}, 'bwd': {...}}; BW (2, N, F), BU (2, N, H)."""
    hs, cs = [], []
    for d, key in enumerate(('fwd', 'bwd')):
        h, c = gru_forward(x, p[key]['W'], p[key]['U'], p[key]['b'], act,
                           None if BW is None else BW[d], None if BU is None else BU[d],
                           reverse=d == 1)
        hs.append(h)
        cs.append(c)
    y = np.concatenate(hs, axis=-1) if merge == 'concat' else hs[0] + hs[1]
    return y, dict(cs=cs, merge=merge, H=hs[0].shape[-1])


def bigru_backward(dy, c):
    H = c['H']
    dx, grads = 0.0, {}
    for d, key in enumerate(('fwd', 'bwd')):
        dh = dy[..., d * H:(d + 1) * H] if c['merge'] == 'concat' else dy
        dxd, dW, dU, db, _ = gru_backward(dh, c['cs'][d])
        dx = dx + dxd
        grads[key] = dict(W=dW, U=dU, b=db)
    return dx, grads


def side_share(own, other, H):
    """Share of the z and r entries whose saturation side differs between two gate slabs."""
    a, b = hs_slope(own[..., :2 * H]), hs_slope(other[..., :2 * H])
    return float(np.mean(a != b))


# ---------------------------------------------------------------- models
def stages_from_model(model):
    """The oracle's stage list (float64 weights) from an engine.Model whose stages are noise (0),
    reshape, conv, bn, act, dropout, dense or bigru."""
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
        elif s.kind == 'bigru':
            p = {d: dict(W=next(it), U=next(it), b=next(it)) for d in ('fwd', 'bwd')}
            out.append(dict(type='bigru', p=p, act=s.act, merge=s.merge, l2_W=s.l2_W,
                            l2_U=s.l2_U))
        else:
            raise NotImplementedError(s.kind)
    return out


def model_forward(stages, x, masks=None, sides=None, training=True):
    """x (T, N, F) real rows -> logits (T, N, C), caches.  The stage list is index-aligned with
    model.stages.  masks: {stage index: (B_W (2, N, F), B_U (2, N, H))} of bigru stages.
    sides: {stage index: gates (T, N, 2, 3H)} -- another computation's saved gates whose
    saturation sides the backward pass of that stage takes (see _slopes)."""
    masks, sides = masks or {}, sides or {}
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
            a = act_apply(st['act'], a)
            c = a
        elif t == 'dense':
            c = a
            a = a @ st['W'] + st['b']
        elif t == 'bigru':
            BW, BU = masks.get(i, (None, None))
            a, c = bigru_forward(a, st['p'], st['act'], st['merge'], BW, BU)
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
            da = da * act_slope(st['act'], c)
        elif t == 'dense':
            out = [np.einsum('tnf,tnc->fc', c, da), da.sum(axis=(0, 1))] + out
            da = da @ st['W'].T
        elif t == 'bigru':
            da, g = bigru_backward(da, c)
            out = [g[k][n] for k in ('fwd', 'bwd') for n in ('W', 'U', 'b')] + out
    return out


def loss_and_grads(stages, x, labels, seq_len, masks=None, sides=None):
    """Mean CTC over the batch (no l2) and its gradients: dict(ctc (N,), logits, grads, caches)."""
    logits, caches = model_forward(stages, x, masks, sides)
    for st in stages:
        if st['type'] == 'conv':
            seq_len = _conv.out_lengths(seq_len, st['stride'][0])
    N = logits.shape[1]
    ctc_n, dlog = _ctc.ctc_loss_grad(logits, labels, seq_len, dtype=np.float64)
    grads = model_backward(stages, caches, dlog / N)
    return dict(ctc=ctc_n, logits=logits, grads=grads, caches=caches)


def trainable(stages):
    """The arrays Adam updates, get_weights() order (running moments left out), with their l2."""
    out = []
    for st in stages:
        t = st['type']
        if t in ('conv', 'dense'):
            out += [(st, 'W', st['l2']), (st, 'b', 0.0)]
        elif t == 'bn':
            out += [(st, 'gamma', 0.0), (st, 'beta', 0.0)]
        elif t == 'bigru':
            for d in ('fwd', 'bwd'):
                out += [(st['p'][d], 'W', st['l2_W']), (st['p'][d], 'U', st['l2_U']),
                        (st['p'][d], 'b', 0.0)]
    return out


def grads_trainable(stages, grads):
    out, it = [], iter(grads)
    for st in stages:
        n = {'conv': 2, 'dense': 2, 'bn': 4, 'bigru': 6}.get(st['type'], 0)
        g = [next(it) for _ in range(n)]
        out += g[:2] if st['type'] == 'bn' else g
    return out


def weights(stages):
    """get_weights() order, running moments included."""
    out = []
    for st in stages:
        t = st['type']
        if t in ('conv', 'dense'):
            out += [st['W'], st['b']]
        elif t == 'bn':
            out += [st['gamma'], st['beta'], st['rm'], st['rv']]
        elif t == 'bigru':
            out += [st['p'][d][k] for d in ('fwd', 'bwd') for k in ('W', 'U', 'b')]
    return out


def train_step(stages, x, labels, seq_len, opt, masks=None, sides=None):
    """One optimisation step of the oracle: gradients + l2, the optimiser (oracle.optim, in place),
    then the running-moment EMA of every BN stage.  Returns the step's loss_and_grads dict."""
    out = loss_and_grads(stages, x, labels, seq_len, masks, sides)
    g = grads_trainable(stages, out['grads'])
    tr = trainable(stages)
    g = [gi + 2.0 * l2 * holder[k] if l2 else gi for gi, (holder, k, l2) in zip(g, tr)]
    opt.step([holder[k] for holder, k, _ in tr], g)
    for st, c in zip(stages, out['caches']):
        if st['type'] == 'bn':
            st['rm'] = BO.ema(st['rm'], c['mean'], st['momentum'])
            st['rv'] = BO.ema(st['rv'], c['var'], st['momentum'])
    return out
