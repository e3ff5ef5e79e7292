"""float64 NumPy restatement of the UNIDIRECTIONAL GRU (a bare ``layers.GRU``: K28, the
one-direction form of csrc/gru.hip) on top of tests/gru_oracle.py: the recurrence with an initial
state, the stage list of a model whose recurrent stages have one direction, and the chunked
restatement of a streaming session.  Test infrastructure only.

The cell, the saved slopes and the ``sides`` mechanism are gru_oracle's, called with
``reverse=False``; nothing of them is restated here.  What is added:
* ``recurrence_forward(..., h0)``: gru_oracle's loop started from h0 instead of zeros (with h0 =
  None it IS gru_oracle's function, called);
* stages of type 'gru' ({W, U, b}: one direction) in the model chains, beside the stage types of
  gru_oracle and the causal depthwise convolution of tests/window_oracle.py;
* ``model_stream``: a model run a few frames at a time with the state (h per GRU stage, the
  last k - 1 input frames per causal convolution) carried explicitly.
"""
import numpy as np

from oracle import conv as _conv
from oracle import ctc as _ctc
from tests import gru_oracle as GO
from tests import window_oracle as WO

act_apply, act_slope = GO.act_apply, GO.act_slope


# ---------------------------------------------------------------- the recurrence alone
def recurrence_forward(zx, U, act, BU=None, h0=None):
    """zx (T, N, 3H), U (H, 3H), h0 (N, H) or None (zeros) -> h (T, N, H), gates (T, N, 3H)."""
    if h0 is None:
        return GO.recurrence_forward(zx, U, act, BU, reverse=False)
    T, N, H3 = zx.shape
    H = H3 // 3
    h = np.zeros((T, N, H), zx.dtype)
    gates = np.zeros_like(zx)
    prev = np.asarray(h0, zx.dtype)
    for t in range(T):
        m = prev if BU is None else prev * BU
        zr = GO.hard_sigmoid(zx[t, :, :2 * H] + m @ U[:, :2 * H])
        z, r = zr[:, :H], zr[:, H:]
        hh = act_apply(act, zx[t, :, 2 * H:] + (r * m) @ U[:, 2 * H:])
        h[t] = z * prev + (1.0 - z) * hh
        gates[t, :, :2 * H] = zr
        gates[t, :, 2 * H:] = hh
        prev = h[t]
    return h, gates


def recurrence_backward(dy, U, h, gates, act, BU=None, sides=None):
    """BPTT from the zero state: gru_oracle's, forward direction."""
    return GO.recurrence_backward(dy, U, h, gates, act, BU, reverse=False, sides=sides)


def rm_of(h, gates, BU=None, h0=None):
    """r (.) h_prev (.) B_U of every frame (what the kernel keeps for dU_h)."""
    H = h.shape[-1]
    hp = GO._prev(h, False)
    if h0 is not None:
        hp[0] = h0
    return gates[..., H:2 * H] * (hp if BU is None else hp * BU[None])


# ---------------------------------------------------------------- models
def stages_from_model(model):
    """gru_oracle.stages_from_model for a model whose 'bigru' stages may have one direction (type
    'gru') and which may hold causal dwconv stages (inference chains)."""
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
        elif s.kind == 'act':
            out.append(dict(type='act', act=s.act))
        elif s.kind == 'dense':
            out.append(dict(type='dense', W=next(it), b=next(it), l2=s.l2))
        elif s.kind == 'dwconv':
            out.append(dict(type='dwconv', W=next(it), b=next(it), pad_left=s.pad_left))
        elif s.kind == 'bigru' and getattr(s, 'directions', 2) == 1:
            out.append(dict(type='gru', W=next(it), U=next(it), b=next(it), act=s.act,
                            l2_W=s.l2_W, l2_U=s.l2_U))
        else:
            raise NotImplementedError(s.kind)
    return out


def model_forward(stages, x, masks=None, sides=None, lens=None):
    """x (T, N, F) real rows -> logits (T, N, C), caches.  masks: {stage index: (B_W (N, F), B_U
    (N, H))} of gru stages; sides: {stage index: gates (T, N, 3H)} (gru_oracle._slopes); lens:
    the lengths a dwconv stage masks its input by."""
    masks, sides = masks or {}, sides or {}
    a, caches = x, []
    for i, st in enumerate(stages):
        t, c = st['type'], None
        if t == 'conv':
            a, c = _conv.conv2d_forward(a, st['W'], st['b'], st['stride'], st['clip'])
        elif t == 'act':
            a = act_apply(st['act'], a)
            c = a
        elif t == 'dense':
            c = a
            a = a @ st['W'] + st['b']
        elif t == 'dwconv':
            a, c = WO.dwconv_forward(a, st['W'], st['b'], st['pad_left'], lens)
        elif t == 'gru':
            BW, BU = masks.get(i, (None, None))
            a, c = GO.gru_forward(a, st['W'], st['U'], st['b'], st['act'], BW, BU, reverse=False)
            c['sides'] = sides.get(i)
        caches.append(c)
    return a, caches


def model_backward(stages, caches, dlogits):
    """-> gradients in get_weights() order (training chains: conv, act, dense, gru)."""
    da, out = dlogits, []
    for st, c in zip(reversed(stages), reversed(caches)):
        t = st['type']
        if t == 'conv':
            da, dW, db = _conv.conv2d_backward(da, c)
            out = [dW, db] + out
        elif t == 'act':
            da = da * act_slope(st['act'], c)
        elif t == 'dense':
            out = [np.einsum('tnf,tnc->fc', c, da), da.sum(axis=(0, 1))] + out
            da = da @ st['W'].T
        elif t == 'gru':
            da, dW, dU, db, _ = GO.gru_backward(da, c)
            out = [dW, dU, db] + out
        elif t == 'dwconv':
            raise NotImplementedError('dwconv in a training chain')
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
    """(holder, key, l2) of every array Adam updates, get_weights() order."""
    out = []
    for st in stages:
        if st['type'] in ('conv', 'dense'):
            out += [(st, 'W', st['l2']), (st, 'b', 0.0)]
        elif st['type'] == 'gru':
            out += [(st, 'W', st['l2_W']), (st, 'U', st['l2_U']), (st, 'b', 0.0)]
    return out


def weights(stages):
    return [holder[k] for holder, k, _ in trainable(stages)]


def train_step(stages, x, labels, seq_len, opt, masks=None, sides=None):
    """One optimisation step of the oracle: gradients + l2, then the optimiser (oracle.optim, in
    place).  Returns the step's loss_and_grads dict."""
    out = loss_and_grads(stages, x, labels, seq_len, masks, sides)
    tr = trainable(stages)
    g = [gi + 2.0 * l2 * holder[k] if l2 else gi
         for gi, (holder, k, l2) in zip(out['grads'], tr)]
    opt.step([holder[k] for holder, k, _ in tr], g)
    return out


# ---------------------------------------------------------------- a session, restated
def model_stream(stages, x, lens, pieces):
    """x (T, N, F) (no conv stage) run ``pieces`` frames at a time with explicit state: h (N, H)
    per gru stage, the last k - 1 masked input frames per causal dwconv -> logits (T, N, C)."""
    assert sum(pieces) == x.shape[0]
    state, outs, t0 = {}, [], 0
    for p in pieces:
        a = x[t0:t0 + p]
        for i, st in enumerate(stages):
            t = st['type']
            if t == 'gru':
                zx = a @ st['W'] + st['b']
                a, _ = recurrence_forward(zx, st['U'], st['act'], None, state.get(i))
                state[i] = a[-1]
            elif t == 'dwconv':
                k = st['W'].shape[0]
                assert st['pad_left'] == k - 1
                tail = state.get(i)
                if tail is None:
                    tail = np.zeros((k - 1,) + a.shape[1:])
                m = (t0 + np.arange(p))[:, None] < np.asarray(lens)[None, :]
                xm = np.concatenate([tail, np.where(m[:, :, None], a, 0.0)], 0)
                a = np.zeros(a.shape) + st['b']
                for j in range(k):
                    a = a + st['W'][j] * xm[j:j + p]
                state[i] = xm[xm.shape[0] - (k - 1):]
            elif t == 'conv':
                raise NotImplementedError('the front-end has no chunked restatement')
            else:
                a, _ = model_forward([st], a)
        outs.append(a)
        t0 += p
    return np.concatenate(outs, 0)
