"""NumPy restatement of time reduction by frame stacking (K33, csrc/timestack.hip; the
TimeReduction layer) and of the models that contain it.  Test infrastructure only.

The length rule: frame t of utterance n is valid iff t < min(T, len_n), len_n clamped to 0 .. T;
without lengths, and for the rows n >= N of a slab, every frame is valid.  An invalid frame counts
as zeros (a select: what the slab holds there is never read).

  stack / unstack            on the real rows and columns, (T, N, F) <-> (ceil(T / k), N, k F)
  stack_slab / unstack_slab  the kernels' contract on padded slabs, pad columns and rows included
  stages_from_model ...      float64 stage lists of CTC models built from noise(0) / dropout(0),
                             Dense, bare LSTM, Bidirectional(LSTM), residual merge and
                             TimeReduction stages: tests/lstm_uni_oracle.py's model functions with
                             the two stage kinds it does not have.  Its recurrences are
                             oracle/lstm.py's, operation by operation.
"""
import numpy as np

from oracle import ctc as _ctc
from tests import lstm_uni_oracle as LU


def out_frames(T, k):
    return -(-int(T) // int(k))


def out_lengths(lens, k):
    return -(-np.asarray(lens) // int(k))


def _valid(T, N, lens):
    """(T, N) bool: frame t of row n is valid."""
    if lens is None:
        return np.ones((T, N), bool)
    ln = np.clip(np.asarray(lens).reshape(-1)[:N], 0, T)
    return np.arange(T)[:, None] < ln[None, :]


def stack(x, k, lens=None):
    """x (T, N, F) -> (ceil(T / k), N, k F); lens: one length per row, or None."""
    T, N, F = x.shape
    To = out_frames(T, k)
    xm = np.where(_valid(T, N, lens)[:, :, None], x, 0)
    full = np.zeros((To * k, N, F), x.dtype)
    full[:T] = xm
    return np.ascontiguousarray(full.reshape(To, k, N, F).transpose(0, 2, 1, 3)).reshape(To, N, k * F)


def unstack(dy, k, T, lens=None):
    """The transpose of stack: dy (ceil(T / k), N, k F) -> (T, N, F), zeros in invalid frames."""
    To, N, kF = dy.shape
    assert To == out_frames(T, k) and kF % k == 0
    F = kF // k
    full = dy.reshape(To, N, k, F).transpose(0, 2, 1, 3).reshape(To * k, N, F)[:T]
    return np.where(_valid(T, N, lens)[:, :, None], full, 0)


def _row_lens(lens, N, n_pad, T):
    """Lengths of all n_pad rows of a slab: lens for n < N, T for the rows behind."""
    out = np.full(n_pad, T, np.int64)
    if lens is not None:
        out[:N] = np.asarray(lens).reshape(-1)[:N]
    return out


def stack_slab(x, lens, N, F, ld_out, k):
    """asr_time_stack_fwd: x (T, n_pad, ld_in) -> y (ceil(T / k), n_pad, ld_out).  Columns >= F of
    x are not read; columns >= k F of y are zeros."""
    T, n_pad, _ = x.shape
    y = np.zeros((out_frames(T, k), n_pad, ld_out), x.dtype)
    y[:, :, :k * F] = stack(x[:, :, :F], k, _row_lens(lens, N, n_pad, T))
    return y


def unstack_slab(dy, lens, N, T, F, ld_in, k):
    """asr_time_stack_bwd: dy (ceil(T / k), n_pad, ld_out) -> dx (T, n_pad, ld_in).  Columns
    >= k F of dy are not read; columns >= F of dx are zeros."""
    n_pad = dy.shape[1]
    dx = np.zeros((T, n_pad, ld_in), dy.dtype)
    dx[:, :, :F] = unstack(dy[:, :, :k * F], k, T, _row_lens(lens, N, n_pad, T))
    return dx


# ---------------------------------------------------------------- models
def stages_from_model(model):
    """LU.stages_from_model plus 'treduce' (k) and 'merge' (skip, coef, scale) stages."""
    it = iter([w.astype(np.float64) for w in model.get_weights()])
    out = []
    for s in model.stages:
        if s.kind == 'reshape' and getattr(s, 'time_factor', 0):
            out.append(dict(type='treduce', k=int(s.time_factor)))
        elif s.kind in ('noise', 'dropout'):
            assert not s.value, 'the oracle chain has no noise'
            out.append(dict(type='pass'))
        elif s.kind == 'merge':
            out.append(dict(type='merge', skip=s.skip, coef=s.coef, scale=s.scale))
        elif s.kind == 'dense':
            out.append(dict(type='dense', W=next(it), b=next(it), l2=s.l2))
        elif s.kind == 'bilstm' and getattr(s, 'directions', 2) == 1:
            out.append(dict(type='lstm', W=next(it), U=next(it), b=next(it), act=s.act,
                            l2_W=s.l2_W, l2_U=s.l2_U))
        elif s.kind == 'bilstm':
            assert s.mi is None and s.ln is None and not (s.zoneout_c or s.zoneout_h)
            dirs = [dict(W=next(it), U=next(it), b=next(it)) for _ in range(2)]
            out.append(dict(type='bilstm', dirs=dirs, act=s.act, l2_W=s.l2_W, l2_U=s.l2_U))
        else:
            raise NotImplementedError(s.kind)
    return out


def model_forward(stages, x, lens, sides=None):
    """x (T, N, F) real rows, lens the INPUT lengths -> logits, caches, the logits' lengths.  Only
    a 'treduce' stage reads lengths: those of its own axis, ceil'ed through the stages before."""
    sides = sides or {}
    a, caches, outs = x, [], []
    lens = np.asarray(lens).reshape(-1)
    for i, st in enumerate(stages):
        t, c = st['type'], None
        if t in ('dense', 'lstm', 'bilstm'):
            a, (c,) = LU.model_forward([st], a, sides={0: sides[i]} if i in sides else None)
        elif t == 'merge':
            a = st['coef'] * (st['scale'] * a + outs[st['skip']])
        elif t == 'treduce':
            c = (a.shape[0], lens)
            a = stack(a, st['k'], lens)
            lens = out_lengths(lens, st['k'])
        caches.append(c)
        outs.append(a)
    return a, caches, lens


def model_backward(stages, caches, dlogits):
    """-> gradients in get_weights() order."""
    da, out, skip = dlogits, [], {}
    for i in range(len(stages) - 1, -1, -1):
        st, c = stages[i], caches[i]
        if i in skip:
            da = da + skip.pop(i)
        t = st['type']
        if t == 'dense':
            out = [np.einsum('tnf,tnc->fc', c, da), da.sum(axis=(0, 1))] + out
            da = da @ st['W'].T
        elif t == 'lstm':
            da, dW, dU, db = LU.lstm_backward(da, c)
            out = [dW, dU, db] + out
        elif t == 'bilstm':
            H = st['dirs'][0]['U'].shape[0]
            dx, g = 0.0, []
            for d in range(2):
                dy = np.ascontiguousarray(da[..., d * H:(d + 1) * H])
                dxd, dW, dU, db = LU.lstm_backward(dy if d == 0 else dy[::-1], c[d])
                dx = dx + (dxd if d == 0 else dxd[::-1])
                g += [dW, dU, db]
            da, out = dx, g + out
        elif t == 'merge':
            da = st['coef'] * da
            skip[st['skip']] = da
            da = st['scale'] * da
        elif t == 'treduce':
            da = unstack(da, st['k'], c[0], c[1])
    return out


def loss_and_grads(stages, x, labels, lens, sides=None):
    """Mean CTC over the batch (no l2) and its gradients: dict(ctc (N,), logits, grads, seq_len)."""
    logits, caches, sl = model_forward(stages, x, lens, sides)
    N = logits.shape[1]
    ctc_n, dlog = _ctc.ctc_loss_grad(logits, labels, sl, dtype=np.float64)
    return dict(ctc=ctc_n, logits=logits, grads=model_backward(stages, caches, dlog / N),
                seq_len=sl)


# ---------------------------------------------------------------- the deep_speech2 / GRU family
def ds2_stages_from_model(model):
    """tests/seqbn_oracle.py's stage list (conv, bn, act, dense, bigru, bigru_bn), with the
    TimeReduction stages -- a 'pass' there, like every reshape -- as dict(type='treduce', k)."""
    from tests import seqbn_oracle as SO
    stages = SO.stages_from_model(model)
    for i, s in enumerate(model.stages):
        if s.kind == 'reshape' and getattr(s, 'time_factor', 0):
            stages[i] = dict(type='treduce', k=int(s.time_factor))
    return stages


def ds2_forward(stages, x, lens, sides=None, training=True):
    """seqbn_oracle.model_forward with the lengths carried along the axes: a strided convolution
    and a 'treduce' stage map them to ceil(len / stride); a batch-normalised GRU takes its
    statistics over the valid frames of ITS axis; 'treduce' masks with those of its input's."""
    from tests import seqbn_oracle as SO
    sides = sides or {}
    a, caches = x, []
    lens = np.asarray(lens).reshape(-1)
    for i, st in enumerate(stages):
        t, c = st['type'], None
        if t == 'treduce':
            c = (a.shape[0], lens)
            a = stack(a, st['k'], lens)
            lens = out_lengths(lens, st['k'])
        elif t == 'bigru_bn':
            a, c = SO.bigru_bn_forward(a, st, lens, None, None, training)
        elif t != 'pass':
            a, (c,) = SO.model_forward([st], a, training=training)
        if t in ('bigru', 'bigru_bn') and i in sides:
            for d in range(2):
                c['cs'][d]['sides'] = sides[i][:, :, d]
        if t == 'conv':
            lens = SO._conv.out_lengths(lens, st['stride'][0])
        caches.append(c)
    return a, caches, lens


def ds2_backward(stages, caches, dlogits):
    """seqbn_oracle.model_backward, stage by stage, with the 'treduce' transpose."""
    from tests import seqbn_oracle as SO
    da, out = dlogits, []
    for st, c in zip(reversed(stages), reversed(caches)):
        t = st['type']
        if t == 'treduce':
            da = unstack(da, st['k'], c[0], c[1])
        elif t == 'conv':
            da, dW, db = SO._conv.conv2d_backward(da, c)
            out = [dW, db] + out
        elif t == 'bn':
            da, dg, dbeta = SO.BO.bn_backward(da, c)
            out = [dg, dbeta, np.zeros_like(dg), np.zeros_like(dg)] + out
        elif t == 'act':
            da = da * SO.GO.act_slope(st['act'], c)
        elif t == 'dense':
            out = [np.einsum('tnf,tnc->fc', c, da), da.sum(axis=(0, 1))] + out
            da = da @ st['W'].T
        elif t == 'bigru':
            da, g = SO.GO.bigru_backward(da, c)
            out = [g[k][n] for k in ('fwd', 'bwd') for n in ('W', 'U', 'b')] + out
        elif t == 'bigru_bn':
            da, g = SO.bigru_bn_backward(da, c)
            out = g + out
    return out


def ds2_loss_and_grads(stages, x, labels, lens, sides=None):
    logits, caches, sl = ds2_forward(stages, x, lens, sides)
    N = logits.shape[1]
    ctc_n, dlog = _ctc.ctc_loss_grad(logits, labels, sl, dtype=np.float64)
    return dict(ctc=ctc_n, logits=logits, grads=ds2_backward(stages, caches, dlog / N),
                caches=caches, seq_len=sl)


def train_step(stages, x, labels, lens, opt, sides=None):
    """One optimisation step (gradients + l2, then oracle.optim's optimiser, in place)."""
    out = loss_and_grads(stages, x, labels, lens, sides)
    tr = LU.trainable(stages)
    g = [gi + 2.0 * l2 * holder[k] if l2 else gi for gi, (holder, k, l2) in zip(out['grads'], tr)]
    opt.step([holder[k] for holder, k, _ in tr], g)
    return out
