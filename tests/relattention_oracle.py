"""float64 NumPy restatement of relative positional multi-head self-attention (Transformer-XL,
arXiv 1901.02860 section 3.3, as the Conformer uses it, arXiv 2005.08100 section 2.1) with explicit
T x T scores, and of the model chains that hold such a stage: every other stage kind is delegated,
stage by stage, to tests/conformer_oracle.py (and through it tests/attention_oracle.py).  Test
infrastructure only.

The core, per sample n and head h of [Q | K | V] (T, N, 3D), D = heads * dh, with pos (2T - 1, D)
the projected table and b_u, b_v (D) the position biases:
    s[t, u] = scale ((q_t + b_u) . k_u + (q_t + b_v) . pos[t - u + T - 1])  for u < lens[n]
    p = softmax_u(s), p = 0 for u >= lens[n];  out_t = sum_u p[t, u] v_u
THE RELATIVE INDEX IS r = t - u: QUERY FRAME MINUS KEY FRAME (positive when the key lies in the
past); row r + T - 1 of the table holds pos_r.  Every frame t < T is a query; only keys are masked.
"""
import numpy as np

from oracle import conv as _conv
from oracle import ctc as _ctc
from tests import attention_oracle as AO
from tests import conformer_oracle as CO


def relpos(T, D):
    """The (2T - 1, D) table, float64 rounded once to fp32 as the library uploads it: row
    r + T - 1: pe[r, 2i] = sin(r 10000^(-2i / D)), pe[r, 2i + 1] = cos(r 10000^(-2i / D))."""
    pe = np.zeros((2 * T - 1, D))
    r = np.arange(-(T - 1), T, dtype=np.float64)
    for f in range(D):
        ang = r * 10000.0 ** (-2.0 * (f // 2) / D)
        pe[:, f] = np.sin(ang) if f % 2 == 0 else np.cos(ang)
    return pe.astype(np.float32).astype(np.float64)


def _rows(T):
    """idx[t, u] = t - u + T - 1, the table row of the pair (query t, key u)."""
    return np.arange(T)[:, None] - np.arange(T)[None, :] + T - 1


def _heads(a, heads):
    """(T, N, D) -> (N, heads, T, dh)."""
    T, N, D = a.shape
    return np.ascontiguousarray(a.reshape(T, N, heads, D // heads).transpose(1, 2, 0, 3))


# ----------------------------------------------------------------------------- the core
def relattn_forward(qkv, pos, bias_u, bias_v, heads, lens=None, scale=None):
    """qkv (T, N, 3D), pos (2T - 1, D), bias_u / bias_v (D) -> out (T, N, D), cache."""
    T, N, D3 = qkv.shape
    D = D3 // 3
    dh = D // heads
    scale = 1.0 / np.sqrt(dh) if scale is None else scale
    lens = np.full(N, T) if lens is None else np.asarray(lens).reshape(-1)
    q, k, v = [_heads(qkv[:, :, i * D:(i + 1) * D], heads) for i in range(3)]
    bu = np.asarray(bias_u, np.float64).reshape(1, heads, 1, dh)
    bv = np.asarray(bias_v, np.float64).reshape(1, heads, 1, dh)
    ph = np.ascontiguousarray(pos[:, :D].reshape(2 * T - 1, heads, dh).transpose(1, 0, 2))
    idx = _rows(T)
    g = (q + bv) @ ph.transpose(0, 2, 1)[None]                  # (N, heads, T, 2T - 1)
    s = (q + bu) @ k.transpose(0, 1, 3, 2) + g[:, :, np.arange(T)[:, None], idx]
    s *= scale
    mask = (np.arange(T)[None, :] < lens[:N, None])[:, None, None, :]      # valid keys
    smax = np.abs(s).max(initial=0.0, where=mask)
    s = np.where(mask, s, -np.inf)
    m = s.max(axis=-1, keepdims=True)
    p = np.exp(s - m)
    l = p.sum(axis=-1, keepdims=True)
    p /= l
    out = (p @ v).transpose(2, 0, 1, 3).reshape(T, N, D)
    lse = (m + np.log(l))[..., 0].transpose(2, 0, 1)
    return out, dict(q=q, k=k, v=v, p=p, lse=lse, scale=scale, out=out, smax=smax, ph=ph, bu=bu,
                     bv=bv, idx=idx)


def relattn_backward(dout, c):
    """-> dqkv (T, N, 3D), dpos (2T - 1, D), dbias_u (D), dbias_v (D)."""
    q, k, v, p, scale, ph, idx = c['q'], c['k'], c['v'], c['p'], c['scale'], c['ph'], c['idx']
    N, heads, T, dh = q.shape
    do = _heads(dout, heads)
    dv = p.transpose(0, 1, 3, 2) @ do
    dp = do @ v.transpose(0, 1, 3, 2)
    ds = p * (dp - (dp * p).sum(axis=-1, keepdims=True))
    dg = np.zeros((N, heads, T, 2 * T - 1))
    dg[:, :, np.arange(T)[:, None], idx] = ds                   # dG[t, t - u + T - 1] = dS[t, u]
    dq_c = scale * (ds @ k)
    dq_p = scale * (dg @ ph[None])
    dk = scale * (ds.transpose(0, 1, 3, 2) @ (q + c['bu']))
    dposh = scale * (dg.transpose(0, 1, 3, 2) @ (q + c['bv'])).sum(axis=0)   # (heads, 2T - 1, dh)
    dqkv = np.concatenate([a.transpose(2, 0, 1, 3).reshape(T, N, heads * dh)
                           for a in (dq_c + dq_p, dk, dv)], axis=-1)
    dpos = dposh.transpose(1, 0, 2).reshape(2 * T - 1, heads * dh)
    return dqkv, dpos, dq_c.sum(axis=(0, 2)).reshape(-1), dq_p.sum(axis=(0, 2)).reshape(-1)


# ----------------------------------------------------------------------------- the layer
def relmha_forward(x, W_qkv, b_qkv, W_pos, bias_u, bias_v, W_o, b_o, heads, lens=None):
    """x (T, N, F) -> y (T, N, n_out), cache.  bias_u, bias_v: (heads, dh)."""
    qkv = x @ W_qkv + b_qkv
    pe = relpos(x.shape[0], W_pos.shape[0])
    ctx, c = relattn_forward(qkv, pe @ W_pos, bias_u.reshape(-1), bias_v.reshape(-1), heads, lens)
    c.update(x=x, ctx=ctx, W_qkv=W_qkv, W_o=W_o, pe=pe, bshape=bias_u.shape)
    return ctx @ W_o + b_o, c


def relmha_backward(dy, c):
    """-> dx, [dW_qkv, db_qkv, dW_pos, dbias_u, dbias_v, dW_o, db_o]."""
    dW_o = np.einsum('tnd,tno->do', c['ctx'], dy)
    db_o = dy.sum(axis=(0, 1))
    dqkv, dpos, dbu, dbv = relattn_backward(dy @ c['W_o'].T, c)
    dW_qkv = np.einsum('tnf,tnd->fd', c['x'], dqkv)
    db_qkv = dqkv.sum(axis=(0, 1))
    return dqkv @ c['W_qkv'].T, [dW_qkv, db_qkv, c['pe'].T @ dpos, dbu.reshape(c['bshape']),
                                 dbv.reshape(c['bshape']), dW_o, db_o]


# ----------------------------------------------------------------------------- model chains
_REL_KEYS = ('W_qkv', 'b_qkv', 'W_pos', 'bias_u', 'bias_v', 'W_o', 'b_o')
_REL_L2 = ('W_qkv', 'W_pos', 'W_o')


class _Plain(object):
    """A model's stages and weights with the relative stages cut out, for CO.stages_from_model."""

    def __init__(self, stages, weights):
        self.stages, self._w = stages, weights

    def get_weights(self):
        return self._w


def stages_from_model(model):
    """Oracle stage list (float64 weights), index-aligned with model.stages: a relative attention
    stage is a dict(type='relmha', ...), every other one is conformer_oracle's."""
    w = list(model.get_weights())
    out = []
    for s in model.stages:
        n = len(s.tensors or ())
        mine, w = w[:n], w[n:]
        if s.kind == 'mha' and getattr(s, 'relative', False):
            st = dict(type='relmha', heads=s.heads, l2=s.l2)
            st.update(zip(_REL_KEYS, [a.astype(np.float64) for a in mine]))
            out.append(st)
        else:
            out += CO.stages_from_model(_Plain([s], mine))
    return out


def model_forward(stages, x, lens=None, training=True):
    """As conformer_oracle.model_forward (lens: INPUT lengths, strided by the conv stages)."""
    a, caches, outs = x, [], []
    lens = None if lens is None else np.asarray(lens).reshape(-1)
    for st in stages:
        t = st['type']
        if t == 'relmha':
            a, c = relmha_forward(a, *[st[k] for k in _REL_KEYS], heads=st['heads'], lens=lens)
        elif t == 'merge':
            a, c = st['coef'] * (st['scale'] * a + outs[st['skip']]), None
        else:
            a, (c,) = CO.model_forward([st], a, lens, training)
            if t == 'conv' and lens is not None:
                lens = _conv.out_lengths(lens, st['stride'][0])
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
            da = st['scale'] * da
        elif t == 'relmha':
            da, g = relmha_backward(da, c)
            out = g + out
        else:
            g, da = CO.model_backward([st], [c], da)
            out = g + out
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


def _keys(st):
    return _REL_KEYS if st['type'] == 'relmha' else CO._KEYS.get(st['type'], ())


def trainable(stages):
    """The arrays Adam updates, get_weights() order (running moments left out), with their l2."""
    return [(st, k, st['l2'] if k in CO._L2 + _REL_L2 else 0.0) for st in stages
            for k in _keys(st) if k not in ('rm', 'rv')]


def grads_trainable(stages, grads):
    keys = [k for st in stages for k in _keys(st)]
    return [g for g, k in zip(grads, keys) if k not in ('rm', 'rv')]


def weights(stages):
    """get_weights() order, running moments included."""
    return [st[k] for st in stages for k in _keys(st)]


def train_step(stages, x, labels, seq_len, opt):
    """One optimisation step of the oracle, as conformer_oracle.train_step."""
    out = loss_and_grads(stages, x, labels, seq_len, training=True)
    tr = trainable(stages)
    g = [gi + 2.0 * l2 * holder[k] if l2 else gi
         for gi, (holder, k, l2) in zip(grads_trainable(stages, out['grads']), tr)]
    opt.step([holder[k] for holder, k, _ in tr], g)
    for st, c in zip(stages, out['caches']):
        if st['type'] == 'bn':
            st['rm'] = CO.BO.ema(st['rm'], c['mean'], st['momentum'])
            st['rv'] = CO.BO.ema(st['rv'], c['var'], st['momentum'])
    return out


greedy = AO.greedy
