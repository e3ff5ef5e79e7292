"""float64 NumPy restatement of limited-context attention (K25: the window of csrc/attn_tile.h on
both attention cores), of the depthwise convolution with a chosen left padding, and of the model
chains that hold such stages: every other stage kind is delegated, stage by stage, to
tests/relattention_oracle.py (and through it conformer_oracle / attention_oracle).  Test
infrastructure only.

THE WINDOW is three integers: chunk >= 1, left >= -1 frames (-1: unlimited), right >= 0 frames.
For query frame t let c0 = (t // chunk) * chunk.  Key u is visible to t iff
    lo(t) <= u < hi(t) and u < lens[n],   hi(t) = c0 + chunk + right,
                                          lo(t) = 0 if left < 0 else max(0, c0 - left).
A row with no visible key has p = 0 everywhere, out = 0 and lse = 0, and passes no gradient.
"""
import numpy as np

from oracle import conv as _conv
from oracle import ctc as _ctc
from tests import attention_oracle as AO
from tests import conformer_oracle as CO
from tests import relattention_oracle as RO

TILE = 64       # the query and key tile of the kernels (asr_attn_plan's bq, bk)


# ----------------------------------------------------------------------------- the window
def window_lo_hi(T, window):
    """lo (T), hi (T) of every query frame."""
    chunk, left, right = window
    c0 = np.arange(T) // chunk * chunk
    lo = np.zeros(T, np.int64) if left < 0 else np.maximum(0, c0 - left)
    return lo, c0 + chunk + right


def window_mask(T, window):
    """(T, T) bool: [t, u] = key u lies in the window of query t (the length mask aside)."""
    lo, hi = window_lo_hi(T, window)
    u = np.arange(T)[None, :]
    return (u >= lo[:, None]) & (u < hi[:, None])


def visible(T, window, lens, N):
    """(N, T, T) bool: the window and the key mask by length."""
    lens = np.full(N, T) if lens is None else np.asarray(lens).reshape(-1)[:N]
    return window_mask(T, window)[None] & (np.arange(T)[None, None, :] < lens[:, None, None])


def tile_pairs(T, window, tile=TILE):
    """The (query tile, key tile) pairs that hold at least one visible pair, lens = None."""
    m = window_mask(T, window)
    return sum(bool(m[q0:q0 + tile, k0:k0 + tile].any())
               for q0 in range(0, T, tile) for k0 in range(0, T, tile))


def _softmax(s, mask):
    """s, mask (N, heads, T, T) -> p, lse (N, heads, T); empty rows: p = 0, lse = 0."""
    s = np.where(mask, s, -np.inf)
    empty = ~mask.any(axis=-1, keepdims=True)
    m = np.where(empty, 0.0, s.max(axis=-1, keepdims=True))
    p = np.exp(s - m)
    l = p.sum(axis=-1, keepdims=True)
    l1 = np.where(empty, 1.0, l)
    return p / l1, np.where(empty, 0.0, m + np.log(l1))[..., 0]


# ----------------------------------------------------------------------------- K21 under a window
def attn_forward(qkv, heads, window, lens=None, scale=None):
    """attention_oracle.attn_forward under a window; the cache serves AO.attn_backward."""
    T, N, D3 = qkv.shape
    D = D3 // 3
    dh = D // heads
    scale = 1.0 / np.sqrt(dh) if scale is None else scale
    q, k, v = [RO._heads(qkv[:, :, i * D:(i + 1) * D], heads) for i in range(3)]
    s = scale * (q @ k.transpose(0, 1, 3, 2))
    mask = np.broadcast_to(visible(T, window, lens, N)[:, None], s.shape)
    smax = np.abs(s).max(initial=0.0, where=mask)
    p, lse = _softmax(s, mask)
    out = (p @ v).transpose(2, 0, 1, 3).reshape(T, N, D)
    return out, dict(q=q, k=k, v=v, p=p, lse=lse.transpose(2, 0, 1), scale=scale, out=out,
                     smax=smax, mask=mask)


attn_backward = AO.attn_backward


# ----------------------------------------------------------------------------- K24 under a window
def relattn_forward(qkv, pos, bias_u, bias_v, heads, window, lens=None, scale=None):
    """relattention_oracle.relattn_forward under a window; the cache serves RO.relattn_backward."""
    T, N, D3 = qkv.shape
    D = D3 // 3
    dh = D // heads
    scale = 1.0 / np.sqrt(dh) if scale is None else scale
    q, k, v = [RO._heads(qkv[:, :, i * D:(i + 1) * D], heads) for i in range(3)]
    bu = np.asarray(bias_u, np.float64).reshape(1, heads, 1, dh)
    bv = np.asarray(bias_v, np.float64).reshape(1, heads, 1, dh)
    ph = np.ascontiguousarray(pos[:, :D].reshape(2 * T - 1, heads, dh).transpose(1, 0, 2))
    idx = RO._rows(T)
    g = (q + bv) @ ph.transpose(0, 2, 1)[None]
    s = scale * ((q + bu) @ k.transpose(0, 1, 3, 2) + g[:, :, np.arange(T)[:, None], idx])
    mask = np.broadcast_to(visible(T, window, lens, N)[:, None], s.shape)
    smax = np.abs(s).max(initial=0.0, where=mask)
    p, lse = _softmax(s, mask)
    out = (p @ v).transpose(2, 0, 1, 3).reshape(T, N, D)
    return out, dict(q=q, k=k, v=v, p=p, lse=lse.transpose(2, 0, 1), scale=scale, out=out,
                     smax=smax, ph=ph, bu=bu, bv=bv, idx=idx, mask=mask)


relattn_backward = RO.relattn_backward


# ----------------------------------------------------------------------------- dwconv, pad_left
def dwconv_forward(x, w, b, pad_left, lens=None):
    """y[t] = b + sum_j w[j] xm[t + j - pad_left]: x (T, N, C), w (k, C), b (C) -> y, cache."""
    T, N, C = x.shape
    k = w.shape[0]
    assert 0 <= pad_left <= k - 1
    m = CO._mask(T, N, lens)
    xp = np.zeros((T + k - 1, N, C))
    xp[pad_left:pad_left + T] = np.where(m[:, :, None], x, 0.0)
    y = np.zeros((T, N, C)) + b
    for j in range(k):
        y += w[j] * xp[j:j + T]
    return y, dict(xp=xp, w=w, mask=m, pad_left=pad_left)


def dwconv_backward(dy, c):
    """-> dx, dw, db: dx[u] = sum_j w[j] dy[u - j + pad_left] below the length."""
    xp, w, m, pl = c['xp'], c['w'], c['mask'], c['pad_left']
    T, k = dy.shape[0], w.shape[0]
    dyp = np.zeros((T + k - 1,) + dy.shape[1:])
    dyp[k - 1 - pl:k - 1 - pl + T] = dy
    dx = np.zeros_like(dy)
    dw = np.zeros_like(w)
    for j in range(k):
        dw[j] = (dy * xp[j:j + T]).sum(axis=(0, 1))
        dx += w[j] * dyp[k - 1 - j:k - 1 - j + T]
    return np.where(m[:, :, None], dx, 0.0), dw, dy.sum(axis=(0, 1))


dwconv_abs_terms = CO.dwconv_abs_terms      # (reads xp and w of the cache only)


# ----------------------------------------------------------------------------- model chains
def stages_from_model(model):
    """relattention_oracle.stages_from_model, plus 'window' on the attention stages and 'pad_left'
    on the depthwise convolutions (None where the model's stage has none)."""
    out = RO.stages_from_model(model)
    for st, s in zip(out, model.stages):
        if s.kind == 'mha':
            st['window'] = getattr(s, 'window', None)
        elif s.kind == 'dwconv':
            st['pad_left'] = getattr(s, 'pad_left', None)
    return out


def _mha_forward(a, st, lens):
    qkv = a @ st['W_qkv'] + st['b_qkv']
    if st['type'] == 'relmha':
        pe = RO.relpos(a.shape[0], st['W_pos'].shape[0])
        ctx, c = relattn_forward(qkv, pe @ st['W_pos'], st['bias_u'].reshape(-1),
                                 st['bias_v'].reshape(-1), st['heads'], st['window'], lens)
        c.update(pe=pe, bshape=st['bias_u'].shape)
    else:
        ctx, c = attn_forward(qkv, st['heads'], st['window'], lens)
    c.update(x=a, ctx=ctx, W_qkv=st['W_qkv'], W_o=st['W_o'])
    return ctx @ st['W_o'] + st['b_o'], c


def model_forward(stages, x, lens=None, training=True):
    """As relattention_oracle.model_forward (lens: INPUT lengths, strided by the conv stages)."""
    a, caches, outs = x, [], []
    lens = None if lens is None else np.asarray(lens).reshape(-1)
    for st in stages:
        t = st['type']
        if t in ('mha', 'relmha') and st.get('window') is not None:
            a, c = _mha_forward(a, st, lens)
        elif t == 'dwconv' and st.get('pad_left') is not None:
            a, c = dwconv_forward(a, st['W'], st['b'], st['pad_left'], lens)
        elif t == 'merge':
            a, c = st['coef'] * (st['scale'] * a + outs[st['skip']]), None
        else:
            a, (c,) = RO.model_forward([st], a, lens, training)
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
        if i in skip:
            da = da + skip.pop(i)
        if t == 'merge':
            da = st['coef'] * da
            skip[st['skip']] = da
            da = st['scale'] * da
        elif t == 'relmha' and st.get('window') is not None:
            da, g = RO.relmha_backward(da, c)
            out = g + out
        elif t == 'mha' and st.get('window') is not None:
            da, g = AO.mha_backward(da, c)
            out = g + out
        elif t == 'dwconv' and st.get('pad_left') is not None:
            da, dw, db = dwconv_backward(da, c)
            out = [dw, db] + out
        else:
            g, da = RO.model_backward([st], [c], da)
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


trainable, grads_trainable, weights, greedy = RO.trainable, RO.grads_trainable, RO.weights, RO.greedy


def train_step(stages, x, labels, seq_len, opt):
    """One optimisation step of the oracle, as relattention_oracle.train_step."""
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
