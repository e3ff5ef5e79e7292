"""The parameter table: every weight tensor of a model described ONCE, as plain data.

``Model._layout`` calls one builder per trainable stage kind (below).  A builder allocates the
stage's blocks in the flat buffers (setting ``s.oW``, ``s.oU``, ``s.ob``, ... for the compute
code) and returns the stage's ``Tensor`` list in Keras ``get_weights()`` order.  Everything that
speaks about weights is a loop over those lists: ``Model.set_weights`` / ``_unpack``, the l2
``segments``, the initial values (``draw``) and the Keras names of callbacks.keras_layers.

A block is a padded array at ``off`` in its buffer ('params': the flat parameters, and the
gradients and optimiser slots laid out like them; 'running': Model.bn_running).  One tensor
occupies the sub-view ``block[index]``, into which its real array goes through ``embed``:
  None                  as it is
  ('um', H, Hp)         (..., 4H) LSTM gate blocks i|f|c|o -> (..., 4Hp) unit-major/gate-minor
  ('blocks', H, Hp, C)  (..., C H) column blocks -> (..., C Hp), each block padded to Hp
Pad entries of a block hold ``fill``: 0, except 1 in the running variances.
"""
import math
from collections import Counter, namedtuple

import numpy as np

from .. import ops


def _pad4(n):
    return (int(n) + 3) // 4 * 4


def _gm2um(a, H, Hp):
    """(..., 4H) gate-major -> (..., 4Hp) unit-major/gate-minor, zero padded."""
    sh = a.shape[:-1]
    g = a.reshape(sh + (4, H))
    out = np.zeros(sh + (Hp, 4), a.dtype)
    out[..., :H, :] = np.swapaxes(g, -1, -2)
    return out.reshape(sh + (4 * Hp,))


def _um2gm(a, H, Hp):
    sh = a.shape[:-1]
    u = a.reshape(sh + (Hp, 4))[..., :H, :]
    return np.swapaxes(u, -1, -2).reshape(sh + (4 * H,))


def _blocks_pad(a, H, Hp, C, fill=0.0):
    """(..., C H) column blocks (GRU z|r|h, RHN h|t[|c], SimpleRNN's one) -> (..., C Hp)."""
    sh = a.shape[:-1]
    out = np.full(sh + (C, Hp), fill, a.dtype)
    out[..., :H] = a.reshape(sh + (C, H))
    return out.reshape(sh + (C * Hp,))


def _blocks_unpad(a, H, Hp, C):
    sh = a.shape[:-1]
    return a.reshape(sh + (C, Hp))[..., :H].reshape(sh + (C * H,))


MI_PARTS = ('mi_alpha', 'mi_beta1', 'mi_beta2')
# the reference iterates a dict literal {'Uh', 'Wx', 'new_c'} (core/layers.py:409): its
# Python-2 order is unspecified, so files are written in this order and READ BY NAME
LN_PARTS = ('ln_gain_Uh', 'ln_bias_Uh', 'ln_gain_Wx', 'ln_bias_Wx', 'ln_gain_new_c',
            'ln_bias_new_c')
ZEROS, ONES = ('blocks', (0.0,)), ('blocks', (1.0,))

# layer: '[forward_|backward_]<Keras layer class>'; name: the Keras weight-name part; shape: the
# real (Keras) shape; init: ('uniform', limit) | ('normal', std) | ('orthogonal', gain) |
# ('blocks', one constant per equal block of a vector); l2: the coefficient of the block
Tensor = namedtuple('Tensor', 'layer name shape off block index embed l2 init buf fill',
                    defaults=(None, 0.0, ZEROS, 'params', 0.0))


class Alloc(object):
    """The running ends of the buffers the builders allocate blocks from (4-float granules)."""

    def __init__(self):
        self.params = 0         # the flat parameters (and gradients)
        self.running = 0        # BatchNormalization running moments (Model.bn_running)
        self.moments = 4        # their moments blocks, behind the 4 flag slots of Model._gbuf

    def take(self, n, buf='params'):
        o = getattr(self, buf)
        setattr(self, buf, o + _pad4(n))
        return o


def size(t):
    return int(np.prod(t.block, dtype=np.int64))


def _block(t, buf):
    return buf[t.off:t.off + size(t)].reshape(t.block)


def clear(t, buf):
    """Fills the tensor's whole block with its pad value (before its tensors are written)."""
    _block(t, buf)[...] = t.fill


def write(t, buf, a, name):
    """Embeds the real array ``a`` (Keras weight ``name``) into the tensor's place in buf."""
    a = np.asarray(a, np.float32)
    if a.shape != t.shape:
        raise ValueError('%s: shape %s expected, got %s' % (name, t.shape, a.shape))
    if t.embed is not None:
        a = (_gm2um(a, *t.embed[1:]) if t.embed[0] == 'um' else
             _blocks_pad(a, *t.embed[1:], fill=t.fill))
    _block(t, buf)[t.index] = a


def read(t, buf):
    a = _block(t, buf)[t.index]
    if t.embed is not None:
        a = (_um2gm if t.embed[0] == 'um' else _blocks_unpad)(a, *t.embed[1:])
    return np.array(a, np.float32)      # (always a copy, never a view of the buffer)


def draw(t, rs):
    """The tensor's initial value (Keras 1.2.2 initialisers), drawn from ``rs``."""
    kind, v = t.init
    if kind == 'uniform':
        a = rs.uniform(-v, v, size=t.shape)
    elif kind == 'normal':
        a = rs.normal(0.0, v, size=t.shape)
    elif kind == 'orthogonal':
        a = rs.normal(0.0, 1.0, t.shape)
        u, _, w = np.linalg.svd(a, full_matrices=False)
        a = v * (u if u.shape == a.shape else w)
    else:
        a = np.repeat(np.asarray(v, np.float64), t.shape[0] // len(v))
    return a.astype(np.float32)


def segments(stages):
    """Sorted (offset, length, l2) of every block of the flat parameters."""
    return sorted(set((t.off, _pad4(size(t)), t.l2) for s in stages for t in s.tensors
                      if t.buf == 'params'))


def keras_names(stages):
    """[(layer name, [weight name, ...])] in Keras-1.2.2 naming, one entry per weight-bearing
    stage: 'bidirectional_k' holds 'forward_gru_k_W:0', ... and an unwrapped GRU's 'gru_k' holds
    'gru_k_W:0', ..., k counting the unwrapped GRU layers (an unwrapped LSTM's 'lstm_k' likewise,
    counting the unwrapped LSTM layers).  Weights are numbered like their
    layer, except a Dense's: its group is named after the TimeDistributed around it, and Keras
    counts the TimeDistributed(Dropout / Activation) layers with those."""
    groups = {'convolution2d': 'convolution2d', 'batchnormalization': 'batchnormalization',
              'layernormalization': 'layernormalization',
              'multiheadattention': 'multiheadattention',
              'relativemultiheadattention': 'relativemultiheadattention',
              'depthwiseconvolution1d': 'depthwiseconvolution1d', 'dense': 'timedistributed'}
    out, n = [], Counter()
    for s in stages:
        if not s.tensors:
            n['timedistributed'] += bool(getattr(s, 'wrapped', False))
            continue
        cls = s.tensors[0].layer.split('_')[-1]
        # ('forward_gru' ends in 'gru' too: an unwrapped GRU / LSTM is told by its whole layer name)
        group = cls if s.tensors[0].layer in ('gru', 'lstm') else groups.get(cls, 'bidirectional')
        n[group] += 1
        n['dense'] += cls == 'dense'
        out.append(('%s_%d' % (group, n[group]),
                    ['%s_%d_%s:0' % (t.layer, n[cls if cls == 'dense' else group], t.name)
                     for t in s.tensors]))
    return out


def _glorot(fan_in, fan_out):
    return ('uniform', math.sqrt(6.0 / (fan_in + fan_out)))


# ---- one builder per trainable stage kind: (stage, Alloc, real input rows) -> [Tensor]
def conv(s, alloc, rows):
    """Convolution2D, Keras 'tf' kernel layout: W (kt, kf, C_in, C_out), b (C_out)."""
    shape = (s.kt, s.kf, s.C_in, s.C_out)
    s.oW, s.ob = alloc.take(np.prod(shape)), alloc.take(s.C_out)
    return [Tensor('convolution2d', 'W', shape, s.oW, shape, (), l2=s.l2,
                   init=_glorot(s.kt * s.kf * s.C_in, s.kt * s.kf * s.C_out)),
            Tensor('convolution2d', 'b', (s.C_out,), s.ob, (s.C_out,), ())]


def dense(s, alloc, rows):
    F = len(rows)
    s.oW, s.ob = alloc.take(s.f_in_pad * s.n_out), alloc.take(s.n_out)
    return [Tensor('dense', 'W', (F, s.n_out), s.oW, (s.f_in_pad, s.n_out), (rows,), l2=s.l2,
                   init=_glorot(F, s.n_out)),
            Tensor('dense', 'b', (s.n_out,), s.ob, (s.n_out,), ())]


def bilstm(s, alloc, rows):
    """W (in, 2, 4Hp), U (2, Hp, 4Hp) and one block of per-unit vectors, 4Hp each, per
    direction: b alone (s.ob) | alpha, beta1, beta2, b (s.omi) | those four (the first three zero
    without mi), the gain / bias of LN(h@U) and LN(x@W), then of LN(c) (H each): 34H (s.ocell,
    csrc/lstm_ln.hip).  Keras order: W, U, b, the mi vectors, the LN pairs."""
    H, Hp, F = s.H, s.Hp, len(rows)
    G, um = 4 * Hp, ('um', H, Hp)
    s.oW, s.oU = alloc.take(s.f_in_pad * 2 * G), alloc.take(2 * Hp * G)
    if s.ln is not None:
        if Hp != H:
            raise NotImplementedError('layer_norm needs num_hiddens % 4 == 0')
        s.ob, vblock = None, (2, 34 * H)
        s.ocell = voff = alloc.take(2 * 34 * H)
    elif s.mi is not None:
        s.ob, vblock = None, (2, 4 * G)
        s.omi = voff = alloc.take(2 * 4 * G)
    else:
        vblock = (2, G)
        s.ob = voff = alloc.take(2 * G)
    b_lo = 0 if s.ob is not None else 3 * G
    out = []
    for d, layer in enumerate(('forward_lstm', 'backward_lstm')):
        out += [Tensor(layer, 'W', (F, 4 * H), s.oW, (s.f_in_pad, 2, G), (rows, d), um, s.l2_W,
                       _glorot(F, 4 * H)),
                Tensor(layer, 'U', (H, 4 * H), s.oU, (2, Hp, G), (d, slice(0, H)), um, s.l2_U,
                       ('orthogonal', 1.1)),
                Tensor(layer, 'b', (4 * H,), voff, vblock, (d, slice(b_lo, b_lo + G)), um,
                       init=('blocks', (0.0, 1.0, 0.0, 0.0)))]
        if s.mi is not None:            # k_init: constant vectors (core/initializers.py)
            out += [Tensor(layer, name, (4 * H,), voff, vblock, (d, slice(k * G, (k + 1) * G)),
                           um, init=('blocks', (float(s.mi[k]),)))
                    for k, name in enumerate(MI_PARTS)]
        if s.ln is not None:
            for k, name in enumerate(LN_PARTS):
                n, lo = (4 * H, (16 + 4 * k) * H) if k < 4 else (H, (28 + k) * H)
                out.append(Tensor(layer, name, (n,), voff, vblock, (d, slice(lo, lo + n)),
                                  um if k < 4 else None, init=('blocks', (float(s.ln[k % 2]),))))
    return out


def lstm_uni(s, alloc, rows):
    """A bare, unidirectional LSTM (csrc/lstm_uni.hip, K29): W (in, 4Hp), U (Hp, 4Hp), b (4Hp) in
    the unit-major / gate-minor layout; the initialisers and l2 of one direction of ``bilstm``
    (the forget block of b is 1)."""
    H, Hp, F = s.H, s.Hp, len(rows)
    G, um = 4 * Hp, ('um', H, Hp)
    s.oW, s.oU, s.ob = alloc.take(s.f_in_pad * G), alloc.take(Hp * G), alloc.take(G)
    return [Tensor('lstm', 'W', (F, 4 * H), s.oW, (s.f_in_pad, G), (rows,), um, s.l2_W,
                   _glorot(F, 4 * H)),
            Tensor('lstm', 'U', (H, 4 * H), s.oU, (Hp, G), (slice(0, H),), um, s.l2_U,
                   ('orthogonal', 1.1)),
            Tensor('lstm', 'b', (4 * H,), s.ob, (G,), (), um,
                   init=('blocks', (0.0, 1.0, 0.0, 0.0)))]


def birnn(s, alloc, rows):
    """Bidirectional(SimpleRNN) (csrc/rnn.hip): W (in, 2, Hp), U (2, Hp, Hp), b (2, Hp)."""
    H, Hp, F = s.H, s.Hp, len(rows)
    pad = ('blocks', H, Hp, 1)
    s.oW, s.oU, s.ob = alloc.take(s.f_in_pad * 2 * Hp), alloc.take(2 * Hp * Hp), alloc.take(2 * Hp)
    # he_normal: normal(0, sqrt(2 / fan_in)), not truncated
    w_init = ('normal', math.sqrt(2.0 / F)) if s.init == 'he_normal' else _glorot(F, H)
    out = []
    for d, layer in enumerate(('forward_simplernn', 'backward_simplernn')):
        out += [Tensor(layer, 'W', (F, H), s.oW, (s.f_in_pad, 2, Hp), (rows, d), pad, s.l2_W,
                       w_init),
                Tensor(layer, 'U', (H, H), s.oU, (2, Hp, Hp), (d, slice(0, H)), pad, s.l2_U,
                       ('orthogonal', 1.1)),
                Tensor(layer, 'b', (H,), s.ob, (2, Hp), (d,), pad)]
    return out


def bigru(s, alloc, rows, layers=('forward_gru', 'backward_gru')):
    """Bidirectional(GRU) (csrc/gru.hip): W (in, 2, 3Hp), U (2, Hp, 3Hp), b (2, 3Hp), column
    blocks z, r, h.  layers = ('gru',): a bare, unidirectional GRU (K28), the same blocks without
    the direction axis.  batch_norm (K18): no b -- gamma, beta (2, 3Hp) each instead (beta is
    what the kernels read as the bias), the running moments (mean | variance) x (2, 3Hp) and the
    moments block kept where the bn stage keeps its own."""
    H, Hp, F, nd = s.H, s.Hp, len(rows), len(layers)
    G, pad = 3 * Hp, ('blocks', H, Hp, 3)
    ax = (2,) if nd == 2 else ()            # the direction axis of a block ...
    s.oW, s.oU = alloc.take(s.f_in_pad * nd * G), alloc.take(nd * Hp * G)
    if s.bn:
        s.ob, s.og, s.obeta = None, alloc.take(2 * G), alloc.take(2 * G)
        s.orun, ovar = alloc.take(2 * G, 'running'), alloc.take(2 * G, 'running')
        s.omom = alloc.take(ops.bn_moments_len(2 * G), 'moments')
    else:
        s.ob = alloc.take(nd * G)
    out = []
    for d, layer in enumerate(layers):
        at = (d,) if nd == 2 else ()        # ... and a direction's place on it
        out += [Tensor(layer, 'W', (F, 3 * H), s.oW, (s.f_in_pad,) + ax + (G,), (rows,) + at, pad,
                       s.l2_W, _glorot(F, 3 * H)),
                Tensor(layer, 'U', (H, 3 * H), s.oU, ax + (Hp, G), at + (slice(0, H),), pad,
                       s.l2_U, ('orthogonal', 1.1))]
        if s.bn:        # (running_std holds the variance, as in keras.layers.BatchNormalization)
            out += [Tensor(layer, 'gamma', (3 * H,), s.og, (2, G), (d,), pad, init=ONES),
                    Tensor(layer, 'beta', (3 * H,), s.obeta, (2, G), (d,), pad),
                    Tensor(layer, 'running_mean', (3 * H,), s.orun, (2, G), (d,), pad,
                           buf='running'),
                    Tensor(layer, 'running_std', (3 * H,), ovar, (2, G), (d,), pad, init=ONES,
                           buf='running', fill=1.0)]
        else:
            out.append(Tensor(layer, 'b', (3 * H,), s.ob, ax + (G,), at, pad))
    return out


def birhn(s, alloc, rows):
    """Bidirectional(RHN) (csrc/rhn.hip): W (in, 2, C Hp), U (2, L, Hp, C Hp), b (2, L, C Hp),
    column blocks h, t [, c] (C = 2 when coupled).  Per direction: W, U_0 .. U_{L-1}, b_0 ..
    b_{L-1}; the highway bias -2 goes to the real t (and c) entries only, pads stay 0."""
    H, Hp, F, L, C = s.H, s.Hp, len(rows), s.depth, s.nblk
    G, pad = C * Hp, ('blocks', H, Hp, C)
    s.oW, s.oU, s.ob = (alloc.take(s.f_in_pad * 2 * G), alloc.take(2 * L * Hp * G),
                        alloc.take(2 * L * G))
    out = []
    for d, layer in enumerate(('forward_rhn', 'backward_rhn')):
        out.append(Tensor(layer, 'W', (F, C * H), s.oW, (s.f_in_pad, 2, G), (rows, d), pad,
                          s.l2_W, _glorot(F, C * H)))
        out += [Tensor(layer, '%d_U' % l, (H, C * H), s.oU, (2, L, Hp, G), (d, l, slice(0, H)),
                       pad, s.l2_U, ('orthogonal', 1.1)) for l in range(L)]
        out += [Tensor(layer, '%d_b' % l, (C * H,), s.ob, (2, L, G), (d, l), pad,
                       init=('blocks', (0.0,) + (-2.0,) * (C - 1))) for l in range(L)]
    return out


def bn(s, alloc, cols):
    """BatchNormalization (csrc/batchnorm.hip): gamma, beta (C each) in the flat parameters;
    running mean | variance in Model.bn_running (not trainable); the moments block of the
    running update behind the gradients' flag slots, so that data parallel the gradient
    all-reduce pools it over the ranks.  cols: the channels that carry real features."""
    C, n, layer = s.C, len(cols), 'batchnormalization'
    s.og, s.obeta = alloc.take(C), alloc.take(C)
    s.orun, ovar = alloc.take(C, 'running'), alloc.take(C, 'running')
    s.omom = alloc.take(ops.bn_moments_len(C), 'moments')
    return [Tensor(layer, 'gamma', (n,), s.og, (C,), (cols,), init=ONES),
            Tensor(layer, 'beta', (n,), s.obeta, (C,), (cols,)),
            Tensor(layer, 'running_mean', (n,), s.orun, (C,), (cols,), buf='running'),
            Tensor(layer, 'running_std', (n,), ovar, (C,), (cols,), init=ONES, buf='running',
                   fill=1.0)]


def ln(s, alloc, cols):
    """LayerNormalization (csrc/layernorm.hip): gain, bias (one entry per physical column of the
    slab row, s.ld) in the flat parameters, no l2; the pad columns stay 0.  cols: the columns
    that carry real features."""
    W, n, layer = s.ld, len(cols), 'layernormalization'
    s.og, s.obeta = alloc.take(W), alloc.take(W)
    return [Tensor(layer, 'gain', (n,), s.og, (W,), (cols,), init=ONES),
            Tensor(layer, 'bias', (n,), s.obeta, (W,), (cols,))]


def mha(s, alloc, rows):
    """MultiHeadAttention (csrc/attention.hip): W_qkv (F, 3D) = [W_q | W_k | W_v], b_qkv (3D),
    W_o (D, n_out), b_o (n_out), D = heads * dh; each of the three projection blocks is drawn
    glorot-uniform on its own (limit sqrt(6 / (F + D))); l2 on the two matrices."""
    F, D, layer = len(rows), s.D, 'multiheadattention'
    lim = math.sqrt(6.0 / (F + D))
    s.oW, s.ob = alloc.take(s.f_in_pad * 3 * D), alloc.take(3 * D)
    s.oWo, s.obo = alloc.take(D * s.n_out), alloc.take(s.n_out)
    return [Tensor(layer, 'W_qkv', (F, 3 * D), s.oW, (s.f_in_pad, 3 * D), (rows,), l2=s.l2,
                   init=('uniform', lim)),
            Tensor(layer, 'b_qkv', (3 * D,), s.ob, (3 * D,), ()),
            Tensor(layer, 'W_o', (D, s.n_out), s.oWo, (D, s.n_out), (), l2=s.l2,
                   init=_glorot(D, s.n_out)),
            Tensor(layer, 'b_o', (s.n_out,), s.obo, (s.n_out,), ())]


def relmha(s, alloc, rows):
    """RelativeMultiHeadAttention (csrc/rel_attention.hip): mha's W_qkv, b_qkv, then W_pos (D, D),
    the projection of the relative sinusoidal table (no bias), pos_bias_u and pos_bias_v
    (heads, dh), then W_o, b_o.  W_pos and the two position biases are glorot-uniform over their
    own shapes; l2 on the three matrices."""
    F, D, layer = len(rows), s.D, 'relativemultiheadattention'
    lim = math.sqrt(6.0 / (F + D))
    s.oW, s.ob = alloc.take(s.f_in_pad * 3 * D), alloc.take(3 * D)
    s.oWp, s.obu, s.obv = alloc.take(D * D), alloc.take(D), alloc.take(D)
    s.oWo, s.obo = alloc.take(D * s.n_out), alloc.take(s.n_out)
    hd = (s.heads, s.dh)
    return [Tensor(layer, 'W_qkv', (F, 3 * D), s.oW, (s.f_in_pad, 3 * D), (rows,), l2=s.l2,
                   init=('uniform', lim)),
            Tensor(layer, 'b_qkv', (3 * D,), s.ob, (3 * D,), ()),
            Tensor(layer, 'W_pos', (D, D), s.oWp, (D, D), (), l2=s.l2, init=_glorot(D, D)),
            Tensor(layer, 'pos_bias_u', hd, s.obu, hd, (), init=_glorot(*hd)),
            Tensor(layer, 'pos_bias_v', hd, s.obv, hd, (), init=_glorot(*hd)),
            Tensor(layer, 'W_o', (D, s.n_out), s.oWo, (D, s.n_out), (), l2=s.l2,
                   init=_glorot(D, s.n_out)),
            Tensor(layer, 'b_o', (s.n_out,), s.obo, (s.n_out,), ())]


def dwconv(s, alloc, rows):
    """DepthwiseConvolution1D (csrc/dwconv.hip): W (k, C) tap major, glorot-uniform with fan_in =
    fan_out = k (one filter per channel: limit sqrt(3 / k)), b (C); l2 on W."""
    layer = 'depthwiseconvolution1d'
    s.oW, s.ob = alloc.take(s.k * s.C), alloc.take(s.C)
    return [Tensor(layer, 'W', (s.k, s.C), s.oW, (s.k, s.C), (), l2=s.l2, init=_glorot(s.k, s.k)),
            Tensor(layer, 'b', (s.C,), s.ob, (s.C,), ())]
