"""The stage kinds of the engine, each described once: ``KINDS`` (at the end of this module) maps
a spec ``type`` to a ``Kind`` of three plain functions, and ``Model._layout`` / ``forward`` /
``backward`` (core/engine.py) are loops that look the kind up.

  build(m, s, st, width)          copies and checks the spec fields of ``st`` onto the Stage ``s``,
                                  calls the kind's builder of the parameter table (core/params.py,
                                  on ``m._alloc``) and returns the new ``(f_real, f_pad)`` from
                                  ``width``, the one it is given
  forward(m, s, si, a, rec, fp)   returns the output slab for the input slab ``a``; what BPTT
                                  reads again goes into ``rec`` (``model._acts[si]``)
  backward(m, s, si, rec, da, bp) returns the gradient with respect to the stage input, or None
                                  when it passes through unchanged or nothing upstream needs it

``fp`` / ``bp`` are the state of one pass (a ``Pass``), filled by ``Model.forward`` / ``backward``:
fp: training, masks, need_grad, n_valid, n_real, bn_weight, seq_len, in_len, n_pad, pipe, pre,
nb (BiLSTM stages seen so far) and stage_masks(i); bp: T, n_pad, rows, n_ref, split, split_side,
overlap, reduce_now, pending, skip_grads, flush_side(), reduce_async() and, per stage, first.
In a model with a TimeReduction stage (the 'treduce' variant of 'reshape', below) the time axis
changes in mid-stack: fp.seq_len is then, for every stage, the lengths on the axis that stage
runs on (``Model.forward`` derives them from in_len by the chain of strides), and the stage's
backward handler sets bp.T / bp.rows to its input's frames for the stages below.

The further fields of a ``Kind`` are the facts the engine reduces over the stage list instead of
keeping lists of kinds: ``mask_shape(s, n_pad)`` (the shape of B_U, for a kind that takes
variational-dropout masks), ``needs_lens`` (forward needs seq_len), ``attention``,
``needs_in_len`` (training needs the input lengths) and ``extra_timeout_flags`` (its kernels'
workspaces carry timeout words of their own).  Whether a stage is the first trainable one is
``s.first``: no stage before it has ``tensors``.

A VARIANT of a kind is a stage of that kind told by an attribute only it carries (``relative`` and
``window`` on 'mha'; ``directions`` = 1 on 'bigru' and on 'bilstm': a bare, unidirectional GRU
or LSTM; ``time_factor`` on 'reshape': TimeReduction, the one reshape that moves data).  The direction count of a recurrent stage is ``_nd(s)``, the one reader of that
attribute: the 'bigru' handlers and the GEMM helpers of the recurrent kinds take it as a number
and serve both forms, the 'bilstm' handlers hand a one-direction stage to ``_lstm_uni_*``, which
use the same helpers.  A variant may stream where its kind does not:
``STREAM_VARIANTS`` (at the end of this module) maps a kind to (is this stage the variant?, its
step handler ``(m, s, si, a, ss)``), and ``stream_variant(s)`` is what ``stream_check`` and
``StreamSession._encoder`` consult FIRST, before ``Kind.stream`` -- which stays None for 'bigru'.

A new stage kind is one builder in params.py and one entry here.  The two-direction LSTM stage is
the scheduled hot path (pipe and side streams, compact BPTT, packed planes, per-layer all-reduce):
its ``forward`` / ``backward`` are written like the handlers here but fill a module of their own,
core/bilstm.py, with their helpers, predicates and switches; the 'bilstm' entry calls them.
"""
import collections

import numpy as np

from .. import ops
from . import params as P
from .params import _pad4


class Pass(object):
    """The state of one forward or backward pass over the stage list."""

    def __init__(self, **state):
        self.__dict__.update(state)


Kind = collections.namedtuple(
    'Kind', 'build forward backward mask_shape needs_lens attention needs_in_len '
            'extra_timeout_flags stream', defaults=(None, False, False, False, False, None))

# K26, chunk-by-chunk inference (core/stream.py).  ``stream(m, s, si, a, ss)`` runs a stage on the
# slab ``a`` of the ss.Tq new frames [ss.t0, ss.t0 + ss.Tq) of a StreamSession ``ss``, whose
# ss.state[si] holds what the stage carries from step to step; ``stream_check(m, s, si)`` (below)
# says why a stage cannot stream.  The kinds of STREAM_AS_FORWARD are per-frame or the identity
# at inference (bn: the running moments): the session calls their ``forward`` on the chunk slab.
# A 'conv' stage belongs to the front-end, which the session runs itself.
# A VARIANT of a kind may stream where the kind as such does not: the unidirectional GRU is a
# 'bigru' stage with one direction.  ``stream_variant(s)`` (below, from STREAM_VARIANTS at the end
# of this module) gives such a stage's step handler, or None; ``StreamSession._encoder`` and
# ``stream_check`` ask it first, before ``Kind.stream``.  The 'bigru' kind itself has no handler:
# the bidirectional layer reads the whole utterance.
STREAM_AS_FORWARD = ('dense', 'ln', 'act', 'glu', 'merge', 'reshape', 'dropout', 'noise',
                     'specaug', 'bn')


def _no_fields(m, s, st, width):
    return width


def _same_slab(m, s, si, a, rec, fp):
    return a


def _pass_through(m, s, si, rec, da, bp):
    return None


# --------------------------------------------------------------------------- noise, dropout
def _noise_build(m, s, st, width):
    s.value = st['value']
    s.wrapped = bool(st.get('wrapped', False))      # TimeDistributed(Dropout)
    return width


def _noise_forward(m, s, si, a, rec, fp):
    if fp.training and s.value > 0:
        out = m._buf('noise%d' % si, a.shape)
        a = ops.gaussian_noise(a, out, s.value, m.rng_seed, 4 * si, m._step)
        if s.f_out_pad != s.f_out and all(p.kind == 'specaug' for p in m.stages[:si]):
            a[:, :, s.f_out:] = 0.0        # keep the input pad columns zero
    return a


def _dropout_forward(m, s, si, a, rec, fp):
    if fp.training and s.value > 0:
        keep = m._buf('dropmask%d' % si, a.shape)
        out = m._buf('dropout%d' % si, a.shape)
        a = ops.dropout_apply(a, out, keep, s.value, 1.0 / (1.0 - s.value),
                              m.rng_seed, 4 * si, m._step)
        rec['mask'] = keep
    return a


def _dropout_backward(m, s, si, rec, da, bp):
    if bp.first:               # nothing trainable upstream: no gradient needed there
        return None
    if 'mask' in rec:
        return ops.mul(da, rec['mask'], m._buf('ddrop%d' % si, da.shape))
    return None


# --------------------------------------------------------------------------- reshape, specaug
def _reshape_build(m, s, st, width):
    s.target = [int(v) for v in st['target']]
    if st.get('time_factor'):       # (only then: the stages of every other model are unchanged)
        return _treduce_build(m, s, st, width)
    return width


# TimeReduction (K33, csrc/timestack.hip) is the 'treduce' VARIANT of the reshape kind: batch
# major, stacking k frames IS keras' Reshape((-1, k F)) of the (T, F) block of an utterance; in
# the time-major slab it moves data, and it changes the time axis.  ``time_factor(s)`` is the one
# reader of the attribute ``time_factor``, which only a variant stage carries.
def time_factor(s):
    """k of a TimeReduction stage, 0 for every other stage."""
    return getattr(s, 'time_factor', 0) if s.kind == 'reshape' else 0


def _refuse_behind_treduce(m, what, why):
    if any(time_factor(p) for p in m.stages):
        raise ValueError('%s behind a TimeReduction stage: %s' % (what, why))


def _treduce_build(m, s, st, width):
    # the stage changes the TIME axis, so what cannot cross it is refused when the model is built
    # (here, in _merge_build, _conv_build and _specaug_build)
    f_real, f_pad = width
    k = int(st['time_factor'])
    lo, hi = ops.TIME_STACK_FACTORS
    if not lo <= k <= hi:
        raise NotImplementedError('TimeReduction: factor %d (in %d .. %d: the limits of '
                                  'asr_time_stack_*)' % (k, lo, hi))
    if s.target != [-1, k * f_real]:
        raise ValueError('TimeReduction(%d) of %d features: target %r' % (k, f_real, s.target))
    if not np.array_equal(m._real_rows(s), np.arange(f_real)):
        raise NotImplementedError(
            'TimeReduction behind a layer whose two directions are padded apart (%d features in '
            '%d columns): the stacked frame takes the leading columns only; use a hidden width '
            'that is a multiple of 4' % (f_real, f_pad))
    s.time_factor = k
    return k * f_real, _pad4(k * f_real)


def _reshape_forward(m, s, si, a, rec, fp):
    """A view -- or, TimeReduction: y[to] = [x[to k], .., x[to k + k - 1]] behind the length mask
    of the stage's OWN time axis (fp.seq_len: Model.forward hands every stage of such a model
    the lengths of the axis it runs on).  Nothing but the input shape is kept for the backward
    pass, which is the transpose of a copy."""
    k = time_factor(s)
    if not k:
        return a
    a = a.contiguous()
    T, n_pad, _ = a.shape
    N = min(fp.n_real, n_pad)
    rec.update(shape=tuple(a.shape), N=N, lens=fp.seq_len)
    out = m._buf('treduce%d' % si, (ops.time_stack_frames(T, k), n_pad, s.f_out_pad))
    return ops.time_stack_fwd(a, out, N, s.f_in, k, lens=fp.seq_len)


def _reshape_backward(m, s, si, rec, da, bp):
    """TimeReduction: the stages below run on the longer axis, so bp.T / bp.rows become the
    input's.  (Work that is already queued for the side stream keeps the values it was queued
    with: the record ``g`` of a BiLSTM stage copies them when its BPTT is launched.)"""
    k = time_factor(s)
    if not k:
        return None
    T, n_pad, _ = rec['shape']
    bp.T, bp.rows = T, T * n_pad
    if bp.first:
        return None
    dx = m._buf('dtreduce%d' % si, rec['shape'])
    return ops.time_stack_bwd(da.contiguous(), dx, rec['N'], s.f_in, k, lens=rec['lens'])


def _specaug_build(m, s, st, width):
    # SpecAugment (K23, csrc/specaug.hip): augments DATA, so nothing trainable and no
    # time stride may come before it (no backward pass exists for it, and its
    # lengths are the input's); its limits are checked here, not at the first launch
    s.policy = {k: st[k] for k in ('time_warp', 'freq_masks', 'freq_width',
                                   'time_masks', 'time_width', 'time_ratio')}
    ops.specaug_check(**s.policy)
    s.policy['mask_value'] = float(st.get('mask_value', 0.0))
    _refuse_behind_treduce(m, 'SpecAugment', 'it augments the input data, within the lengths of '
                           'the input time axis')
    if any(p.tensors or getattr(p, 'st', 1) > 1 for p in m.stages):
        raise ValueError(
            'SpecAugment behind a trainable or time-strided layer: it augments the '
            'input data (per utterance, on the input time axis), not activations, '
            'and belongs directly behind Input')
    return width


def _specaug_forward(m, s, si, a, rec, fp):
    if fp.training:        # (never in place: the caller keeps its slab)
        out = m._buf('specaug%d' % si, a.shape)
        a = ops.specaug_apply(a.contiguous(), out, min(fp.n_real, fp.n_pad), s.f_in,
                              m.rng_seed, 4 * si, m._step, lens=fp.in_len,
                              **s.policy)
    return a


# --------------------------------------------------------------------------- act, glu, posenc
def _act_build(m, s, st, width):
    s.act = st['activation']        # 'tanh' / 'relu' / 'linear' / clipped_relu()
    s.wrapped = bool(st.get('wrapped', False))      # TimeDistributed(Activation)
    return width


def _act_forward(m, s, si, a, rec, fp):
    if not getattr(s, 'fused', False):     # (else applied by the BN stage before)
        out = m._buf('act%d' % si, a.shape)
        a = ops.activation_fwd(a.contiguous(), out, s.act)
    return a


def _act_backward(m, s, si, rec, da, bp):
    if not bp.first and not getattr(s, 'fused', False):
        # (swish: its derivative is read from the stage INPUT)
        return ops.activation_bwd(da.contiguous(), rec['out'],
                                  m._buf('dact%d' % si, da.shape), s.act,
                                  x=rec['in'].contiguous() if s.act == 'swish' else None)
    return None


def _glu_build(m, s, st, width):
    f_real, f_pad = width
    if f_real % 8 or f_pad != f_real:
        raise NotImplementedError(
            'GLU over %d features (%d columns): the width must be a multiple of 8 '
            'without pad columns' % (f_real, f_pad))
    s.C = f_real // 2
    return s.C, s.C


def _glu_forward(m, s, si, a, rec, fp):
    a = a.contiguous()
    rec['in'] = a
    return ops.glu_fwd(a, m._buf('glu%d' % si, (a.shape[0], fp.n_pad, s.C)))


def _glu_backward(m, s, si, rec, da, bp):
    if not bp.first:
        a_in = rec['in']
        return ops.glu_bwd(a_in, da.contiguous(), m._buf('dglu%d' % si, a_in.shape))
    return None


def _posenc_build(m, s, st, width):
    s.D = width[0]                  # (no parameters: the table depends on (T, D) only)
    return width


def _posenc_forward(m, s, si, a, rec, fp):
    out = m._buf('posenc%d' % si, a.shape)
    return ops.posenc_add(a.contiguous(), out, min(fp.n_real, fp.n_pad), s.D)


def _posenc_stream(m, s, si, a, ss):
    """The rows [t0, t0 + Tq) of the table: it has no end, the session takes it ever longer."""
    out = m._buf('posenc%d' % si, a.shape)
    return ops.posenc_add(a.contiguous(), out, ss.N, s.D, pe=ss.posenc_rows(s.D))


# --------------------------------------------------------------------------- merge
def _merge_build(m, s, st, width):
    f_real, f_pad = width
    s.mode, s.skip = st['mode'], int(st['skip'])
    s.scale = float(st.get('scale', 1.0))   # of the first input ('sum' only)
    if s.scale != 1.0 and s.mode != 'sum':
        raise NotImplementedError("merge(scale=%r): with mode='sum' only" % s.scale)
    src = m.stages[s.skip]
    if any(time_factor(p) for p in m.stages[s.skip + 1:]):
        raise ValueError('merge: the skip connection spans a TimeReduction stage: its two inputs '
                         'would be on different time axes; put the merge on one side of the stage')
    if (src.f_out, src.f_out_pad) != (f_real, f_pad):
        raise ValueError('merge: widths differ (%d vs %d)' % (src.f_out, f_real))
    s.coef = 1.0 if s.mode == 'sum' else 0.5
    return width


def _merge_forward(m, s, si, a, rec, fp):       # residual: c * (scale * new + skip)
    out = m._buf('merge%d' % si, a.shape)
    return ops.axpby(s.coef * s.scale, a, s.coef, m._acts[s.skip]['out'], out)


def _merge_backward(m, s, si, rec, da, bp):
    """The skip input's share waits in bp.skip_grads until the loop reaches that stage."""
    if s.coef != 1.0:
        da = ops.axpby(s.coef, da, 0.0, da, m._buf('dmerge%d' % si, da.shape))
    bp.skip_grads[s.skip] = da
    if s.scale != 1.0:          # the branch gets scale * d, the skip d
        da = ops.axpby(s.scale, da, 0.0, da, m._buf('dscale%d' % si, da.shape))
    return da


# --------------------------------------------------------------------------- dense
def _dense_build(m, s, st, width):
    s.n_out = st['n_out']
    s.l2 = st.get('l2', 0.0)
    s.tensors = P.dense(s, m._alloc, m._real_rows(s))
    s.in_map = None
    return s.n_out, s.n_out


def _dense_forward(m, s, si, a, rec, fp):
    T = a.shape[0]
    out = m._buf('dense%d' % si, (T, fp.n_pad, s.n_out))
    ops.gemm(a, m.params, out, T * fp.n_pad, s.n_out, s.f_in_pad, b_off=s.oW,
             bias=m._view(s.ob, s.n_out))
    return out


def _dense_backward(m, s, si, rec, da, bp):
    T, n_pad, rows = bp.T, bp.n_pad, bp.rows
    gmx = ops.absmax(da, m._buf('damax%d' % si, (1,)))
    ops.gemm(rec['in'], da, m.grads, s.f_in_pad, s.n_out, rows, trans_a=True,
             c_off=s.oW, split_k=bp.split, b_absmax=gmx)
    ops.colsum(da, rows, s.n_out, s.n_out, m._gview(s.ob, s.n_out))
    if bp.first:
        return None
    dx = m._buf('da_s%d' % si, (T, n_pad, s.f_in_pad))
    ops.gemm(da, m.params, dx, rows, s.f_in_pad, s.n_out, trans_b=True,
             b_off=s.oW, a_absmax=gmx)
    return dx


# --------------------------------------------------------------------------- conv
def _conv_build(m, s, st, width):
    # 2-D convolution front-end (K13): W (kt, kf, C_in, C_out) + b (C_out), Keras
    # 'tf' kernel layout; the slab keeps its channel-minor rows (F * C)
    f_real, f_pad = width
    for k in ('F_in', 'C_in', 'C_out', 'kt', 'kf', 'st', 'sf'):
        setattr(s, k, int(st[k]))
    s.clip, s.l2 = float(st['clip']), float(st.get('l2', 0.0))
    s.F_out = -(-s.F_in // s.sf)
    if f_real != s.F_in * s.C_in or f_pad != f_real:
        raise ValueError('conv stage: %d input features (a multiple of 4) expected, '
                         'got %d (padded %d)' % (s.F_in * s.C_in, f_real, f_pad))
    if (s.F_out * s.C_out) % 4:
        raise ValueError('conv stage: F_out * C_out must be a multiple of 4')
    # limits of asr_conv2d_* (csrc/conv.hip), checked when the model is BUILT rather
    # than at the first launch / the first backward pass:
    if not 1 <= s.kt <= 16:
        raise ValueError('conv stage: kernel length over time %d not in 1..16 '
                         '(asr_conv2d_* keeps one plane shift per time tap)' % s.kt)
    if s.st < 1 or s.sf < 1:
        raise ValueError('conv stage: strides must be >= 1')
    _refuse_behind_treduce(m, 'a conv stage', 'the convolution front-end reads the (time, '
                           'frequency) image of the input, and a stacked frame is k frames of it '
                           'side by side')
    if s.st > 1 and any(p.tensors for p in m.stages):
        raise ValueError(
            'conv stage with time stride %d behind a trainable stage: asr_conv2d_dgrad '
            'exists for time stride 1 only, so a time-strided convolution must be the '
            'FIRST trainable stage (its input is data and needs no gradient)' % s.st)
    s.tensors = P.conv(s, m._alloc, None)
    return s.F_out * s.C_out, s.F_out * s.C_out


def _conv_op(m, si, s, T, n_pad):
    """The ops.Conv2d of stage si for this slab shape (owns the layer's workspace: the
    packed planes of x and dz live there between the forward and backward calls)."""
    key = (si, int(T), int(n_pad))
    op = m._convs.get(key)
    if op is None:
        for k in [k for k in m._convs if k[0] == si]:
            del m._convs[k]
        op = m._convs[key] = ops.Conv2d(T, n_pad, s.F_in, s.C_in, s.C_out, s.kt, s.kf,
                                        s.st, s.sf, s.clip, m.device)
    return op


def _conv_forward(m, s, si, a, rec, fp):
    op = _conv_op(m, si, s, a.shape[0], fp.n_pad)
    # clipped ReLU: applied in the GEMM epilogue, only y exists (its mask
    # 0 < z < clip reads the same from y); linear: y is z
    y = m._buf('convy%d' % si, (op.T_out, fp.n_pad, s.F_out * s.C_out))
    nw = s.kt * s.kf * s.C_in * s.C_out
    op.fwd(a.contiguous(), m._view(s.oW, nw), m._view(s.ob, s.C_out),
           None if s.clip > 0 else y, y, x_absmax=m._clip_bound(si))
    rec.update(op=op, z=y)
    return y


def _conv_backward(m, s, si, rec, da, bp):
    bp.flush_side()
    op, z, a_in = rec['op'], rec['z'], rec['in']
    nw = s.kt * s.kf * s.C_in * s.C_out
    da = da.contiguous()
    dx = None
    if not bp.first:
        dx = m._buf('da_s%d' % si, a_in.shape)
        op.dgrad(da, z, m._view(s.oW, nw), dx)
    # (x planes: still in the layer's workspace from the forward call; dz's, if dgrad ran)
    op.wgrad(a_in, da, z, m._gview(s.oW, nw), m._gview(s.ob, s.C_out),
             reuse_x=True, reuse_dz=dx is not None)
    return dx


# --------------------------------------------------------------------------- dwconv
def _dwconv_build(m, s, st, width):
    # depthwise convolution over time (K22, csrc/dwconv.hip); its limits are checked
    # here, when the model is built, not at the first launch
    f_real, f_pad = width
    s.k, s.C, s.l2 = int(st['k']), f_real, float(st.get('l2', 0.0))
    if s.k < 1 or s.k > ops.DWCONV_MAX_KERNEL or s.k % 2 == 0:
        raise NotImplementedError(
            "DepthwiseConvolution1D: kernel_size %d (odd, in 1 .. %d: 'same' padding, "
            'the tile of asr_dwconv1d_*)' % (s.k, ops.DWCONV_MAX_KERNEL))
    if f_real % 4 or f_pad != f_real:
        raise NotImplementedError(
            'DepthwiseConvolution1D over %d channels (%d columns): the width must be '
            'a multiple of 4 without pad columns' % (f_real, f_pad))
    if st.get('causal'):            # (only then: the stages of every other model are unchanged)
        s.pad_left = s.k - 1        # the causal left padding, in place of the 'same' (k - 1) / 2
    s.tensors = P.dwconv(s, m._alloc, None)
    return width


def _dwconv_forward(m, s, si, a, rec, fp):
    N = min(fp.n_real, fp.n_pad)
    a = a.contiguous()
    # (the keyword only when set: the calls of every other model are what they were)
    pad = {'pad_left': s.pad_left} if hasattr(s, 'pad_left') else {}
    rec.update(**{'in': a, 'N': N, 'lens': fp.seq_len, 'pad': pad})
    out = m._buf('dwconv%d' % si, a.shape)
    return ops.dwconv1d_fwd(a, m._view(s.oW, s.k * s.C), m._view(s.ob, s.C), out,
                            N, s.k, lens=fp.seq_len, **pad)


def _dwconv_backward(m, s, si, rec, da, bp):
    # dW / db into the gradients, dx behind the same length mask
    a_in = rec['in']
    dx = None if bp.first else m._buf('ddwconv%d' % si, a_in.shape)
    ops.dwconv1d_bwd(a_in, m._view(s.oW, s.k * s.C), da.contiguous(), dx,
                     m._gview(s.oW, s.k * s.C),
                     m._buf('dwdb%d' % si, (s.C,)) if s.bias_dead
                     else m._gview(s.ob, s.C), rec['N'], s.k, lens=rec['lens'],
                     **rec['pad'])
    return dx


def _dwconv_stream(m, s, si, a, ss):
    """The causal convolution of the new frames: they go into the stage's ring of input frames
    (k - 1 + step rows, zero-filled when created or reset), which holds the k - 1 frames before
    them from the steps before."""
    a = a.contiguous()
    st = ss.state.setdefault(si, {})
    if 'ring' not in st:
        st['ring'] = ss.zeros((s.k - 1 + ss.step, a.shape[1], a.shape[2]))
    ops.ring_put(a, st['ring'], ss.t0)
    out = m._buf('dwconv%d' % si, a.shape)
    return ops.dwconv1d_stream_fwd(st['ring'], m._view(s.oW, s.k * s.C), m._view(s.ob, s.C),
                                   ss.lens, out, ss.N, s.k, ss.t0)


# --------------------------------------------------------------------------- bn
def _bn_build(m, s, st, width):
    f_real, f_pad = width
    s.eps, s.momentum = float(st.get('epsilon', 1e-3)), float(st.get('momentum', 0.99))
    fc = st.get('fc')
    s.grouped = fc is not None and int(fc[1]) < f_pad
    if s.grouped:
        s.C = int(fc[1])            # per channel of the (N, T, F, C) conv image
        if f_pad != f_real or f_pad != int(fc[0]) * s.C or s.C % 4 or s.C > 256:
            raise NotImplementedError(
                'BatchNormalization on an (N, T, %d, %d) image: the channel count '
                'must be a multiple of 4, at most 256' % (int(fc[0]), s.C))
    else:
        s.C = f_pad                 # per column, pad columns get gamma = beta = 0
        if f_pad % 4:
            raise NotImplementedError('BatchNormalization over %d features: the '
                                      'width must be a multiple of 4' % f_real)
    s.n_real = s.C if s.grouped else f_real
    s.clip = 0.0                    # > 0: a following clipped ReLU fused (Model._layout)
    s.tensors = P.bn(s, m._alloc, m._bn_cols(s))
    return width


def _bn_forward(m, s, si, a, rec, fp):
    """BatchNormalization stage: batch statistics of the n_real real rows in training (saved
    for the backward pass; the moments block of the running update written behind the flag
    slots), the running moments otherwise."""
    a = a.contiguous()
    T, n_pad, ld = a.shape
    y = m._buf('bn%d' % si, a.shape)
    gamma, beta = m._view(s.og, s.C), m._view(s.obeta, s.C)
    rm, rv, mom = m._bn_views(s, s.C)
    if not fp.training:
        return ops.bn_fwd_infer(a, y, gamma, beta, rm, rv, min(fp.n_real, n_pad), ld, s.C,
                                s.eps, s.clip)
    stats = m._buf('bnstats%d' % si, (ops.bn_stats_len(s.C),))
    # data parallel the moments are taken about the running mean (the same on every rank),
    # weighted by the rank's real frames, and pooled by the gradient all-reduce
    dist = m._dist_active()
    ops.bn_fwd_train(a, y, gamma, beta, stats, min(fp.n_real, n_pad), ld, s.C, s.eps, s.clip,
                     moments=mom, shift=rm if dist else None,
                     weight=float(fp.bn_weight * T))
    rec.update(stats=stats, N=min(fp.n_real, n_pad), shift=None if dist else stats[:s.C])
    return y


def _bn_backward(m, s, si, rec, da, bp):
    # dgamma / dbeta into the gradients, dx from the saved statistics (x re-read)
    a_in = rec['in']
    dx = None if bp.first else m._buf('dbn%d' % si, a_in.shape)
    ops.bn_bwd(a_in.contiguous(), da.contiguous(), m._view(s.og, s.C),
               m._view(s.obeta, s.C), rec['stats'], dx, m._gview(s.og, s.C),
               m._gview(s.obeta, s.C), rec['N'], a_in.shape[2], s.C, s.clip)
    return dx


# --------------------------------------------------------------------------- ln
def _ln_build(m, s, st, width):
    # LayerNormalization (K20, csrc/layernorm.hip): per frame over its real columns,
    # which it keeps as it is given them (like 'bn': no projection of its own)
    f_real, f_pad = width
    s.eps = float(st.get('epsilon', 1e-5))
    cols = m._real_rows(s)
    s.ld = f_pad
    if np.array_equal(cols, np.arange(f_real)):
        s.segs, s.seg_H, s.seg_Hp = 1, f_real, f_pad
    else:       # [0, H) and [Hp, Hp + H): two directions padded apart
        s.segs, s.seg_H = 2, len(cols) // 2
        s.seg_Hp = int(cols[s.seg_H])
    if f_pad % 4 or s.seg_Hp % 4 or s.segs * s.seg_Hp > f_pad:
        raise NotImplementedError('LayerNormalization over %d features: the width '
                                  'must be a multiple of 4' % f_real)
    if f_pad > ops.LN_MAX_WIDTH:
        raise NotImplementedError(
            'LayerNormalization over %d features (%d columns): the asr_ln_* kernels '
            'keep a row in the registers of one wave, at most %d columns'
            % (f_real, f_pad, ops.LN_MAX_WIDTH))
    s.tensors = P.ln(s, m._alloc, cols)
    return width


def _ln_forward(m, s, si, a, rec, fp):
    """LayerNormalization stage: the same pass in training and inference; (mu, 1 / sigma)
    of every row is kept only when a backward pass will read it."""
    a = a.contiguous()
    T, n_pad, ld = a.shape
    y = m._buf('ln%d' % si, a.shape)
    N = min(fp.n_real, n_pad)
    stats = m._buf('lnstats%d' % si, (ops.ln_stats_len(T, n_pad),)) if fp.need_grad else None
    ops.ln_fwd(a, y, m._view(s.og, ld), m._view(s.obeta, ld), N, s.seg_H, s.seg_Hp,
               s.segs, s.eps, stats=stats)
    rec.update(stats=stats, N=N)
    return y


def _ln_backward(m, s, si, rec, da, bp):
    # dgain / dbias into the gradients, dx from the saved (mu, 1 / sigma) (x re-read)
    a_in = rec['in']
    ld = a_in.shape[2]
    dx = None if bp.first else m._buf('dln%d' % si, a_in.shape)
    ops.ln_bwd(a_in.contiguous(), da.contiguous(), m._view(s.og, ld), rec['stats'],
               dx, m._gview(s.og, ld), m._gview(s.obeta, ld), rec['N'],
               s.seg_H, s.seg_Hp, s.segs)
    return dx


# --------------------------------------------------------------------------- mha
def _mha_build(m, s, st, width):
    # multi-head self-attention (K21, csrc/attention.hip): the [Q | K | V] projection,
    # the fused attention core, the output projection
    s.heads, s.dh = int(st['heads']), int(st['dh'])
    s.D, s.n_out, s.l2 = s.heads * s.dh, int(st['n_out']), float(st.get('l2', 0.0))
    if st.get('context') is not None:       # (only then, like relative below)
        s.window = _mha_window(st['context'])   # (chunk, left, right) of K25, csrc/attn_tile.h
    if st.get('relative'):          # (only then: the stages of every other model are unchanged)
        return _relmha_build(m, s, st, width)
    if s.heads < 1 or s.dh % 16 or not 16 <= s.dh <= 128:
        raise NotImplementedError(
            'MultiHeadAttention: head_dim %d (a multiple of 16 in 16 .. 128: the tile '
            'of the asr_attn_* kernels), %d heads' % (s.dh, s.heads))
    s.tensors = P.mha(s, m._alloc, m._real_rows(s))
    return s.n_out, s.n_out


def _mha_window(context):
    w = tuple(int(v) for v in context)
    if len(w) != 3 or w[0] < 1 or w[1] < -1 or w[2] < 0:
        raise ValueError('MultiHeadAttention: context %r ([chunk >= 1, left >= -1 (-1: unlimited), '
                         'right >= 0] in frames)' % (context,))
    return w


def _mha_forward(m, s, si, a, rec, fp):
    """MultiHeadAttention stage: qkv = a W_qkv + b_qkv (one GEMM), the fused attention core
    over each utterance's valid keys (seq_len: device lengths on this time axis; None: every
    frame), the output projection.  The row log-sum-exp is kept only for a backward pass."""
    if getattr(s, 'relative', False):
        return _relmha_forward(m, s, si, a, rec, fp)
    a = a.contiguous()
    T, n_pad, _ = a.shape
    rows, D, N = T * n_pad, s.D, min(fp.n_real, n_pad)
    # (the keyword only when set: the calls of every other model are what they were)
    win = {'window': s.window} if hasattr(s, 'window') else {}
    qkv = m._buf('qkv%d' % si, (T, n_pad, 3 * D))
    ops.gemm(a, m.params, qkv, rows, 3 * D, s.f_in_pad, b_off=s.oW,
             bias=m._view(s.ob, 3 * D))
    ctx = m._buf('attn%d' % si, (T, n_pad, D))
    lse = m._buf('lse%d' % si, (ops.attn_lse_len(T, n_pad, s.heads),)) if fp.need_grad \
        else None
    ops.attn_fwd(qkv, ctx, N, s.heads, s.dh, lens=fp.seq_len, lse=lse, **win)
    out = m._buf('mha%d' % si, (T, n_pad, s.n_out))
    ops.gemm(ctx, m.params, out, rows, s.n_out, D, b_off=s.oWo,
             bias=m._view(s.obo, s.n_out))
    rec.update(qkv=qkv, ctx=ctx, lse=lse, N=N, lens=fp.seq_len, win=win)
    return out


def _mha_backward(m, s, si, rec, da, bp):
    """The two projections' wgrad / colsum / dgrad GEMMs around asr_attn_bwd; returns dx, or
    None for the first trainable stage.  The relative variant: asr_relattn_bwd in its place,
    which also writes dpos and the two position-bias gradients; dW_pos = pe^T dpos."""
    a_in = rec['in'].contiguous()
    split = bp.split
    T, n_pad, _ = a_in.shape
    rows, D = T * n_pad, s.D
    da = da.contiguous()
    gmx = ops.absmax(da, m._buf('damax%d' % si, (1,)))
    ops.gemm(rec['ctx'], da, m.grads, D, s.n_out, rows, trans_a=True, c_off=s.oWo,
             split_k=split, b_absmax=gmx)
    ops.colsum(da, rows, s.n_out, s.n_out, m._gview(s.obo, s.n_out))
    dctx = m._buf('dattn%d' % si, (T, n_pad, D))
    ops.gemm(da, m.params, dctx, rows, D, s.n_out, trans_b=True, b_off=s.oWo,
             a_absmax=gmx)
    dqkv = m._buf('dqkv%d' % si, (T, n_pad, 3 * D))
    if getattr(s, 'relative', False):
        dpos = m._buf('drelpos%d' % si, (2 * T - 1, D))
        ops.relattn_bwd(rec['qkv'], rec['pos'], m._view(s.obu, D), m._view(s.obv, D),
                        rec['ctx'], rec['lse'], dctx, dqkv, dpos, m._gview(s.obu, D),
                        m._gview(s.obv, D), rec['N'], s.heads, s.dh, lens=rec['lens'],
                        **rec['win'])
        # dW_pos = pe^T dpos with the constant 1 taken off the cosine columns (sum_r dpos_r = 0:
        # ops.relpos_grad_table), in exact fp32: the table's small entries are below fp16's range
        ops.gemm(ops.relpos_get(T, D, dpos.device, grad=True), dpos, m.grads, D, D, 2 * T - 1,
                 trans_a=True, c_off=s.oWp, split_k=split, precision=0)
    else:
        ops.attn_bwd(rec['qkv'], rec['ctx'], rec['lse'], dctx, dqkv, rec['N'], s.heads, s.dh,
                     lens=rec['lens'], **rec['win'])
    qmx = ops.absmax(dqkv, m._buf('dqkvmax%d' % si, (1,)))
    ops.gemm(a_in, dqkv, m.grads, s.f_in_pad, 3 * D, rows, trans_a=True, c_off=s.oW,
             split_k=split, b_absmax=qmx)
    # db_q and db_v.  Softmax does not see a shift of all scores of a row, so the key bias
    # has no effect and its gradient is identically 0: a column sum of dK would leave
    # rounding noise there, which Adam would normalise into steps of +-lr.  It is never
    # produced: that third of the gradient keeps the zero the buffer is created with.
    ops.colsum(dqkv, rows, D, 3 * D, m._gview(s.ob, D))
    ops.colsum(dqkv, rows, D, 3 * D, m._gview(s.ob + 2 * D, D), x_off=2 * D)
    if bp.first:
        return None
    dx = m._buf('da_s%d' % si, (T, n_pad, s.f_in_pad))
    ops.gemm(dqkv, m.params, dx, rows, s.f_in_pad, 3 * D, trans_b=True, b_off=s.oW,
             a_absmax=qmx)
    return dx


def _relmha_build(m, s, st, width):
    # the relative variant of the mha kind (K24, csrc/rel_attention.hip): RelativeMultiHeadAttention
    s.relative = True
    if s.heads < 1 or s.dh % 16 or not 16 <= s.dh <= ops.RELATTN_MAX_HEAD_DIM:
        raise NotImplementedError(
            'RelativeMultiHeadAttention: head_dim %d (a multiple of 16 in 16 .. %d: the band '
            'tiles of the asr_relattn_* kernels leave no LDS for more), %d heads'
            % (s.dh, ops.RELATTN_MAX_HEAD_DIM, s.heads))
    s.tensors = P.relmha(s, m._alloc, m._real_rows(s))
    return s.n_out, s.n_out


def _relmha_forward(m, s, si, a, rec, fp):
    """RelativeMultiHeadAttention stage: the qkv GEMM, Pos = pe W_pos (the (2T - 1, D) relative
    table: it does not depend on the batch, one GEMM per forward pass of the stage), the fused
    relative attention core, the output projection."""
    a = a.contiguous()
    T, n_pad, _ = a.shape
    rows, D, N = T * n_pad, s.D, min(fp.n_real, n_pad)
    # (the keyword only when set: the calls of every other model are what they were)
    win = {'window': s.window} if hasattr(s, 'window') else {}
    qkv = m._buf('qkv%d' % si, (T, n_pad, 3 * D))
    ops.gemm(a, m.params, qkv, rows, 3 * D, s.f_in_pad, b_off=s.oW,
             bias=m._view(s.ob, 3 * D))
    pe = ops.relpos_get(T, D, a.device)
    pos = m._buf('relpos%d' % si, (2 * T - 1, D))
    ops.gemm(pe, m.params, pos, 2 * T - 1, D, D, b_off=s.oWp, precision=0)    # (exact fp32)
    ctx = m._buf('attn%d' % si, (T, n_pad, D))
    lse = m._buf('lse%d' % si, (ops.attn_lse_len(T, n_pad, s.heads),)) if fp.need_grad \
        else None
    ops.relattn_fwd(qkv, pos, m._view(s.obu, D), m._view(s.obv, D), ctx, N, s.heads, s.dh,
                    lens=fp.seq_len, lse=lse, **win)
    out = m._buf('mha%d' % si, (T, n_pad, s.n_out))
    ops.gemm(ctx, m.params, out, rows, s.n_out, D, b_off=s.oWo,
             bias=m._view(s.obo, s.n_out))
    rec.update(qkv=qkv, ctx=ctx, lse=lse, N=N, lens=fp.seq_len, pos=pos, win=win)
    return out


def _mha_stream(m, s, si, a, ss):
    """Both attention variants on the new frames: the qkv GEMM of the chunk, its [K | V] columns
    into the stage's ring (THE RING of csrc/attn_tile.h, zero-filled when created or reset), the
    streaming attention core of the new queries against the ring, the output projection.  The
    relative table covers the relative indices of a visible pair, -(P - 1) .. P - 1 with P = left
    + chunk; it is projected once per session (pe W_pos, exact fp32, as _relmha_forward does)."""
    a = a.contiguous()
    Tq, n_pad, _ = a.shape
    rows, D = Tq * n_pad, s.D
    chunk, left, _ = s.window
    st = ss.state.setdefault(si, {})
    if 'ring' not in st:
        st['ring'] = ss.zeros((ops.attn_stream_plan(s.window, ss.step), n_pad, 2 * D))
    qkv = m._buf('qkv%d' % si, (Tq, n_pad, 3 * D))
    ops.gemm(a, m.params, qkv, rows, 3 * D, s.f_in_pad, b_off=s.oW, bias=m._view(s.ob, 3 * D))
    ops.ring_put(qkv, st['ring'], ss.t0, col0=D, cols=2 * D)
    ctx = m._buf('attn%d' % si, (Tq, n_pad, D))
    if getattr(s, 'relative', False):
        if 'pos' not in st:
            P_ = left + chunk
            st['pos'] = ss.zeros((2 * P_ - 1, D))
            ops.gemm(ops.relpos_get(P_, D, a.device), m.params, st['pos'], 2 * P_ - 1, D, D,
                     b_off=s.oWp, precision=0)
        ops.relattn_stream_fwd(qkv, st['ring'], ss.lens, st['pos'], m._view(s.obu, D),
                               m._view(s.obv, D), ctx, ss.N, s.heads, s.dh, ss.t0, s.window)
    else:
        ops.attn_stream_fwd(qkv, st['ring'], ss.lens, ctx, ss.N, s.heads, s.dh, ss.t0, s.window)
    out = m._buf('mha%d' % si, (Tq, n_pad, s.n_out))
    ops.gemm(ctx, m.params, out, rows, s.n_out, D, b_off=s.oWo, bias=m._view(s.obo, s.n_out))
    return out


def stream_check(m, s, si):
    """Why stage si cannot run chunk by chunk (K26), or None: no device is touched."""
    kind = KINDS[s.kind]
    if stream_variant(s) is not None:
        return None
    if time_factor(s):
        return ('it is a TimeReduction stage: a session counts frames on one time axis (its '
                'chunks, rings and committed prefix are in the frames of the encoder), and the '
                'stage changes the axis in mid-stack')
    if s.kind == 'mha':
        w = getattr(s, 'window', None)
        if w is None or w[1] < 0 or w[2] != 0:
            return ('its context is %r: a streaming attention layer needs a window (chunk, left '
                    '>= 0, 0), a bounded left context and no right context' % (w,))
    elif s.kind == 'dwconv':
        if getattr(s, 'pad_left', None) != s.k - 1:
            return 'it is not causal (causal=True: no output frame reads a later input frame)'
    elif s.kind == 'conv':
        return None                 # (the front-end: checked as a whole by the session)
    elif kind.stream is None and s.kind not in STREAM_AS_FORWARD:
        return 'a %s stage reads the whole utterance' % s.kind
    return None


# --------------------------------------------------------------------------- one or two directions
def _nd(s):
    """The directions of a recurrent stage ``s`` (or of the spec entry one is being built from):
    2, or 1 for a bare GRU / LSTM, the one-direction variant of 'bigru' / 'bilstm'.  The attribute
    ``directions`` is set on a variant stage only, and read here only."""
    return s.get('directions', 2) if isinstance(s, dict) else getattr(s, 'directions', 2)


def _rec_fields(s, st, merge=True):
    """What the recurrent kinds share; merge: Bidirectional(SimpleRNN | GRU | RHN) (csrc/rnn.hip,
    gru.hip, rhn.hip), whose two outputs are concatenated or summed."""
    s.H = st['H']
    s.Hp = _pad4(s.H)
    if merge:
        s.merge = st.get('merge_mode', 'concat')
    s.act = st.get('activation') or 'tanh'      # (LSTM: core/layers.py:452, :463)
    s.dropout_W, s.dropout_U = st.get('dropout_W', 0.0), st.get('dropout_U', 0.0)
    s.l2_W, s.l2_U = st.get('l2_W', 0.0), st.get('l2_U', 0.0)


def _uni_stream(keys):
    """The step handler of a one-direction stage whose state is one (n_pad, Hp) vector per key
    ('h', and 'c' for the LSTM): the stage's own forward handler on the new frames, from the
    state into the other buffer of each pair, then the swaps.  The pairs are zero-filled when
    created or reset (StreamSession.reset); there is no ring."""
    def step(m, s, si, a, ss):
        st = ss.state.setdefault(si, {})
        for k in keys:
            if k not in st:
                st[k] = [ss.zeros((a.shape[1], s.Hp)), ss.zeros((a.shape[1], s.Hp))]
        # h0 / h_last (and c0 / c_last) of the recurrence: the first buffer of a pair, the second
        carry = {k + sfx: t for k in keys for sfx, t in zip(('0', '_last'), st[k])}
        out = KINDS[s.kind].forward(m, s, si, a, {}, ss._pass(), carry)
        for k in keys:
            st[k].reverse()
        return out
    return step


# --------------------------------------------------------------------------- bilstm
def _bilstm_build(m, s, st, width):
    if _nd(st) == 1:
        return _lstm_uni_build(m, s, st, width)
    _rec_fields(s, st, merge=False)
    s.mi = st.get('mi')                     # [alpha, beta1, beta2] inits or None
    s.ln = st.get('layer_norm')             # [gain_init, bias_init] or None
    s.zoneout_c = float(st.get('zoneout_c') or 0.0)
    s.zoneout_h = float(st.get('zoneout_h') or 0.0)
    s.tensors = P.bilstm(s, m._alloc, m._real_rows(s))
    return 2 * s.H, 2 * s.Hp


def _bilstm_forward(m, s, si, a, rec, fp, carry=None):
    if _nd(s) == 1:
        return _lstm_uni_forward(m, s, si, a, rec, fp, carry)
    from . import bilstm        # (imports Pass and _nd from here)
    return bilstm.forward(m, s, si, a, rec, fp)


def _bilstm_backward(m, s, si, rec, da, bp):
    if _nd(s) == 1:
        return _lstm_uni_backward(m, s, si, rec, da, bp)
    from . import bilstm
    return bilstm.backward(m, s, si, rec, da, bp)


# The unidirectional LSTM (K29, csrc/lstm_uni.hip): the one-direction variant of the kind, as the
# unidirectional GRU is of 'bigru' (below).  None of the scheduled paths of the bidirectional
# body (packed planes, pipe and side streams, compact BPTT) applies to it: bilstm.py asks its
# ``is_bilstm`` (kind 'bilstm' AND two directions) wherever it decides one of them.  What
# is here is the LSTM's own (the buffers, the recurrence, db); the GEMMs are the shared helpers'
# (below) with one direction and G = 4 Hp.
def _lstm_uni_build(m, s, st, width):
    """mi / ln are None and the zoneouts 0, for whoever reads them off a 'bilstm' stage."""
    for k in ('mi', 'layer_norm', 'zoneout_c', 'zoneout_h'):
        if st.get(k):
            raise NotImplementedError('a unidirectional LSTM stage has no %s: the kernels of '
                                      'csrc/lstm_uni.hip are the plain cell only' % k)
    s.directions = 1
    _rec_fields(s, st, merge=False)
    s.mi = s.ln = None
    s.zoneout_c = s.zoneout_h = 0.0
    s.tensors = P.lstm_uni(s, m._alloc, m._real_rows(s))
    return s.H, s.Hp


def _lstm_uni_forward(m, s, si, a, rec, fp, carry=None):
    """zx (T, n_pad, 4Hp) = (a (.) B_W) @ W + b, then the recurrence: from the zero state, or
    (streaming, _uni_stream) with the state arguments ``carry``."""
    a = a.contiguous()
    n_pad = fp.n_pad
    T, Hp = a.shape[0], s.Hp
    BW, BU = fp.stage_masks(si)[:2]
    rec['BW'], rec['BU'] = BW, BU
    zx = m._buf('uzx%d' % si, (T, n_pad, 4 * Hp))
    _rec_proj(m, a, s, zx, 4 * Hp, BW, T * n_pad, n_pad, bias=m._view(s.ob, 4 * Hp), nd=1)
    h = m._buf('uh%d' % si, (T, n_pad, Hp))
    cell = m._buf('ucell%d' % si, (T, n_pad, Hp))
    gates = m._buf('ugates%d' % si, (T, n_pad, 4 * Hp))
    ops.lstm_uni_seq_fwd(zx, m._view(s.oU, Hp * 4 * Hp), h, cell, gates, T, n_pad, Hp, act=s.act,
                         mask_u=None if BU is None else BU[0], **(carry or {}))
    rec.update(h=h, cell=cell, gates=gates)
    return h


def _lstm_uni_backward(m, s, si, rec, da, bp):
    """BPTT from the zero state, then dU = (h_prev (.) B_U)^T dz over the (T - 1) n_pad rows that
    have an h_prev, dW = (x (.) B_W)^T dz, db from the per-batch-tile sums, dx = B_W (.)
    (dz @ W^T).  Returns dx (or None)."""
    T, n_pad = da.shape[0], da.shape[1]
    Hp, G = s.Hp, 4 * s.Hp
    BW, BU, h = rec['BW'], rec['BU'], rec['h']
    BU = None if BU is None else BU[0]
    dz = m._buf('udz%d' % si, (T, n_pad, G))
    dbp = m._buf('udbp%d' % si, (n_pad // 16, G))
    zmx = m._buf('udzmax%d' % si, (1,))
    ops.lstm_uni_seq_bwd(da.contiguous(), m._view(s.oU, Hp * G), h, rec['cell'], rec['gates'], dz,
                         T, n_pad, Hp, act=s.act, mask_u=BU, db_part=dbp, dz_absmax=zmx)
    ops.colsum(dbp, n_pad // 16, G, G, m._gview(s.ob, G))
    _rec_du_prev(m, h, dz, s.oU, 0, G, G, T, n_pad, Hp, BU, bp.split, zmx, nd=1)
    _rec_dw(m, rec['in'].contiguous(), dz, s, G, BW, T * n_pad, n_pad, bp.split, zmx, nd=1)
    return _rec_dx(m, dz, s, si, G, BW, T, n_pad, zmx, bp.first, nd=1)


def _mask_shape(s, n_pad):
    return (2, n_pad, s.Hp)


# --------------------------------------------------------------------------- SimpleRNN, GRU, RHN
def _rec_width(s):
    return (2 * s.H, 2 * s.Hp) if _nd(s) == 2 and s.merge == 'concat' else (s.H, s.Hp)


def _birnn_build(m, s, st, width):
    _rec_fields(s, st)
    s.init = st.get('init', 'glorot_uniform')
    s.tensors = P.birnn(s, m._alloc, m._real_rows(s))
    return _rec_width(s)


def _bigru_build(m, s, st, width):
    """Bidirectional(GRU), or a bare GRU (K28): the one-direction variant of the kind, which has
    no merge and no batch normalisation of the projection."""
    nd = _nd(st)
    if nd == 1:
        if st.get('batch_norm'):
            raise NotImplementedError('a unidirectional GRU stage has no batch_norm: the '
                                      'sequence-wise normalisation kernels take both directions '
                                      'of a layer')
        s.directions = 1
    _rec_fields(s, st, merge=nd == 2)
    # batch_norm (K18, csrc/batchnorm.hip): sequence-wise BN of the input projection
    s.bn = bool(st.get('batch_norm', False))
    if s.bn:
        s.bn_eps = float(st.get('bn_epsilon', 1e-3))
        s.bn_momentum = float(st.get('bn_momentum', 0.99))
    s.tensors = P.bigru(s, m._alloc, m._real_rows(s),
                        ('forward_gru', 'backward_gru') if nd == 2 else ('gru',))
    return _rec_width(s)


def _birhn_build(m, s, st, width):
    _rec_fields(s, st)
    s.depth = int(st.get('depth', 1))
    s.coupling = bool(st.get('coupling', True))
    s.nblk = 2 if s.coupling else 3
    s.tensors = P.birhn(s, m._alloc, m._real_rows(s))
    return _rec_width(s)


def _birhn_mask_shape(s, n_pad):
    # (one B_U per level, all from the one stream 4 * stage + 1)
    return (2, s.depth, n_pad, s.Hp)


# The GEMMs around a recurrence (SimpleRNN, GRU, RHN, the one-direction GRU and LSTM).  G is the
# gate width of one direction: the rows of zx and of the gate gradient dg hold the nd directions
# of the stage, nd G wide, and so do W's.  A one-direction stage is handed the (2, n_pad, .) mask
# pair of its kind like any other (same shapes, streams and step) and reads direction 0 of it.
def _rec_proj(m, a, s, zx, G, BW, rows, n_pad, bias=None, nd=2):
    """zx = (a (.) B_W[d]) @ W_d (+ b_d), every direction; bias (nd G) or None."""
    if BW is None:
        ops.gemm(a, m.params, zx, rows, nd * G, s.f_in_pad, b_off=s.oW, bias=bias)
        return
    for d in range(nd):
        ops.gemm(a, m.params, zx, rows, G, s.f_in_pad, ldb=nd * G, ldc=nd * G,
                 b_off=s.oW + d * G, c_off=d * G,
                 bias=None if bias is None else bias[d * G:(d + 1) * G],
                 a_scale=BW[d], a_scale_period=n_pad)


def _rec_dw(m, a_in, dg, s, G, BW, rows, n_pad, split, zmx, nd=2):
    """dW[d] = (x (.) B_W[d])^T dg_d."""
    if BW is None:
        ops.gemm(a_in, dg, m.grads, s.f_in_pad, nd * G, rows, trans_a=True, c_off=s.oW,
                 split_k=split, b_absmax=zmx)
        return
    for d in range(nd):
        ops.gemm(a_in, dg, m.grads, s.f_in_pad, G, rows, trans_a=True, ldb=nd * G,
                 ldc=nd * G, b_off=d * G, c_off=s.oW + d * G, split_k=split,
                 a_scale=BW[d], a_scale_period=n_pad, b_absmax=zmx)


def _rec_dx(m, dg, s, si, G, BW, T, n_pad, zmx, first, nd=2):
    """dx = sum_d B_W[d] (.) (dg_d @ W_d^T); None for the first stage."""
    if first:
        return None
    rows = T * n_pad
    dx = m._buf('da_s%d' % si, (T, n_pad, s.f_in_pad))
    if BW is None:
        ops.gemm(dg, m.params, dx, rows, s.f_in_pad, nd * G, trans_b=True, b_off=s.oW,
                 a_absmax=zmx)
        return dx
    for d in range(nd):
        ops.gemm(dg, m.params, dx, rows, s.f_in_pad, G, trans_b=True, lda=nd * G,
                 ldb=nd * G, a_off=d * G, b_off=s.oW + d * G, c_scale=BW[d],
                 c_scale_period=n_pad, beta=0.0 if d == 0 else 1.0, a_absmax=zmx)
    return dx


def _rec_du_prev(m, h, dg, c_off, d, G, N, T, n_pad, Hp, scale, split, zmx, h_off=0, nd=2):
    """grads[c_off:] (Hp, G), columns [0, N) = (h_prev (.) scale)^T dg_d[:, :N], where h_prev is
    the slab h (T, n_pad, nd, Hp) at h_off one frame earlier in direction d's processing
    order: 0 before the first frame, so T == 1 leaves zeros."""
    kk = (T - 1) * n_pad
    if kk > 0:
        ops.gemm(h, dg, m.grads, Hp, N, kk, trans_a=True, lda=nd * Hp, ldb=nd * G, ldc=G,
                 a_off=h_off + d * Hp + (0 if d == 0 else n_pad * nd * Hp),
                 b_off=d * G + (n_pad * nd * G if d == 0 else 0), c_off=c_off,
                 split_k=split, a_scale=scale, a_scale_period=n_pad, b_absmax=zmx)
    else:
        m._gview(c_off, Hp * G).view(Hp, G)[:, :N].zero_()


def _birnn_forward(m, s, si, a, rec, fp):
    T, n_pad, Hp = a.shape[0], fp.n_pad, s.Hp
    BW, BU = fp.stage_masks(si)[:2]
    rec['BW'], rec['BU'] = BW, BU
    zx = m._buf('rzx%d' % si, (T, n_pad, 2, Hp))
    _rec_proj(m, a.contiguous(), s, zx, Hp, BW, T * n_pad, n_pad,
              bias=m._view(s.ob, 2 * Hp))
    h = m._buf('rh%d' % si, (T, n_pad, 2, Hp))
    ysum = m._buf('rsum%d' % si, (T, n_pad, Hp)) if s.merge == 'sum' else None
    rec['ws'] = ops.rnn_seq_fwd(zx, m._view(s.oU, 2 * Hp * Hp), h, T, n_pad, Hp,
                                act=s.act, mask_u=BU, y_sum=ysum, mode=m.lstm_mode)
    rec['h'] = h
    return ysum if ysum is not None else h.view(T, n_pad, 2 * Hp)


def _birnn_backward(m, s, si, rec, da, bp):
    """BPTT of a SimpleRNN stage (csrc/rnn.hip), then its weight gradients and dx from the
    GEMMs: dU[d] = (h_prev (.) B_U)^T dz_d, dW[d] = (x (.) B_W)^T dz_d, db from BPTT's
    per-batch-tile sums, dx = sum_d B_W[d] (.) (dz_d @ W_d^T).  Returns dx (or None)."""
    split = bp.split
    T, n_pad = da.shape[0], da.shape[1]
    rows, Hp = T * n_pad, s.Hp
    BW, BU, h, a_in = rec['BW'], rec['BU'], rec['h'], rec['in']
    dz = m._buf('rdz%d' % si, (T, n_pad, 2, Hp))
    dbp = m._buf('rdbp%d' % si, (n_pad // 16, 2, Hp))
    zmx = m._buf('rdzmax%d' % si, (1,))
    rec['ws_b'] = ops.rnn_seq_bwd(da.contiguous(), m._view(s.oU, 2 * Hp * Hp), h, dz, T,
                                  n_pad, Hp, act=s.act, mask_u=BU,
                                  shared_dy=s.merge == 'sum', mode=m.lstm_mode,
                                  db_part=dbp, dz_absmax=zmx)
    ops.colsum(dbp, n_pad // 16, 2 * Hp, 2 * Hp, m._gview(s.ob, 2 * Hp))
    for d in range(2):
        _rec_du_prev(m, h, dz, s.oU + d * Hp * Hp, d, Hp, Hp, T, n_pad, Hp,
                     None if BU is None else BU[d], split, zmx)
    _rec_dw(m, a_in, dz, s, Hp, BW, rows, n_pad, split, zmx)
    return _rec_dx(m, dz, s, si, Hp, BW, T, n_pad, zmx, bp.first)


def _bigru_forward(m, s, si, a, rec, fp, carry=None):
    """GRU stage, one or two directions (csrc/gru.hip): zx = (a (.) B_W[d]) @ W_d + b_d from the
    GEMMs, then the recurrence; h, the gates z | r | hh and r (.) m are kept for BPTT.
    batch_norm: the GEMMs write the bias-free projection p into a buffer of the layer (the
    backward pass reads it again), and zx = BN(p) goes to a scratch all layers share (BPTT
    never reads zx).  carry: the state arguments of a one-direction stage that streams."""
    a = a.contiguous()
    n_pad, nd = fp.n_pad, _nd(s)
    T, Hp = a.shape[0], s.Hp
    dirs = (2,) if nd == 2 else ()          # (one direction: the slabs have no direction axis)
    BW, BU = fp.stage_masks(si)[:2]
    rec['BW'], rec['BU'] = BW, BU
    zx = m._buf('gzx%d' % si, (T, n_pad) + dirs + (3 * Hp,))
    _rec_proj(m, a, s, zx, 3 * Hp, BW, T * n_pad, n_pad,
              bias=None if s.bn else m._view(s.ob, nd * 3 * Hp), nd=nd)
    if s.bn:
        zx = _seqbn_forward(m, s, si, zx, rec, fp)
    h = m._buf('gh%d' % si, (T, n_pad) + dirs + (Hp,))
    gates = m._buf('ggates%d' % si, (T, n_pad) + dirs + (3 * Hp,))
    rm = m._buf('grm%d' % si, (T, n_pad) + dirs + (Hp,))
    rec.update(h=h, gates=gates, rm=rm)
    U = m._view(s.oU, nd * Hp * 3 * Hp)
    if nd == 1:
        ops.gru_uni_seq_fwd(zx, U, h, gates, rm, T, n_pad, Hp, act=s.act,
                            mask_u=None if BU is None else BU[0], **(carry or {}))
        return h
    ysum = m._buf('gsum%d' % si, (T, n_pad, Hp)) if s.merge == 'sum' else None
    ops.gru_seq_fwd(zx, U, h, gates, rm, T, n_pad, Hp, act=s.act, mask_u=BU, y_sum=ysum)
    return ysum if ysum is not None else h.view(T, n_pad, 2 * Hp)


def _seqbn_forward(m, s, si, p, rec, fp):
    """zx = BN(p) of a GRU(batch_norm=True) stage (K18): batch statistics over the valid frames
    in training (saved, with p, for the backward pass; the moments block of the running
    update written behind the flag slots), the running moments otherwise."""
    T, n_pad = p.shape[0], p.shape[1]
    Wd = 6 * s.Hp
    N = min(int(fp.n_real or n_pad), n_pad)
    p3 = p.view(T, n_pad, Wd)
    y = m._buf('gzxbn_%d' % Wd, (T, n_pad, Wd))
    gamma, beta = m._view(s.og, Wd), m._view(s.obeta, Wd)
    rm, rv, mom = m._bn_views(s, Wd)
    if not fp.training:
        ops.seqbn_fwd_infer(p3, y, gamma, beta, rm, rv, N, Wd, s.bn_eps)
        return y.view(T, n_pad, 2, 3 * s.Hp)
    stats = m._buf('gbnstats%d' % si, (ops.seqbn_stats_len(Wd),))
    # (data parallel: moments about the running mean, pooled by the gradient all-reduce, as
    # in _bn_forward; the weight |V| is counted on the device, 0 for a zero-weight dummy)
    dist = m._dist_active()
    ops.seqbn_fwd_train(p3, y, gamma, beta, stats, N, Wd, lens=fp.seq_len, eps=s.bn_eps,
                        moments=mom, shift=rm if dist else None,
                        weight=0.0 if fp.bn_weight == 0 else 1.0)
    rec.update(p=p3, stats=stats, N=N, lens=fp.seq_len, shift=None if dist else stats[:Wd])
    return y.view(T, n_pad, 2, 3 * s.Hp)


def _bigru_backward(m, s, si, rec, da, bp):
    """BPTT of a GRU stage (csrc/gru.hip; one direction: from the zero state), then its weight
    gradients and dx from the GEMMs:
    dU_z, dU_r [d] = (h_prev (.) B_U)^T [da_z | da_r], dU_h[d] = (r (.) m)^T da_h (r (.) m
    kept by the forward pass), dW[d] = (x (.) B_W)^T da_d, db from the per-batch-tile sums,
    dx = sum_d B_W[d] (.) (da_d @ W_d^T).  Returns dx (or None)."""
    split, nd = bp.split, _nd(s)
    T, n_pad = da.shape[0], da.shape[1]
    rows, Hp, G = T * n_pad, s.Hp, 3 * s.Hp
    dirs = (2,) if nd == 2 else ()
    BW, BU, h, a_in = rec['BW'], rec['BU'], rec['h'], rec['in']
    dg = m._buf('gda%d' % si, (T, n_pad) + dirs + (G,))
    dbp = m._buf('gdbp%d' % si, (n_pad // 16,) + dirs + (G,))
    zmx = m._buf('gdamax%d' % si, (1,))
    U = m._view(s.oU, nd * Hp * G)
    if nd == 1:
        ops.gru_uni_seq_bwd(da.contiguous(), U, h, rec['gates'], dg, T, n_pad, Hp, act=s.act,
                            mask_u=None if BU is None else BU[0], db_part=dbp, dz_absmax=zmx)
    else:
        ops.gru_seq_bwd(da.contiguous(), U, h, rec['gates'], dg, T, n_pad, Hp, act=s.act,
                        mask_u=BU, shared_dy=s.merge == 'sum', db_part=dbp, dz_absmax=zmx)
    if not s.bn:
        ops.colsum(dbp, n_pad // 16, nd * G, nd * G, m._gview(s.ob, nd * G))
    for d in range(nd):
        oU = s.oU + d * Hp * G
        _rec_du_prev(m, h, dg, oU, d, G, 2 * Hp, T, n_pad, Hp,
                     None if BU is None else BU[d], split, zmx, nd=nd)
        ops.gemm(rec['rm'], dg, m.grads, Hp, Hp, rows, trans_a=True, lda=nd * Hp,
                 ldb=nd * G, ldc=G, a_off=d * Hp, b_off=d * G + 2 * Hp,
                 c_off=oU + 2 * Hp, split_k=split, b_absmax=zmx)
    if s.bn:
        # dU above came from da; dW and dx come from dp = BN'(da), which has its own absmax
        # (dbeta is what colsum(db_part) would give: the one reduction pass writes both)
        dp = m._buf('gdp_%d' % (6 * Hp), (T, n_pad, 6 * Hp))
        zmx = m._buf('gdpmax%d' % si, (1,))
        ops.seqbn_bwd(rec['p'], dg.view(T, n_pad, 6 * Hp), m._view(s.og, 6 * Hp),
                      rec['stats'], dp, m._gview(s.og, 6 * Hp), rec['N'], 6 * Hp,
                      lens=rec['lens'], dbeta=m._gview(s.obeta, 6 * Hp), dp_absmax=zmx)
        dg = dp
    _rec_dw(m, a_in.contiguous(), dg, s, G, BW, rows, n_pad, split, zmx, nd=nd)
    return _rec_dx(m, dg, s, si, G, BW, T, n_pad, zmx, bp.first, nd=nd)


def _birhn_forward(m, s, si, a, rec, fp):
    """Bidirectional(RHN) stage (csrc/rhn.hip): zx = (a (.) B_W[d]) @ W_d from the GEMMs (the
    kernel adds every level's bias), then the recurrence; the states and gates of all levels
    are kept for BPTT, level-major.  B_U is (2, L, n_pad, Hp): one mask per level."""
    a = a.contiguous()
    n_pad = fp.n_pad
    T, Hp, Ld, Wd = a.shape[0], s.Hp, s.depth, s.nblk * s.Hp
    rows = T * n_pad
    BW, BU = fp.stage_masks(si)[:2]
    rec['BW'], rec['BU'] = BW, BU
    zx = m._buf('hzx%d' % si, (T, n_pad, 2, Wd))
    _rec_proj(m, a, s, zx, Wd, BW, rows, n_pad)
    h = m._buf('hh%d' % si, (Ld, T, n_pad, 2, Hp))
    gates = m._buf('hgates%d' % si, (Ld, T, n_pad, 2, Wd))
    ysum = m._buf('hsum%d' % si, (T, n_pad, Hp)) if s.merge == 'sum' else None
    ops.rhn_seq_fwd(zx, m._view(s.oU, 2 * Ld * Hp * Wd), m._view(s.ob, 2 * Ld * Wd), h,
                    gates, T, n_pad, Hp, Ld, coupling=s.coupling, act=s.act, mask_u=BU,
                    y_sum=ysum)
    rec.update(h=h, gates=gates)
    return ysum if ysum is not None else h[Ld - 1].view(T, n_pad, 2 * Hp)


def _birhn_backward(m, s, si, rec, da, bp):
    """BPTT of an RHN stage (csrc/rhn.hip), then its weight gradients and dx from the GEMMs:
    dU_l[d] = (s_prev^l (.) B_U[d, l])^T da^l, where s_prev^l is the states slab of level
    l - 1 or, for l = 0, slab L - 1 one frame earlier in the direction's processing order;
    dW[d] = (x (.) B_W)^T da^0_d, db from the per-batch-tile sums,
    dx = sum_d B_W[d] (.) (da^0_d @ W_d^T).  Returns dx (or None)."""
    split = bp.split
    T, n_pad = da.shape[0], da.shape[1]
    rows, Hp, Ld, Wd = T * n_pad, s.Hp, s.depth, s.nblk * s.Hp
    BW, BU, h, a_in = rec['BW'], rec['BU'], rec['h'], rec['in']
    dg = m._buf('hda%d' % si, (Ld, T, n_pad, 2, Wd))
    dbp = m._buf('hdbp%d' % si, (n_pad // 16, 2, Ld, Wd))
    zmx = m._buf('hdamax%d' % si, (1,))
    ops.rhn_seq_bwd(da.contiguous(), m._view(s.oU, 2 * Ld * Hp * Wd), h, rec['gates'], dg,
                    T, n_pad, Hp, Ld, coupling=s.coupling, act=s.act, mask_u=BU,
                    shared_dy=s.merge == 'sum', db_part=dbp, dz_absmax=zmx)
    ops.colsum(dbp, n_pad // 16, 2 * Ld * Wd, 2 * Ld * Wd, m._gview(s.ob, 2 * Ld * Wd))
    for d in range(2):
        for l in range(Ld):
            oU = s.oU + (d * Ld + l) * Hp * Wd
            scale = None if BU is None else BU[d, l]
            if l > 0:
                ops.gemm(h, dg, m.grads, Hp, Wd, rows, trans_a=True, lda=2 * Hp,
                         ldb=2 * Wd, ldc=Wd, a_off=(l - 1) * rows * 2 * Hp + d * Hp,
                         b_off=l * rows * 2 * Wd + d * Wd, c_off=oU, split_k=split,
                         a_scale=scale, a_scale_period=n_pad, b_absmax=zmx)
            else:
                _rec_du_prev(m, h, dg, oU, d, Wd, Wd, T, n_pad, Hp, scale, split, zmx,
                             h_off=(Ld - 1) * rows * 2 * Hp)
    _rec_dw(m, a_in.contiguous(), dg, s, Wd, BW, rows, n_pad, split, zmx)
    return _rec_dx(m, dg, s, si, Wd, BW, T, n_pad, zmx, bp.first)


KINDS = {
    'noise': Kind(_noise_build, _noise_forward, _pass_through),
    'dropout': Kind(_noise_build, _dropout_forward, _dropout_backward),
    'reshape': Kind(_reshape_build, _reshape_forward, _reshape_backward),
    'specaug': Kind(_specaug_build, _specaug_forward, _pass_through, needs_in_len=True),
    'act': Kind(_act_build, _act_forward, _act_backward),
    'glu': Kind(_glu_build, _glu_forward, _glu_backward),
    'posenc': Kind(_posenc_build, _posenc_forward, _pass_through,    # d(x + pe) / dx = 1
                   stream=_posenc_stream),
    'merge': Kind(_merge_build, _merge_forward, _merge_backward),
    'dense': Kind(_dense_build, _dense_forward, _dense_backward),
    'conv': Kind(_conv_build, _conv_forward, _conv_backward),
    'dwconv': Kind(_dwconv_build, _dwconv_forward, _dwconv_backward, needs_lens=True,
                   stream=_dwconv_stream),
    'bn': Kind(_bn_build, _bn_forward, _bn_backward),
    'ln': Kind(_ln_build, _ln_forward, _ln_backward),
    'mha': Kind(_mha_build, _mha_forward, _mha_backward, needs_lens=True, attention=True,
                stream=_mha_stream),
    'bilstm': Kind(_bilstm_build, _bilstm_forward, _bilstm_backward, mask_shape=_mask_shape),
    'birnn': Kind(_birnn_build, _birnn_forward, _birnn_backward, mask_shape=_mask_shape,
                  extra_timeout_flags=True),
    'bigru': Kind(_bigru_build, _bigru_forward, _bigru_backward, mask_shape=_mask_shape),
    'birhn': Kind(_birhn_build, _birhn_forward, _birhn_backward,
                  mask_shape=_birhn_mask_shape),
}

# Variants of a kind with a step handler of their own (see the K26 note at the top):
# kind -> (says whether a stage is the variant, its stream(m, s, si, a, ss)).  The bare GRU and
# LSTM share one (_uni_stream): the forward handler of training, given the state they carry.
STREAM_VARIANTS = {
    'bigru': (lambda s: _nd(s) == 1, _uni_stream(('h',))),
    'bilstm': (lambda s: _nd(s) == 1, _uni_stream(('h', 'c'))),
}


def stream_variant(s):
    """The step handler of a stage that streams as a variant of its kind, or None."""
    is_variant, handler = STREAM_VARIANTS.get(s.kind, (None, None))
    return handler if handler is not None and is_variant(s) else None
