"""The two-direction LSTM stage, the scheduled hot path: the 'bilstm' handlers of the stage-kind
table (core/stages.py) and what exists only for them -- switches, geometry predicates, packed
operands, the frame-range pipeline on the pipe stream, compact BPTT, weight gradients deferred to
the side stream.  Plain functions over ``(m, s, si, ...)`` as in stages.py; all state stays on the
``Model`` ``m``, whose ``forward`` / ``backward`` call ``begin_forward`` / ``begin_backward`` /
``end_backward`` around their loops.  ``forward`` and ``backward`` here are sequences of phases;
``_handoff`` + ``_mark`` and ``_tail_fork`` say the stream protocol once.
"""
import contextlib
import functools
import os

import torch

from .. import ops
from .stages import Pass, _nd


# --------------------------------------------------------------------------- switches
def switches(m):
    """The switches of the schedule, read once per ``Model`` (``Model.__init__``)."""
    # weight-gradient GEMMs run on a side stream, concurrently with the next
    # layer's persistent BPTT kernel (which occupies only H/16 x chains CUs)
    # ASR_OVERLAP: 1 = always, 0 = never, auto (default) = unless a layer's recurrence
    # fills every CU (cfg3: 2 directions x 4 batch tiles x 32 workgroups = 256): its waves
    # hold 480 of a SIMD's 512 registers, no GEMM wave fits beside them, and a GEMM launched
    # on the side stream only waits (measured: 51.9 vs 52.5 ms per cfg3 step, but every
    # GEMM duration in a profile doubled by the wait) -- decided per batch in forward()
    m._overlap_mode = os.environ.get('ASR_OVERLAP', 'auto')
    m.overlap = m._overlap_mode != '0'
    m._side = torch.cuda.Stream(device=m.device) if m.device.type == 'cuda' else None
    # the GEMMs either side of a recurrence are pipelined against its last steps
    # (frames whose both directions are already final), on a third stream
    # 'auto': only when a layer's recurrence leaves at least half of the CUs to the GEMMs
    # it is pipelined against (cfg2: 64 of 256 workgroups; not cfg3's 256 of 256)
    m._pipeline_mode = os.environ.get('ASR_PIPELINE', 'auto')
    # the recurrence is cut after split/16 of its steps (frames [T-S, S) are final then)
    m._pipe_split16 = min(15, max(9, int(os.environ.get('ASR_PIPE_SPLIT', '13'))))
    # (ASR_PIPE_HALVES=0: the pipelined GEMMs wait for whole frames -- comparison switch)
    m._pipe_halves = os.environ.get('ASR_PIPE_HALVES', '1') != '0'
    m.pipeline = m.overlap and m._pipeline_mode == '1'
    # ASR_BPTT_COMPACT: auto (default) = where a layer's BPTT would fill every CU (cfg3) it is
    # launched in the COMPACT geometry (asr_lstm_args.compact: H/32 workgroups per chain,
    # half the CUs, bit-identical gradients, a longer step) whenever the weight-gradient
    # GEMMs of the layer above are waiting, and those run beside it on the side stream
    # instead of behind it; 0 = never (the serial schedule of rounds 1-4), 1 = wherever the
    # compact kernel exists
    m._compact_mode = os.environ.get('ASR_BPTT_COMPACT', 'auto')
    # ASR_BPTT_PLANES=0: BPTT always writes the fp32 dz slab and a pack pass follows (the
    # round 1-5 path; A/B switch).  Default: BPTT writes the packed planes itself where its
    # kernel can (backward()); per-stage bounds of max|dz| live in _buf('dzbound<si>')
    m._dz_planes_mode = os.environ.get('ASR_BPTT_PLANES', '1') != '0'
    m._dz_bound_key = {}         # stage -> (fault generation, weights epoch) of its bound
    m._weights_epoch = 0         # bumped when weights are replaced from outside
    m._dz_measure_passes = 0     # measuring BPTT passes run so far (first step of a layer)
    m._pipe = torch.cuda.Stream(device=m.device) if m.device.type == 'cuda' else None
    # big GEMMs on operands packed once into split-fp16 planes (ops.pack_hl / gemm_hl);
    # ASR_GEMM_PACKED=0 keeps the convert-per-tile kernels, ASR_GEMM_PREC=0 (exact fp32) too
    # 'auto': from 512 hidden units on (measured: +4 % at 5 x BiLSTM(512) with the 256 x 256
    # tile, -6 % at 5 x BiLSTM(256), where the frame-range pipelining of the per-tile path
    # and the absent pack passes win)
    m._packed_mode = os.environ.get('ASR_GEMM_PACKED', 'auto')
    m.packed = False                       # decided in _layout (needs the stage list)
    m._hl = {}
    m._dz_free = [None, None]    # per dz buffer: the side stream's last reader is done
    m._dz_parity = 0


def packed_on(m):
    """``m.packed``, once the stage list is known (``Model._layout``)."""
    return (os.environ.get('ASR_GEMM_PREC', '1') != '0' and
            (m._packed_mode == '1' or (m._packed_mode == 'auto' and _widest(m) >= 512)))


# --------------------------------------------------------------------------- predicates
def is_bilstm(s):
    """A BIDIRECTIONAL LSTM stage: the one every scheduled path of this module is about (packed
    planes, the sizing by the widest recurrence, the pipe and side streams, compact BPTT).  A
    'bilstm' stage with ``directions`` = 1 is the unidirectional variant (core/stages.py,
    csrc/lstm_uni.hip): it takes none of them."""
    return s.kind == 'bilstm' and _nd(s) == 2


def _y_bounded(s):
    """|h| <= 1 for a BiLSTM stage whose output activation is bounded (h = o * act(c), 0 <= o
    <= 1): only then may a packed operand built from its y take 1 as the tensor bound (x the
    inverted-dropout scale, far below the 2^8 head-room of pow2_scale(1)).  relu / linear /
    softplus carry an unbounded c through: those outputs are measured."""
    return is_bilstm(s) and s.act in ('tanh', 'sigmoid', 'hard_sigmoid', 'softsign')


def stage_packed(m, s):
    """Whether a BiLSTM stage's GEMMs run on packed operands (plain cell only)."""
    return (m.packed and is_bilstm(s) and s.mi is None and s.ln is None
            and s.f_in_pad % 8 == 0 and s.Hp % 8 == 0)      # 16-byte rows of the planes


def _widest(m):
    """Hidden units (padded) of the widest BiLSTM stage, 0 without one."""
    return max([st.Hp for st in m.stages if is_bilstm(st)] + [0])


def _num_cu(m):
    if not hasattr(m, '_num_cu'):
        m._num_cu = torch.cuda.get_device_properties(m.device).multi_processor_count
    return m._num_cu


def _workgroups(m, n_pad):
    """Workgroups of the widest recurrence at ``n_pad``: 2 directions x batch tiles of 16 x
    sixteen units each."""
    return 2 * (n_pad // 16) * ((_widest(m) + 15) // 16)


def recurrence_fills_chip(m, n_pad):
    return m.device.type == 'cuda' and _workgroups(m, n_pad) >= _num_cu(m)


def bptt_compact(m, s, n_pad):
    """True if stage s's BPTT may run in the compact geometry with GEMMs on the CUs it
    leaves free (plain cell, persistent kernels, H = 256 / 512, at most half of the CUs)."""
    if m._compact_mode == '0' or m.device.type != 'cuda' or m.lstm_mode != 0:
        return False
    if not is_bilstm(s) or s.mi is not None or s.ln is not None or s.Hp not in (256, 512):
        return False
    if s.zoneout_c > 0 or s.zoneout_h > 0 or s.act != 'tanh':
        return False
    if os.environ.get('ASR_LSTM_PREC', '1') == '0':
        return False
    if m._compact_mode == '1':
        return True
    return (recurrence_fills_chip(m, n_pad)
            and 2 * (n_pad // 16) * (s.Hp // 32) <= _num_cu(m) // 2)


def pipeline_on(m, n_pad):
    if not m.overlap or m._pipeline_mode == '0':
        return False
    if m._pipeline_mode == '1':
        return True
    return 0 < _workgroups(m, n_pad) <= _num_cu(m) // 2


# --------------------------------------------------------------------------- streams
def _mark(m):
    """A new event behind the work enqueued so far on the current stream."""
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(m.device))
    return ev


@contextlib.contextmanager
def _handoff(m, other, ready=None):
    """Hands the current stream's work over to the stream ``other``: the body runs on ``other``,
    behind ``ready`` (default: an event recorded here and now).  The body ends with ``_mark(m)``
    for whoever waits for its results."""
    if ready is None:
        ready = _mark(m)
    with torch.cuda.stream(other):
        other.wait_event(ready)
        yield


def _tail_fork(m, on_pipe, on_main):
    """Two independent pieces, each a launch-bound GEMM or two of ~25 us (r6): one on the pipe
    stream (idle by now), the other here, which then waits for the first.
    ASR_PIPE_TAIL_FORK=0: both here, ``on_main`` first."""
    if m._pipe is None or os.environ.get('ASR_PIPE_TAIL_FORK', '1') == '0':
        on_main()
        on_pipe()
        return
    with _handoff(m, m._pipe):
        on_pipe()
        done = _mark(m)
    on_main()
    torch.cuda.current_stream(m.device).wait_event(done)


# --------------------------------------------------------------------------- packed operands
def _const_one(m):
    if not hasattr(m, '_one'):
        m._one = torch.ones(1, dtype=torch.float32, device=m.device)
    return m._one


def _pack_weights(m):
    """W of every packed stage -> planes for x@W (reduction over the input features:
    (8H, in)) and for dz@W^T (reduction over the gate columns: (in, 8H)); one pass per W,
    ~0.3 GB per step at cfg3.  Only the FIRST packed stage's planes are needed at once: its
    pack runs on the calling stream, the others' (two small kernels each, launch-bound: 0.15 ms
    of a cfg3 step when they sat in front of the first GEMM) on the side stream beside the
    first layer's work; m._w_ready[si] is the event the stage's first GEMM waits for."""
    m._w_ready = {}
    packed = [(si, s) for si, s in enumerate(m.stages) if stage_packed(m, s)]

    def pack(si, s):
        n = s.f_in_pad * 8 * s.Hp
        w = m.params[s.oW:s.oW + n]
        amax = ops.absmax(w, m._buf('wamax%d' % si, (1,)))
        ops.pack_hl(m.params, s.f_in_pad, 8 * s.Hp, src_off=s.oW, absmax=amax,
                    r=m._planes('Wn%d' % si, s.f_in_pad, 8 * s.Hp),
                    c=m._planes('Wt%d' % si, 8 * s.Hp, s.f_in_pad))
    aside = (m._side is not None and m.device.type == 'cuda' and len(packed) > 1
             and os.environ.get('ASR_PACK_W_ASIDE', '1') != '0')
    for k, (si, s) in enumerate(packed):
        if k == 0 or not aside:
            pack(si, s)
    if aside:
        # (the weights are final on the calling stream here)
        with _handoff(m, m._side):
            for si, s in packed[1:]:
                pack(si, s)
                m._w_ready[si] = _mark(m)


def _await_weights(m, si):
    """The calling stream waits for stage si's weight planes (packed on the side stream)."""
    ev = getattr(m, '_w_ready', {}).pop(si, None)
    if ev is not None:
        torch.cuda.current_stream(m.device).wait_event(ev)


def _pack_input(m, si, s, a, BW, rows, n_pad, amax):
    """The stage's input slab (rows, f_in_pad) [x B_W of each direction] -> (rows, f_in_pad)
    planes: x@W reduces over their columns, dW = x^T dz over their rows (asr_gemm_hl's
    k_major form reads them transposed out of LDS -- no second orientation is packed).
    One entry per direction when masks are on, else one shared entry."""
    r0 = m._planes('ar%d_0' % si, rows, s.f_in_pad)
    if BW is None:
        ops.pack_hl(a, rows, s.f_in_pad, absmax=amax, r=r0)
        return [r0]
    # both directions' planes in ONE pass over the slab (the source is read once)
    r1 = m._planes('ar%d_1' % si, rows, s.f_in_pad)
    ops.pack_hl(a, rows, s.f_in_pad, mask=BW[0], mask_period=n_pad, absmax=amax, r=r0,
                mask2=BW[1], r2=r1)
    return [r0, r1]


def _gate_gemm_hl(m, s, si, pa, zx, rows):
    """zx = (a (.) B_W) @ W + b from packed planes (both directions in one GEMM without
    masks, one GEMM per direction with them)."""
    Hp = s.Hp
    _await_weights(m, si)
    Wt = m._planes('Wt%d' % si, 8 * Hp, s.f_in_pad)
    bias = m._view(s.ob, 8 * Hp)
    if len(pa) == 1:
        ops.gemm_hl(pa[0], Wt, zx, rows, 8 * Hp, s.f_in_pad, bias=bias)
        return
    for d in range(2):
        ops.gemm_hl(pa[d], Wt, zx, rows, 4 * Hp, s.f_in_pad, b_row=d * 4 * Hp,
                    c_off=d * 4 * Hp, ldc=8 * Hp, bias=bias[d * 4 * Hp:(d + 1) * 4 * Hp])


# --------------------------------------------------------------------------- per-tile GEMMs
def _gate_gemm(m, a, s, zx, BW, r0, r1, n_pad):
    """zx[r0:r1] = (a[r0:r1] (.) B_W) @ W + b over slab rows [r0, r1) (whole frames): one 8H
    GEMM, or one per direction when each has its own input mask (two Keras layers)."""
    mr, Hp = r1 - r0, s.Hp
    if mr <= 0:
        return
    # with multiplicative integration the bias enters inside the cell (z = alpha Wx Uh
    # + beta1 Uh + beta2 Wx + b), so the projection is the bare product
    bias = m._view(s.ob, 8 * Hp) if (s.mi is None and s.ln is None) else None
    for d in ((None,) if BW is None else range(2)):
        n, c0 = (8 * Hp, 0) if d is None else (4 * Hp, d * 4 * Hp)
        mask = {} if d is None else {'mask_w': BW[d]}
        ops.gate_gemm('fwd', mr, n_pad, s.f_in_pad, n, m.params, s.oW + c0, 8 * Hp, 8 * Hp,
                      x=a, x_off=r0 * s.f_in_pad,
                      bias=None if bias is None else bias[c0:c0 + n],
                      zx=zx, z_off=r0 * 8 * Hp + c0, **mask)


def _gate_gemm_half(m, a, s, zx, BW, r0, r1, n_pad, half, first):
    """One half of the reduction of the projection over slab rows [r0, r1): the input is
    [y_f, y_b] of the BiLSTM stage below, half 0 = its forward direction's columns, 1 = the
    backward direction's.  first: zx = partial + b, else zx += partial."""
    mr, Hp, kh = r1 - r0, s.Hp, s.f_in_pad // 2
    if mr <= 0:
        return
    bias = m._view(s.ob, 8 * Hp) if first else None
    for d in (range(2) if BW is not None else (None,)):
        n, c0 = (8 * Hp, 0) if d is None else (4 * Hp, d * 4 * Hp)
        ops.gemm(a, m.params, zx, mr, n, kh, lda=s.f_in_pad, ldb=8 * Hp, ldc=8 * Hp,
                 a_off=r0 * s.f_in_pad + half * kh, b_off=s.oW + half * kh * 8 * Hp + c0,
                 c_off=r0 * 8 * Hp + c0, beta=0.0 if first else 1.0,
                 bias=None if bias is None else bias[c0:c0 + n],
                 a_scale=None if d is None else BW[d], a_scale_period=n_pad,
                 a_scale_off=half * kh, a_scale_ld=s.f_in_pad)


def _dx_gemm_dir(m, dz, s, dx, BW, r0, r1, n_pad, zmx, d, beta):
    """Direction d's term of _dx_gemm over slab rows [r0, r1): dx = beta dx + B_W[d] (.)
    (dz_d @ W_d^T)."""
    mr, Hp = r1 - r0, s.Hp
    if mr <= 0:
        return
    ops.gate_gemm('dgrad', mr, n_pad, s.f_in_pad, 4 * Hp, m.params, s.oW + d * 4 * Hp,
                  8 * Hp, 8 * Hp, mask_w=None if BW is None else BW[d], dz=dz,
                  z_off=r0 * 8 * Hp + d * 4 * Hp, dz_absmax=zmx, dx=dx,
                  dx_off=r0 * s.f_in_pad, dx_beta=beta)


def _dx_gemm(m, dz, s, dx, BW, r0, r1, n_pad, zmx):
    """dx[r0:r1] = sum_d B_W[d] (.) (dz_d[r0:r1] @ W_d^T) over slab rows [r0, r1): one 8H GEMM
    without masks, else direction 0's term and direction 1's on top."""
    mr, Hp = r1 - r0, s.Hp
    if mr <= 0:
        return
    if BW is None:
        ops.gate_gemm('dgrad', mr, n_pad, s.f_in_pad, 8 * Hp, m.params, s.oW, 8 * Hp,
                      8 * Hp, dz=dz, z_off=r0 * 8 * Hp, dz_absmax=zmx, dx=dx,
                      dx_off=r0 * s.f_in_pad)
        return
    for d in range(2):
        _dx_gemm_dir(m, dz, s, dx, BW, r0, r1, n_pad, zmx, d, 0.0 if d == 0 else 1.0)


# --------------------------------------------------------------------------- forward
def begin_forward(m, T, n_pad, n_valid, need_grad):
    """What ``Model.forward`` decides per batch for its BiLSTM stages: the overlap of the side
    stream (auto), the frame-range pipeline, the weight planes.  Returns ``fp.pipe``."""
    if m._overlap_mode == 'auto':
        m.overlap = not recurrence_fills_chip(m, n_pad)
    m._pipe_now = pipeline_on(m, n_pad)
    # (the packed-operand GEMMs take whole slabs: no frame-range pipelining with them)
    t_rec = m.out_frames(T)              # frames the recurrent stack sees
    pipe = (m._pipe_now and m._pipe is not None and m.lstm_mode == 0 and t_rec >= 16
            and not m.packed)
    m._pipe_now = m._pipe_now and not m.packed
    if n_valid == 1 and not need_grad:      # one utterance: the tile-free kernel, whole layers
        pipe = False
    if any(stage_packed(m, st) for st in m.stages):
        _pack_weights(m)
    return pipe


def _variant_args(m, s, si, T, n_pad, training, masks):
    """Keyword arguments of the optional cell variants for ops.lstm_seq_fwd (and, with
    the backward extras added later, lstm_seq_bwd): {} for the plain cell."""
    var = {}
    if s.act != 'tanh' and s.ln is None:        # any other activation: the variant kernels
        var['act'] = s.act
    if s.mi is not None and s.ln is None:
        var['mi'] = m._view(s.omi, 32 * s.Hp)
        var['uh'] = m._buf('uh%d' % si, (T, n_pad, 2, 4 * s.Hp))
    if s.zoneout_c > 0 or s.zoneout_h > 0:
        if masks is not None and si in masks and len(masks[si]) == 4:
            kc, kh = masks[si][2], masks[si][3]          # explicit (T, 2, Hp) coefficients
        else:
            def coef(level, name):
                if not (0 < level < 1):
                    return None
                buf = m._buf('%s%d' % (name, si), (T, 2, s.Hp))
                if training:    # keep mask, shared over the batch, fresh every frame
                    ops.dropout_masks(buf, level, 1.0, m.rng_seed,
                                      4 * si + (2 if name == 'zonec' else 3), m._step)
                else:           # test phase: (h - h_prev) * (1 - level) + h_prev
                    buf.fill_(1.0 - level)
                return buf
            kc, kh = coef(s.zoneout_c, 'zonec'), coef(s.zoneout_h, 'zoneh')
        if kc is not None:
            var['zone_c'] = kc
        if kh is not None:
            var['zone_h'] = kh
    return var


def forward(m, s, si, a, rec, fp):
    """The BiLSTM entry of the stage table (core/stages.py): the input projection (whole, or
    what the layer below has not projected already on the pipe stream), the recurrence, and
    the next BiLSTM layer's projection of the frames that are final before its last steps."""
    T, n_pad, Hp = a.shape[0], fp.n_pad, s.Hp   # (a time-strided convolution shortens the slab)
    BW, BU = fp.stage_masks(si)[:2]
    rec['BW'], rec['BU'] = BW, BU
    var = rec['var'] = _variant_args(m, s, si, T, n_pad, fp.training, fp.masks)
    if s.mi is None and s.ln is None:
        zx = m._buf('zx%d_%d' % (fp.nb % 2, Hp), (T, n_pad, 2, 4 * Hp))
    else:       # x@W is needed again by BPTT: one buffer per layer
        zx = m._buf('zxmi%d' % si, (T, n_pad, 2, 4 * Hp))
        rec['zx'] = zx
    fp.nb += 1
    _project_input(m, s, si, a, rec, fp, zx, BW)
    return _recurrence(m, s, si, rec, fp, zx, BU, var)


def _project_input(m, s, si, a, rec, fp, zx, BW):
    """zx = (a (.) B_W) @ W + b: on packed planes, whole, or -- where the layer below projected
    ahead (``fp.pre[si]``: its event, by halves?) -- what is left of it."""
    T, n_pad = a.shape[0], fp.n_pad
    rows = T * n_pad
    S = (m._pipe_split16 * T) // 16
    main = torch.cuda.current_stream(m.device)
    inner_done, halves = fp.pre.pop(si, (None, False))
    if stage_packed(m, s):
        # |y| < 1 behind a BiLSTM stage with a bounded activation; anything else
        # is measured
        prev = m.stages[si - 1] if si > 0 else None
        bound = m._clip_bound(si)
        amax = _const_one(m) if (prev is not None and _y_bounded(prev)) \
            else (bound if bound is not None
                  else ops.absmax(a, m._buf('aamax%d' % si, (1,))))
        rec['pa'] = _pack_input(m, si, s, a, BW, rows, n_pad, amax)
        _gate_gemm_hl(m, s, si, rec['pa'], zx, rows)
    elif inner_done is None:
        _gate_gemm(m, a, s, zx, BW, 0, rows, n_pad)
    elif halves:
        # frames [T-S, S) were projected while the previous layer ran, and of the
        # others the half of the reduction that was final by then (below): what is
        # left on the critical path is the other half of those frames
        main.wait_event(inner_done)
        # (r6) the two row ranges are independent and each is two launch-bound GEMMs
        # of ~25 us: one range on the pipe stream (idle by now), the other here
        half = functools.partial(_gate_gemm_half, m, a, s, zx, BW)
        _tail_fork(m, lambda: half(S * n_pad, rows, n_pad, 0, False),
                   lambda: half(0, (T - S) * n_pad, n_pad, 1, False))
    else:       # frames [T-S, S) were projected while the previous layer ran
        _gate_gemm(m, a, s, zx, BW, 0, (T - S) * n_pad, n_pad)
        _gate_gemm(m, a, s, zx, BW, S * n_pad, rows, n_pad)
        main.wait_event(inner_done)


def _recurrence(m, s, si, rec, fp, zx, BU, var):
    """y of the stage: the layer-norm cell, the recurrence in two launches with the next
    layer's projection beside the second, or one launch."""
    T, n_pad, Hp = zx.shape[0], fp.n_pad, s.Hp
    S = (m._pipe_split16 * T) // 16
    # (the single-utterance kernel writes row 0 only: no junk in the padding rows)
    one = fp.n_valid == 1 and not fp.need_grad
    y = m._buf('y%d' % si, (T, n_pad, 2 * Hp), zero=one)
    cell = m._buf('cell%d' % si, (T, n_pad, 2, Hp), zero=one)
    gates = m._buf('gates%d' % si, (T, n_pad, 2, 4 * Hp), zero=one)
    U = m._view(s.oU, 2 * Hp * 4 * Hp)
    nxt = m.stages[si + 1] if si + 1 < len(m.stages) else None
    if s.ln is not None:        # generic row-per-workgroup cell (csrc/lstm_ln.hip)
        uh = m._buf('uh%d' % si, (T, n_pad, 2, 4 * Hp))
        rec['uh'] = uh
        ops.lstm_ln_seq_fwd(zx, U, m._view(s.ocell, 68 * Hp), uh, y, cell, gates, T,
                            n_pad, Hp, has_mi=s.mi is not None, mask_u=BU,
                            zone_c=var.get('zone_c'), zone_h=var.get('zone_h'),
                            act=s.act)
    elif fp.pipe and nxt is not None and is_bilstm(nxt) and not var \
            and nxt.mi is None and nxt.ln is None:
        # after S = 13T/16 steps the frames [T-S, S) of y are final in BOTH
        # directions: the next layer's input projection of those frames runs
        # on the pipe stream while this recurrence finishes its last steps
        # (nothing runs beside the first S steps: the library's choice of geometry;
        # the GEMMs of the next layer run beside the last T - S: sixteen units per
        # workgroup there, i.e. the fewest CUs)
        ops.lstm_seq_fwd(zx, U, y, cell, gates, T, n_pad, Hp, mask_u=BU,
                         mode=m.lstm_mode, steps=(0, S))
        fp.pre[si + 1] = _project_ahead(m, s, si, nxt, y, fp, S)
        rec['ws'] = ops.lstm_seq_fwd(zx, U, y, cell, gates, T, n_pad, Hp, mask_u=BU,
                                     mode=m.lstm_mode, steps=(S, T - S), units=16)
    else:
        rec['ws'] = ops.lstm_seq_fwd(
            zx, U, y, cell, gates, T, n_pad, Hp, mask_u=BU, mode=m.lstm_mode,
            n_valid=fp.n_valid if not fp.need_grad else 0, **var)
    rec.update(y=y, cell=cell, gates=gates)
    return y


def _project_ahead(m, s, si, nxt, y, fp, S):
    """On the pipe stream, behind the first S steps of stage si's recurrence: the next BiLSTM
    stage's projection of what is final in y by then.  Returns what that stage finds in
    ``fp.pre``: (the event behind these GEMMs, whether they went by halves)."""
    T, n_pad = y.shape[0], fp.n_pad
    rows = T * n_pad
    zx_n = m._buf('zx%d_%d' % (fp.nb % 2, nxt.Hp), (T, n_pad, 2, 4 * nxt.Hp))
    with _handoff(m, m._pipe):
        BWn = fp.stage_masks(si + 1)[0]
        _gate_gemm(m, y, nxt, zx_n, BWn, (T - S) * n_pad, S * n_pad, n_pad)
        # (the next stage's input must be exactly [y_f, y_b] of this one)
        halves = m._pipe_halves and nxt.f_in_pad == 2 * s.Hp
        if halves:
            # x = [y_f, y_b]: after S steps y_f is final on the frames [0, T-S)
            # too and y_b on [S, T) -- their halves of the reduction
            # (+ bias) go ahead as well
            _gate_gemm_half(m, y, nxt, zx_n, BWn, 0, (T - S) * n_pad, n_pad, 0, True)
            _gate_gemm_half(m, y, nxt, zx_n, BWn, S * n_pad, rows, n_pad, 1, True)
        done = _mark(m)
    return done, halves


# --------------------------------------------------------------------------- backward
def begin_backward(m, T, n_pad):
    """The state of one backward pass (``bp``): the all-reduce decision, the side-stream queue
    of deferred weight-gradient work and the split-K of what runs there."""
    # ASR_AR_OVERLAP: auto (default) = per-layer asynchronous all-reduces beside the BPTT of
    # the layers below ONLY while a recurrence leaves CUs free (cfg2: 64 of 256).  Where a
    # recurrence fills the chip with no compact schedule (ASR_BPTT_COMPACT=0) its
    # spin-waiting workgroups must all be resident, and an RCCL kernel that takes CUs first
    # stalls the whole chain: there the gradients are reduced by ONE collective over the flat
    # buffer after BPTT (110.6 MB: 0.6-2.5 ms of a ~40 ms step).  1 = always overlap, 0 = never.  The decision must be the SAME on every
    # rank (mismatched collective sequences hang RCCL): it is taken on the rank-invariant
    # reference shard pad16(ceil(n_global / world)), never on this rank's own n_pad -- the
    # shards of a ragged last batch differ by one utterance and can straddle a multiple of 16.
    # Round 6: the COMPACT backward schedule leaves half of the CUs to the side stream during
    # every BPTT below the top layer, so the same per-layer collectives run there too: layer
    # l + 1's bucket goes out on the communicator's stream once its weight-gradient GEMMs have
    # finished on the side stream, i.e. beside the compact BPTT of layer l - 1 (the top
    # layer's chip-filling BPTT comes first and has no collective beside it); what is left
    # for the end of the step is the bottom layer + Dense + the flag slots.  compact_any is
    # a function of the reference shard as well.
    ar_mode = os.environ.get('ASR_AR_OVERLAP', 'auto')
    n_ref = m._ar_ref_pad if m._ar_ref_pad else n_pad
    compact_any = any(bptt_compact(m, st, n_ref) for st in m.stages)
    reduce_now = (m._dist_active() and ar_mode != '0'
                  and (ar_mode == '1' or not recurrence_fills_chip(m, n_ref)
                       or compact_any))
    m._ar_covered = []
    m._ar_decision = reduce_now
    # the side stream is in use if the recurrences leave CUs free by themselves (cfg2) or
    # are made to (compact BPTT geometry, cfg3)
    # (decided, like the collective schedule, on the RANK-INVARIANT reference shard: every
    # rank then walks the same branches below, whatever its own shard of a ragged batch)
    overlap = m.overlap or compact_any
    m._compact_launches = 0
    # split-K of the weight-gradient GEMMs that run beside a compact BPTT: sized to the CUs
    # that are free there (ASR_SIDE_SLOTS, measurement switch; 0 = as on the whole chip)
    side_slots = int(os.environ.get('ASR_SIDE_SLOTS', '0'))
    split = 'auto'
    split_side = ('auto:%d' % side_slots) if (compact_any and not m.overlap and side_slots) \
        else split
    bp = Pass(T=T, n_pad=n_pad, rows=T * n_pad, n_ref=n_ref, split=split, split_side=split_side,
              overlap=overlap, reduce_now=reduce_now, pending=[],
              skip_grads={},        # stage index -> gradient to add to that stage's OUTPUT
              reduce_async=functools.partial(_reduce_async, m), first=False)
    bp.flush_side = functools.partial(_flush_side, m, bp)
    return bp


def end_backward(m, bp):
    """What is still queued goes to the side stream, and the calling stream waits for it."""
    bp.flush_side()
    if bp.overlap and m._side is not None:
        torch.cuda.current_stream(m.device).wait_stream(m._side)


def _reduce_async(m, lo, hi, after):
    """This slice of the gradients is final once the work on stream ``after`` is done: its
    all-reduce (on the communicator's own stream) runs beside the BPTT of the layers below."""
    from ..parallel import grad_comm
    grad_comm(m.device).allreduce_after(m.grads[lo:hi], after)
    m._ar_covered.append((lo, hi))


def _flush_side(m, bp):
    """Enqueues the deferred weight-gradient work on the side stream (called right AFTER the
    next layer's BPTT kernel has been launched on the main stream)."""
    while bp.pending:
        fn, ready, par, rng = bp.pending.pop(0)
        with _handoff(m, m._side, ready):
            fn('gemm_side')
            m._dz_free[par] = _mark(m)
        if bp.reduce_now and rng is not None:
            bp.reduce_async(rng[0], rng[1], m._side)


def backward(m, s, si, rec, da, bp):
    """The BiLSTM entry of the stage table (core/stages.py): BPTT, the dX GEMMs on the
    critical path, and the weight-gradient GEMMs -- run here, or deferred in bp.pending to
    run on the side stream beside the BPTT of the layer below (bp.flush_side())."""
    g, var = _grad_buffers(m, s, si, rec, bp)
    pipe_b = (getattr(m, '_pipe_now', False) and m._pipe is not None
              and not bp.first and m.lstm_mode == 0 and bp.T >= 16 and not var
              and s.ln is None)
    dx_inner = None
    if pipe_b:
        dx_inner = _bptt_pipelined(m, s, si, rec, da, bp, g)
    elif s.ln is not None:
        _bptt_layer_norm(m, s, rec, da, bp, g, var)
    else:
        _bptt_plain(m, s, si, rec, da, bp, g, var)
    _grad_operands(m, s, si, rec, g)
    dx = _dx(m, s, si, bp, g, dx_inner)
    _place_weight_grads(m, s, si, bp, g)
    return da if dx is None else dx


def _grad_buffers(m, s, si, rec, bp):
    """The record ``g`` of what the stage's gradient GEMMs read (filled in by the phases that
    follow) and the cell variant's BPTT arguments.  g.pgrad: (per-row parameter-gradient
    sums, rows, cols, offset) of the cell form."""
    T, n_pad, Hp = bp.T, bp.n_pad, s.Hp
    # two dz buffers alternate so that the side stream may still read layer
    # l's dz while layer l-1's BPTT writes the other one
    par = m._dz_parity = 1 - m._dz_parity
    dz = m._buf('dz%d' % par, (T, n_pad, 2, 4 * Hp))
    if bp.overlap and m._dz_free[par] is not None:
        torch.cuda.current_stream(m.device).wait_event(m._dz_free[par])
    g = Pass(par=par, dz=dz, gsrc=dz,           # gsrc: the slab the dW / dX GEMMs read
             zmx=m._buf('dzmax%d' % par, (1,)), pdz_r=None, planes_now=False, dx=None,
             a_in=rec['in'], BW=rec['BW'], BU=rec['BU'], y=rec['y'], pa=rec.get('pa'),
             U=m._view(s.oU, 2 * Hp * 4 * Hp), T=T, n_pad=n_pad, rows=bp.rows,
             split=bp.split, split_side=bp.split_side)
    var = dict(rec.get('var') or {})
    if s.ln is not None:
        g.gsrc = m._buf('dwx%d' % par, (T, n_pad, 2, 4 * Hp))
        dpar = m._buf('dcellp%d' % si, (n_pad, 2, 34 * Hp))
        g.pgrad = (dpar, n_pad, 68 * Hp, s.ocell)
    elif s.mi is not None:
        g.gsrc = m._buf('dwx%d' % par, (T, n_pad, 2, 4 * Hp))
        dmi = m._buf('dmi%d' % si, (n_pad // 16, 2, 4, 4 * Hp))
        var.update(wx=rec['zx'], dwx=g.gsrc, dmi=dmi)
        g.pgrad = (dmi, n_pad // 16, 32 * Hp, s.omi)
    else:
        # plain cell: BPTT leaves the bias gradient as per-batch-tile sums of dz
        # (accumulated in registers over the steps), so nothing re-reads the dz
        # slab for it; the tiles are added up on the side stream
        dbp = m._buf('dbpart%d' % si, (n_pad // 16, 2, 4 * Hp))
        g.pgrad = (dbp, n_pad // 16, 8 * Hp, s.ob)
    return g, var


def _bptt(m, s, rec, da, g, dz, **kw):
    """One BPTT launch of the stage (``dz``: the fp32 slab it writes, or None)."""
    return ops.lstm_seq_bwd(da, g.U, rec['cell'], rec['gates'], dz, g.T, g.n_pad, s.Hp,
                            mask_u=g.BU, mode=m.lstm_mode, dz_absmax=g.zmx, **kw)


def _bptt_pipelined(m, s, si, rec, da, bp, g):
    """BPTT in two launches: after S steps the gate gradients of frames [T-S, S) are final
    in both directions, and their dX GEMMs overlap the last steps on the pipe stream.
    Returns the event behind those GEMMs."""
    T, n_pad, rows = g.T, g.n_pad, g.rows
    S = (m._pipe_split16 * T) // 16
    dz, BW, zmx = g.dz, g.BW, g.zmx
    dx = g.dx = m._buf('da_s%d' % si, (T, n_pad, s.f_in_pad))
    _bptt(m, s, rec, da, g, dz, steps=(0, S), db_part=g.pgrad[0])
    ready = _mark(m)
    bp.flush_side()    # previous layer's dW/dU/db now overlap this BPTT
    with _handoff(m, m._pipe, ready):
        _dx_gemm(m, dz, s, dx, BW, (T - S) * n_pad, S * n_pad, n_pad, zmx)
        if m._pipe_halves:
            # the forward direction's BPTT (frames T-1 .. 0) has also finished
            # [S, T), the backward direction's [0, T-S): their terms of dx
            _dx_gemm_dir(m, dz, s, dx, BW, S * n_pad, rows, n_pad, zmx, 0, 0.0)
            _dx_gemm_dir(m, dz, s, dx, BW, 0, (T - S) * n_pad, n_pad, zmx, 1, 0.0)
        dx_inner = _mark(m)
    rec['ws_b'] = _bptt(m, s, rec, da, g, dz, steps=(S, T - S), db_part=g.pgrad[0])
    return dx_inner


def _bptt_layer_norm(m, s, rec, da, bp, g, var):
    """BPTT of the layer-norm cell (csrc/lstm_ln.hip): two gradient slabs, one scale."""
    ops.lstm_ln_seq_bwd(da, rec['zx'], g.U, m._view(s.ocell, 68 * s.Hp), rec['uh'],
                        rec['y'], rec['cell'], rec['gates'], g.dz, g.gsrc, g.pgrad[0], g.T,
                        g.n_pad, s.Hp, has_mi=s.mi is not None, mask_u=g.BU,
                        zone_c=var.get('zone_c'), zone_h=var.get('zone_h'),
                        act=s.act)
    # one pre-scale for the gradient GEMMs: max over both gradient slabs
    ops.absmax(g.dz, g.zmx)
    tmp = ops.absmax(g.gsrc, m._buf('dzmax_t', (1,)))
    torch.maximum(g.zmx, tmp, out=g.zmx)
    bp.flush_side()


def _bptt_plain(m, s, si, rec, da, bp, g, var):
    """BPTT in one launch (any cell variant but layer norm): compact where weight gradients
    wait to run beside it, writing packed planes of dz where its kernel can."""
    if s.mi is None:
        var['db_part'] = g.pgrad[0]
    # compact geometry only while there is work to run beside it (the top
    # layer's BPTT has none: it keeps the whole chip and the shorter step)
    cmp_now = bool(bp.pending) and not m.overlap and bptt_compact(m, s, bp.n_ref)
    m._compact_launches += int(cmp_now)
    # BPTT writes dz as packed planes itself where its kernel can (the plain cell
    # at H = 256 / 512 on the two-dimensional-split kernels): the pack pass over
    # the fp32 slab (2.1 GB per layer at cfg3) disappears.  The planes' scale has
    # to be known before the pass: a per-layer bound kept at ~64 x the measured
    # max|dz| by asr_lstm_dz_guard (hysteresis: identical inputs see identical
    # scales); a layer without a bound yet -- first step, after a fault or new
    # weights -- runs one MEASURING pass first (fp32 slab, discarded).
    plain = not any(var.get(k) is not None
                    for k in ('act', 'zone_c', 'zone_h', 'mi', 'uh'))
    g.planes_now = (m._dz_planes_mode and stage_packed(m, s) and plain
                    and m.lstm_mode == 0
                    and ops.lstm_dz_hl_supported(g.T, g.n_pad, s.Hp, compact=cmp_now))
    if g.planes_now:
        g.pdz_r = m._planes('dzr%d' % g.par, g.rows, 8 * s.Hp)
        bound = m._buf('dzbound%d' % si, (1,))
        key = (m._fault_gen, m._weights_epoch)
        if m._dz_bound_key.get(si) != key:
            bound.zero_()
            _bptt(m, s, rec, da, g, g.dz, compact=cmp_now, **var)
            ops.lstm_dz_guard(g.zmx, bound, False)
            m._dz_bound_key[si] = key
            m._dz_measure_passes += 1
        rec['ws_b'] = _bptt(m, s, rec, da, g, None, compact=cmp_now, dz_planes=g.pdz_r,
                            dz_bound=bound, **var)
        ops.lstm_dz_guard(g.zmx, bound, True)
    else:
        rec['ws_b'] = _bptt(m, s, rec, da, g, g.dz, compact=cmp_now, **var)
    bp.flush_side()    # previous layer's dW/dU/db now overlap this BPTT


def _grad_operands(m, s, si, rec, g):
    """Behind BPTT, on the main stream: the planes of dz where BPTT has not written them, and
    the bound of |y| for its planes."""
    g.hl = stage_packed(m, s)
    if g.hl and not g.planes_now:
        # dz -> (rows, 8H) planes, once: dX reduces over their gate columns, the
        # weight gradients over their rows (k_major); the scale is the BPTT kernel's
        # own max|dz|
        g.pdz_r = m._planes('dzr%d' % g.par, g.rows, 8 * s.Hp)
        ops.pack_hl(g.dz, g.rows, 8 * s.Hp, absmax=g.zmx, r=g.pdz_r)
    # bound of |y| for its planes (dU): 1 behind a bounded activation, else measured
    # (here, on the main stream, before the side stream's packs read it)
    g.ymx = _const_one(m) if (not g.hl or _y_bounded(s)) \
        else ops.absmax(g.y, m._buf('yamax%d' % si, (1,)))


def _dx(m, s, si, bp, g, dx_inner):
    """The gradient with respect to the stage input (None for the first trainable stage): the
    rest of the pipelined form, by halves or by whole frames; from packed planes; or whole."""
    T, n_pad, rows, Hp = g.T, g.n_pad, g.rows, s.Hp
    S = (m._pipe_split16 * T) // 16
    dz, BW, zmx, dx = g.dz, g.BW, g.zmx, g.dx
    on = (m, dz, s, dx, BW)
    main = torch.cuda.current_stream(m.device)
    if dx_inner is not None and m._pipe_halves:
        main.wait_event(dx_inner)
        # (r6: two independent row ranges, one launch-bound GEMM each: two streams)
        _tail_fork(m, lambda: _dx_gemm_dir(*on, 0, (T - S) * n_pad, n_pad, zmx, 0, 1.0),
                   lambda: _dx_gemm_dir(*on, S * n_pad, rows, n_pad, zmx, 1, 1.0))
    elif dx_inner is not None:
        _dx_gemm(m, dz, s, dx, BW, 0, (T - S) * n_pad, n_pad, zmx)
        _dx_gemm(m, dz, s, dx, BW, S * n_pad, rows, n_pad, zmx)
        main.wait_event(dx_inner)
    elif not bp.first and g.hl:
        dx = m._buf('da_s%d' % si, (T, n_pad, s.f_in_pad))
        Wn = m._planes('Wn%d' % si, s.f_in_pad, 8 * Hp)
        if BW is None:
            ops.gemm_hl(g.pdz_r, Wn, dx, rows, s.f_in_pad, 8 * Hp)
        else:       # dx = sum_d B_W[d] (.) (dz_d @ W_d^T)
            for d in range(2):
                ops.gemm_hl(g.pdz_r, Wn, dx, rows, s.f_in_pad, 4 * Hp, a_k=d * 4 * Hp,
                            b_k=d * 4 * Hp, c_scale=BW[d], c_scale_period=n_pad,
                            beta=0.0 if d == 0 else 1.0)
    elif not bp.first:
        dx = m._buf('da_s%d' % si, (T, n_pad, s.f_in_pad))
        _dx_gemm(m, g.gsrc, s, dx, BW, 0, rows, n_pad, zmx)
    return dx


def _grads_U(m, s, g, wsn):
    """dU[d] = (h_prev (.) B_U)^T dz[d]: h_prev is y shifted by one step in the direction's
    processing order (zero at its first step) -- a row offset of y's planes, or of y."""
    Hp, n_pad = s.Hp, g.n_pad
    kk = (g.T - 1) * n_pad
    for d in range(2):
        if kk <= 0:
            m._gview(s.oU + d * Hp * 4 * Hp, Hp * 4 * Hp).zero_()
        elif g.hl:
            # (one pair of buffers per stream: the bottom layer's gradients run on
            # the main stream while the side stream may still read its own pair)
            yu = m._planes('yu%d%s' % (d, '' if wsn == 'gemm_side' else '_m'), g.rows, Hp)
            ops.pack_hl(g.y, g.rows, Hp, ld=2 * Hp, src_off=d * Hp, absmax=g.ymx, r=yu,
                        mask=None if g.BU is None else g.BU[d], mask_period=n_pad)
            ops.gemm_hl(yu, g.pdz_r, m.grads, Hp, 4 * Hp, kk, a_row=0 if d == 0 else n_pad,
                        b_k=d * 4 * Hp, b_row=n_pad if d == 0 else 0, ws_name=wsn, k_major=True,
                        c_off=s.oU + d * Hp * 4 * Hp,
                        split_k=g.split_side if wsn == 'gemm_side' else g.split)
        else:
            ops.gemm(g.y, g.dz, m.grads, Hp, 4 * Hp, kk, trans_a=True, lda=2 * Hp, ldb=8 * Hp,
                     ldc=4 * Hp, a_off=d * Hp + (0 if d == 0 else n_pad * 2 * Hp),
                     b_off=d * 4 * Hp + (n_pad * 8 * Hp if d == 0 else 0),
                     c_off=s.oU + d * Hp * 4 * Hp, split_k=g.split, ws_name=wsn, b_absmax=g.zmx,
                     a_scale=None if g.BU is None else g.BU[d], a_scale_period=n_pad)


def _grads_W(m, s, g, wsn):
    """dW = (x (.) B_W)^T d(x@W), from planes or per tile; the bias (or MI / LN parameter)
    gradients come from BPTT's per-tile partial sums, never from a pass over the dz slab."""
    Hp = s.Hp
    sp = g.split_side if wsn == 'gemm_side' else g.split
    for d in ((None,) if g.BW is None else range(2)):   # (one entry of g.pa without masks)
        n, c0 = (8 * Hp, 0) if d is None else (4 * Hp, d * 4 * Hp)
        if g.hl:
            one = {} if d is None else {'b_k': c0, 'ldc': 8 * Hp}
            ops.gemm_hl(g.pa[d or 0], g.pdz_r, m.grads, s.f_in_pad, n, g.rows, c_off=s.oW + c0,
                        split_k=sp, ws_name=wsn, k_major=True, **one)
        else:
            one = {} if d is None else {'mask_w': g.BW[d], 'z_off': c0}
            ops.gate_gemm('wgrad', g.rows, g.n_pad, s.f_in_pad, n, m.params, s.oW + c0, 8 * Hp,
                          8 * Hp, x=g.a_in, dz=g.gsrc, dz_absmax=g.zmx, dW=m.grads,
                          dw_off=s.oW + c0, split_k=g.split, ws_name=wsn, **one)
    buf, nrow, ncol, goff = g.pgrad
    ops.colsum(buf, nrow, ncol, ncol, m._gview(goff, ncol), ws_name=wsn + '_cs')


def _place_weight_grads(m, s, si, bp, g):
    """Runs the stage's weight-gradient GEMMs here, or queues them for the side stream."""
    gu, gw = functools.partial(_grads_U, m, s, g), functools.partial(_grads_W, m, s, g)

    def both(wsn):
        gu(wsn)
        gw(wsn)
    # (compact schedule: is there a BiLSTM stage below whose BPTT this layer's
    # weight gradients could run beside?  A convolution / Dense / nothing below:
    # chip-filling GEMMs either way -- one stream, as in the serial schedule)
    below = any(is_bilstm(st) for st in m.stages[:si])
    if not bp.overlap or ((bp.first or not below) and not m.overlap):
        # no side stream (a recurrence fills the chip), or the compact schedule's tail, whose
        # GEMMs each fill the chip: one stream.  This layer's gradients are final on the main
        # stream; their all-reduce runs beside the layers below instead of after them all
        both('gemm')
        if bp.reduce_now and not bp.first:
            bp.reduce_async(s.p_lo, s.p_hi, torch.cuda.current_stream(m.device))
    elif bp.first:
        # nothing left to hide behind: share the tail between both streams
        bp.pending.append((gu, _mark(m), g.par, None))
        bp.flush_side()
        gw('gemm')
    else:
        # the side stream starts once the dX GEMMs (critical path) are done,
        # i.e. together with the next layer's BPTT kernel
        bp.pending.append((both, _mark(m), g.par, (s.p_lo, s.p_hi)))
