"""Execution engine behind ``ctc_model()``: runs the stage list on the HIP kernels.

Replaces what Keras 1.2.2 + TensorFlow 1.3.0 do for the reference once
``model.compile`` / ``fit_generator`` / ``evaluate_generator`` are called
(train.py:140-143, 213-217, 223-227; eval.py:76-80): forward, CTC loss, BPTT,
global-norm clip + Adam/SGD, greedy/beam decode and LER.  Everything numeric goes
through the C ABI (asr_study_amd.ops); torch provides device buffers, streams and
the RCCL all-reduce only.

Data layout: activations are time-major slabs (T, n_pad, features) with the batch
rounded up to a multiple of 16 (padding rows stay zero / get zero gradient).  All
parameters live in ONE flat float32 buffer (so the optimiser and the all-reduce are
single launches); LSTM gate axes are stored unit-major/gate-minor (see
include/asr_hip.h) and hidden sizes are rounded up to a multiple of 4 with zero
weights (eyben's 78/27-unit layers).  get_weights()/set_weights() speak the
reference's Keras layout: per Bidirectional layer [W (in,4H), U (H,4H), b (4H)] for
the forward then the backward copy, gate blocks i,f,c,o; Dense [W, b].  Where each weight
lies in the flat buffer, and how it is padded, is the parameter table of core/params.py.

What a stage kind reads from its spec, computes and differentiates is its entry of the stage-kind
table of core/stages.py; ``_layout`` / ``forward`` / ``backward`` here are the prologues, one loop
over the stages and the epilogues.  The two-direction LSTM stage, whose launches are scheduled
over three streams, is core/bilstm.py: its handlers, its switches (``bilstm.switches``) and what
it decides per pass (``bilstm.begin_forward`` / ``begin_backward`` / ``end_backward``).
"""
import math
import os
import time

import numpy as np
import torch

from .. import ops
from . import bilstm
from . import optimizers as _opt
from . import params as P
from .params import _pad4
from .stages import KINDS, Pass, _nd, time_factor


# where a Model lives when the factory is given no ``device`` (host-only tests build on 'cpu':
# weights I/O works there, every compute call still needs the HIP library and a GPU)
DEFAULT_DEVICE = os.environ.get('ASR_DEVICE', 'cuda:0')


class Stage(object):
    pass


class _Feeder(object):
    """Bounded producer queue over a batch generator (Keras' GeneratorEnqueuer with one
    worker THREAD, train.py:215-216).  The generator's exception, if any, is re-raised in
    the consumer."""

    def __init__(self, generator, max_q_size=10, device=None):
        import queue
        import threading
        self._q = queue.Queue(maxsize=max(1, int(max_q_size)))
        self._stop = threading.Event()
        self._gen = generator

        def work():
            try:
                if device is not None and device.type == 'cuda':
                    torch.cuda.set_device(device)    # the current device is per thread
                while not self._stop.is_set():
                    item = next(self._gen)
                    while not self._stop.is_set():
                        try:
                            self._q.put((item, None), timeout=0.1)
                            break
                        except queue.Full:
                            continue
            except BaseException as e:           # StopIteration included: surfaces in get()
                self._q.put((None, e))
        self._t = threading.Thread(target=work, name='asr-batch-feeder', daemon=True)
        self._t.start()

    def get(self):
        item, err = self._q.get()
        if err is not None:
            raise err
        return item

    def close(self):
        self._stop.set()
        try:
            while True:
                self._q.get_nowait()
        except Exception:
            pass
        self._t.join(timeout=5.0)


class Model(object):
    """The object ``ctc_model(inputs, output)`` returns (core/models.py:31-52)."""

    def __init__(self, spec, num_features, device=None, seed=0, lstm_mode=0):
        self.device = torch.device(device or DEFAULT_DEVICE)
        self.spec = spec
        self.num_features = int(num_features)
        self.lstm_mode = int(os.environ.get('ASR_LSTM_MODE', lstm_mode))   # 1 = stepwise kernels
        # A persistent recurrent kernel that abandoned a bounded spin demotes the model to the
        # stepwise kernels only for a while: after `_retry_gap` clean optimisation steps the
        # persistent kernels are tried again (the gap doubles with every further fallback).
        # A model that was ASKED for mode 1 stays there.
        self._mode_pinned = self.lstm_mode == 1
        self._retry_at = None
        self._retry_gap = int(os.environ.get('ASR_LSTM_RETRY_STEPS', '64'))
        self.fallbacks = 0              # timeouts survived (bench.py asserts 0)
        self.vetoed_steps = 0           # optimisation steps skipped because of them
        self._fault_gen = 0
        self.optimizer = None
        self.metrics_names = ['loss', 'ctc_loss', 'decoder_loss', 'decoder_ler']
        self.decoder = dict(is_greedy=True)
        self.stop_training = False
        self._bufs = {}
        self._step = 0
        self._enqueued = self._checked = 0   # train_on_batch steps enqueued / whose flags were read
        self._ar_ref_pad = 0            # rank-invariant reference shard (set per batch)
        self._ar_covered = []
        # the side and pipe streams, the packed-operand planes and the switches of the BiLSTM
        # schedule (overlap, pipeline, compact BPTT, planes written by BPTT)
        bilstm.switches(self)
        # training-time noise comes from the library's counter-based streams (ops.dropout_masks
        # ...: Philox-4x32-10 keyed by this seed; stream id = 4 * stage index + kind, step =
        # the optimisation step), so a step's masks are a pure function of (seed, stage, step)
        # ... and, data parallel, of the rank: every rank draws its OWN noise for its shard
        # (the rank is mixed in when the key is used: the process group may be created later)
        self._rng_base = (int(seed) + 12345) & (2 ** 64 - 1)
        self._layout(seed)

    @property
    def rng_seed(self):
        import torch.distributed as dist
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        return (self._rng_base + rank * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)

    # ------------------------------------------------------------------ params
    def _layout(self, seed):
        """Reads the stage list: per stage its attributes and, for a trainable kind, its rows of
        the parameter table (core/params.py), which allocates its blocks of the flat buffers --
        both by the kind's ``build`` of the stage-kind table (core/stages.py).  Then the passes
        that look at more than one stage."""
        self.stages = []
        # the input features are padded to a multiple of 4 columns (zero column(s), zero
        # weight rows) so that the first layer's GEMMs qualify for the 16-byte fast path
        f_real, f_pad = self.num_features, _pad4(self.num_features)
        self.f_in_pad0 = f_pad
        alloc = self._alloc = P.Alloc()     # (the builders of core/stages.py allocate from it)
        trainable_below = False
        for st in self.spec:
            s = Stage()
            s.kind = st['type']
            if s.kind not in KINDS:
                raise ValueError(s.kind)
            s.p_lo = alloc.params           # this stage's slice of the flat param / grad buffers
            s.f_in, s.f_in_pad = f_real, f_pad
            s.tensors = []                  # (core/params.py; stays empty without weights)
            s.first = not trainable_below   # no weights below: nothing there needs a gradient
            f_real, f_pad = KINDS[s.kind].build(self, s, st, (f_real, f_pad))
            trainable_below = trainable_below or bool(s.tensors)
            s.f_out, s.f_out_pad = f_real, f_pad
            s.p_hi = alloc.params
            self.stages.append(s)
        del self._alloc
        self.packed = bilstm.packed_on(self)
        self.num_classes = f_real
        kinds = [KINDS[st.kind] for st in self.stages]
        # (slots 2, 3 of the timeout flags: the SimpleRNN workspaces', ops.collect_timeout_flags)
        self._has_rnn = any(k.extra_timeout_flags for k in kinds)
        # forward needs seq_len: the attention keys and the depthwise convolution's frames
        self._has_mha = any(k.attention for k in kinds)
        self._needs_lens = any(k.needs_lens for k in kinds)
        # ... and in_len, the lengths on the INPUT time axis: a SpecAugment stage's utterances
        self._has_specaug = any(k.needs_in_len for k in kinds)
        self._bn = [(i, st) for i, st in enumerate(self.stages) if st.kind == 'bn']
        self._seqbn = [(i, st) for i, st in enumerate(self.stages)
                       if st.kind == 'bigru' and st.bn]
        skips = set(st.skip for st in self.stages if st.kind == 'merge')
        for i, st in self._bn:
            # BN followed by a clipped ReLU: one pass (asr_bn_* clip), the Activation stage is
            # then a pass-through (unless a residual branch reads the BN output itself)
            nxt = self.stages[i + 1] if i + 1 < len(self.stages) else None
            if (nxt is not None and nxt.kind == 'act' and isinstance(nxt.act, (tuple, list))
                    and nxt.act[0] == 'clipped_relu' and float(nxt.act[1]) > 0
                    and i not in skips and os.environ.get('ASR_BN_FUSE', '1') != '0'):
                st.clip = float(nxt.act[1])
                nxt.fused = True
        for i, st in enumerate(self.stages):
            # a depthwise convolution straight in front of a per-column BatchNormalization: the
            # batch mean takes its bias out again, so the bias gradient (the sum of the BN input
            # gradient over exactly the frames BN averages) is identically 0.  A column sum
            # would leave rounding noise there, which Adam would normalise into steps of +-lr:
            # it is never produced and keeps the zero the gradient buffer is created with (as
            # the key bias of the mha stage).
            if st.kind == 'dwconv':
                nxt = self.stages[i + 1] if i + 1 < len(self.stages) else None
                st.bias_dead = (nxt is not None and nxt.kind == 'bn' and not nxt.grouped
                                and i not in skips)
        # the time strides in stage order: the strided convolutions and the TimeReduction stages
        # (K33).  _axis_of[i]: how many of them lie in front of stage i, i.e. which time axis its
        # INPUT is on (0: the model input's); read only when the model has a TimeReduction
        strided = [(i, st.st if st.kind == 'conv' else time_factor(st))
                   for i, st in enumerate(self.stages)
                   if (st.kind == 'conv' and st.st > 1) or time_factor(st)]
        self.time_strides = [k for _, k in strided]
        self._treduce = any(time_factor(st) for st in self.stages)
        self._axis_of = [sum(1 for j, _ in strided if j < i) for i in range(len(self.stages))]
        self._convs = {}
        self.n_params = off = alloc.params
        self.params = torch.zeros(off, dtype=torch.float32, device=self.device)
        # gradients + 4 trailing floats: [0:2] carry this rank's recurrent-kernel timeout flags
        # through the gradient all-reduce (sum > 0 on every rank if ANY rank timed out), so a
        # veto of the update is collective and costs no collective of its own; behind them the
        # BatchNormalization stages' moments blocks (none without such a stage)
        self._gbuf = torch.zeros(off + alloc.moments, dtype=torch.float32, device=self.device)
        self.grads = self._gbuf[:off]
        self.bn_running = torch.zeros(max(alloc.running, 4), dtype=torch.float32,
                                      device=self.device)
        self._segments = P.segments(self.stages)
        self._segs_dev, self._nseg = ops.make_segments(self._segments, self.device)
        self._norm = torch.zeros(2, dtype=torch.float64, device=self.device)
        # initial values: all from ONE stream, in stage order and Keras order within a stage
        rs = np.random.RandomState(seed)
        self.set_weights([P.draw(t, rs) for s in self.stages for t in s.tensors])

    def _real_rows(self, s):
        """Map of the padded input-feature rows of a stage to its real rows: the output columns
        of the last stage before it that has an input projection (BatchNormalization and
        LayerNormalization keep the columns they are given), whose two directions are padded
        apart when it concatenates them."""
        prev = None
        for st in self.stages:
            if st is s:
                break
            if hasattr(st, 'oW'):
                prev = st
            elif time_factor(st):       # (a stacked frame has no pad columns inside)
                prev = None
        if (prev is not None and hasattr(prev, 'Hp') and prev.Hp != prev.H
                and getattr(prev, 'merge', 'concat') == 'concat'
                and _nd(prev) == 2):
            idx = np.concatenate([np.arange(prev.H), prev.Hp + np.arange(prev.H)])
        else:
            idx = np.arange(s.f_in)
        return idx

    def set_weights(self, weights):
        """weights: flat list in the reference's Keras order (see module doc)."""
        bufs = {'params': self.params.detach().cpu().numpy().copy(),
                'running': self.bn_running.detach().cpu().numpy().copy()}
        tensors = [t for s in self.stages for t in s.tensors]
        names = [n for _, ns in P.keras_names(self.stages) for n in ns]
        for t in tensors:                   # (pads: 0, running variances 1)
            P.clear(t, bufs[t.buf])
        it = iter(weights)
        for t, name in zip(tensors, names):
            P.write(t, bufs[t.buf], next(it), name)
        self.params.copy_(torch.from_numpy(bufs['params']))
        self.bn_running.copy_(torch.from_numpy(bufs['running']))
        self._weights_epoch += 1        # (bounds measured under the old weights are dropped)

    def _bn_cols(self, s):
        """Physical channels of a BatchNormalization stage that carry real features."""
        return np.arange(s.C) if s.grouped else self._real_rows(s)

    def _bn_views(self, s, n):
        """(running mean, running variance, moments block) of the n channels of a
        BatchNormalization stage (n = C) or a GRU(batch_norm=True) stage (n = 6 Hp)."""
        o = self.n_params + s.omom
        return (self.bn_running[s.orun:s.orun + n],
                self.bn_running[s.orun + _pad4(n):s.orun + _pad4(n) + n],
                self._gbuf[o:o + ops.bn_moments_len(n)])

    def _unpack(self, flat, running=None):
        """flat (params / grads / optimiser slots) -> Keras-order arrays.  running: the host copy
        of bn_running (get_weights), 'zeros' (get_gradients: the running moments have none) or
        None (optimiser slots: trainable weights only)."""
        out = []
        for s in self.stages:
            for t in s.tensors:
                if t.buf == 'params':
                    out.append(P.read(t, flat))
                elif isinstance(running, str):
                    out.append(np.zeros(t.shape, np.float32))
                elif running is not None:
                    out.append(P.read(t, running))
        return out

    def get_weights(self):
        return self._unpack(self.params.detach().cpu().numpy(),
                            running=self.bn_running.detach().cpu().numpy())

    def get_gradients(self):
        """Last computed gradients (before clipping, without the l2 term), in the
        same order/layout as get_weights()."""
        return self._unpack(self.grads.detach().cpu().numpy(), running='zeros')

    def count_params(self):
        return int(sum(w.size for w in self.get_weights()))

    # ------------------------------------------------------------------ compile
    def compile(self, loss=None, optimizer=None, metrics=None, loss_weights=None):
        """Keras signature (train.py:140-143).  ``loss``/``metrics`` are accepted for
        surface compatibility: the objective is always 1*mean(ctc) + 0*decoder + l2."""
        if isinstance(optimizer, str):
            optimizer = _opt.get(optimizer)
        self.optimizer = optimizer
        if optimizer is not None:
            optimizer.bind(self)

    # ------------------------------------------------------------------ buffers
    def _buf(self, name, shape, zero=False):
        """Cached float32 buffer.  zero=True fills it with zeros WHEN IT IS CREATED, on the
        current stream -- only for buffers whose first user runs on that same stream (a fill
        kernel is not ordered against the side / pipe streams, which wait on events only)."""
        key = (name, tuple(int(x) for x in shape))
        b = self._bufs.get(key)
        if b is None:
            # drop stale shapes of the same name to bound memory
            for k in [k for k in self._bufs if k[0] == name]:
                del self._bufs[k]
            b = (torch.zeros if zero else torch.empty)(key[1], dtype=torch.float32,
                                                       device=self.device)
            self._bufs[key] = b
        return b

    def _view(self, off, n):
        return self.params[off:off + n]

    def _gview(self, off, n):
        return self.grads[off:off + n]

    def _planes(self, name, rows, k):
        """Cached ops.HlPlanes buffer (rows, k) under `name` (stale shapes dropped)."""
        key = (name, int(rows), int(k))
        b = self._hl.get(key)
        if b is None:
            for kk in [kk for kk in self._hl if kk[0] == name]:
                del self._hl[kk]
            b = ops.HlPlanes(rows, k, self.device)
            self._hl[key] = b
        return b

    # (the BiLSTM predicates of core/bilstm.py that tests and stages ask the model for)
    _is_bilstm = staticmethod(bilstm.is_bilstm)
    _stage_packed = bilstm.stage_packed
    _recurrence_fills_chip = bilstm.recurrence_fills_chip

    # ------------------------------------------------------------------ forward
    def forward(self, x, training=False, masks=None, need_grad=True, n_valid=0, n_real=None,
                bn_weight=None, seq_len=None, in_len=None):
        """x: (T, n_pad, F) float32 CUDA slab -> logits (T, n_pad, C).
        need_grad=False (evaluation / prediction) skips what only BPTT would read; n_valid=1
        with it (one utterance, predict.py) selects the tile-free recurrent kernel.
        n_real: the real samples of the slab (rows n < n_real of every frame; default n_valid, else
        n_pad), over which BatchNormalization takes its training statistics; bn_weight: samples
        this rank contributes to the running moments (default n_real; 0 = a zero-weight dummy).
        seq_len: device int32 lengths of the real samples on the recurrent stack's time axis (what
        CTC gets): the valid frames of a GRU(batch_norm=True) stage's training statistics and the
        visible keys of a MultiHeadAttention stage and the frames a DepthwiseConvolution1D stage
        reads, in training and inference (None: every frame).
        in_len: device int32 lengths of the real samples on the INPUT time axis (x's frames): the
        utterances a SpecAugment stage warps and masks within, in training (None: every frame).
        A model with a TimeReduction stage has more than one time axis behind its front-end, and
        ceil(len / k) cannot be inverted: it takes in_len in every phase, derives the lengths of
        every axis from it on the device (_axis_lens) and hands each stage those of its own axis
        as fp.seq_len; without in_len (and seq_len) every frame is valid.

        masks: optional explicit variational-dropout masks (parity tests):
        {stage_index: (BW (2, n_pad, f_in_pad), BU (2, n_pad, Hp))}.
        """
        T, n_pad, F = x.shape
        assert F in (self.num_features, self.f_in_pad0) and n_pad % 16 == 0
        if F != self.f_in_pad0:
            # (T, n_pad, F) -> zero-padded (T, n_pad, pad4(F)); the pad columns of the
            # buffer are written once (zeros) and never touched again
            key = ('xpad', (T, n_pad, self.f_in_pad0))
            fresh = key not in self._bufs
            xp = self._buf('xpad', (T, n_pad, self.f_in_pad0))
            if fresh:
                xp.zero_()
            xp[:, :, :F].copy_(x)
            x = xp
        a = x
        self._acts = []
        drawn = [None]
        pipe = bilstm.begin_forward(self, T, n_pad, n_valid, need_grad)
        n_real = int(n_real or n_valid or n_pad)
        bn_weight = n_real if bn_weight is None else int(bn_weight)

        def stage_masks(i):
            st = self.stages[i]
            if masks is not None and i in masks:
                return masks[i][:2]
            if training and (st.dropout_W > 0 or st.dropout_U > 0):
                if drawn[0] is None:
                    drawn[0] = self._draw_all_masks(n_pad)
                return drawn[0][i]
            return None, None
        fp = Pass(training=training, masks=masks, need_grad=need_grad, n_valid=n_valid,
                  n_real=n_real, bn_weight=bn_weight, seq_len=seq_len, in_len=in_len,
                  n_pad=n_pad, pipe=pipe, pre={}, nb=0, stage_masks=stage_masks)
        axes = self._axis_lens(in_len, seq_len) if self._treduce else None
        for si, s in enumerate(self.stages):
            rec = {'in': a}
            if axes is not None:        # (a model without the stage: one seq_len, as ever)
                fp.seq_len = axes[self._axis_of[si]]
            a = rec['out'] = KINDS[s.kind].forward(self, s, si, a, rec, fp)
            self._acts.append(rec)
        return a

    def _axis_lens(self, in_len, seq_len):
        """The device lengths on every time axis of a model with a TimeReduction stage: [input
        axis, behind the first stride, ...], each ceil(previous / stride), computed on the device
        from the input lengths (no host copy).  All None when no lengths are given."""
        n = len(self.time_strides) + 1
        if in_len is None:
            if seq_len is not None:
                raise ValueError(
                    'a model with a TimeReduction stage needs in_len, the lengths on the INPUT '
                    'time axis: the stages in front of the reduction run on a longer axis than '
                    'seq_len, and ceil(len / k) cannot be inverted')
            return [None] * n
        axes = [in_len.to(torch.int32)]
        for st in self.time_strides:
            axes.append(torch.div(axes[-1] + (st - 1), st, rounding_mode='floor').to(torch.int32))
        return axes

    def _input_lens(self, lens):
        """in_len of forward() for a model with a TimeReduction stage (None for any other): the
        host or device input lengths as a device int32 tensor."""
        if not self._treduce:
            return None
        if torch.is_tensor(lens):
            return lens.to(self.device, dtype=torch.int32)
        return torch.as_tensor(np.asarray(lens, np.int32).reshape(-1)).to(self.device)

    def _bn_update(self):
        """Running-moment update of every BatchNormalization stage, once per optimisation step,
        behind the optimiser: skipped on the device with the update (the same flag words as the
        optimiser's guard), so a vetoed step leaves the statistics alone; no host sync."""
        if not (self._bn or self._seqbn) or not getattr(self, '_acts', None):
            return
        flags = self.veto_flags()
        # GRU(batch_norm=True): one channel per column of zx
        for si, s, n, momentum in ([(si, s, 6 * s.Hp, s.bn_momentum) for si, s in self._seqbn] +
                                   [(si, s, s.C, s.momentum) for si, s in self._bn]):
            rec = self._acts[si]
            if 'stats' not in rec:
                continue
            rm, rv, mom = self._bn_views(s, n)
            ops.bn_update_running(rm, rv, mom, n, momentum, shift=rec['shift'], flags=flags)

    def _clip_bound(self, si):
        """1-element device tensor >= max|input of stage si| when that input is a clipped-ReLU
        convolution's output (0 <= y <= clip), seen through reshapes; else None (measure)."""
        j = si - 1
        while j >= 0 and self.stages[j].kind == 'reshape':
            j -= 1
        if j < 0 or self.stages[j].kind != 'conv' or not self.stages[j].clip > 0:
            return None
        key = ('clipbound', float(self.stages[j].clip))
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = torch.full((1,), float(self.stages[j].clip),
                                              dtype=torch.float32, device=self.device)
        return t

    def out_frames(self, T):
        """Frames of the logits for T input frames (ceil(T / st) per time-strided layer)."""
        for st in self.time_strides:
            T = -(-int(T) // st)
        return int(T)

    def out_lengths(self, lens):
        """inputs_length -> lengths on the logits' time axis (host array or device tensor)."""
        for st in self.time_strides:
            if torch.is_tensor(lens):
                lens = torch.div(lens + (st - 1), st, rounding_mode='floor').to(lens.dtype)
            else:
                lens = -(-np.asarray(lens) // st)
        return lens

    def _draw_all_masks(self, n_pad):
        """Variational-dropout masks of every BiLSTM stage for one batch (core/models.py:265-266:
        one mask per batch and direction, constant over time, inverted scaling), from the
        library's counter-based streams: {stage: (B_W (2, n_pad, in), B_U (2, n_pad, H))} with
        stream id 4 * stage (B_W) / 4 * stage + 1 (B_U) at step self._step.  An RHN stage has one
        B_U per level: (2, L, n_pad, H), all from that one stream."""
        out = {}
        for si, s in enumerate(self.stages):
            mask_shape = KINDS[s.kind].mask_shape
            if mask_shape is None or not (s.dropout_W > 0 or s.dropout_U > 0):
                continue
            BW = self._buf('BW%d' % si, (2, n_pad, s.f_in_pad))
            BU = self._buf('BU%d' % si, mask_shape(s, n_pad))
            for k, (t, p) in enumerate(((BW, s.dropout_W), (BU, s.dropout_U))):
                if p > 0:
                    ops.dropout_masks(t, p, 1.0 / (1.0 - p), self.rng_seed, 4 * si + k, self._step)
                else:
                    t.fill_(1.0)
            out[si] = (BW, BU)
        return out

    # ------------------------------------------------------------------ backward
    def backward(self, dlogits):
        """dlogits (T, n_pad, C) -> fills self.grads (raw, no l2, no clip)."""
        T, n_pad, _ = dlogits.shape
        da = dlogits
        # (the all-reduce decision and the side-stream queue of the weight gradients)
        bp = bilstm.begin_backward(self, T, n_pad)
        for si in range(len(self.stages) - 1, -1, -1):
            s = self.stages[si]
            if si in bp.skip_grads:         # the residual branch rejoins here
                g = bp.skip_grads.pop(si)
                da = ops.axpby(1.0, da, 1.0, g, self._buf('dskip%d' % si, da.shape))
            bp.first = s.first
            dx = KINDS[s.kind].backward(self, s, si, self._acts[si], da, bp)
            da = dx if dx is not None else da
        bilstm.end_backward(self, bp)
        return da

    # ------------------------------------------------------------------ batches
    def _key_lens(self, lens, T):
        """lens: host lengths on the logits' time axis of a batch of T input frames.  A model
        with a MultiHeadAttention or DepthwiseConvolution1D stage refuses lengths outside
        1 .. out_frames(T) here, while they are on the host (the kernels would clamp them
        silently)."""
        lens = np.asarray(lens).reshape(-1)
        if self._needs_lens and lens.size and (lens.min() < 1 or lens.max() > self.out_frames(T)):
            raise ValueError('inputs_length: every utterance needs 1 .. %d frames on the '
                             'attention / convolution layers\' time axis (%d input frames), '
                             'got %d .. %d'
                             % (self.out_frames(T), T, lens.min(), lens.max()))
        return lens

    def _prep_labels(self, labels, seq_len, T):
        N = len(labels)
        lmax = max([len(l) for l in labels] + [1])
        lab = np.zeros((N, lmax), np.int32)
        seq_len = self.out_lengths(np.asarray(seq_len).reshape(-1))   # on the logits' time axis
        seq_len = self._key_lens(seq_len, T)
        for n, l in enumerate(labels):
            l = np.asarray(l, np.int64).reshape(-1)
            need = len(l) + int(np.sum(l[1:] == l[:-1])) if len(l) else 0
            if need > int(seq_len[n]):
                raise ValueError('Not enough time for target transition sequence '
                                 '(required: %d, available: %d) in sample %d'
                                 % (need, int(seq_len[n]), n))
            lab[n, :len(l)] = l
        dev = self.device
        return (torch.from_numpy(lab).to(dev),
                torch.tensor([len(l) for l in labels], dtype=torch.int32, device=dev),
                torch.as_tensor(np.asarray(seq_len, np.int32)).to(dev))

    def to_slab(self, x_ntf):
        """(N, T, F) batch-major host/GPU array (the reference's layout) -> (T, n_pad, F)."""
        t = torch.as_tensor(np.asarray(x_ntf, np.float32)) if not torch.is_tensor(x_ntf) else x_ntf
        t = t.to(self.device, dtype=torch.float32)
        N, T, F = t.shape
        n_pad = ops.pad16(N)
        slab = torch.zeros((T, n_pad, F), dtype=torch.float32, device=self.device)
        slab[:, :N] = t.permute(1, 0, 2)
        return slab

    def _unpack_inputs(self, inputs):
        x, labels, lens = inputs[0], inputs[1], inputs[2]
        if hasattr(labels, 'tocsr'):            # scipy.sparse (the reference's batches)
            csr = labels.tocsr()
            labels = [csr.data[csr.indptr[i]:csr.indptr[i + 1]] if i < csr.shape[0] else []
                      for i in range(len(np.asarray(lens).reshape(-1)))]
        lens = np.asarray(lens).reshape(-1)
        if torch.is_tensor(x) and x.dim() == 3 and x.shape[1] % 16 == 0 and \
                getattr(x, '_asr_time_major', False):
            slab = x
        elif isinstance(x, tuple) and x[0] == 'slab':
            slab = x[1]
        else:
            slab = self.to_slab(x)
        return slab, [np.asarray(l).reshape(-1) for l in labels], lens

    def loss_and_grads(self, slab, labels, seq_len, training=True, masks=None, n_global=None,
                       n_ref=None):
        """One forward + CTC + backward.  Returns per-sample CTC loss (device) and
        logits; self.grads holds d(mean ctc)/d params."""
        lab, lab_len, sl = self._prep_labels(labels, seq_len, slab.shape[0])
        in_len = self._input_lens(seq_len)
        if self._has_specaug and training:
            # the batch's input lengths, for the SpecAugment stage (a copy like the three above)
            in_len = torch.as_tensor(np.asarray(seq_len, np.int32).reshape(-1)).to(self.device)
        return self.loss_and_grads_device(slab, lab, lab_len, sl, len(labels), training, masks,
                                          n_global, n_ref, in_len=in_len)

    def loss_and_grads_device(self, slab, lab, lab_len, sl, N, training=True, masks=None,
                              n_global=None, n_ref=None, in_len=None):
        """Same with labels (N, l_max) / label_len / seq_len already on the device.
        in_len: device int32 input lengths for a SpecAugment stage (None: every frame is valid).
        n_global: samples of the GLOBAL batch (gradient scale 1/n_global; 0 = this rank holds a
        zero-weight dummy); n_ref: the global batch size again, for decisions every rank must
        take alike (it survives n_global = 0)."""
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        ng = int(n_ref or n_global or N * world)
        self._ar_ref_pad = ops.pad16((ng + world - 1) // world)
        logits = self.forward(slab, training=training, masks=masks, n_real=N,
                              bn_weight=0 if n_global == 0 else N, seq_len=sl, in_len=in_len)
        dlog = self._buf('dlogits', logits.shape)
        # n_global = 0: a zero-weight dummy shard (parallel.ShardedBatch.n_local == 0)
        ctc = ops.ctc_loss_grad(logits, lab, lab_len, sl, N, grad=dlog,
                                grad_scale=0.0 if n_global == 0 else 1.0 / float(n_global or N))
        self.backward(dlog)
        return ctc, logits, sl

    def train_step_device(self, slab, lab, lab_len, sl, N, world=1):
        """A full optimisation step with every input resident in HBM and no host
        synchronisation: forward, CTC, BPTT, (RCCL all-reduce), clip + update, greedy
        decode for the LER metric.  Returns device tensors (ctc, decoded, lengths)."""
        self._maybe_retry_persistent()
        in_len = sl.to(torch.int32) if (self._has_specaug or self._treduce) else None   # (input frames)
        sl = self.out_lengths(sl)
        ctc, logits, sl = self.loss_and_grads_device(slab, lab, lab_len, sl, N, training=True,
                                                     n_global=N * world, in_len=in_len)
        self._allreduce()
        self._step += 1
        self.optimizer.step(self)
        self._bn_update()
        dec, dlen = ops.ctc_greedy(logits, sl, N)
        return ctc, dec, dlen

    def _dist_active(self):
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and (
            dist.get_world_size() > 1 or os.environ.get('ASR_FORCE_ALLREDUCE') == '1')

    # ------------------------------------------------------------------ timeouts
    def _collect_flags(self):
        """This rank's recurrent-kernel timeout flags -> the two flag slots behind the
        gradients (as 0.0 / 1.0), enqueued on the current stream."""
        ops.collect_timeout_flags(self._gbuf[self.n_params:], self.device)

    def veto_flags(self):
        """What the optimiser's guard looks at: data parallel, the all-reduced flag slots
        (non-zero on EVERY rank when any rank timed out, so all ranks skip the same update);
        single process, None = the workspaces' own sticky words."""
        # (slots 2, 3: the SimpleRNN workspaces' flags, ops.collect_timeout_flags)
        n = 4 if getattr(self, '_has_rnn', False) else 2
        return self._gbuf[self.n_params:self.n_params + n] if self._dist_active() else None

    def _flag_snapshot(self):
        v = self.veto_flags()
        return ops.lstm_timeout_flags(self.device) if v is None else v.clone()

    def _maybe_retry_persistent(self):
        """After a fallback the stepwise kernels run for `_retry_gap` clean steps, then the
        persistent ones get another chance (every rank takes the same decision: the detection
        is collective)."""
        if (self.lstm_mode == 1 and not self._mode_pinned and self._retry_at is not None
                and self._step >= self._retry_at):
            self.lstm_mode = 0
            self._retry_at = None

    def _handle_timeout(self, flags, gen, train=True):
        """flags: a step's snapshot of the (collective) timeout flags, gen: self._fault_gen
        when that step was enqueued.  Returns True when the step was vetoed (its update did not
        happen and its activations are invalid): the caller drops its metrics.  Bookkeeping:
        the sticky flags stay set until they are cleared HERE, so every step enqueued between
        the fault and its detection -- in the lagged (sync=False) loop: this one and the one
        already in flight behind it -- was vetoed on the device; all of them are taken back
        from the optimiser's iteration count (Adam bias correction, decay) and from the
        noise-stream step AT ONCE, so no later step re-uses an iteration number.
        Evaluation (train=False) decides on this rank's own flags: no collective may be issued
        from test_on_batch (rank 0 alone runs the final test), and a rank that evaluates on the
        stepwise kernels for a while computes the same arithmetic as the others."""
        inflight = self._enqueued - self._checked       # train steps not yet checked (>= 1)
        if train:
            self._checked += 1
        if not bool(flags.any().item()):
            return False
        from .._lib import AsrHipError
        if gen < self._fault_gen:
            return True                 # enqueued before the fallback took effect: known
        if self.lstm_mode == 1:
            raise AsrHipError('a recurrent LSTM kernel reported a timeout in stepwise mode: '
                              'device fault')
        if train and self.optimizer is not None:
            n = max(1, inflight)
            self.optimizer.iterations = max(0, self.optimizer.iterations - n)
            self._step = max(0, self._step - n)
            self.vetoed_steps += n
        # A persistent kernel abandoned a bounded spin (a peer workgroup was not co-resident).
        # The update of every step enqueued since was vetoed on the device (ops.optim_guard),
        # so the weights are intact: clear the flags and go on with the stepwise kernels (one
        # launch per step, identical arithmetic, no co-residency) for a while.
        import logging
        logging.getLogger(__name__).warning(
            'persistent LSTM kernel timed out waiting for a peer workgroup; the affected '
            'step(s) were skipped; stepwise kernels (mode 1) for the next %d steps',
            self._retry_gap)
        torch.cuda.synchronize(self.device)
        ops.clear_timeout_flags(self.device)
        self._gbuf[self.n_params:].zero_()
        self.lstm_mode = 1
        self.fallbacks += 1
        self._fault_gen += 1
        self._retry_at = self._step + self._retry_gap
        self._retry_gap = min(2 * self._retry_gap, 1 << 14)
        return True

    def _allreduce(self):
        """Sums the gradients over the ranks: RCCL through the library's C ABI (asr_comm_*,
        parallel.CapiComm).  Layers whose weight gradients were finished during BPTT were already
        reduced there, asynchronously on the communicator's stream (backward(), only where a
        recurrence leaves CUs free); the rest of the flat buffer -- everything, where BPTT fills
        the chip -- is reduced here in place, TOGETHER with the two timeout-flag slots behind
        it, and the current stream then waits for all of them."""
        if not self._dist_active():
            return 1
        from ..parallel import grad_comm, world_size
        comm = grad_comm(self._gbuf.device)
        self._collect_flags()
        total = self._gbuf.numel()      # (the flag slots and any BN moments blocks behind them)
        covered = sorted(getattr(self, '_ar_covered', []))
        pos = 0
        for lo, hi in covered + [(total, total)]:
            if lo > pos:
                comm.allreduce_after(self._gbuf[pos:lo], None)   # behind the current stream's work
            pos = max(pos, hi)
        comm.join(None)
        self._ar_covered = []
        return world_size()

    def train_on_batch(self, inputs, outputs=None, masks=None, sync=True):
        """One optimisation step on a batch ``[x, labels, inputs_length]``.

        Returns [loss, ctc_loss, decoder_loss, decoder_ler] when ``sync`` (like
        Keras), else the device tensors needed to compute them later."""
        assert self.optimizer is not None, 'compile() first'
        self._maybe_retry_persistent()
        slab, labels, lens = self._unpack_inputs(inputs)
        N = len(labels)
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # a rank's shard of a global batch says how many samples the GLOBAL batch had (shards
        # are unequal when the batch is not divisible by the world; parallel.ShardedBatch)
        n_global = n_ref = getattr(inputs, 'n_global', N * world)
        if getattr(inputs, 'n_local', N) == 0:
            n_global = 0
        gen = self._fault_gen
        ctc, logits, sl = self.loss_and_grads(slab, labels, lens, training=True, masks=masks,
                                              n_global=n_global, n_ref=n_ref)
        self._allreduce()
        self._step += 1
        self._enqueued += 1
        self.optimizer.step(self)
        self._bn_update()
        dec, dlen = ops.ctc_greedy(logits, sl, N)
        if not sync:
            # snapshots of this step's small result tensors (the buffers behind them are
            # reused by the next step): metrics can then be fetched one step later
            return (ctc.clone(), dec.clone(), dlen.clone(), self._norm[1:2].clone(),
                    self._flag_snapshot(), gen)
        m = self._metrics(ctc, dec, dlen, labels, gen=gen)
        if m is None:
            # the step was vetoed (timeout): run it again, on the stepwise kernels
            return self.train_on_batch(inputs, outputs, masks=masks, sync=True)
        return m

    def _lagged(self, pending):
        """Metrics of a step enqueued earlier, or None if its update was vetoed."""
        (ctc, dec, dlen, pen, flags, gen), labels, _ = pending
        return self._metrics(ctc, dec, dlen, labels, pen=pen, flags=flags, gen=gen)

    def _metrics(self, ctc, dec, dlen, labels, hyps=None, pen=None, flags=None, gen=None,
                 train=True):
        ctc_h = ctc.cpu().numpy().astype(np.float64)
        # the persistent recurrent kernels bound every spin; one that gave up has left
        # invalid activations behind: handled here, at the step's host synchronisation point
        flags = self._flag_snapshot() if flags is None else flags
        if self._handle_timeout(flags, self._fault_gen if gen is None else gen, train):
            return None
        if pen is not None:
            pen = float(pen.item())
        else:
            pen = float(self._norm[1].item()) if self.optimizer is not None else 0.0
        if hyps is None:
            dec_h, dlen_h = dec.cpu().numpy(), dlen.cpu().numpy()
            hyps = [dec_h[n, :dlen_h[n]].tolist() for n in range(len(labels))]
        ler = float(np.mean(ops.edit_distance_host(hyps, [list(l) for l in labels])))
        ctc_mean = float(np.mean(ctc_h))
        return [ctc_mean + pen, ctc_mean, 0.0, ler]

    def test_on_batch(self, inputs, outputs=None):
        slab, labels, lens = self._unpack_inputs(inputs)
        N = len(labels)
        lab, lab_len, sl = self._prep_labels(labels, lens, slab.shape[0])
        logits = self.forward(slab, training=False, need_grad=False, n_valid=N,
                              seq_len=sl if self._needs_lens else None,
                              in_len=self._input_lens(lens))
        ctc = ops.ctc_loss_grad(logits, lab, lab_len, sl, N, grad=None)
        hyps = None
        dec = dlen = None
        if self.decoder.get('is_greedy', True):
            dec, dlen = ops.ctc_greedy(logits, sl, N)
        else:
            dec, dlen = self._beam(logits, sl, N)
        # l2 penalty of the current weights (reported in 'loss', as Keras does)
        if self.optimizer is None or self._step == 0:
            w2 = 0.0
            flat = self.params
            for off, n, l2 in self._segments:
                if l2:
                    w2 += l2 * float((flat[off:off + n].double() ** 2).sum().item())
            self._norm[1] = w2
        m = self._metrics(ctc, dec, dlen, labels, hyps, train=False,
                          flags=ops.lstm_timeout_flags(self.device))
        if m is None:       # a forward kernel timed out: evaluate the batch again, stepwise
            return self.test_on_batch(inputs, outputs)
        return m

    def predict(self, x, inputs_length=None):
        """Decoded label sequences for a batch (greedy or beam, per self.decoder), or the
        (N, T, C) logits when the model was loaded without a decoder (predict.py's
        --no_decoder).  ``x`` may also be the ``[inputs, inputs_length]`` list a
        predict-mode DatasetIterator yields (predict.py:88)."""
        if isinstance(x, list) and len(x) == 2 and inputs_length is None:
            x, inputs_length = x
        if isinstance(x, tuple) and x[0] == 'slab':
            x = x[1]
        slab = x if (torch.is_tensor(x) and x.dim() == 3 and x.shape[1] % 16 == 0) else self.to_slab(x)
        N = len(inputs_length) if inputs_length is not None else slab.shape[1]
        lens = np.asarray(inputs_length if inputs_length is not None else [slab.shape[0]] * N).reshape(-1)
        sl = None
        if self._needs_lens or self.decoder is not None:
            sl = self._key_lens(self.out_lengths(lens), slab.shape[0]).astype(np.int32)
            sl = torch.as_tensor(sl).to(self.device)
        logits = self.forward(slab, training=False, need_grad=False, n_valid=N,
                              seq_len=sl if self._needs_lens else None,
                              in_len=self._input_lens(lens))
        if self.decoder is None:
            return logits[:, :N].permute(1, 0, 2).contiguous().cpu().numpy()
        if self.decoder.get('is_greedy', True):
            dec, dlen = ops.ctc_greedy(logits, sl, N)
            dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
            return [dec[n, :dlen[n]].tolist() for n in range(N)]
        dec, dlen = self._beam(logits, sl, N)
        dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
        return [dec[n, :dlen[n]].tolist() for n in range(N)]

    def stream(self, n_streams=1, step=None, beam=None, feature=None):
        """A StreamSession (core/stream.py, K26): cached chunk-by-chunk inference of n_streams
        streams in lock-step, ``step`` strided frames per internal step (a multiple of the
        attention chunk; default: the smallest one >= 16).  Raises ValueError, naming the stage
        and the reason, before any device call unless every attention stage has a window (chunk,
        left >= 0, 0), every depthwise convolution is causal and every other stage is per-frame at
        inference or the two-convolution front-end; NotImplementedError for a beam decoder
        unless ``beam`` asks for it.  beam=True: the session decodes with the device beam search
        (K27) at the width, merge_repeated and LM of self.decoder; a dict (beam_width,
        merge_repeated, lm, lm_alpha, lm_beta, max_frames) overrides them.  feed() then returns
        the labels newly committed, hypothesis() the current best, finish() the rest
        (StreamSession); max_frames (strided frames per stream, default 3000) sizes the prefix
        tree: about max_frames * beam_width * (num_classes - 1) * 8 bytes per stream.
        feature: a norm='running' extractor of preprocessing.audio; the session then owns its
        FeatureStream and takes raw samples through feed_audio / finish_audio (K30)."""
        from .stream import StreamSession
        return StreamSession(self, n_streams, step, beam, feature)

    def align(self, x, labels, inputs_length):
        """Forced alignment (K19): where in its utterance each label of a KNOWN transcript lies.
        ``x`` as predict takes it, ``labels`` a list of label lists, ``inputs_length`` in input
        frames.  A transcript too long for its utterance raises the ValueError training raises.
        Returns {'alignments': [{'segments': [(label_index, label, start, end_exclusive), ...],
        'score': log-probability of the path, 'path': lattice state per logit frame}, ...],
        'time_stride': input frames per logit frame}; segment bounds are in LOGIT frames."""
        if isinstance(x, tuple) and x[0] == 'slab':
            x = x[1]
        slab = x if (torch.is_tensor(x) and x.dim() == 3 and x.shape[1] % 16 == 0) else self.to_slab(x)
        labels = [np.asarray(l).reshape(-1) for l in labels]
        N = len(labels)
        lens = np.asarray(inputs_length).reshape(-1)
        lab, lab_len, sl = self._prep_labels(labels, lens, slab.shape[0])
        logits = self.forward(slab, training=False, need_grad=False, n_valid=N,
                              seq_len=sl if self._needs_lens else None,
                              in_len=self._input_lens(lens))
        from .ctc_utils import align_paths
        path, score = align_paths(logits, lab, lab_len, sl, N)
        sl_h = sl.cpu().numpy()
        out = [{'segments': ops.ctc_segments(path[n], labels[n]), 'score': float(score[n]),
                'path': path[n, :int(sl_h[n])].tolist()} for n in range(N)]
        return {'alignments': out, 'time_stride': int(np.prod(self.time_strides or [1]))}

    def _beam(self, logits, seq_len_dev, N):
        """core/ctc_utils.py:48-50 (K9): the library's host decoder (decode_host.cpp: one
        utterance per host thread, on a copy of the logits) or the device decoder (beam.hip: the
        logits stay in HBM) -- same strings either way; ops.beam_decoder_choice picks (host
        while every utterance gets its own host thread, ASR_BEAM=device / host force one).  With
        a character LM in self.decoder (``lm``, ``lm_alpha``, ``lm_beta``) the LM forms of both."""
        width = int(self.decoder.get('beam_width', 100))
        merge = self.decoder.get('merge_repeated', True)
        from .ctc_utils import lm_of
        lm = lm_of(self.decoder, logits.shape[2])   # (CharLM, alpha, beta) or None
        if ops.beam_decoder_choice(N, width, logits.shape[2]) == 'device':
            if lm is None:
                dec, dlen, _ = ops.ctc_beam_search(logits, seq_len_dev, N, width, merge)
            else:
                dec, dlen, _ = ops.ctc_beam_search_lm(
                    logits, seq_len_dev, N, width, merge,
                    lm[0].fused_device(lm[1], lm[2], logits.device), lm[0].order)
            return dec, dlen
        lens = seq_len_dev.cpu().numpy()
        if lm is None:
            hyps, _ = ops.ctc_beam_search_host(logits.cpu().numpy(), lens, N, width, merge)
        else:
            hyps, _ = ops.ctc_beam_search_lm_host(logits.cpu().numpy(), lens, N, width, merge,
                                                  lm[0].fused(lm[1], lm[2]), lm[0].order)
        T = logits.shape[0]
        dec = np.full((N, T), -1, np.int32)
        for n, h in enumerate(hyps):
            dec[n, :len(h)] = h
        return torch.from_numpy(dec), torch.tensor([len(h) for h in hyps], dtype=torch.int32)

    # ------------------------------------------------------------------ loops
    def fit_generator(self, generator, samples_per_epoch, nb_epoch, verbose=1, callbacks=None,
                      validation_data=None, nb_val_samples=None, max_q_size=10, nb_worker=1,
                      initial_epoch=0, **kwargs):
        """Keras-1.2.2 signature (train.py:213-217).  Like Keras' generator queue
        (``nb_worker=1``: ONE producer thread, ``max_q_size`` batches deep) the batches
        are drawn on a background thread, so HDF5 reads / padding / label parsing overlap
        the GPU step; the per-batch metrics of step i are fetched while step i+1 runs
        (the step itself never synchronises with the host)."""
        callbacks = callbacks or []
        history = []
        for cb in callbacks:
            cb.set_model(self)
            cb.on_train_begin()
        feeder = _Feeder(generator, max_q_size, self.device)
        try:
            for epoch in range(initial_epoch, nb_epoch):
                t0 = time.time()
                seen, seen_local, sums = 0, 0, np.zeros(4)
                pending = None              # (device results, labels, n) of the previous step

                def account(pend):
                    # a step whose update was vetoed (recurrent-kernel timeout) has no valid
                    # activations: it counts for nothing
                    m = self._lagged(pend)
                    if m is None:
                        return 0
                    sums[:] += np.array(m) * pend[2]
                    return pend[2]
                while seen < samples_per_epoch:
                    inputs, outputs = feeder.get()
                    slab, labels, lens = self._unpack_inputs(inputs)
                    # an epoch counts GLOBAL samples; this rank's metrics weigh its own
                    n = getattr(inputs, 'n_local', len(labels))
                    batch = [('slab', slab), labels, lens]
                    if hasattr(inputs, 'n_global'):
                        from ..parallel import ShardedBatch
                        batch = ShardedBatch(batch, inputs.n_global, inputs.n_local)
                    res = self.train_on_batch(batch, outputs, sync=False)
                    if pending is not None:
                        seen_local += account(pending)
                    pending = (res, labels, n)
                    seen += getattr(inputs, 'n_global', len(labels))
                if pending is not None:
                    seen_local += account(pending)
                # the training-side logs are GLOBAL means: callbacks that monitor them (LR
                # schedules, early stopping) must take the same decision on every rank
                from ..parallel import reduce_metrics
                logs = dict(zip(self.metrics_names, reduce_metrics(sums, seen_local)))
                if validation_data is not None:
                    val = self.evaluate_generator(validation_data, nb_val_samples)
                    for k, v in zip(self.metrics_names, val):
                        logs['val_' + k] = v
                if verbose:
                    shown = ' - '.join('%s: %.4f' % (k, logs[k]) for k in
                                       ('loss', 'decoder_ler', 'val_loss', 'val_decoder_ler')
                                       if k in logs)
                    print('Epoch %d/%d - %.0fs - %s' % (epoch + 1, nb_epoch, time.time() - t0,
                                                        shown))
                history.append(logs)
                for cb in callbacks:
                    cb.on_epoch_end(epoch, logs)
                if self.stop_training:
                    break
        finally:
            feeder.close()
        for cb in callbacks:
            cb.on_train_end()
        return history

    def evaluate_generator(self, generator, val_samples, max_q_size=10, nb_worker=1, **kwargs):
        """Returns [loss, ctc_loss, decoder_loss, <decoder>_ler] averaged with batch-size
        weights (train.py:223-227, eval.py:76-80).  Batches are drawn on a producer thread
        (Keras' generator queue), so host reads overlap the forward pass and the decoder."""
        seen, sums = 0, np.zeros(4)
        feeder = _Feeder(generator, max_q_size, self.device)
        try:
            while seen < val_samples:
                inputs, outputs = feeder.get()
                n = len(np.asarray(inputs[2]).reshape(-1))
                sums += np.array(self.test_on_batch(inputs, outputs)) * n
                seen += n
        finally:
            feeder.close()
        return (sums / max(seen, 1)).tolist()
