"""K26, cached chunk-by-chunk (streaming) inference of an encoder whose look-ahead is bounded (K25:
every attention layer under a window (chunk, left >= 0, 0), every depthwise convolution causal).

``Model.stream()`` returns a ``StreamSession``.  It keeps, per stage, what the stage carries from
step to step -- the ring of keys and values of an attention layer, the ring of input frames of a
depthwise convolution, the (N, H) state of a unidirectional GRU, the (N, H) hidden and cell
states of a unidirectional LSTM (core/stages.py: the ``stream`` handlers; a bare GRU or LSTM has
no look-ahead at all), the greedy decoder's last label
-- and runs the stage list on ``step`` new strided frames at a time, one launch per stage and no
host synchronisation inside a step.  The result is the full forward of the whole utterance:
bit for bit in the attention cores and the convolutions (their kernels add the same terms in the
same order), to rounding in the GEMMs (a chunk is another M).  Forward only.

THE FRONT-END (conv=True: Convolution2D at time stride 2, then Convolution2D at stride 1) has no
cached form.  For each step the session runs the two stages over a window of buffered input
frames of a FIXED shape, with a halo on both sides, and keeps the rows no window edge has touched
(``Schedule``).  The session is defined against the full forward of a slab with an EVEN number of
input frames: the window starts at an even frame, so its outputs use the tap alignment of the
even-T 'same' rule, p1 = (kt1 - 2) // 2; an odd total length gets one zero frame appended at
``finish()``.  Input frames outside the stream and first-convolution rows outside its strided
frames are zeros, as the padding of the full forward is.
"""
import numpy as np
import torch

from .. import ops
from .stages import KINDS, STREAM_AS_FORWARD, Pass, stream_check, stream_variant

NO_END = 1 << 30            # the length of a stream whose end is not known yet


class Schedule(object):
    """Which strided frames can be emitted after how many input frames, and the front-end's
    window: plain integers, no device.

    Without a front-end a strided frame is an input frame and is emitted once its step is
    complete.  With it (kernels kt1 at stride 2, kt2 at stride 1) the first convolution's row s
    reads the input frames 2 s - p1 .. 2 s - p1 + kt1 - 1 and the second's row t the rows t - l2
    .. t + r2 of the first, l2 = (kt2 - 1) // 2, r2 = kt2 - 1 - l2: strided frame t is emitted
    once the input up to ``reach(t)`` = 2 (c_end(t) - 1 + r2) + kt1 - 1 - p1 has been fed, c_end
    the end of t's step (the reach formula of the transformer factory's docstring).  The window of
    the step [c0, c0 + step) covers the first convolution's rows c0 - l2 - a .. c0 + step - 1 + r2
    + b, where the a = ceil(p1 / 2) rows on the left and the b = ceil((kt1 - p1 - 2) / 2) rows on
    the right are the ones a window edge touches: ``rows1`` rows from 2 (c0 - l2 - a) input
    frames on, of which the second convolution's rows ``keep`` .. keep + step - 1 are the step's.
    Recomputing the halo costs ``rows1 / step`` of the front-end per step."""

    def __init__(self, step, front=None):
        self.step, self.front = int(step), front
        if front is not None:
            kt1, kt2 = front
            self.kt1, self.p1 = kt1, (kt1 - 2) // 2
            self.l2 = (kt2 - 1) // 2
            self.r2 = kt2 - 1 - self.l2
            self.a = -(-self.p1 // 2)
            self.b = max(0, -(-(kt1 - self.p1 - 2) // 2))
            self.keep = self.a + self.l2
            self.rows1 = self.keep + self.step + self.r2 + self.b
            self.stride = 2
        else:
            self.stride = 1

    def reach(self, t):
        """The last input frame strided frame t waits for."""
        c_end = (t // self.step + 1) * self.step
        if self.front is None:
            return c_end - 1
        return 2 * (c_end - 1 + self.r2) + self.kt1 - 1 - self.p1

    def ready(self, frames_in, emitted=0):
        """Strided frames that can be emitted after frames_in input frames (whole steps; emitted:
        a multiple of step known to be ready, where the search starts)."""
        n = emitted
        while self.reach(n) < frames_in:
            n += self.step
        return n

    def total(self, frames_in):
        """Strided frames of a finished stream of frames_in input frames."""
        return -(-int(frames_in) // self.stride)

    def window_start(self, c0):
        """The first input frame of the window of the step at c0 (even; negative at the start)."""
        return 2 * (c0 - self.keep)


def front_end(model):
    """(index one past the front-end's last stage, (kt1, kt2) or None).  Raises ValueError,
    naming the stage, for a convolution the session cannot window."""
    convs = [i for i, s in enumerate(model.stages) if s.kind == 'conv']
    if not convs:
        return 0, None
    for i, s in enumerate(model.stages[:convs[-1]]):
        if s.kind not in ('conv', 'reshape', 'specaug', 'noise', 'dropout'):
            raise ValueError('stage %d (%s) cannot stream: it lies before the convolution of '
                             'stage %d, and only the front-end is run over windows of the input'
                             % (i, s.kind, convs[-1]))
    strides = [model.stages[i].st for i in convs]
    if strides != [2, 1]:
        raise ValueError('stage %d (conv) cannot stream: the front-end the session windows is two '
                         'Convolution2D at time strides 2 and 1, not %r' % (convs[0], strides))
    return convs[-1] + 1, (model.stages[convs[0]].kt, model.stages[convs[1]].kt)


BEAM_MAX_FRAMES = 3000      # strided frames a beam session's tree is sized for by default


def beam_config(model, beam):
    """The beam decoder of Model.stream(beam=...), before any device call: None for beam=None;
    else a dict beam_width, merge_repeated, max_frames and lm (None or (CharLM, alpha, beta)).
    ``True`` takes width, merge_repeated and the LM from model.decoder (which must then be a beam
    decoder), a dict overrides them and may give max_frames."""
    if beam is None or beam is False:
        return None
    from . import ctc_utils
    over = {} if beam is True else dict(beam)
    unknown = set(over) - {'beam_width', 'merge_repeated', 'max_frames', 'lm', 'lm_alpha',
                           'lm_beta'}
    if unknown:
        raise ValueError('beam: unknown keys %s' % sorted(unknown))
    dec = dict(model.decoder or {})
    if beam is True and dec.get('is_greedy', True):
        raise ValueError('beam=True takes the beam decoder of the model, which has %s: give a '
                         'dict (beam_width, ...) instead'
                         % ('a greedy one' if model.decoder else 'none'))
    dec.update(over, is_greedy=False)
    cfg = dict(beam_width=int(dec.get('beam_width', 100)),
               merge_repeated=bool(dec.get('merge_repeated', True)),
               max_frames=int(dec.get('max_frames', BEAM_MAX_FRAMES)),
               lm=ctc_utils.lm_of(dec, model.num_classes))
    if not 1 <= cfg['beam_width'] <= 1024:
        raise ValueError('beam: beam_width %d, the device decoder takes 1 .. 1024'
                         % cfg['beam_width'])
    if cfg['max_frames'] < 1:
        raise ValueError('beam: max_frames %d' % cfg['max_frames'])
    return cfg


def check(model, step, beam=None):
    """What Model.stream refuses, before any device call -> (step, first encoder stage, front)."""
    for si, s in enumerate(model.stages):
        why = stream_check(model, s, si)
        if why is not None:
            raise ValueError('stage %d (%s) cannot stream: %s' % (si, s.kind, why))
    enc0, front = front_end(model)
    if beam is None and model.decoder is not None and not model.decoder.get('is_greedy', True):
        raise NotImplementedError('streaming decode is greedy unless asked otherwise: pass '
                                  'beam=True (or a dict) to Model.stream for the beam search of '
                                  'the model\'s decoder, or load it with a greedy decoder or none')
    chunk = 1
    for s in model.stages:
        if s.kind == 'mha':
            chunk = int(np.lcm(chunk, s.window[0]))
    if step is None:
        step = -(-16 // chunk) * chunk
    step = int(step)
    if step < 1 or step % chunk:
        raise ValueError('step %d: a positive multiple of the chunk, %d strided frames'
                         % (step, chunk))
    if beam is not None and step > beam['max_frames']:
        raise ValueError('beam: max_frames %d is less than one step, %d strided frames'
                         % (beam['max_frames'], step))
    return step, enc0, front


class StreamSession(object):
    """Chunk-by-chunk inference of ``n_streams`` streams that advance in lock-step (Model.stream).

    feed(x, ended=None)  x (N, t, F): t >= 0 new input frames of every stream (a stream that has
                         ended is fed zeros, whatever x holds there).  ended: None, or N entries,
                         each None or the stream's total input length -- needed for a model whose
                         layers mask by length no later than the feed that carries the stream's
                         last frame.  Runs as many whole steps as the input allows and returns the
                         new logits (N, new_frames, C) when the model has no decoder, else the
                         newly decoded labels per stream (greedy).
    finish()             the remainder, a last partial chunk included, with the true end-of-slab
                         padding; the same kind of result.  An odd number of input frames under a
                         front-end gets one zero frame appended first: the session equals the full
                         forward of THAT slab.
    reset()              zero-fills the state: the session serves another set of streams.
    frames_in, frames_out  input frames fed, strided frames emitted.
    feed_audio(samples, ended=None), finish_audio()   with Model.stream(feature=...): raw samples
                         (N, s) through the session's FeatureStream (preprocessing/audio.py,
                         norm='running') and its new rows through feed / finish; ``ended`` in
                         samples.

    With ``beam`` (K27, beam_config): the device beam search resumed chunk by chunk
    (ops.ctc_beam_stream).  feed() returns per stream the labels NEWLY COMMITTED -- the growth
    of the stable prefix, the labels on the path to the deepest common ancestor of the whole
    beam, which no later frame can change; hypothesis() the current best (labels, score) per
    stream; finish() the rest of the final best hypothesis.  Everything returned, joined, is the
    whole-utterance beam decode of the stream's logits.  A stream may have max_frames strided
    frames (default 3000): beyond, feed / finish raise ValueError before they take the input or
    launch anything, and the session stays as it was.  The tree takes
    64 + (1 + B (C - 1)) 8 + B 4 (8 with an LM) bytes per stream, B = max_frames * beam_width,
    rounded up to 256: 64.8 MB + 1.2 MB at 3000 frames, width 100 and 28 classes.

    The absolute positional table is taken as long as the stream has grown (ops.posenc_get, in
    powers of two from 1024 rows): a stream has no length to size it by."""

    def __init__(self, model, n_streams=1, step=None, beam=None, feature=None):
        self.beam = beam_config(model, beam)
        self.audio = None           # the FeatureStream of feed_audio (Model.stream(feature=))
        if feature is not None:
            if feature.num_feats != model.num_features:
                raise ValueError('feature: %s gives %s columns, the model takes %d'
                                 % (feature, feature.num_feats, model.num_features))
            self.audio = feature.stream(n_streams)
        self.step, self.enc0, front = check(model, step, self.beam)
        self.model, self.N = model, int(n_streams)
        # the decoder the session was made under: a later change of model.decoder (another
        # session of the same model with another decoder) does not reach into this one
        self.decoder = model.decoder
        if self.N < 1:
            raise ValueError('n_streams %d' % self.N)
        self.n_pad = ops.pad16(self.N)
        self.schedule = Schedule(self.step, front)
        self.state = {}             # stage index -> what the stage carries (core/stages.py)
        self._conv = {}             # front-end stage index -> its ops.Conv2d on the window
        self._beam_state = None     # ops.BeamStreamState, made at the first step
        self.reset()

    # ------------------------------------------------------------------ what the handlers use
    def zeros(self, shape):
        return torch.zeros(tuple(int(v) for v in shape), dtype=torch.float32,
                           device=self.model.device)

    def posenc_rows(self, D):
        need, cap = self.t0 + self.Tq, 1024
        while cap < need:
            cap *= 2
        return ops.posenc_get(cap, D, self.model.device)[self.t0:need]

    # ------------------------------------------------------------------ state
    def reset(self):
        for st in self.state.values():
            for k in [k for k in st if k not in ('ring', 'h', 'c')]:
                del st[k]           # (projected tables: the weights may have changed)
            # a ring, or the pair(s) of state buffers of a unidirectional GRU ('h') or LSTM ('h'
            # and 'c'), which have no ring
            for t in (([st['ring']] if 'ring' in st else []) + list(st.get('h', ()))
                      + list(st.get('c', ()))):
                t.zero_()
        self.frames_in = self.frames_out = 0
        self.t0 = self.Tq = 0
        self._ended = [None] * self.N           # input lengths, where known
        self._finished = False
        self._pend = None                       # input frames from self._base on, time major
        self._base = 0
        self._lens_host = np.full(self.N, NO_END, np.int64)      # on the strided axis
        self.lens = None                        # ... on the device, made at the first step
        self._greedy = None
        if self._beam_state is not None:
            self._beam_state.zero_()            # (the records only: the tree needs no fill)
        self._committed = [0] * self.N          # labels of the stable prefix already returned
        self._hyp = [([], 0.0) for _ in range(self.N)]
        self._stable = [0] * self.N
        if self.audio is not None:
            self.audio.reset()

    # ------------------------------------------------------------------ raw audio (K30)
    def _audio(self):
        if self.audio is None:
            raise RuntimeError('this session takes features: make it with '
                               'Model.stream(..., feature=<a norm=\'running\' extractor>) to '
                               'feed raw audio')
        return self.audio

    def feed_audio(self, samples, ended=None):
        """samples (N, s): s new samples of every stream; ended: None, or per stream None / its
        total length in SAMPLES.  The front-end's new rows (FeatureStream.feed) go through
        feed(): the same kind of result."""
        fs = self._audio()
        fs._set_ended(ended)
        known = [None if e is None else fs.frames_of(e) for e in fs._ends]
        return self.feed(fs.feed(samples), ended=known)

    def finish_audio(self):
        """Ends every stream at the samples fed, then finish()."""
        fs = self._audio()
        rows = fs.finish()
        out = self.feed(rows, ended=[fs.frames_of(e) for e in fs._ends])
        rest = self.finish()
        if self.beam is not None or self.decoder is not None:
            return [a + b for a, b in zip(out, rest)]
        return np.concatenate([out, rest], 1)

    def _set_ended(self, ended):
        if ended is None:
            return
        if len(ended) != self.N:
            raise ValueError('ended: %d entries for %d streams' % (len(ended), self.N))
        for n, e in enumerate(ended):
            if e is None or e == self._ended[n]:
                continue
            e = int(e)
            strided = self.schedule.total(e)
            if self._ended[n] is not None:
                raise ValueError('stream %d: its length was given as %d before' % (n, self._ended[n]))
            if e < 1 or e < self.frames_in or strided < self.frames_out:
                raise ValueError(
                    'stream %d: the length %d lies before what was fed (%d input frames) or '
                    'emitted (%d strided frames) as frames of the stream'
                    % (n, e, self.frames_in, self.frames_out))
            self._ended[n] = e
            self._lens_host[n] = strided
            self.lens = None

    def _append(self, x):
        """x (N, t, F) host or device -> the pending slab, an ended stream's frames as zeros."""
        m = self.model
        x = torch.as_tensor(np.asarray(x, np.float32)) if not torch.is_tensor(x) else x
        if x.dim() != 3 or x.shape[0] != self.N or x.shape[2] != m.num_features:
            raise ValueError('feed: x is (%d streams, frames, %d features), got %s'
                             % (self.N, m.num_features, tuple(x.shape)))
        t = int(x.shape[1])
        if t == 0:
            return
        slab = self.zeros((t, self.n_pad, m.f_in_pad0))
        slab[:, :self.N, :m.num_features] = x.to(m.device, dtype=torch.float32).permute(1, 0, 2)
        for n, e in enumerate(self._ended):
            if e is not None and e < self.frames_in + t:
                slab[max(0, e - self.frames_in):, n] = 0.0
        self._pend = slab if self._pend is None else torch.cat([self._pend, slab], 0)
        self.frames_in += t

    # ------------------------------------------------------------------ the public calls
    def feed(self, x, ended=None):
        if self._finished:
            raise RuntimeError('feed after finish(): reset() starts another stream')
        self._set_ended(ended)
        shape = x.shape if hasattr(x, 'shape') else np.shape(x)
        if len(shape) == 3:     # (a shape _append refuses is refused there)
            self._beam_room(self.schedule.ready(self.frames_in + int(shape[1]), self.frames_out))
        self._append(x)
        return self._run(self.schedule.ready(self.frames_in, self.frames_out))

    def finish(self):
        if self._finished:
            raise RuntimeError('finish() twice: reset() starts another stream')
        total = self.frames_in + (self.frames_in % self.schedule.stride)    # (one zero frame)
        known = [e if e is not None else total for e in self._ended]
        self._beam_room(self.schedule.total(total),
                        np.array([self.schedule.total(e) for e in known]))
        self._finished = True
        self._set_ended([total if e is None else None for e in self._ended])
        return self._run(self.schedule.total(total), end=total)

    # ------------------------------------------------------------------ steps
    def _run(self, upto, end=None):
        m, outs = self.model, []
        while self.frames_out < upto:
            self.t0, self.Tq = self.frames_out, min(self.step, upto - self.frames_out)
            if self.lens is None:
                self.lens = torch.as_tensor(self._lens_host.astype(np.int32)).to(m.device)
            a = self._front(end) if self.schedule.front else self._take()
            logits = self._encoder(a)
            if self.beam is not None:
                chunk_len = np.clip(self._lens_host - self.t0, 0, self.Tq).astype(np.int32)
                outs = [self._beam_step(logits, chunk_len)]     # (only the last one is read)
            elif self.decoder is None:
                outs.append(logits[:, :self.N].clone())
            else:
                chunk_len = np.clip(self._lens_host - self.t0, 0, self.Tq).astype(np.int32)
                if self._greedy is None:
                    self._greedy = torch.full((self.N,), -1, dtype=torch.int32, device=m.device)
                outs.append(ops.ctc_greedy_stream(logits, torch.as_tensor(chunk_len).to(m.device),
                                                  self._greedy, self.N))
            self.frames_out += self.Tq
        if self.beam is not None:
            return self._beam_result(outs)
        if self.decoder is None:
            if not outs:
                return np.zeros((self.N, 0, m.num_classes), np.float32)
            return torch.cat(outs, 0).permute(1, 0, 2).contiguous().cpu().numpy()
        labels = [[] for _ in range(self.N)]
        for dec, dlen in outs:
            dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
            for n in range(self.N):
                labels[n] += dec[n, :dlen[n]].tolist()
        return labels

    # ------------------------------------------------------------------ the beam decoder (K27)
    def _beam_room(self, upto, lens=None):
        """Refuses, before the input is taken and before any launch, the steps up to strided frame
        ``upto`` if they would take a stream past max_frames: the session stays as it was."""
        if self.beam is None or upto <= self.frames_out:
            return
        reach = int(np.minimum(self._lens_host if lens is None else lens, upto).max())
        if reach > self.beam['max_frames']:
            raise ValueError('a stream would reach %d strided frames: the beam session was made '
                             'for max_frames=%d' % (reach, self.beam['max_frames']))

    def _beam_step(self, logits, chunk_len):
        m, b = self.model, self.beam
        if self._beam_state is None:
            lm = None
            if b['lm'] is not None:
                table, alpha, beta = b['lm']
                lm = (table.fused_device(alpha, beta, m.device), table.order)
            self._beam_state = ops.BeamStreamState(self.N, m.num_classes, b['beam_width'],
                                                   b['max_frames'], lm, m.device)
        return ops.ctc_beam_stream(logits, torch.as_tensor(chunk_len).to(m.device),
                                   self._beam_state, self.N, b['beam_width'],
                                   b['merge_repeated'], b['max_frames'])

    def _beam_result(self, outs):
        """The one copy to the host of a feed: the last step's hypothesis.  -> the labels the
        stable prefix has grown by (feed) or all that is left of the best hypothesis (finish)."""
        if outs:
            dec, dlen, stable, score = outs[-1]
            dlen, stable, score = dlen.cpu().numpy(), stable.cpu().numpy(), score.cpu().numpy()
            dec = dec[:, :max(1, int(dlen.max()))].cpu().numpy()
            self._hyp = [(dec[n, :dlen[n]].tolist(), float(score[n])) for n in range(self.N)]
            self._stable = [int(v) for v in stable]
        new = []
        for n in range(self.N):
            upto = len(self._hyp[n][0]) if self._finished else \
                (self._stable[n] if outs else self._committed[n])
            new.append(self._hyp[n][0][self._committed[n]:upto])
            self._committed[n] = max(self._committed[n], upto)
        return new

    def hypothesis(self):
        """Beam sessions: the current best (labels, log score) per stream, the committed labels
        included; it may still change behind them."""
        if self.beam is None:
            raise RuntimeError('hypothesis(): the session has no beam decoder (Model.stream(beam=))')
        return [(list(l), s) for l, s in self._hyp]

    def _take(self):
        """The step's input frames off the pending slab (no front-end: they are the strided ones;
        the zero frames past the end of a finished stream never reach a step)."""
        a = self._pend[:self.Tq].contiguous()
        self._pend = self._pend[self.Tq:]
        self._base += self.Tq
        return a

    def _front(self, end):
        """The front-end over the window of this step (Schedule): input frames outside the
        stream and first-convolution rows outside its strided frames are zeros."""
        m, sc = self.model, self.schedule
        w0, rows_in = sc.window_start(self.t0), 2 * sc.rows1
        if self._pend is not None and w0 > self._base:          # frames no later window reads
            self._pend = self._pend[w0 - self._base:]
            self._base = w0
        a = m._buf('streamwin', (rows_in, self.n_pad, m.f_in_pad0))
        a.zero_()
        lo, hi = max(w0, self._base), min(w0 + rows_in, self.frames_in)
        if hi > lo:
            a[lo - w0:hi - w0].copy_(self._pend[lo - self._base:hi - self._base])
        first = True
        fp = self._pass()
        for si in range(self.enc0):
            s = m.stages[si]
            if s.kind != 'conv':
                continue            # (reshape, and what is the identity at inference)
            op = self._conv.get(si)
            if op is None:
                op = self._conv[si] = ops.Conv2d(a.shape[0], self.n_pad, s.F_in, s.C_in, s.C_out,
                                                 s.kt, s.kf, s.st, s.sf, s.clip, m.device)
            y = m._buf('streamconv%d' % si, (op.T_out, self.n_pad, s.F_out * s.C_out))
            nw = s.kt * s.kf * s.C_in * s.C_out
            op.fwd(a, m._view(s.oW, nw), m._view(s.ob, s.C_out), None if s.clip > 0 else y, y,
                   x_absmax=m._clip_bound(si))
            if first:               # rows of the first convolution that are padding, not frames
                s0 = self.t0 - sc.keep              # the strided frame of row 0
                if s0 < 0:
                    y[:-s0].zero_()
                if end is not None and sc.total(end) < s0 + sc.rows1:
                    y[max(0, sc.total(end) - s0):].zero_()
                first = False
            a = y
        return a[sc.keep:sc.keep + self.Tq]

    def _pass(self):
        return Pass(training=False, masks=None, need_grad=False, n_valid=self.N, n_real=self.N,
                    bn_weight=self.N, seq_len=None, in_len=None, n_pad=self.n_pad, pipe=False,
                    pre={}, nb=0, stage_masks=lambda i: (None, None))

    def _encoder(self, a):
        """The stages behind the front-end on the slab of the step's strided frames."""
        m, fp = self.model, self._pass()
        m._acts = [{'in': None, 'out': None} for _ in range(self.enc0)]
        for si in range(self.enc0, len(m.stages)):
            s = m.stages[si]
            kind = KINDS[s.kind]
            rec = {'in': a}
            step = stream_variant(s) or kind.stream
            if step is not None:
                a = step(m, s, si, a, self)
            else:
                assert s.kind in STREAM_AS_FORWARD
                a = kind.forward(m, s, si, a, rec, fp)
            rec['out'] = a
            m._acts.append(rec)
        return a
