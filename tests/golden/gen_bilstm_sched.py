"""Writes tests/golden/bilstm_sched_parent.json: the SCHEDULE of the two-direction LSTM stage --
every library call AND every event record, event wait and stream wait, on which stream, in which
order -- and the bits it computed, recorded ON THE GPU at the commit BEFORE the two BiLSTM bodies
left ``Model`` for asr_study_amd/core/bilstm.py and were cut into phases (13a71ec).  The JSON was
written by running this file on that commit, before the engine was touched;
tests/test_gpu_bilstm_sched.py records every case again and compares for equality.

The recorder is the one of gen_engine_trace.py, whose ``recording()`` here also patches
``torch.cuda.Event.record`` and ``torch.cuda.Stream.wait_event`` / ``wait_stream`` /
``record_event`` for its duration.  They append to the same list, between the ``ops`` lines:

  <stream> record e<k>           the stream is the one the event is recorded ON (the argument, or
                                 the current stream without one)
  <stream> wait e<k>             the stream that waits
  <stream> wait_stream <name>

Events are numbered by first appearance (the recorder keeps them alive, so k names one event).
What torch does inside one of the four (``wait_stream`` records an event and waits for it) and
what the library does inside an ``ops`` call is not listed.

A case builds ONE model under its switches (``os.environ``, restored afterwards) and runs its
steps on it.  A training step is ``Model.forward(slab, training=True, masks=..., n_real=N)`` and
``Model.backward(dlogits)``, slab and dlogits from one RandomState; an inference step is
``Model.forward(slab, training=False, need_grad=False, n_valid=...)``.  CTC is not run, for the
reason gen_rec_bits.py gives.  Recorded per step:

  calls   the recorder's full lines (in the file: indices into one table of distinct lines)
  bits    the SHA-256 of the raw bytes of the real rows of the logits and of every array of
          ``get_gradients()``; left out of a case whose bits differed between two recordings
          on the parent (second argument below)
  compact_launches, dz_measure_passes      the model's counters behind the step

Run (needs a GPU and the built library): python tests/golden/gen_bilstm_sched.py [dst [earlier]]
-- ``earlier``: a file this wrote before; a case whose bits differ from it keeps its calls only."""
import contextlib
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

_spec = importlib.util.spec_from_file_location('gen_engine_trace',
                                               os.path.join(HERE, 'gen_engine_trace.py'))
trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(trace)

_B = dict(num_features=13, num_classes=6)
_256 = dict(_B, num_hiddens=256, num_layers=2, dropout=0.0)
_512 = dict(_B, num_hiddens=512, num_layers=3, dropout=0.0)
_12 = dict(_B, num_hiddens=12, num_layers=2, dropout=0.2)
_S256 = dict(N=32, T=32, steps=2)
# three steps, the weights replaced (by themselves) before the third: the measuring BPTT pass
# runs at step 1, not at step 2, and again once the weights epoch has moved
_S512 = dict(N=64, T=16, steps=3, reweigh=2)


def _case(name, kw, env=None, N=5, T=19, steps=2, reweigh=None, infer=None, zone=False):
    return dict(name=name, kw=kw, env=env or {}, N=N, T=T, steps=steps, reweigh=reweigh,
                infer=infer, zone=zone)


CASES = [
    # the frame-range pipeline with halves and the tail fork, in both passes; weight gradients
    # deferred to the side stream (streams: main, side and pipe)
    _case('h256_pipeline', _256, **_S256),
    # the halves' tails one after the other on the main stream
    _case('h256_no_tail_fork', _256, {'ASR_PIPE_TAIL_FORK': '0'}, **_S256),
    # whole-frame pipeline: wait_event(inner_done) / wait_event(dx_inner) BEHIND the outer GEMMs
    _case('h256_whole_frames', _256, {'ASR_PIPE_HALVES': '0'}, **_S256),
    # one masked GEMM per direction in _gate_gemm, _gate_gemm_half, _dx_gemm, _dx_gemm_dir and
    # grads_U / grads_W
    _case('h256_dropout', dict(_256, dropout=0.2), **_S256),
    # per-tile GEMMs without the pipeline: dX in one piece, weight gradients still deferred
    _case('h256_no_pipeline', _256, {'ASR_PIPELINE': '0'}, **_S256),
    # ... and the ``not overlap`` placement: everything on the main stream
    _case('h256_no_overlap', _256, {'ASR_OVERLAP': '0'}, **_S256),
    # packed operands, weight planes packed aside, dz planes written by BPTT behind a measuring
    # pass, compact BPTT while weight gradients are pending, the bottom layer's shared tail
    _case('h512_compact', _512, **_S512),
    # the pack pass behind BPTT, two input plane sets out of one pack, one gemm_hl per direction
    # for zx, dx and dW
    _case('h512_dropout_no_planes', dict(_512, dropout=0.2), {'ASR_BPTT_PLANES': '0'}, **_S512),
    # every weight pack on the calling stream
    _case('h512_pack_w_inline', _512, {'ASR_PACK_W_ASIDE': '0'}, **_S512),
    # a chip-filling BPTT per layer, nothing beside it
    _case('h512_no_compact', _512, {'ASR_BPTT_COMPACT': '0'}, **_S512),
    # unbounded output: the measured bound of |y| (input planes, dU), the variant kernel above
    # packed planes with a pack pass
    _case('h512_relu', dict(_512, activation='relu'), **_S512),
    # layer-norm cell with multiplicative integration: x@W kept per layer, the max of two
    # gradient slabs, pgrad = the cell parameters' per-row sums
    _case('h12_mi_ln_res', dict(_B, num_hiddens=12, num_layers=2, mi=[1.0, .5, .5],
                                layer_norm=[1.0, 0.0], residual='sum', dropout=0.2)),
    # multiplicative integration alone: the variant kernel with wx / dwx / dmi, pgrad = dmi
    _case('h12_mi', dict(_12, mi=[1.0, .5, .5])),
    # zoneout on both states, explicit (T, 2, Hp) coefficients in ``masks``
    _case('h12_zoneout', dict(_12, zoneout=0.3), zone=True),
    # one frame: dU is zero-filled (kk <= 0), per-tile form ...
    _case('h12_one_frame', _12, T=1, steps=1),
    # ... and packed form
    _case('h512_one_frame', _512, N=16, T=1, steps=1),
    # inference, one utterance then the whole batch: the tile-free kernel on zero-created
    # buffers and no pipeline, then the training kernels without what only BPTT reads
    _case('h256_infer', _256, N=32, T=32, infer=(1, 32)),
    _case('h512_infer', _512, N=64, T=16, infer=(1, 64)),
]
NAMES = [c['name'] for c in CASES]


class SchedRecorder(trace.Recorder):
    """The Recorder plus the event and stream-wait lines (module doc)."""

    def __init__(self, model, x):
        super(SchedRecorder, self).__init__(model, x)
        self.events, self.inner = [], 0

    def stream_name(self, st):
        for name, s in (('main', self.main), ('side', self.m._side), ('pipe', self.m._pipe)):
            if st == s:
                return name
        if st not in self.streams:
            self.streams.append(st)
        return 'other%d' % self.streams.index(st)

    def event(self, ev):
        for k, e in enumerate(self.events):
            if e is ev:
                return 'e%d' % k
        self.events.append(ev)
        return 'e%d' % (len(self.events) - 1)

    def sync(self, fn, line):
        """Pass-through for one of the four torch methods; line(*args) -> its text."""
        def call(*a, **k):
            if self.depth == 0 and self.inner == 0:
                self.lines.append(line(*a, **k))
            self.inner += 1
            try:
                return fn(*a, **k)
            finally:
                self.inner -= 1
        return call

    @contextlib.contextmanager
    def recording(self):
        cuda = self.torch.cuda

        def on(stream):
            return cuda.current_stream() if stream is None else stream
        patches = [
            (cuda.Event, 'record', lambda ev, stream=None:
             '%s record %s' % (self.stream_name(on(stream)), self.event(ev))),
            (cuda.Stream, 'wait_event', lambda st, ev:
             '%s wait %s' % (self.stream_name(st), self.event(ev))),
            (cuda.Stream, 'wait_stream', lambda st, other:
             '%s wait_stream %s' % (self.stream_name(st), self.stream_name(other))),
            (cuda.Stream, 'record_event', lambda st, ev=None:
             '%s record %s' % (self.stream_name(st), 'e?' if ev is None else self.event(ev))),
        ]
        saved = [(cls, n, cls.__dict__[n]) for cls, n, _ in patches]
        with super(SchedRecorder, self).recording():
            try:
                for cls, n, line in patches:
                    setattr(cls, n, self.sync(cls.__dict__[n], line))
                yield self
            finally:
                for cls, n, fn in saved:
                    setattr(cls, n, fn)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _zone_masks(m, T, n_pad, rs):
    """{stage: (B_W, B_U, keep_c, keep_h)} of every BiLSTM stage: dropout masks as
    gen_rec_bits.py draws them, zoneout keep masks (T, 2, Hp) shared over the batch."""
    import torch
    out = {}
    for si, s in enumerate(m.stages):
        if s.kind == 'bilstm':
            drop = [((rs.rand(*sh) > 0.2) / 0.8) for sh in ((2, n_pad, s.f_in_pad),
                                                            (2, n_pad, s.Hp))]
            keep = [(rs.rand(T, 2, s.Hp) > 0.3) for _ in range(2)]
            out[si] = tuple(torch.as_tensor(a.astype(np.float32)).to(m.device)
                            for a in drop + keep)
    return out


def record(name):
    """The steps of one case: a list of {'calls', 'bits', ...}."""
    import torch
    from asr_study_amd.core import models
    c = CASES[NAMES.index(name)]
    old = {k: os.environ.get(k) for k in c['env']}
    os.environ.update(c['env'])
    try:
        m = models.brsmv1(device='cuda:0', seed=0, **c['kw'])
        rs = np.random.RandomState(17)
        N, T, C = c['N'], c['T'], c['kw']['num_classes']
        out = []
        for k in range(len(c['infer']) if c['infer'] else c['steps']):
            if k == c['reweigh']:
                m.set_weights(m.get_weights())
            slab = m.to_slab(rs.standard_normal((N, T, m.num_features)).astype(np.float32))
            n_pad = slab.shape[1]
            rec = SchedRecorder(m, slab)
            if c['infer']:
                nv = c['infer'][k]
                with rec.recording():
                    logits = m.forward(slab, training=False, need_grad=False, n_valid=nv)
                torch.cuda.synchronize()
                out.append({'n_valid': nv, 'calls': rec.lines,
                            'bits': {'logits': _sha(logits[:, :nv].cpu().numpy())}})
                continue
            masks = _zone_masks(m, T, n_pad, rs) if c['zone'] else None
            dl = np.zeros((T, n_pad, C), np.float32)
            dl[:, :N] = rs.standard_normal((T, N, C))
            dl = torch.as_tensor(dl).to(m.device)
            with rec.recording():
                logits = m.forward(slab, training=True, masks=masks, n_real=N)
                m.backward(dl)
            torch.cuda.synchronize()
            bits = {'logits': _sha(logits[:, :N].cpu().numpy())}
            for i, g in enumerate(m.get_gradients()):
                bits['grad%02d' % i] = _sha(g)
            out.append({'calls': rec.lines, 'bits': bits,
                        'compact_launches': m._compact_launches,
                        'dz_measure_passes': m._dz_measure_passes})
        return out
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def expand(table):
    """The file's form -> {case: steps} with ``calls`` as lines."""
    return {name: [dict(st, calls=[table['lines'][i] for i in st['calls']]) for st in steps]
            for name, steps in table['cases'].items()}


if __name__ == '__main__':
    lines, cases = [], {}
    index = {}
    earlier = None
    if len(sys.argv) > 2:
        with open(sys.argv[2]) as f:
            earlier = json.load(f)['cases']
    for name in NAMES:
        steps = record(name)
        if earlier is not None and any('bits' not in e or e['bits'] != s['bits']
                                       for e, s in zip(earlier[name], steps)):
            print(name, 'bits differ between two recordings: calls only', flush=True)
            for s in steps:
                del s['bits']
        for s in steps:
            s['calls'] = [index.setdefault(l, len(index)) for l in s['calls']]
        cases[name] = steps
        print(name, [len(s['calls']) for s in steps],
              [(s.get('compact_launches'), s.get('dz_measure_passes')) for s in steps],
              flush=True)
    lines = sorted(index, key=index.get)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'bilstm_sched_parent.json')
    with open(dst, 'w') as f:
        json.dump({'lines': lines, 'cases': cases}, f, sort_keys=True, indent=0)
        f.write('\n')
