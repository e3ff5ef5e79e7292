"""Writes tests/golden/engine_trace_parent.json: the sequence of library calls one training step
(and, for the small models, one inference pass) of ``Model`` makes -- which call, on which
stream, on which buffers -- recorded ON THE GPU from the commit BEFORE the stage-kind table of
asr_study_amd/core/stages.py existed (8426f04), when ``Model.forward`` / ``Model.backward`` were
one ``if s.kind == ...`` chain each.  The JSON was written by running this file on that commit,
before the engine was touched; tests/test_gpu_engine_trace.py records every case again and
compares for equality.

The recorder wraps every public callable the ``asr_study_amd.ops`` module defines, and the
``fwd`` / ``dgrad`` / ``wgrad`` methods of ``ops.Conv2d``, with a pass-through (the real kernels
run) that appends one line per call the ENGINE makes (not those the library makes inside
itself: some sit behind process-wide caches): ``<stream> <name>(<arguments>)``.

  stream    main / side / pipe (``torch.cuda.current_stream()`` against ``model._side`` /
            ``model._pipe``), any other stream other<k>, numbered by first appearance
  a tensor  <base>+<element offset>[<shape>|<stride>] (and its dtype unless float32); base is
            params, gbuf, bn_running, one, the name of the ``model._bufs`` entry that contains
            its ``data_ptr()``, x (the input slab), else tmp<k>, numbered by first appearance
            (the recorder keeps every such tensor alive, so k names one allocation)
  HlPlanes  their ``model._hl`` name and (rows, k)
  the rest  numbers, strings, None, tuples and lists as they are

It does not see torch event records and waits, nor torch's own kernels (copies, fills).

Run (needs a GPU and the built library): python tests/golden/gen_engine_trace.py"""
import contextlib
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

_TF = dict(num_features=16, num_classes=6, d_model=32, num_heads=2, num_layers=1)
_DS2 = dict(num_features=16, num_classes=6, num_hiddens=8, num_layers=1, conv_filters=4,
            batch_norm=True)
_RHN = dict(num_features=13, num_classes=6, num_hiddens=10, num_layers=1, dropout=0.2)
# (name, factory, arguments, N, T, also trace an inference pass)
CASES = [
    ('transformer', 'transformer', dict(_TF), 5, 20, True),
    ('conformer', 'conformer', dict(_TF), 5, 20, True),
    ('conformer_specaug', 'conformer', dict(_TF, spec_augment=True), 5, 20, True),
    ('deep_speech2_bn', 'deep_speech2', dict(_DS2), 5, 20, True),
    ('deep_speech2_gru_seqbn', 'deep_speech2', dict(_DS2, rnn_type='gru',
                                                    batch_norm='recurrent'), 5, 20, True),
    ('deep_speech2_gru_ln', 'deep_speech2', dict(_DS2, batch_norm='layer', rnn_type='gru'),
     5, 20, True),
    ('deep_speech', 'deep_speech', dict(num_features=13, num_hiddens=12, num_classes=6),
     5, 19, True),
    ('rhn', 'rhn', dict(_RHN), 5, 19, True),
    ('rhn_d3_uncoupled_sum', 'rhn', dict(_RHN, depth=3, coupling=False, merge_mode='sum'),
     5, 19, True),
    ('brsmv1_mi_ln_res', 'brsmv1', dict(num_features=13, num_classes=6, num_hiddens=12,
                                        num_layers=2, mi=[1.0, .5, .5], layer_norm=[1.0, 0.0],
                                        residual='sum', dropout=0.2), 5, 19, True),
    # the frame-range pipeline, its halves form, the tail fork, side-stream weight gradients
    ('brsmv1_256_pipeline', 'brsmv1', dict(num_hiddens=256, num_layers=2, dropout=0.0),
     32, 32, False),
    # packed-operand GEMMs, planes written by BPTT, compact BPTT with deferred pending work
    ('brsmv1_512_compact', 'brsmv1', dict(num_hiddens=512, num_layers=3, dropout=0.0),
     64, 16, False),
]


class Recorder(object):
    def __init__(self, model, x):
        import torch
        from asr_study_amd import ops
        self.torch, self.ops, self.m, self.x = torch, ops, model, x
        self.lines, self.depth = [], 0
        self.main = torch.cuda.current_stream(model.device)
        self.streams, self.tmps, self.keep = [], {}, []

    def stream(self):
        cur = self.torch.cuda.current_stream(self.m.device)
        for name, s in (('main', self.main), ('side', self.m._side), ('pipe', self.m._pipe)):
            if cur == s:
                return name
        if cur not in self.streams:
            self.streams.append(cur)
        return 'other%d' % self.streams.index(cur)

    def bases(self):
        m = self.m
        yield 'params', m.params
        yield 'gbuf', m._gbuf
        yield 'bn_running', m.bn_running
        if hasattr(m, '_one'):
            yield 'one', m._one
        for key, b in m._bufs.items():
            yield str(key[0]), b
        yield 'x', self.x

    def tensor(self, t):
        p = t.data_ptr()
        where = None
        if t.numel():
            for name, b in self.bases():
                lo = b.data_ptr()
                if lo <= p < lo + b.numel() * b.element_size():
                    where = (name, (p - lo) // t.element_size())
                    break
        if where is None:
            lo = t.untyped_storage().data_ptr()
            if lo not in self.tmps:
                self.tmps[lo] = 'tmp%d' % len(self.tmps)
                self.keep.append(t)
            where = (self.tmps[lo], (p - lo) // t.element_size())
        dt = '' if t.dtype == self.torch.float32 else str(t.dtype).replace('torch.', ':')
        return '%s+%d[%s|%s]%s' % (where[0], where[1], 'x'.join(map(str, t.shape)),
                                  ','.join(map(str, t.stride())), dt)

    def render(self, v):
        if self.torch.is_tensor(v):
            return self.tensor(v)
        if isinstance(v, self.HlPlanes):
            for key, b in self.m._hl.items():
                if b is v:
                    return '%s(%d,%d)' % (key[0], v.rows, v.k)
            return 'planes?(%d,%d)' % (v.rows, v.k)
        if isinstance(v, (list, tuple)):
            return ('(%s)' if isinstance(v, tuple) else '[%s]') % ', '.join(map(self.render, v))
        if isinstance(v, (np.generic,)):
            v = v.item()
        if v is None or isinstance(v, (bool, int, float, str)):
            return repr(v)
        return str(v) if isinstance(v, self.torch.device) else '<%s>' % type(v).__name__

    def wrap(self, name, fn, skip_self=False):
        def call(*a, **k):
            shown = a[1:] if skip_self else a
            args = [self.render(v) for v in shown] + ['%s=%s' % (n, self.render(k[n]))
                                                      for n in sorted(k)]
            if self.depth == 0:     # (what the library calls inside itself is the library's)
                self.lines.append('%s %s(%s)' % (self.stream(), name, ', '.join(args)))
            self.depth += 1
            try:
                return fn(*a, **k)
            finally:
                self.depth -= 1
        return call

    @contextlib.contextmanager
    def recording(self):
        ops = self.ops
        self.HlPlanes = ops.HlPlanes
        saved = {n: v for n, v in vars(ops).items()
                 if not n.startswith('_') and (inspect.isfunction(v) or inspect.isclass(v))
                 and v.__module__ == ops.__name__}
        methods = {n: getattr(ops.Conv2d, n) for n in ('fwd', 'dgrad', 'wgrad')}
        try:
            for n, v in saved.items():
                setattr(ops, n, self.wrap(n, v))
            for n, v in methods.items():
                setattr(saved['Conv2d'], n, self.wrap('Conv2d.' + n, v, skip_self=True))
            yield self
        finally:
            for n, v in saved.items():
                setattr(ops, n, v)
            for n, v in methods.items():
                setattr(saved['Conv2d'], n, v)


def inputs(m, N, T):
    """(slab, labels, lengths): ragged lengths that leave room for the labels behind any time
    stride; the values do not enter the trace."""
    rs = np.random.RandomState(3)
    slab = m.to_slab(rs.standard_normal((N, T, m.num_features)).astype(np.float32))
    lens = np.array([T - 2 * (n % 4) for n in range(N)])
    labels = [[1 + n % 4, 2] for n in range(N)]
    return slab, labels, lens


def trace(factory, kwargs, N, T, infer):
    """{'train': lines of one loss_and_grads(training=True)[, 'infer': lines of one
    forward(training=False, need_grad=False)]} and the model."""
    import torch
    from asr_study_amd.core import models
    m = getattr(models, factory)(device='cuda:0', seed=0, **kwargs)
    slab, labels, lens = inputs(m, N, T)
    out = {}
    rec = Recorder(m, slab)
    with rec.recording():
        m.loss_and_grads(slab, labels, lens, training=True)
    out['train'] = rec.lines
    if infer:
        sl = torch.as_tensor(np.asarray(m.out_lengths(lens), np.int32)).to(m.device)
        rec = Recorder(m, slab)
        with rec.recording():
            m.forward(slab, training=False, need_grad=False, n_valid=N,
                      seq_len=sl if m._needs_lens else None)
        out['infer'] = rec.lines
    torch.cuda.synchronize()
    return out, m


if __name__ == '__main__':
    table = {}
    only = sys.argv[2:]             # (case names: a subset, in this order)
    for name, factory, kw, N, T, infer in (sorted((c for c in CASES if c[0] in only),
                                                  key=lambda c: only.index(c[0]))
                                           if only else CASES):
        table[name], m = trace(factory, kw, N, T, infer)
        print(name, {k: len(v) for k, v in table[name].items()},
              getattr(m, '_compact_launches', None), flush=True)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'engine_trace_parent.json')
    with open(dst, 'w') as f:
        json.dump(table, f, sort_keys=True, indent=0)
        f.write('\n')
