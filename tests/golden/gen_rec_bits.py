"""Writes tests/golden/rec_bits_parent.json: what the recurrent stage handlers of
asr_study_amd/core/stages.py (SimpleRNN, GRU, RHN, the one-direction GRU and LSTM) computed and
launched ON THE GPU at the commit BEFORE the one- and two-direction forms came to share one set of
handlers and helpers (73c7a5f).  The JSON was written by running this file on that commit, before
the handlers were touched; tests/test_gpu_rec_bits.py records every case again and compares for
equality.

A training case builds a small model with a fixed seed and runs, per step (T, masks):
``Model.forward(training=True)`` with the masks passed in (keep > 0.2, scaled by 1 / 0.8, in the
(2, n_pad, .) shapes the kind takes) and ``Model.backward(dlogits)``, everything drawn from one
RandomState.  CTC is not run: its kernels accumulate with float atomics, the recurrences and
``ops.gemm`` do not, so the bits are repeatable.  Recorded per step:

  bits    the SHA-256 of the raw bytes of the real rows of the logits and of every array of
          ``get_gradients()``
  calls   the call skeleton, with the Recorder of gen_engine_trace.py: stream and name of every
          ``ops`` call the engine makes, and M, N, K of a ``gemm``.  It stands in for a timing: the
          same kernels in the same order at the same sizes take the time they took.

A streaming case feeds T = 7 frames to a session in chunks of 3, 3 and 1, then, after ``reset()``,
the same frames in chunks of 1, once to a session of step 3 and once to one of step 1 (a session
runs whole steps: the recurrence is called on 3, 3 and 1 frames, then on 1 frame at a time), and
records the hash of the concatenated outputs of the four passes and the skeleton.  All cases use
N = 5 (n_pad = 16) and 10 features.

Run (needs a GPU and the built library): python tests/golden/gen_rec_bits.py [dst]"""
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

N, F = 5, 10


def _gru_stack(L, o):
    o = L.GRU(10, activation='tanh')(o)         # (H no multiple of 4; first stage: no dx)
    return L.GRU(14, activation='relu')(o)


def _lstm_stack(L, o):
    o = L.LSTM(10)(o)
    return L.LSTM(14, activation='relu')(o)


def _gru_mixed(L, o):
    o = L.TimeDistributed(L.Dense(12))(o)
    o = L.DepthwiseConvolution1D(3, causal=True)(o)
    return _gru_stack(L, o)


# name -> (the layers between Input and Dense(8), the steps (T, masks on) run on ONE model)
TRAIN_CASES = {
    'gru_stack_plain': (_gru_stack, [(7, False), (1, False)]),
    'gru_stack_masks': (_gru_stack, [(7, True), (1, True)]),
    'lstm_stack_plain': (_lstm_stack, [(7, False), (1, False)]),
    'lstm_stack_masks': (_lstm_stack, [(7, True), (1, True)]),
    # the bare stage reads real rows that are padded apart
    'bigru_below_gru': (lambda L, o: L.GRU(6)(L.Bidirectional(L.GRU(6))(o)), [(7, True)]),
    'bilstm_below_lstm': (lambda L, o: L.LSTM(6)(L.Bidirectional(L.LSTM(6))(o)), [(7, True)]),
    # the two-direction users of the shared helpers
    'birnn': (lambda L, o: L.Bidirectional(L.SimpleRNN(10))(o), [(7, True)]),
    'bigru_sum': (lambda L, o: L.Bidirectional(L.GRU(10), merge_mode='sum')(o), [(7, True)]),
    'bigru_bn': (lambda L, o: L.Bidirectional(L.GRU(10, batch_norm=True))(o), [(7, True)]),
    'birhn_d2': (lambda L, o: L.Bidirectional(L.RHN(10, depth=2))(o), [(7, True)]),
}
STREAM_CASES = {'stream_gru_stack': _gru_stack, 'stream_lstm_stack': _lstm_stack,
                'stream_gru_mixed': _gru_mixed}
CASES = sorted(TRAIN_CASES) + sorted(STREAM_CASES)


class Skeleton(trace.Recorder):
    """The Recorder's lines cut down to ``<stream> <name>[ M N K]``."""

    def wrap(self, name, fn, skip_self=False):
        def call(*a, **k):
            if self.depth == 0:
                dims = ' %d %d %d' % tuple(a[3:6]) if name == 'gemm' else ''
                self.lines.append('%s %s%s' % (self.stream(), name, dims))
            self.depth += 1
            try:
                return fn(*a, **k)
            finally:
                self.depth -= 1
        return call


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _model(body):
    from asr_study_amd.core import layers as L
    from asr_study_amd.core.models import ctc_model
    x_in = L.Input(name='inputs', shape=(None, F))
    m = ctc_model(x_in, L.TimeDistributed(L.Dense(8))(body(L, x_in)), seed=0)
    m.decoder = None
    return m


def _masks(m, n_pad, rs):
    """{stage: (B_W, B_U)} for every stage whose kind takes masks, on the device."""
    import torch
    from asr_study_amd.core.stages import KINDS
    out = {}
    for si, s in enumerate(m.stages):
        shape = KINDS[s.kind].mask_shape
        if shape is not None:
            out[si] = tuple(
                torch.as_tensor(((rs.rand(*sh) > 0.2) / 0.8).astype(np.float32)).to(m.device)
                for sh in ((2, n_pad, s.f_in_pad), shape(s, n_pad)))
    return out


def record_train(name):
    import torch
    body, steps = TRAIN_CASES[name]
    m = _model(body)
    rs = np.random.RandomState(11)
    out = []
    for T, masks_on in steps:
        slab = m.to_slab(rs.standard_normal((N, T, F)).astype(np.float32))
        n_pad = slab.shape[1]
        masks = _masks(m, n_pad, rs) if masks_on else None
        dl = np.zeros((T, n_pad, 8), np.float32)
        dl[:, :N] = rs.standard_normal((T, N, 8))
        dl = torch.as_tensor(dl).to(m.device)
        rec = Skeleton(m, slab)
        with rec.recording():
            logits = m.forward(slab, training=True, masks=masks, n_real=N)
            m.backward(dl)
        torch.cuda.synchronize()
        bits = {'logits': _sha(logits[:, :N].cpu().numpy())}
        for i, g in enumerate(m.get_gradients()):
            bits['grad%02d' % i] = _sha(g)
        out.append({'T': T, 'masks': masks_on, 'bits': bits, 'calls': rec.lines})
    return out


def record_stream(name):
    m = _model(STREAM_CASES[name])
    x = np.random.RandomState(12).standard_normal((N, 7, F)).astype(np.float32)
    rec = Skeleton(m, None)
    outs = []
    with rec.recording():
        for step in (3, 1):         # (a session runs whole steps: the recurrence sees 3, 3, 1 / 1)
            ss = m.stream(n_streams=N, step=step)
            for pieces in ([3, 3, 1], [1] * 7):
                pos = 0
                for p in pieces:
                    outs.append(ss.feed(x[:, pos:pos + p]))
                    pos += p
                outs.append(ss.finish())
                ss.reset()
    got = np.concatenate(outs, 1)
    assert got.shape == (N, 28, 8), got.shape
    return {'bits': {'logits': _sha(got)}, 'calls': rec.lines}


def record(name):
    return record_train(name) if name in TRAIN_CASES else record_stream(name)


if __name__ == '__main__':
    table = {}
    for name in CASES:
        table[name] = record(name)
        print(name, flush=True)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'rec_bits_parent.json')
    with open(dst, 'w') as f:
        json.dump(table, f, sort_keys=True, indent=0)
        f.write('\n')
