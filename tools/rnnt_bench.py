#!/usr/bin/env python
"""Transducer measurements (csrc/rnnt.hip).

    python tools/rnnt_bench.py kernel   # asr_rnnt_loss_grad alone, loss only and with gradients,
                                        # beside asr_ctc_loss_grad on the same frames

    python tools/rnnt_bench.py steps    # one training step of transducer(encoder='gru') beside the
                                        # CTC step of the same encoder, alternating

``steps``: 64 utterances of 999 log-mel-80 frames (500 strided frames behind the two convolutions),
100 labels each, Adam with clipnorm 400, 10 steps after 3 of warm-up per model, each model built
twice in alternation; the transducer step is also timed with its greedy decode for the LER metric
taken out (``decode off``), to show what the loss and the second tower cost by themselves.

``kernel`` times each call with device events (median of 5 after 2 of warm-up) at the project's
workload, N = 64 utterances, T = 500 strided frames, U = 100 labels, J = 512, C = 29, once with
every utterance full and once with ragged lengths (250 .. 500 frames, 40 .. 100 labels), and
prints milliseconds, the workspace, the lattice cells, the ALGORITHMIC flops (the joint forward
2 J C per cell, its backward 4 J C: what one materialised pass would execute) with the rate that
gives, and the flops the three recomputing phases execute (the joint product six times over).  It
is also the program to put behind ``rocprofv3 --kernel-trace --stats --output-format csv --`` (a
run of its own, no counters) for the time of each phase."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_study_amd import _lib, ops  # noqa: E402


def _median_ms(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernel(N=64, T=500, U=100, J=512, Cc=29):
    dev = 'cuda:0'
    rs = np.random.RandomState(0)
    n_pad = ops.pad16(N)
    enc = torch.randn(T, n_pad, J, device=dev)
    pred = torch.randn(U + 1, n_pad, J, device=dev)
    W = torch.randn(J, Cc, device=dev) / np.sqrt(J)
    b = torch.zeros(Cc, device=dev)
    labels = torch.tensor(rs.randint(0, Cc - 1, (N, U)).astype(np.int32), device=dev)
    grads = [torch.empty_like(enc), torch.empty_like(pred), torch.empty_like(W),
             torch.empty_like(b)]
    logits = torch.randn(T, n_pad, Cc, device=dev)
    dlogits = torch.empty_like(logits)
    ws = _lib.load().asr_rnnt_workspace_bytes(T, U + 1, N, n_pad, J, Cc)
    print('N %d, T %d, U %d, J %d, C %d: workspace %.1f MB (the joint\'s hidden tensor would be '
          '%.2f GB)' % (N, T, U, J, Cc, ws / 1e6, N * T * (U + 1) * J * 4 / 1e9))
    for tag, tl, ul in (('full', np.full(N, T), np.full(N, U)),
                        ('ragged', rs.randint(T // 2, T + 1, N), rs.randint(2 * U // 5, U + 1, N))):
        sl = torch.tensor(tl.astype(np.int32), device=dev)
        ll = torch.tensor(ul.astype(np.int32), device=dev)
        cells = int(np.sum(tl * (ul + 1)))
        algo = 6.0 * J * Cc * cells
        calls = [
            ('asr_ctc_loss_grad (T, N, C) logits',
             lambda: ops.ctc_loss_grad(logits, labels, ll, sl, N, grad=dlogits), None),
            ('asr_rnnt_loss_grad, loss only',
             lambda: ops.rnnt_loss_grad(enc, pred, W, b, labels, ll, sl, N, J), 2.0 * J * Cc * cells),
            ('asr_rnnt_loss_grad, four gradients',
             lambda: ops.rnnt_loss_grad(enc, pred, W, b, labels, ll, sl, N, J, grads=grads,
                                        grad_scale=1.0 / N), algo),
        ]
        print('%s: %.2f M lattice cells' % (tag, cells / 1e6))
        for name, fn, flops in calls:
            med, lo, hi = _median_ms(fn)
            extra = ''
            if flops:
                extra = '; algorithmic %.1f GFLOP = %.1f TFLOP/s' % (flops / 1e9, flops / med / 1e9)
                if flops == algo:
                    extra += ', executed %.1f GFLOP' % (2 * algo / 1e9)
            print('  %-38s median %8.3f ms (min %.3f, max %.3f)%s' % (name, med, lo, hi, extra),
                  flush=True)


def steps(N=64, T=999, F=80, U=100):
    import time
    from asr_study_amd.core import models, optimizers
    rs = np.random.RandomState(5)
    x = rs.randn(N, T, F).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=U)) for _ in range(N)]
    lens = np.full(N, T)

    def ctc():
        return models.deep_speech2(rnn_type='gru', bidirectional=False, seed=0)

    def rnnt():
        return models.transducer(encoder='gru', seed=0)

    def rnnt_plain():
        m = rnnt()
        empty = (torch.zeros((N, 1), dtype=torch.int32, device=m.device),
                 torch.zeros(N, dtype=torch.int32, device=m.device))
        m._greedy = lambda f, sl, n: empty
        return m
    names = (('deep_speech2 gru uni, CTC step', ctc), ('transducer gru, step', rnnt),
             ('transducer gru, step, decode off', rnnt_plain))
    out = {}
    for name, make in names * 2:
        model = make()
        model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
        slab = model.to_slab(x)
        ts = []
        for i in range(13):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.train_on_batch([('slab', slab), lab, lens])
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out.setdefault(name, []).append(ts[3:])
        print('%s: median %.2f ms, min %.2f, max %.2f (10 steps after 3 of warm-up)'
              % (name, np.median(ts[3:]), min(ts[3:]), max(ts[3:])), flush=True)
        del model
        torch.cuda.empty_cache()
    print('medians: ' + ', '.join('%s %.2f ms' % (n, float(np.median(np.concatenate(out[n]))))
                                  for n, _ in names), flush=True)


if __name__ == '__main__':
    {'kernel': kernel, 'steps': steps}[sys.argv[1]]()
