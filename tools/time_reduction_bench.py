#!/usr/bin/env python
"""Time-reduction measurements (csrc/timestack.hip, the TimeReduction stage).

    python tools/time_reduction_bench.py kernel   # asr_time_stack_fwd / _bwd beside asr_axpby

    python tools/time_reduction_bench.py steps    # a training step of aed(encoder='blstm') and of
                                                  # transducer(encoder='lstm'), each with and
                                                  # without time_reduction=[[2, 2]], alternating

``kernel`` times each call with device events (median of 5 after 2 of warm-up) on a slab of T = 500
frames, N = 64 utterances, F = 1024 features, k = 2, once with every utterance full and once with
ragged lengths (250 .. 500), beside asr_axpby over the same number of floats.  The stacking calls
read the slab once and write it once (8 bytes per float, the ragged case less on the read side);
asr_axpby reads two operands and writes one (12 bytes per float): the GB/s column counts each
call's own bytes.  It is also the program to put behind ``rocprofv3 --kernel-trace --stats
--output-format csv --`` (a run of its own, no counters).

``steps``: 64 utterances of log-mel-80 frames (250 for aed, 500 for the transducer), 100 labels
each, the factories' default 5 x 512 encoders, Adam with clipnorm 400, 10 steps after 3 of warm-up
per model, each model built twice in alternation."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_study_amd import ops  # noqa: E402
from tools.rnnt_bench import _median_ms  # noqa: E402


def kernel(T=500, N=64, F=1024, k=2):
    dev = 'cuda:0'
    rs = np.random.RandomState(0)
    n_pad = ops.pad16(N)
    To = ops.time_stack_frames(T, k)
    x = torch.randn(T, n_pad, F, device=dev)
    y = torch.empty(To, n_pad, k * F, device=dev)
    dy = torch.randn(To, n_pad, k * F, device=dev)
    dx = torch.empty_like(x)
    a, b, c = torch.randn_like(x), torch.randn_like(x), torch.empty_like(x)
    n = x.numel()
    print('T %d, N %d (n_pad %d), F %d, k %d: %.1f M floats' % (T, N, n_pad, F, k, n / 1e6))
    for tag, lens in (('full', None), ('ragged', rs.randint(T // 2, T + 1, N))):
        ld = None if lens is None else torch.tensor(lens.astype(np.int32), device=dev)
        valid = n if lens is None else int(np.sum(lens)) * F
        calls = [
            ('asr_time_stack_fwd', lambda: ops.time_stack_fwd(x, y, N, F, k, lens=ld),
             4.0 * (valid + To * k * n_pad * F)),
            ('asr_time_stack_bwd', lambda: ops.time_stack_bwd(dy, dx, N, F, k, lens=ld),
             4.0 * (valid + n)),
            ('asr_axpby (same floats)', lambda: ops.axpby(1.0, a, 1.0, b, c), 12.0 * n),
        ]
        print('%s:' % tag)
        for name, fn, nbytes in calls:
            med, lo, hi = _median_ms(fn)
            print('  %-26s median %7.1f us (min %.1f, max %.1f); %.1f MB = %.2f TB/s'
                  % (name, med * 1e3, lo * 1e3, hi * 1e3, nbytes / 1e6, nbytes / med / 1e9),
                  flush=True)


def steps(N=64, F=80, U=100):
    import time
    from asr_study_amd.core import models, optimizers
    rs = np.random.RandomState(5)
    lab = [list(rs.randint(0, 27, size=U)) for _ in range(N)]
    names = (
        ('aed blstm, T 250', 250, lambda: models.aed(encoder='blstm', seed=0)),
        ('aed blstm, T 250, time_reduction [[2, 2]]', 250,
         lambda: models.aed(encoder='blstm', seed=0, time_reduction=[[2, 2]])),
        ('transducer lstm, T 500', 500, lambda: models.transducer(encoder='lstm', seed=0)),
        ('transducer lstm, T 500, time_reduction [[2, 2]]', 500,
         lambda: models.transducer(encoder='lstm', seed=0, time_reduction=[[2, 2]])),
    )
    out = {}
    for name, T, make in names * 2:
        x = np.random.RandomState(T).randn(N, T, F).astype(np.float32)
        lens = np.full(N, T)
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
                                  for n, _, _ in names), flush=True)


if __name__ == '__main__':
    {'kernel': kernel, 'steps': steps}[sys.argv[1]]()
