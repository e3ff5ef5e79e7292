#!/usr/bin/env python
"""Conformer measurements (csrc/dwconv.hip).

    python tools/conformer_bench.py kernels  # asr_dwconv1d_fwd / _bwd, GLU, Swish beside asr_axpby
    python tools/conformer_bench.py steps    # one training step of conformer(), transformer() and
                                             # deep_speech2(), alternating, at the cfg3 input

``kernels`` times each call with device events (median of 20 after 3 of warm-up) on the slab
(T, N, C) = (500, 64, 256), k = 31, ragged lengths 200 .. 500, and prints microseconds, the slabs
of T N C floats the call has to move (its ALGORITHMIC bytes), the rate that gives, and the time
per slab moved over asr_axpby's (which moves three such slabs: the yardstick of the same run).
It is also the program to put behind ``rocprofv3 --kernel-trace --stats --output-format csv --``
(a run of its own, no counters)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_study_amd import ops  # noqa: E402


def _median_us(fn, reps=20, warm=3):
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
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernels(T=500, N=64, C=256, k=31):
    dev = 'cuda:0'
    rs = np.random.RandomState(0)
    lens = torch.tensor(rs.randint(200, T + 1, size=N).astype(np.int32), device=dev)
    x, dy = torch.randn(T, N, C, device=dev), torch.randn(T, N, C, device=dev)
    x2 = torch.randn(T, N, 2 * C, device=dev)
    y, dx, dx2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x2)
    w, b = torch.randn(k, C, device=dev) * 0.2, torch.randn(C, device=dev)
    dw, db = torch.empty_like(w), torch.empty_like(b)
    slab = T * N * C * 4
    # (name, call, slabs of T N C floats read + written)
    calls = [
        ('asr_axpby', lambda: ops.axpby(0.5, x, 1.0, dy, y), 3),
        ('asr_dwconv1d_fwd', lambda: ops.dwconv1d_fwd(x, w, b, y, N, k, lens=lens), 2),
        ('asr_dwconv1d_bwd', lambda: ops.dwconv1d_bwd(x, w, dy, dx, dw, db, N, k, lens=lens), 3),
        ('asr_dwconv1d_bwd, no dx', lambda: ops.dwconv1d_bwd(x, w, dy, None, dw, db, N, k,
                                                             lens=lens), 2),
        ('asr_glu_fwd', lambda: ops.glu_fwd(x2, y), 3),
        ('asr_glu_bwd', lambda: ops.glu_bwd(x2, dy, dx2), 5),
        ('asr_swish_fwd', lambda: ops.swish_fwd(x, y), 2),
        ('asr_swish_bwd', lambda: ops.swish_bwd(x, dy, dx), 3),
    ]
    plan = ops.dwconv1d_plan(T, N, C, k, N=N), ops.dwconv1d_plan(T, N, C, k, N=N, backward=True)
    print('(T %d, N %d, C %d, k %d): forward %s, weight gradient %s' % ((T, N, C, k) + plan))
    per_slab = None
    for name, fn, slabs in calls:
        med, lo, hi = _median_us(fn)
        if per_slab is None:
            per_slab = med / slabs
        print('%-26s median %7.1f us (min %.1f, max %.1f); %d slabs = %.1f MB, %.2f TB/s; per slab '
              '%.2f x axpby' % (name, med, lo, hi, slabs, slabs * slab / 1e6,
                                slabs * slab / med / 1e6, med / slabs / per_slab), flush=True)


def steps():
    from asr_study_amd.core import models, optimizers
    rs = np.random.RandomState(5)
    x = rs.randn(64, 1000, 80).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=60)) for _ in range(64)]
    names = ('conformer', 'transformer', 'deep_speech2')
    out = {}
    for name in names * 2:
        model = getattr(models, name)(seed=0)
        model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
        slab = model.to_slab(x)
        ts = []
        for i in range(13):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.train_on_batch([('slab', slab), lab, np.full(64, 1000)])
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[3:]
        out.setdefault(name, []).append(ts)
        print('%s (%d parameters): median %.2f ms, min %.2f, max %.2f (10 steps after 3 of '
              'warm-up); fallbacks %d' % (name, model.count_params(), np.median(ts), min(ts),
                                          max(ts), model.fallbacks), flush=True)
        del model
        torch.cuda.empty_cache()
    med = {n: float(np.median(np.concatenate(out[n]))) for n in names}
    print('medians: %s; conformer / transformer = %.3f, conformer / deep_speech2 = %.3f'
          % (', '.join('%s %.2f ms' % (n, med[n]) for n in names),
             med['conformer'] / med['transformer'], med['conformer'] / med['deep_speech2']),
          flush=True)


if __name__ == '__main__':
    {'kernels': kernels, 'steps': steps}[sys.argv[1]]()
