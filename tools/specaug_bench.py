#!/usr/bin/env python
"""SpecAugment measurements (csrc/specaug.hip).

    python tools/specaug_bench.py kernels  # asr_specaug_apply with and without the warp, beside
                                           # asr_axpby on the same slab
    python tools/specaug_bench.py steps    # one training step of conformer() with and without
                                           # spec_augment=True, alternating, at the cfg3 input

``kernels`` times each call with device events (median of 20 after 3 of warm-up) on the cfg3 input
slab (T, N, F) = (999, 64, 80), ragged lengths 400 .. 999, and prints microseconds, the slabs of
T N F floats the call has to move (its ALGORITHMIC bytes: one read and one write), the rate that
gives, and the time per slab moved over asr_axpby's (which moves three such slabs: the yardstick
of the same run).  It is also the program to put behind ``rocprofv3 --kernel-trace --stats
--output-format csv --`` (a run of its own, no counters)."""
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


def kernels(T=999, N=64, F=80):
    dev = 'cuda:0'
    rs = np.random.RandomState(0)
    lens = torch.tensor(rs.randint(400, T + 1, size=N).astype(np.int32), device=dev)
    x, z = torch.randn(T, N, F, device=dev), torch.randn(T, N, F, device=dev)
    y = torch.empty_like(x)
    slab = T * N * F * 4
    step = [0]

    def aug(**pol):
        def call():
            step[0] += 1
            ops.specaug_apply(x, y, N, F, 1, 0, step[0], lens=lens, **pol)
        return call
    # (name, call, slabs of T N F floats read + written)
    calls = [
        ('asr_axpby', lambda: ops.axpby(0.5, x, 1.0, z, y), 3),
        ('asr_specaug_apply, masks (defaults)', aug(), 2),
        ('asr_specaug_apply, warp 80 + masks', aug(time_warp=80), 2),
        ('asr_specaug_apply, warp 80 alone', aug(time_warp=80, freq_masks=0, time_masks=0), 2),
        ('asr_specaug_apply, 32 + 32 masks', aug(freq_masks=32, freq_width=2, time_masks=32,
                                                 time_width=10, time_ratio=1.0), 2),
    ]
    print('(T %d, N %d, F %d): one slab = %.1f MB' % (T, N, F, slab / 1e6))
    per_slab = None
    for name, fn, slabs in calls:
        med, lo, hi = _median_us(fn)
        if per_slab is None:
            per_slab = med / slabs
        print('%-36s median %7.1f us (min %.1f, max %.1f); %d slabs = %.1f MB, %.2f TB/s; per '
              'slab %.2f x axpby' % (name, med, lo, hi, slabs, slabs * slab / 1e6,
                                     slabs * slab / med / 1e6, med / slabs / per_slab), flush=True)


def steps():
    from asr_study_amd.core import models, optimizers
    rs = np.random.RandomState(5)
    x = rs.randn(64, 999, 80).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=60)) for _ in range(64)]
    names = ('conformer', 'conformer + spec_augment')
    out = {}
    for name in names * 2:
        model = models.conformer(seed=0, spec_augment=name != 'conformer')
        model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
        slab = model.to_slab(x)
        ts = []
        for i in range(13):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.train_on_batch([('slab', slab), lab, np.full(64, 999)])
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[3:]
        out.setdefault(name, []).append(ts)
        print('%s: median %.2f ms, min %.2f, max %.2f (10 steps after 3 of warm-up); fallbacks %d'
              % (name, np.median(ts), min(ts), max(ts), model.fallbacks), flush=True)
        del model
        torch.cuda.empty_cache()
    med = {n: float(np.median(np.concatenate(out[n]))) for n in names}
    print('medians: %s; with / without = %.4f, difference %.3f ms'
          % (', '.join('%s %.2f ms' % (n, med[n]) for n in names),
             med[names[1]] / med[names[0]], med[names[1]] - med[names[0]]), flush=True)


if __name__ == '__main__':
    {'kernels': kernels, 'steps': steps}[sys.argv[1]]()
