#!/usr/bin/env python
"""LayerNormalization measurements (csrc/layernorm.hip).

    python tools/ln_bench.py kernels    # asr_ln_fwd / asr_ln_bwd beside asr_bn_fwd_train / asr_bn_bwd
    python tools/ln_bench.py steps      # step time of deep_speech2(batch_norm='layer') over
                                        # deep_speech2(batch_norm=True), alternating, at cfg3 geometry

``kernels`` times every call with device events (median of 20 after 3 of warm-up) at the cfg3
slabs of 500 x 64 rows, width 1280 (the conv image) and 1024 (in front of a recurrent layer), and
prints microseconds and TB/s of ALGORITHMIC bytes (LN forward 2 S, backward 3 S; BN forward 3 S,
backward 5 S for a slab of S bytes).  It is also the program to put behind
``rocprofv3 --kernel-trace --stats --output-format csv --`` (a run of its own, no counters) for the
per-kernel figures of profiles/k20_ln_vs_bn_kernel_stats.md."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_study_amd import ops  # noqa: E402


def kernels():
    dev = 'cuda:0'
    T, N, n_pad = 500, 64, 64
    for ld in (1280, 1024):
        x = torch.randn(T, n_pad, ld, device=dev)
        dy = torch.randn(T, n_pad, ld, device=dev)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        g, b = torch.rand(ld, device=dev) + 0.5, torch.randn(ld, device=dev)
        dg, db = torch.empty(ld, device=dev), torch.empty(ld, device=dev)
        st = torch.empty(ops.ln_stats_len(T, n_pad), device=dev)
        bst = torch.empty(ops.bn_stats_len(ld), device=dev)
        mom = torch.empty(ops.bn_moments_len(ld), device=dev)
        res = {}
        for name, fn in (
                ('ln_fwd', lambda: ops.ln_fwd(x, y, g, b, N, ld, ld, 1, 1e-5, stats=st)),
                ('ln_bwd', lambda: ops.ln_bwd(x, dy, g, st, dx, dg, db, N, ld, ld, 1)),
                ('bn_fwd_train', lambda: ops.bn_fwd_train(x, y, g, b, bst, N, ld, ld, 1e-3, 0.0,
                                                          moments=mom, weight=float(N * T))),
                ('bn_bwd', lambda: ops.bn_bwd(x, dy, g, b, bst, dx, dg, db, N, ld, ld, 0.0))):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            res[name] = float(np.median(ts))
        S = T * n_pad * ld * 4
        byts = {'ln_fwd': 2 * S, 'ln_bwd': 3 * S, 'bn_fwd_train': 3 * S, 'bn_bwd': 5 * S}
        print('width %d: ' % ld + '; '.join('%s %.1f us %.2f TB/s' % (k, v, byts[k] / v / 1e6)
                                            for k, v in res.items()), flush=True)


def steps():
    from asr_study_amd.core import models, optimizers
    rs = np.random.RandomState(5)
    x = rs.randn(64, 1000, 80).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=60)) for _ in range(64)]
    out = {}
    for name, kw in (('bn', dict(batch_norm=True)), ('ln', dict(batch_norm='layer')),
                     ('bn', dict(batch_norm=True)), ('ln', dict(batch_norm='layer'))):
        model = models.deep_speech2(seed=0, **kw)
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
        print('%s: median %.2f ms, min %.2f, max %.2f (10 steps after 3 of warm-up); fallbacks %d'
              % (name, np.median(ts), min(ts), max(ts), model.fallbacks), flush=True)
        del model
        torch.cuda.empty_cache()
    bn = np.median(np.concatenate(out['bn']))
    ln = np.median(np.concatenate(out['ln']))
    print('ratio ln / bn = %.3f (medians %.2f / %.2f ms)' % (ln / bn, ln, bn), flush=True)


if __name__ == '__main__':
    {'kernels': kernels, 'steps': steps}[sys.argv[1]]()
