#!/usr/bin/env python
"""Self-attention measurements (csrc/attention.hip).

    python tools/attn_bench.py kernels  # asr_attn_fwd / asr_attn_bwd alone, and asr_relattn_fwd /
                                        # asr_relattn_bwd beside them
    python tools/attn_bench.py steps    # one training step of transformer() beside deep_speech2()
                                        # (the cfg3 BiLSTM), alternating, at the cfg3 input
    python tools/attn_bench.py relative_steps   # conformer(positions='relative') beside
                                        # conformer(), alternating, at the cfg3 input

``kernels`` times each call with device events (median of 20 after 3 of warm-up) at
(T, N, heads, dh) = (500, 64, 4, 64) and (1000, 64, 4, 64), every key visible, and prints
milliseconds, the ALGORITHMIC rate (forward 4 T^2 D flops per sample, backward 10 T^2 D: the
scores once, dP, dV, dQ, dK), the EXECUTED rate (the backward computes the scores and dP in both of
its passes: 14 T^2 D; tiles are whole, so T rounds up to the tile) and the executed rate over the
fp32 peak (157.3 TFLOP/s, vector FMA and fp32 MFMA alike).  It is also the program to put behind
``rocprofv3 --kernel-trace --stats --output-format csv --`` (a run of its own, no counters)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_study_amd import ops  # noqa: E402

PEAK_FP32 = 157.3e12


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


def kernels():
    dev = 'cuda:0'
    for T, N, heads, dh in ((500, 64, 4, 64), (1000, 64, 4, 64)):
        D = heads * dh
        qkv = torch.randn(T, N, 3 * D, device=dev)
        dout = torch.randn(T, N, D, device=dev)
        out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
        lse = torch.empty(ops.attn_lse_len(T, N, heads), device=dev)
        plan = ops.attn_plan(T, N, heads, dh)
        Tt = -(-T // plan['bq']) * plan['bq']
        fwd = _median_us(lambda: ops.attn_fwd(qkv, out, N, heads, dh, lse=lse))
        bwd = _median_us(lambda: ops.attn_bwd(qkv, out, lse, dout, dqkv, N, heads, dh))
        # the relative calls on the same qkv: forward 6 T^2 D algorithmic (the
        # relative term is a second score product) and 8 executed (the band product is 64 x 128
        # per tile pair, half of it falls outside the tile); backward 16 T^2 D algorithmic (+ the
        # relative score term once, dS Pos, dS^T Q') and 42 executed (its three passes: 14 + 12 +
        # 16; half of the third pass's products fall outside its band tile)
        pos = torch.randn(2 * T - 1, D, device=dev)
        bu, bv = torch.randn(D, device=dev) * 0.5, torch.randn(D, device=dev) * 0.5
        dpos, dbu, dbv = torch.empty_like(pos), torch.empty_like(bu), torch.empty_like(bv)
        rfwd = _median_us(lambda: ops.relattn_fwd(qkv, pos, bu, bv, out, N, heads, dh, lse=lse))
        rbwd = _median_us(lambda: ops.relattn_bwd(qkv, pos, bu, bv, out, lse, dout, dqkv, dpos,
                                                  dbu, dbv, N, heads, dh))
        print('(T %d) relative / plain: forward %.2f, backward %.2f'
              % (T, rfwd[0] / fwd[0], rbwd[0] / bwd[0]), flush=True)
        for name, (med, lo, hi), alg, exe in (
                ('fwd', fwd, 4.0 * T * T * D * N, 4.0 * Tt * Tt * D * N),
                ('bwd', bwd, 10.0 * T * T * D * N, 14.0 * Tt * Tt * D * N),
                ('relative fwd', rfwd, 6.0 * T * T * D * N, 8.0 * Tt * Tt * D * N),
                ('relative bwd', rbwd, 16.0 * T * T * D * N, 42.0 * Tt * Tt * D * N)):
            print('(T %d, N %d, heads %d, dh %d) %s: median %.3f ms (min %.3f, max %.3f); '
                  'algorithmic %.1f TFLOP/s, executed %.1f TFLOP/s = %.1f %% of the fp32 peak'
                  % (T, N, heads, dh, name, med / 1e3, lo / 1e3, hi / 1e3, alg / med / 1e6,
                     exe / med / 1e6, 100.0 * exe / (med * 1e-6) / PEAK_FP32), flush=True)


def steps():
    from asr_study_amd.core import models, optimizers
    rs = np.random.RandomState(5)
    x = rs.randn(64, 1000, 80).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=60)) for _ in range(64)]
    out = {}
    for name in ('transformer', 'deep_speech2', 'transformer', 'deep_speech2'):
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
    tr = np.median(np.concatenate(out['transformer']))
    ds = np.median(np.concatenate(out['deep_speech2']))
    print('transformer / deep_speech2 = %.3f (medians %.2f / %.2f ms)' % (tr / ds, tr, ds),
          flush=True)


def relative_steps():
    """One training step of conformer(positions='relative') beside conformer(), alternating twice
    in one process, at the cfg3 input (the method of ``steps``)."""
    from asr_study_amd.core import models, optimizers
    rs = np.random.RandomState(5)
    x = rs.randn(64, 1000, 80).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=60)) for _ in range(64)]
    out = {}
    for positions in ('relative', 'absolute', 'relative', 'absolute'):
        model = models.conformer(positions=positions, seed=0)
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
        out.setdefault(positions, []).append(ts)
        print('conformer(positions=%r) (%d parameters): median %.2f ms, min %.2f, max %.2f (10 '
              'steps after 3 of warm-up); fallbacks %d'
              % (positions, model.count_params(), np.median(ts), min(ts), max(ts),
                 model.fallbacks), flush=True)
        del model
        torch.cuda.empty_cache()
    rel = np.median(np.concatenate(out['relative']))
    ab = np.median(np.concatenate(out['absolute']))
    print('relative / absolute = %.3f (medians %.2f / %.2f ms)' % (rel / ab, rel, ab), flush=True)


if __name__ == '__main__':
    {'kernels': kernels, 'steps': steps, 'relative_steps': relative_steps}[sys.argv[1]]()
