#!/usr/bin/env python
"""Attention encoder-decoder measurements (csrc/cross_attention.hip, csrc/aed.hip).

    python tools/aed_bench.py kernel   # asr_attn_cross_fwd / _bwd and asr_aed_loss_grad alone

    python tools/aed_bench.py steps    # one training step of aed(encoder='blstm') beside the CTC
                                       # step of the same encoder (brsmv1), alternating

``kernel`` times each call with device events (median of 5 after 2 of warm-up) at N = 64
utterances, Tq = 101 decoder rows (100 labels + EOS), Tk = 250 encoder frames, 4 heads of 64
(d_att 256), C = 29, once with every utterance full and once with ragged lengths (125 .. 250
frames, 40 .. 100 labels), and prints milliseconds with the ALGORITHMIC flops of the attention (4
dh per (query, key) pair forward, 10 dh backward: what one materialised pass would execute) and
of the joint (2 J C per row forward, 6 J C with gradients).  It is also the program to put behind
``rocprofv3 --kernel-trace --stats --output-format csv --`` (a run of its own, no counters).

``steps``: 64 utterances of 250 log-mel-80 frames, 100 labels each, Adam with clipnorm 400, 10
steps after 3 of warm-up per model, each model built twice in alternation; the decoder step is
also timed with its greedy decode for the LER metric taken out (``decode off``)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_study_amd import ops  # noqa: E402
from tools.rnnt_bench import _median_ms  # noqa: E402


def kernel(N=64, Tq=101, Tk=250, heads=4, dh=64, Cc=29):
    dev = 'cuda:0'
    rs = np.random.RandomState(0)
    n_pad, D = ops.pad16(N), heads * dh
    q = torch.randn(Tq, n_pad, D, device=dev)
    kv = torch.randn(Tk, n_pad, 2 * D, device=dev)
    ctx, dout = torch.empty_like(q), torch.randn(Tq, n_pad, D, device=dev)
    lse = torch.empty(ops.attn_lse_len(Tq, n_pad, heads), device=dev)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    W = torch.randn(D, Cc, device=dev) / np.sqrt(D)
    b = torch.zeros(Cc, device=dev)
    labels = torch.tensor(rs.randint(0, Cc - 1, (N, Tq - 1)).astype(np.int32), device=dev)
    grads = [torch.empty_like(q), torch.empty_like(q), torch.empty_like(W), torch.empty_like(b)]
    print('N %d, Tq %d, Tk %d, %d heads of %d, C %d' % (N, Tq, Tk, heads, dh, Cc))
    for tag, kl, ul in (('full', np.full(N, Tk), np.full(N, Tq - 1)),
                        ('ragged', rs.randint(Tk // 2, Tk + 1, N),
                         rs.randint(2 * (Tq - 1) // 5, Tq, N))):
        k_lens = torch.tensor(kl.astype(np.int32), device=dev)
        ll = torch.tensor(ul.astype(np.int32), device=dev)
        q_lens = ll + 1
        pairs = int(np.sum((ul + 1) * kl)) * heads
        rows = int(np.sum(ul + 1))
        calls = [
            ('asr_attn_cross_fwd',
             lambda: ops.attn_cross_fwd(q, kv, ctx, N, heads, dh, q_lens=q_lens, k_lens=k_lens,
                                        lse=lse), 4.0 * dh * pairs),
            ('asr_attn_cross_bwd',
             lambda: ops.attn_cross_bwd(q, kv, ctx, lse, dout, dq, dkv, N, heads, dh,
                                        q_lens=q_lens, k_lens=k_lens), 10.0 * dh * pairs),
            ('asr_aed_loss_grad, loss only',
             lambda: ops.aed_loss_grad(ctx, q, W, b, labels, ll, N), 2.0 * D * Cc * rows),
            ('asr_aed_loss_grad, four gradients',
             lambda: ops.aed_loss_grad(ctx, q, W, b, labels, ll, N, grads=grads,
                                       grad_scale=1.0 / N, eps=0.1), 6.0 * D * Cc * rows),
        ]
        print('%s: %.2f M (query, key, head) pairs, %d decoder rows' % (tag, pairs / 1e6, rows))
        for name, fn, flops in calls:
            med, lo, hi = _median_ms(fn)
            print('  %-36s median %8.3f ms (min %.3f, max %.3f); algorithmic %.2f GFLOP = %.2f '
                  'TFLOP/s' % (name, med, lo, hi, flops / 1e9, flops / med / 1e9), flush=True)


def steps(N=64, T=250, F=80, U=100):
    import time
    from asr_study_amd.core import models, optimizers
    rs = np.random.RandomState(5)
    x = rs.randn(N, T, F).astype(np.float32)
    lab = [list(rs.randint(0, 27, size=U)) for _ in range(N)]
    lens = np.full(N, T)

    def ctc():
        return models.brsmv1(num_features=F, num_hiddens=512, seed=0)

    def aed():
        return models.aed(encoder='blstm', seed=0)

    def aed_plain():
        m = aed()
        empty = (torch.zeros((N, 1), dtype=torch.int32, device=m.device),
                 torch.zeros(N, dtype=torch.int32, device=m.device))
        m._greedy = lambda f, sl, n: empty
        return m
    names = (('brsmv1 5 x 512, CTC step', ctc), ('aed blstm, step', aed),
             ('aed blstm, step, decode off', aed_plain))
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
