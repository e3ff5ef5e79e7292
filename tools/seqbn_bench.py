#!/usr/bin/env python
"""Sequence-wise batch normalisation measurements (K18, csrc/batchnorm.hip asr_seqbn_*, DESIGN.md
17): prints ONE JSON line with

* microseconds and algorithmic TB/s of each call on the cfg3 GRU projection slab 500 x 64 x 3072,
  with full lengths and with lengths uniform in [250, 500]: forward training (statistics pass +
  finalize + apply: p read twice, zx written once, 3 S bytes for a slab of S bytes), forward
  inference (2 S), backward (reduce pass over p and da, then p, da read and dp written: 5 S; p
  and da each counted once per pass as in tools/bn_bench.py);
* milliseconds per train_step_device of deep_speech2(rnn_type='gru', batch_norm=True) and of
  deep_speech2(rnn_type='gru', batch_norm='recurrent') at the cfg3 geometry (64 x 10 s,
  log-mel-80).  --root DIR imports the package from another checkout (the parent commit's
  baseline; it must have been built), --variants picks the models.

Every measurement runs in a child process under its own time limit (--limit seconds).

    python tools/seqbn_bench.py [--reps 20] [--steps 5] [--warmup 2] [--limit 300]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N, N_PAD, W = 500, 64, 64, 3072
LENS = ('full', 'uniform_250_500')


def _kernel(name, reps):
    import numpy as np
    import torch
    from asr_study_amd import ops
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(T, N_PAD, W, device=dev, generator=g)
    da = torch.randn(T, N_PAD, W, device=dev, generator=g)
    y, dp = torch.empty_like(p), torch.empty_like(p)
    gamma = torch.rand(W, device=dev, generator=g) + 0.5
    beta = torch.randn(W, device=dev, generator=g)
    rm, rv = torch.zeros(W, device=dev), torch.ones(W, device=dev)
    stats = torch.empty(ops.seqbn_stats_len(W), device=dev)
    mom = torch.empty(ops.bn_moments_len(W), device=dev)
    dg, db, mx = (torch.empty(W, device=dev), torch.empty(W, device=dev),
                  torch.empty(1, device=dev))
    lens = np.full(N, T) if name == 'full' else np.random.RandomState(0).randint(250, 501, size=N)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    S = p.numel() * 4
    calls = (('fwd_train', 3, lambda: ops.seqbn_fwd_train(p, y, gamma, beta, stats, N, W,
                                                          lens=lens_d, moments=mom)),
             ('fwd_infer', 2, lambda: ops.seqbn_fwd_infer(p, y, gamma, beta, rm, rv, N, W)),
             ('bwd', 5, lambda: ops.seqbn_bwd(p, da, gamma, stats, dp, dg, N, W, lens=lens_d,
                                              dbeta=db, dp_absmax=mx)))
    out = {'valid_share': round(float(lens.sum()) / (T * N), 3)}
    for cname, k, fn in calls:
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        times.sort()
        us = times[len(times) // 2]
        out[cname] = {'us': round(us, 1), 'us_min': round(times[0], 1), 'us_max': round(times[-1], 1),
                      'alg_bytes': k * S, 'TBps': round(k * S / (us * 1e-6) / 1e12, 2)}
    return out


def _train(variant, steps, warmup):
    import time
    import numpy as np
    import torch
    from asr_study_amd.core import models, optimizers
    bn = {'layer_input': True, 'recurrent': 'recurrent', 'none': False}[variant]
    model = models.deep_speech2(seed=0, rnn_type='gru', batch_norm=bn)
    model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
    n, t = 64, 1000
    rs = np.random.RandomState(0)
    x = rs.randn(n, t, model.num_features).astype(np.float32)
    labels = [rs.randint(1, model.num_classes - 1, size=80) for _ in range(n)]
    slab = model.to_slab(x)
    lab, lab_len, sl = model._prep_labels(labels, np.full(n, t), t)
    for _ in range(warmup):
        model.train_step_device(slab, lab, lab_len, sl, n)
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        t0 = time.time()
        ctc, _, _ = model.train_step_device(slab, lab, lab_len, sl, n)
        torch.cuda.synchronize()
        times.append((time.time() - t0) * 1e3)
    flags = model._flag_snapshot().cpu().numpy()
    assert np.isfinite(ctc.cpu().numpy()).all() and not flags.any(), flags
    return {'ms_per_step': round(sum(times) / len(times), 2),
            'ms_median': round(sorted(times)[len(times) // 2], 2),
            'ms_min': round(min(times), 2), 'ms_max': round(max(times), 2),
            'fallbacks': model.fallbacks}


def _child(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import __graft_entry__ as g
    g.build()
    if args.one[0] == 'kernel':
        res = _kernel(args.one[1], args.reps)
    else:
        res = _train(args.one[1], args.steps, args.warmup)
    print('RESULT ' + json.dumps(res))


def _run(argv, limit):
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, cwd=ROOT,
                           capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return {'error': 'time limit %d s' % limit}, False
    for line in p.stdout.splitlines():
        if line.startswith('RESULT '):
            return json.loads(line[7:]), True
    tail = (p.stderr or '').strip().splitlines()[-3:]
    # a fault / abort / kill ends the run: nothing more is started on the GPU
    return {'error': 'exit %d: %s' % (p.returncode, ' | '.join(tail))}, p.returncode not in (
        -6, -11, 134, 139, -9, 137)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--limit', type=int, default=300)
    ap.add_argument('--no-train', action='store_true', help='kernels only')
    ap.add_argument('--no-kernels', action='store_true', help='train steps only')
    ap.add_argument('--variants', default='layer_input,recurrent',
                    help="models to step: 'layer_input' (batch_norm=True), 'recurrent', 'none'")
    ap.add_argument('--root', default=ROOT, help='checkout to import the package from')
    ap.add_argument('--one', nargs='+', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return _child(args)
    out = {'kernels': {}, 'train': {}}
    go = True
    for name in (() if args.no_kernels else LENS):
        if not go:
            break
        out['kernels'][name], go = _run(['--one', 'kernel', name, '--reps', str(args.reps),
                                         '--root', args.root], args.limit)
    for variant in (() if args.no_train else args.variants.split(',')):
        if not go:
            break
        out['train'][variant], go = _run(['--one', 'train', variant, '--steps', str(args.steps),
                                          '--warmup', str(args.warmup), '--root', args.root],
                                         args.limit)
    a = out['train'].get('recurrent', {}).get('ms_per_step')
    b = out['train'].get('layer_input', {}).get('ms_per_step')
    if a and b:
        out['train']['recurrent_minus_layer_input_ms'] = round(a - b, 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
