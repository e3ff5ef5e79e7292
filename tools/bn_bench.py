#!/usr/bin/env python
"""BatchNormalization measurements (csrc/batchnorm.hip): prints ONE JSON line with

* microseconds and algorithmic TB/s of each BN call at the cfg3 sizes -- the 500 x 64 x (40 * 32)
  conv map per channel, the 500 x 64 x 1280 flattened input and the 500 x 64 x 1024 BiLSTM
  outputs: forward training (statistics pass + finalize + apply: x read twice, y written once,
  3 S bytes for a slab of S bytes), forward inference (2 S), backward (reduce pass over x and dy,
  then x, dy read and dx written: 5 S), each plain and with the fused clipped ReLU;
* milliseconds per train_step_device of deep_speech2(batch_norm=True) and deep_speech2() at the
  cfg3 geometry (64 x 10 s, log-mel-80).

Every measurement runs in a child process under its own time limit (--limit seconds).

    python tools/bn_bench.py [--reps 20] [--steps 5] [--warmup 2] [--limit 300]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (T, N, n_pad, ld, C)
SHAPES = {'conv_map_500x64x40x32': (500, 64, 64, 1280, 32),
          'input_500x64x1280': (500, 64, 64, 1280, 1280),
          'bilstm_500x64x1024': (500, 64, 64, 1024, 1024)}


def _kernel(name, reps):
    import torch
    from asr_study_amd import ops
    T, N, n_pad, ld, C = SHAPES[name]
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(T, n_pad, ld, device=dev, generator=g)
    dy = torch.randn(T, n_pad, ld, device=dev, generator=g)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    gamma = torch.rand(C, device=dev, generator=g) + 0.5
    beta = torch.randn(C, device=dev, generator=g)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    stats = torch.empty(ops.bn_stats_len(C), device=dev)
    mom = torch.empty(ops.bn_moments_len(C), device=dev)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    S = x.numel() * 4
    out = {}
    for clip in (0.0, 20.0):
        calls = (('fwd_train', 3, lambda: ops.bn_fwd_train(x, y, gamma, beta, stats, N, ld, C,
                                                           clip=clip, moments=mom,
                                                           weight=float(N * T))),
                 ('fwd_infer', 2, lambda: ops.bn_fwd_infer(x, y, gamma, beta, rm, rv, N, ld, C,
                                                           clip=clip)),
                 ('bwd', 5, lambda: ops.bn_bwd(x, dy, gamma, beta, stats, dx, dg, db, N, ld, C,
                                               clip=clip)))
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
            key = cname + ('_clip' if clip > 0 else '')
            out[key] = {'us': round(us, 1), 'us_min': round(times[0], 1),
                        'alg_bytes': k * S, 'TBps': round(k * S / (us * 1e-6) / 1e12, 2)}
    return out


def _train(batch_norm, steps, warmup):
    import time
    import numpy as np
    import torch
    from asr_study_amd.core import models, optimizers
    model = models.deep_speech2(seed=0, batch_norm=bool(batch_norm))
    model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
    N, T = 64, 1000
    rs = np.random.RandomState(0)
    x = rs.randn(N, T, model.num_features).astype(np.float32)
    labels = [rs.randint(1, model.num_classes - 1, size=80) for _ in range(N)]
    slab = model.to_slab(x)
    lab, lab_len, sl = model._prep_labels(labels, np.full(N, T), T)
    for _ in range(warmup):
        model.train_step_device(slab, lab, lab_len, sl, N)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(steps):
        ctc, _, _ = model.train_step_device(slab, lab, lab_len, sl, N)
    torch.cuda.synchronize()
    ms = (time.time() - t0) * 1e3 / steps
    flags = model._flag_snapshot().cpu().numpy()
    assert np.isfinite(ctc.cpu().numpy()).all() and not flags.any(), flags
    return {'ms_per_step': round(ms, 2), 'fallbacks': model.fallbacks}


def _child(args):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    if args.one[0] == 'kernel':
        res = _kernel(args.one[1], args.reps)
    else:
        res = _train(int(args.one[1]), args.steps, args.warmup)
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
    ap.add_argument('--one', nargs='+', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return _child(args)
    out = {'kernels': {}, 'train': {}}
    go = True
    for name in SHAPES:
        if not go:
            break
        out['kernels'][name], go = _run(['--one', 'kernel', name, '--reps', str(args.reps)],
                                        args.limit)
    for bn in ((1, 0) if not args.no_train else ()):
        if not go:
            break
        key = 'deep_speech2_bn' if bn else 'deep_speech2'
        out['train'][key], go = _run(['--one', 'train', str(bn), '--steps', str(args.steps),
                                      '--warmup', str(args.warmup)], args.limit)
    if 'deep_speech2_bn' in out['train'] and 'ms_per_step' in out['train'].get('deep_speech2', {}):
        a, b = out['train']['deep_speech2_bn'].get('ms_per_step'), out['train']['deep_speech2'][
            'ms_per_step']
        if a:
            out['train']['bn_overhead_pct'] = round(100.0 * (a - b) / b, 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
