#!/usr/bin/env python
"""SimpleRNN measurements (csrc/rnn.hip): prints ONE JSON line with

* forward and BPTT microseconds per step of both launch forms (stepwise / persistent) at
  (H, n_pad, T) = (2048, 64, 1000) and (1824, 64, 1000), and the form the plan picks there;
* milliseconds per train_step_device of deep_speech and maas at their defaults on 64 x 10 s
  utterances (1000 frames, 81 features).

Every measurement runs in a child process under its own time limit (--limit seconds).

    python tools/rnn_bench.py [--reps 5] [--steps 5] [--warmup 2] [--limit 300]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2048, 64, 1000), (1824, 64, 1000)]


def _kernel(H, n_pad, T, mode, reps):
    import torch
    from asr_study_amd import ops
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    U = torch.randn(2, H, H, device=dev, generator=g) * (0.5 / H ** 0.5)
    zx = torch.randn(T, n_pad, 2, H, device=dev, generator=g)
    h = torch.empty(T, n_pad, 2, H, device=dev)
    dy = torch.randn(T, n_pad, H, device=dev, generator=g)
    dz = torch.empty(T, n_pad, 2, H, device=dev)
    dbp = torch.empty(n_pad // 16, 2, H, device=dev)
    zmx = torch.empty(1, device=dev)
    act = ('clipped_relu', 20.0)
    out = {}
    for name, fn in (('fwd', lambda: ops.rnn_seq_fwd(zx, U, h, T, n_pad, H, act=act, mode=mode)),
                     ('bwd', lambda: ops.rnn_seq_bwd(dy, U, h, dz, T, n_pad, H, act=act,
                                                     shared_dy=True, mode=mode, db_part=dbp,
                                                     dz_absmax=zmx))):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ws = fn()
            e1.record()
            torch.cuda.synchronize()
            ops.lstm_status(ws)
            times.append(e0.elapsed_time(e1) * 1e3 / T)
        times.sort()
        out[name + '_us_per_step'] = round(times[len(times) // 2], 3)
        out[name + '_us_per_step_min'] = round(times[0], 3)
    return out


def _train(factory, steps, warmup):
    import time
    import numpy as np
    import torch
    from asr_study_amd.core import models, optimizers
    model = getattr(models, factory)(seed=0)
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
    if args.one[0] == 'plan':
        from asr_study_amd import ops
        res = {'H%d_n%d_T%d' % (H, n, T): ops.rnn_plan(T, n, H) for H, n, T in SHAPES}
    elif args.one[0] == 'kernel':
        H, n_pad, T, mode = (int(v) for v in args.one[1:])
        res = _kernel(H, n_pad, T, mode, args.reps)
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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--limit', type=int, default=300)
    ap.add_argument('--one', nargs='+', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return _child(args)
    sys.path.insert(0, ROOT)
    out = {'kernels': {}, 'train': {}}
    go = True
    for H, n_pad, T in SHAPES:
        key = 'H%d_n%d_T%d' % (H, n_pad, T)
        row = {}
        for mode, form in ((1, 'stepwise'), (2, 'persistent')):
            if not go:
                break
            row[form], go = _run(['--one', 'kernel', str(H), str(n_pad), str(T), str(mode),
                                  '--reps', str(args.reps)], args.limit)
        out['kernels'][key] = row
    if go:
        out['plan'], go = _run(['--one', 'plan'], args.limit)
    for factory in ('deep_speech', 'maas'):
        if not go:
            break
        out['train'][factory], go = _run(['--one', 'train', factory, '--steps', str(args.steps),
                                          '--warmup', str(args.warmup)], args.limit)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
