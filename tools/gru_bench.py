#!/usr/bin/env python
"""GRU measurements (csrc/gru.hip): prints ONE JSON line with

* forward and BPTT microseconds per step of the stepwise form (the only one) at (H, n_pad, T) =
  (512, 64, 500) and (1024, 64, 500), with the bytes and FLOPs a step moves beside them;
* milliseconds per train_step_device of deep_speech2 at its defaults (cfg3 geometry: 64 x 10 s,
  80 log-mel, 5 x 512) with rnn_type='gru' and with rnn_type='lstm'.

Every measurement runs in a child process under its own time limit (--limit seconds).

    python tools/gru_bench.py [--reps 5] [--steps 5] [--warmup 2] [--limit 300]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(512, 64, 500), (1024, 64, 500)]


def step_cost(H, n_pad):
    """(FLOPs, bytes) of one step of both directions, forward and BPTT: three H x H products
    per direction each way; U (or U^T) is read once per batch tile, the slabs once."""
    NR = 64 if n_pad % 64 == 0 else 32 if n_pad % 32 == 0 else 16
    flops = 2 * 2 * n_pad * H * 3 * H
    u_bytes = 2 * (n_pad // NR) * 3 * H * H * 4
    fwd_slabs = 2 * n_pad * H * 4 * (3 + 1 + 3 + 1 + 1 + 1)     # zx, h_prev, gates, rm w+r, h
    bwd_slabs = 2 * n_pad * H * 4 * (1 + 3 + 2 + 3 + 3 + 4)     # dy, gates, h, da w, da r, g/qr
    return {'flops': flops, 'fwd_bytes': u_bytes + fwd_slabs, 'bwd_bytes': u_bytes + bwd_slabs}


def _kernel(H, n_pad, T, mode, reps):
    import torch
    from asr_study_amd import ops
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    U = torch.randn(2, H, 3 * H, device=dev, generator=g) * (0.5 / H ** 0.5)
    zx = torch.randn(T, n_pad, 2, 3 * H, device=dev, generator=g)
    h = torch.empty(T, n_pad, 2, H, device=dev)
    gates = torch.empty(T, n_pad, 2, 3 * H, device=dev)
    rm = torch.empty(T, n_pad, 2, H, device=dev)
    dy = torch.randn(T, n_pad, 2 * H, device=dev, generator=g)
    da = torch.empty(T, n_pad, 2, 3 * H, device=dev)
    dbp = torch.empty(n_pad // 16, 2, 3 * H, device=dev)
    zmx = torch.empty(1, device=dev)
    out = dict(step_cost(H, n_pad))
    for name, fn in (('fwd', lambda: ops.gru_seq_fwd(zx, U, h, gates, rm, T, n_pad, H, mode=mode)),
                     ('bwd', lambda: ops.gru_seq_bwd(dy, U, h, gates, da, T, n_pad, H, mode=mode,
                                                     db_part=dbp, dz_absmax=zmx))):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / T)
        times.sort()
        us = times[len(times) // 2]
        out[name + '_us_per_step'] = round(us, 3)
        out[name + '_us_per_step_min'] = round(times[0], 3)
        out[name + '_us_per_step_max'] = round(times[-1], 3)
        out[name + '_tflops'] = round(out['flops'] / us * 1e-6, 2)
        out[name + '_tb_per_s'] = round(out[name + '_bytes'] / us * 1e-6, 3)
    return out


def _train(rnn_type, steps, warmup):
    import time
    import numpy as np
    import torch
    from asr_study_amd.core import models, optimizers
    model = models.deep_speech2(seed=0, rnn_type=rnn_type)
    model.compile(optimizer=optimizers.Adam(lr=1e-4, clipnorm=400))
    N, T = 64, 1000
    rs = np.random.RandomState(0)
    x = rs.randn(N, T, model.num_features).astype(np.float32)
    labels = [rs.randint(1, model.num_classes - 1, size=60) for _ in range(N)]
    slab = model.to_slab(x)
    lab, lab_len, sl = model._prep_labels(labels, np.full(N, T), T)
    for _ in range(warmup):
        model.train_step_device(slab, lab, lab_len, sl, N)
    torch.cuda.synchronize()
    each = []
    for _ in range(steps):
        t0 = time.time()
        ctc, _, _ = model.train_step_device(slab, lab, lab_len, sl, N)
        torch.cuda.synchronize()
        each.append((time.time() - t0) * 1e3)
    ms = sorted(each)[len(each) // 2]
    flags = model._flag_snapshot().cpu().numpy()
    assert np.isfinite(ctc.cpu().numpy()).all() and not flags.any(), flags
    return {'ms_per_step': round(ms, 2), 'ms_min': round(min(each), 2),
            'ms_max': round(max(each), 2), 'fallbacks': model.fallbacks}


def _child(args):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    if args.one[0] == 'plan':
        from asr_study_amd import ops
        res = {'H%d_n%d_T%d' % (H, n, T): ops.gru_plan(T, n, H) for H, n, T in SHAPES}
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
        for mode, form in ((1, 'stepwise'),):
            if not go:
                break
            row[form], go = _run(['--one', 'kernel', str(H), str(n_pad), str(T), str(mode),
                                  '--reps', str(args.reps)], args.limit)
        out['kernels'][key] = row
    if go:
        out['plan'], go = _run(['--one', 'plan'], args.limit)
    for rnn_type in ('gru', 'lstm'):
        if not go:
            break
        out['train'][rnn_type], go = _run(['--one', 'train', rnn_type, '--steps', str(args.steps),
                                           '--warmup', str(args.warmup)], args.limit)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
