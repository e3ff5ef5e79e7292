#!/usr/bin/env python
"""RHN measurements (csrc/rhn.hip): prints ONE JSON line with

* forward and BPTT microseconds per MICRO-step (one level of one frame, i.e. one launch) of the
  stepwise form (the only one) at (H, n_pad, T) = (512, 64, 500) and (1024, 64, 500), depth 2,
  coupled and uncoupled: the median of --reps calls with their min and max, and the bytes and
  FLOPs a micro-step moves beside them;
* milliseconds per train_step_device of rhn(num_hiddens=512, depth=2) and of brsmv1 at the same
  width on 64 x 10 s of 80 log-mel features.

Every measurement runs in a child process under its own time limit (--limit seconds).

    python tools/rhn_bench.py [--reps 5] [--steps 5] [--warmup 2] [--limit 300]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(512, 64, 500), (1024, 64, 500)]
DEPTH = 2


def step_cost(H, n_pad, C):
    """(FLOPs, bytes) of one micro-step of both directions, forward and BPTT: C H x H products per
    direction each way; U_l (or U_l^T) is read once per batch tile, the slabs once."""
    NR = 64 if n_pad % 64 == 0 else 32 if n_pad % 32 == 0 else 16
    flops = 2 * 2 * n_pad * H * C * H
    u_bytes = 2 * (n_pad // NR) * C * H * H * 4
    # forward: the state read twice (operand, carry), zx at level 0 (averaged in: 1 / depth of
    # the launches), gates and state written
    fwd_slabs = 2 * n_pad * H * 4 * (2 + C / float(DEPTH) + C + 1)
    # BPTT: da read (operand), g read + written, the carry gate, the level below's gates and
    # state read, its da written, dy at level L-1 (1 / depth of the launches)
    bwd_slabs = 2 * n_pad * H * 4 * (C + 2 + 1 + C + 1 + C + 1.0 / DEPTH)
    return {'flops': flops, 'fwd_bytes': int(u_bytes + fwd_slabs),
            'bwd_bytes': int(u_bytes + bwd_slabs)}


def _kernel(H, n_pad, T, coupling, reps):
    import torch
    from asr_study_amd import ops
    dev = 'cuda:0'
    L, C = DEPTH, 2 if coupling else 3
    g = torch.Generator(device=dev).manual_seed(0)
    U = torch.randn(2, L, H, C * H, device=dev, generator=g) * (0.5 / H ** 0.5)
    b = torch.zeros(2, L, C, H, device=dev)
    b[:, :, 1:] = -2.0
    b = b.view(2, L, C * H)
    zx = torch.randn(T, n_pad, 2, C * H, device=dev, generator=g)
    h = torch.empty(L, T, n_pad, 2, H, device=dev)
    gates = torch.empty(L, T, n_pad, 2, C * H, device=dev)
    dy = torch.randn(T, n_pad, 2 * H, device=dev, generator=g)
    da = torch.empty(L, T, n_pad, 2, C * H, device=dev)
    dbp = torch.empty(n_pad // 16, 2, L, C * H, device=dev)
    zmx = torch.empty(1, device=dev)
    out = dict(step_cost(H, n_pad, C))
    for name, fn in (('fwd', lambda: ops.rhn_seq_fwd(zx, U, b, h, gates, T, n_pad, H, L,
                                                     coupling=coupling)),
                     ('bwd', lambda: ops.rhn_seq_bwd(dy, U, h, gates, da, T, n_pad, H, L,
                                                     coupling=coupling, db_part=dbp,
                                                     dz_absmax=zmx))):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / (T * L))
        times.sort()
        us = times[len(times) // 2]
        out[name + '_us_per_microstep'] = round(us, 3)
        out[name + '_us_per_microstep_min'] = round(times[0], 3)
        out[name + '_us_per_microstep_max'] = round(times[-1], 3)
        out[name + '_tflops'] = round(out['flops'] / us * 1e-6, 2)
        out[name + '_tb_per_s'] = round(out[name + '_bytes'] / us * 1e-6, 3)
    return out


def _train(which, steps, warmup):
    import time
    import numpy as np
    import torch
    from asr_study_amd.core import models, optimizers
    if which == 'rhn':
        model = models.rhn(num_features=80, num_hiddens=512, depth=DEPTH, seed=0)
    else:
        model = models.brsmv1(num_features=80, num_hiddens=512, seed=0)
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
        res = {'H%d_n%d_T%d_%s_%s' % (H, n, T, c, 'bwd' if bw else 'fwd'):
               ops.rhn_plan(T, n, H, depth=DEPTH, coupling=c == 'coupled', backward=bw)
               for H, n, T in SHAPES for c in ('coupled', 'uncoupled') for bw in (False, True)}
    elif args.one[0] == 'kernel':
        H, n_pad, T, coupling = (int(v) for v in args.one[1:])
        res = _kernel(H, n_pad, T, bool(coupling), args.reps)
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
    out = {'depth': DEPTH, 'kernels': {}, 'train': {}}
    go = True
    for H, n_pad, T in SHAPES:
        key = 'H%d_n%d_T%d' % (H, n_pad, T)
        row = {}
        for coupling, name in ((1, 'coupled'), (0, 'uncoupled')):
            if not go:
                break
            row[name], go = _run(['--one', 'kernel', str(H), str(n_pad), str(T), str(coupling),
                                  '--reps', str(args.reps)], args.limit)
        out['kernels'][key] = row
    if go:
        out['plan'], go = _run(['--one', 'plan'], args.limit)
    for which in ('rhn', 'brsmv1'):
        if not go:
            break
        out['train'][which], go = _run(['--one', 'train', which, '--steps', str(args.steps),
                                        '--warmup', str(args.warmup)], args.limit)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
