#!/usr/bin/env python
"""Limited-context attention measurements (K25): the windowed forward and backward
calls of K21 (csrc/attention.hip) and K24 (csrc/rel_attention.hip) beside the unwindowed calls of
the same build.

    python tools/attn_window_bench.py [--rounds R] [--reps K] [--json FILE] [--window C L R]

Shape: the cfg3 slab, T 500 strided frames, 64 samples, 4 heads of 64, ragged lengths >= 200
(seeded).  Windows: (16, 64, 0) chunk-wise with four chunks of left context, (1, -1, 0) causal,
(1, 32, 32) symmetric.  Every call is warmed up, then timed with device events over K
back-to-back launches (one event pair around the K launches, ending in a synchronise: the time
per call is that over K).  The unwindowed call and the three windows ALTERNATE within a round, R
rounds in one process; the figure of a variant is the median over the rounds, its SPREAD the
(max - min) / median over the rounds -- the run-to-run spread a difference has to exceed.

Printed per call: milliseconds, spread, ``tile_pairs`` of the plan (the (query tile, key tile)
pairs one (sample, head) of the forward launch visits without lens; all pairs for the unwindowed
call), the ratio of the tile counts and the ratio of the times.  The expectation is a time ratio
near the tile ratio; the lengths are ragged, so the unwindowed call itself skips the key tiles
past each utterance's length, which the count (lens = NULL) does not know: the count of the
visited tiles WITH the lengths is printed beside it.  The windowed results are checked against
the unwindowed ones for the window (1, T, T) (bit-equal) before anything is timed.

--window C L R times that one window beside the unwindowed call: the program to put behind
``rocprofv3 --kernel-trace --stats --output-format csv --`` (a run of its own), where the
kernels are the instantiations ``attn_fwd_kernel<dh, WIN, REL, false>``, ``attn_bwd_dq_kernel<dh,
WIN, REL>`` and ``attn_bwd_dkv_kernel<dh, WIN, REL>`` of csrc/attn_core.h (WIN true: windowed;
REL true: the relative family) and ``relattn_bwd_dpos_kernel<dh, WIN>``.

A measurement path without a GPU fails; it does not fall back."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_study_amd import ops  # noqa: E402

T, N, HEADS, DH = 500, 64, 4, 64
WINDOWS = [None, (16, 64, 0), (1, -1, 0), (1, 32, 32)]
TILE = 64


def visited_pairs(window, lens):
    """(query tile, key tile) pairs the forward launch visits, summed over the samples, with the
    lengths: the definition of the window restated on the host."""
    total = 0
    for ln in lens:
        for q0 in range(0, T, TILE):
            ql = min(q0 + TILE, T) - 1
            if window is None:
                lo, hi = 0, ln
            else:
                chunk, left, right = window
                lo = 0 if left < 0 else max(0, q0 // chunk * chunk - left)
                hi = min(ql // chunk * chunk + chunk + right, ln)
            k0 = lo // TILE * TILE
            if hi > k0:
                total += -(-(hi - k0) // TILE)
    return int(total)


def _time_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=None)
    ap.add_argument('--window', type=int, nargs=3, default=None, metavar=('C', 'L', 'R'))
    args = ap.parse_args()
    windows = WINDOWS if args.window is None else [None, tuple(args.window)]
    if not torch.cuda.is_available():
        raise SystemExit('attn_window_bench: no GPU; nothing is measured without one')
    dev = 'cuda:0'
    torch.manual_seed(0)
    rs = np.random.RandomState(0)
    lens_h = rs.randint(200, T + 1, size=N)
    lens_h[0], lens_h[-1] = T, 200
    lens = torch.tensor(lens_h.astype(np.int32), device=dev)
    D = HEADS * DH
    qkv = torch.randn(T, N, 3 * D, device=dev)
    dout = torch.randn(T, N, D, device=dev)
    pos = torch.randn(2 * T - 1, D, device=dev)
    bu, bv = torch.randn(D, device=dev) * 0.5, torch.randn(D, device=dev) * 0.5
    out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
    lse = torch.empty(ops.attn_lse_len(T, N, HEADS), device=dev)
    dpos, dbu, dbv = torch.empty_like(pos), torch.empty_like(bu), torch.empty_like(bv)

    def call(kernel, direction, w):
        if kernel == 'K21' and direction == 'fwd':
            return lambda: ops.attn_fwd(qkv, out, N, HEADS, DH, lens=lens, lse=lse, window=w)
        if kernel == 'K21':
            return lambda: ops.attn_bwd(qkv, out, lse, dout, dqkv, N, HEADS, DH, lens=lens,
                                        window=w)
        if direction == 'fwd':
            return lambda: ops.relattn_fwd(qkv, pos, bu, bv, out, N, HEADS, DH, lens=lens,
                                           lse=lse, window=w)
        return lambda: ops.relattn_bwd(qkv, pos, bu, bv, out, lse, dout, dqkv, dpos, dbu, dbv, N,
                                       HEADS, DH, lens=lens, window=w)

    # the yardstick's bits: a window that hides nothing gives the unwindowed results
    for kernel in ('K21', 'K24'):
        res = []
        for w in (None, (1, T, T)):
            call(kernel, 'fwd', w)()
            call(kernel, 'bwd', w)()
            torch.cuda.synchronize()
            res.append([t.clone() for t in (out, lse, dqkv) + ((dpos, dbu, dbv) if kernel == 'K24'
                                                               else ())])
        assert all(torch.equal(a, b) for a, b in zip(*res)), kernel + ': (1, T, T) differs'

    all_pairs = (-(-T // TILE)) ** 2
    pairs = {None: all_pairs}
    for w in windows[1:]:
        pairs[w] = ops.attn_win_plan(T, N, HEADS, DH, w)['tile_pairs']
        assert pairs[w] == ops.relattn_win_plan(T, N, HEADS, DH, w)['tile_pairs']
    visited = {w: visited_pairs(w, lens_h) for w in windows}
    rows = []
    for kernel in ('K21', 'K24'):
        for direction in ('fwd', 'bwd'):
            fns = {w: call(kernel, direction, w) for w in windows}
            if direction == 'bwd':                              # lse and out of this kernel
                call(kernel, 'fwd', None)()
            for fn in fns.values():                             # warm every variant
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {w: [] for w in windows}
            for _ in range(args.rounds):
                for w in windows:                               # alternating within a round
                    if direction == 'bwd':                      # the forward results of THIS window
                        call(kernel, 'fwd', w)()
                    times[w].append(_time_ms(fns[w], args.reps))
            base = float(np.median(times[None]))
            for w in windows:
                med = float(np.median(times[w]))
                spread = (max(times[w]) - min(times[w])) / med
                rows.append(dict(kernel=kernel, call=direction, window=w, ms=med, spread=spread,
                                 tile_pairs=pairs[w], tile_ratio=pairs[w] / all_pairs,
                                 visited=visited[w], visited_ratio=visited[w] / visited[None],
                                 time_ratio=med / base))
                print('%s %s window %-12s: %.3f ms (spread %.1f %% over %d rounds of %d calls); '
                      'tile_pairs %d of %d = %.3f; with the lengths %d of %d = %.3f; time ratio '
                      '%.3f' % (kernel, direction, w, med, 100 * spread, args.rounds, args.reps,
                                pairs[w], all_pairs, pairs[w] / all_pairs, visited[w],
                                visited[None], visited[w] / visited[None], med / base),
                      flush=True)
    ok = True
    for r in rows:
        if r['window'] == windows[1]:
            b = [x for x in rows if x['kernel'] == r['kernel'] and x['call'] == r['call']
                 and x['window'] is None][0]
            faster = r['ms'] * (1 + r['spread']) < b['ms'] * (1 - b['spread'])
            ok = ok and faster
            print('%s %s %s faster than the full call by more than the spread: %s'
                  % (r['kernel'], r['call'], r['window'], faster), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(dict(T=T, N=N, heads=HEADS, dh=DH, rounds=args.rounds, reps=args.reps,
                           rows=[dict(r, window=list(r['window']) if r['window'] else None)
                                 for r in rows]), f, indent=1)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
