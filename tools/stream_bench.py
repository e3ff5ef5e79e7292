#!/usr/bin/env python
"""Cached chunk-by-chunk inference measurements (K26): milliseconds per step of a
StreamSession and its real-time factor, beside the only thing the library could do before it:
Model.forward over a trailing slab of left + chunk strided frames for every chunk.

    python tools/stream_bench.py [--rounds R] [--reps K] [--json FILE] [--streams 1 64]

Model: conformer(positions='relative', context=(16, 64, 0), causal_conv=True) at the factory's
default sizes (80 features, the two-convolution front-end, d_model 256, 4 heads, 6 blocks), 10 ms
of audio per input frame, time stride 2.  A step is 16 strided frames = 320 ms of audio.

  stream   session.feed() of one step's input frames (device resident) with no decoder: the
           front-end over its window, every stage on 16 new frames, the logits back on the host
  re-run   Model.forward (inference) over 2 (left + chunk) = 160 input frames, which is NOT equal
           to the full forward (the left context of layer 2 would need layer 1's, and so on)

Both are warmed up, then timed with device events over K back-to-back calls (one event pair
around the K calls, ending in a synchronise); the two ALTERNATE within a round, R rounds in one
process; a figure is the median over the rounds, its SPREAD (max - min) / median over the rounds.
The real-time factor is the time of a step over the audio it covers, per session (all streams
advance together).  No ratio is fixed in advance.

A measurement path without a GPU fails; it does not fall back."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_study_amd import ops  # noqa: E402
from asr_study_amd.core import models  # noqa: E402

CONTEXT = (16, 64, 0)
FRAME_MS = 10.0


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--streams', type=int, nargs='+', default=[1, 64])
    ap.add_argument('--json', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('stream_bench: no GPU')
    model = models.conformer(positions='relative', context=CONTEXT, causal_conv=True, dropout=0)
    model.decoder = None
    rs = np.random.RandomState(0)
    results = []
    for n in args.streams:
        ss = model.stream(n_streams=n)
        per_step = ss.step * ss.schedule.stride
        audio_ms = per_step * FRAME_MS
        x = torch.tensor(rs.randn(n, per_step, model.num_features).astype(np.float32),
                         device=model.device)
        slab = model.to_slab(rs.randn(n, 2 * (CONTEXT[0] + CONTEXT[1]), model.num_features)
                             .astype(np.float32))
        lens = torch.full((n,), slab.shape[0] // 2, dtype=torch.int32, device=model.device)
        variants = {
            'stream': lambda: ss.feed(x),
            're-run': lambda: model.forward(slab, training=False, need_grad=False, n_valid=n,
                                            seq_len=lens)[:, :n].cpu(),
        }
        for _ in range(6):                  # (the first feeds emit nothing: the front-end's reach)
            for fn in variants.values():
                fn()
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ms[k].append(timed(fn, args.reps))
        for k, v in ms.items():
            med = float(np.median(v))
            per = med * (ss.step / CONTEXT[0] if k == 're-run' else 1.0)    # per 16 strided frames
            r = dict(streams=n, variant=k, ms=med, spread=float((max(v) - min(v)) / med),
                     ms_per_step=per, rtf=per / audio_ms, n_pad=ops.pad16(n))
            results.append(r)
            print('%2d streams  %-7s %8.3f ms  (spread %.3f)  per %d strided frames %8.3f ms  '
                  'RTF %.4f' % (n, k, med, r['spread'], ss.step, per, r['rtf']))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == '__main__':
    main()
