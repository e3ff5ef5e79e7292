#!/usr/bin/env python
"""Cached chunk-by-chunk inference measurements (K26): milliseconds per step of a
StreamSession and its real-time factor, beside the only thing the library could do before it:
Model.forward over a trailing slab of left + chunk strided frames for every chunk.

    python tools/stream_bench.py [--rounds R] [--reps K] [--json FILE] [--streams 1 64]
                                 [--decoder none greedy beam] [--beam_width 8 100]
    python tools/stream_bench.py --beam_call_cost [--beam_width 8 100] [--streams 1 64]
    python tools/stream_bench.py --model ds2_uni [--streams 1 16]
    python tools/stream_bench.py --model brsmv1_uni [--streams 1 16]
    python tools/stream_bench.py --audio [--model ...] [--streams 1 64]
    python tools/stream_bench.py --frontend_batch

Model: conformer(positions='relative', context=(16, 64, 0), causal_conv=True) at the factory's
default sizes (80 features, the two-convolution front-end, d_model 256, 4 heads, 6 blocks), 10 ms
of audio per input frame, time stride 2.  A step is 16 strided frames = 320 ms of audio.

  stream   session.feed() of one step's input frames (device resident) with no decoder: the
           front-end over its window, every stage on 16 new frames, the logits back on the host
  re-run   Model.forward (inference) over 2 (left + chunk) = 160 input frames, which is NOT equal
           to the full forward (the left context of layer 2 would need layer 1's, and so on)

``--model ds2_uni`` (K28) times deep_speech2(rnn_type='gru', bidirectional=False)
at the factory's sizes instead (80 features, the two-convolution front-end, 5 x 512 unidirectional
GRU): the same step of 16 strided frames = 320 ms of audio, the same ``stream`` variant and
decoders.  It has no ``re-run`` variant: a recurrent layer has no bounded left context to re-run
over.

``--model brsmv1_uni`` (K29) times brsmv1(bidirectional=False) at the factory's
sizes (39 features, no front-end, 5 x 256 unidirectional LSTM): a step is 16 input frames = 160 ms
of audio (no time stride), one launch per frame and layer.  No ``re-run`` variant either.

``--decoder`` adds sessions that decode (K27), timed in the same rounds as the
decoder-less one: ``greedy`` (variant 'stream+greedy': asr_ctc_greedy_stream per step) and
``beam`` (variant 'stream+beam<W>' per ``--beam_width``: the resumable device beam search,
Model.stream(beam=dict(beam_width=W)), its tree sized for the frames this run feeds).  The logits
are those of the untrained default model on random input, and a beam session's cost is that of
the stream positions the run passes through (a few hundred to a thousand frames in).

``--beam_call_cost`` times the decoder's kernel alone instead (no model): what a call of
asr_ctc_beam_stream costs beside its frames.  1024 frames of 28-class logits (randn * 2, +2 on the
blank, +4 on one class per frame) are fed to fresh streams in calls of Tq = 16 and of Tq = 1, each
followed by a call with chunk_len = 0 (state load, stable-prefix walk, hypothesis write; no
frame, no save); device events around EACH call, so a figure includes the enqueue of the call and
is an upper bound of the kernel's time; medians over the calls of frames 512 .. 1023.  The
stable-prefix walk is taken from the kernel's own counter (BeamStreamState.counters: walk_s) over
the same calls.

``--audio`` (K30) adds the front-end to the step: variant 'stream+audio' is
session.feed_audio() of the step's raw samples (device resident, 160 per input frame) on a session
made with Model.stream(feature=...) -- LogFbank(num_filt=80, norm='running'), or
MFCC(norm='running') for brsmv1_uni -- and 'front-end' the FeatureStream.feed of the same samples
alone.  ``--frontend_batch`` times the batch front-end call (64 utterances of 10 s, log-mel 80:
cfg3's shape) with norm='utterance' and with norm='running', alternating.

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


WARMUP = 6                  # feeds per variant before the timed rounds


def decoding(model, n, x, beam):
    """feed() of a session that decodes: greedy (beam None) or the beam search.  A session keeps
    the decoder it was made under (StreamSession.decoder), so the model serves the decoder-less
    sessions again afterwards."""
    model.decoder = {'is_greedy': True}
    try:
        ss = model.stream(n_streams=n, beam=beam)
    finally:
        model.decoder = None
    return lambda: ss.feed(x)


def beam_call_cost(widths, streams, T=1024, C=28, max_frames=3000):
    rs = np.random.RandomState(0)
    results = []
    for n in streams:
        n_pad = ops.pad16(n)
        x = rs.randn(T, n_pad, C).astype(np.float32) * 2
        x[:, :, C - 1] += 2.0
        x[np.arange(T)[:, None], np.arange(n_pad)[None], rs.randint(0, C, size=(T, n_pad))] += 4.0
        slab = torch.from_numpy(x).cuda()
        zero = torch.zeros(n, dtype=torch.int32, device='cuda:0')
        for width in widths:
            for tq in (16, 1):
                st = ops.BeamStreamState(n, C, width, max_frames, None, 'cuda:0')
                full = torch.full((n,), tq, dtype=torch.int32, device='cuda:0')
                with_frames, without, walk0 = [], [], None
                for t0 in range(0, T, tq):
                    if t0 == T // 2:
                        walk0 = st.counters(0)['walk_s']
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    ev[0].record()
                    out = ops.ctc_beam_stream(slab[t0:t0 + tq], full, st, n, width, True, max_frames)
                    ev[1].record()
                    ops.ctc_beam_stream(slab[t0:t0 + tq], zero, st, n, width, True, max_frames)
                    ev[2].record()
                    torch.cuda.synchronize()
                    if t0 >= T // 2:
                        with_frames.append(ev[0].elapsed_time(ev[1]))
                        without.append(ev[1].elapsed_time(ev[2]))
                walk = (st.counters(0)['walk_s'] - walk0) * 1e3 / (2 * len(without))
                r = dict(streams=n, width=width, Tq=tq, calls=len(without),
                         ms=float(np.median(with_frames)), ms_no_frame=float(np.median(without)),
                         no_frame_spread=float((max(without) - min(without)) / np.median(without)),
                         ms_walk=walk, decoded_len=float(out[1].float().mean()),
                         stable_len=float(out[2].float().mean()))
                results.append(r)
                print('%2d streams  width %4d  Tq %2d: %7.3f ms, without a frame %7.3f ms (spread '
                      '%.2f), of which the stable-prefix walk %7.4f ms; hypothesis %.0f labels, '
                      '%.0f stable' % (n, width, tq, r['ms'], r['ms_no_frame'],
                                       r['no_frame_spread'], walk, r['decoded_len'],
                                       r['stable_len']))
    return results


def frontend_batch(rounds, reps, n_utt=64, seconds=10.0):
    """The batch front-end call at cfg3's shape under both normalisations."""
    from asr_study_amd.preprocessing import audio
    rs = np.random.RandomState(0)
    n = int(seconds * 16000)
    lens = [n] * n_utt
    flat = torch.from_numpy(rs.randn(n_utt * n).astype(np.float32)).cuda()
    offs = torch.arange(n_utt, dtype=torch.int32, device='cuda:0') * n
    dlen = torch.full((n_utt,), n, dtype=torch.int32, device='cuda:0')
    feats = {k: audio.LogFbank(num_filt=80, norm=k) for k in ('utterance', 'running')}
    calls = {k: (lambda f=f: f.batch_device(flat, offs, dlen, lens)) for k, f in feats.items()}
    for fn in calls.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            ms[k].append(timed(fn, reps))
    results = []
    for k, v in ms.items():
        med = float(np.median(v))
        results.append(dict(norm=k, n_utt=n_utt, seconds=seconds, ms=med,
                            spread=float((max(v) - min(v)) / med)))
        print('front-end batch call, %d x %.0f s, log-mel 80, norm=%-9s %8.3f ms  (spread %.3f)'
              % (n_utt, seconds, k, med, results[-1]['spread']))
    return results


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--streams', type=int, nargs='+', default=[1, 64])
    ap.add_argument('--json', default=None)
    ap.add_argument('--decoder', nargs='+', default=['none'], choices=['none', 'greedy', 'beam'])
    ap.add_argument('--beam_width', type=int, nargs='+', default=[100])
    ap.add_argument('--beam_call_cost', action='store_true')
    ap.add_argument('--model', default='conformer', choices=['conformer', 'ds2_uni', 'brsmv1_uni'])
    ap.add_argument('--audio', action='store_true')
    ap.add_argument('--frontend_batch', action='store_true')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('stream_bench: no GPU')
    if args.frontend_batch:
        results = frontend_batch(args.rounds, args.reps)
        if args.json:
            with open(args.json, 'w') as f:
                json.dump(results, f, indent=1)
        return results
    if args.beam_call_cost:
        results = beam_call_cost(args.beam_width, args.streams)
        if args.json:
            with open(args.json, 'w') as f:
                json.dump(results, f, indent=1)
        return results
    if args.model == 'ds2_uni':
        model = models.deep_speech2(rnn_type='gru', bidirectional=False, dropout=0)
    elif args.model == 'brsmv1_uni':
        model = models.brsmv1(bidirectional=False, dropout=0)
    else:
        model = models.conformer(positions='relative', context=CONTEXT, causal_conv=True,
                                 dropout=0)
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
        variants = {}
        if 'none' in args.decoder:
            variants['stream'] = lambda: ss.feed(x)
        if 'greedy' in args.decoder:
            variants['stream+greedy'] = decoding(model, n, x, None)
        for width in (args.beam_width if 'beam' in args.decoder else ()):
            frames = (WARMUP + args.rounds * args.reps) * ss.step    # every feed of this run
            variants['stream+beam%d' % width] = decoding(
                model, n, x, dict(beam_width=width, max_frames=max(3000, frames)))
        if args.audio:
            from asr_study_amd.preprocessing import audio
            feat = (audio.MFCC(norm='running') if args.model == 'brsmv1_uni'
                    else audio.LogFbank(num_filt=80, norm='running'))
            sa = model.stream(n_streams=n, feature=feat)
            wave = torch.tensor(rs.randn(n, per_step * 160).astype(np.float32),
                                device=model.device)
            fs = feat.stream(n)
            variants['stream+audio'] = lambda: sa.feed_audio(wave)
            variants['front-end'] = lambda: fs.feed(wave)
        if args.model == 'conformer':
            variants.update({
                're-run': lambda: model.forward(slab, training=False, need_grad=False, n_valid=n,
                                                seq_len=lens)[:, :n].cpu(),
            })
        for _ in range(WARMUP):             # (the first feeds emit nothing: the front-end's reach)
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
