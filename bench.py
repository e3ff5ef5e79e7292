#!/usr/bin/env python
"""Headline benchmark: audio-seconds/second TRAINED on the acoustic hot path
(MFCC/log-mel front-end -> BiLSTM stack fwd/bwd -> CTC loss/grad/greedy decode ->
global-norm clip + Adam, + RCCL gradient all-reduce when N > 1), synthetic 16 kHz
10 s utterances, random-init weights of the named topology.

    python bench.py --gpus N --steps K --warmup W [--config cfg3|cfg2] [--full]
                    [--dump-outputs DIR]

Default workload: cfg3 (BASELINE.json configs[2], the configuration the north-star targets
and the 1/2/4/8 scaling curve are quoted on: 5 x BiLSTM(512), 80 log-mel features, batch 64
per GPU).  One process per GPU, weak scaling (per-GPU batch fixed).  With ``--gpus N > 1``
and no WORLD_SIZE in the environment the script launches itself under
``python -m torch.distributed.run --nproc-per-node N`` (so both ``python bench.py --gpus 8``
and the explicit torchrun form run 8 ranks); rank 0 prints ONE JSON line.  A "step" = one
pass of the hot path over one mini-batch whose samples are already resident in HBM when
the timed region starts.

A plain run sets up, warms up, times the K steps and prints the line: the contract fields,
`config`, `fallbacks` and the rooflines taken from the timed steps' own HIP events.  Every
measurement that takes runs of its own -- the companion configurations, the gate-GEMM and
CTC rooflines, predict latency, beam search, dataset build, the all-reduce bus bandwidth and
the CPU baseline -- runs only with ``--full``.  ``--dump-outputs DIR`` writes what the last
timed step computed (per-utterance CTC loss, greedy decode and its lengths, and a fixed,
seeded sample of the updated parameters and of their gradients) as DIR/<name>.npy; the inputs
depend on the arguments only, so two builds can be compared output for output.

The ONE stdout line is small (< LINE_LIMIT bytes, tests/test_bench_launch.py): the contract
fields, `config`, ONE `roofline` (the family with the largest share of GPU time, over ALL of
its launches; the launches that own the chip are its `chip_owning` sub-object), `cpu_baseline`
(the NumPy oracle port on this host's cores, bounded sample, N = 1 only), and compact
{value, ms_per_step, frac} objects / scalars for the companion measurements (``--full``):
  as_written        BASELINE.json configs[2] WITH its 2-conv front-end (own process),
  cfg2 / cfg2_n128  configs[1], and its topology at a chip-filling batch (own processes),
  exact_fp32        cfg3 again with every product on the exact-fp32 MFMA instructions,
  lstm_*_us_per_step, gate_gemm_frac, ctc_*, predict_ms, beam_s, dataset_build_audio_s_per_s,
  allreduce         bus bandwidth of the gradient all-reduce, N > 1 only.
Everything else -- notes, per-role tables, every per-kernel roofline object, calibration --
is the DETAIL object: written to bench_detail.json next to this script (and gpurun_out/ when
that directory exists) and echoed on stderr behind the prefix "bench detail: ".
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CONFIGS = {
    # BASELINE.json configs[1]: brsmv1 defaults, batch 32
    'cfg2': dict(model='brsmv1', F=39, H=256, L=5, C=28, N=32, feat='mfcc',
                 desc='brsmv1 5xBiLSTM(256), MFCC-39, 28-class CTC, batch 32 x 10 s @16 kHz'),
    # the same topology at a batch that fills the chip (16 chains x 16 workgroups = 256 CUs;
    # cfg2's own batch of 32 occupies 64): the `cfg2_n128` sub-object of the line
    'cfg2_n128': dict(model='brsmv1', F=39, H=256, L=5, C=28, N=128, feat='mfcc',
                      desc='brsmv1 5xBiLSTM(256), MFCC-39, 28-class CTC, batch 128 x 10 s @16 kHz '
                           '(configs[1] topology, chip-filling batch)'),
    # BASELINE.json configs[2] minus its conv front-end: 5xBiLSTM(512), 80-dim log-mel, batch 64
    # (the configuration the north-star targets are quoted on; as written -> cfg3_conv below)
    'cfg3': dict(model='brsmv1', F=80, H=512, L=5, C=28, N=64, feat='logfbank80',
                 desc='5xBiLSTM(512), log-mel-80, 28-class CTC, batch 64 x 10 s @16 kHz'),
    # BASELINE.json configs[2] WITH its "2 conv front-end" (models.deep_speech2; no reference
    # counterpart, README.md:118): 32 x (11 x 41) / (2, 2) and 32 x (11 x 21) / (1, 2), clipped
    # ReLU 20 -> the recurrent stack sees 500 frames of 640 features.  Reported as the
    # `cfg3_conv` sub-object of the cfg3 line (the headline stays cfg3 for continuity).
    'cfg3_conv': dict(model='deep_speech2', F=80, H=512, L=5, C=28, N=64, feat='logfbank80',
                      desc='2 x conv2d (32 ch, 11x41/(2,2), 11x21/(1,2), clipped ReLU) + '
                           '5xBiLSTM(512), log-mel-80, 28-class CTC, batch 64 x 10 s @16 kHz'),
}
PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: fp32-in MFMA = fp32 vector peak
PEAK_F16_MFMA_TFLOPS = 2500.0     # dense fp16/bf16 MFMA peak
PEAK_HBM_GBS = 8000.0
SAMPLES = 160000                  # 10 s @ 16 kHz -> T = 999 frames


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_command(n, argv, port=None):
    """The command ``python bench.py --gpus n`` re-executes itself as (one rank per GPU)."""
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node',
            str(int(n)), '--master-addr', '127.0.0.1', '--master-port',
            str(port or _free_port()), os.path.abspath(__file__)] + list(argv)


def _rec_kernel_name(H, backward):
    """The recurrent kernel asr_lstm_plan selects for the plain cell at hidden size H (csrc/lstm.hip,
    make_plan): the wide kernels at 256 / 512, the any-H ones otherwise."""
    exact = os.environ.get('ASR_LSTM_PREC', '1') == '0'
    if H not in (256, 512):
        return 'lstm_bwd_kernel_h' if backward else 'lstm_fwd_kernel_h'
    if not backward:
        return 'lstm_fwd_kernel_x<%d, %s>' % (H // 128, 'true' if exact else 'false')
    if exact or H == 512:
        return 'lstm_bwd_kernel_c<%d, %s> (two-dimensional split)' % (H // 256, 'true' if exact else 'false')
    return 'lstm_bwd_kernel_x<%d>' % (H // 64)


def _pmc_traffic(config):
    """HBM bytes per LAYER of the recurrent kernels from the committed rocprofv3 PMC passes
    (FETCH_SIZE x2 + WRITE_SIZE, per-launch average x launches per layer):
    profiles/pmc_traffic.json, written from profiles/*_hbm_traffic.md."""
    try:
        with open(os.path.join(ROOT, 'profiles', 'pmc_traffic.json')) as f:
            return json.load(f).get(config, {})
    except Exception:
        return {}


def cpu_baseline(cfg):
    """The oracle (a NumPy port of the reference algorithm: per-timestep two-matmul LSTM
    loop, CPU CTC, BPTT, Adam; float64 front-end) timed on this host, on BOUNDED samples of
    the workload: value = whole training step at the benchmarked topology on
    N <= 16 utterances of the benchmark's full 10 s (T = 999); plus the front-end alone on
    10 s utterances (1 core and all cores) and one cfg1 step (1 x BiLSTM(100), batch 4 x 10 s).
    `cores` = the host's CPUs, `blas_threads` = the threads the matmuls actually used."""
    from oracle import frontend as OF
    from oracle import lstm as OL
    from oracle import optim as OO
    kind, kw = ('mfcc', {}) if cfg['feat'] == 'mfcc' else ('logfbank', {'num_filt': 80})
    try:
        import threadpoolctl
        threads = max([p.get('num_threads', 1) for p in threadpoolctl.threadpool_info()] + [1])
    except Exception:
        threads = os.cpu_count() or 1

    def timed(fn, min_s, max_s, min_reps=1):
        fn()                                              # warm caches / BLAS threads
        t0 = time.time()
        reps = 0
        while reps < min_reps or time.time() - t0 < min_s:
            fn()
            reps += 1
            if reps >= min_reps and time.time() - t0 > max_s:
                break
        return (time.time() - t0) / reps, reps

    def train_step_fn(F, H, L, C, n, secs, feat_kind, feat_kw):
        rs = np.random.RandomState(0)
        sigs = [rs.randn(int(16000 * secs)).astype(np.float32) for _ in range(n)]
        labels = [rs.randint(0, 25, size=rs.randint(2, 12)).tolist() for _ in range(n)]
        params = OL.init_model(seed=0, num_features=F, num_hiddens=H, num_layers=L,
                               num_classes=C, dtype=np.float32)
        opt = OO.Adam(lr=1e-3, clipnorm=400.0)

        def step():
            feats = [OF.extract(feat_kind, s.astype(np.float64), **feat_kw).astype(np.float32)
                     for s in sigs]
            x = np.stack(feats, axis=1)                   # (T, N, F)
            out = OL.loss_and_grads(params, x, labels, [x.shape[0]] * n, weight_decay=1e-4)
            opt.step([a for _, a in OL.flatten(params)], [a for _, a in OL.flatten(out['grads'])])
        return step

    # (1) the benchmarked topology at the benchmark's FULL utterance length (10 s, T = 999) on
    # a bounded share of its batch.  The per-timestep matmuls are small (N x 2H @ 2H x 4H), where
    # more BLAS threads are not faster: a short calibration (T = 24 frames) picks the thread
    # count and, from its time per frame, the largest N in {16, 8, 4} whose full-length step is
    # estimated under ~30 s; then ONE full-length step is timed after a warm-up step at T = 99.
    ncpu = os.cpu_count() or 1
    try:
        import threadpoolctl
    except Exception:
        threadpoolctl = None
    cands = sorted({min(ncpu, c) for c in (8, 32, 128, ncpu)}) if threadpoolctl else [threads]
    calib = {}
    for thr in cands:
        ctx = threadpoolctl.threadpool_limits(thr) if threadpoolctl else None
        try:
            dtc, _ = timed(train_step_fn(cfg['F'], cfg['H'], cfg['L'], cfg['C'], 16, 0.255, kind, kw),
                           0.0, 0.0, min_reps=1)
        finally:
            if ctx is not None:
                ctx.restore_original_limits()
        calib[thr] = dtc
    best_thr = min(calib, key=calib.get)
    per_frame_16 = calib[best_thr] / 24.0           # seconds per frame at N = 16
    n = 16
    while n > 4 and per_frame_16 * (n / 16.0) * 999 > 30.0:
        n //= 2
    secs = 10.0
    ctx = threadpoolctl.threadpool_limits(best_thr) if threadpoolctl else None
    try:
        # warm-up: one step of the SAME topology and batch on 1 s utterances (T = 99: BLAS thread
        # pool at best_thr, allocator, weights in cache; a tenth of the timed step), then ONE
        # full-length step is timed
        train_step_fn(cfg['F'], cfg['H'], cfg['L'], cfg['C'], n, 1.0, kind, kw)()
        step = train_step_fn(cfg['F'], cfg['H'], cfg['L'], cfg['C'], n, secs, kind, kw)
        t0 = time.time()
        step()
        dt = time.time() - t0
    finally:
        if ctx is not None:
            ctx.restore_original_limits()
    out = {'value': round(n * secs / dt, 2), 'unit': 'audio-seconds/s', 'cores': int(ncpu),
           'blas_threads': int(best_thr), 'kind': 'port', 'utterances': int(n),
           'calibration_s_per_24_frames': {str(k): round(v, 3) for k, v in calib.items()},
           'sample': '%d utterances x %.0f s (T=999: the benchmark\'s full length, %d of its %d '
                     'utterances), same topology, ONE step of %.1f s: NumPy/BLAS float32 oracle '
                     'port (per-timestep two-matmul LSTM loop as Keras consume_less=gpu) incl. '
                     'float64 front-end, CTC, BPTT, clip+Adam; BLAS threads chosen by a 24-frame '
                     'calibration' % (n, secs, n, cfg['N'], dt)}
    # (2) front-end alone, 10 s utterances: one core, then all cores (process pool)
    sig10 = np.random.RandomState(1).randn(SAMPLES)
    dt1, _ = timed(lambda: OF.extract(kind, sig10, **kw), 1.0, 4.0)
    out['frontend_1core'] = {'value': round(10.0 / dt1, 1), 'unit': 'audio-seconds/s', 'cores': 1,
                             'sample': 'one 10 s utterance, %s' % cfg['feat']}
    try:
        import multiprocessing as mp
        ncpu = os.cpu_count() or 1
        per = 8                                           # utterances per worker
        with mp.get_context('fork').Pool(ncpu) as pool:
            pool.map(_fe_job, [(kind, kw, 50 + i, 1) for i in range(ncpu)], chunksize=1)  # warm
            t0 = time.time()
            pool.map(_fe_job, [(kind, kw, 100 + i, per) for i in range(ncpu)], chunksize=1)
            dta = time.time() - t0
        out['frontend_allcores'] = {'value': round(10.0 * per * ncpu / dta, 1),
                                    'unit': 'audio-seconds/s', 'cores': ncpu,
                                    'sample': '%d x 10 s utterances over a %d-process pool, one '
                                              'BLAS thread each' % (per * ncpu, ncpu)}
    except Exception as e:                                # never fail the bench on the baseline
        out['frontend_allcores'] = {'error': repr(e)[:200]}
    # (3) cfg1: 26-dim MFCC, 1 x BiLSTM(100), batch 4 x 10 s (the reference's CPU-runnable case)
    dt2, reps2 = timed(train_step_fn(26, 100, 1, 28, 4, 10.0, 'mfcc', {'dd': False}), 2.0, 10.0)
    out['cfg1_step'] = {'value': round(40.0 / dt2, 2), 'unit': 'audio-seconds/s',
                        'cores': int(ncpu), 'blas_threads': int(threads),
                        'sample': 'cfg1: 4 x 10 s, 1xBiLSTM(100), %d step(s) of %.2f s' % (reps2, dt2)}
    return out


def _fe_job(job):
    from oracle import frontend as OF
    kind, kw, seed, count = job
    try:                                   # one BLAS / OpenMP thread per worker process
        import threadpoolctl
        ctx = threadpoolctl.threadpool_limits(1)
    except Exception:
        ctx = None
    sig = np.random.RandomState(seed).randn(SAMPLES)
    n = 0
    for _ in range(count):
        n += OF.extract(kind, sig, **kw).shape[0]
    del ctx
    return n


def predict_latency(dev):
    """predict.py's unit of work (predict.py:73-93): ONE 10 s utterance through front-end,
    5 x BiLSTM(256) forward (brsmv1 defaults) and greedy decode, in milliseconds per
    utterance (the single-utterance recurrent kernel, fwd_body_n1)."""
    import torch
    from asr_study_amd import ops
    from asr_study_amd.core import models
    from asr_study_amd.preprocessing import audio
    model = models.brsmv1(num_features=39, num_classes=28, num_hiddens=256, num_layers=5,
                          dropout=0.2, weight_decay=1e-4, seed=0, device=dev)
    feat = audio.MFCC(device=dev)
    sig = np.random.RandomState(5).randn(SAMPLES).astype(np.float32)
    out = {'utterance_seconds': 10.0, 'topology': 'brsmv1 5xBiLSTM(256), MFCC-39'}
    def once():
        slab, frames = feat.batch([sig])
        logits = model.forward(slab, training=False, need_grad=False, n_valid=1)
        return ops.ctc_greedy(logits, frames, 1)
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 10
    for _ in range(reps):
        once()
    torch.cuda.synchronize()
    out['n1_kernel_ms'] = round((time.perf_counter() - t0) / reps * 1e3, 3)
    for ws in ('lstm_fwd',):
        ops.lstm_status(ops.WS.get(ws, 0, dev))
    out['real_time_factor'] = round(10.0 / (out['n1_kernel_ms'] * 1e-3), 1)
    return out


def eval_beam(dev, model, slab, n_valid, frames):
    """eval.py's decoder (utils/core_utils.py:67-72: beam search, width 400 by default; README's
    25.13 % LER used 100) on the bench batch: seconds per batch on the device
    (asr_ctc_beam_device: logits stay in HBM) and with the library's host decoder (one
    utterance per host thread, after a D2H copy of the logits)."""
    import torch
    from asr_study_amd import ops
    logits = model.forward(slab, training=False, need_grad=False, n_valid=n_valid)
    sl = torch.full((n_valid,), int(frames), dtype=torch.int32, device=dev)
    out = {'utterances': int(n_valid), 'frames': int(frames), 'classes': int(logits.shape[2])}
    for width in (100, 400):
        ops.ctc_beam_search(logits, sl, n_valid, width)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec, dlen, _ = ops.ctc_beam_search(logits, sl, n_valid, width)
        torch.cuda.synchronize()
        out['device_width_%d_s' % width] = round(time.perf_counter() - t0, 4)
        t0 = time.perf_counter()
        host, _ = ops.ctc_beam_search_host(logits.cpu().numpy(), [int(frames)] * n_valid, n_valid, width)
        out['host_width_%d_s' % width] = round(time.perf_counter() - t0, 4)
        d, l = dec.cpu().numpy(), dlen.cpu().numpy()
        out['same_strings_width_%d' % width] = bool(
            all(d[n, :l[n]].tolist() == host[n] for n in range(n_valid)))
    out['host_threads'] = min(int(n_valid), os.cpu_count() or 1)
    # what eval.py / ctc_utils.decode actually run (ops.beam_decoder_choice, ASR_BEAM=auto): the
    # host decoder while every utterance gets its own host thread, the device decoder beyond
    out['default_decoder'] = ops.beam_decoder_choice(n_valid, 100, int(logits.shape[2]))
    for width in (100, 400):
        out['default_width_%d_s' % width] = out['%s_width_%d_s' % (out['default_decoder'], width)]
    return out


def dataset_build(dev, feat, utterances=2048, pool=32, chunk=64):
    """N1 (extras/make_dataset.py:31-48 -> DatasetParser.to_h5, datasets/dataset_parser.py:
    87-177): a synthetic corpus of `utterances` x 10 s through the GPU front-end into the
    reference's HDF5 layout, END TO END -- host concatenation, H2D, the feature kernels, D2H,
    slicing and the HDF5 write (ctypes libhdf5) -- in audio-seconds per second.  The samples
    come from a pool of `pool` distinct N(0,1) signals (generating 2048 x 160000 normals would
    time the host RNG, not the path)."""
    import tempfile
    from asr_study_amd.datasets.dataset_parser import DatasetParser
    rs = np.random.RandomState(11)
    sigs = [rs.randn(SAMPLES).astype(np.float32) for _ in range(pool)]

    class Synth(DatasetParser):
        def _iter(self):
            for i in range(utterances):
                yield {'input': sigs[i % pool], 'label': 'abc', 'duration': 10.0}
    out = {'utterances': utterances, 'utterance_seconds': 10.0, 'chunk': chunk,
           'features': str(feat) + str(feat.num_feats)}
    with tempfile.TemporaryDirectory() as tmp:
        for fmt in ('h5', 'npz'):
            try:
                path = os.path.join(tmp, 'corpus.' + fmt)
                t0 = time.perf_counter()
                Synth(name='synth').to_h5(path, input_parser=feat, split_sets=False,
                                          chunk=chunk, fmt=fmt)
                dt = time.perf_counter() - t0
                out.update(value=round(utterances * 10.0 / dt, 1), unit='audio-seconds/s',
                           seconds=round(dt, 3), format=fmt,
                           file_MB=round(os.path.getsize(path) / 1e6, 1))
                break
            except Exception as e:                     # no libhdf5 on this host: npz layout
                out['%s_error' % fmt] = repr(e)[:200]
    return out


def _sub_bench(config, env_extra, steps, warmup, dropout):
    """Runs this script in its own process (other config / other arithmetic switches) and
    returns a compact object from its JSON line."""
    env = dict(os.environ, **env_extra)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.abspath(__file__), '--gpus', '1', '--steps', str(steps),
           '--warmup', str(warmup), '--config', config, '--dropout', str(dropout),
           '--full', '--no-cpu-baseline', '--no-extras', '--emit', 'detail']
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=600, stdin=subprocess.DEVNULL)
        lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith('{')]
        if r.returncode != 0 or not lines:
            return {'error': (r.stderr.decode() or r.stdout.decode())[-300:]}
        d = json.loads(lines[-1])
    except Exception as e:
        return {'error': repr(e)[:300]}
    keep = {k: d[k] for k in ('value', 'unit', 'ms_per_step', 'steps', 'warmup', 'arithmetic')}
    keep['workload'] = d['config']['workload']
    for k in ('roofline', 'roofline_lstm_fwd', 'roofline_lstm_bwd', 'roofline_gemm_step', 'roofline_conv'):
        if k not in d:
            continue
        keep[k] = {kk: d[k].get(kk) for kk in ('kernel', 'bound', 'achieved', 'peak', 'unit', 'frac',
                                               'us_per_timestep', 'avg_launch_ms', 'traffic',
                                               'algorithmic_fp32_tflops', 'ms_per_step',
                                               'per_role_ms', 'per_role_algorithmic_tflops', 'geometry',
                                               'chip_owning', 'shared', 'launches_per_step')
                   if kk in d[k]}
    keep['roofline_gate_gemm'] = {kk: d['roofline_gate_gemm'].get(kk) for kk in
                                  ('kernel', 'achieved', 'peak', 'unit', 'frac',
                                   'algorithmic_fp32_tflops', 'avg_launch_ms', 'pack_ms')}
    return keep


LINE_LIMIT = 6000                 # bytes of the ONE stdout line (the driver keeps an 8 KB tail)
CONTRACT_KEYS = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step',
                 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data')
ROOF_KEYS = ('kernel', 'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'avg_launch_ms')


def _short(text, n):
    text = str(text)
    return text if len(text) <= n else text[:n - 3] + '...'


def _roof_compact(r):
    """The `roofline` object of the line: the required keys (traffic stays, null when no counter
    pass covers the kernel), GPU time per step, and the chip-owning / shared subsets' fractions."""
    out = {k: r.get(k) for k in ROOF_KEYS}
    out['kernel'] = _short(out['kernel'], 110)
    for k in ('launches_per_step', 'ms_per_step', 'us_per_timestep'):
        if r.get(k) is not None:
            out[k] = r[k]
    for sub in ('chip_owning', 'shared'):
        if r.get(sub):
            out[sub] = {k: r[sub].get(k) for k in ('frac', 'ms_per_step', 'launches_per_step',
                                                   'avg_launch_ms')}
    return out


def _sub_compact(d):
    """A companion run (its own process) as {value, ms_per_step, frac, ...}."""
    if not isinstance(d, dict):
        return None
    if 'error' in d:
        return {'error': _short(d['error'], 120)}
    out = {'value': d.get('value'), 'ms_per_step': d.get('ms_per_step')}
    roof = d.get('roofline') or {}
    out['frac'] = roof.get('frac')
    out['roofline_kernel'] = _short(roof.get('kernel', ''), 40)
    for key, name in (('roofline_lstm_fwd', 'fwd_us'), ('roofline_lstm_bwd', 'bwd_us')):
        if (d.get(key) or {}).get('us_per_timestep') is not None:
            out[name] = d[key]['us_per_timestep']
    if (d.get('roofline_gate_gemm') or {}).get('frac') is not None:
        out['gate_gemm_frac'] = d['roofline_gate_gemm']['frac']
    return out


def compact_line(detail, limit=LINE_LIMIT):
    """The ONE JSON object bench.py prints on stdout, from the full DETAIL object of a run.
    Pure function of `detail` (tests/test_bench_launch.py builds it from a canned measurement).
    Optional keys are dropped from the end of `optional` until the line fits `limit`."""
    line = {k: detail.get(k) for k in CONTRACT_KEYS}
    line['dtype'] = _short(line['dtype'], 48)
    cfg = dict(detail.get('config') or {})
    cfg['workload'] = _short(cfg.get('workload', ''), 120)
    if 'baseline_config' in cfg:
        cfg['baseline_config'] = _short(cfg['baseline_config'], 100)
    line['config'] = cfg
    line['roofline'] = _roof_compact(detail['roofline']) if detail.get('roofline') else None
    cb = detail.get('cpu_baseline')
    if cb:
        c = {k: cb.get(k) for k in ('value', 'unit', 'cores', 'kind', 'blas_threads', 'utterances')}
        c['sample'] = _short(cb.get('sample', ''), 150)
        for k in ('frontend_1core', 'frontend_allcores', 'cfg1_step'):
            if isinstance(cb.get(k), dict) and cb[k].get('value') is not None:
                c[k] = cb[k]['value']
        line['cpu_baseline'] = c
    optional = []                            # (key, value): most dispensable LAST

    def opt(key, value):
        if value is not None:
            optional.append((key, value))
    opt('fallbacks', detail.get('fallbacks'))
    for k in ('as_written', 'cfg2', 'cfg2_n128', 'exact_fp32'):
        src = detail.get('cfg3_conv') if k == 'as_written' else detail.get(k)
        opt(k, _sub_compact(src))
    for key, name in (('roofline_lstm_fwd', 'lstm_fwd_us_per_step'),
                      ('roofline_lstm_bwd', 'lstm_bwd_us_per_step')):
        opt(name, (detail.get(key) or {}).get('us_per_timestep'))
    geo = (detail.get('roofline_lstm_bwd') or {}).get('geometry')
    if geo:
        opt('lstm_bwd_us_per_step_by_geometry', {'compact': geo.get('compact_us_per_timestep'),
                                                 'default': geo.get('default_us_per_timestep')})
    opt('gate_gemm_frac', (detail.get('roofline_gate_gemm') or {}).get('frac'))
    ctc = detail.get('roofline_ctc') or {}
    if ctc:
        opt('ctc', {'hbm_frac': ctc.get('frac'), 'ms': ctc.get('avg_ms'), 'traffic': ctc.get('traffic')})
    conv = detail.get('roofline_conv') or {}
    if conv:
        opt('conv', {'frac': conv.get('frac'), 'ms_per_step': conv.get('ms_per_step')})
    ar = detail.get('allreduce')
    if ar:
        opt('allreduce', {k: ar.get(k) for k in ('bytes', 'ms', 'bus_GBps')})
    opt('ranks_seen_by_rccl', detail.get('ranks_seen_by_rccl'))
    arm = detail.get('allreduce_model') or {}
    opt('allreduce_model_ring_8gpu_ms', arm.get('ring_8gpu_ms'))
    pl = detail.get('predict_latency') or {}
    opt('predict_ms', pl.get('n1_kernel_ms', _short(pl.get('error'), 80) if pl.get('error') else None))
    eb = detail.get('eval_beam') or {}
    if eb:
        opt('beam_s', {'decoder': eb.get('default_decoder'), 'w100': eb.get('default_width_100_s'),
                       'w400': eb.get('default_width_400_s'),
                       'device_w100': eb.get('device_width_100_s'),
                       'host_w100': eb.get('host_width_100_s')}
            if 'error' not in eb else {'error': _short(eb['error'], 80)})
    db = detail.get('dataset_build') or {}
    opt('dataset_build_audio_s_per_s', db.get('value', _short(db.get('error'), 80) if db.get('error') else None))
    opt('detail', detail.get('detail_file'))
    while True:
        out = dict(line)
        out.update(optional)
        text = json.dumps(out)
        if len(text) < limit or not optional:
            return out
        optional.pop()


def emit(detail, stream_out=None, stream_err=None):
    """Writes the DETAIL object to bench_detail.json (+ gpurun_out/), names that file on stderr
    (ONE short line: a reader that keeps only a tail of stdout + stderr together must still find
    the whole compact line in it; ASR_BENCH_ECHO_DETAIL=1 echoes the detail object there as
    well) and prints the compact line as the LAST thing on stdout."""
    stream_out = stream_out or sys.stdout
    stream_err = stream_err or sys.stderr
    path = os.environ.get('ASR_BENCH_DETAIL', os.path.join(ROOT, 'bench_detail.json'))
    paths = [path]
    if os.path.isdir(os.path.join(ROOT, 'gpurun_out')):
        paths.append(os.path.join(ROOT, 'gpurun_out', 'bench_detail.json'))
    detail['detail_file'] = os.path.basename(path)
    text = json.dumps(detail)
    for p_ in paths:
        try:
            with open(p_, 'w') as f:
                f.write(text + '\n')
        except OSError:
            pass
    if os.environ.get('ASR_BENCH_ECHO_DETAIL') == '1':
        print('bench detail: ' + text, file=stream_err)
    else:
        print('bench detail: %d bytes in %s' % (len(text), ', '.join(paths)), file=stream_err)
    stream_err.flush()
    line = json.dumps(compact_line(detail))
    assert len(line) < 8192
    print(line, file=stream_out)
    stream_out.flush()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--config', default=os.environ.get('ASR_BENCH_CONFIG', 'cfg3'),
                    choices=sorted(CONFIGS))
    ap.add_argument('--dropout', type=float, default=0.2)      # brsmv1 default
    ap.add_argument('--full', action='store_true',
                    help='also run every measurement beyond the headline: companion '
                         'configurations, gate-GEMM / CTC rooflines, predict latency, beam search, '
                         'dataset build, all-reduce bandwidth, CPU baseline')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed as DIR/<name>.npy')
    ap.add_argument('--no-cpu-baseline', action='store_true',
                    help='with --full: skip the CPU baseline')
    ap.add_argument('--no-extras', action='store_true',
                    help='with --full: skip the cfg2 / exact-fp32 companion runs')
    ap.add_argument('--emit', default='compact', choices=('compact', 'detail'),
                    help='stdout line: the compact line (default) or the full detail object '
                         '(what the companion runs hand to their parent)')
    args = ap.parse_args()
    cfg = CONFIGS[args.config]

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # `python bench.py --gpus N`: one rank per GPU under torch.distributed.run
        env = dict(os.environ)
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        cmd = launch_command(args.gpus, sys.argv[1:])
        if os.environ.get('ASR_BENCH_DRY_LAUNCH') == '1':      # launch-contract test hook
            print(json.dumps({'launch': cmd}))
            return 0
        return subprocess.call(cmd, env=env, cwd=ROOT)

    import torch
    import torch.distributed as dist
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    cpu_stub = os.environ.get('ASR_BENCH_CPU_STUB') == '1'     # launch-contract test (gloo, no GPU)
    if cpu_stub:
        return _cpu_stub(args, rank, world)
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a GPU (the hot path has no CPU fallback)')
    if world != args.gpus and rank == 0:
        print('bench.py: --gpus %d but WORLD_SIZE=%d; reporting n_gpus=%d'
              % (args.gpus, world, world), file=sys.stderr)
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    force_dist = os.environ.get('ASR_FORCE_ALLREDUCE') == '1'   # exercise RCCL at world 1 (tests)
    if world > 1 or force_dist:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)

    import __graft_entry__
    __graft_entry__.build()
    from asr_study_amd import ops
    from asr_study_amd.core import models, optimizers
    from asr_study_amd.preprocessing import audio

    N, F, H, L, C = cfg['N'], cfg['F'], cfg['H'], cfg['L'], cfg['C']
    factory = getattr(models, cfg['model'])
    model = factory(num_features=F, num_classes=C, num_hiddens=H, num_layers=L,
                    dropout=args.dropout, weight_decay=1e-4, seed=0, device=dev)
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    feat = audio.MFCC(device=dev) if cfg['feat'] == 'mfcc' else audio.LogFbank(num_filt=80, device=dev)

    # ---- synthetic inputs, resident in HBM before the timed region
    sig = np.empty(N * SAMPLES, np.float32)
    for i in range(N):
        sig[i * SAMPLES:(i + 1) * SAMPLES] = np.random.RandomState(1000 * rank + i).randn(SAMPLES)
    audio_d = torch.from_numpy(sig).to(dev)
    offs = (torch.arange(N, dtype=torch.int32) * SAMPLES).to(dev)
    lens = torch.full((N,), SAMPLES, dtype=torch.int32, device=dev)
    host_lens = [SAMPLES] * N
    rs = np.random.RandomState(77 + rank)
    lab_len = rs.randint(2, 50, size=N)
    lab = np.zeros((N, 49), np.int32)
    for n in range(N):
        lab[n, :lab_len[n]] = rs.randint(0, 25, size=lab_len[n])
    lab_d = torch.from_numpy(lab).to(dev)
    lab_len_d = torch.from_numpy(lab_len.astype(np.int32)).to(dev)

    lstm_ev = {'lstm_seq_fwd': [], 'lstm_seq_bwd': [], 'gemm_hl': [], 'gemm': []}
    conv_ev = []           # (event, event, algorithmic flops, role) of the asr_conv2d_* calls
    gemm_side = {}         # id(start event) -> launched on the side stream (beside a compact BPTT)
    compact_ev = []        # BPTT launches in the compact geometry (asr_lstm_args.compact)
    main_stream = torch.cuda.current_stream(dev)

    def _timed_conv(role):
        orig = getattr(ops.Conv2d, role)

        def timed(self, *a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = orig(self, *a, **k)
            e1.record()
            g = self.args
            conv_ev.append((e0, e1, 2.0 * self.T_out * g.n_pad * self.F_out * g.C_out *
                            g.kt * g.kf * g.C_in, role))
            return r
        return orig, timed

    def _timed(name):
        orig = getattr(ops, name)

        def timed(*a, **k):
            # HIP events on the stream the kernel is launched on (torch's current stream --
            # also inside the engine's side-stream blocks)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = orig(*a, **k)
            e1.record()
            if name.startswith('gemm'):
                # positional (A, B, C, M, N, K): algorithmic flops of the launch
                lstm_ev[name].append((e0, e1, 2.0 * a[3] * a[4] * a[5]))
                # launches on the engine's side stream share the chip with a compact BPTT
                gemm_side[id(e0)] = torch.cuda.current_stream(dev) != main_stream
            else:
                # a layer's recurrence may be launched in slices (asr_lstm_args.step_count)
                steps = k.get('steps')
                lstm_ev[name].append((e0, e1, int(steps[1]) if steps else None))
                if k.get('compact'):
                    compact_ev.append((e0, e1))
            return r
        return orig, timed

    def step(record=False):
        slab, frames = feat.batch_device(audio_d, offs, lens, host_lens)
        if record:
            saved = {}
            for name in lstm_ev:
                saved[name], wrapped = _timed(name)
                setattr(ops, name, wrapped)
            saved_c = {}
            for role in ('fwd', 'dgrad', 'wgrad'):
                saved_c[role], wrapped = _timed_conv(role)
                setattr(ops.Conv2d, role, wrapped)
            try:
                return model.train_step_device(slab, lab_d, lab_len_d, frames, N, world)
            finally:
                for name, fn in saved.items():
                    setattr(ops, name, fn)
                for role, fn in saved_c.items():
                    setattr(ops.Conv2d, role, fn)
        return model.train_step_device(slab, lab_d, lab_len_d, frames, N, world)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = None
    for _ in range(args.steps):
        out = step(record=True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    # the persistent kernels must not have abandoned a spin -- on ANY rank (a timed-out step is
    # vetoed on every rank through the flag slots of the gradient all-reduce; a run with one is
    # not a measurement)
    timeouts = int(ops.lstm_timeout_flags(dev).ne(0).sum().item()) + int(model.fallbacks)
    ranks_seen = 1
    if world > 1 or force_dist:
        # through the product's own communicator (asr_comm_*): what the gradients travel on
        from asr_study_amd import parallel
        t = torch.tensor([float(timeouts), 1.0], dtype=torch.float32, device=dev)
        parallel.grad_comm(dev).allreduce_sum_(t)
        timeouts, ranks_seen = int(t[0].item()), int(t[1].item())
        assert ranks_seen == world, 'RCCL saw %d ranks, WORLD_SIZE is %d' % (ranks_seen, world)
    assert timeouts == 0, ('%d recurrent-kernel timeout(s) / fallback(s) during the timed steps: '
                           'not a valid measurement' % timeouts)
    for name in ('lstm_fwd', 'lstm_bwd'):
        ops.lstm_status(ops.WS.get(name, 0, dev))
    ctc = out[0].cpu().numpy()
    assert np.all(np.isfinite(ctc)), 'non-finite CTC loss in the benchmark step'
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out, model)

    extra = {'fallbacks': timeouts, 'ranks_seen_by_rccl': ranks_seen}
    # modelled cost of the step's ONE gradient all-reduce over xGMI at 8 ranks (7 links x ~153
    # GB/s per GPU, point to point): a ring moves 2 (n-1)/n S over one link per direction; a
    # direct reduce-scatter + all-gather uses all 7
    gbytes = (model.n_params + 4) * 4
    extra['allreduce_model'] = {
        'bytes': gbytes, 'schedule': 'one collective over the flat buffer after BPTT where a '
        'recurrence fills the chip (ASR_AR_OVERLAP=auto), per-layer async beside BPTT otherwise',
        'ring_8gpu_ms': round(2.0 * 7 / 8 * gbytes / 77e9 * 1e3, 3),
        'direct_8gpu_ms': round(2.0 * 7 / 8 * gbytes / (7 * 77e9) * 1e3, 3)}
    if world > 1 and args.full:
        # ---- bus bandwidth of the gradient all-reduce (outside the timed region): the flat
        # fp32 gradient buffer, as one collective; bus = 2 (n-1)/n * bytes / time
        g = model._gbuf
        from asr_study_amd import parallel
        comm = parallel.grad_comm(dev)          # asr_comm_*: RCCL behind the C ABI
        for _ in range(2):
            comm.allreduce_sum_(g)
        torch.cuda.synchronize()
        dist.barrier()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        reps = 5
        for _ in range(reps):
            comm.allreduce_sum_(g)
        e1.record()
        torch.cuda.synchronize()
        ar_ms = torch.tensor([e0.elapsed_time(e1) / reps], dtype=torch.float64, device=dev)
        dist.all_reduce(ar_ms, op=dist.ReduceOp.MAX)
        model._gbuf[model.n_params:].zero_()
        nbytes = g.numel() * 4
        extra['allreduce'] = {
            'bytes': nbytes, 'ms': round(float(ar_ms.item()), 4),
            'bus_GBps': round(2.0 * (world - 1) / world * nbytes / (float(ar_ms.item()) * 1e-3) / 1e9, 2),
            'backend': 'rccl through the C ABI (asr_comm_allreduce_sum)', 'note': 'one fp32 all-reduce of the flat '
            'gradient buffer (+ the timeout-flag slots), exactly as the step issues it'}
    if rank == 0 and args.full:
        # ---- secondary roofline figures (outside the timed region): the gate GEMM of
        # a middle layer and the CTC loss+gradient, each timed with HIP events
        T0 = 999
        n_pad0 = ops.pad16(N)
        rows = T0 * n_pad0

        def ev_time(fn, reps=5):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps
        xg = torch.randn(rows, 2 * H, device=dev)
        wg = torch.randn(2 * H, 8 * H, device=dev) * 0.05
        zg = torch.empty(rows, 8 * H, device=dev)
        gf = 2.0 * rows * 8 * H * 2 * H
        exact = os.environ.get('ASR_GEMM_PREC', '1') == '0'
        packed = model.packed
        t_pack = None
        if packed:
            # operands converted once (asr_pack_hl), then the plain fp16 x 3 GEMM (asr_gemm_hl)
            pa, pb = ops.HlPlanes(rows, 2 * H, dev), ops.HlPlanes(8 * H, 2 * H, dev)
            one = torch.ones(1, device=dev)
            ops.pack_hl(wg, 2 * H, 8 * H, absmax=ops.absmax(wg), c=pb)
            t_pack = ev_time(lambda: ops.pack_hl(xg, rows, 2 * H, absmax=one, r=pa))
            tg = ev_time(lambda: ops.gemm_hl(pa, pb, zg, rows, 8 * H, 2 * H))
        else:
            tg = ev_time(lambda: ops.gemm(xg, wg, zg, rows, 8 * H, 2 * H))
        # split-fp16: every fp32 product is three fp16 MFMAs, so the matrix pipes execute
        # 3x the algorithmic flops; the roofline is the dense fp16 MFMA peak
        mult, peak = (1, PEAK_F32_MFMA_TFLOPS) if exact else (3, PEAK_F16_MFMA_TFLOPS)
        extra['roofline_gate_gemm'] = {
            'kernel': '%s %dx%dx%d (x@W, one BiLSTM layer)' % (
                'gemm_f32_mfma_kernel' if exact else
                'gemm_hlp_kernel<4,4,2>' if packed else 'gemm_f16x2_fast_kernel', rows, 8 * H, 2 * H),
            'pack_ms': None if t_pack is None else round(t_pack, 4),
            'bound': 'mfma', 'achieved': round(mult * gf / tg / 1e9, 2), 'peak': peak,
            'unit': 'TFLOP/s', 'frac': round(mult * gf / tg / 1e9 / peak, 4),
            'algorithmic_fp32_tflops': round(gf / tg / 1e9, 2),
            'vs_fp32_mfma_peak': round(gf / tg / 1e9 / PEAK_F32_MFMA_TFLOPS, 4),
            'avg_launch_ms': round(tg, 4),
            'note': 'achieved = executed MFMA flop/s on the pipe in use (split-fp16: 3 fp16 MFMAs '
                    'per fp32 product, fp32 accumulate, vs the dense fp16 peak); '
                    'algorithmic_fp32_tflops = 2*M*N*K / time'}
        lg = torch.randn(T0, n_pad0, C, device=dev)
        gg = torch.empty_like(lg)
        sl0 = torch.full((N,), T0, dtype=torch.int32, device=dev)
        tc = ev_time(lambda: ops.ctc_loss_grad(lg, lab_d, lab_len_d, sl0, N, grad=gg,
                                               grad_scale=1.0 / N))
        cb = 2.0 * T0 * N * C * 4
        extra['roofline_ctc'] = {
            'kernel': 'ctc_logsoftmax + ctc_alpha_beta + ctc_grad (T=%d, N=%d, C=%d)' % (T0, N, C),
            'bound': 'hbm', 'achieved': round(cb / tc / 1e6, 2), 'peak': PEAK_HBM_GBS,
            'unit': 'GB/s', 'frac': round(cb / tc / 1e6 / PEAK_HBM_GBS, 5),
            'avg_ms': round(tc, 4), 'share_of_step': round(tc / (dt / args.steps * 1e3), 4),
            'algorithmic_bytes': cb, 'traffic': _pmc_traffic(args.config).get('ctc'),
            'note': 'LATENCY-bound, not HBM-bound: a 999-step dependent recursion per utterance '
                    '(>= 1 log-sum-exp per step); the north-star 60 % HBM target is not '
                    'reachable for a sequential recursion (DESIGN.md 8) and the kernel is '
                    'about 1 % of the step'}
        del xg, wg, zg, lg, gg
        pa = pb = None
    if rank == 0:
        T = model.out_frames(999)       # frames the recurrent stack sees (500 behind the conv)
        n_pad = ops.pad16(N)
        ms = dt / args.steps * 1e3
        value = world * N * 10.0 / (dt / args.steps)

        def lstm_times(name):
            ev = lstm_ev[name]
            if not ev:
                return None, None, None
            tot = float(sum(a.elapsed_time(b) for a, b, _ in ev))
            steps = float(sum(T if n is None else n for _, _, n in ev))
            return tot / len(ev), tot, steps        # ms per launch, total ms, total steps
        fwd_t, bwd_t = lstm_times('lstm_seq_fwd'), lstm_times('lstm_seq_bwd')
        cmp_ids = {id(a) for a, _ in compact_ev}
        bwd_cmp = [(a, b, n) for a, b, n in lstm_ev['lstm_seq_bwd'] if id(a) in cmp_ids]
        bwd_def = [(a, b, n) for a, b, n in lstm_ev['lstm_seq_bwd'] if id(a) not in cmp_ids]

        def us_step(evs):
            if not evs:
                return None
            return round(sum(a.elapsed_time(b) for a, b, _ in evs) * 1e3 /
                         sum(T if n is None else n for _, _, n in evs), 3)
        # dominant kernels: the persistent recurrent kernels (one launch per layer and
        # pass, both directions).  Algorithmic flops per launch = 2*T*n_pad*2 dirs*H*4H
        # (h@U forward, dz@U^T in BPTT); algorithmic HBM bytes per launch:
        # fwd reads zx, writes y+cell+gates; bwd reads dy+gates+cell, writes dz.
        flops = 2.0 * T * n_pad * 2 * H * 4 * H
        slab_b = 4.0 * T * n_pad * 2 * H
        alg_bytes = {'fwd': 4 * slab_b + slab_b + slab_b + 4 * slab_b,
                     'bwd': slab_b + 4 * slab_b + slab_b + 4 * slab_b}
        pmc = _pmc_traffic(args.config)

        rec_exact = os.environ.get('ASR_LSTM_PREC', '1') == '0'

        def roof(kind, times, kernel):
            # The recurrences are LATENCY-bound (T dependent steps, one cross-workgroup hand-off
            # each): the figure of merit is us_per_timestep.  `achieved` / `peak` / `frac` are the
            # flop/s the matrix pipe EXECUTES against the peak of the pipe it runs on -- split
            # fp16: 3 v_mfma_f32_16x16x32_f16 per fp32 product vs the 2.5 PF dense-fp16 peak,
            # which is what the PMC's SQ_VALU_MFMA_BUSY_CYCLES measures (profiles/*_pmc_step_*);
            # the algorithmic fp32 rate against the fp32-MFMA peak (SURVEY 8d's yardstick, 3x
            # easier to "reach" on fp16 pipes) is kept under its own, explicitly named keys.
            mult, peak = (1, PEAK_F32_MFMA_TFLOPS) if rec_exact else (3, PEAK_F16_MFMA_TFLOPS)
            per_launch_ms, tot_ms, tot_steps = times
            if not tot_ms:
                return {'kernel': kernel, 'bound': 'latency (hand-off)', 'achieved': None,
                        'peak': peak, 'unit': 'TFLOP/s', 'frac': None, 'traffic': None}
            # a launch covers steps_per_launch of the layer's T dependent steps: its share
            # of the layer's algorithmic flops / bytes / PMC traffic is that fraction
            share = tot_steps / T / (tot_ms / per_launch_ms)      # avg fraction of a layer
            alg = flops * (tot_steps / T) / (tot_ms * 1e-3) / 1e12
            return {'kernel': kernel, 'bound': 'latency (hand-off)',
                    'achieved': round(mult * alg, 3), 'peak': peak, 'unit': 'TFLOP/s',
                    'frac': round(mult * alg / peak, 4),
                    'pipe': 'fp32 MFMA' if rec_exact else 'fp16 MFMA (3 per fp32 product)',
                    'algorithmic_fp32_tflops': round(alg, 3),
                    'algorithmic_vs_fp32_mfma_peak': round(alg / PEAK_F32_MFMA_TFLOPS, 4),
                    'traffic': round(pmc[kind] * share, 1) if kind in pmc else None,
                    'algorithmic_bytes': round(alg_bytes[kind] * share, 1),
                    'hbm_GBps': round(alg_bytes[kind] * (tot_steps / T) / (tot_ms * 1e-3) / 1e9, 1),
                    'avg_launch_ms': round(per_launch_ms, 4),
                    'steps_per_launch': round(tot_steps / (tot_ms / per_launch_ms), 1),
                    'us_per_timestep': round(tot_ms * 1e3 / tot_steps, 3),
                    'flops_per_launch': flops * share,
                    'note': 'latency-bound recurrence (T dependent steps, cross-workgroup '
                            'hand-off per step; a layer may be launched in slices when its '
                            'neighbouring GEMMs are pipelined): DESIGN.md 5.  achieved = executed '
                            'MFMA flop/s on the pipe in use; traffic = PMC bytes per launch '
                            '(profiles/pmc_traffic.json)'}
        split = os.environ.get('ASR_GEMM_PREC', '1') != '0' or os.environ.get('ASR_LSTM_PREC', '1') != '0'

        def gemm_roof():
            # every big GEMM of the step (x@W, dz@W^T, x^T dz, h^T dz, Dense), timed in place.
            # achieved / frac / avg_launch_ms / ms_per_step are taken over ALL launches of the
            # family.  Launches on the side stream run on the CUs a compact BPTT leaves free (128
            # of 256 at cfg3) or queue behind it: their durations are wall time on a SHARED chip;
            # the launches that have the chip to themselves (main stream) are `chip_owning`, the
            # others `shared` -- two subsets of the same sum, not a different definition of it.
            ev_all = lstm_ev['gemm_hl'] + lstm_ev['gemm']
            if not ev_all:
                return None
            ev = [e for e in ev_all if not gemm_side.get(id(e[0]))]
            ev_side = [e for e in ev_all if gemm_side.get(id(e[0]))]
            exact = os.environ.get('ASR_GEMM_PREC', '1') == '0'
            mult, peak = (1, PEAK_F32_MFMA_TFLOPS) if exact else (3, PEAK_F16_MFMA_TFLOPS)
            packed = len(lstm_ev['gemm_hl']) > 0

            def subset(evs):
                if not evs:
                    return None
                tot = float(sum(a.elapsed_time(b) for a, b, _ in evs))
                fl = float(sum(f for _, _, f in evs))
                ach = mult * fl / (tot * 1e-3) / 1e12
                return {'achieved': round(ach, 2), 'frac': round(ach / peak, 4),
                        'algorithmic_fp32_tflops': round(fl / (tot * 1e-3) / 1e12, 2),
                        'launches_per_step': round(len(evs) / float(args.steps), 1),
                        'avg_launch_ms': round(tot / len(evs), 4),
                        'ms_per_step': round(tot / args.steps, 3),
                        'algorithmic_tflop_per_step': round(fl / args.steps / 1e12, 3)}
            r = {'kernel': ('gemm_hlx_kernel<4,4,2> / gemm_hlp_kernel<4,4,2> (256x256 tile, K-major / '
                            'persistent row-major; operands packed once into split-fp16 planes)'
                            if packed else
                            'gemm_f32_mfma_kernel' if exact else 'gemm_f16x2_fast_kernel') +
                           ': all GEMM launches of the step',
                 'bound': 'mfma', 'peak': peak, 'unit': 'TFLOP/s', 'traffic': pmc.get('gemm')}
            r.update(subset(ev_all))
            r['chip_owning'] = subset(ev)
            r['shared'] = subset(ev_side)
            r['note'] = ('achieved = executed MFMA flop/s (split-fp16: 3 fp16 MFMAs per fp32 product) '
                         'summed over ALL launches of the family / their summed HIP-event durations, vs '
                         'the dense fp16 MFMA peak.  chip_owning = the main-stream launches (x@W, dX, '
                         'the bottom layer\'s gradients, Dense); shared = the K-major weight-gradient '
                         'launches on the side stream beside the compact BPTT of the layer below '
                         '(wall time on half of a power-capped chip).  Alone on the chip x@W runs at '
                         'roofline_gate_gemm.frac.  PMC: profiles/r6*_pmc_step_cfg3.md; the power-cap '
                         'analysis: DESIGN.md 6')
            return r
        line = {
            'metric': 'audio-seconds/sec trained (MFCC+BiLSTM+CTC)',
            'value': round(value, 1), 'unit': 'audio-seconds/s', 'n_gpus': world,
            'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(ms, 3),
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
            'dtype': 'f32 (products: split-f16 hi+lo MFMA)' if split else 'f32',
            'data': 'synthetic',
            'arithmetic': ('fp32 storage and accumulation; matrix products as split-fp16 (hi+lo) '
                           'MFMAs, 2^-22 relative error per product (parity tolerance 1e-4, pinned '
                           'at T=999 by tests/test_gpu_fullsize_parity.py); ASR_LSTM_PREC=0 '
                           'ASR_GEMM_PREC=0 selects exact fp32 MFMA (see exact_fp32)')
            if split else 'exact fp32 MFMA everywhere',
            'config': {'workload': '%s: %s' % (args.config, cfg['desc']),
                       'baseline_config': {
                           'cfg3': 'configs[2] minus its conv front-end (BASELINE.md 3 / north-star '
                                   'targets); as written -> as_written / cfg3_conv',
                           'cfg3_conv': 'configs[2] as written',
                           'cfg2': 'configs[1]'}.get(args.config, args.config),
                       'global_batch': world * N, 'utterance_seconds': 10.0, 'frames': T,
                       'dropout': args.dropout, 'optimizer': 'adam(clipnorm=400)',
                       'parallelism': 'dp%d' % world, 'params': model.count_params()},
            'roofline': roof('bwd', bwd_t, '%s (persistent BPTT of one BiLSTM layer, both '
                                            'directions)' % _rec_kernel_name(H, True)),
            'roofline_lstm_fwd': roof('fwd', fwd_t, '%s (persistent forward recurrence of one '
                                                     'BiLSTM layer)' % _rec_kernel_name(H, False)),
        }
        if bwd_cmp:
            line['roofline']['geometry'] = {
                'compact_launches_per_step': round(len(bwd_cmp) / float(args.steps), 2),
                'compact_us_per_timestep': us_step(bwd_cmp),
                'default_launches_per_step': round(len(bwd_def) / float(args.steps), 2),
                'default_us_per_timestep': us_step(bwd_def),
                'note': 'compact = lstm_bwd_kernel_c<.., NBLK = 2>: H/32 workgroups per chain, half '
                        'of the CUs, with the weight-gradient GEMMs of the layer above on the other '
                        'half (wall time per step INCLUDES that sharing); default = the layer with '
                        'nothing to run beside it (the top one) on the whole chip'}
        line.update(extra)
        line['allreduce_model']['ring_share_of_step'] = round(
            line['allreduce_model']['ring_8gpu_ms'] / ms, 4)
        # `roofline` is the family with the largest share of the step: the BPTT recurrence, the
        # forward recurrence or the GEMMs (all three stay in the line under their own keys)
        gr = gemm_roof()
        if gr is not None:
            line['roofline_gemm_step'] = gr
            # (GPU time per step of each family, all launches)
            shares = {'roofline_gemm_step': gr['ms_per_step'],
                      'roofline_lstm_fwd': (fwd_t[1] or 0.0) / args.steps,
                      'roofline_lstm_bwd': (bwd_t[1] or 0.0) / args.steps}
            line['roofline_lstm_bwd'] = line['roofline']
            top = max(shares, key=shares.get)
            line['roofline'] = dict(line[top], dominant_of={k: round(v, 3) for k, v in shares.items()})
        if conv_ev:
            # K13: the convolution front-end's three entry points (band build, packs, the
            # segmented / K-major GEMMs, activation, band fold), HIP events in place
            tot = float(sum(a.elapsed_time(b) for a, b, _, _ in conv_ev))
            fl = float(sum(f for _, _, f, _ in conv_ev))
            per_role = {}
            for a, b, f, role in conv_ev:
                t_, f_ = per_role.get(role, (0.0, 0.0))
                per_role[role] = (t_ + a.elapsed_time(b), f_ + f)
            mult, peak = (3, PEAK_F16_MFMA_TFLOPS)
            line['roofline_conv'] = {
                'kernel': 'asr_conv2d_{fwd,dgrad,wgrad}: banded-matrix form on gemm_hlx_kernel '
                          '(segmented reduction over the time taps; K-major per tap for dW)',
                'bound': 'mfma', 'achieved': round(mult * fl / (tot * 1e-3) / 1e12, 2),
                'peak': peak, 'unit': 'TFLOP/s',
                'frac': round(mult * fl / (tot * 1e-3) / 1e12 / peak, 4),
                'algorithmic_fp32_tflops': round(fl / (tot * 1e-3) / 1e12, 2),
                'ms_per_step': round(tot / args.steps, 3),
                'algorithmic_tflop_per_step': round(fl / args.steps / 1e12, 4),
                'per_role_ms': {r: round(t_ / args.steps, 3) for r, (t_, _) in per_role.items()},
                'per_role_algorithmic_tflops': {r: round(f_ / (t_ * 1e-3) / 1e12, 1)
                                                for r, (t_, f_) in per_role.items()},
                'traffic': pmc.get('conv'),
                'note': 'achieved = 3 x the ALGORITHMIC convolution flops (2 M Ko kt kf Ci per '
                        'pass; split-fp16) / time of the whole entry point.  The banded form '
                        'multiplies more than those flops on the matrix pipes: the band of a '
                        'time tap is kf / F_in dense (layer 1: 41 of 80 -> ~2x), cut by the '
                        'frequency blocks where the channel count allows (layer 2: ~1.3x), '
                        'so the pipes are busier than `frac` says'}
        if world == 1 and args.full and not args.no_extras:
            if args.config == 'cfg3':
                line['cfg3_conv'] = _sub_bench('cfg3_conv', {}, args.steps, args.warmup, args.dropout)
                # BASELINE.json configs[2] AS WRITTEN ("5xBiLSTM(512) + 2 conv front-end"): the
                # headline stays the stack without it (the north-star targets' configuration,
                # twice the recurrent steps per audio second, continuous since round 1)
                line['as_written'] = {
                    k: line['cfg3_conv'].get(k) for k in ('value', 'unit', 'ms_per_step', 'workload')}
                line['as_written']['note'] = ('BASELINE.json configs[2] as written; the headline '
                                              '`value` is the same stack WITHOUT the conv front-end')
            line['cfg2'] = _sub_bench('cfg2', {}, args.steps, args.warmup, args.dropout)
            # the reference's default topology is bounded by its batch of 32 (a quarter of the
            # CUs for 85 % of the step): the same model at a batch that fills the chip
            line['cfg2_n128'] = _sub_bench('cfg2_n128', {}, max(5, args.steps // 2), args.warmup,
                                           args.dropout)
            line['exact_fp32'] = _sub_bench(args.config, {'ASR_LSTM_PREC': '0', 'ASR_GEMM_PREC': '0'},
                                            max(3, args.steps // 2), 2, args.dropout)
            try:
                line['predict_latency'] = predict_latency(dev)
            except Exception as e:                # a companion figure never fails the bench
                line['predict_latency'] = {'error': repr(e)[:300]}
            try:
                slab_e, _ = feat.batch_device(audio_d, offs, lens, host_lens)
                line['eval_beam'] = eval_beam(dev, model, slab_e, N, slab_e.shape[0])
            except Exception as e:
                line['eval_beam'] = {'error': repr(e)[:300]}
            try:
                line['dataset_build'] = dataset_build(dev, feat)
            except Exception as e:
                line['dataset_build'] = {'error': repr(e)[:300]}
        if world == 1 and args.full and not args.no_cpu_baseline:
            line['cpu_baseline'] = cpu_baseline(cfg)
        if args.emit == 'detail':
            print(json.dumps(line))
        else:
            emit(line)
    if world > 1 or force_dist:
        dist.barrier()
        dist.destroy_process_group()
    return 0


DUMP_SAMPLE = 1 << 20             # parameters / gradients sampled into the dump (4 MB each)


def dump_outputs(path, out, model):
    """What the last timed step handed its caller, as float32 .npy files: the per-utterance CTC
    loss, the greedy decode (-1 padded) and its lengths, and the same DUMP_SAMPLE entries
    (RandomState(0), sorted, distinct) of the updated flat parameters and of the step's
    gradients; `sample_index` names those entries."""
    os.makedirs(path, exist_ok=True)
    ctc, dec, dlen = out
    arrays = {'ctc_loss': ctc, 'greedy_decode': dec, 'greedy_decode_len': dlen}
    n = model.n_params
    idx = np.arange(n) if n <= DUMP_SAMPLE else np.unique(
        np.random.RandomState(0).randint(0, n, size=DUMP_SAMPLE))
    import torch
    idx_d = torch.from_numpy(idx).to(model.params.device)
    arrays['params_sample'] = model.params.index_select(0, idx_d)
    arrays['grads_sample'] = model.grads.index_select(0, idx_d)
    arrays['sample_index'] = torch.from_numpy(idx.astype(np.float64))
    for name, a in arrays.items():
        a = a.detach().cpu().numpy()
        np.save(os.path.join(path, name + '.npy'),
                a.astype(np.float64 if a.dtype == np.float64 else np.float32))


def _cpu_stub(args, rank, world):
    """Launch-contract check without a GPU (tests/test_bench_launch.py): every rank joins a
    gloo group, rank 0 prints the line's launch-related fields.  Measures nothing."""
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group('gloo', rank=rank, world_size=world)
        t = torch.ones(1)
        dist.all_reduce(t)
        assert int(t.item()) == world
    if rank == 0:
        print(json.dumps({'stub': True, 'n_gpus': world, 'steps': args.steps,
                          'warmup': args.warmup, 'gpus_arg': args.gpus}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
