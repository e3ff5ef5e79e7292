"""CTC forced alignment (K19, asr_ctc_align) against the alpha chain alone (asr_ctc_loss_grad with
grad = NULL) at T = 999, N = 64, C = 29, 100 .. 150 labels per utterance (PPL 4).

    python tools/ctc_align_bench.py                  the two call times, alternating, same process:
                                                     median of 5 rounds with min - max, one JSON line
    python tools/ctc_align_bench.py --calls 50       50 calls of each and nothing else: the program
                                                     to put behind a kernel trace (per-kernel times,
                                                     the backtrace's share)
    python tools/ctc_align_bench.py --stats DIR      per-kernel table from the kernel-stats csv of
                                                     such a trace

Call times are device events around ``reps`` back-to-back calls on one stream (the label checks
of ops.ctc_align synchronise with the host, so the C entry point is called directly)."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

T, N, CLS, L_LO, L_HI = 999, 64, 29, 100, 150


def setup():
    import torch
    from asr_study_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    logits = torch.from_numpy((3.0 * rs.randn(T, N, CLS)).astype(np.float32)).to(dev)
    lens = rs.randint(L_LO, L_HI + 1, size=N)
    lab = np.zeros((N, L_HI), np.int32)
    for n, ln in enumerate(lens):
        lab[n, :ln] = rs.randint(0, CLS - 1, size=ln)
    lab_d = torch.from_numpy(lab).to(dev)
    ll = torch.from_numpy(lens.astype(np.int32)).to(dev)
    sl = torch.full((N,), T, dtype=torch.int32, device=dev)
    path = torch.empty((N, T), dtype=torch.int32, device=dev)
    score = torch.empty(N, dtype=torch.float32, device=dev)
    loss = torch.empty(N, dtype=torch.float32, device=dev)
    nb_a = lib.asr_ctc_align_workspace_bytes(T, N, N, CLS, L_HI)
    nb_l = lib.asr_ctc_workspace_bytes(T, N, N, CLS, L_HI)
    ws_a = torch.empty(nb_a, dtype=torch.uint8, device=dev)
    ws_l = torch.empty(nb_l, dtype=torch.uint8, device=dev)
    p = ops._ptr
    keep = (logits, lab_d, ll, sl, path, score, loss, ws_a, ws_l)

    def align():
        _lib.check(lib.asr_ctc_align(p(logits), p(lab_d), p(ll), p(sl), T, N, N, CLS, L_HI,
                                     p(path), p(score), p(ws_a), nb_a, ops._stream()), 'align')

    def alpha():
        _lib.check(lib.asr_ctc_loss_grad(p(logits), p(lab_d), p(ll), p(sl), T, N, N, CLS, L_HI,
                                         1.0, p(loss), None, p(ws_l), nb_l, ops._stream()), 'loss')

    word = 1 if L_HI <= 127 else (2 if L_HI <= 255 else 4)
    return torch, align, alpha, keep, dict(bp_bytes=int(N * T * 64 * word), ws_bytes=int(nb_a))


def timed(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def bench(rounds, reps):
    torch, align, alpha, keep, info = setup()
    for _ in range(20):
        align()
        alpha()
    torch.cuda.synchronize()
    ta, tl = [], []
    for _ in range(rounds):
        ta.append(timed(torch, align, reps))
        tl.append(timed(torch, alpha, reps))
    out = dict(shape=dict(T=T, N=N, C=CLS, labels=[L_LO, L_HI]), rounds=rounds, reps=reps,
               align_ms=dict(median=float(np.median(ta)), min=min(ta), max=max(ta)),
               alpha_chain_ms=dict(median=float(np.median(tl)), min=min(tl), max=max(tl)),
               ratio=float(np.median(ta) / np.median(tl)), **info)
    print(json.dumps(out))
    return out


def calls(k):
    torch, align, alpha, keep, info = setup()
    for _ in range(k):
        align()
        alpha()
    torch.cuda.synchronize()


def stats(directory):
    rows = []
    for fn in glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True):
        with open(fn) as f:
            rows += [r for r in csv.DictReader(f) if 'ctc_' in r.get('Name', '')]
    total = {}
    for r in rows:
        name = r['Name']
        for key in ('ctc_lse_kernel', 'ctc_viterbi_kernel', 'ctc_backtrace_kernel',
                    'ctc_alpha_beta_kernel'):
            if key in name:
                c, ns = total.get(key, (0, 0.0))
                total[key] = (c + int(r['Calls']), ns + float(r['TotalDurationNs']))
    for key, (c, ns) in sorted(total.items()):
        print('%-24s %6d calls  %9.1f us per call' % (key, c, ns / c / 1e3))
    if 'ctc_viterbi_kernel' in total and 'ctc_backtrace_kernel' in total:
        v = total['ctc_viterbi_kernel'][1] / total['ctc_viterbi_kernel'][0]
        b = total['ctc_backtrace_kernel'][1] / total['ctc_backtrace_kernel'][0]
        print('backtrace share of (forward + backtrace): %.1f %%' % (100 * b / (v + b)))
    return total


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=300)
    ap.add_argument('--calls', type=int, default=0)
    ap.add_argument('--stats', type=str, default=None)
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
    elif a.calls:
        calls(a.calls)
    else:
        bench(a.rounds, a.reps)
