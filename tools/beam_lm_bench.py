"""Cost of the character LM in the device beam search, and host against device with it.

1. ops.ctc_beam_search_lm against ops.ctc_beam_search on the same 64 x 999 x 28 slab at widths
   100 and 400, order 3: median / min / max of 10 calls after 2 of warm-up, and the phase counters
   of utterance 0 of both (asr_ctc_beam[_lm]_device_counters).
2. tools/beam_crossover.py's method with the LM: seconds per batch of N utterances on the device
   and on the host decoder, with the process confined to 16 host threads.

Run from the repository root on a machine with one MI355X; prints one JSON object per line."""
import json
import os
import sys
import time

os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:16])      # 16 usable host threads
sys.path.insert(0, os.getcwd())
import numpy as np      # noqa: E402
import torch            # noqa: E402
from asr_study_amd import ops               # noqa: E402
from asr_study_amd.lm import CharLM         # noqa: E402

T, C, ORDER = 999, 28, 3
rs = np.random.RandomState(0)
lm = CharLM.estimate([rs.randint(0, C - 1, size=rs.randint(5, 40)).tolist() for _ in range(400)],
                     C - 1, ORDER)
w, wd = lm.fused(1.0, 0.0), lm.fused_device(1.0, 0.0, 'cuda:0')


def timed(f, n=10, warm=2):
    ts = []
    for _ in range(n + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = ts[warm:]
    return dict(median=float(np.median(ts)), min=min(ts), max=max(ts))


def slab(N):
    lg = torch.from_numpy((rs.randn(T, ops.pad16(N), C) * 2).astype(np.float32)).cuda()
    return lg, torch.full((N,), T, dtype=torch.int32, device='cuda')


N = 64
lg, sl = slab(N)
for W in (100, 400):
    plain = timed(lambda: ops.ctc_beam_search(lg, sl, N, W))
    plain_c = ops.ctc_beam_counters(lg.shape, N, W, 0, lg.device)
    with_lm = timed(lambda: ops.ctc_beam_search_lm(lg, sl, N, W, True, wd, ORDER))
    lm_c = ops.ctc_beam_lm_counters(lg.shape, N, W, 0, lg.device)
    print(json.dumps(dict(what='lm_cost', N=N, width=W, plain=plain, lm=with_lm,
                          ratio=with_lm['median'] / plain['median'], plain_counters=plain_c,
                          lm_counters=lm_c)), flush=True)
for N in (16, 64, 256):
    lg, sl = slab(N)
    host_in = lg.cpu().numpy()
    for W in (100, 400):
        d = timed(lambda: ops.ctc_beam_search_lm(lg, sl, N, W, True, wd, ORDER), 3, 1)
        h = timed(lambda: ops.ctc_beam_search_lm_host(host_in, [T] * N, N, W, True, w, ORDER), 3, 1)
        hp = timed(lambda: ops.ctc_beam_search_host(host_in, [T] * N, N, W, True), 3, 1)
        print(json.dumps(dict(what='crossover', N=N, width=W, host_threads=len(os.sched_getaffinity(0)),
                              device_lm=d['median'], host_lm=h['median'],
                              host_plain=hp['median'])), flush=True)
