"""-m gpu: ELEMENT-WISE parity of the HIP path with the float64 oracle at the benchmarked
sizes (T = 999 frames; cfg2 = 5 x BiLSTM(256), N = 32, with and without dropout masks /
ragged lengths; cfg3's topology 5 x BiLSTM(512) on a 16-utterance slice of its batch).

The oracle ran once in the build container (oracle/gen_golden_model.py, minutes per case)
and left compact fixtures in tests/golden/model_<case>{,_grads,_states}.npz; the inputs are seeded recipes
(oracle/fullsize_cases.py) rebuilt here.  Compared, under the DEFAULT arithmetic (split-fp16
products) and under ASR_LSTM_PREC=0 ASR_GEMM_PREC=0 (exact fp32 MFMA):

  logits of 50 frames spread over T, every utterance       atol 1e-4
  layer-1 / layer-5 h and c at t in {0,1,T/2,T-2,T-1}      atol 1e-4
  per-utterance CTC loss                                    rtol 1e-4
  1000 sampled entries of every gradient tensor             atol 1e-4 * max|g| of the tensor
  sums over every 256 contiguous gradient entries (r6:      atol 16e-4 * max|g|
      EVERY entry of every tensor is in one checksum)
  every gradient tensor's L2 norm                           rtol 1e-3
  per-frame argmax (the greedy decoder's decision)          EXACT on every frame the oracle
      decides by more than 2e-4 (twice the activation tolerance; with random-init weights
      ~2 % of the frames are closer than that and could flip legitimately)
  greedy decode (device kernel)                             EXACT vs collapsing the device
      logits' argmax on the host, i.e. exact given the argmax parity above
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import fullsize_cases as FC
from oracle import lstm as OL
from tests.gpu_util import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def _engine_masks(case, model):
    """oracle-layout masks -> {stage index: (B_W (2, n_pad, f_in_pad), B_U (2, n_pad, Hp))}."""
    if case['masks'] is None:
        return None
    cfg = case['cfg']
    N, H, F = cfg['N'], cfg['H'], cfg['F']
    n_pad = (N + 15) // 16 * 16
    out = {}
    stages = [i for i, s in enumerate(model.stages) if s.kind == 'bilstm']
    for li, si in enumerate(stages):
        s = model.stages[si]
        BW = np.ones((2, n_pad, s.f_in_pad), np.float32)
        BU = np.ones((2, n_pad, s.Hp), np.float32)
        for di, d in enumerate(('fwd', 'bwd')):
            bw, bu = case['masks'][li][d]
            if li == 0:
                BW[di, :N, :F] = bw
            else:
                BW[di, :N, :H] = bw[:, :H]
                BW[di, :N, s.Hp:s.Hp + H] = bw[:, H:]
            BU[di, :N, :H] = bu
        out[si] = (torch.from_numpy(BW).cuda(), torch.from_numpy(BU).cuda())
    return out


def _check(name):
    from asr_study_amd import ops
    from asr_study_amd.core import ctc_utils, models
    fix = FC.load_fixture(GOLDEN, name)
    case = FC.build(name)
    cfg, T = case['cfg'], case['T']
    N, F, H, L, C = cfg['N'], cfg['F'], cfg['H'], cfg['L'], cfg['C']
    # the regenerated inputs are the ones the fixture was computed from
    idx, probe = FC.feature_probe(case['x'])
    assert np.abs(probe - fix['feat_probe']).max() < 1e-5
    assert np.array_equal(case['lens'], fix['lens'])
    dev = torch.device('cuda:0')
    if cfg.get('conv'):         # configs[2] as written: the stack behind its 2-conv front-end
        model = models.deep_speech2(num_features=F, num_classes=C, num_hiddens=H, num_layers=L,
                                    conv_filters=cfg['conv'][0][0],
                                    conv_kernels=[c[1:3] for c in cfg['conv']],
                                    conv_strides=[c[3:5] for c in cfg['conv']],
                                    max_value=cfg['conv'][0][5], dropout=0.0, weight_decay=0.0,
                                    seed=1, device=dev)
    else:
        model = models.brsmv1(num_features=F, num_classes=C, num_hiddens=H, num_layers=L,
                              dropout=0.0, weight_decay=0.0, seed=1, device=dev)
    model.set_weights([a for _, a in OL.flatten(case['params'])])
    n_pad = ops.pad16(N)
    slab = torch.zeros((T, n_pad, F), dtype=torch.float32, device=dev)
    slab[:, :N] = torch.from_numpy(case['x']).to(dev)
    ctc, logits, _ = model.loss_and_grads(slab, case['labels'], case['lens'], training=False,
                                          masks=_engine_masks(case, model))
    torch.cuda.synchronize()
    for ws in ('lstm_fwd', 'lstm_bwd'):
        ops.lstm_status(ops.WS.get(ws, 0, dev))
    lg = logits[:, :N].cpu().numpy()
    T = lg.shape[0]                                    # the logits' time axis (T' behind a conv)
    lens_out = FC.out_frames(cfg, case['lens'])
    fr = fix['logit_frames']
    assert report(name + ' logits@50 frames', lg[fr], fix['logits']) < 1e-4
    # hidden / cell states of the first and last BiLSTM layer
    sf = FC.state_frames(T)
    nu = FC.STATE_UTTS
    bl = [i for i, s in enumerate(model.stages) if s.kind == 'bilstm']
    for li, si in ((0, bl[0]), (L - 1, bl[-1])):
        y = model._acts[si]['y'][sf][:, :nu].cpu().numpy()
        c = model._acts[si]['cell'][sf][:, :nu].reshape(len(sf), nu, -1).cpu().numpy()
        assert report('%s h layer %d' % (name, li + 1), y, fix['h_l%d' % li]) < 1e-4
        assert report('%s c layer %d' % (name, li + 1), c, fix['c_l%d' % li]) < 1e-4
    np.testing.assert_allclose(ctc.cpu().numpy(), fix['ctc'], rtol=1e-4)
    # gradients: sampled entries + norms
    names = [str(n) for n in fix['grad_names']]
    got = model.get_gradients()
    assert len(got) == len(names)
    worst, worst_b, nblocks = 0.0, 0.0, 0
    for i, (gname, g) in enumerate(zip(names, got)):
        flat = np.asarray(g, np.float64).reshape(-1)
        want = fix['g%02d_samples' % i]
        norm, gmax = fix['g%02d_stats' % i]
        err = np.abs(flat[FC.grad_sample_index(i, flat.size)] - want).max()
        worst = max(worst, err / max(gmax, 1e-30))
        assert err < 1e-4 * gmax + 1e-9, (gname, err, gmax)
        assert abs(np.sqrt(np.sum(flat ** 2)) - norm) < 1e-3 * norm + 1e-9, gname
        # EVERY entry: sums over blocks of 256 contiguous entries against the oracle's (a
        # per-entry error e moves a block sum by at most 256 e, by ~ sqrt(256) e when the errors
        # are independent: the bound below is the latter at e = 1e-4 max|g|, so one wrong entry
        # of 1.6e-3 max|g|, or a wrong stripe, fails it)
        bs = FC.grad_block_sums(flat)
        wantb = fix['g%02d_blocks' % i].astype(np.float64)
        assert bs.shape == wantb.shape, gname
        berr = np.abs(bs - wantb).max()
        worst_b = max(worst_b, berr / max(gmax, 1e-30))
        assert berr < 1e-4 * gmax * np.sqrt(FC.GRAD_BLOCK) + 1e-9, (gname, berr, gmax)
        nblocks += bs.size
    print('[parity] %-28s worst sampled-gradient error = %.3e x max|g| over %d tensors; worst '
          'block-sum error = %.3e x max|g| over %d blocks of %d (every entry)'
          % (name, worst, len(names), worst_b, nblocks, FC.GRAD_BLOCK))
    # decoder decisions
    am = np.argmax(lg, axis=-1)
    valid = np.arange(T)[:, None] < np.asarray(lens_out)[None, :]
    decided = (fix['margin'] > 2e-4) & valid
    assert np.array_equal(am[decided], fix['argmax'][decided])
    flips = int(np.sum((am != fix['argmax']) & valid))
    print('[parity] %-28s argmax exact on %d decided frames; %d of %d close calls flipped'
          % (name, int(decided.sum()), flips, int((valid & ~decided).sum())))
    hyp = ctc_utils.decode((logits, lens_out), is_greedy=True)
    for n in range(N):
        seq, prev = [], -1
        for t in range(int(lens_out[n])):
            k = int(am[t, n])
            if k != prev and k != C - 1:
                seq.append(k)
            prev = k
        assert hyp[n] == seq, n
        if flips == 0:
            assert seq == fix['greedy'][n, :fix['greedy_len'][n]].tolist()


@pytest.mark.timeout(600)
@pytest.mark.parametrize('name', sorted(FC.CASES))
def test_fullsize_elementwise_parity(name):
    _check(name)


@pytest.mark.timeout(900)
def test_fullsize_elementwise_parity_exact_fp32():
    """The same comparison with every product on the exact-fp32 MFMA instructions (the
    switches are read once per process, hence the child process)."""
    env = dict(os.environ, ASR_LSTM_PREC='0', ASR_GEMM_PREC='0')
    out = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x',
                          '-s', '-k', 'test_fullsize_elementwise_parity and not exact', '-m', 'gpu'],
                         env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         timeout=850, stdin=subprocess.DEVNULL)
    text = out.stdout.decode()
    print(text[-3000:])
    assert out.returncode == 0, text[-3000:]
    assert '%d passed' % len(FC.CASES) in text


_GRAD_DUMP = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, os.environ["ASR_ROOT"])
from oracle import fullsize_cases as FC
from oracle import lstm as OL
from asr_study_amd import ops
from asr_study_amd.core import models
case = FC.build(os.environ["ASR_CASE"])
cfg, T = case["cfg"], case["T"]
N, F, H, L, C = cfg["N"], cfg["F"], cfg["H"], cfg["L"], cfg["C"]
dev = torch.device("cuda:0")
if cfg.get("conv"):
    model = models.deep_speech2(num_features=F, num_classes=C, num_hiddens=H, num_layers=L,
                                conv_filters=cfg["conv"][0][0],
                                conv_kernels=[c[1:3] for c in cfg["conv"]],
                                conv_strides=[c[3:5] for c in cfg["conv"]],
                                max_value=cfg["conv"][0][5], dropout=0.0, weight_decay=0.0,
                                seed=1, device=dev)
else:
    model = models.brsmv1(num_features=F, num_classes=C, num_hiddens=H, num_layers=L, dropout=0.0,
                          weight_decay=0.0, seed=1, device=dev)
model.set_weights([a for _, a in OL.flatten(case["params"])])
slab = torch.zeros((T, ops.pad16(N), F), dtype=torch.float32, device=dev)
slab[:, :N] = torch.from_numpy(case["x"]).to(dev)
ctc, logits, _ = model.loss_and_grads(slab, case["labels"], case["lens"], training=False)
torch.cuda.synchronize()
for ws in ("lstm_fwd", "lstm_bwd"):
    ops.lstm_status(ops.WS.get(ws, 0, dev))
np.savez(os.environ["ASR_DUMP"], ctc=ctc.cpu().numpy(), logits=logits[:, :N].cpu().numpy(),
         **{"g%02d" % i: g for i, g in enumerate(model.get_gradients())})
'''


@pytest.mark.timeout(900)
@pytest.mark.parametrize('case_name', ['cfg3', 'cfg3_conv'])
def test_cfg3_split_fp16_vs_exact_fp32_over_every_gradient_element(tmp_path, case_name):
    """(cfg3_conv: the same stack behind its 2-conv front-end, configs[2] as written -- the
    convolutions' dW / db included, over every element.)
    The headline arithmetic (fp32 operands as fp16 hi + lo, lo*lo dropped, ONE power-of-two
    scale per GEMM operand tensor) against the exact-fp32 MFMA path at FULL cfg3 size (5 x
    BiLSTM(512), 64 x 999 frames), over EVERY element of every gradient tensor, the logits and
    the losses -- not samples.  Bounds:
      * absolute:  |split - exact| <= 1e-5 * max|g| of the tensor  (10x inside the 1e-4 parity bar)
      * RELATIVE, on every entry above 1e-6 * max|g|: this is where a per-tensor scale would show
        (operand elements below 2^-23 * max|x| keep only absolute precision); the worst entry and
        the 99.9th percentile are printed and bounded.
    Each arithmetic runs in its own process (the library reads its switches once)."""
    dumps = {}
    for tag, env_extra in (('split', {}), ('exact', {'ASR_LSTM_PREC': '0', 'ASR_GEMM_PREC': '0'})):
        path = str(tmp_path / (tag + '.npz'))
        env = dict(os.environ, ASR_ROOT=ROOT, ASR_DUMP=path, ASR_CASE=case_name, **env_extra)
        out = subprocess.run([sys.executable, '-c', _GRAD_DUMP], env=env, cwd=ROOT,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=420,
                             stdin=subprocess.DEVNULL)
        assert out.returncode == 0, out.stdout.decode()[-3000:]
        dumps[tag] = np.load(path)
    a, b = dumps['split'], dumps['exact']
    assert report(case_name + ' logits split vs exact (all)', a['logits'], b['logits']) < 2e-5
    np.testing.assert_allclose(a['ctc'], b['ctc'], rtol=2e-6)
    keys = sorted(k for k in a.files if k.startswith('g'))
    worst_abs = worst_rel = worst_p999 = 0.0
    for k in keys:
        ga, gb = a[k].astype(np.float64).ravel(), b[k].astype(np.float64).ravel()
        m = np.abs(gb).max()
        err = np.abs(ga - gb)
        big = np.abs(gb) > 1e-6 * m
        rel = err[big] / np.abs(gb[big])
        p999 = float(np.percentile(rel, 99.9)) if rel.size else 0.0
        print('[parity] %s %s: n=%d max|g|=%.3e abs err %.2e x max; entries > 1e-6 max: %d, '
              'rel err worst %.2e, p99.9 %.2e, median %.2e'
              % (case_name, k, ga.size, m, err.max() / m, int(big.sum()), rel.max() if rel.size else 0.0,
                 p999, float(np.median(rel)) if rel.size else 0.0))
        worst_abs = max(worst_abs, err.max() / m)
        worst_rel = max(worst_rel, rel.max() if rel.size else 0.0)
        worst_p999 = max(worst_p999, p999)
    print('[parity] %s split-fp16 vs exact fp32, all %d tensors: worst abs %.2e x max|g|, worst '
          'relative (entries > 1e-6 max) %.2e, worst p99.9 relative %.2e'
          % (case_name, len(keys), worst_abs, worst_rel, worst_p999))
    assert worst_abs < 1e-5
    assert worst_p999 < 1e-2 and worst_rel < 1.0
