"""-m gpu: CTC forced alignment on the device (K19, asr_ctc_align) against the float64 oracle on
the fixture set F, under the pass conditions of tests/test_ctc_align_host.py (valid path; path
score and returned score within 4 * E32 * max(1, |best|); exact path where the oracle's gap is
>= 1e-2 nats), plus ties, infeasible rows, determinism, a dirty workspace, the untouched loss
kernels, Model.align, and the align.py command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ctc_align_oracle as O
from tests.gpu_util import dev, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(case):
    from asr_study_amd import ops
    lab, lab_len = O.packed(case)
    path, score = ops.ctc_align(to_dev(case['logits']), to_dev(lab), to_dev(lab_len),
                                to_dev(case['seq_len']), case['N'])
    torch.cuda.synchronize()
    return path, score


@pytest.fixture(scope='module')
def device_results():
    return [tuple(t.cpu().numpy() for t in _run(case)) for case in O.fixtures()]


def test_kernel_against_the_oracle_on_F(device_results):
    worst = [0.0, 0.0]
    exact = 0
    report = []
    for case, rows, (path, score) in zip(O.fixtures(), O.reference(), device_results):
        assert path.shape == (case['N'], case['T']) and path.dtype == np.int32
        w1, w2, ex = O.compare(case, rows, path, score, report)
        worst = [max(worst[0], w1), max(worst[1], w2)]
        exact += ex
    rel = max(d2 / max(1.0, abs(best)) for _, _, best, _, _, d2, _ in report)
    print('kernel: E32 = %.3e; worst path-score deviation %.3g tol, worst score deviation '
          '%.3g tol (%.3e relative); %d paths compared exactly'
          % (O.e32(), worst[0], worst[1], rel, exact))
    assert exact >= 25


def test_kernel_paths_equal_the_host_form(device_results):
    from asr_study_amd import ops
    for case, rows, (path, score) in zip(O.fixtures(), O.reference(), device_results):
        lab, lab_len = O.packed(case)
        hpath, hscore = ops.ctc_align_host(case['logits'], lab, lab_len, case['seq_len'],
                                           case['N'])
        for n, (best, want, gap) in enumerate(rows):
            if want is None:
                assert np.all(path[n] == -1) and np.all(hpath[n] == -1)
            elif gap >= O.GAP_MIN:
                assert np.array_equal(path[n], hpath[n]), (case['name'], n)


def test_l_max_512_is_an_argument_error():
    from asr_study_amd import _lib, ops
    logits = torch.zeros((4, 16, 5), device=dev())
    lab = torch.zeros((1, 512), dtype=torch.int32, device=dev())
    with pytest.raises(_lib.AsrHipError, match='l_max=512'):
        ops.ctc_align(logits, lab, to_dev(np.array([1], np.int32)),
                      to_dev(np.array([4], np.int32)), 1)
    with pytest.raises(ValueError, match='outside'):
        ops.ctc_align(logits, to_dev(np.array([[0, 4]], np.int32)),
                      to_dev(np.array([2], np.int32)), to_dev(np.array([4], np.int32)), 1)


def test_exact_ties_follow_the_tie_rule():
    T, N, C = 9, 3, 4
    labels = [[1, 1, 2], [], [0]]
    case = O._case('ties', np.zeros((T, 16, C), np.float32), labels, [T] * N, 16)
    path, score = [t.cpu().numpy() for t in _run(case)]
    lp = O.log_softmax(case['logits'][:, 0])
    for n in range(N):
        best, want, _ = O.viterbi(lp, labels[n], C - 1)
        assert np.array_equal(path[n], want), (n, path[n], want)
        assert abs(score[n] - best) < 1e-5
    assert path[0].tolist() == [1, 2, 3, 5, 6, 6, 6, 6, 6]


def test_infeasible_utterance_leaves_the_others_alone():
    rs = np.random.RandomState(3)
    T, C = 6, 5
    labels = [[0, 1, 2], [1, 1, 1, 1], [2, 3], [0, 1, 2, 3]]
    seq = [6, 6, 5, 3]                             # row 1 needs 7 frames, row 3 needs 4
    case = O._case('infeasible', (3.0 * rs.randn(T, 16, C)).astype(np.float32), labels, seq, 16)
    path, score = [t.cpu().numpy() for t in _run(case)]
    for n in (1, 3):
        assert np.all(path[n] == -1) and score[n] == -np.inf
    for n in (0, 2):
        best, want, _ = O.viterbi(O.log_softmax(case['logits'][:seq[n], n]), labels[n], C - 1)
        assert np.array_equal(path[n, :seq[n]], want) and np.all(path[n, seq[n]:] == -1)
        assert abs(score[n] - best) < 1e-5


def test_same_call_twice_and_a_dirty_workspace(device_results):
    """Bit-identical results across calls, and with the workspace filled with 0xFF bytes before
    the call: every byte that is read has been written by the call itself."""
    from asr_study_amd import ops
    for k in (2, 7, 9):                            # PPL 1 ragged, PPL 4, PPL 8
        case = O.fixtures()[k]
        path, score = device_results[k]
        ops.WS.bufs[('ctc_align', str(dev()))].fill_(255)
        p2, s2 = [t.cpu().numpy() for t in _run(case)]
        assert np.array_equal(p2, path) and np.array_equal(s2.view(np.int32), score.view(np.int32))
        p3, s3 = [t.cpu().numpy() for t in _run(case)]
        assert np.array_equal(p3, path) and np.array_equal(s3.view(np.int32), score.view(np.int32))


def test_loss_kernels_are_unchanged_by_an_align_call():
    from asr_study_amd import ops
    case = O.fixtures()[2]
    lab, lab_len = O.packed(case)
    args = (to_dev(case['logits']), to_dev(lab), to_dev(lab_len), to_dev(case['seq_len']), case['N'])
    g1 = torch.empty_like(args[0])
    l1 = ops.ctc_loss_grad(*args, grad=g1).clone()
    ops.ctc_align(*args)
    g2 = torch.empty_like(args[0])
    l2 = ops.ctc_loss_grad(*args, grad=g2).clone()
    torch.cuda.synchronize()
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    assert np.isinf(l1.cpu().numpy()[2]) and np.isfinite(l1.cpu().numpy()[:2]).all()


def _check_model_alignment(model, x, labels, lens):
    out = model.align(x, labels, lens)
    slab = model.to_slab(x)
    logits = model.forward(slab, training=False, need_grad=False, n_valid=len(labels))
    logits = logits.cpu().numpy()
    sl = np.asarray(model.out_lengths(np.asarray(lens)))
    worst = 0.0
    for n, a in enumerate(out['alignments']):
        Tn = int(sl[n])
        lp = O.log_softmax(logits[:Tn, n])
        best, want, gap = O.viterbi(lp, labels[n], logits.shape[2] - 1)
        tol = O.tolerance(best)
        assert len(a['path']) == Tn
        got = O.path_score(lp, labels[n], a['path'])
        worst = max(worst, abs(got - best) / tol, abs(a['score'] - best) / tol)
        assert abs(got - best) <= tol and abs(a['score'] - best) <= tol, (n, got, a['score'], best)
        if gap >= O.GAP_MIN:
            assert np.array_equal(a['path'], want), n
        assert [s[1] for s in a['segments']] == list(labels[n])
        bounds = [(lo, hi) for _, _, lo, hi in a['segments']]
        for i, (lo, hi) in enumerate(bounds):
            assert 0 <= lo < hi <= Tn and (i + 1 == len(bounds) or hi <= bounds[i + 1][0])
    print('Model.align: worst deviation %.3g tol' % worst)
    return out


def test_model_align_against_the_oracle_on_its_own_logits():
    from asr_study_amd.core import models
    model = models.brsmv1(num_features=12, num_classes=28, num_hiddens=16, num_layers=1,
                          dropout=0.0, seed=3)
    rs = np.random.RandomState(4)
    x = rs.randn(4, 40, 12).astype(np.float32)
    labels = [[1, 2, 3, 3, 9], [], [7], [4, 4, 4, 20, 0, 26]]
    lens = [40, 25, 3, 31]
    out = _check_model_alignment(model, x, labels, lens)
    assert out['time_stride'] == 1
    with pytest.raises(ValueError, match='Not enough time for target transition sequence'):
        model.align(x, [[1, 1, 1], [2], [3], [4]], [4, 25, 3, 31])


def test_model_with_a_time_stride_aligns_on_the_strided_axis():
    from asr_study_amd.core import models
    model = models.deep_speech2(num_features=16, num_classes=28, num_hiddens=16, num_layers=1,
                                conv_filters=4, conv_kernels=((5, 7), (3, 5)), dropout=0.0,
                                weight_decay=0.0, seed=2)
    rs = np.random.RandomState(6)
    x = rs.randn(3, 41, 16).astype(np.float32)
    labels = [[1, 2, 2], [5], [3, 4, 5, 6, 7, 8]]
    lens = [41, 13, 30]
    out = _check_model_alignment(model, x, labels, lens)
    assert out['time_stride'] == 2 == int(np.prod(model.time_strides))
    assert [len(a['path']) for a in out['alignments']] == [21, 7, 15]


def test_full_size_call():
    """T = 999, N = 64, C = 29, 100 .. 150 labels: every score finite and every path valid
    (vectorised check); the oracle runs on 4 utterances."""
    rs = np.random.RandomState(8)
    T, N, C = 999, 64, 29
    labels = [O.random_label(rs, int(rs.randint(100, 151)), C, int(rs.randint(0, 5)))
              for _ in range(N)]
    seq = rs.randint(700, T + 1, size=N)
    seq[0] = T
    case = O._case('full', (3.0 * rs.randn(T, 64, C)).astype(np.float32), labels, seq, 64)
    lab, lab_len = O.packed(case)
    path, score = [t.cpu().numpy() for t in _run(case)]
    assert np.isfinite(score).all() and (score < 0).all()
    assert O.paths_valid(path, lab, lab_len, case['seq_len']).all()
    worst = 0.0
    for n in (0, 1, 31, 63):
        Tn = int(seq[n])
        lp = O.log_softmax(case['logits'][:Tn, n])
        best, want, gap = O.viterbi(lp, labels[n], C - 1)
        tol = O.tolerance(best)
        got = O.path_score(lp, labels[n], path[n, :Tn])
        worst = max(worst, abs(got - best) / tol, abs(score[n] - best) / tol)
        assert abs(got - best) <= tol and abs(score[n] - best) <= tol, (n, got, score[n], best)
        if gap >= O.GAP_MIN:
            assert np.array_equal(path[n, :Tn], want), n
    print('full size: worst deviation %.3g tol' % worst)


def test_align_command_line_in_a_child_process(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'align_cli_worker.py'),
                          str(tmp_path), 'gpu'], cwd=ROOT, env=dict(os.environ),
                         stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=280)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    line = [ln for ln in out.stdout.decode().splitlines() if ln.startswith('RESULT ')][0]
    res = json.loads(line[7:])
    assert res['refused'] and res['returned'] == len(res['lines']) > 0
    for row, text in zip(res['lines'], res['sanitised']):
        assert ''.join(c['char'] for c in row['chars']) == text
        assert np.isfinite(row['score']) and row['score'] < 0
        last_frame = 0
        for c in row['chars']:
            assert last_frame <= c['start_frame'] < c['end_frame']
            last_frame = c['end_frame']
            assert c['start'] is None and c['end'] is None     # stored features: no win_step
    # --file --text with the feature extractor named: times in seconds, increasing
    assert len(res['file_lines']) == 1
    row = res['file_lines'][0]
    assert ''.join(c['char'] for c in row['chars']) == 'hello world'
    last_time = 0.0
    for c in row['chars']:
        assert last_time <= c['start'] < c['end']
        assert abs(c['start'] - 0.01 * c['start_frame']) < 1e-9           # mfcc: win_step 0.01
        assert abs(c['end'] - 0.01 * c['end_frame']) < 1e-9
        last_time = c['end']
