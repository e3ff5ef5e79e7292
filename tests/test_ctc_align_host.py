"""CTC forced alignment (K19) without a GPU: the float64 oracle against a brute force, the
library's host form (asr_ctc_align_host) against the oracle on the fixture set F, exact ties,
infeasible utterances, argument errors, ops.ctc_segments, Model.align on a device='cpu' model and
the align.py command line.

Pass conditions (tests/ctc_align_oracle.py: compare): every returned path is a valid alignment;
its float64 score and the returned float32 score lie within tol = 4 * E32 * max(1, |best|) of the
oracle's best, E32 being the largest relative deviation of the oracle's own recursion evaluated
in float32 on F (asserted below 2e-6); the path equals the oracle's wherever the oracle's
uniqueness gap is >= 1e-2 nats, which at most 20 % of F may miss."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ctc_align_oracle as O
from asr_study_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def ops():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from asr_study_amd import ops
    return ops


def test_oracle_matches_brute_force():
    """All transcripts of length <= 3 over 3 labels (C = 4, repeats included), T = 1 .. 6."""
    rs = np.random.RandomState(5)
    cases = feasible = 0
    for T in range(1, 7):
        lp = O.log_softmax(3.0 * rs.randn(T, 4))
        for Ln in range(0, 4):
            for label in itertools.product(range(3), repeat=Ln):
                score, path, gap = O.viterbi(lp, label, 3)
                want, wpath = O.brute_force(lp, label, 3)
                cases += 1
                if wpath is None:
                    assert path is None and score == -np.inf
                    assert len(label) + O.repeats(label) > T
                    continue
                feasible += 1
                assert len(label) + O.repeats(label) <= T
                assert abs(score - want) <= 1e-12, (T, label, score, want)
                assert np.array_equal(path, wpath), (T, label)
                assert abs(O.path_score(lp, label, path, 3) - score) <= 1e-12
                assert gap > 0
    assert cases == 6 * 40 and feasible > 100


def test_gap_is_the_distance_to_the_second_best_alignment():
    rs = np.random.RandomState(11)
    lp = O.log_softmax(2.0 * rs.randn(6, 4))
    label = [0, 1, 1]
    score, path, gap = O.viterbi(lp, label, 3)
    cls, skip = O._lattice(label, 3)
    others = []
    for p in itertools.product(range(len(cls)), repeat=6):
        try:
            O.check_path(label, p)
        except AssertionError:
            continue
        if not np.array_equal(p, path):
            others.append(O.path_score(lp, label, p, 3))
    assert abs((score - max(others)) - gap) < 1e-12


def test_path_score_rejects_invalid_paths():
    lp = O.log_softmax(np.zeros((4, 4)))
    O.path_score(lp, [1, 1], [1, 2, 3, 3])
    for bad in ([1, 3, 3, 3],          # skip between equal labels
                [2, 2, 3, 4],          # starts past state 1
                [0, 1, 1, 2],          # ends before 2L - 1
                [1, 0, 3, 4],          # moves back
                [0, 1, 2, 5]):         # a move of 3
        with pytest.raises(AssertionError):
            O.path_score(lp, [1, 1], bad)


def test_fixture_set_has_few_thin_gaps_and_float32_is_good_enough():
    """On the oracle alone, before any implementation is compared."""
    total = thin = 0
    for case, rows in zip(O.fixtures(), O.reference()):
        for best, path, gap in rows:
            total += 1
            thin += path is not None and gap < O.GAP_MIN
    share = thin / float(total)
    e32 = O.e32()
    print('F: %d utterances, %d below the gap of %g nats (%.1f %%); E32 = %.3e'
          % (total, thin, O.GAP_MIN, 100 * share, e32))
    assert total >= 30 and share <= 0.2
    assert 0 < e32 < 2e-6


def test_host_form_against_the_oracle(ops):
    worst = [0.0, 0.0]
    exact = 0
    report = []
    for case, rows in zip(O.fixtures(), O.reference()):
        lab, lab_len = O.packed(case)
        path, score = ops.ctc_align_host(case['logits'], lab, lab_len, case['seq_len'], case['N'])
        assert path.shape == (case['N'], case['T']) and path.dtype == np.int32
        w1, w2, ex = O.compare(case, rows, path, score, report)
        worst = [max(worst[0], w1), max(worst[1], w2)]
        exact += ex
    rel = max(d2 / max(1.0, abs(best)) for _, _, best, _, _, d2, _ in report)
    print('host form: E32 = %.3e; worst path-score deviation %.3g tol, worst score deviation '
          '%.3g tol (%.3e relative); %d paths compared exactly'
          % (O.e32(), worst[0], worst[1], rel, exact))
    assert exact >= 25


def test_l_max_512_is_an_argument_error(ops):
    logits = np.zeros((4, 16, 5), np.float32)
    lab = np.zeros((1, 512), np.int32)
    with pytest.raises(L.AsrHipError, match='l_max=512'):
        ops.ctc_align_host(logits, lab, [1], [4], 1)
    ops.ctc_align_host(logits, lab[:, :511], [1], [4], 1)


def test_exact_ties_follow_the_tie_rule(ops):
    """All-zero logits: every alignment has the same probability; stay before -1 before -2 and
    2 L before 2 L - 1 put the labels in the earliest feasible frames, then blanks."""
    T, N, C = 9, 3, 4
    labels = [[1, 1, 2], [], [0]]
    logits = np.zeros((T, 16, C), np.float32)
    lab = np.zeros((N, 3), np.int32)
    for n, l in enumerate(labels):
        lab[n, :len(l)] = l
    path, score = ops.ctc_align_host(logits, lab, [3, 0, 1], [T] * N, N)
    lp = O.log_softmax(logits[:, 0])
    for n in range(N):
        best, want, _ = O.viterbi(lp, labels[n], C - 1)
        assert np.array_equal(path[n], want), (n, path[n], want)
        assert abs(score[n] - best) < 1e-5
    assert path[0].tolist() == [1, 2, 3, 5, 6, 6, 6, 6, 6]
    assert path[1].tolist() == [0] * 9
    assert path[2].tolist() == [1, 2, 2, 2, 2, 2, 2, 2, 2]


def test_infeasible_utterance_leaves_the_others_alone(ops):
    rs = np.random.RandomState(3)
    T, C = 6, 5
    logits = (3.0 * rs.randn(T, 16, C)).astype(np.float32)
    lab = np.array([[0, 1, 2, 0], [1, 1, 1, 1], [2, 3, 0, 0], [0, 1, 2, 3]], np.int32)
    lab_len = np.array([3, 4, 2, 4], np.int32)
    seq = np.array([6, 6, 5, 3], np.int32)         # row 1 needs 7 frames, row 3 needs 4
    path, score = ops.ctc_align_host(logits, lab, lab_len, seq, 4)
    assert np.all(path[1] == -1) and score[1] == -np.inf
    assert np.all(path[3] == -1) and score[3] == -np.inf
    alone, score_alone = ops.ctc_align_host(logits, lab[[0, 2]][:, :3].copy(),
                                            lab_len[[0, 2]], seq[[0, 2]], 2)
    # (utterance 2 sits in column 1 of that call: compare through the oracle instead)
    for n in (0, 2):
        best, want, _ = O.viterbi(O.log_softmax(logits[:seq[n], n]), lab[n, :lab_len[n]], C - 1)
        assert np.array_equal(path[n, :seq[n]], want) and np.all(path[n, seq[n]:] == -1)
        assert abs(score[n] - best) < 1e-5
    assert np.array_equal(alone[0], path[0]) and score_alone[0] == score[0]


def test_argument_errors(ops):
    logits = np.zeros((4, 16, 5), np.float32)
    lab = np.array([[0, 1]], np.int32)
    for bad in (4, -1, 7):                         # 4 is the blank
        with pytest.raises(ValueError, match='outside'):
            ops.ctc_align_host(logits, np.array([[0, bad]], np.int32), [2], [4], 1)
    ops.ctc_align_host(logits, np.array([[0, 9]], np.int32), [1], [4], 1)   # past label_len
    with pytest.raises(ValueError):
        ops.ctc_align_host(logits, lab, [3], [4], 1)                         # label_len > l_max
    with pytest.raises(ValueError):
        ops.ctc_align_host(logits, lab, [2], [], 1)
    with pytest.raises(ValueError):
        ops.ctc_align_host(logits[0], lab, [2], [4], 1)
    with pytest.raises(L.AsrHipError):
        ops.ctc_align_host(logits, np.zeros((17, 2), np.int32), [2] * 17, [4] * 17, 17)  # N > n_pad
    lib = L.load()
    assert lib.asr_ctc_align_host(None, None, None, None, 4, 1, 16, 5, 2, None, None) != 0
    assert b'null' in lib.asr_last_error()
    assert lib.asr_ctc_align(None, None, None, None, 4, 1, 16, 5, 2, None, None, None, 0,
                             None) != 0
    assert lib.asr_ctc_align_workspace_bytes(4, 1, 16, 5, 512) == 0
    # 64 / 64 / 128 / 256 bytes of back-pointers per frame and utterance
    sizes = [lib.asr_ctc_align_workspace_bytes(1000, 64, 64, 29, l) for l in (63, 127, 255, 511)]
    small = lib.asr_ctc_align_workspace_bytes(1000, 64, 64, 29, 1)
    assert sizes[0] == small and sizes[1] == small
    assert sizes[2] - small == 64 * 1000 * 64 and sizes[3] - small == 3 * 64 * 1000 * 64


def test_segments_round_trip(ops):
    labels = [3, 3, 7]
    path = [0, 1, 1, 2, 3, 5, 5, 6, -1, -1]
    segs = ops.ctc_segments(path, labels)
    assert segs == [(0, 3, 1, 3), (1, 3, 4, 5), (2, 7, 5, 7)]
    back = np.full(len(path), -2)
    for q, lab, lo, hi in segs:
        assert lab == labels[q]
        back[lo:hi] = 2 * q + 1
    assert all(b == p for b, p in zip(back, path) if p >= 0 and p % 2 == 1)
    assert ops.ctc_segments([-1, -1, -1], labels) == []
    assert ops.ctc_segments([0, 0, 0], []) == []
    with pytest.raises(ValueError):
        ops.ctc_segments([0, 1, 2, 2], labels)


def test_ctc_utils_align_takes_the_host_form_for_host_logits(ops):
    import torch
    from asr_study_amd.core import ctc_utils
    case, rows = O.fixtures()[2], O.reference()[2]
    out = ctc_utils.align((torch.from_numpy(case['logits']), case['labels'], case['seq_len']))
    assert len(out) == case['N']
    for n, (segs, score) in enumerate(out):
        best, want, _ = rows[n]
        if want is None:
            assert segs == [] and score == -np.inf
            continue
        assert [s[1] for s in segs] == case['labels'][n]
        assert abs(score - best) <= O.tolerance(best)
        for q, lab, lo, hi in segs:
            assert np.all(want[lo:hi] == 2 * q + 1)


def test_model_align_on_a_cpu_model(ops, monkeypatch):
    """The network has no host form: forward() is replaced by fixed logits; labels, lengths, the
    too-short check and the alignment itself are Model.align's own."""
    import torch
    from asr_study_amd.core import models
    model = models.brsmv1(num_features=8, num_classes=12, num_hiddens=8, num_layers=1,
                          device='cpu')
    rs = np.random.RandomState(2)
    T, N = 30, 3
    logits = torch.from_numpy((3.0 * rs.randn(T, 16, 12)).astype(np.float32))
    monkeypatch.setattr(model, 'forward', lambda slab, **kw: logits)
    x = np.zeros((N, T, 8), np.float32)
    labels = [[1, 2, 2, 3], [], [5, 0, 5, 5, 7, 10]]
    lens = [30, 12, 9]
    with pytest.raises(ValueError, match='Not enough time for target transition sequence'):
        model.align(x, [[1, 1, 1], [2], [3]], [4, 12, 4])
    out = model.align(x, labels, lens)
    assert out['time_stride'] == 1 and len(out['alignments']) == N
    for n, a in enumerate(out['alignments']):
        assert [s[1] for s in a['segments']] == labels[n]
        assert [s[0] for s in a['segments']] == list(range(len(labels[n])))
        bounds = [(lo, hi) for _, _, lo, hi in a['segments']]
        for i, (lo, hi) in enumerate(bounds):
            assert 0 <= lo < hi <= lens[n]
            assert i + 1 == len(bounds) or hi <= bounds[i + 1][0]
        assert len(a['path']) == lens[n]
        best, want, gap = O.viterbi(O.log_softmax(logits[:lens[n], n].numpy()), labels[n], 11)
        assert abs(a['score'] - best) <= O.tolerance(best)
        assert abs(O.path_score(O.log_softmax(logits[:lens[n], n].numpy()), labels[n],
                                a['path']) - best) <= O.tolerance(best)


def test_align_command_line_in_a_child_process(ops, tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'align_cli_worker.py'),
                          str(tmp_path), 'cpu'], cwd=ROOT, env=dict(os.environ),
                         stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    line = [ln for ln in out.stdout.decode().splitlines() if ln.startswith('RESULT ')][0]
    res = json.loads(line[7:])
    assert res['refused'] and res['returned'] == len(res['lines']) > 0
    for row, text in zip(res['lines'], res['sanitised']):
        assert ''.join(c['char'] for c in row['chars']) == text
        assert np.isfinite(row['score']) and row['score'] < 0 and row['time_stride'] == 1
        last = 0
        for c in row['chars']:
            assert last <= c['start_frame'] < c['end_frame']
            last = c['end_frame']
            assert c['start'] is None and c['end'] is None     # raw audio: no win_step


def test_kernel_logic_as_a_sequential_model():
    """csrc/ctc.hip's Viterbi and backtrace kernels restated lane by lane in NumPy
    (tests/ctc_align_kernel_model.py: pair geometry, wave shift, 4-bit back-pointer fields in a
    dirty workspace, re-centring, staged backtrace) under the same pass conditions on F, and on
    the all-zero tie case."""
    from tests import ctc_align_kernel_model as KM
    worst = [0.0, 0.0]
    exact = 0
    for case, rows in zip(O.fixtures(), O.reference()):
        lab, lab_len = O.packed(case)
        path, score = KM.align(case['logits'], lab, lab_len, case['seq_len'], case['N'])
        w1, w2, ex = O.compare(case, rows, path, score)
        worst = [max(worst[0], w1), max(worst[1], w2)]
        exact += ex
    print('kernel model: worst path-score deviation %.3g tol, worst score deviation %.3g tol; '
          '%d paths compared exactly' % (worst[0], worst[1], exact))
    assert exact >= 25
    labels = [[1, 1, 2], [], [0]]
    lab = np.array([[1, 1, 2], [0, 0, 0], [0, 0, 0]], np.int32)
    path, _ = KM.align(np.zeros((9, 16, 4), np.float32), lab, [3, 0, 1], [9, 9, 9], 3)
    for n in range(3):
        _, want, _ = O.viterbi(O.log_softmax(np.zeros((9, 4))), labels[n], 3)
        assert np.array_equal(path[n], want)
