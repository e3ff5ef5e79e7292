"""K9 with a character language model on the device (asr_ctc_beam_lm_device, csrc/beam.hip)
against the host decoder with the same fused table (asr_ctc_beam_lm_host, pinned to the float64
oracle by tests/test_clm_host.py) and, on tied scores, against the oracle directly: identical
label sequences, scores to 1e-6, at every instantiation boundary of the kernel, orders 1-4,
positive and negative per-label bonuses, ragged and empty utterances, merge_repeated on and off,
the full 999-frame length; then the model, ctc_utils.decode and the command lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from asr_study_amd.lm import CharLM
from tests import clm_oracle as CO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(0.8, 0.0), (1.5, 0.7), (0.5, -0.5)]           # (alpha, beta)


def _random_corpus(K, seed, n=200, max_len=20):
    rs = np.random.RandomState(seed)
    p = rs.dirichlet(np.full(K, 0.3))
    return [rs.choice(K, size=rs.randint(0, max_len), p=p).tolist() for _ in range(n)]


@pytest.fixture(scope='module')
def models27():
    corpus = _random_corpus(27, 99)
    return {order: CharLM.estimate(corpus, 27, order) for order in (1, 2, 3, 4)}


def _slab(x):
    from asr_study_amd import ops
    T, N, C = x.shape
    slab = np.zeros((T, ops.pad16(N), C), np.float32)
    slab[:, :N] = x
    return slab


def _device(slab, lens, N, W, merge, w, order):
    from asr_study_amd import ops
    T = slab.shape[0]
    dec, dlen, score = ops.ctc_beam_search_lm(
        torch.from_numpy(slab).cuda(), torch.tensor(np.asarray(lens, np.int32)).cuda(), N, W,
        merge, torch.from_numpy(np.array(w)).cuda(), order)
    torch.cuda.synchronize()
    dec, dlen, score = dec.cpu().numpy(), dlen.cpu().numpy(), score.cpu().numpy()
    for n in range(N):
        assert 0 <= dlen[n] <= T and (dec[n, dlen[n]:] == -1).all()
    return [dec[n, :dlen[n]].tolist() for n in range(N)], score, (dec, dlen)


def _both(x, lens, W, merge, w, order):
    """x (T, N, C) -> (device strings, device scores, host strings, host scores)."""
    from asr_study_amd import ops
    slab = _slab(x)
    N = x.shape[1]
    got, score, _ = _device(slab, lens, N, W, merge, w, order)
    want, wscore = ops.ctc_beam_search_lm_host(slab, np.asarray(lens, np.int32), N, W, merge, w,
                                               order)
    return got, score, want, wscore


def _first_case(W):
    """tests/test_gpu_beam.py::test_device_beam_equals_host_decoder's logits and lengths."""
    rs = np.random.RandomState(W)
    T, N, C = 60, 9, 28
    x = (rs.randn(T, N, C) * rs.choice([0.05, 1.0, 4.0], size=(1, N, 1))).astype(np.float32)
    x[:, 3:6, C - 1] += 3.0
    return x, [T, 0, 1, 17, T, 33, 2, T, 45]


@pytest.mark.parametrize('W', [1, 3, 64, 100, 128, 129, 448, 449, 1024])
@pytest.mark.parametrize('merge', [True, False])
def test_device_lm_beam_equals_host_decoder(models27, W, merge):
    x, lens = _first_case(W)
    # orders 1-3 at every instantiation boundary, order 4 at the README's width and the largest
    for order in {100: (4,), 1024: (1, 2, 3, 4)}.get(W, (1, 2, 3)):
        for alpha, beta in PAIRS:
            w = models27[order].fused(alpha, beta)
            got, score, want, wscore = _both(x, lens, W, merge, w, order)
            assert got == want, (order, alpha, beta)
            np.testing.assert_allclose(score, wscore, rtol=1e-6, atol=1e-6)
    assert any(len(s) for s in want)


@pytest.mark.parametrize('C,W', [(2, 4), (3, 5), (5, 7), (6, 40), (64, 100)])
def test_device_lm_beam_on_tied_scores_equals_host_and_oracle(C, W):
    """Logits and the fused table rounded to halves: exact ties between siblings, between a
    candidate and the beam's bottom and between evicted branches."""
    rs = np.random.RandomState(C * 100 + W)
    T, N, K = 22, 16, C - 1
    order = 2 if C == 64 else 3
    x = np.round(rs.randn(T, N, C) * 2).astype(np.float32) / 2
    x[:, :4] = 0.0                                       # all-equal frames
    lm = CharLM.estimate(_random_corpus(K, C, n=40, max_len=10), K, order)
    w = (np.round(lm.fused(1.0, 0.5) * 2) / 2).astype(np.float32)
    assert len(np.unique(w)) > 1 or K == 1
    lens = [T] * N
    for merge in (True, False):
        got, score, want, wscore = _both(x, lens, W, merge, w, order)
        assert got == want
        np.testing.assert_allclose(score, wscore, rtol=1e-6, atol=1e-6)
        for n in range(0, N, 3):
            o, osc = CO.beam_search_lm_one(x[:, n], W, w, order, merge_repeated=merge)
            assert got[n] == o
            assert abs(score[n] - osc) <= 1e-5 * max(1.0, abs(osc))


@pytest.mark.parametrize('W', [3, 100, 449])
def test_zero_table_is_the_plain_device_decoder_bit_for_bit(W):
    from asr_study_amd import ops
    x, lens = _first_case(W)
    slab = _slab(x)
    logits = torch.from_numpy(slab).cuda()
    sl = torch.tensor(np.asarray(lens, np.int32)).cuda()
    for merge in (True, False):
        dec, dlen, score = ops.ctc_beam_search(logits, sl, 9, W, merge)
        torch.cuda.synchronize()
        for order in (1, 3):
            z = np.zeros((28 ** (order - 1), 27), np.float32)
            _, _, (ldec, ldlen) = got = _device(slab, lens, 9, W, merge, z, order)
            assert np.array_equal(ldec, dec.cpu().numpy())
            assert np.array_equal(ldlen, dlen.cpu().numpy())
            assert np.array_equal(got[1].view(np.int32), score.cpu().numpy().view(np.int32))


def test_determinism_and_pad_rows(models27):
    """The same call twice: every output bit-identical; junk in the n_pad - N pad rows of the
    slab changes nothing."""
    W, order = 129, 3
    x, lens = _first_case(W)
    w = models27[order].fused(1.5, 0.7)
    slab = _slab(x)
    a = _device(slab, lens, 9, W, True, w, order)
    b = _device(slab, lens, 9, W, True, w, order)
    junk = slab.copy()
    junk[:, 9:] = np.random.RandomState(0).randn(*junk[:, 9:].shape).astype(np.float32) * 50
    junk[::3, 9:] = np.inf
    c = _device(junk, lens, 9, W, True, w, order)
    for other in (b, c):
        assert np.array_equal(a[2][0], other[2][0]) and np.array_equal(a[2][1], other[2][1])
        assert np.array_equal(a[1].view(np.int32), other[1].view(np.int32))


def test_full_length_width_400(models27):
    """T = 999 (10 s utterances), width 400, 28 classes, order 3: the eval.py configuration."""
    rs = np.random.RandomState(5)
    T, N, C = 999, 4, 28
    x = (rs.randn(T, N, C) * 2).astype(np.float32)
    x[:, :, C - 1] += 2.0
    x[:, 1] *= 0.1
    got, score, want, wscore = _both(x, [T, T, 640, T], 400, True, models27[3].fused(0.8, 0.3), 3)
    assert got == want and all(len(s) for s in got)
    np.testing.assert_allclose(score, wscore, rtol=1e-6, atol=1e-6)


def test_model_and_ctc_utils_decode_with_a_language_model(monkeypatch):
    """engine.Model with lm= in its decoder under ASR_BEAM=device equals the host decoder on the
    same logits and never calls it; core/ctc_utils.decode gives the same lists under host,
    device and auto."""
    from asr_study_amd import ops
    from asr_study_amd.core import ctc_utils, models
    rs = np.random.RandomState(0)
    N, T, F, C = 5, 40, 12, 9
    lm = CharLM.estimate(_random_corpus(C - 1, 3, n=60, max_len=8), C - 1, 3)
    model = models.brsmv1(num_features=F, num_classes=C, num_hiddens=16, num_layers=2,
                          dropout=0.0, seed=1, is_greedy=False, beam_width=100, lm=lm,
                          lm_alpha=0.8, lm_beta=0.3)
    assert model.decoder['lm'] is lm and model.decoder['lm_beta'] == 0.3
    x = rs.randn(N, T, F).astype(np.float32)
    lens = np.array([T, 31, T, 8, 25])
    slab = model.to_slab(x)
    logits_dev = model.forward(slab, training=False, need_grad=False, n_valid=N)
    logits = logits_dev.cpu().numpy()
    w = lm.fused(0.8, 0.3)
    want, _ = ops.ctc_beam_search_lm_host(logits, lens, N, 100, True, w, 3)
    kw = dict(is_greedy=False, beam_width=100, lm=lm, lm_alpha=0.8, lm_beta=0.3)
    monkeypatch.setenv('ASR_BEAM', 'host')
    host = ctc_utils.decode((logits_dev, lens), **kw)
    monkeypatch.delenv('ASR_BEAM')
    auto = ctc_utils.decode((logits_dev, lens), **kw)
    monkeypatch.setenv('ASR_BEAM', 'device')

    def boom(*a, **k):
        raise AssertionError('host decoder called')
    calls = []
    device_lm = ops.ctc_beam_search_lm

    def spy(*a, **k):
        calls.append(a[-1])                              # the order
        return device_lm(*a, **k)
    monkeypatch.setattr(ops, 'ctc_beam_search_lm_host', boom)
    monkeypatch.setattr(ops, 'ctc_beam_search_host', boom)
    monkeypatch.setattr(ops, 'ctc_beam_search', boom)    # (nor the plain device decoder)
    monkeypatch.setattr(ops, 'ctc_beam_search_lm', spy)
    assert model.predict(x, lens) == want
    assert ctc_utils.decode((logits_dev, lens), **kw) == host == auto == want
    assert calls == [3, 3] and any(len(h) for h in want)
    labels = [rs.randint(0, C - 1, size=3).tolist() for _ in range(N)]
    assert np.isfinite(model.test_on_batch([('slab', slab), labels, lens])).all()
    with pytest.raises(ValueError):                      # a model over 27 labels, 9 classes
        ctc_utils.decode((logits_dev, lens), is_greedy=False,
                         lm=CharLM(np.zeros((1, 27), np.float32), 27, 1))
    with pytest.raises(ValueError):
        ctc_utils.decode((logits_dev, lens), is_greedy=True, lm=lm)


def test_command_lines_end_to_end(tmp_path):
    """One child process: extras/make_dataset.py (dummy) -> train.py (one epoch, tiny) ->
    extras/make_lm.py -> eval.py --lm -> predict.py --lm; the LER is finite and the
    transcriptions are those of ctc_utils.decode(..., lm=...) on the same model."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'clm_cli_worker.py'),
                          str(tmp_path)], cwd=ROOT, env=dict(os.environ), stdin=subprocess.DEVNULL,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    line = [ln for ln in out.stdout.decode().splitlines() if ln.startswith('RESULT ')][0]
    res = json.loads(line[7:])
    assert len(res['eval']) == 4 and np.isfinite(res['eval']).all() and res['eval'][3] >= 0
    assert res['lm_order'] == 3 and res['lm_labels'] == 27
    assert len(res['predicted']) > 0 and res['predicted'] == res['direct']
