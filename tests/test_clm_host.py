"""Character language model (asr_study_amd/lm.py) and the host prefix beam decoder with it
(asr_ctc_beam_lm_host, csrc/decode_host.cpp), without a GPU: the Witten-Bell estimator against a
hand-computed table and a second implementation, the file format, the decoder against the
float64 oracle with the two scorer hooks (tests/clm_oracle.py) and against brute force, the toy
task on which the model must lower the label error rate, and the make_lm command line."""
import os

import numpy as np
import pytest

from asr_study_amd import _lib as L
from asr_study_amd.lm import CharLM
from oracle import decode as OD
from tests import clm_oracle as CO

PAIRS = [(0.8, 0.0), (1.5, 0.7), (0.5, -0.5)]           # (alpha, beta)


@pytest.fixture(scope='module')
def ops():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L.load()
    from asr_study_amd import ops
    return ops


def _random_corpus(K, seed, n=60, max_len=14):
    rs = np.random.RandomState(seed)
    # a skewed alphabet, so that some histories are never seen and backoff is exercised
    p = rs.dirichlet(np.full(K, 0.3))
    return [rs.choice(K, size=rs.randint(0, max_len), p=p).tolist() for _ in range(n)]


# ------------------------------------------------------------------ estimator
def test_witten_bell_known_answer():
    m = CharLM.estimate([[0, 1], [0, 0]], num_labels=2, order=2)
    assert m.n_ctx == 3 and m.root == 2 and m.logp.dtype == np.float32
    want = np.array([[7 / 12., 5 / 12.], [2 / 3., 1 / 3.], [8 / 9., 1 / 9.]])
    assert np.abs(np.exp(m.logp.astype(np.float64)) - want).max() < 1e-7


@pytest.mark.parametrize('order', [1, 2, 3, 4])
def test_rows_are_distributions(order):
    m = CharLM.estimate(_random_corpus(5, order), 5, order)
    p = np.exp(m.logp.astype(np.float64))
    assert m.logp.shape == (6 ** (order - 1), 5)
    assert np.abs(p.sum(axis=1) - 1.0).max() < 1e-6 and (p > 0).all()


@pytest.mark.parametrize('K,order', [(4, 1), (4, 2), (4, 3), (3, 4), (2, 5), (27, 2)])
def test_estimator_equals_the_oracles(K, order):
    corpus = _random_corpus(K, 10 * K + order)
    got = CharLM.estimate(corpus, K, order).logp
    want = np.log(CO.estimate(corpus, K, order)).astype(np.float32)
    assert np.abs(got.astype(np.float64) - want).max() < 1e-6


def test_context_walk():
    """K = 3, order 3: contexts are two base-4 digits, oldest first, 3 = before the sentence."""
    m = CharLM(np.zeros((16, 3), np.float32), 3, 3)
    assert (m.n_ctx, m.root) == (16, 15)                 # (3, 3)
    c = m.root
    walk = []
    for label in [2, 0, 0, 1]:
        c = m.next(c, label)
        walk.append(c)
    assert walk == [3 * 4 + 2, 2 * 4 + 0, 0, 0 * 4 + 1]
    one = CharLM(np.zeros((1, 3), np.float32), 3, 1)
    assert (one.n_ctx, one.root, one.next(0, 2)) == (1, 0, 0)


def test_fused_is_float32_and_cached():
    m = CharLM.estimate(_random_corpus(4, 3), 4, 2)
    w = m.fused(1.5, 0.7)
    assert w.dtype == np.float32 and w is m.fused(1.5, 0.7)
    assert np.array_equal(w, np.float32(1.5) * m.logp + np.float32(0.7))


# ------------------------------------------------------------------ file
def test_file_round_trip_and_refusals(tmp_path):
    from asr_study_amd.preprocessing import text
    from asr_study_amd.lm import parser_vocab
    vocab = parser_vocab(text.simple_char_parser)
    assert len(vocab) == 27 and vocab[:3] == 'abc' and vocab[-1] == ' '
    m = CharLM.estimate(_random_corpus(27, 1), 27, 2, vocab=vocab)
    path = str(tmp_path / 'lm.npz')
    m.save(path)
    assert os.path.exists(path)
    back = CharLM.load(path)
    assert (back.order, back.num_labels, back.vocab) == (2, 27, vocab)
    assert np.array_equal(back.logp.view(np.int32), m.logp.view(np.int32))
    back.check(28, text.simple_char_parser)
    with pytest.raises(ValueError) as e:
        back.check(30)
    assert '27' in str(e.value) and '29' in str(e.value)
    with pytest.raises(ValueError):
        back.check(28, text.complex_char_parser)
    for order in (0, 6):
        with pytest.raises(ValueError):
            CharLM.estimate([[0, 1]], 2, order)
        with pytest.raises(ValueError):
            CharLM(np.zeros((1, 2), np.float32), 2, order)
    with pytest.raises(ValueError):                      # 100^4 contexts x 99 labels: no int32
        CharLM.estimate([[0]], 99, 5)


def test_greedy_decoder_refuses_a_language_model():
    from asr_study_amd.core import ctc_utils
    m = CharLM(np.zeros((1, 3), np.float32), 3, 1)
    with pytest.raises(ValueError):
        ctc_utils.decoder_config(is_greedy=True, lm=m)
    assert ctc_utils.decoder_config(is_greedy=False, lm=m, lm_alpha=0.5)['lm_alpha'] == 0.5
    assert 'lm' not in ctc_utils.decoder_config(is_greedy=False)


# ------------------------------------------------------------------ host decoder
def _first_case(W):
    """tests/test_gpu_beam.py::test_device_beam_equals_host_decoder's logits and lengths."""
    rs = np.random.RandomState(W)
    T, N, C = 60, 9, 28
    x = (rs.randn(T, N, C) * rs.choice([0.05, 1.0, 4.0], size=(1, N, 1))).astype(np.float32)
    x[:, 3:6, C - 1] += 3.0
    return x, np.array([T, 0, 1, 17, T, 33, 2, T, 45], np.int32)


def _slab(x, n_pad=16):
    T, N, C = x.shape
    slab = np.zeros((T, n_pad, C), np.float32)
    slab[:, :N] = x
    return slab


@pytest.fixture(scope='module')
def models27():
    corpus = _random_corpus(27, 99, n=200, max_len=20)
    return {order: CharLM.estimate(corpus, 27, order) for order in (1, 2, 3)}


@pytest.mark.parametrize('W', [1, 3, 100])
def test_zero_table_is_the_plain_decoder_bit_for_bit(ops, W):
    x, lens = _first_case(W)
    slab = _slab(x)
    for merge in (True, False):
        want, wscore = ops.ctc_beam_search_host(slab, lens, 9, W, merge)
        for order in (1, 3):
            z = np.zeros((28 ** (order - 1), 27), np.float32)
            got, score = ops.ctc_beam_search_lm_host(slab, lens, 9, W, merge, z, order)
            assert got == want
            assert np.array_equal(score.view(np.int32), wscore.view(np.int32))


@pytest.mark.parametrize('order', [1, 2, 3])
@pytest.mark.parametrize('W', [1, 3, 100])
def test_host_decoder_equals_oracle(ops, models27, W, order):
    x, lens = _first_case(W)
    slab = _slab(x)
    for alpha, beta in PAIRS:
        w = models27[order].fused(alpha, beta)
        merged, plain, oscore = CO.beam_search_lm_both(x, lens, W, w, order)
        for merge, want in ((True, merged), (False, plain)):
            got, score = ops.ctc_beam_search_lm_host(slab, lens, 9, W, merge, w, order)
            assert got == want, (alpha, beta, merge)
            for n in range(9):
                assert abs(score[n] - oscore[n]) <= 1e-5 * max(1.0, abs(oscore[n]))
    assert any(len(s) for s in merged)


@pytest.mark.parametrize('seed', range(6))
def test_full_width_is_the_exact_argmax(ops, seed):
    """T = 5, C = 4: at most 364 prefixes, so width 1024 never evicts and the decode is the
    labelling with the largest CTC score + sum of w."""
    rs = np.random.RandomState(seed)
    T, C, order = 5, 4, 3
    x = (rs.randn(T, 1, C) * 2).astype(np.float32)
    lm = CharLM.estimate(_random_corpus(3, seed, n=30, max_len=6), 3, order)
    w = lm.fused(1.5, 0.7)
    scores = CO.bruteforce(x[:, 0], w, order)
    best = max(scores, key=scores.get)
    got, score = ops.ctc_beam_search_lm_host(_slab(x), [T], 1, 1024, False, w, order)
    assert tuple(got[0]) == best
    assert abs(score[0] - scores[best]) <= 1e-5 * max(1.0, abs(scores[best]))
    o, osc = CO.beam_search_lm_one(x[:, 0], 1024, w, order, merge_repeated=False)
    assert tuple(o) == best and abs(osc - scores[best]) < 1e-9


# ------------------------------------------------------------------ it helps
def test_language_model_lowers_the_label_error_rate(ops):
    """Five words over 4 letters + space, 300 training sentences, 64 noisy utterances, order 3,
    alpha 1, beta 0, width 16: the oracle's LER with the model is at most 0.6 x its LER without
    (this corpus: 0.126 against 0.469), and the implementation returns the oracle's strings."""
    train, truths, x, lens = CO.lexicon_corpus()
    lm = CharLM.estimate(train, CO.TOY_K, 3)
    w = lm.fused(1.0, 0.0)
    plain, _ = CO.beam_search_lm(x, lens, 16)
    with_lm, _ = CO.beam_search_lm(x, lens, 16, w, 3)
    ler0, ler1 = OD.ler(plain, truths), OD.ler(with_lm, truths)
    print('LER without / with the LM: %.3f / %.3f' % (ler0, ler1))
    assert ler1 <= 0.6 * ler0
    got0, _ = ops.ctc_beam_search_host(x, lens, 64, 16, True)
    got1, _ = ops.ctc_beam_search_lm_host(x, lens, 64, 16, True, w, 3)
    assert got0 == plain and got1 == with_lm


# ------------------------------------------------------------------ command line
def test_make_lm_command_line(tmp_path):
    from asr_study_amd import cli
    from asr_study_amd.datasets.dummy import Dummy
    from asr_study_amd.preprocessing import text
    ds = Dummy(num_speakers=3, num_utterances_per_speaker=4, max_duration=0.05,
               min_duration=0.02, split=[0.5, 0.25], seed=1, fs=16e3)
    data = str(tmp_path / 'd.npz')
    ds.to_h5(data, input_parser=None, label_parser=text.simple_char_parser, fmt='npz')
    extra = tmp_path / 'more.txt'
    extra.write_text(u'the cat sat\non the mat\n')
    out = [str(tmp_path / name) for name in ('a.npz', 'b.npz', 'c.npz')]
    for path in out[:2]:
        assert cli.make_lm_main(['--dataset', data, '--subset', 'train', '--order', '3',
                                 '--output_file', path]) == path
    a, b = CharLM.load(out[0]), CharLM.load(out[1])
    assert (a.order, a.num_labels, a.logp.shape) == (3, 27, (28 * 28, 27))
    assert a.logp.tobytes() == b.logp.tobytes()
    a.check(28, text.simple_char_parser)
    p = np.exp(a.logp.astype(np.float64))
    assert np.abs(p.sum(axis=1) - 1).max() < 1e-6
    cli.make_lm_main(['--text', str(extra), '--order', '2', '--output_file', out[2]])
    c = CharLM.load(out[2])
    t, h = text.simple_char_parser('t')[0], text.simple_char_parser('h')[0]
    assert c.order == 2 and c.logp[t, h] == c.logp[t].max()      # 'h' follows 't' most often
    with pytest.raises(ValueError):
        cli.make_lm_main(['--output_file', out[2]])


# ------------------------------------------------------------------ the device kernel's loop
@pytest.mark.parametrize('C,W', [(3, 2), (4, 5), (6, 8), (6, 40)])
def test_device_loop_model_with_the_hooks_equals_oracle(C, W):
    """tests/beam_device_lm_model.py (the kernel's phases with block_ctx / b_ctx and the two
    hooks) against the oracle: positive and negative w, and scores rounded to halves so that
    ties and the early exit of the turn loop are exercised."""
    from tests.beam_device_lm_model import beam_device_lm_model
    rs = np.random.RandomState(C * 10 + W)
    K, order, T = C - 1, 3, 18
    lm = CharLM.estimate(_random_corpus(K, C, n=40, max_len=10), K, order)
    for case, (alpha, beta) in enumerate(PAIRS + [(1.0, 2.0)]):
        x = (rs.randn(T, C) * 2).astype(np.float32)
        w = lm.fused(alpha, beta)
        if case % 2:
            x, w = np.round(x * 2) / 2, (np.round(w * 2) / 2).astype(np.float32)
        for merge in (True, False):
            got, score = beam_device_lm_model(x, W, w, order, merge)
            want, wscore = CO.beam_search_lm_one(x, W, w, order, merge)
            assert got == want and abs(score - wscore) <= 1e-9 * max(1.0, abs(wscore))
