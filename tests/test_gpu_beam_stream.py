"""-m gpu: the streaming beam decoder (K27).  The resumable kernel (asr_ctc_beam_stream,
asr_ctc_beam_lm_stream) fed in chunks against the whole-utterance kernels it restates
(ops.ctc_beam_search, ops.ctc_beam_search_lm): the same strings and the same score bits for every
split; the state record and the tree; stable_len against tests/beam_stream_model.py; the sessions
of Model.stream(beam=...) and predict.py --stream_beam against the whole-utterance decode of the
streamed logits."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.beam_stream_model import beam_stream_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _i32(a):
    return torch.tensor(np.asarray(a, np.int32), device='cuda:0')


def _slab(x):
    from asr_study_amd import ops
    T, N, C = x.shape
    slab = np.zeros((T, ops.pad16(N), C), np.float32)
    slab[:, :N] = x
    return torch.from_numpy(slab).cuda()


def _whole(slab, lens, N, W, merge, lm=None):
    from asr_study_amd import ops
    if lm is None:
        dec, dlen, score = ops.ctc_beam_search(slab, _i32(lens), N, W, merge)
    else:
        dec, dlen, score = ops.ctc_beam_search_lm(slab, _i32(lens), N, W, merge, lm[0], lm[1])
    torch.cuda.synchronize()
    dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
    return [dec[n, :dlen[n]].tolist() for n in range(N)], score.cpu().numpy()


def _tree(state, n):
    """The used part of stream n's tree: (rec rows as int32 pairs, block_parent)."""
    h = state.header()
    nblocks, K = int(h['nblocks'][n]), state.C - 1
    per = state.ws_bytes // state.N
    max_blocks = state.max_frames * state.width
    ws = state.ws[n * per:(n + 1) * per].cpu().numpy()
    rec = ws[64:64 + (1 + nblocks * K) * 8].view(np.int32).reshape(-1, 2)
    off = 64 + (1 + max_blocks * K) * 8
    return rec.copy(), ws[off:off + nblocks * 4].view(np.int32).copy()


def _streamed(slab, lens, N, W, merge, chunk, lm=None, max_frames=None, fill=None):
    """The slab in chunks of `chunk` frames -> ([(strings, scores, stable_len) per chunk], state).
    Checks on the way: the padding of decoded, and that what was committed (the stable prefix)
    is never retracted; 'joined' (committed labels + the rest at the end) is the last string."""
    from asr_study_amd import ops
    T, _, C = slab.shape
    lens = np.asarray(lens)
    max_frames = T if max_frames is None else max_frames
    state = ops.BeamStreamState(N, C, W, max_frames, lm, 'cuda:0')
    if fill is not None:
        state.ws = torch.full((state.ws_bytes,), fill, dtype=torch.uint8, device='cuda:0')
    outs, committed = [], [[] for _ in range(N)]
    for t0 in range(0, T, chunk):
        part = slab[t0:t0 + chunk].contiguous()
        cl = np.clip(lens - t0, 0, part.shape[0])
        dec, dlen, stable, score = ops.ctc_beam_stream(part, _i32(cl), state, N, W, merge,
                                                       max_frames)
        torch.cuda.synchronize()
        dec, dlen, stable = dec.cpu().numpy(), dlen.cpu().numpy(), stable.cpu().numpy()
        strings = [dec[n, :dlen[n]].tolist() for n in range(N)]
        for n in range(N):
            assert (dec[n, dlen[n]:] == -1).all() and dec.shape[1] == max_frames
            assert len(committed[n]) <= stable[n] <= dlen[n], (t0, n)
            assert strings[n][:len(committed[n])] == committed[n], (t0, n)     # never retracted
            committed[n] = strings[n][:stable[n]]
        outs.append((strings, score.cpu().numpy(), stable.tolist()))
    return outs, state


_MODEL = {}


def _model_stable(x, n, Tn, W, merge):
    """stable_len of stream n after every frame (the stable node does not depend on the split)."""
    key = (x.shape, float(x.sum()), n, Tn, W, merge)
    if key not in _MODEL:
        _, outs = beam_stream_model(x[:Tn, n], W, [1] * Tn, merge)
        _MODEL[key] = [0] + [o[2] for o in outs]
    return _MODEL[key]


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('merge', [True, False])
@pytest.mark.parametrize('W', [1, 3, 64, 129, 449])
def test_every_split_gives_the_whole_utterance_decode(W, merge):
    """Strings equal, score bit-equal, the same record and tree for every split; stable_len is
    the model's after every chunk.  129 and 449 take the E = 7 and E = 16 instantiations."""
    rs = np.random.RandomState(W)
    T, C = (24, 28) if W == 449 else (40, 6)
    N = 3
    lens = [T, 17, 1]
    x = (rs.randn(T, N, C) * 1.5).astype(np.float32)
    # stream 0 peaked, its first half sharply: an early error costs more than W later ones, so the
    # whole beam comes to agree on the early labels and the stable prefix grows at every width
    x[np.arange(T), 0, rs.randint(0, C, size=T)] += np.where(np.arange(T) < T // 2, 40.0, 6.0)
    slab = _slab(x)
    want, wscore = _whole(slab, lens, N, W, merge)
    assert any(len(s) for s in want)
    assert _model_stable(x, 0, T, W, merge)[-1] > 0
    ref = None
    for chunk in (1, 7, T):
        outs, state = _streamed(slab, lens, N, W, merge, chunk)
        strings, score, _ = outs[-1]
        assert strings == want, chunk
        assert np.array_equal(score.view(np.int32), wscore.view(np.int32)), chunk
        h = state.header()
        assert h['frames_done'].tolist() == lens and not h['overflow'].any()
        got = (state.rec.cpu().numpy(), [_tree(state, n) for n in range(N)])
        if ref is None:
            ref = got
        else:
            assert np.array_equal(got[0], ref[0]), chunk
            for n in range(N):
                assert np.array_equal(got[1][n][0], ref[1][n][0]), (chunk, n)
                assert np.array_equal(got[1][n][1], ref[1][n][1]), (chunk, n)
        # W = 449 is the one width with more entries than threads: the walk's second pass
        for n in range(N):
            model = _model_stable(x, n, lens[n], W, merge)
            for i, (_, _, stable) in enumerate(outs):
                frames = min(lens[n], min(T, (i + 1) * chunk))
                assert stable[n] == model[frames], (chunk, n, i)


@pytest.mark.parametrize('C,W', [(2, 4), (3, 5), (5, 7), (6, 40)])
def test_stream_on_tied_logits_equals_oracle(C, W):
    """The logits of test_device_beam_on_tied_logits_equals_oracle, in chunks of 5."""
    from oracle import decode as OD
    rs = np.random.RandomState(C * 100 + W)
    T, N = 22, 16
    x = np.round(rs.randn(T, N, C) * 2).astype(np.float32) / 2
    x[:, :4] = 0.0
    slab = _slab(x)
    for merge in (True, False):
        want, wscore = _whole(slab, [T] * N, N, W, merge)
        outs, _ = _streamed(slab, [T] * N, N, W, merge, 5)
        got, score, _ = outs[-1]
        assert got == want and np.array_equal(score.view(np.int32), wscore.view(np.int32))
        for n in range(0, N, 3):
            o, osc = OD.beam_search_decode_one(x[:, n], W, merge_repeated=merge, dtype=np.float64)
            assert got[n] == o[0]
            assert abs(score[n] - osc[0]) <= 1e-5 * max(1.0, abs(osc[0]))
            model = _model_stable(x, n, T, W, merge)
            for i, (_, _, stable) in enumerate(outs):
                assert stable[n] == model[min(T, 5 * (i + 1))], (n, i)


def _lm(K, order=3, alpha=0.8, beta=0.3):
    from asr_study_amd.lm import CharLM
    rs = np.random.RandomState(K)
    p = rs.dirichlet(np.full(K, 0.3))
    corpus = [rs.choice(K, size=rs.randint(0, 12), p=p).tolist() for _ in range(80)]
    return CharLM.estimate(corpus, K, order), alpha, beta


@pytest.mark.parametrize('merge', [True, False])
def test_lm_stream_equals_the_lm_decoder(merge):
    rs = np.random.RandomState(8)
    T, N, C, W = 40, 3, 6, 8
    lens = [T, 17, 1]
    table, alpha, beta = _lm(C - 1)
    lm = (torch.from_numpy(np.array(table.fused(alpha, beta))).cuda(), table.order)
    slab = _slab((rs.randn(T, N, C) * 1.5).astype(np.float32))
    want, wscore = _whole(slab, lens, N, W, merge, lm)
    plain, _ = _whole(slab, lens, N, W, merge)
    assert want != plain                                    # the table decides something
    for chunk in (5, T):
        outs, state = _streamed(slab, lens, N, W, merge, chunk, lm)
        assert outs[-1][0] == want
        assert np.array_equal(outs[-1][1].view(np.int32), wscore.view(np.int32))
        assert state.header()['frames_done'].tolist() == lens


def test_state_record_rules():
    from asr_study_amd import ops
    rs = np.random.RandomState(4)
    T, N, C, W = 16, 3, 6, 5
    x = (rs.randn(T, N, C) * 1.5).astype(np.float32)
    slab = _slab(x)
    lens = [T, 9, 16]
    # a workspace pre-filled with 0x7f bytes gives the results of a zeroed one
    a, sa = _streamed(slab, lens, N, W, True, 7, fill=0)
    b, sb = _streamed(slab, lens, N, W, True, 7, fill=0x7f)
    for (s1, sc1, st1), (s2, sc2, st2) in zip(a, b):
        assert s1 == s2 and st1 == st2 and np.array_equal(sc1.view(np.int32), sc2.view(np.int32))
    assert torch.equal(sa.rec, sb.rec)
    # chunk_len = 0 leaves the record byte-identical: a live one and a fresh one
    before = sa.rec.clone()
    out0 = ops.ctc_beam_stream(slab[:4].contiguous(), _i32([0, 0, 0]), sa, N, W, True, T)
    assert torch.equal(sa.rec, before)
    dec, dlen = out0[0].cpu().numpy(), out0[1].cpu().numpy()
    assert [dec[n, :dlen[n]].tolist() for n in range(N)] == a[-1][0]
    assert out0[2].cpu().tolist() == a[-1][2]
    fresh = ops.BeamStreamState(N, C, W, T, None, 'cuda:0')
    dec, dlen, stable, score = ops.ctc_beam_stream(slab[:4].contiguous(), _i32([0, 0, 0]), fresh,
                                                   N, W, True, T)
    assert not fresh.rec.any() and not dlen.any() and not stable.any() and not score.any()
    assert (dec == -1).all()
    # zero-filling the records alone starts the streams again, on the used tree
    sa.zero_()
    again = ops.ctc_beam_stream(slab, _i32(lens), sa, N, W, True, T)
    assert torch.equal(sa.rec, before) and torch.equal(again[3].cpu(), torch.from_numpy(a[-1][1]))
    # a stream takes max_frames frames: a call at frames_done = max_frames processes nothing and
    # sets the flag; a chunk that crosses the bound is processed up to it
    want8, wscore8 = _whole(slab[:8].contiguous(), [8, 8, 8], N, W, True)
    st = ops.BeamStreamState(N, C, W, 8, None, 'cuda:0')
    ops.ctc_beam_stream(slab[:5].contiguous(), _i32([5, 5, 5]), st, N, W, True, 8)
    assert not st.header()['overflow'].any()
    dec, dlen, _, score = ops.ctc_beam_stream(slab[5:10].contiguous(), _i32([5, 3, 0]), st, N, W,
                                              True, 8)
    h = st.header()
    assert h['frames_done'].tolist() == [8, 8, 5] and h['overflow'].tolist() == [1, 0, 0]
    dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
    assert [dec[n, :dlen[n]].tolist() for n in range(2)] == want8[:2]
    assert np.array_equal(score.cpu().numpy()[:2].view(np.int32), wscore8[:2].view(np.int32))
    full = st.rec.clone()
    ops.ctc_beam_stream(slab[10:13].contiguous(), _i32([3, 1, 0]), st, N, W, True, 8)
    h = st.header()
    assert h['frames_done'].tolist() == [8, 8, 5] and h['overflow'].tolist() == [1, 1, 0]
    per = st.rec_bytes // N
    keep = torch.ones(st.rec_bytes, dtype=torch.bool)
    keep[per + 16:per + 20] = False                          # stream 1's overflow field
    assert torch.equal(st.rec.cpu()[keep], full.cpu()[keep])
    # a record that cannot be this geometry's (more entries than the width; more blocks than the
    # frames left have room for) is flagged, left as it is and answered with the empty hypothesis
    for field, value in ((0, W + 1), (0, -2), (1, 8 * W)):
        bad = ops.BeamStreamState(N, C, W, 8, None, 'cuda:0')
        ops.ctc_beam_stream(slab[:5].contiguous(), _i32([5, 5, 5]), bad, N, W, True, 8)
        bad.rec.view(torch.int32)[field] = value                # stream 0's nb / nblocks
        kept = bad.rec.clone()
        dec, dlen, stable, _ = ops.ctc_beam_stream(slab[5:8].contiguous(), _i32([3, 3, 3]), bad,
                                                   N, W, True, 8)
        h = bad.header()
        assert h['overflow'].tolist() == [1, 0, 0] and h['frames_done'].tolist() == [5, 8, 8]
        assert dlen.cpu().tolist()[0] == 0 and stable.cpu().tolist()[0] == 0
        assert torch.equal(bad.rec[:16], kept[:16]) and torch.equal(bad.rec[20:per], kept[20:per])
        dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
        assert dec[1, :dlen[1]].tolist() == want8[1]            # the other streams go on
    # the geometry of the call must be the state's
    with pytest.raises(ValueError):
        ops.ctc_beam_stream(slab[:4].contiguous(), _i32([4, 4, 4]), st, N, W + 1, True, 8)


# ----------------------------------------------------------------------------- the session
PIECES = [1, 7, 13, 3, 17]


def _session_case(beam, whole):
    """The small relative conformer of tests/test_gpu_stream.py, N = 2 streams of 41 and 30
    frames: the joined result of the beam session against `whole` over the logits a second,
    decoder-less session returns for the same pieces."""
    from tests import test_gpu_stream as TS
    from tests import test_gpu_window as TW
    rs = np.random.RandomState(31)
    model = TW._conformer()
    TW._randomise(model, rs)
    model.decoder = None
    N, T = 2, sum(PIECES)
    lens = np.array([T, 30])
    x = TW._batch(rs, N, T, 10, lens)
    logits = np.concatenate(TS._feed_all(model.stream(n_streams=N), x, lens, PIECES)[0], 1)
    assert logits.shape[:2] == (N, T)
    want, wscore = whole(_slab(np.ascontiguousarray(logits.transpose(1, 0, 2))), lens.tolist(), N)
    ss = model.stream(n_streams=N, beam=beam)
    outs, emitted = TS._feed_all(ss, x, lens, PIECES)
    assert emitted == [0, 0, 16, 16, 32]
    joined = [sum((o[n] for o in outs), []) for n in range(N)]
    assert joined == want and any(len(w) for w in want)
    hyp = ss.hypothesis()
    assert [h[0] for h in hyp] == want
    assert np.array_equal(np.array([h[1] for h in hyp], np.float32).view(np.int32),
                          wscore.view(np.int32))
    return model, ss, x, lens, want


def test_session_equals_the_beam_decode_of_the_streamed_logits():
    from tests import test_gpu_stream as TS
    model, ss, x, lens, want = _session_case(
        dict(beam_width=8), lambda slab, l, N: _whole(slab, l, N, 8, True))
    # reset(): the records alone; the session then serves the same streams to the same result
    ss.reset()
    assert ss.hypothesis() == [([], 0.0)] * 2 and not ss._beam_state.rec.any()
    outs, _ = TS._feed_all(ss, x, lens, PIECES)
    assert [sum((o[n] for o in outs), []) for n in range(2)] == want
    # a stream longer than max_frames is refused on the host, before the launch
    small = model.stream(n_streams=2, beam=dict(beam_width=8, max_frames=20))
    small.feed(x[:, :16])
    with pytest.raises(ValueError):
        small.feed(x[:, 16:32])
    assert small.frames_out == 16


def test_session_with_a_language_model():
    table, alpha, beta = _lm(7)

    def whole(slab, lens, N):
        return _whole(slab, lens, N, 8, True,
                      (table.fused_device(alpha, beta, slab.device), table.order))
    _session_case(dict(beam_width=8, lm=table, lm_alpha=alpha, lm_beta=beta), whole)


# ----------------------------------------------------------------------------- the command line
def test_cli_predict_stream_beam(tmp_path, capsys):
    """predict.py --stream 80 --stream_beam --beam_width 8 on the tiny trained model of
    tests/test_gpu_stream.py's CLI test: the last printed hypothesis of every utterance is the
    result of a beam session fed the same pieces."""
    sys.path.insert(0, ROOT)
    import train
    import predict as predict_cli
    from asr_study_amd import cli
    from asr_study_amd.datasets import h5lite
    from asr_study_amd.datasets.dataset_generator import DatasetGenerator
    from asr_study_amd.utils import core_utils, generic_utils
    fmt = 'h5' if h5lite.available() else 'npz'
    fname = str(tmp_path / ('dummy.' + fmt))
    cli.make_dataset_main(['--parser', 'dummy', '--parser_params', 'num_speakers', '4',
                           'num_utterances_per_speaker', '6', 'max_duration', '1.2',
                           'min_duration', '0.6', 'max_label_length', '8', 'split',
                           '[0.5, 0.25]', 'seed', '3', '--input_parser', 'logfbank',
                           '--input_parser_params', 'num_filt', '16', '--output_file', fname])
    out = str(tmp_path / 'run')
    train.main(['--dataset', fname, '--model', 'conformer', '--model_params', 'num_features',
                '16', 'd_model', '32', 'num_heads', '2', 'num_layers', '2', 'd_ff', '64',
                'kernel_size', '7', 'num_classes', '28', 'conv_filters', '4', 'conv_kernels',
                '[[5,7],[3,5]]', 'positions', 'relative', 'context', '[4, 8, 0]', 'causal_conv',
                'True', '--num_epochs', '1', '--batch_size', '4', '--save', out, '--seed', '1',
                '--lr', '0.001'])
    best = os.path.join(out, 'best.h5')
    capsys.readouterr()
    results = predict_cli.main(['--model', best, '--dataset', fname, '--stream', '80',
                                '--stream_beam', '--beam_width', '8'])
    printed = capsys.readouterr().out
    shown = [l.split('Predicted: ', 1)[1] for l in printed.splitlines() if 'Predicted: ' in l]
    assert len(results) == len(shown) > 0 and shown == [r['best'] for r in results]
    tails = [l for l in printed.splitlines() if 'frames in: ' in l]
    assert tails and all(l.endswith(']') and '[' in l for l in tails)
    parser = generic_utils.get_from_module('preprocessing.text', 'simple_char_parser', params=[])
    flow = DatasetGenerator(None, parser, batch_size=1, seed=0, mode='predict',
                            shuffle=False).flow_from_fname(fname, datasets='test')
    model = core_utils.load_model(best, mode='predict', decoder=False)
    ss = model.stream(1, beam=dict(beam_width=8))
    for r in results:
        x, lens = flow.next()
        T = int(np.asarray(lens).reshape(-1)[0])
        x = np.asarray(x, np.float32)
        ss.reset()
        ids = []
        for pos in range(0, T, 8):
            end = min(T, pos + 8)
            ids += ss.feed(x[:, pos:end], ended=[T] if end == T else None)[0]
        ids += ss.finish()[0]
        assert ids == ss.hypothesis()[0][0] and r['best'] == parser.imap(ids)
    with pytest.raises(ValueError):
        predict_cli.main(['--model', best, '--dataset', fname, '--stream_beam'])
