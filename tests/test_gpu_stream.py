"""-m gpu: cached chunk-by-chunk inference (K26).  The streaming kernels against the whole-utterance
kernels they restate, bit for bit (csrc/attention.hip, rel_attention.hip, dwconv.hip, ctc.hip) and
against the float64 oracle (kernel bound 1e-5, as tests/test_gpu_window.py); the sessions of
Model.stream against the float64 oracle of the whole utterance (model bound 1e-4, as there) and
against Model.predict."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import stream_oracle as SO
from tests import test_gpu_window as TW
from tests import window_oracle as WO

pytestmark = pytest.mark.gpu

ROOT = TW.ROOT
N_PAD = 16
WINDOWS = [(4, 8, 0), (16, 64, 0), (1, 5, 0), (1, 0, 0), (64, 64, 0), (7, 3, 0)]


def _i32(a):
    return torch.tensor(np.asarray(a, np.int32), device='cuda:0')


# ----------------------------------------------------------------------------- the attention kernels
def _steps(window):
    return [window[0]] + ([4 * window[0]] if 4 * window[0] <= 64 else [])


def _stream_attn(kind, d, N, heads, dh, lens, window, step, fill=0.0):
    """The whole slab d['qkv'] fed `step` frames at a time through ring_put and the streaming
    core; the ring starts filled with `fill`.  -> out (T, n_pad, D + pad columns), ring rows."""
    from asr_study_amd import ops
    T, n_pad, ld = d['qkv'].shape
    D = heads * dh
    R = ops.attn_stream_plan(window, step)
    qkv, kv_len = TW._dev(d['qkv']), _i32(lens)
    ring = torch.full((R, n_pad, 2 * D + 4), fill, dtype=torch.float32, device='cuda:0')
    out = torch.full((T, n_pad, D + 4), 7.0, dtype=torch.float32, device='cuda:0')
    if kind == 'rel':
        P = window[1] + window[0]
        # the rows of the whole-utterance table at the relative indices -(P - 1) .. P - 1
        pos = TW._dev(d['pos'][T - P:T + P - 1])
        bu, bv = TW._dev(d['bias_u']), TW._dev(d['bias_v'])
    for t0 in range(0, T, step):
        q = qkv[t0:t0 + step]
        ops.ring_put(q, ring, t0, col0=D, cols=2 * D)
        if kind == 'attn':
            ops.attn_stream_fwd(q, ring, kv_len, out[t0:t0 + step], N, heads, dh, t0, window)
        else:
            ops.relattn_stream_fwd(q, ring, kv_len, pos, bu, bv, out[t0:t0 + step], N, heads, dh,
                                   t0, window)
    torch.cuda.synchronize()
    return out.cpu().numpy(), R


def _whole_attn(kind, d, N, heads, dh, lens, window):
    from asr_study_amd import ops
    T, n_pad, _ = d['qkv'].shape
    out = torch.full((T, n_pad, heads * dh + 4), 7.0, dtype=torch.float32, device='cuda:0')
    if kind == 'attn':
        ops.attn_fwd(TW._dev(d['qkv']), out, N, heads, dh, lens=_i32(lens), window=window)
    else:
        ops.relattn_fwd(TW._dev(d['qkv']), TW._dev(d['pos']), TW._dev(d['bias_u']),
                        TW._dev(d['bias_v']), out, N, heads, dh, lens=_i32(lens), window=window)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _attn_case(window, heads, dh, seed=0):
    """T = 2 R + 7 with R the ring of the largest step: every ring wraps at least twice."""
    from asr_study_amd import ops
    rs = np.random.RandomState(seed)
    N = 3
    T = 2 * max(ops.attn_stream_plan(window, s) for s in _steps(window)) + 7
    lens = np.array([T, 65, 7])
    return TW._make(rs, T, N, N_PAD, heads, dh, lens), N, T, lens


# (the relative family refuses dh > 64)
STREAM_HEADS = [(heads, dh, kind) for heads, dh in [(2, 16), (1, 64), (1, 48), (1, 128)]
                for kind in ('attn', 'rel') if kind == 'attn' or dh <= 64]


@pytest.mark.parametrize('heads,dh,kind', STREAM_HEADS, ids=['%d-%d-%s' % c for c in STREAM_HEADS])
@pytest.mark.parametrize('window', WINDOWS, ids=['%d_%d_%d' % w for w in WINDOWS])
def test_streamed_attention_is_the_whole_utterance_kernel(kind, window, heads, dh):
    """Bit for bit the rows of asr_*_win_fwd on the whole qkv slab, for every step; lengths that
    end inside a chunk (T), one past a tile boundary (65) and inside the first tile (7)."""
    d, N, T, lens = _attn_case(window, heads, dh)
    D = heads * dh
    whole = _whole_attn(kind, d, N, heads, dh, lens, window)
    want = TW._oracle(kind, d, N, heads, dh, lens, window)['out']
    for step in _steps(window):
        got, R = _stream_attn(kind, d, N, heads, dh, lens, window, step)
        assert T >= 2 * R + 7 and R % 64 == 0
        for n in range(N):
            assert np.array_equal(got[:lens[n], n, :D], whole[:lens[n], n, :D]), (step, n)
            e = TW._rel(got[:lens[n], n, :D], want[:lens[n], n])
            assert e < TW.BOUND, (step, n, e)
        assert np.isfinite(got).all()
        assert not got[:, N:].any() and not got[:, :, D:].any()     # pad rows, pad columns


@pytest.mark.parametrize('kind', ['attn', 'rel'])
@pytest.mark.parametrize('window', [(4, 8, 0), (16, 64, 0), (1, 0, 0)])
def test_stale_ring_rows_reach_nothing(kind, window):
    """A ring that starts filled with 1e30 instead of zeros gives the same bits: what a ring row
    holds of a frame outside the window (or of no frame yet) meets a select, never a product."""
    d, N, T, lens = _attn_case(window, 2, 16, seed=1)
    step = _steps(window)[-1]
    a, _ = _stream_attn('attn' if kind == 'attn' else 'rel', d, N, 2, 16, lens, window, step)
    b, _ = _stream_attn('attn' if kind == 'attn' else 'rel', d, N, 2, 16, lens, window, step,
                        fill=1e30)
    assert np.isfinite(b).all()
    for n in range(N):
        assert np.array_equal(a[:lens[n], n], b[:lens[n], n]), n


# ----------------------------------------------------------------------------- depthwise convolution
@pytest.mark.parametrize('k', [1, 3, 31, 63])
def test_streamed_dwconv_is_the_causal_whole_utterance_kernel(k):
    from asr_study_amd import ops
    rs = np.random.RandomState(k)
    T, N, C = 130, 4, 8
    lens = np.array([0, 1, 64, 130])
    x = (rs.randn(T, N_PAD, C) * 3.0).astype(np.float32)
    x[:, :N] = rs.randn(T, N, C).astype(np.float32)
    w, b = rs.randn(k, C).astype(np.float32), rs.randn(C).astype(np.float32)
    xd, wd, bd, ld = TW._dev(x), TW._dev(w), TW._dev(b), _i32(lens)
    whole = torch.full_like(xd, 7.0)
    ops.dwconv1d_fwd(xd, wd, bd, whole, N, k, lens=ld, pad_left=k - 1)
    whole = whole.cpu().numpy()
    for step in (5, 16, 64):
        ring = torch.zeros((k - 1 + step, N_PAD, C), dtype=torch.float32, device='cuda:0')
        got = torch.full_like(xd, 7.0)
        for t0 in range(0, T, step):
            ops.ring_put(xd[t0:t0 + step], ring, t0)
            ops.dwconv1d_stream_fwd(ring, wd, bd, ld, got[t0:t0 + step], N, k, t0)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert np.array_equal(got[:, :N], whole[:, :N]), step
        assert not got[:, N:].any()
    y64, _ = WO.dwconv_forward(x[:, :N].astype(np.float64), w.astype(np.float64),
                               b.astype(np.float64), k - 1, lens)
    assert TW._rel(whole[:, :N], y64) < TW.BOUND


# ----------------------------------------------------------------------------- greedy
def _crafted_logits():
    """C = 5 (blank 4), T = 40, two streams.  At the boundaries of the steps 3 and 16: a label
    repeated across 15 | 16 and 2 | 3, label-blank-label over 31 .. 33 and 5 .. 7, blanks over
    9 | 10 | 11 and 17 | 18, and one tie (the first maximum wins)."""
    path = [0, 0, 0, 0, 1, 1, 4, 1, 4, 4, 4, 4, 2, 2, 4, 3, 3, 3, 4, 4, 0, 2, 2, 1, 4, 4, 0, 0, 3, 3,
            3, 1, 4, 1, 1, 2, 4, 0, 4, 4]
    assert len(path) == 40
    rs = np.random.RandomState(3)
    lg = rs.rand(40, N_PAD, 5).astype(np.float32)
    for t, c in enumerate(path):
        lg[t, 0, c] += 2.0
        lg[t, 1, path[(t + 7) % 40]] += 2.0
    lg[20, 0, :] = [1.0, 1.0, 0.5, 0.0, 0.2]            # a tie: label 0
    return lg, np.array([40, 17])


@pytest.mark.parametrize('step', [1, 3, 16])
def test_streamed_greedy_is_the_whole_utterance_decoder(step):
    from asr_study_amd import ops
    lg, lens = _crafted_logits()
    N, T = 2, 40
    lgd = TW._dev(lg)
    dec, dlen = ops.ctc_greedy(lgd, _i32(lens), N)
    dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
    want = [dec[n, :dlen[n]].tolist() for n in range(N)]
    assert want == WO.greedy(lg[:, :N].astype(np.float64), lens) and len(want[0]) > 10
    state = torch.full((N,), -1, dtype=torch.int32, device='cuda:0')
    got, last = [[] for _ in range(N)], [-1] * N
    for t0 in range(0, T, step):
        cl = np.clip(lens - t0, 0, min(step, T - t0))
        d, dl = ops.ctc_greedy_stream(lgd[t0:t0 + step], _i32(cl), state, N)
        d, dl = d.cpu().numpy(), dl.cpu().numpy()
        add, last = SO.greedy_chunk(lg[t0:t0 + step, :N], cl, last)
        for n in range(N):
            assert d[n, :dl[n]].tolist() == add[n] and (d[n, dl[n]:] == -1).all()
            got[n] += add[n]
        assert state.cpu().numpy().tolist() == last
    assert got == want


# ----------------------------------------------------------------------------- models
def _feed_all(ss, x, lens, pieces):
    """x (N, T, F) in pieces; a stream's length is told with the piece that carries its last
    frame.  -> the results of every feed and of finish, frames_out after each feed."""
    outs, emitted, pos = [], [], 0
    for p in pieces:
        ended = None if lens is None else [int(l) if pos < l <= pos + p else None for l in lens]
        outs.append(ss.feed(x[:, pos:pos + p], ended))
        emitted.append(ss.frames_out)
        pos += p
    outs.append(ss.finish())
    return outs, emitted


def _stream_parity(model, x, lens, pieces, tag, x_whole=None):
    """Streamed logits of the valid frames against the float64 oracle of the whole utterance
    (1e-4, the model bound of tests/test_gpu_window.py), the device difference to Model.predict's
    logits (printed), the streamed greedy labels against Model.predict's."""
    N = x.shape[0]
    x_whole = x if x_whole is None else x_whole
    stages = WO.stages_from_model(model)
    x64 = model.to_slab(x_whole)[:, :N].cpu().numpy().astype(np.float64)
    want, _ = WO.model_forward(stages, x64, lens, training=False)
    out_lens = model.out_lengths(np.asarray(lens))
    model.decoder = None
    whole = model.predict(x_whole, lens)
    ss = model.stream(n_streams=N)
    outs, emitted = _feed_all(ss, x, lens, pieces)
    got = np.concatenate(outs, 1)
    assert got.shape == whole.shape == (N,) + want.shape[::2], (got.shape, whole.shape)
    assert ss.frames_in == x.shape[1] and ss.frames_out == got.shape[1]
    e = max(TW._rel(got[n, :out_lens[n]], want[:out_lens[n], n]) for n in range(N))
    dev = max(TW._rel(got[n, :out_lens[n]], whole[n, :out_lens[n]]) for n in range(N))
    print('[stream] %s: logits vs float64 oracle %.3e, vs Model.forward on the device %.3e'
          % (tag, e, dev))
    assert e < 1e-4, (tag, e)
    model.decoder = {'is_greedy': True}
    labels = model.predict(x_whole, lens)
    ss = model.stream(n_streams=N)
    outs, _ = _feed_all(ss, x, lens, pieces)
    assert [sum((o[n] for o in outs), []) for n in range(N)] == labels, tag
    return ss, emitted


PIECES = [1, 7, 13, 3, 16]
LENS = np.array([40, 33, 9])


@pytest.mark.parametrize('build', ['blocks', 'conformer'])
def test_streamed_models_vs_oracle(build):
    rs = np.random.RandomState(21)
    model = TW._blocks((4, 8, 0)) if build == 'blocks' else TW._conformer()
    TW._randomise(model, rs)
    x = TW._batch(rs, 3, 40, 10, LENS)
    ss, emitted = _stream_parity(model, x, LENS, PIECES, build)
    assert ss.step == 16 and emitted == [0, 0, 16, 16, 32]


def test_streamed_model_with_batch_norm_on_its_running_moments():
    rs = np.random.RandomState(22)
    model = TW._conformer(conv_norm='batch')
    TW._randomise(model, rs)
    x = TW._batch(rs, 3, 40, 10, LENS)
    before = model.bn_running.clone()
    labels = [rs.randint(0, 7, size=k).tolist() for k in (3, 2, 1)]
    for _ in range(2):
        model.train_on_batch([('slab', model.to_slab(x)), labels, LENS])
    assert not torch.equal(before, model.bn_running)        # not the initial moments
    _stream_parity(model, x, LENS, PIECES, 'conformer, batch norm')


def _front_end_model(rs):
    model = TW._conformer(context=(4, 8, 0), num_features=16, conv=True, conv_filters=4,
                          conv_kernels=((5, 7), (3, 5)))
    TW._randomise(model, rs)
    return model


def test_streamed_model_with_the_front_end():
    """kernels (5, 7) and (3, 5), T = 80 input frames in pieces that cut through windows; the
    strided frames emitted after each feed are those of the reach formula."""
    rs = np.random.RandomState(23)
    model = _front_end_model(rs)
    lens = np.array([80, 61, 18])
    pieces = [3, 22, 1, 30, 24]
    x = TW._batch(rs, 3, 80, 16, lens)
    ss, emitted = _stream_parity(model, x, lens, pieces, 'front-end')
    reach = lambda t: 2 * (t // 16 * 16 + 16 - 1 + (3 - 1) // 2) + 5 - 1 - (5 - 2) // 2
    want = [len([t for t in range(40) if reach(t) < fed]) // 16 * 16 for fed in np.cumsum(pieces)]
    assert emitted == want == [0, 0, 0, 16, 32], (emitted, want)


def test_streamed_model_with_an_odd_number_of_input_frames():
    """T = 79: the session appends one zero frame at finish() and equals the full forward of
    that slab of 80 frames."""
    rs = np.random.RandomState(24)
    model = _front_end_model(rs)
    x = rs.randn(2, 79, 16).astype(np.float32)
    x80 = np.concatenate([x, np.zeros((2, 1, 16), np.float32)], 1)
    _stream_parity(model, x, np.array([79, 79]), [3, 22, 1, 30, 23], 'odd T', x_whole=x80)


def test_reset_gives_the_bits_of_a_fresh_session():
    rs = np.random.RandomState(25)
    model = TW._conformer()
    TW._randomise(model, rs)
    model.decoder = None
    x1, x2 = TW._batch(rs, 3, 40, 10, LENS), TW._batch(rs, 3, 40, 10, LENS)
    ss = model.stream(n_streams=3)
    first = np.concatenate(_feed_all(ss, x1, LENS, PIECES)[0], 1)
    with pytest.raises(RuntimeError):
        ss.feed(x2[:, :1])
    ss.reset()
    assert ss.frames_in == ss.frames_out == 0
    again = np.concatenate(_feed_all(ss, x2, LENS, PIECES)[0], 1)
    fresh = np.concatenate(_feed_all(model.stream(n_streams=3), x2, LENS, PIECES)[0], 1)
    assert np.array_equal(again, fresh) and not np.array_equal(first, again)
    # a length that lies before frames already emitted as the stream's is refused
    ss.reset()
    ss.feed(x1[:, :20])
    assert ss.frames_out == 16
    with pytest.raises(ValueError):
        ss.feed(x1[:, 20:21], ended=[12, None, None])


# ----------------------------------------------------------------------------- the command line
def test_cli_roundtrip_predict_stream(tmp_path):
    sys.path.insert(0, ROOT)
    import train
    import predict as predict_cli
    from asr_study_amd import cli
    from asr_study_amd.datasets import h5lite
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
    # The run without --stream: predict.py decodes with a beam search of width 400 there, whose
    # hypotheses are not the greedy ones on a barely trained model ('nr' against ''), so the
    # comparison is made where the two runs decode alike: the network outputs of both runs, and
    # the streamed hypotheses against the greedy decode of the non-streaming outputs.
    plain = predict_cli.main(['--model', best, '--dataset', fname, '--no_decoder'])
    raw = predict_cli.main(['--model', best, '--dataset', fname, '--no_decoder', '--stream', '80'])
    streamed = predict_cli.main(['--model', best, '--dataset', fname, '--stream', '80'])
    assert len(streamed) == len(raw) == len(plain) > 0
    # An utterance with an ODD number of input frames: the session appends one zero frame and
    # equals the full forward of that even slab (the 'same' rule of the strided convolution
    # aligns its taps by the parity of T), so the reference of every utterance is Model.predict
    # on its even slab; for an even T that is the run without --stream itself.
    from asr_study_amd.datasets.dataset_generator import DatasetGenerator
    from asr_study_amd.utils import core_utils, generic_utils
    parser = generic_utils.get_from_module('preprocessing.text', 'simple_char_parser', params=[])
    flow = DatasetGenerator(None, parser, batch_size=1, seed=0, mode='predict',     # (stored features)
                            shuffle=False).flow_from_fname(fname, datasets='test')
    model = core_utils.load_model(best, mode='predict', decoder=False)
    assert flow.len == len(plain)
    even = 0
    for p, r, s in zip(plain, raw, streamed):
        x, lens = flow.next()
        T = int(np.asarray(lens).reshape(-1)[0])
        x = np.asarray(x, np.float32)[:, :T]
        if T % 2:
            x = np.concatenate([x, np.zeros((1, 1, x.shape[2]), np.float32)], 1)
        want = model.predict(x, [T])[0]
        e = TW._rel(r['best'], want)
        print('[stream] cli: T %d, streamed vs the even slab %.3e, vs the run without --stream '
              '%.3e' % (T, e, TW._rel(r['best'], p['best'])))
        assert r['best'].shape == want.shape == p['best'].shape and e < 1e-4, (T, e)
        if T % 2 == 0:
            even += 1
            assert TW._rel(r['best'], p['best']) < 1e-4, T
        ids = WO.greedy(want[:, None, :].astype(np.float64), [len(want)])[0]
        assert s['best'] == parser.imap(ids) and s['label'] == p['label']
    assert even > 0
    # a model that cannot stream is refused with the session's message
    train.main(['--dataset', fname, '--model', 'conformer', '--model_params', 'num_features',
                '16', 'd_model', '32', 'num_heads', '2', 'num_layers', '1', 'd_ff', '64',
                'kernel_size', '7', 'num_classes', '28', 'conv', 'False', '--num_epochs', '1',
                '--batch_size', '4', '--save', out + '2', '--seed', '1'])
    with pytest.raises(ValueError) as e:
        predict_cli.main(['--model', os.path.join(out + '2', 'best.h5'), '--dataset', fname,
                          '--stream', '80'])
    assert 'cannot stream' in str(e.value)
