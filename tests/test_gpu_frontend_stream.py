"""-m gpu: the online front-end (csrc/frontend.hip: fe_finalize_running_kernel,
asr_frontend_stream).

1. The batch call with norm='running' against the float64 oracle (tests/frontend_stream_oracle.py).
   Bar per frame t and column: 2 * TOL * max(1, sd_T / (sd_t + eps)) -- TOL = 1e-4 is the bar of
   tests/test_gpu_frontend.py for the error relative to the whole-utterance standard deviation
   sd_T, the running divisor is sd_t, and the value and the running mean each carry that error;
   without mean_norm the rounding of the float32 output itself is added, 2^-24 |value|.
2. FeatureStream over any split of the signals equals the batch call bit for bit.
3. The default is norm='utterance'.
4. Model.stream(feature=...).feed_audio against Model.predict on the batch-extracted features.
5. predict.py --stream MS --stream_audio.
"""
import os
import sys

import numpy as np
import pytest
import torch

from tests import frontend_stream_oracle as FO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4                                  # tests/test_gpu_frontend.py
PIECES = (7, 159, 160, 161, 400, 401, 1000, None)


def _feature(name, **more):
    from asr_study_amd.preprocessing import audio
    _, cls, kw = FO.CONFIGS[name]
    return getattr(audio, cls)(**dict(kw, norm='running', **more))


def _batch_lengths(n_utt):
    """Mixed lengths, the longest not first.  The 17 utterances cross the pad16 boundary and hold
    every length of FO.LENGTHS (the step 2 is coprime to their number, 9), eight of them twice."""
    if n_utt == 3:
        return [561, 16000, 2]
    lens = [FO.LENGTHS[(2 * i + 1) % len(FO.LENGTHS)] for i in range(n_utt)]
    assert set(lens) == set(FO.LENGTHS)
    return lens


# ------------------------------------------------------------------------------ 1. the batch call
@pytest.mark.parametrize('name', sorted(FO.CONFIGS))
def test_batch_running_norm_against_the_oracle(name):
    kind, _, kw = FO.CONFIGS[name]
    feat = _feature(name)
    eps = 1e-8
    worst = 0.0
    for n_utt in (3, 17):
        lens = _batch_lengths(n_utt)
        sigs = [FO.signal(n, 500 + 10 * i + n_utt) for i, n in enumerate(lens)]
        slab, frames = feat.batch(sigs)
        slab, frames = slab.cpu().numpy(), frames.cpu().numpy()
        assert slab.shape[1] == (16 if n_utt == 3 else 32) and slab.dtype == np.float32
        assert np.all(slab[:, n_utt:] == 0), 'batch-padding rows'
        for i, x in enumerate(sigs):
            rows = FO.kept(kind, x, **kw)
            want = FO.running_standardize(rows, kw.get('mean_norm', True),
                                          kw.get('var_norm', True), eps)
            T = want.shape[0]
            assert frames[i] == T, (name, i, frames[i], T)
            got = slab[:T, i]
            assert np.isfinite(got).all()
            assert np.all(slab[T:, i] == 0), 'past the utterance'
            sd = FO.running_sd(rows)
            bar = 2 * TOL * np.maximum(1.0, sd[-1][None, :] / (sd + eps))
            if not kw.get('mean_norm', True):
                # ... plus the rounding of the float32 the value is written as, half an ulp of
                # it: without mean_norm frame 0 is x / eps, about 1e9, which no float32 holds to
                # 2e-4 (sd_T = sd_0 = 0 for a one-frame utterance)
                bar = bar + 2.0 ** -24 * np.abs(want)
            ratio = float((np.abs(got - want) / bar).max())
            worst = max(worst, ratio)
            assert ratio < 1.0, (name, n_utt, i, lens[i], ratio)
            if kw.get('mean_norm', True):
                assert np.all(got[0] == 0), 'frame 0 is exactly 0 under mean_norm'
                if name == 'lfb80':
                    assert np.all(got[:, list(FO.EMPTY_FILTERS_80)] == 0), 'empty filters'
    print('[frontend-stream] %s: worst error / bar %.3e' % (name, worst))


# ------------------------------------------------------------------------------ 2. streaming
def _run_stream(fs, sigs, piece, tell_end=True):
    """Feeds the signals in lock-step in pieces of ``piece`` samples (None: all at once), a
    stream's length with the feed that carries its last sample (tell_end) or at finish() ->
    the rows per stream (t, F) on the device.  Checks the row count of every feed against
    FrameSchedule."""
    from asr_study_amd.preprocessing import audio
    N, lens = len(sigs), [len(s) for s in sigs]
    top = max(lens)
    x = np.zeros((N, top), np.float32)
    for i, s in enumerate(sigs):
        x[i, :len(s)] = s
    x = torch.from_numpy(x).cuda()
    sc = audio.FrameSchedule(fs.cfg.frame_len, fs.cfg.frame_step, fs.lookahead_frames,
                             fs.cfg.stride)
    outs, known = [], [None] * N
    for lo, hi in FO.pieces(top, piece):
        ended = None
        if tell_end:
            ended = [n if lo < n <= hi else None for n in lens]
            known = [n if n <= hi else None for n in lens]
        before = fs.frames_out
        out = fs.feed(x[:, lo:hi], ended)
        want_rows = sc.kept(sc.window(hi, known))
        assert fs.samples_in == hi and fs.frames_out == want_rows, (piece, hi, fs.frames_out)
        assert tuple(out.shape) == (N, want_rows - before, fs.feature.num_feats)
        outs.append(out)
    outs.append(fs.finish())
    assert fs.frames_out == max(fs.frames_of(n) for n in lens)
    return torch.cat(outs, 1)


def _check_stream(feat, sigs, pieces, fs=None):
    slab, frames = feat.batch(sigs)
    frames = frames.cpu().numpy()
    N = len(sigs)
    fresh = fs is None
    fs = fs or feat.stream(N)
    for k, piece in enumerate(pieces):
        if k or not fresh:
            fs.reset()
        got = _run_stream(fs, sigs, piece)
        assert got.shape[1] == slab.shape[0]
        for i in range(N):
            assert fs.frames_of(len(sigs[i])) == frames[i]
            assert torch.equal(got[i], slab[:, i]), (piece, i, len(sigs[i]))
    return fs


@pytest.mark.parametrize('name', sorted(FO.CONFIGS))
def test_streaming_equals_batch_bit_for_bit(name):
    feat = _feature(name)
    # one stream: a second of audio, pieces around the frame step and the frame length
    _check_stream(feat, [FO.signal(16000, 11)], PIECES[1:])
    fs = _check_stream(feat, [FO.signal(1999, 12)], (7,))
    # 561 feeds of one sample: calls that only append to the carry between calls that emit
    _check_stream(feat, [FO.signal(561, 13)], (1,), fs)
    # three streams that end in different feeds: 1120 = 7 * 160 ends on a piece boundary of the
    # 7-, 160- and (400 samples) the 400-sample pieces; one stream is a single zero-padded frame
    sigs = [FO.signal(n, 20 + n) for n in (1999, 400, 1120)]
    _check_stream(feat, sigs, PIECES)
    # seventeen streams across the pad16 boundary
    lens = [FO.LENGTHS[:-1][(3 * i + 1) % 8] for i in range(16)] + [1120]
    _check_stream(feat, [FO.signal(n, 40 + i) for i, n in enumerate(lens)], PIECES)


def test_the_end_may_arrive_with_finish_and_reset_repeats_the_bits():
    feat = _feature('mfcc39')
    sigs = [FO.signal(1999, 3)]
    slab, _ = feat.batch(sigs)
    fs = feat.stream(1)
    assert fs.lookahead_frames == 4 and fs.samples_in == fs.frames_out == 0
    first = _run_stream(fs, sigs, 160, tell_end=False)
    assert torch.equal(first[0], slab[:, 0])
    with pytest.raises(RuntimeError):
        fs.feed(np.zeros((1, 10), np.float32))
    fs.reset()
    assert fs.samples_in == fs.frames_out == 0
    again = _run_stream(fs, sigs, 160, tell_end=False)
    assert torch.equal(first, again)
    # a length that lies before the samples already fed is refused; the wrong shape too
    fs.reset()
    fs.feed(np.zeros((1, 800), np.float32))
    with pytest.raises(ValueError):
        fs.feed(np.zeros((1, 10), np.float32), ended=[700])
    with pytest.raises(ValueError):
        fs.feed(np.zeros((2, 10), np.float32))
    # a length given ahead and not reached: finish() is refused, the stream goes on
    fs.reset()
    x = torch.from_numpy(np.asarray(sigs[0], np.float32))[None].cuda()
    rows = [fs.feed(x[:, :800], ended=[1999])]
    with pytest.raises(ValueError, match='1999'):
        fs.finish()
    rows += [fs.feed(x[:, 800:]), fs.finish()]
    assert torch.equal(torch.cat(rows, 1)[0], slab[:, 0])


# ------------------------------------------------------------------------------ 3. the default
def test_the_default_is_utterance_normalisation():
    from asr_study_amd.preprocessing import audio
    sigs = [FO.signal(n, 70 + n) for n in (1999, 561, 16000)]
    for cls, kw in ((audio.MFCC, {}), (audio.LogFbank, {'num_filt': 80})):
        a, fa = cls(**kw).batch(sigs)
        b, fb = cls(norm='utterance', **kw).batch(sigs)
        c, _ = cls(norm='running', **kw).batch(sigs)
        assert torch.equal(a, b) and torch.equal(fa, fb)
        assert not torch.equal(a, c)


# ------------------------------------------------------------------------------ 4. end to end
def _models(which):
    from asr_study_amd.core import models, optimizers
    from asr_study_amd.preprocessing import audio
    if which == 'brsmv1':
        feat = audio.MFCC(norm='running')
        m = models.brsmv1(num_features=39, num_classes=8, num_hiddens=16, num_layers=1,
                          bidirectional=False, dropout=0, seed=1)
    else:
        feat = audio.LogFbank(num_filt=16, norm='running')
        # (d_model = 32, not 16: the relative-attention kernels take head widths of 16 .. 64,
        # and two heads of 8 do not exist)
        m = models.conformer(num_features=16, num_classes=8, d_model=32, num_heads=2,
                             num_layers=1, kernel_size=3, positions='relative',
                             context=[4, 8, 0], causal_conv=True, seed=1)
    m.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    return m, feat


@pytest.mark.parametrize('which', ['brsmv1', 'conformer'])
@pytest.mark.parametrize('N', [1, 3])
def test_audio_streaming_end_to_end(which, N):
    from tests.test_gpu_window import _rel
    model, feat = _models(which)
    lens = [16000, 9000, 12345][:N]
    sigs = [0.1 * FO.signal(n, 90 + n) for n in lens]
    # (99 frames: under the conformer's convolution front-end the session equals the full
    # forward of the slab with one zero frame appended, StreamSession.finish)
    slab, frames = feat.batch(sigs, t_out=100 if which == 'conformer' else 99)
    frames = frames.cpu().numpy()
    assert frames.max() == 99
    x = np.zeros((N, 16000), np.float32)
    for i, s in enumerate(sigs):
        x[i, :len(s)] = s

    def run(session):
        outs = []
        for lo in range(0, 16000, 1600):
            hi = lo + 1600
            outs.append(session.feed_audio(x[:, lo:hi],
                                           [n if lo < n <= hi else None for n in lens]))
        outs.append(session.finish_audio())
        return outs

    model.decoder = None
    whole = model.predict(('slab', slab), frames)
    ss = model.stream(n_streams=N, feature=feat)
    got = np.concatenate(run(ss), 1)
    assert got.shape == whole.shape
    out_lens = model.out_lengths(frames)
    e = max(_rel(got[n, :out_lens[n]], whole[n, :out_lens[n]]) for n in range(N))
    print('[frontend-stream] %s, %d streams: logits vs Model.predict %.3e' % (which, N, e))
    assert e < 1e-4, (which, N, e)
    model.decoder = {'is_greedy': True}
    labels = model.predict(('slab', slab), frames)
    outs = run(model.stream(n_streams=N, feature=feat))
    assert [sum((o[n] for o in outs), []) for n in range(N)] == labels
    with pytest.raises(RuntimeError, match='feature'):
        model.stream(n_streams=N).feed_audio(x[:, :1600])


# ------------------------------------------------------------------------------ 5. the command line
def test_cli_predict_stream_audio(tmp_path, capsys):
    """A dataset of raw audio (no input parser at make_dataset), two tiny models trained with the
    parser running on the fly -- one with ``norm running``, one without -- so that the parser and
    its parameters are in the checkpoints; predict.py is then given NO parser flags."""
    sys.path.insert(0, ROOT)
    import train
    import predict as predict_cli
    from scipy.io import wavfile
    from asr_study_amd import cli
    from asr_study_amd.datasets import h5lite
    from asr_study_amd.utils.core_utils import load_meta
    from tests import window_oracle as WO
    from tests.test_gpu_window import _rel
    fmt = 'h5' if h5lite.available() else 'npz'
    parser = ['--input_parser', 'logfbank', '--input_parser_params', 'num_filt', '16']
    wav = str(tmp_path / 'x.wav')
    rs = np.random.RandomState(5)
    wavfile.write(wav, 16000, np.round(3000 * rs.randn(16000)).astype(np.int16))
    fname = str(tmp_path / ('dummy.' + fmt))
    cli.make_dataset_main(['--parser', 'dummy', '--parser_params', 'num_speakers', '4',
                           'num_utterances_per_speaker', '6', 'max_duration', '1.2',
                           'min_duration', '0.6', 'max_label_length', '8', 'split',
                           '[0.5, 0.25]', 'seed', '3', '--output_file', fname])
    best = {}
    for norm, extra in (('running', ['norm', 'running']), ('utterance', [])):
        out = str(tmp_path / ('run_' + norm))
        train.main(['--dataset', fname, '--model', 'brsmv1', '--model_params', 'num_features',
                    '16', 'num_hiddens', '16', 'num_layers', '1', 'bidirectional', 'False',
                    '--num_epochs', '1', '--batch_size', '4', '--save', out, '--seed', '1',
                    '--lr', '0.001'] + parser + extra)
        best[norm] = os.path.join(out, 'best.h5')
    stored = load_meta(best['running'])['training_args']
    assert stored['input_parser'] == 'logfbank'
    assert [str(v) for v in stored['input_parser_params']] == ['num_filt', '16', 'norm', 'running']
    from asr_study_amd.cli import utils
    text = utils.get_from_module('preprocessing.text', 'simple_char_parser', params=[])

    def greedy(logits):
        # the non-streamed run's string, decoded as the session decodes (greedy; predict.py's
        # own decoder there is a beam search of width 400, which a barely trained model does not
        # follow)
        return text.imap(WO.greedy(logits[:, None, :].astype(np.float64), [len(logits)])[0])

    # ---- one file
    plain = predict_cli.main(['--model', best['running'], '--file', wav, '--no_decoder'])
    raw = predict_cli.main(['--model', best['running'], '--file', wav, '--no_decoder',
                            '--stream', '100', '--stream_audio'])
    assert raw[0]['best'].shape == plain[0]['best'].shape
    assert _rel(raw[0]['best'], plain[0]['best']) < 1e-4
    capsys.readouterr()
    streamed = predict_cli.main(['--model', best['running'], '--file', wav, '--stream', '100',
                                 '--stream_audio'])
    printed = capsys.readouterr().out
    assert printed.count('frames in:') == 10 and 'Predicted:' in printed
    assert streamed[0]['best'] == greedy(plain[0]['best'])
    # ---- a dataset whose input parser runs on the fly
    plain = predict_cli.main(['--model', best['running'], '--dataset', fname, '--no_decoder'])
    streamed = predict_cli.main(['--model', best['running'], '--dataset', fname, '--stream',
                                 '100', '--stream_audio'])
    assert len(streamed) == len(plain) > 0
    for p, r in zip(plain, streamed):
        assert r['best'] == greedy(p['best']) and r['label'] == p['label']
    # ---- the model whose stored input parser is utterance-normalised is refused
    with pytest.raises(ValueError, match='--input_parser_params norm running'):
        predict_cli.main(['--model', best['utterance'], '--file', wav, '--stream', '100',
                          '--stream_audio'])
