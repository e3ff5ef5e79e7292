"""-m gpu: MFCC / log-mel front-end through the product classes vs the golden
vectors generated from the reference's own code (tests/golden) and the oracle.
Tolerance on the standardised (unit-variance) features: 1e-4 absolute (the north-star
bar): the per-frame chain runs in float64 like the reference (csrc/frontend.hip), so what
remains is the float32 cast of the input samples (<= 6e-6, measured with the oracle) and of
the output.

The second half runs the table of tests/frontend_cases.py (every frame, column and batch edge of
fe_frames_kernel, fe_finalize_kernel<8|16> and fe_zero_pad_rows_kernel) against the float64 oracle
computed on the spot, with float32-exact inputs, and the raw C entry points into a guarded,
sentinel-filled slab.  Bars: TOL for standardised features, TOL * max(1, max|want|) for
mfcc_nomean (un-shifted values), 1e-5 * max(1, max|want|) for the un-normalised configurations
(the bar of test_no_norm_and_properties), exactly 0 for digital silence; the batch equalities are
bit for bit.  Worst |err| measured on the MI355X per configuration (test_table_against_oracle):
    mfcc39 2.3e-07   mfcc13 1.2e-07   mfcc26 1.2e-07   lfb80 8.5e-06   lfb64 1.9e-07
    lfb21_d_dd 1.2e-07   lfb65 2.3e-07   lfb128_full 5.0e-06   mfcc26x26 1.2e-07
    mfcc_w512 1.2e-07   mfcc_w320_s80 1.2e-07   mfcc_8k 2.3e-07   mfcc_pe0 1.5e-07
    mfcc_novar 9.5e-07                                                     (bar: TOL = 1e-4)
    lfb41_d_dd_s3c1 1.8e-05   mfcc39_s2c2 1.5e-05    (TOL; <= 1.4e-5 of it is the reference's
                                                      float32 cast before it standardises)
    mfcc_nomean 1.9e-06 (0.0004 of TOL * max|want|)
    mfcc39_raw 1.9e-06 (0.004 of 1e-5 * max|want|)
    lfb41_d_dd_s3c1_raw 7.1e-16   mfcc39_s2c2_raw 2.8e-15   (both sides float32 there)
'silence' is left out of these figures: the kernel gives exactly 0 there, the reference <= 1.8e-6.
No later bar is set from them here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import frontend as OF
from tests import frontend_cases as FC

pytestmark = pytest.mark.gpu
TOL = 1e-4

CONFIGS = {
    'mfcc39': ('MFCC', {}),
    'mfcc26': ('MFCC', {'dd': False}),
    'mfcc13': ('MFCC', {'d': False, 'dd': False}),
    'logfbank40': ('LogFbank', {}),
    'logfbank80': ('LogFbank', {'num_filt': 80}),
    'logfbank41_d_dd': ('LogFbank', {'append_energy': True, 'd': True, 'dd': True}),
    'mfcc39_s2c2': ('MFCC', {'stride': 2, 'num_context': 2}),
}


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_against_reference_golden(name, golden_dir):
    from asr_study_amd.preprocessing import audio
    from tests.gpu_util import report
    cls, kw = CONFIGS[name]
    feat = getattr(audio, cls)(**kw)
    g = np.load(os.path.join(golden_dir, 'frontend_%s.npz' % name))
    worst = 0.0
    for key in g.files:
        parts = key.split('_')
        n, seed = int(parts[0][1:]), int(parts[1][1:])
        x = np.random.RandomState(seed).randn(n)
        y = feat(x)
        assert y.shape == g[key].shape, (key, y.shape, g[key].shape)
        report('%s %s' % (name, key), y, g[key])
        worst = max(worst, float(np.max(np.abs(y - g[key]))) if y.size else 0.0)
    assert worst < TOL


def test_ragged_batch_into_time_major_slab():
    from asr_study_amd.preprocessing import audio
    rs = np.random.RandomState(0)
    lens = [16000, 300, 52345, 401, 160000, 8000]
    sigs = [rs.randn(n) for n in lens]
    feat = audio.MFCC()
    slab, frames = feat.batch(sigs)              # (T, n_pad, 39) CUDA, frames (N,)
    torch.cuda.synchronize()
    slab = slab.cpu().numpy()
    frames = frames.cpu().numpy()
    assert slab.shape[1] == 16 and slab.shape[2] == 39
    for i, s in enumerate(sigs):
        want = OF.extract('mfcc', s)
        assert frames[i] == want.shape[0]
        assert np.abs(slab[:frames[i], i] - want).max() < TOL
        assert np.all(slab[frames[i]:, i] == 0)           # pad_sequences 'post'
    assert np.all(slab[:, len(sigs):] == 0)               # batch padding rows


def test_no_norm_and_properties():
    from asr_study_amd.preprocessing import audio
    x = np.random.RandomState(5).randn(20000)
    y = audio.LogFbank(num_filt=80)(x)
    # empty mel filters 1 and 7 -> constant column -> exactly 0
    assert np.all(y[:, 1] == 0) and np.all(y[:, 7] == 0)
    assert np.abs(y.mean(0)).max() < 1e-4
    live = [c for c in range(80) if c not in (1, 7)]
    assert np.abs(y[:, live].std(0) - 1).max() < 1e-3
    y2 = audio.MFCC(mean_norm=False, var_norm=False)(x)
    want = OF.extract('mfcc', x, mean_norm=False, var_norm=False)
    assert np.abs(y2 - want).max() < 1e-5 * max(1.0, np.abs(want).max())


# ----------------------------------------------------------------------- tests/frontend_cases.py
def _feat(name, **more):
    from asr_study_amd.preprocessing import audio
    c = FC.CONFIGS[name]
    return getattr(audio, c.cls)(**dict(c.kw, **more))


def _want(name, x):
    with np.errstate(all='ignore'):
        return np.asarray(FC.want(name, x), np.float64)


def _bar(name, want):
    top = max(1.0, float(np.abs(want).max())) if want.size else 1.0
    if FC.is_raw(name):
        return 1e-5 * top
    if name == 'mfcc_nomean':
        return TOL * top
    return TOL


def _check(name, what, got, want, kind='noise'):
    """Shape (the frame count) first, then the values; returns err / bar."""
    assert got.shape == want.shape, (name, what, got.shape, want.shape)
    assert got.dtype == np.float32 and np.isfinite(got).all(), (name, what)
    bar = _bar(name, want)
    if kind == 'silence':
        assert np.all(got == 0), (name, what, 'silence must standardise to exactly 0')
        assert np.abs(want).max() < TOL
    err = float(np.abs(got - want).max())
    assert err < bar, (name, what, err, bar)
    return err, err / bar


@pytest.mark.parametrize('name', list(FC.CONFIGS))
def test_table_against_oracle(name):
    """Every case of the configuration through feat(x) and, all at once, through feat.batch."""
    feat = _feat(name)
    cases = FC.cases(name)
    sigs = [FC.signal(name, c) for c in cases]
    wants = [_want(name, x) for x in sigs]
    # (the worst figure leaves 'silence' out: there the kernel is exactly 0 and the difference is
    # the reference's own, the rounding of its mean)
    worst, worst_ratio, at = 0.0, 0.0, None
    for c, x, w in zip(cases, sigs, wants):
        err, ratio = _check(name, c, feat(x), w, c.kind)
        if ratio >= worst_ratio and c.kind != 'silence':
            worst, worst_ratio, at = err, ratio, c
    slab, frames = feat.batch(sigs)
    torch.cuda.synchronize()
    slab, frames = slab.cpu().numpy(), frames.cpu().numpy()
    assert slab.shape == (max(w.shape[0] for w in wants), (len(sigs) + 15) // 16 * 16,
                          FC.CONFIGS[name].f_out)
    for i, (c, w) in enumerate(zip(cases, wants)):
        assert frames[i] == w.shape[0], (name, c, frames[i])
        err, ratio = _check(name, ('batch', c), slab[:frames[i], i], w, c.kind)
        if ratio >= worst_ratio and c.kind != 'silence':
            worst, worst_ratio, at = err, ratio, ('batch', c)
        assert np.all(slab[frames[i]:, i] == 0), (name, c)
    assert np.all(slab[:, len(sigs):] == 0)
    print('[frontend] %-20s %3d cases: worst |err| %.3e = %.4f of its bar, at %s'
          % (name, len(cases), worst, worst_ratio, at))


# ------------------------------------------------------------------ raw entry point, guarded slab
def _launch(feat, sigs, n_pad, t_out, ws=None):
    """asr_frontend_mfcc_batch / asr_frontend_logfbank_batch into a sentinel-filled slab between
    two guard bands, with a workspace of the test's own (NaN bit patterns unless handed in: a
    read of anything the call did not write shows).  Returns (out, frames, ws), not yet read."""
    from asr_study_amd import _lib as L
    from tests.gpu_util import to_dev
    from tests.test_gpu_flat import Guarded
    if feat._tables is None:
        feat._build_tables()
    cfg, tables = feat._tables
    lib = L.load()
    lens = [int(len(s)) for s in sigs]
    n_utt = len(sigs)
    audio = to_dev(np.concatenate([np.asarray(s, np.float32) for s in sigs]))
    offsets = to_dev(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32))
    lengths = to_dev(np.asarray(lens, np.int32))
    hl = (C.c_int * n_utt)(*lens)
    f_out = lib.asr_frontend_num_feats(C.byref(cfg)) * (2 * cfg.num_context + 1)
    max_frames = max(lib.asr_frontend_num_frames(n, cfg.frame_len, cfg.frame_step) for n in lens)
    nbytes = lib.asr_frontend_workspace_bytes(C.byref(cfg), n_utt, max_frames)
    if ws is None:
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device='cuda:0')
    assert ws.numel() >= nbytes
    out = Guarded(int(t_out) * int(n_pad) * f_out)
    frames = Guarded(n_utt, dtype=torch.int32, fill=-7)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    head = (C.byref(cfg), ptr(audio), ptr(offsets), ptr(lengths), hl, n_utt, int(n_pad),
            ptr(tables['window']), ptr(tables['mel']), ptr(tables['mel_range']))
    tail = (ptr(out.t), int(t_out), ptr(frames.t), ptr(ws), nbytes,
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if cfg.kind == 0:
        rc = lib.asr_frontend_mfcc_batch(*(head + (ptr(tables['dct']),) + tail))
    else:
        rc = lib.asr_frontend_logfbank_batch(*(head + tail))
    torch.cuda.synchronize()
    try:
        L.check(rc, 'asr_frontend_*_batch')
    except L.AsrHipError as e:
        e.guarded = (out, frames)
        raise
    return out, frames, ws


def _slab(feat, sigs, n_pad, t_out, ws=None):
    """-> ((t_out, n_pad, f_out) slab, frames (n_utt,)) after the checks every call must pass: both
    guards intact, no sentinel left in the slab or in the frame counts."""
    from tests.test_gpu_flat import SENT
    out, frames, _ = _launch(feat, sigs, n_pad, t_out, ws)
    got = out.numpy().reshape(int(t_out), int(n_pad), -1)
    fr = frames.numpy()
    assert not (got == SENT).any(), ('unwritten elements', np.argwhere(got == SENT)[:4])
    assert not np.isnan(got).any(), ('NaN', np.argwhere(np.isnan(got))[:4])
    return got, fr


def _ts_of(name, sigs):
    L_, S_ = FC.framing(name)
    stride = FC.CONFIGS[name].kw.get('stride', 1)
    return [FC.strided(OF.num_frames(len(s), L_, S_), stride) for s in sigs]


def _bits_equal(a, b, what):
    from tests.test_gpu_flat import _same_bits
    assert a.shape == b.shape, (what, a.shape, b.shape)
    _same_bits(a.ravel(), b.ravel(), what)


@pytest.mark.parametrize('name', FC.BATCH_CONFIGS)
def test_guarded_slab_batch_shapes(name):
    feat = _feat(name)
    context = FC.CONFIGS[name].kw.get('num_context', 0) > 0
    for n_utt, n_pad in FC.BATCH_SHAPES:
        sigs = FC.batch_signals(name, n_utt)
        ts = _ts_of(name, sigs)
        assert n_utt == 1 or int(np.argmax(ts)) != 0           # the longest is not the first
        base = None
        for dt in FC.T_OUT_DELTAS:
            t_out = max(ts) + dt
            got, fr = _slab(feat, sigs, n_pad, t_out)
            what = (name, n_utt, n_pad, t_out)
            assert fr.tolist() == [min(t, t_out) for t in ts], what
            for i, t in enumerate(ts):
                assert np.all(got[min(t, t_out):, i] == 0), what + (i,)      # pad_sequences 'post'
            assert np.all(got[:, n_utt:] == 0), what                        # batch padding rows
            if dt == 0:
                base = got
                for i, (x, t) in enumerate(zip(sigs, ts)):
                    # (standardised context below MIN_CONTEXT_T frames: FC.cases)
                    if context and OF.num_frames(len(x), *FC.framing(name)) < FC.MIN_CONTEXT_T:
                        continue
                    _check(name, what + (i,), got[:t, i], _want(name, x))
            else:
                # more or fewer time steps change nothing in the rows both slabs have
                keep = min(t_out, base.shape[0])
                _bits_equal(got[:keep], base[:keep], what)
                assert np.all(got[base.shape[0]:] == 0), what


@pytest.mark.parametrize('name', FC.SHARED_DELTA_CONFIGS)
def test_alone_equals_in_batch_and_twice_equals_once(name):
    """The configurations in which two workgroups of fe_finalize_kernel write the same delta
    column of the workspace."""
    from asr_study_amd import ops
    feat = _feat(name)
    sigs = FC.batch_signals(name, 17)
    ts = _ts_of(name, sigs)
    t_out = max(ts)
    out, frames, ws = _launch(feat, sigs, 32, t_out)
    first = out.numpy().reshape(t_out, 32, -1)
    again, fr = _slab(feat, sigs, 32, t_out, ws=ws)          # the workspace the first call left
    _bits_equal(again, first, (name, 'twice'))
    assert fr.tolist() == ts
    for i, x in enumerate(sigs):
        alone, fr1 = _slab(feat, [x], 1, t_out)
        assert fr1.tolist() == [ts[i]]
        _bits_equal(alone[:, 0], first[:, i], (name, 'alone', i))
    # short utterances right after a long one, through the product path: the workspace entry is
    # reused, its rows stale; a dropped entry is the state of a fresh process
    L_, S_ = FC.framing(name)
    long = FC.make_signal('noise', FC.full_len(257, L_, S_), 4242, L_, S_)
    short = [FC.make_signal('noise', FC.full_len(T, L_, S_) + k, 4300 + T, L_, S_)
             for T, k in ((5, 0), (1, 0), (3, 1), (2, 0), (4, 1))]

    def run_short():
        slab, frames = feat.batch(short)
        torch.cuda.synchronize()
        return slab.cpu().numpy(), frames.cpu().numpy()

    feat.batch([long, long])
    key = [k for k in ops.WS.bufs if k[0] == 'frontend']
    assert len(key) == 1
    size_after_long = ops.WS.bufs[key[0]].numel()
    stale, fr_stale = run_short()
    assert ops.WS.bufs[key[0]].numel() == size_after_long       # reused, not regrown
    del ops.WS.bufs[key[0]]
    fresh, fr_fresh = run_short()
    assert ops.WS.bufs[key[0]].numel() < size_after_long
    _bits_equal(stale, fresh, (name, 'short after long'))
    assert fr_stale.tolist() == fr_fresh.tolist() == _ts_of(name, short)


REJECTED = {
    'nfft_256': ('MFCC', {'nfft': 256}),
    'win_len_640': ('MFCC', {'win_len': 0.04}),                  # frame_len 640 > NFFT
    'num_filt_129': ('LogFbank', {'num_filt': 129}),
    'num_cep_65': ('MFCC', {'num_filt': 80, 'num_cep': 65}),
}


def _untouched(guarded):
    from tests.test_gpu_flat import SENT
    out, frames = guarded
    assert np.all(out.numpy() == SENT) and np.all(frames.numpy() == -7)


@pytest.mark.parametrize('case', sorted(REJECTED))
def test_rejected_arguments_write_nothing(case):
    from asr_study_amd import _lib as L
    from asr_study_amd.preprocessing import audio
    cls, kw = REJECTED[case]
    feat = getattr(audio, cls)(**kw)
    x = FC.make_signal('noise', 3000, 9, 400, 160)
    with pytest.raises(L.AsrHipError) as info:
        _launch(feat, [x, x[:700]], 16, 20)
    _untouched(info.value.guarded)
    with pytest.raises(L.AsrHipError):
        feat(x)


def test_one_sample_utterance_is_rejected():
    from asr_study_amd import _lib as L
    feat = _feat('mfcc39')
    x = FC.make_signal('noise', 3000, 9, 400, 160)
    with pytest.raises(L.AsrHipError) as info:
        _launch(feat, [x, x[:1], x[:700]], 16, 20)
    _untouched(info.value.guarded)
    with pytest.raises(L.AsrHipError):
        feat.batch([x, x[:1], x[:700]])
    with pytest.raises(TypeError):
        feat(x[:1])
    got, fr = _slab(feat, [x, x[:2], x[:700]], 16, 20)           # two samples are enough
    assert fr.tolist() == [18, 1, 3]
