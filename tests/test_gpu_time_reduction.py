"""-m gpu: asr_time_stack_fwd / _bwd (K33, csrc/timestack.hip) against tests/time_reduction_oracle.py.

A copy has no tolerance: every comparison is bit for bit.  Poisoning: every output is pre-filled
with NaN (and lies between two guard bands that must come back untouched), and so are the columns
of the input that the kernels may not read (>= F of x, >= k F of dy).  The result must hold no NaN
and equal the oracle everywhere, pad columns and the rows n >= N included.

The case table.  GEOS restates the issue's F / ld_in / ld_out triples -- (8, 8, 16), (8, 12, 20),
(5, 8, 12), (39, 40, 80), which are for k = 2 -- as (F, ld_in, extra): ld_out = pad4(k F) + extra,
so that every k of TK has a legal ld_out and k = 2 gives exactly those four.  F = 8: the 16-byte
path; F = 5, 39: the scalar path, a column group that straddles two source frames.

The grid edges.  The launch (timestack.hip, ts_blocks): one item per four OUTPUT columns, 256
threads, at most 4096 workgroups, a grid-stride loop: CAP = 4096 * 256 items per trip.  Forward
items = ceil(T / k) n_pad ld_out / 4, backward items = T n_pad ld_in / 4.  The narrowest rows, k =
2, F = ld_in = 4, ld_out = 8, n_pad = 16, give 16 items per frame either way, so T = CAP / 16 fills
one grid exactly in BOTH directions, and T = CAP / 16 + 99 wraps both into a ragged second trip
(odd: the last group is partial)."""
import numpy as np
import pytest
import torch

from tests import time_reduction_oracle as TR
from tests.gpu_util import to_dev
from tests.test_gpu_flat import Guarded, _same_bits

pytestmark = pytest.mark.gpu

TK = [(1, 2), (2, 2), (3, 2), (7, 3), (9, 4), (17, 8), (16, 8)]
GEOS = [(8, 8, 0), (8, 12, 4), (5, 8, 0), (39, 40, 0)]
BATCH = [(1, 16), (3, 16), (16, 16), (17, 32)]
CAP = 4096 * 256
EDGE_K, EDGE_F, EDGE_NPAD = 2, 4, 16
EDGE_T = [CAP // 16, CAP // 16 + 99]
NAN = float('nan')


def _pad4(n):
    return (n + 3) // 4 * 4


def test_case_table_is_what_the_issue_states():
    assert [(F, ld, _pad4(2 * F) + e) for F, ld, e in GEOS] == \
        [(8, 8, 16), (8, 12, 20), (5, 8, 12), (39, 40, 80)]
    for T in EDGE_T:
        fwd = TR.out_frames(T, EDGE_K) * EDGE_NPAD * (EDGE_K * EDGE_F // 4)
        bwd = T * EDGE_NPAD * (EDGE_F // 4)
        assert (fwd == CAP and bwd == CAP) if T == EDGE_T[0] else \
            (CAP < fwd < 2 * CAP and CAP < bwd < 2 * CAP and fwd % 256 and bwd % 256)


def ragged(T, k, N):
    """Lengths that hold, as far as N goes: the largest len <= T with len % k == 1, 0, T, 1, T - 1,
    two values the kernels clamp (T + 3, -2), then a fixed walk over 0 .. T."""
    lk1 = ((T - 1) // k) * k + 1
    pool = [lk1, 0, T, 1, max(T - 1, 0), T + 3, -2] + [(5 * i + 2) % (T + 1) for i in range(N)]
    return np.array(pool[:N], np.int32)


def _lens_modes(T, k, N):
    return [('none', None), ('full', np.full(N, T, np.int32)), ('ragged', ragged(T, k, N))]


def _run(x, lens, N, F, ld_out, k, dy):
    """-> y, dx, dx of y (all NumPy), each checked for guard bands and a repeated call."""
    from asr_study_amd import ops
    T, n_pad, ld_in = x.shape
    To = TR.out_frames(T, k)
    xd, dyd = to_dev(x), to_dev(dy)
    ld = None if lens is None else to_dev(lens)
    out = []
    for shape, call in (((To, n_pad, ld_out), lambda o: ops.time_stack_fwd(xd, o, N, F, k, lens=ld)),
                        ((T, n_pad, ld_in), lambda o: ops.time_stack_bwd(dyd, o, N, F, k, lens=ld))):
        bits = []
        for _ in range(2):
            g = Guarded(int(np.prod(shape)), fill=NAN)
            # (NaN != NaN: the guard check of Guarded compares with ==, so check bands by bits)
            call(g.t.view(*shape))
            torch.cuda.synchronize()
            h = g.buf.cpu().numpy()
            assert np.isnan(h[:g.lo]).all() and np.isnan(h[g.lo + g.n:]).all(), 'guard band'
            bits.append(h[g.lo:g.lo + g.n].reshape(shape).copy())
        assert np.array_equal(bits[0].view(np.uint32), bits[1].view(np.uint32)), 'repeat differs'
        out.append(bits[0])
    y, dx = out
    # bwd(fwd(x)): y's own pad columns are zeros, which bwd never reads
    g = torch.full((T, n_pad, ld_in), NAN, dtype=torch.float32, device='cuda:0')
    ops.time_stack_bwd(to_dev(y), g, N, F, k, lens=ld)
    return y, dx, g.cpu().numpy()


def _check(x, lens, N, F, ld_out, k, dy, what):
    T, n_pad, ld_in = x.shape
    y, dx, back = _run(x, lens, N, F, ld_out, k, dy)
    want_y = TR.stack_slab(x, lens, N, F, ld_out, k)
    want_dx = TR.unstack_slab(dy, lens, N, T, F, ld_in, k)
    for got, want, name in ((y, want_y, 'y'), (dx, want_dx, 'dx')):
        assert not np.isnan(got).any(), (what, name)
        _same_bits(got.ravel(), want.ravel(), '%s %s' % (what, name))
    # frames >= len and pad columns of dx: exactly zero
    valid = TR._valid(T, n_pad, TR._row_lens(lens, N, n_pad, T))
    assert not dx[~valid].any() and not dx[:, :, F:].any(), what
    assert not y[:, :, k * F:].any(), what
    # bwd(fwd(x)) = x with its invalid frames and pad columns zeroed
    proj = np.zeros_like(x)
    proj[:, :, :F] = np.where(valid[:, :, None], x[:, :, :F], 0)
    _same_bits(back.ravel(), proj.ravel(), what + ' bwd(fwd(x))')


def _data(rs, T, n_pad, F, ld_in, ld_out, k):
    x = rs.randn(T, n_pad, ld_in).astype(np.float32)
    x[:, :, F:] = NAN                                   # never read
    dy = rs.randn(TR.out_frames(T, k), n_pad, ld_out).astype(np.float32)
    dy[:, :, k * F:] = NAN
    return x, dy


@pytest.mark.parametrize('F,ld_in,extra', GEOS)
@pytest.mark.parametrize('T,k', TK)
def test_bit_equal_to_the_oracle(T, k, F, ld_in, extra):
    ld_out = _pad4(k * F) + extra
    rs = np.random.RandomState(1000 * T + 10 * k + F)
    for N, n_pad in BATCH:
        x, dy = _data(rs, T, n_pad, F, ld_in, ld_out, k)
        for name, lens in _lens_modes(T, k, N):
            _check(x, lens, N, F, ld_out, k, dy, 'T%d k%d F%d N%d/%d %s' % (T, k, F, N, n_pad, name))


@pytest.mark.parametrize('T', EDGE_T, ids=['one_grid', 'ragged_second_trip'])
def test_grid_edges(T):
    rs = np.random.RandomState(T % 1000)
    k, F, n_pad = EDGE_K, EDGE_F, EDGE_NPAD
    x, dy = _data(rs, T, n_pad, F, F, k * F, k)
    N = 5
    lens = np.array([T, T - 1, (T // 2) | 1, 1, 0], np.int32)
    _check(x, lens, N, F, k * F, k, dy, 'edge T%d' % T)


def test_padding_independence():
    """The same utterances in a slab of T frames and in one of T + 5 frames with noise behind each
    length: identical rows on every valid output frame (and exact zeros behind them)."""
    from asr_study_amd import ops
    rs = np.random.RandomState(7)
    for (F, ld_in, extra), k in ((GEOS[1], 3), (GEOS[2], 2), (GEOS[3], 4)):
        T, N, n_pad = 11, 4, 16
        ld_out = _pad4(k * F) + extra
        lens = np.array([11, 7, 1, 4], np.int32)
        short = rs.randn(T, n_pad, ld_in).astype(np.float32)
        long = (100.0 * rs.randn(T + 5, n_pad, ld_in)).astype(np.float32)     # noise everywhere ...
        for n in range(N):
            long[:lens[n], n] = short[:lens[n], n]          # ... but on the valid frames
        outs = []
        for x in (short, long):
            y = torch.full((TR.out_frames(x.shape[0], k), n_pad, ld_out), NAN, device='cuda:0')
            ops.time_stack_fwd(to_dev(x), y, N, F, k, lens=to_dev(lens))
            outs.append(y.cpu().numpy())
        lo = TR.out_lengths(lens, k)
        for n in range(N):
            assert np.array_equal(outs[0][:lo[n], n].view(np.uint32),
                                  outs[1][:lo[n], n].view(np.uint32)), (F, k, n)
            assert not outs[0][lo[n]:, n].any() and not outs[1][lo[n]:, n].any()
