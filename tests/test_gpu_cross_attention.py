"""-m gpu: the cross-attention entry points (csrc/cross_attention.hip: the passes of csrc/attn_core.h
with CROSS = true) against the float64 oracle (tests/aed_oracle.py), against asr_attn_fwd /
asr_attn_bwd bit for bit, and their zeros, padding independence, repeats and refusals."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import aed_oracle as AO

pytestmark = pytest.mark.gpu

BOUND = 1e-5          # tests/test_gpu_attention.py::_check's: max error <= 1e-5 max |want|
PAD_Q, PAD_KV, PAD_O = 4, 8, 4      # ld_* wider than the data


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def _ints(a):
    return None if a is None else torch.tensor(np.asarray(a, np.int32), device='cuda:0')


def _make(rs, Tq, Tk, N, n_pad, heads, dh, q_lens, k_lens):
    """Data at scale 1 in the valid rows and columns; junk at 3x the scale everywhere else: the
    pad samples, the pad columns, the query rows at or past q_lens (q AND dout) and the keys at or
    past k_lens."""
    D = heads * dh
    q = (rs.randn(Tq, n_pad, D + PAD_Q) * 3.0).astype(np.float32)
    kv = (rs.randn(Tk, n_pad, 2 * D + PAD_KV) * 3.0).astype(np.float32)
    dout = (rs.randn(Tq, n_pad, D + PAD_O) * 3.0).astype(np.float32)
    ql, kl = AO.clamp_lens(q_lens, k_lens, N, Tq, Tk)
    for n in range(N):
        q[:ql[n], n, :D] = rs.randn(ql[n], D)
        dout[:ql[n], n, :D] = rs.randn(ql[n], D)
        kv[:kl[n], n, :2 * D] = rs.randn(kl[n], 2 * D)
    return q, kv, dout


def _run(q, kv, dout, N, heads, dh, q_lens, k_lens, backward=True):
    """Host float32 slabs -> out, lse, dq, dkv (host).  Outputs start from the sentinel 7.0: what
    is not written shows."""
    from asr_study_amd import ops
    Tq, n_pad, _ = q.shape
    qd, kd, dd = _dev(q), _dev(kv), _dev(dout)
    ql, kl = _ints(q_lens), _ints(k_lens)
    out = torch.full_like(dd, 7.0)
    lse = torch.full((ops.attn_lse_len(Tq, n_pad, heads),), 7.0, device='cuda:0')
    ops.attn_cross_fwd(qd, kd, out, N, heads, dh, q_lens=ql, k_lens=kl, lse=lse)
    dq, dkv = torch.full_like(qd, 7.0), torch.full_like(kd, 7.0)
    if backward:
        ops.attn_cross_bwd(qd, kd, out, lse, dd, dq, dkv, N, heads, dh, q_lens=ql, k_lens=kl)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (out, lse.view(Tq, n_pad, heads), dq, dkv)]


def _rel(got, want, size=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / (size or max(np.abs(want).max(), 1e-30)))


def _check(tag, q, kv, dout, N, heads, dh, q_lens, k_lens):
    Tq, Tk, D = q.shape[0], kv.shape[0], heads * dh
    out, lse, dq, dkv = _run(q, kv, dout, N, heads, dh, q_lens, k_lens)
    wo, c = AO.cross_forward(q[:, :N, :D], kv[:, :N, :2 * D], heads, q_lens, k_lens)
    wdq, wdkv = AO.cross_backward(dout[:, :N, :D], c)
    ql, kl = c['ql'], c['kl']
    sizes = dict(out=None, lse=None, dq=None, dkv=None)
    if (kl == 1).all():
        # every utterance has ONE key: p = 1 and dS = p (dO . v - D) is exactly 0 in the oracle, so
        # dQ is measured against the size of the terms that cancel, scale |dO . v| max |k|
        # (test_gpu_attention.py::test_single_frame_returns_v_exactly states the same)
        assert not wdq.any()
        terms = np.abs(dout[:, :N, :D].astype(np.float64) * kv[0, :N, D:2 * D])
        terms = terms.reshape(Tq, N, heads, dh).sum(axis=-1)
        terms = max(terms[:ql[n], n].max(initial=0.0) for n in range(N))      # valid rows only
        sizes['dq'] = float(terms * np.abs(kv[0, :N, :D]).max() / np.sqrt(dh))
    errs = {}
    for name, got, want in (('out', out[:, :N, :D], wo), ('lse', lse[:, :N], c['lse']),
                            ('dq', dq[:, :N, :D], wdq), ('dkv', dkv[:, :N, :2 * D], wdkv)):
        errs[name] = _rel(got, want, sizes[name])
    print('[cross] %s: %s (bound %.1e)'
          % (tag, ' '.join('%s %.2e' % kv_ for kv_ in sorted(errs.items())), BOUND))
    for a in (out, lse, dq, dkv):
        assert np.isfinite(a).all(), tag
    for name, e in errs.items():
        assert e <= BOUND, (tag, name, e)
    # exact zeros: pad samples, pad columns, masked query rows, masked keys
    assert not out[:, N:].any() and not out[:, :, D:].any(), tag
    assert not lse[:, N:].any(), tag
    assert not dq[:, N:].any() and not dq[:, :, D:].any(), tag
    assert not dkv[:, N:].any() and not dkv[:, :, 2 * D:].any(), tag
    for n in range(N):
        assert not out[ql[n]:, n].any() and not lse[ql[n]:, n].any(), (tag, n)
        assert not dq[ql[n]:, n].any() and not dkv[kl[n]:, n].any(), (tag, n)
    return out, lse, dq, dkv


def _lens(rs, T, N, lo, first_small):
    """Ragged lengths in lo .. T: utterance 0 full, then the smallest values, then random."""
    v = [T] + list(first_small)[:max(N - 1, 0)]
    v += list(rs.randint(lo, T + 1, size=max(N - len(v), 0)))
    return np.asarray(v[:N], np.int32)


TQ, TK = (1, 63, 64, 65, 130), (1, 64, 65, 200)
COMBOS = list(itertools.product((16, 64, 128), (1, 3), (1, 3, 17)))     # dh, heads, N
# every (Tq, Tk) pair; (dh, heads, N) walk through all 18 combinations beside them
CASES = [(tq, tk) + COMBOS[i % len(COMBOS)]
         for i, (tq, tk) in enumerate(itertools.product(TQ, TK))]


def test_cases_cover_the_edges():
    assert {c[2:] for c in CASES} == set(COMBOS)
    assert {c[:2] for c in CASES} == set(itertools.product(TQ, TK))


@pytest.mark.parametrize('Tq,Tk,dh,heads,N', CASES)
def test_parity(Tq, Tk, dh, heads, N):
    """Ragged lengths: q_len = 1 and k_len = 1 in every batch of 3 or more, q_len = 0 for one
    utterance; a single utterance is one short of full on both sides."""
    rs = np.random.RandomState(1000 * Tq + Tk)
    n_pad = (N + 15) // 16 * 16
    if N == 1:
        q_lens, k_lens = np.asarray([max(Tq - 1, 1)]), np.asarray([max(Tk - 3, 1)])
    else:
        q_lens = _lens(rs, Tq, N, 0, [1, 0])
        k_lens = _lens(rs, Tk, N, 1, [min(Tk, 64), 1])
    q, kv, dout = _make(rs, Tq, Tk, N, n_pad, heads, dh, q_lens, k_lens)
    _check('Tq=%d Tk=%d dh=%d heads=%d N=%d' % (Tq, Tk, dh, heads, N), q, kv, dout, N, heads, dh,
           q_lens, k_lens)


def test_null_lens_are_full_lengths():
    rs = np.random.RandomState(3)
    Tq, Tk, N, heads, dh = 65, 70, 3, 2, 32
    q, kv, dout = _make(rs, Tq, Tk, N, 16, heads, dh, None, None)
    a = _check('null', q, kv, dout, N, heads, dh, None, None)
    b = _run(q, kv, dout, N, heads, dh, np.full(N, Tq), np.full(N, Tk))
    c = _run(q, kv, dout, N, heads, dh, np.full(N, Tq + 9), np.full(N, Tk + 9))     # clamped
    for u, v, w in zip(a, b, c):
        assert np.array_equal(u, v) and np.array_equal(u, w)


@pytest.mark.parametrize('T,N,heads,dh,ragged', [(130, 3, 3, 16, True), (65, 17, 1, 64, True),
                                                 (64, 2, 1, 128, False), (1, 3, 2, 32, False)])
def test_same_bits_as_self_attention(T, N, heads, dh, ragged):
    """q, k, v the three column blocks of one qkv slab, Tq = Tk, q_lens = NULL: out / lse are
    asr_attn_fwd's and dq, dkv the blocks of asr_attn_bwd's dqkv, bit for bit."""
    from asr_study_amd import ops
    rs = np.random.RandomState(T + dh)
    D, n_pad = heads * dh, (N + 15) // 16 * 16
    lens = _lens(rs, T, N, 1, [1, min(T, 64)]) if ragged else None
    qkv = rs.randn(T, n_pad, 3 * D + 4).astype(np.float32)
    dout = rs.randn(T, n_pad, D).astype(np.float32)
    x, do, ld = _dev(qkv), _dev(dout), _ints(lens)
    out = torch.full_like(do, 7.0)
    lse = torch.full((ops.attn_lse_len(T, n_pad, heads),), 7.0, device='cuda:0')
    dqkv = torch.full_like(x, 7.0)
    ops.attn_fwd(x, out, N, heads, dh, lens=ld, lse=lse)
    ops.attn_bwd(x, out, lse, do, dqkv, N, heads, dh, lens=ld)
    torch.cuda.synchronize()
    want = [t.cpu().numpy() for t in (out, lse.view(T, n_pad, heads), dqkv)]
    got = _run(qkv[..., :D], qkv[..., D:3 * D], dout, N, heads, dh, None, lens)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1][:, :N], want[1][:, :N])     # (K21 writes lse for real samples only)
    assert np.array_equal(got[2], want[2][..., :D])
    assert np.array_equal(got[3], want[2][..., D:3 * D])


def test_padding_independence_and_repeats():
    """An utterance's rows are the same bits with Tq and Tk padded further, alone and in a batch,
    and on a second run."""
    rs = np.random.RandomState(9)
    Tq, Tk, N, heads, dh = 65, 70, 3, 2, 32
    D = heads * dh
    q_lens, k_lens = np.asarray([65, 20, 64]), np.asarray([70, 65, 9])
    q, kv, dout = _make(rs, Tq, Tk, N, 16, heads, dh, q_lens, k_lens)
    base = _check('base', q, kv, dout, N, heads, dh, q_lens, k_lens)
    again = _run(q, kv, dout, N, heads, dh, q_lens, k_lens)
    for u, v in zip(base, again):
        assert np.array_equal(u, v)
    # more padding on both time axes (junk rows), a wider batch
    q2, kv2, dout2 = _make(rs, 130, 200, N, 32, heads, dh, [0] * N, [1] * N)
    q2[:Tq, :16], kv2[:Tk, :16], dout2[:Tq, :16] = q, kv, dout
    wide = _run(q2, kv2, dout2, N, heads, dh, q_lens, k_lens)
    for u, v, rows in zip(base, wide, (Tq, Tq, Tq, Tk)):
        assert np.array_equal(u[:, :N], v[:rows, :N])
        assert not v[rows:].any()
    # utterance 1 alone
    one = _run(q[:, 1:17].copy(), kv[:, 1:17].copy(), dout[:, 1:17].copy(), 1, heads, dh,
               q_lens[1:2], k_lens[1:2])
    for u, v in zip(base, one):
        assert np.array_equal(u[:, 1], v[:, 0])
    assert D == 64


def test_decode_step_is_a_row_of_the_training_call():
    """Tq = 1 with the query of row t gives row t of the whole call, bit for bit."""
    rs = np.random.RandomState(12)
    Tq, Tk, N, heads, dh = 5, 70, 3, 4, 16
    k_lens = np.asarray([70, 33, 1])
    q, kv, dout = _make(rs, Tq, Tk, N, 16, heads, dh, None, k_lens)
    whole = _run(q, kv, dout, N, heads, dh, None, k_lens, backward=False)
    for t in (0, 4):
        row = _run(q[t:t + 1], kv, dout[t:t + 1], N, heads, dh, None, k_lens, backward=False)
        assert np.array_equal(row[0][0], whole[0][t]) and np.array_equal(row[1][0], whole[1][t])


def _args(ops, L, q, kv, out, lse, dout, dq, dkv, N, heads, dh):
    a = ops._attn_cross_args(q, kv, out, N, heads, dh, None, lse=lse, dout=dout, dq=dq, dkv=dkv)
    return a


@pytest.mark.parametrize('field,value', [
    ('dh', 24), ('dh', 144), ('dh', 0), ('Tq', 0), ('Tk', 0), ('N', 0), ('N', 17), ('heads', 0),
    ('ld_q', 28), ('ld_q', 34), ('ld_kv', 60), ('ld_kv', 66), ('ld_out', 28), ('ld_out', 34),
    ('scale', 0.0), ('n_pad', 65536)])
def test_refusals_launch_nothing(field, value):
    """Bad geometry: ASR_ERR_INVALID from the size function (0), the forward and the backward
    call, and no output is touched."""
    from asr_study_amd import _lib as L
    from asr_study_amd import ops
    heads, dh, N = 2, 16, 3
    q = torch.zeros((4, 16, 32), device='cuda:0')
    kv = torch.zeros((6, 16, 64), device='cuda:0')
    out, dout = torch.full_like(q, 7.0), torch.zeros_like(q)
    lse = torch.full((4 * 16 * heads,), 7.0, device='cuda:0')
    dq, dkv = torch.full_like(q, 7.0), torch.full_like(kv, 7.0)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda:0')
    a = _args(ops, L, q, kv, out, lse, dout, dq, dkv, N, heads, dh)
    lib = L.load()
    assert lib.asr_attn_cross_workspace_bytes(ctypes.byref(a)) > 0
    setattr(a, field, value)
    invalid = L.CONSTANTS['ASR_ERR_INVALID']
    assert lib.asr_attn_cross_workspace_bytes(ctypes.byref(a)) == 0
    assert lib.asr_attn_cross_fwd(ctypes.byref(a), None) == invalid
    assert b'attn_cross_fwd' in lib.asr_last_error()
    assert lib.asr_attn_cross_bwd(ctypes.byref(a), ws.data_ptr(), ws.numel(), None) == invalid
    torch.cuda.synchronize()
    for t in (out, lse, dq, dkv):
        assert bool((t == 7.0).all())
    assert lib.asr_attn_cross_fwd(None, None) == invalid


def test_missing_pointers_and_workspace_are_refused():
    from asr_study_amd import _lib as L
    from asr_study_amd import ops
    heads, dh, N = 2, 16, 3
    q = torch.zeros((4, 16, 32), device='cuda:0')
    kv = torch.zeros((6, 16, 64), device='cuda:0')
    out, dout = torch.full_like(q, 7.0), torch.zeros_like(q)
    lse = torch.zeros((4 * 16 * heads,), device='cuda:0')
    dq, dkv = torch.full_like(q, 7.0), torch.full_like(kv, 7.0)
    lib = L.load()
    a = _args(ops, L, q, kv, out, lse, dout, dq, dkv, N, heads, dh)
    a.kv = None
    assert lib.asr_attn_cross_fwd(ctypes.byref(a), None) == L.CONSTANTS['ASR_ERR_INVALID']
    a = _args(ops, L, q, kv, out, lse, dout, dq, dkv, N, heads, dh)
    assert lib.asr_attn_cross_bwd(ctypes.byref(a), None, 0, None) == \
        L.CONSTANTS['ASR_ERR_WORKSPACE']
    a.dkv = None
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda:0')
    assert lib.asr_attn_cross_bwd(ctypes.byref(a), ws.data_ptr(), ws.numel(), None) == \
        L.CONSTANTS['ASR_ERR_INVALID']
    torch.cuda.synchronize()
    for t in (out, dq, dkv):
        assert bool((t == 7.0).all())
