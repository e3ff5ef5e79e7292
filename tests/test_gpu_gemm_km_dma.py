"""-m gpu: the DMA-staged K-major packed GEMM (gemm_hlt_dma_kernel, ASR_GEMM_KM_DMA=1) against the
register-staged K-major kernel (ASR_GEMM_KM_DMA=0).  Same planes, same products in the same order
per accumulator, same epilogue, partials and reduce: every output bit equal, no tolerance -- and
against a float64 product at the tolerance tests/test_gpu_gemm.py uses for this GEMM.

The switch is read per call and the form runs wherever the 256 x 256 K-major tile runs with at
least MIN_SLABS slabs per split, so the shapes are the smallest at which it can go wrong."""
import numpy as np
import pytest
import torch

from tests.gpu_util import to_dev

pytestmark = pytest.mark.gpu

MIN_SLABS = 2             # kKmDmaMinSlabs (csrc/gemm_hl.hip): the prologue stages two whole slabs
BIG = 64.0                # what lies beside and behind the operands: an over-read changes bits


def _planes(A, B):
    from asr_study_amd import ops
    pa = ops.HlPlanes(A.shape[0], A.shape[1], 'cuda:0')
    pb = ops.HlPlanes(B.shape[0], B.shape[1], 'cuda:0')
    Ad, Bd = to_dev(A), to_dev(B)
    ops.pack_hl(Ad, A.shape[0], A.shape[1], absmax=ops.absmax(Ad), r=pa)
    ops.pack_hl(Bd, B.shape[0], B.shape[1], absmax=ops.absmax(Bd), r=pb)
    return pa, pb


def _run(monkeypatch, mode, pa, pb, C0, M, N, K, kw, stream=None):
    from asr_study_amd import ops
    monkeypatch.setenv('ASR_GEMM_KM_DMA', mode)
    Cd = to_dev(C0)
    if stream is None:
        ops.gemm_hl(pa, pb, Cd, M, N, K, k_major=True, **kw)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ops.gemm_hl(pa, pb, Cd, M, N, K, k_major=True, **kw)
    return Cd


def _both(monkeypatch, pa, pb, C0, M, N, K, kw, want, scale):
    off = _run(monkeypatch, '0', pa, pb, C0, M, N, K, kw)
    torch.cuda.synchronize()
    on = [_run(monkeypatch, '1', pa, pb, C0, M, N, K, kw) for _ in range(2)]
    torch.cuda.synchronize()
    got = off.cpu().numpy()
    err = np.abs(got - want).max()
    print('k_major %dx%dx%d %s: err %.3e, bound %.3e' % (M, N, K, sorted(kw), err, 2e-6 * scale * K + 2e-5))
    for o in on:
        assert torch.equal(o, off)
    assert err < 2e-6 * scale * K + 2e-5


def _embedded(M, N, K, seed, r0=0, ca=0, cb=0):
    """Operands inside wider, longer planes whose other elements are large: the rows before and
    behind the reduction range and the columns beside M and N must not be read into a sum."""
    rs = np.random.RandomState(seed)
    A = np.full((r0 + K + 40, ca + M + 48), BIG, dtype=np.float32)
    B = np.full((r0 + K + 40, cb + N + 64), BIG, dtype=np.float32)
    A[r0:r0 + K, ca:ca + M] = rs.randn(K, M)
    B[r0:r0 + K, cb:cb + N] = rs.randn(K, N) * 0.05
    As, Bs = A[r0:r0 + K, ca:ca + M].astype(np.float64), B[r0:r0 + K, cb:cb + N].astype(np.float64)
    # (the tolerance is scaled by the operands themselves, not by BIG around them: a BIG times an
    # operand element read into a sum must fail the float64 check too)
    return A, B, As.T @ Bs, np.abs(As).max() * np.abs(Bs).max()


@pytest.mark.parametrize('K', [32 * MIN_SLABS, 32 * MIN_SLABS + 32, 32 * MIN_SLABS - 32])
def test_one_tile_at_and_around_the_shortest_pipeline(K, monkeypatch):
    """K = the pipeline's minimum and one slab more run the DMA form; one slab less runs the
    register-staged kernel under both settings and stays equal."""
    M = N = 256
    A, B, want, scale = _embedded(M, N, K, K)
    pa, pb = _planes(A, B)
    C0 = np.zeros((M, N), np.float32)
    _both(monkeypatch, pa, pb, C0, M, N, K, {}, want, scale)


def test_edge_tiles_and_k_tail_inside_wider_planes(monkeypatch):
    """300 x 272 x 136: edge tiles in both dimensions, a K tail of 8, lda / ldb > M / N; the
    neighbouring columns and the following rows hold BIG."""
    M, N, K = 300, 272, 136
    A, B, want, scale = _embedded(M, N, K, 1, r0=5, ca=32, cb=48)
    pa, pb = _planes(A, B)
    rs = np.random.RandomState(2)
    C0 = rs.randn(M, N).astype(np.float32)
    kw = dict(a_row=5, a_k=32, b_row=5, b_k=48, alpha=0.75, beta=0.5)
    _both(monkeypatch, pa, pb, C0, M, N, K, kw, 0.75 * want + 0.5 * C0, scale)


@pytest.mark.parametrize('sk', [3, 'auto'])
def test_split_k_with_uneven_ranges(sk, monkeypatch):
    """512 x 256 x 1000 in three ranges of 352, 352 and 296 (a tail of 8 in the last), and the
    split the step would pick."""
    M, N, K = 512, 256, 1000
    A, B, want, scale = _embedded(M, N, K, 3)
    pa, pb = _planes(A, B)
    C0 = np.zeros((M, N), np.float32)
    _both(monkeypatch, pa, pb, C0, M, N, K, dict(split_k=sk), want, scale)


@pytest.mark.parametrize('d', [0, 1])
def test_the_recurrent_weight_gradient_form(d, monkeypatch):
    """dU[d] = h_prev^T dz[d] at H = 256: y's planes and dz's shifted against each other by one
    frame (n_pad rows), B = direction d's 4H gate columns inside 8H-wide planes."""
    H, T, n_pad = 256, 9, 16
    rows, K = T * n_pad, (T - 1) * n_pad
    rs = np.random.RandomState(10 + d)
    y = rs.randn(rows, H).astype(np.float32)
    dz = (rs.randn(rows, 8 * H) * 1e-3).astype(np.float32)
    pa, pb = _planes(y, dz)
    a_row, b_row = (0, n_pad) if d == 0 else (n_pad, 0)
    kw = dict(a_row=a_row, b_row=b_row, b_k=d * 4 * H, split_k='auto')
    want = y[a_row:a_row + K].astype(np.float64).T @ \
        dz[b_row:b_row + K, d * 4 * H:(d + 1) * 4 * H].astype(np.float64)
    C0 = np.zeros((H, 4 * H), np.float32)
    _both(monkeypatch, pa, pb, C0, H, 4 * H, K, kw, want, np.abs(y).max() * np.abs(dz).max())


def test_a_batch_sharing_b(monkeypatch):
    """batch = 3 with distinct a_batch_row shifts: the convolution's per-tap weight gradient."""
    M, N, K, shifts = 256, 300, 200, [0, 32, 5]
    rs = np.random.RandomState(4)
    a = rs.randn(K + max(shifts), M).astype(np.float32)
    b = (rs.randn(K, N) * 0.05).astype(np.float32)
    pa, pb = _planes(a, b)
    want = np.concatenate([a[s:s + K].astype(np.float64).T @ b.astype(np.float64) for s in shifts])
    C0 = np.full((len(shifts) * M, N), 9.0, np.float32)
    for sk in (0, 2):
        _both(monkeypatch, pa, pb, C0, M, N, K, dict(batch_rows=shifts, split_k=sk), want,
              np.abs(a).max() * np.abs(b).max())


def test_on_two_streams_at_once(monkeypatch):
    M, N, K = 512, 512, 1000
    A, B, _, _ = _embedded(M, N, K, 5)
    pa, pb = _planes(A, B)
    C0 = np.zeros((M, N), np.float32)
    off = _run(monkeypatch, '0', pa, pb, C0, M, N, K, {})
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [_run(monkeypatch, '1', pa, pb, C0, M, N, K, {}, stream=s1 if i % 2 == 0 else s2)
            for i in range(6)]
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o, off)


def test_training_step_is_bit_identical_with_the_dma_form(monkeypatch):
    """One forward + CTC + backward of 2 x BiLSTM(512) at T = 24, batch 16 (packed stages: dW and
    dU of both layers reach the 256 x 256 K-major tile): losses and every gradient bit-equal with
    the form off and on."""
    from asr_study_amd.core import models
    rs = np.random.RandomState(3)
    N, T, F, C, H = 16, 24, 40, 29, 512
    model = models.brsmv1(num_features=F, num_classes=C, num_hiddens=H, num_layers=2, dropout=0.2,
                          weight_decay=0.0, seed=5)
    assert model.packed and all(model._stage_packed(s) for s in model.stages if s.kind == 'bilstm')
    x = rs.randn(N, T, F).astype(np.float32)
    labels = [rs.randint(0, C - 1, size=rs.randint(1, 4)).tolist() for _ in range(N)]
    lens = [T] * N
    slab = model.to_slab(x)
    res = {}
    for mode in ('0', '1'):
        monkeypatch.setenv('ASR_GEMM_KM_DMA', mode)
        ctc, logits, _ = model.loss_and_grads(slab, labels, lens, training=True)
        torch.cuda.synchronize()
        res[mode] = (ctc.clone(), logits.clone(), model.grads.clone())
    assert torch.isfinite(res['0'][2]).all() and res['0'][2].abs().max() > 0
    for a, b in zip(res['1'], res['0']):
        assert torch.equal(a, b)
