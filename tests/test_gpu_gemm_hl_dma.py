"""-m gpu: the DMA-staged persistent packed GEMM (gemm_hlp_kernel<.., DMA>, ASR_GEMM_DMA) against
the register-staged forms (ASR_GEMM_DMA=0).  Same planes, same products in the same order per
accumulator, same epilogue: every output bit equal, no tolerance.

ASR_GEMM_DMA=2 sends EVERY plain row-major launch of the 256 x 256 tile with K >= 4 slabs to the
DMA form, however few tiles it has, so the shapes here are the smallest at which the form can go
wrong; =1 is the dispatch of a real step (at least two tiles per compute unit)."""
import numpy as np
import pytest
import torch

from tests.gpu_util import to_dev

pytestmark = pytest.mark.gpu

SHAPES = [
    (256, 256, 128),      # one interior tile, the shortest K loop (4 slabs)
    (512, 256, 160),      # two tiles per column: the load cursor crosses a tile boundary mid-prefetch
    (300, 272, 136),      # row and column edge tiles, K tail of 8: out-of-range lanes deliver zeros
    (1024, 512, 256),     # more tiles than one XCD's first hand-out
]
OPTS = ['bias', 'mask', 'view', 'offs']


def _case(M, N, K, opts):
    """Planes and keyword arguments of one launch.  'offs': A and B are sub-ranges of wider planes,
    as bilstm._dx (a_k / b_k: one direction's gate columns of dz and W^T) and _gate_gemm_hl (b_row:
    one direction's rows of W) pass them -- the reduction tail then lies INSIDE the planes, over
    the other direction's data, and only the kernel's own range test keeps it out."""
    from asr_study_amd import ops
    rs = np.random.RandomState(M + N + K + len(opts))
    a_k = b_k = 48 if opts == 'offs' else 0
    b_row = 16 if opts == 'offs' else 0
    Kf, Nf = K + a_k + (40 if opts == 'offs' else 0), N + b_row
    A = rs.randn(M, Kf).astype(np.float32)
    B = (rs.randn(Kf, Nf) * 0.05).astype(np.float32)
    pa = ops.HlPlanes(M, Kf, 'cuda:0')
    pb = ops.HlPlanes(Nf, Kf, 'cuda:0')
    Ad, Bd = to_dev(A), to_dev(B)
    ops.pack_hl(Ad, M, Kf, absmax=ops.absmax(Ad), r=pa)
    ops.pack_hl(Bd, Kf, Nf, absmax=ops.absmax(Bd), c=pb)
    ldc = N + 64 if opts == 'view' else N
    C0 = rs.randn(M, ldc).astype(np.float32)
    kw = {}
    if opts == 'bias':
        kw = dict(bias=to_dev(rs.randn(N).astype(np.float32)))
    elif opts == 'mask':
        cm = to_dev(((rs.rand(16, N) > 0.3) / 0.7).astype(np.float32))
        kw = dict(beta=1.0, c_scale=cm, c_scale_period=16)
    elif opts == 'view':
        kw = dict(c_off=32, ldc=ldc)
    elif opts == 'offs':
        kw = dict(a_k=a_k, b_k=b_k, b_row=b_row)
    def want():
        return A[:, a_k:a_k + K].astype(np.float64) @ B[b_k:b_k + K, b_row:b_row + N].astype(np.float64)
    return pa, pb, C0, kw, want, np.abs(A).max() * np.abs(B).max()


def _run(monkeypatch, mode, pa, pb, C0, M, N, K, kw, stream=None):
    from asr_study_amd import ops
    monkeypatch.setenv('ASR_GEMM_DMA', mode)
    Cd = to_dev(C0)
    if stream is None:
        ops.gemm_hl(pa, pb, Cd, M, N, K, **kw)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ops.gemm_hl(pa, pb, Cd, M, N, K, **kw)
    return Cd


@pytest.mark.parametrize('opts', OPTS)
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_dma_form_is_bit_identical(M, N, K, opts, monkeypatch):
    pa, pb, C0, kw, want, scale = _case(M, N, K, opts)
    off = _run(monkeypatch, '0', pa, pb, C0, M, N, K, kw)
    torch.cuda.synchronize()
    outs = [_run(monkeypatch, '2', pa, pb, C0, M, N, K, kw) for _ in range(3)]   # re-armed block
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o, off)
    if opts in ('bias', 'offs'):          # and the register-staged side is a GEMM at all
        got = off.cpu().numpy() - (kw['bias'].cpu().numpy() if opts == 'bias' else 0.0)
        assert np.abs(got - want()).max() < 2e-6 * scale * K + 2e-5


def test_dma_form_on_two_streams_at_once(monkeypatch):
    M, N, K = 1024, 512, 256
    pa, pb, C0, kw, _, _ = _case(M, N, K, 'bias')
    off = _run(monkeypatch, '0', pa, pb, C0, M, N, K, kw)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [_run(monkeypatch, '2', pa, pb, C0, M, N, K, kw, stream=s1 if i % 2 == 0 else s2)
            for i in range(6)]
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o, off)


def test_dma_form_in_the_dispatch_of_a_step(monkeypatch):
    """ASR_GEMM_DMA=1: the form runs where the persistent form runs -- two tiles per compute unit
    and more; every workgroup walks several tiles, the hand-out runs dry on all XCDs."""
    M, N, K = 8192, 4352, 160
    pa, pb, C0, kw, _, _ = _case(M, N, K, 'bias')
    off = _run(monkeypatch, '0', pa, pb, C0, M, N, K, kw)
    torch.cuda.synchronize()
    on = _run(monkeypatch, '1', pa, pb, C0, M, N, K, kw)
    torch.cuda.synchronize()
    assert torch.equal(on, off)


def test_training_step_is_bit_identical_with_the_dma_form(monkeypatch):
    """One forward + CTC + backward of 2 x BiLSTM(512) with dropout 0.2 (T = 24, batch 16: packed
    stages; the second layer's x@W and both layers' dX reach the 256 x 256 tile): logits and
    every gradient bit-equal with the form on and off.  The masks are a function of (seed, stage,
    step), so both runs draw the same ones."""
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
    for mode in ('0', '2'):
        monkeypatch.setenv('ASR_GEMM_DMA', mode)
        _, logits, _ = model.loss_and_grads(slab, labels, lens, training=True)
        torch.cuda.synchronize()
        res[mode] = (logits.clone(), model.grads.clone())
    assert torch.isfinite(res['0'][1]).all() and res['0'][1].abs().max() > 0
    assert torch.equal(res['2'][0], res['0'][0])
    assert torch.equal(res['2'][1], res['0'][1])
