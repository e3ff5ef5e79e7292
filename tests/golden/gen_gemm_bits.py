"""Writes tests/golden/gemm_bits_parent.json: what every entry point of the GEMM family
(asr_gemm, asr_pack_hl, asr_gemm_hl in all its forms, asr_absmax, asr_colsum) wrote ON THE GPU at
the commit BEFORE csrc/gemm.hip was split by kernel family and its repeated pieces were written
once (b120917).  The JSON was written by running this file on that commit, before the source was
touched; tests/test_gpu_gemm_bits.py records every case again and compares for equality.  The
float64 tests of the family pass under a reordered sum; these do not.

A case is a function that returns {name: SHA-256 of the raw bytes of one output array}.  An
output is hashed WHOLE: the untouched part of a strided or offset C, the padding of packed planes
(pre-filled with 7.0) and the guard columns behind a column sum are part of the bytes.  Inputs
come from a seeded NumPy RandomState.  Nothing in the family accumulates with float atomics --
split-K reduces in a fixed order, absmax takes an integer max -- so the bits are repeatable: the
main program records everything twice and writes nothing unless the two agree.

The sizes are the smallest at which each variant can still go wrong (edge tiles in both
directions, K tails, an odd slab count, both tiles, every split), not the workload's; the three
persistent shapes are the smallest that reach gemm_hlp_kernel (two 256-tiles per workgroup of a
256-workgroup grid, five slabs).

Run (needs a GPU and the built library): python tests/golden/gen_gemm_bits.py [dst]"""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

DEV = 'cuda:0'


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


@contextlib.contextmanager
def _env(name, value):
    """value None: the variable unset."""
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def _sync():
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- asr_gemm
# M, N, K, trans_a, trans_b, split_k: CASES of tests/test_gpu_gemm.py (edge tiles, K = 16 / 28 /
# 39, unaligned lda, split 3 / 4; precision 1 on (257, 130, 39) runs the generic split-fp16 kernel)
GEMM_SHAPES = [
    (300, 200, 64, False, False, 0),
    (257, 130, 39, False, False, 0),
    (128, 128, 16, True, False, 0),
    (77, 28, 100, False, True, 0),
    (39, 1024, 999, True, False, 4),
    (512, 96, 700, True, True, 3),
    (1000, 260, 28, False, True, 0),
]


def _gemm_case(M, N, K, ta, tb, sk, prec):
    def run():
        from asr_study_amd import ops
        rs = np.random.RandomState(M * 3 + N + K + prec)
        A = rs.randn(K, M) if ta else rs.randn(M, K)
        B = rs.randn(N, K) if tb else rs.randn(K, N)
        if prec == 1:                               # gradient-like magnitudes, one outlier
            A *= 1e-5
            A[0, 0] = 3e-3
        Ad, Cd = _dev(A), _dev(rs.randn(M, N))
        ops.gemm(Ad, _dev(B), Cd, M, N, K, trans_a=ta, trans_b=tb, alpha=0.75, beta=0.5,
                 bias=_dev(rs.randn(N)), split_k=sk, precision=prec,
                 a_absmax=ops.absmax(Ad) if prec == 1 else None)
        _sync()
        return {'C': _sha(Cd)}
    return run


def _gemm_masks_views(prec):
    """The case of test_gemm_masks_and_strided_views (dU: a masked, shifted column slice times an
    offset B, split 2; dX: a C-row mask), the dU output a view (c_off, ldc > N) of a wider one."""
    def run():
        import torch
        from asr_study_amd import ops
        rs = np.random.RandomState(0)
        T, NB, H = 9, 16, 20
        y, dz = _dev(rs.randn(T * NB, 2 * H)), _dev(rs.randn(T * NB, 8 * H))
        mask = _dev((rs.rand(NB, H) > 0.3) / 0.7)
        out = {}
        for name, ldc, c_off in (('dU', 4 * H, 0), ('dU_view', 4 * H + 8, 4)):
            c = torch.full((H, ldc), 3.0, device=DEV)
            ops.gemm(y, dz, c, H, 4 * H, (T - 1) * NB, trans_a=True, lda=2 * H, ldb=8 * H,
                     ldc=ldc, c_off=c_off if ldc > 4 * H else 0, a_scale=mask, a_scale_period=NB,
                     b_off=NB * 8 * H, split_k=2, precision=prec,
                     beta=0.5 if ldc > 4 * H else 0.0)
            _sync()
            out[name] = _sha(c)
        W = _dev(rs.randn(24, 8 * H))
        mw = _dev((rs.rand(NB, 24) > 0.2) / 0.8)
        c = torch.zeros((T * NB, 24), device=DEV)
        ops.gemm(dz, W, c, T * NB, 24, 8 * H, trans_b=True, c_scale=mw, c_scale_period=NB,
                 precision=prec)
        _sync()
        out['dX'] = _sha(c)
        return out
    return run


def _gemm_fast(ta, tb, masked, sk):
    """gemm_f16x2_fast_kernel<ta, !tb, masked>: (260, 132, 72) has interior and edge tiles, three
    slabs (an odd count) and a K tail of 8."""
    def run():
        from asr_study_amd import ops
        M, N, K = 260, 132, 72
        rs = np.random.RandomState(4 * ta + 2 * tb + masked + 10 * sk)
        A = rs.randn(K, M) if ta else rs.randn(M, K)
        B = rs.randn(N, K) if tb else rs.randn(K, N)
        mask = _dev((rs.rand(16, A.shape[1]) > 0.3) / 0.7) if masked else None
        Ad, Bd, Cd = _dev(A), _dev(B), _dev(rs.randn(M, N))
        ops.gemm(Ad, Bd, Cd, M, N, K, trans_a=ta, trans_b=tb, alpha=0.75, beta=0.5,
                 bias=_dev(rs.randn(N)), a_scale=mask, a_scale_period=16 if masked else 0,
                 split_k=sk, precision=1, a_absmax=ops.absmax(Ad), b_absmax=ops.absmax(Bd))
        _sync()
        return {'C': _sha(Cd)}
    return run


# ------------------------------------------------------------------------------------- asr_pack_hl
def _planes(rows, k):
    from asr_study_amd import ops
    p = ops.HlPlanes(rows, k, DEV)
    p.hl.fill_(7.0)
    return p


def _pack_case(rows, cols, ld, off, period, two, both, mode):
    """mode: the value of ASR_PACK_ROWS (None = unset; '0' = the tiled kernel where the streaming
    one applies).  both: row and column planes in one pass."""
    def run():
        from asr_study_amd import ops
        rs = np.random.RandomState(rows + cols + off)
        sd = _dev(rs.randn(rows, ld) * 0.3)
        m1 = _dev((rs.rand(period, cols) > 0.2) / 0.8) if period else None
        m2 = _dev((rs.rand(period, cols) > 0.2) / 0.8) if two else None
        r, r2 = _planes(rows, cols), _planes(rows, cols) if two else None
        c = _planes(cols, rows) if both else None
        with _env('ASR_PACK_ROWS', mode):
            ops.pack_hl(sd, rows, cols, ld=ld, src_off=off, mask=m1, mask_period=period,
                        absmax=ops.absmax(sd), r=r, c=c, mask2=m2, r2=r2)
            _sync()
        out = {'r': _sha(r.hl), 'scale': _sha(r.scale)}
        if two:
            out['r2'] = _sha(r2.hl)
        if both:
            out['c'] = _sha(c.hl)
        return out
    return run


# ------------------------------------------------------------------------------------- asr_gemm_hl
def _packed(a, rows, cols, orient):
    """Planes of the (rows, cols) array a: 'r' = rows x (cols as K), 'c' = cols x (rows as K)."""
    from asr_study_amd import ops
    ad = _dev(a)
    p = _planes(rows, cols) if orient == 'r' else _planes(cols, rows)
    ops.pack_hl(ad, rows, cols, absmax=ops.absmax(ad), **{orient: p})
    return p


def _hl_row_case(M, N, K, sk=0, opts='plain', tile=0):
    def run():
        import torch
        from asr_study_amd import ops
        rs = np.random.RandomState(M + N + K + sk)
        pa = _packed(rs.randn(M, K), M, K, 'r')
        pb = _packed(rs.randn(K, N) * 0.05, K, N, 'c')
        kw, ldc = {}, N
        if opts == 'full':
            kw = dict(alpha=0.75, beta=0.5, bias=_dev(rs.randn(N)),
                      c_scale=_dev((rs.rand(16, N) > 0.3) / 0.7), c_scale_period=16)
        elif opts == 'view':                        # 16-byte aligned view of a wider matrix
            ldc = N + 64
            kw = dict(c_off=32, ldc=ldc, bias=_dev(rs.randn(N)))
        elif opts == 'view_odd':                    # unaligned: the element-wise epilogue
            ldc = N + 5
            kw = dict(c_off=3, ldc=ldc, beta=0.5)
        Cd = _dev(rs.randn(M + 1, ldc))             # (a row more: the view's last row fits)
        ops.gemm_hl(pa, pb, Cd, M, N, K, split_k=sk, tile=tile, **kw)
        _sync()
        return {'C': _sha(Cd)}
    return run


def _hl_km_case(M, N, K, sk=0, tile=0):
    """k_major, as test_gemm_hl_k_major_matches_float64: plane-row and column-group offsets."""
    def run():
        from asr_study_amd import ops
        rs = np.random.RandomState(M + N + K + tile)
        r0, ca, cb = 5, 32, 48
        ra, wa, wb = K + r0 + 3, M + ca + 16, N + cb + 32
        pa = _packed(rs.randn(ra, wa), ra, wa, 'r')
        pb = _packed(rs.randn(ra, wb) * 0.05, ra, wb, 'r')
        Cd = _dev(rs.randn(M, N))
        ops.gemm_hl(pa, pb, Cd, M, N, K, a_row=r0, a_k=ca, b_row=r0 + 2, b_k=cb, alpha=0.75,
                    beta=0.5, split_k=sk, tile=tile, k_major=True)
        _sync()
        return {'C': _sha(Cd)}
    return run


def _hl_batch_case(M, N, K, shifts, sk):
    def run():
        import torch
        from asr_study_amd import ops
        rs = np.random.RandomState(M + N + K + sk)
        rows = K + max(shifts)
        pa = _packed(rs.randn(rows, M), rows, M, 'r')
        pb = _packed(rs.randn(K, N), K, N, 'r')
        c = torch.full((len(shifts) * M + 2, N), 9.0, device=DEV)
        ops.gemm_hl(pa, pb, c, M, N, K, k_major=True, batch_rows=shifts, split_k=sk)
        _sync()
        return {'C': _sha(c)}
    return run


def _hl_seg_case(M, N, seg_k, shifts, sk):
    def run():
        import torch
        from asr_study_amd import ops
        rs = np.random.RandomState(M + N + seg_k)
        rows, K = M + max(shifts), seg_k * len(shifts)
        pa = _packed(rs.randn(rows, seg_k), rows, seg_k, 'r')
        pb = _packed(rs.randn(N, K), N, K, 'r')
        c = torch.full((M, N), 9.0, device=DEV)
        ops.gemm_hl(pa, pb, c, M, N, K, a_seg_k=seg_k, a_seg_rows=shifts, split_k=sk)
        _sync()
        return {'C': _sha(c)}
    return run


def _conv_fwd_clamp():
    """The smallest forward case of tests/test_gpu_conv.py through ops.Conv2d: with z the GEMM
    writes z, without it the clipped ReLU runs in the segmented GEMM's epilogue (clamp_hi)."""
    import torch
    from asr_study_amd import ops
    T, N, F, Ci, Co, kt, kf, st, sf, clip = 13, 5, 12, 1, 4, 5, 7, 2, 2, 1.0
    rs = np.random.RandomState(T * 31 + F)
    n_pad = ops.pad16(N)
    x = np.zeros((T, n_pad, F * Ci))
    x[:, :N] = rs.randn(T, N, F * Ci)
    xd, Wd, bd = _dev(x), _dev(rs.randn(kt, kf, Ci, Co) * 0.3), _dev(rs.randn(Co) * 0.2)
    out = {}
    for fused in (False, True):
        op = ops.Conv2d(T, n_pad, F, Ci, Co, kt, kf, st, sf, clip, DEV)
        y = torch.full((op.T_out, n_pad, op.F_out * Co), 7.0, device=DEV)
        z = None if fused else torch.full_like(y, 7.0)
        op.fwd(xd, Wd, bd, z, y)
        _sync()
        out['y_fused' if fused else 'y'] = _sha(y)
        if z is not None:
            out['z'] = _sha(z)
    return out


def _hl_persist_case(M, N, K, opts):
    """Under ASR_GEMM_PERSIST = 1 (gemm_hlp_kernel) and = 0 (gemm_hlx_kernel), the same planes.
    The old C of the mask case is one random block of rows repeated (M x N floats drawn one by
    one would be most of the case's time)."""
    def run():
        import torch
        from asr_study_amd import ops
        rs = np.random.RandomState(M + N + K)
        pa = _packed(rs.randn(M, K), M, K, 'r')
        pb = _packed(rs.randn(K, N) * 0.05, K, N, 'c')
        kw = {}
        if opts == 'mask':
            kw = dict(alpha=0.75, beta=0.5, bias=_dev(rs.randn(N)),
                      c_scale=_dev((rs.rand(16, N) > 0.3) / 0.7), c_scale_period=16)
        block = _dev(rs.randn(61, N))
        C0 = block.repeat((M + 60) // 61, 1)[:M].contiguous()
        out = {}
        for mode in ('1', '0'):
            with _env('ASR_GEMM_PERSIST', mode):
                Cd = C0.clone()
                ops.gemm_hl(pa, pb, Cd, M, N, K, **kw)
                _sync()
            out['C_persist' + mode] = _sha(Cd)
        return out
    return run


# ------------------------------------------------------------------------------------- flat
def _absmax_case(n):
    def run():
        import torch
        from asr_study_amd import ops
        from tests import flat_cases as FC
        x = np.random.RandomState(9).randn(n).astype(np.float32)
        xd = _dev(x)
        out = {}
        for k, pos in enumerate([None] + FC.absmax_positions(n)):
            if pos is not None:
                xd = _dev(x)
                xd[pos] = -(3.5 + k) if k % 2 else 3.5 + k
            o = torch.full((4,), 7.0, device=DEV)
            ops.absmax(xd, o)
            _sync()
            out['max_at_%s' % pos] = _sha(o)
        return out
    return run


def _colsum_case(M):
    def run():
        import torch
        from asr_study_amd import ops
        from tests import flat_cases as FC
        rs = np.random.RandomState(10 + M % 97)
        out = {}
        for N in FC.COLSUM_N:
            data = rs.randn(M, N).astype(np.float32)
            out0 = rs.randn(N + 3).astype(np.float32) * np.float32(50.0)
            for ld_mul, off_mul in FC.COLSUM_LD:
                X = np.full((M, ld_mul * N), 1e30, np.float32)
                X[:, off_mul * N:off_mul * N + N] = data
                Xd = _dev(X)
                for beta in FC.COLSUM_BETA:
                    o = _dev(out0)
                    ops.colsum(Xd, M, N, ld_mul * N, o, beta=beta, x_off=off_mul * N)
                    _sync()
                    out['N%d_ld%d_beta%g' % (N, ld_mul, beta)] = _sha(o)
        return out
    return run


def _cases():
    c = {}
    for (M, N, K, ta, tb, sk) in GEMM_SHAPES:
        for prec in (0, 1):
            c['gemm_p%d_%dx%dx%d' % (prec, M, N, K)] = _gemm_case(M, N, K, ta, tb, sk, prec)
    for prec in (0, 1):
        c['gemm_p%d_masks_views' % prec] = _gemm_masks_views(prec)
    for ta in (False, True):
        for tb in (False, True):
            for masked in (False, True):
                c['gemm_fast_ta%d_tb%d_mask%d' % (ta, tb, masked)] = _gemm_fast(ta, tb, masked, 0)
    c['gemm_fast_ta1_tb0_mask1_split2'] = _gemm_fast(True, False, True, 2)

    c['pack_300x200_both'] = _pack_case(300, 200, 200, 0, 0, False, True, None)
    c['pack_300x200_both_masked'] = _pack_case(300, 200, 200, 0, 16, False, True, None)
    c['pack_333x100_two_masks'] = _pack_case(333, 100, 104, 0, 48, True, False, None)
    for mode in (None, '0'):
        tag = 'rows' if mode is None else 'tiled'
        c['pack_257x16_' + tag] = _pack_case(257, 16, 16, 0, 0, False, False, mode)
        c['pack_333x48_off8_two_masks_' + tag] = _pack_case(333, 48, 64, 8, 48, True, False, mode)

    c['hl_300x200x64'] = _hl_row_case(300, 200, 64)                     # the 128 tile
    c['hl_260x132x40'] = _hl_row_case(260, 132, 40)
    c['hl_300x260x72'] = _hl_row_case(300, 260, 72)                     # the 256 tile, edges
    c['hl_300x260x72_tile128'] = _hl_row_case(300, 260, 72, tile=128)
    c['hl_300x260x328_split3'] = _hl_row_case(300, 260, 328, sk=3)
    c['hl_260x132x328_split3'] = _hl_row_case(260, 132, 328, sk=3)
    c['hl_300x260x72_full'] = _hl_row_case(300, 260, 72, opts='full')
    c['hl_260x132x40_full'] = _hl_row_case(260, 132, 40, opts='full')
    c['hl_512x256x72_full'] = _hl_row_case(512, 256, 72, opts='full')   # interior tiles only
    c['hl_300x260x72_view'] = _hl_row_case(300, 260, 72, opts='view')
    c['hl_300x260x72_view_odd'] = _hl_row_case(300, 260, 72, opts='view_odd')
    for tile in (0, 128):
        c['hl_km_300x200x64_tile%d' % tile] = _hl_km_case(300, 200, 64, tile=tile)
        c['hl_km_260x132x41_tile%d' % tile] = _hl_km_case(260, 132, 41, tile=tile)
        c['hl_km_300x260x41_tile%d' % tile] = _hl_km_case(300, 260, 41, tile=tile)
    c['hl_km_260x132x200_split3'] = _hl_km_case(260, 132, 200, sk=3)
    c['hl_km_300x260x200_split3'] = _hl_km_case(300, 260, 200, sk=3)
    c['hl_km_batch_80x132x100'] = _hl_batch_case(80, 132, 100, [3, 0, 11], 0)
    c['hl_km_batch_80x132x100_split3'] = _hl_batch_case(80, 132, 100, [3, 0, 11], 3)
    c['hl_km_batch_256x300x70'] = _hl_batch_case(256, 300, 70, [0, 32, 16, 80], 0)
    c['hl_seg_130x70x32'] = _hl_seg_case(130, 70, 32, [5, 0, 9, 2, 7], 0)
    c['hl_seg_300x260x64'] = _hl_seg_case(300, 260, 64, [0, 48, 16, 32], 0)
    c['hl_seg_256x256x64_split2'] = _hl_seg_case(256, 256, 64, [16, 0, 32, 48], 2)
    c['conv_fwd_clamp'] = _conv_fwd_clamp
    c['hl_persist_8192x4352x160'] = _hl_persist_case(8192, 4352, 160, 'plain')
    c['hl_persist_8292x4200x328'] = _hl_persist_case(8292, 4200, 328, 'plain')
    c['hl_persist_8292x4200x256_mask'] = _hl_persist_case(8292, 4200, 256, 'mask')

    from tests import flat_cases as FC
    for n in FC.sizes('absmax'):
        c['absmax_n%d' % n] = _absmax_case(n)
    for M in FC.COLSUM_M:
        c['colsum_M%d' % M] = _colsum_case(M)
    return c


_CASES = _cases()
CASES = sorted(_CASES)


def record(name):
    return _CASES[name]()


if __name__ == '__main__':
    import time
    tables = []
    for rep in range(2):
        table = {}
        for name in CASES:
            t0 = time.time()
            table[name] = record(name)
            print('%d %-40s %.2f s' % (rep, name, time.time() - t0), flush=True)
        tables.append(table)
    differ = [n for n in CASES if tables[0][n] != tables[1][n]]
    if differ:
        sys.exit('not repeatable, nothing written: %s' % differ)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'gemm_bits_parent.json')
    with open(dst, 'w') as f:
        json.dump(tables[0], f, sort_keys=True, indent=0)
        f.write('\n')
