"""What tests/test_gpu_batchnorm.py, tests/test_gpu_seqbn.py, tests/test_gpu_bn_bits.py and
tests/golden/gen_bn_bits.py share: the shapes of the kernel tests of csrc/batchnorm.hip, the
construction of their inputs, the runs of the kernels, and the record of a run (SHA-256 of the
inputs and of every array the kernels return) that pins their bits."""
import hashlib

import numpy as np

# (T, N, n_pad, ld, W, C): 2-D widths 1, 3, 32, 1024, 1026 (with pads) and 2048, the 40 x 32
# conv image, rows from 1 to 64 000 with n_pad > N; C = 12: C / 4 = 3 does not divide 64, so
# cw = 63, rw = 4 and four lanes of every workgroup idle, and the boundary of the two column tiles
# (252 = 21 * 12) falls on a channel boundary
BN_CASES = [(1, 1, 16, 4, 1, None), (7, 5, 16, 4, 3, None), (50, 13, 16, 32, 32, None),
            (100, 64, 64, 1024, 1024, None), (33, 20, 32, 1028, 1026, None),
            (20, 50, 64, 2048, 2048, None), (60, 9, 16, 1280, 1280, 32),
            (1000, 64, 64, 32, 32, None), (31, 3, 16, 80, 80, 8), (9, 3, 16, 504, 504, 12)]

# (T, N, n_pad, ld, W, Hp, H): the slab of a GRU with H = 18 (Hp = 20: pad columns inside every
# block), pad columns behind W, the cfg3 width 3072 with N = n_pad and N < n_pad, a narrow slab
SEQBN_CASES = [(30, 5, 16, 120, 120, 20, 18), (33, 20, 32, 1028, 1026, None, None),
               (60, 64, 64, 3072, 3072, None, None), (50, 13, 16, 3072, 3072, None, None),
               (7, 3, 16, 24, 24, None, None), (1, 1, 16, 4, 3, None, None)]

# the bit pin alone: 3200 real rows in 100 row partitions, so the finalize's lane-strided loop
# takes a second trip (at a fifth of the rows of the 1000-frame case)
BITS_ONLY = (50, 64, 64, 32, 32)


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda:0')


def bn_inputs(T, N, n_pad, ld, W, C):
    """x, gamma, beta, dy, running mean, running variance of a BatchNormalization case."""
    rs = np.random.RandomState(T + W)
    Cn = W if C is None else C
    x = np.zeros((T, n_pad, ld), np.float32)
    x[:, :N, :W] = rs.randn(T, N, W) * 1.5 + rs.randn(W) * 0.5
    x[:, N:, :] = rs.randn(T, n_pad - N, ld)       # junk in padding rows / columns: ignored
    x[:, :N, W:] = rs.randn(T, N, ld - W)
    if C is None and W >= 3:
        x[:, :N, 1] = 1e3 + 0.1 * rs.randn(T, N)    # stability: |mean| 1e3, std 0.1
        x[:, :N, 2] = 0.25                          # a constant column: var 0
    gamma, beta = rs.rand(Cn) + 0.5, rs.randn(Cn) * 0.3
    dy = rs.randn(T, n_pad, ld).astype(np.float32)
    rm, rv = rs.randn(Cn), rs.rand(Cn) + 0.5
    return x, gamma, beta, dy, rm, rv


def run_bn_kernels(x, N, W, C, gamma, beta, dy, clip, rm=None, rv=None):
    """x (T, n_pad, ld) host float32 -> y, stats, dx, dgamma, dbeta, infer y, moments (host
    arrays)."""
    import torch
    from asr_study_amd import ops
    xd, dyd = _dev(x), _dev(dy)
    y = torch.full_like(xd, 7.0)            # pads must be written, not left alone
    stats = torch.empty(ops.bn_stats_len(C), device='cuda:0')
    mom = torch.empty(ops.bn_moments_len(C), device='cuda:0')
    g, b = _dev(gamma), _dev(beta)
    ops.bn_fwd_train(xd, y, g, b, stats, N, W, C, 1e-3, clip, moments=mom, weight=float(N))
    dx = torch.full_like(xd, 7.0)
    dg, db = torch.empty(C, device='cuda:0'), torch.empty(C, device='cuda:0')
    ops.bn_bwd(xd, dyd, g, b, stats, dx, dg, db, N, W, C, clip)
    yi = torch.full_like(xd, 7.0)
    if rm is not None:
        ops.bn_fwd_infer(xd, yi, g, b, _dev(rm), _dev(rv), N, W, C, 1e-3, clip)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (y, stats, dx, dg, db, yi, mom)]


def ragged(rs, T, N):
    """Lengths in [1, T] with one sample of length 1 and one of length T (N >= 2)."""
    lens = rs.randint(1, T + 1, size=N)
    lens[0] = T
    if N > 1:
        lens[-1] = 1
    return lens


def seqbn_inputs(T, N, n_pad, ld, W, Hp, H, is_ragged):
    """p, gamma, beta, da, lengths, running mean, running variance and the mask of the pad
    columns inside a GRU slab of a sequence-wise BatchNormalization case."""
    rs = np.random.RandomState(T + W)
    p = np.zeros((T, n_pad, ld), np.float32)
    p[:, :N, :W] = rs.randn(T, N, W) * 1.5 + rs.randn(W) * 0.5
    p[:, N:, :] = rs.randn(T, n_pad - N, ld)       # junk in padding rows / columns: ignored
    p[:, :N, W:] = rs.randn(T, N, ld - W)
    if W >= 3:
        p[:, :N, 1] = 1e3 + 0.1 * rs.randn(T, N)    # stability: |mean| 1e3, std 0.1
        p[:, :N, 2] = 0.25                          # a constant column: var 0
    gamma, beta = rs.rand(W) + 0.5, rs.randn(W) * 0.3
    gamma[0] = 0.0                                  # xhat comes from p, never from y
    pad = np.zeros(W, bool)
    if Hp is not None:      # pad columns of a GRU slab: p = 0 (zero weight columns), gamma = beta = 0
        pad = (np.arange(W) % Hp) >= H
        p[:, :N, :W][..., pad] = 0.0
        gamma[pad] = 0.0
        beta[pad] = 0.0
    da = rs.randn(T, n_pad, ld).astype(np.float32)  # non-zero on padded frames and pads
    lens = ragged(rs, T, N) if is_ragged else (None if T % 2 else np.full(N, T))
    rm, rv = rs.randn(W), rs.rand(W) + 0.5
    return p, gamma, beta, da, lens, rm, rv, pad


def run_seqbn_kernels(p, N, W, lens, gamma, beta, da, rm=None, rv=None, shift=None, weight=1.0):
    """p, da (T, n_pad, ld) host float32 -> y, stats, dp, dgamma, dbeta, infer y, moments,
    max |dp| (host arrays)."""
    import torch
    from asr_study_amd import ops
    pd, dad = _dev(p), _dev(da)
    ld = None if lens is None else torch.tensor(np.asarray(lens), dtype=torch.int32,
                                                device='cuda:0')
    y = torch.full_like(pd, 7.0)            # pads must be written, not left alone
    stats = torch.empty(ops.seqbn_stats_len(W), device='cuda:0')
    mom = torch.empty(ops.bn_moments_len(W), device='cuda:0')
    g, b = _dev(gamma), _dev(beta)
    ops.seqbn_fwd_train(pd, y, g, b, stats, N, W, lens=ld, eps=1e-3, moments=mom,
                        shift=None if shift is None else _dev(shift), weight=weight)
    dp = torch.full_like(pd, 7.0)
    dg, db = torch.empty(W, device='cuda:0'), torch.empty(W, device='cuda:0')
    mx = torch.full((1,), 7.0, device='cuda:0')
    ops.seqbn_bwd(pd, dad, g, stats, dp, dg, N, W, lens=ld, dbeta=db, dp_absmax=mx)
    yi = torch.full_like(pd, 7.0)
    if rm is not None:
        ops.seqbn_fwd_infer(pd, yi, g, b, _dev(rm), _dev(rv), N, W, 1e-3)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (y, stats, dp, dg, db, yi, mom, mx)]


# ------------------------------------------------------------------------------ the bit pin
_BN_OUT = ('y', 'stats', 'dx', 'dgamma', 'dbeta', 'infer_y', 'moments')
_SEQBN_OUT = _BN_OUT + ('dp_absmax',)


def _bit_cases():
    """name -> (kind, shape, clip or ragged): every case of the two kernel parity tests plus
    BITS_ONLY, for both families."""
    out = {}
    for shape in BN_CASES + [BITS_ONLY + (None,)]:
        for tag, clip in (('plain', 0.0), ('clip', 2.0)):
            out['bn-%s-%s' % ('-'.join(map(str, shape)), tag)] = ('bn', shape, clip)
    for shape in SEQBN_CASES + [BITS_ONLY + (None, None)]:
        for tag, rag in (('ragged', True), ('full', False)):
            out['seqbn-%s-%s' % ('-'.join(map(str, shape)), tag)] = ('seqbn', shape, rag)
    return out


BIT_CASES = _bit_cases()


def _sha(arrays):
    """One SHA-256 over the raw bytes of the arrays (None: the word 'None'), in order."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(b'None' if a is None else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def bit_inputs(name):
    """(the inputs of BIT_CASES[name], their SHA-256)."""
    kind, shape, flag = BIT_CASES[name]
    arrays = bn_inputs(*shape) if kind == 'bn' else seqbn_inputs(*(shape + (flag,)))[:7]
    return arrays, _sha(arrays)


def bit_outputs(name, arrays):
    """{output name: SHA-256 of its raw bytes} of one run of the kernels on bit_inputs(name)."""
    kind, shape, flag = BIT_CASES[name]
    T, N, n_pad, ld, W = shape[:5]
    if kind == 'bn':
        x, gamma, beta, dy, rm, rv = arrays
        C = W if shape[5] is None else shape[5]
        got = run_bn_kernels(x, N, W, C, gamma, beta, dy, flag, rm, rv)
        return {k: _sha([a]) for k, a in zip(_BN_OUT, got)}
    p, gamma, beta, da, lens, rm, rv = arrays
    got = run_seqbn_kernels(p, N, W, lens, gamma, beta, da, rm, rv)
    return {k: _sha([a]) for k, a in zip(_SEQBN_OUT, got)}
