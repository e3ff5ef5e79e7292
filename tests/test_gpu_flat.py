"""-m gpu: the flat element-wise and reduction kernels at every case of tests/flat_cases.py -- past
one grid, at every tail length, on both alignments of the optimiser -- against float64 NumPy
(oracle/rng.py, oracle/optim.py and tests/conformer_oracle.py where they exist).  Every output is
pre-filled with a sentinel and has a guard band behind it (and in front of it where the view is
offset) that must come back untouched.

Bounds.  mul, the random words / masks / dropout products, relu / linear / clipped ReLU and
absmax are exact: bit for bit.  (relu and the clipped ReLU of +-0 are a zero of either sign:
fmaxf(-0, +0) may return either operand.)  axpby: |err| <= 2^-23 (|a x| + |b y|), two roundings,
contracted or not.  colsum: |err| <= 2^-23 (|beta out0| + |sum|), float64 partials and one or two
fp32 roundings.  tanh: BOUND (tests/test_gpu_conformer.py) absolute forward, 2^-22 |dy| backward
(y^2 and 1 - y^2 round at 2^-24 each below 1, the product once more).  swish / GLU, Gaussian
noise, the norm's random case and the optimiser's p: the bars of their existing tests; m, v and
the velocity: BOUND against oracle/optim.py."""
import numpy as np
import pytest
import torch

from oracle import optim as OO
from oracle import rng as ORNG
from tests import conformer_oracle as CO
from tests import flat_cases as FC
from tests.gpu_util import report, to_dev
from tests.test_gpu_conformer import BOUND, SPECIAL

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats behind (and in front of) every output
SENT = -777.25                  # exact in float32; no kernel under test produces it
SEED, SID, STEP = (0x1234 << 32) | 0xBEEF, 11, 42
EPS23, EPS22 = 2.0 ** -23, 2.0 ** -22
_BASE = {}


def _base(seed, n):
    """n standard normals (float32) of a stream drawn once per module and seed; past 2^20 of
    them the stream repeats (no kernel here has that period)."""
    if seed not in _BASE:
        _BASE[seed] = np.random.RandomState(seed).randn((1 << 20) + 77).astype(np.float32)
    return np.resize(_BASE[seed], n)


class Guarded(object):
    """A float32 (or int32) device buffer of n elements between two guard bands; `off` shifts the
    view by that many elements off the 16-byte alignment of the allocation."""

    def __init__(self, n, off=0, dtype=torch.float32, fill=SENT, init=None):
        self.n, self.lo = n, GUARD + off
        self.fill = int(fill) if dtype == torch.int32 else fill
        self.buf = torch.full((self.lo + n + GUARD,), self.fill, dtype=dtype, device='cuda:0')
        self.t = self.buf[self.lo:self.lo + n]
        assert self.t.data_ptr() % 16 == (4 * off) % 16
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)))

    def numpy(self):
        """The payload, after checking that neither guard band was written."""
        h = self.buf.cpu().numpy()
        assert (h[:self.lo] == self.fill).all(), 'write in front of the buffer'
        assert (h[self.lo + self.n:] == self.fill).all(), 'write behind the buffer'
        return h[self.lo:self.lo + self.n].copy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want, what):
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, '%s: %d elements differ, first at %d (got %r want %r)' % (
        what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _within(got, want, bound, what):
    """|got - want| <= bound element by element; prints the worst ratio before it asserts."""
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.isfinite(np.asarray(got)).all(), what
    ratio = err / np.where(bound > 0, bound, 1.0)
    ratio[(bound == 0) & (err == 0)] = 0.0
    ratio[(bound == 0) & (err > 0)] = np.inf
    i = int(np.argmax(ratio))
    print('[flat] %-34s max|err| %.3e, worst err/bound %.3f at %d' % (what, err.max(), ratio[i], i))
    assert ratio[i] <= 1.0, (what, i, float(err[i]), float(np.broadcast_to(bound, err.shape)[i]))
    return err.max()


# ------------------------------------------------------------------------------------- random
@pytest.mark.parametrize('n', FC.sizes('random'))
def test_random_streams_bit_equal_to_the_oracle(n):
    from asr_study_amd import _lib as L, ops
    lib = L.load()
    words = ORNG.words(n, SEED, SID, STEP)
    w = Guarded(n, dtype=torch.int32, fill=-7)
    L.check(lib.asr_random_words(ops._ptr(w.t), n, SEED, SID, STEP, ops._stream()), 'words')
    assert np.array_equal(w.numpy().view(np.uint32), words)
    m = Guarded(n)
    ops.dropout_masks(m.t, 0.2, 1.25, SEED, SID, STEP)
    _same_bits(m.numpy(), ORNG.keep_mask(n, 0.2, 1.25, SEED, SID, STEP), 'keep mask')
    x = _base(1, n)
    want = ORNG.keep_mask(n, 0.35, 1.0 / 0.65, SEED, SID + 1, STEP)
    xd = to_dev(x)
    out, mk = Guarded(n), Guarded(n)
    ops.dropout_apply(xd, out.t, mk.t, 0.35, 1.0 / 0.65, SEED, SID + 1, STEP)
    _same_bits(mk.numpy(), want, 'dropout mask_out')
    _same_bits(out.numpy(), x * want, 'dropout product')
    out2 = Guarded(n)
    ops.dropout_apply(xd, out2.t, None, 0.35, 1.0 / 0.65, SEED, SID + 1, STEP)
    _same_bits(out2.numpy(), x * want, 'dropout product, no mask_out')
    inp = Guarded(n, init=x)
    ops.dropout_apply(inp.t, inp.t, None, 0.35, 1.0 / 0.65, SEED, SID + 1, STEP)
    _same_bits(inp.numpy(), x * want, 'dropout in place')
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                 # the input is only read


@pytest.mark.parametrize('n', FC.sizes('random'))
def test_gaussian_noise_with_and_without_an_input(n):
    from asr_study_amd import ops
    x = _base(2, n)
    z64 = 0.5 * ORNG.normal(n, SEED, SID + 2, STEP)
    z, pure = Guarded(n), Guarded(n)
    ops.gaussian_noise(to_dev(x), z.t, 0.5, SEED, SID + 2, STEP)
    ops.gaussian_noise(None, pure.t, 0.5, SEED, SID + 2, STEP)
    e1 = report('noise + x n=%d' % n, z.numpy(), x.astype(np.float64) + z64)
    e2 = report('pure noise n=%d' % n, pure.numpy(), z64)
    assert e1 < 2e-5 and e2 < 2e-5


# ------------------------------------------------------------------------------------- mul, axpby
@pytest.mark.parametrize('n', FC.sizes('mul'))
def test_mul_is_the_fp32_product(n):
    from asr_study_amd import ops
    x, y = _base(3, n), _base(4, n)
    out = Guarded(n)
    ops.mul(to_dev(x), to_dev(y), out.t)
    _same_bits(out.numpy(), x * y, 'mul n=%d' % n)
    inp = Guarded(n, init=x)                                          # in place: out is x
    ops.mul(inp.t, to_dev(y), inp.t)
    _same_bits(inp.numpy(), x * y, 'mul in place n=%d' % n)


@pytest.mark.parametrize('n', FC.sizes('axpby'))
def test_axpby_within_two_roundings(n):
    from asr_study_amd import ops
    x, y = _base(3, n), _base(4, n)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    xd, yd = to_dev(x), to_dev(y)
    for a, b in ((1.7, -0.3), (1.0, 1.0)):
        a32, b32 = float(np.float32(a)), float(np.float32(b))
        out = Guarded(n)
        ops.axpby(a, xd, b, yd, out.t)
        _within(out.numpy(), a32 * x64 + b32 * y64,
                EPS23 * (np.abs(a32 * x64) + np.abs(b32 * y64)), 'axpby %g %g n=%d' % (a, b, n))
    coef = float(np.float32(0.70710678))                              # core/stages.py: y is x, b 0
    out = Guarded(n)
    ops.axpby(coef, xd, 0.0, xd, out.t)
    _within(out.numpy(), coef * x64, EPS23 * np.abs(coef * x64), 'axpby coef, 0, y = x n=%d' % n)
    assert torch.equal(xd.cpu(), torch.from_numpy(x))


# ------------------------------------------------------------------------------------- activations
def _act_input(n, clip):
    x = _base(5, n) * np.float32(4.0)
    edge = np.concatenate([SPECIAL, np.array([clip, -clip, 0.0, -0.0, np.nextafter(
        np.float32(clip), np.float32(0)), np.nextafter(np.float32(clip), np.float32(1e9))],
        np.float32)])
    k = min(n, edge.size)
    x[:k] = edge[:k]
    x[n - k:] = edge[:k][::-1]                     # the tail and the wrapped trip get them too
    return x


CLIP = 20.0


@pytest.mark.parametrize('n', FC.sizes('activation'))
def test_relu_linear_and_clipped_relu_are_exact(n):
    from asr_study_amd import ops
    x = _act_input(n, CLIP)
    dy = _base(6, n)
    xd, dyd = to_dev(x), to_dev(dy)
    clip32 = np.float32(CLIP)
    for act, want, slope in (
            ('relu', np.maximum(x, np.float32(0)), lambda y: y > 0),
            ('linear', x, lambda y: np.ones(y.shape, bool)),
            (('clipped_relu', CLIP), np.minimum(np.maximum(x, np.float32(0)), clip32),
             lambda y: (y > 0) & (y < clip32))):
        y = Guarded(n)
        ops.activation_fwd(xd, y.t, act)
        got = y.numpy()
        nz = want != 0
        assert np.array_equal(got, want), act                         # numerically, zeros included
        _same_bits(got[nz], want[nz], '%s forward n=%d' % (act, n))
        if act == 'linear':
            _same_bits(got, want, 'linear forward n=%d' % n)
        # the derivative is read from y; 0 and clip both count as clipped (slope 0)
        yin = want.astype(np.float32)
        dx = Guarded(n)
        ops.activation_bwd(dyd, to_dev(yin), dx.t, act)
        _same_bits(dx.numpy(), dy * slope(yin).astype(np.float32), '%s backward n=%d' % (act, n))
    if n >= SPECIAL.size:
        yin = np.minimum(np.maximum(x, np.float32(0)), clip32)
        assert (yin == 0).any() and (yin == clip32).any()


@pytest.mark.parametrize('n', FC.sizes('activation'))
def test_tanh_forward_and_backward(n):
    from asr_study_amd import ops
    x = _act_input(n, CLIP)
    dy = _base(6, n)
    y = Guarded(n)
    ops.activation_fwd(to_dev(x), y.t, 'tanh')
    want = np.tanh(x.astype(np.float64))
    _within(y.numpy(), want, np.full(n, BOUND), 'tanh forward n=%d' % n)
    yin = want.astype(np.float32)                                     # +-1 and +-0 among them
    dx = Guarded(n)
    ops.activation_bwd(to_dev(dy), to_dev(yin), dx.t, 'tanh')
    y64, dy64 = yin.astype(np.float64), dy.astype(np.float64)
    _within(dx.numpy(), dy64 * (1.0 - y64 * y64), EPS22 * np.abs(dy64), 'tanh backward n=%d' % n)


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


@pytest.mark.parametrize('n', FC.sizes('swish'))
def test_swish_past_one_grid(n):
    from asr_study_amd import ops
    x = _act_input(n, CLIP)
    dy = _base(6, n)
    y, dx = Guarded(n), Guarded(n)
    xd = to_dev(x)
    ops.swish_fwd(xd, y.t)
    ops.swish_bwd(xd, to_dev(dy), dx.t)
    y, dx = y.numpy(), dx.numpy()
    x64 = x.astype(np.float64)
    wy, wdx = CO.swish(x64), CO.swish_backward(dy.astype(np.float64), x64)
    ey, edx = _rel(y, wy), _rel(dx, wdx)
    print('[flat] swish n %d: y %.2e dx %.2e (bound %.0e)' % (n, ey, edx, BOUND))
    assert np.isfinite(y).all() and np.isfinite(dx).all()
    assert ey < BOUND and edx < BOUND
    small = np.abs(x64) <= 20
    assert np.abs(y - wy)[small].max(initial=0.0) <= 1e-5 * 20


@pytest.mark.parametrize('rows,C,ld_in,ld_out', FC.GLU_CASES)
def test_glu_past_one_grid(rows, C, ld_in, ld_out):
    from asr_study_amd import ops
    x = _base(7, rows * ld_in).reshape(rows, ld_in) * np.float32(3.0)
    x[-1, :2 * C] = np.resize(SPECIAL, 2 * C)
    x[0, C:2 * C] = np.resize(SPECIAL, C)
    dy = _base(8, rows * ld_out).reshape(rows, ld_out)
    y, dx = Guarded(rows * ld_out), Guarded(rows * ld_in)
    xd = to_dev(x)
    ops.glu_fwd(xd, y.t.view(rows, ld_out), C_=C)
    ops.glu_bwd(xd, to_dev(dy), dx.t.view(rows, ld_in), C_=C)
    y, dx = y.numpy().reshape(rows, ld_out), dx.numpy().reshape(rows, ld_in)
    x64 = x[:, :2 * C].astype(np.float64)
    ey = _rel(y[:, :C], CO.glu_forward(x64)[0])
    edx = _rel(dx[:, :2 * C], CO.glu_backward(dy[:, :C].astype(np.float64), x64))
    print('[flat] glu rows %d C %d ld %d/%d: y %.2e dx %.2e (bound %.0e)'
          % (rows, C, ld_in, ld_out, ey, edx, BOUND))
    assert np.isfinite(y).all() and np.isfinite(dx).all()
    assert ey < BOUND and edx < BOUND
    assert not y[:, C:].any() and not dx[:, 2 * C:].any()


# ------------------------------------------------------------------------------------- absmax
@pytest.mark.parametrize('n', FC.sizes('absmax'))
def test_absmax_is_exactly_the_maximum(n):
    from asr_study_amd import ops
    x = np.clip(_base(9, n), -3, 3)
    xd = to_dev(x)
    out = Guarded(1)
    ops.absmax(xd, out.t)
    _same_bits(out.numpy(), np.abs(x).max(keepdims=True), 'absmax n=%d' % n)
    for k, pos in enumerate(FC.absmax_positions(n)):
        val = np.float32(3.5 + k) * (-1 if k % 2 else 1)              # every second one negative
        old = xd[pos].clone()
        xd[pos] = float(val)
        out = Guarded(1)
        ops.absmax(xd, out.t)
        got = out.numpy()
        assert got[0] == abs(val), (n, pos, got[0], val)
        xd[pos] = old
    for fill in (0.0, -0.0):
        out = Guarded(1)
        ops.absmax(torch.full((n,), fill, device='cuda:0'), out.t)
        assert _bits(out.numpy())[0] == 0, (n, fill)


# ------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize('M', FC.COLSUM_M)
@pytest.mark.parametrize('N', FC.COLSUM_N)
def test_colsum_slices_strides_and_beta(M, N):
    from asr_study_amd import ops
    data = _base(10, M * N).reshape(M, N)
    want = data.astype(np.float64).sum(axis=0)
    out0 = _base(11, N + 3) * np.float32(50.0)
    for ld_mul, off_mul in FC.COLSUM_LD:
        ldx, x_off = ld_mul * N, off_mul * N
        X = np.full((M, ldx), 1e30, np.float32)                       # what must never be read
        X[:, x_off:x_off + N] = data
        Xd = to_dev(X)
        for beta in FC.COLSUM_BETA:
            out = Guarded(N + 3, init=out0)                           # three columns past N
            if beta == 0.0:
                out.t[:N] = float('nan')                              # beta 0 does not read out
            ops.colsum(Xd, M, N, ldx, out.t, beta=beta, x_off=x_off)
            got = out.numpy()
            _same_bits(got[N:], out0[N:], 'colsum columns past N')
            prev = beta * out0[:N].astype(np.float64)
            _within(got[:N], prev + want, EPS23 * (np.abs(prev) + np.abs(want)),
                    'colsum M=%d N=%d ldx=%d beta=%g' % (M, N, ldx, beta))


# ------------------------------------------------------------------------------------- norm
def _norm_run(p, g, segs, off):
    from asr_study_amd import ops
    n = p.size
    sd, nseg = ops.make_segments(segs, 'cuda:0')
    pd, gd = Guarded(n, off, init=p), Guarded(n, off, init=g)
    norm = torch.full((2 + GUARD,), SENT, dtype=torch.float64, device='cuda:0')
    ops.grad_norm(pd.t, gd.t, sd, nseg, norm[:2])
    h = norm.cpu().numpy()
    assert (h[2:] == SENT).all()
    _same_bits(pd.numpy(), p, 'params after the norm')
    _same_bits(gd.numpy(), g, 'grads after the norm')
    return h[:2]


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'offset'])
@pytest.mark.parametrize('n,layout', FC.norm_cases())
def test_norm_random_data(n, layout, off):
    segs = FC.layouts(n)[layout]
    p, g = _base(12, n), _base(13, n)
    l2 = FC.l2_vector(segs, n).astype(np.float64)
    p64 = p.astype(np.float64)
    want = np.sqrt(np.sum((g.astype(np.float64) + 2 * l2 * p64) ** 2))
    pen = np.sum(l2 * p64 ** 2)
    got = _norm_run(p, g, segs, off)
    print('[flat] norm n=%d %s off=%d: rel err %.2e, penalty err %.2e'
          % (n, layout, off, abs(got[0] - want) / want, abs(got[1] - pen) / max(1.0, pen)))
    assert abs(got[0] - want) < 1e-5 * want
    assert abs(got[1] - pen) < 1e-5 * max(1.0, pen)


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'offset'])
@pytest.mark.parametrize('n,layout', FC.norm_cases())
def test_norm_exact_probes(n, layout, off):
    """What random data cannot show (one of n random terms moves the norm by 1/(2n)): weights of
    1.0 at K = k^2 probes -- index 0, n - 1, both sides of every trip, half-trip, chunk and segment
    boundary -- and zeros elsewhere; the gradient at a probe is 1 - 2 l2 of ITS segment (exact:
    l2 is 0 or a power of two), so that the regularised gradient g + 2 l2 w is exactly 1.0 there.
    Then norm[0] == k and norm[1] == l2 * (probes in regularised segments), exactly: a dropped or
    doubled element, or a neighbour's l2, changes the result."""
    segs = FC.layouts(n)[layout]
    pos, k = FC.probes(n, segs)
    l2 = FC.l2_vector(segs, n)
    p, g = np.zeros(n, np.float32), np.zeros(n, np.float32)
    p[pos] = 1.0
    g[pos] = np.float32(1.0) - np.float32(2.0) * l2[pos]
    got = _norm_run(p, g, segs, off)
    count = int((l2[pos] != 0).sum())
    print('[flat] norm probes n=%d %s off=%d: K=%d got %r want (%d, %r)'
          % (n, layout, off, k * k, tuple(got), k, FC.L2 * count))
    assert got[0] == float(k) and got[1] == FC.L2 * count


# ------------------------------------------------------------------------------------- Adam, SGD
LR, MU = 1e-2, 0.9


def _optim_run(kind, n, segs, clip, off, grads, tag):
    """Three steps of `kind` over `grads` from the views at `off`: p to the existing 2e-5, m / v
    (the velocity) to BOUND, the one-call form bit-equal to norm + step, the guards untouched;
    then a vetoed step (asr_optim_guard with flags [1, 0]) that changes nothing."""
    from asr_study_amd import ops
    dev = 'cuda:0'
    sd, nseg = ops.make_segments(segs, dev)
    l2vec = FC.l2_vector(segs, n).astype(np.float64)
    p0 = _base(14, n)
    p_ref = [p0.astype(np.float64)]
    opt = OO.Adam(lr=LR, clipnorm=clip) if kind == 'adam' else \
        OO.SGD(lr=LR, momentum=MU, clipnorm=clip)
    zeros = np.zeros(n, np.float32)
    P, M, V = Guarded(n, off, init=p0), Guarded(n, off, init=zeros), Guarded(n, off, init=zeros)
    P2, M2, V2 = Guarded(n, off, init=p0), Guarded(n, off, init=zeros), Guarded(n, off, init=zeros)
    norm = torch.zeros(2, dtype=torch.float64, device=dev)
    norm2 = torch.zeros_like(norm)
    worst = {}
    for step, g in enumerate(grads, 1):
        g_tot = g.astype(np.float64) + 2 * l2vec * p_ref[0]
        want_norm = np.sqrt(np.sum(g_tot ** 2))
        opt.step(p_ref, [g_tot])
        G = Guarded(n, off, init=g)
        ops.grad_norm(P.t, G.t, sd, nseg, norm)
        if kind == 'adam':
            ops.adam_step(P.t, G.t, M.t, V.t, sd, nseg, norm, clip, LR, step)
            ops.clip_adam_step(P2.t, G.t, M2.t, V2.t, sd, nseg, norm2, clip, LR, step)
        else:
            ops.sgd_step(P.t, G.t, M.t, sd, nseg, norm, clip, LR, MU)
            ops.clip_sgd_step(P2.t, G.t, M2.t, sd, nseg, norm2, clip, LR, MU)
        torch.cuda.synchronize()
        assert torch.equal(P.buf, P2.buf) and torch.equal(M.buf, M2.buf) and \
            torch.equal(V.buf, V2.buf) and torch.equal(norm, norm2)
        _same_bits(G.numpy(), g, 'grads are only read')
        nh = norm.cpu().numpy()
        assert abs(nh[0] - want_norm) <= 1e-5 * want_norm, (tag, step, nh[0], want_norm)
        refs = [('p', P, p_ref[0], 2e-5)]
        if kind == 'adam':
            refs += [('m', M, opt.m[0], BOUND), ('v', V, opt.v[0], BOUND)]
        else:
            refs += [('vel', M, opt.vel[0], BOUND)]
        for name, buf, want, bar in refs:
            e = np.abs(buf.numpy().astype(np.float64) - want).max()
            worst[name] = max(worst.get(name, 0.0), e)
            assert e < bar, (tag, step, name, e)
    print('[flat] %-40s %s' % (tag, ' '.join('%s %.2e' % kv for kv in sorted(worst.items()))))
    # the veto: norm[0] becomes -1 and the update kernels return without touching anything
    before = [b.buf.clone() for b in (P, M, V)]
    flags = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    ops.optim_guard(norm, dev, flags=flags)
    G = Guarded(n, off, init=grads[0])
    if kind == 'adam':
        ops.adam_step(P.t, G.t, M.t, V.t, sd, nseg, norm, clip, LR, len(grads) + 1)
    else:
        ops.sgd_step(P.t, G.t, M.t, sd, nseg, norm, clip, LR, MU)
    torch.cuda.synchronize()
    assert norm[0].item() == -1.0
    for b, was in zip((P, M, V), before):
        assert torch.equal(b.buf, was)
    # flags [0, 0] veto nothing
    ops.grad_norm(P.t, G.t, sd, nseg, norm)
    ops.optim_guard(norm, dev, flags=torch.zeros(2, dtype=torch.int32, device=dev))
    assert norm[0].item() > 0.0
    return nh


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'offset'])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
@pytest.mark.parametrize('n,layout', FC.update_cases('adam'))
def test_adam_and_sgd_three_steps(n, layout, kind, off):
    """clipnorm below the norm (3.0: every step is clipped once n is large; n <= 3 also sees the
    unclipped branch) and above it (1e6)."""
    assert FC.update_cases('adam') == FC.update_cases('sgd')
    segs = FC.layouts(n)[layout]
    grads = [_base(20 + s, n) for s in range(3)]
    for clip in (3.0, 1e6):
        _optim_run(kind, n, segs, clip, off, grads, '%s n=%d %s clip=%g off=%d'
                   % (kind, n, layout, clip, off))


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_clipnorm_equal_to_the_norm(kind):
    """`>=` clips.  The norm is a float32-representable value exactly: +-1 at k^2 probes and no
    regulariser (the edge layout's boundaries, l2 = 0), so norm[0] == k == clipnorm on every
    step, and the step is the oracle's (whose scale clipnorm / norm is then 1)."""
    n = FC.OPTIM_N
    segs = [(o, ln, 0.0) for o, ln, _ in FC.layouts(n)['edges']]
    pos, k = FC.probes(n, segs)
    grads = []
    for s in range(3):
        g = np.zeros(n, np.float32)
        g[pos] = np.where((pos + s) % 3 == 0, -1.0, 1.0)
        grads.append(g)
    for off in (0, 1):
        nh = _optim_run(kind, n, segs, float(k), off, grads, '%s clip == norm == %d off=%d'
                        % (kind, k, off))
        assert nh[0] == float(k)
