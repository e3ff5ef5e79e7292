"""GPU checks of the transducer kernels (csrc/rnnt.hip) against the float64 oracle
tests/rnnt_oracle.py.  Bounds (the project's CTC and full-size parity bound): loss rtol 1e-4,
every gradient tensor max |err| <= 1e-4 max |oracle gradient of that tensor|.  Every call runs
with rows n >= N of its inputs set to NaN, its outputs preset to a sentinel and its workspace
filled with NaN bit patterns, so a row that leaks, an element that is not written and a workspace
word that is read before it is written all show."""
import numpy as np
import pytest
import torch

from tests import rnnt_oracle as RO

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
NAMES = ('d_enc', 'd_pred', 'dW_out', 'db_out')


def _case(seed, T, l_max, N, n_pad, J, Cc, seq_len=None, label_len=None, w_scale=None):
    rs = np.random.RandomState(seed)
    Jp = (J + 3) // 4 * 4
    enc = rs.randn(T, n_pad, Jp).astype(np.float32)
    pred = rs.randn(l_max + 1, n_pad, Jp).astype(np.float32)
    w_scale = 1.0 / np.sqrt(J) if w_scale is None else w_scale
    W = (rs.randn(J, Cc) * w_scale).astype(np.float32)
    b = (rs.randn(Cc) * 0.3).astype(np.float32)
    labels = rs.randint(0, Cc - 1, (N, l_max + 1))[:, :l_max].astype(np.int32)
    seq_len = np.full(N, T) if seq_len is None else np.asarray(seq_len)
    label_len = np.full(N, l_max) if label_len is None else np.asarray(label_len)
    enc[:, N:] = np.nan
    pred[:, N:] = np.nan
    return dict(enc=enc, pred=pred, W=W, b=b, labels=labels, seq_len=seq_len.astype(np.int32),
                label_len=label_len.astype(np.int32), N=N, J=J)


def _run(c, grads=True, grad_scale=1.0):
    """The kernel on a case -> loss (N) and the four gradients (or None) as NumPy arrays."""
    from asr_study_amd import _lib, ops
    dev = 'cuda'
    enc, pred = torch.from_numpy(c['enc']).to(dev), torch.from_numpy(c['pred']).to(dev)
    W, b = torch.from_numpy(c['W']).to(dev), torch.from_numpy(c['b']).to(dev)
    labels = torch.from_numpy(np.ascontiguousarray(c['labels'])).to(dev)
    ll, sl = torch.from_numpy(c['label_len']).to(dev), torch.from_numpy(c['seq_len']).to(dev)
    T, n_pad, _ = enc.shape
    nbytes = _lib.load().asr_rnnt_workspace_bytes(T, pred.shape[0], c['N'], n_pad, c['J'],
                                                  b.numel())
    assert nbytes > 0
    ops.WS.get('rnnt', nbytes, enc.device).fill_(255)        # every float and double a NaN
    g = None
    if grads:
        g = [torch.full_like(enc, SENTINEL), torch.full_like(pred, SENTINEL),
             torch.full_like(W, SENTINEL), torch.full_like(b, SENTINEL)]
    loss = torch.full((c['N'],), SENTINEL, dtype=torch.float32, device=dev)
    ops.rnnt_loss_grad(enc, pred, W, b, labels, ll, sl, c['N'], c['J'], grads=g,
                       grad_scale=grad_scale, loss=loss)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), None if g is None else [t.cpu().numpy() for t in g]


_ORACLE = {}


def _oracle(key, c, grad_scale=1.0):
    """Computed once per case and shared; never modified."""
    if key not in _ORACLE:
        _ORACLE[key] = RO.loss_and_grads(c['enc'], c['pred'], c['W'], c['b'], c['labels'],
                                         c['label_len'], c['seq_len'], c['N'], grad_scale)
    return _ORACLE[key]


def _compare(tag, c, got_loss, got, want):
    wl = want[0]
    lerr = np.abs(got_loss - wl) / np.abs(wl)
    worst = 0.0
    for name, a, w in zip(NAMES, got, want[1:]):
        assert np.isfinite(a).all(), (tag, name)
        scale = np.abs(w).max()
        err = np.abs(a - w).max() / scale
        worst = max(worst, err)
        print('[rnnt] %s %s: max|err| %.3e of max|grad| %.3e' % (tag, name, err, scale))
    print('[rnnt] %s loss rel err %.3e, worst gradient %.3e (bound 1e-4)' % (tag, lerr.max(), worst))
    assert lerr.max() <= 1e-4, (tag, lerr)
    for name, a, w in zip(NAMES, got, want[1:]):
        assert np.abs(a - w).max() <= 1e-4 * np.abs(w).max(), (tag, name)
    _check_zero_regions(tag, c, got)


def _check_zero_regions(tag, c, got):
    """d_enc is 0 at frames t >= T_n, d_pred at positions u > U_n, both in rows n >= N and in the
    padding columns: entry by entry (a sentinel or a NaN that leaked is not 0)."""
    d_enc, d_pred = got[0], got[1]
    T, U1, J, N = d_enc.shape[0], d_pred.shape[0], c['J'], c['N']
    Tn, Un = RO.clamp_lens(c['seq_len'], c['label_len'], T, U1 - 1)
    for n in range(d_enc.shape[1]):
        t_n, u_n = (Tn[n], Un[n] + 1) if n < N else (0, 0)
        assert not d_enc[t_n:, n].any(), (tag, 'd_enc', n)
        assert not d_pred[u_n:, n].any(), (tag, 'd_pred', n)
    assert not d_enc[:, :, J:].any() and not d_pred[:, :, J:].any(), tag


def _check(tag, c):
    loss, g = _run(c)
    _compare(tag, c, loss, g, _oracle(tag, c))
    return loss, g


# ------------------------------------------------------------------ lattice shapes
@pytest.mark.parametrize('T,U', [(1, 0), (1, 2), (5, 0), (2, 5), (7, 3)])
def test_lattice_edges(T, U):
    c = _case(100 + 10 * T + U, T, U, 1, 16, 12, 5)
    loss, _ = _check('edge T%d U%d' % (T, U), c)
    if (T, U) == (1, 0):                                     # the loss is -lp_blank(0, 0)
        _, z = RO.joint(np.float64(c['enc'][:1, 0, :12]), np.float64(c['pred'][:1, 0, :12]),
                        np.float64(c['W']), np.float64(c['b']))
        assert abs(loss[0] + RO.log_softmax(z)[0, 0, 4]) <= 1e-4 * abs(loss[0])


@pytest.mark.parametrize('U1', [63, 64, 65, 128, 129, 256])
def test_wave_boundaries(U1):
    """One, two and four waves per chain, and the lanes on both sides of every wave boundary; the
    second utterance ends in the middle of the label axis."""
    c = _case(U1, 4, U1 - 1, 2, 16, 8, 6, seq_len=(4, 3), label_len=(U1 - 1, U1 // 2))
    _check('U1 %d' % U1, c)


def test_ragged_batch():
    c = _case(7, 9, 6, 3, 16, 36, 29, seq_len=(9, 1, 5), label_len=(6, 0, 3))
    _check('ragged', c)


def test_second_batch_tile():
    rs = np.random.RandomState(17)
    c = _case(17, 5, 3, 17, 32, 8, 6, seq_len=rs.randint(1, 6, 17), label_len=rs.randint(0, 4, 17))
    _check('N17', c)


@pytest.mark.parametrize('J', [4, 36, 512])
@pytest.mark.parametrize('Cc', [2, 29, 64])
def test_widths(J, Cc):
    c = _case(J + Cc, 3, 2, 2, 16, J, Cc, seq_len=(3, 2), label_len=(2, 1))
    _check('J%d C%d' % (J, Cc), c)


def test_tile_edges_in_both_lattice_axes():
    """More than one 16 x 16 cell tile along t and along u, neither a multiple of 16."""
    c = _case(33, 35, 18, 2, 16, 20, 7, seq_len=(35, 17), label_len=(18, 16))
    _check('tiles', c)


def test_prescribed_logits_isolate_the_lattice():
    """J = C, pred = 0, W_out = s I, b_out = 0, enc = atanh(x / s): the logits of cell (t, u) are
    x(t, :) exactly, and d_enc(t, j) = sum_u dz(t, u, j) s (1 - (x / s)^2)."""
    rs = np.random.RandomState(11)
    T, U, Cc, s = 10, 4, 5, 4.0
    x = rs.uniform(-3.0, 3.0, (T, Cc))
    y = [int(v) for v in rs.randint(0, Cc - 1, U)]
    c = _case(11, T, U, 1, 16, Cc, Cc)
    c['enc'][:, 0, :Cc] = np.arctanh(x / s)
    c['enc'][:, 0, Cc:] = 0.0
    c['pred'][:, 0] = 0.0
    c['W'][:] = s * np.eye(Cc)
    c['b'][:] = 0.0
    c['labels'][0] = y
    loss, g = _run(c)
    lp = RO.log_softmax(np.repeat(x[:, None, :], U + 1, axis=1))
    want_loss, _, _, dz = RO.lattice(lp, y)
    want = dz.sum(axis=1) * s * (1.0 - (x / s) ** 2)
    err = np.abs(g[0][:, 0, :Cc] - want).max() / np.abs(want).max()
    print('[rnnt] prescribed logits: loss rel err %.3e, d_enc %.3e'
          % (abs(loss[0] - want_loss) / want_loss, err))
    assert abs(loss[0] - want_loss) <= 1e-4 * want_loss
    assert err <= 1e-4


def test_precision_on_a_long_lattice():
    """N = 2, T = 300, U = 80, C = 29, J = 32, logits of standard deviation about 3: where a plain
    float32 log-space recursion measured 6e-4.  Measured with the re-centred chains: loss 3.9e-8,
    d_enc 2.4e-5, d_pred 5.2e-5, dW_out 3.7e-5, db_out 3.0e-5 of each tensor's maximum."""
    c = _case(300, 300, 80, 2, 16, 32, 29, seq_len=(300, 251), label_len=(80, 67),
              w_scale=3.0 / (0.8 * np.sqrt(32)))
    _check('T300 U80', c)


# ------------------------------------------------------------------ call semantics
@pytest.fixture(scope='module')
def ragged():
    c = _case(7, 9, 6, 3, 16, 36, 29, seq_len=(9, 1, 5), label_len=(6, 0, 3))
    return c, _run(c)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_loss_only_call_gives_the_same_bits(ragged):
    c, (loss, _) = ragged
    only, g = _run(c, grads=False)
    assert g is None and np.array_equal(_bits(only), _bits(loss))
    assert np.abs(only - _oracle('ragged', c)[0]).max() <= 1e-4 * np.abs(only).max()


def test_repeated_call_gives_the_same_bits(ragged):
    c, (loss, g) = ragged
    loss2, g2 = _run(c)
    assert np.array_equal(_bits(loss2), _bits(loss))
    for name, a, a2 in zip(NAMES, g, g2):
        assert np.array_equal(_bits(a), _bits(a2)), name


def test_grad_scale_scales_every_gradient_and_not_the_loss(ragged):
    c, (loss, g) = ragged
    loss4, g4 = _run(c, grad_scale=0.25)                     # a power of two: exact
    assert np.array_equal(_bits(loss4), _bits(loss))
    for name, a, a4 in zip(NAMES, g, g4):
        assert np.abs(a).max() > 0
        assert np.array_equal(_bits(a4), _bits(a * np.float32(0.25))), name
    _compare('scaled', c, loss4, g4, _oracle('ragged/4', c, 0.25))


# ------------------------------------------------------------------ helpers and the greedy step
@pytest.mark.parametrize('N,n_pad', [(3, 16), (17, 32)])
def test_onehot_rows_and_rows_select(N, n_pad):
    from asr_study_amd import ops
    rs = np.random.RandomState(N)
    l_max, width, ld = 5, 7, 8
    labels = rs.randint(0, width, (N, l_max)).astype(np.int32)
    ll = rs.randint(0, l_max + 1, N).astype(np.int32)
    ll[0], ll[1] = l_max, 0
    out = torch.full((l_max + 1, n_pad, ld), SENTINEL, device='cuda')
    ops.onehot_rows(torch.from_numpy(labels).cuda(), torch.from_numpy(ll).cuda(), N, n_pad,
                    width, out=out, ld=ld)
    assert np.array_equal(out.cpu().numpy(), RO.onehot_rows(labels, ll, N, n_pad, width, ld))
    a = rs.randn(n_pad, 12).astype(np.float32)
    b = rs.randn(n_pad, 12).astype(np.float32)
    mask = rs.randint(0, 2, N).astype(np.int32)
    mask[0], mask[1] = 1, 0
    want = RO.rows_select(mask, a, b, N)
    ad, bd, md = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(mask).cuda()
    got = ops.rows_select(md, ad, bd, torch.full_like(ad, SENTINEL), N)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    ops.rows_select(md, ad, bd, bd, N)                       # in place on b
    assert np.array_equal(_bits(bd.cpu().numpy()), _bits(want))


@pytest.mark.parametrize('N,n_pad,max_symbols', [(3, 16, 1), (3, 16, 10), (17, 32, 2)])
def test_greedy_step_follows_its_python_model(N, n_pad, max_symbols):
    """A dozen iterations with a prescribed predictor output per iteration; every state word is
    compared after every call.  Classes 0 and 1 have identical weights and the largest bias, so
    the arg-max meets exact ties (the first maximum wins); one utterance has no frames, another
    ends after one."""
    from asr_study_amd import ops
    rs = np.random.RandomState(N + max_symbols)
    T, J, Cc, iters = 4, 10, 6, 12
    cap = T * max_symbols
    enc = rs.randn(T, n_pad, 12).astype(np.float32)
    enc[:, N:] = np.nan
    W = rs.randn(J, Cc).astype(np.float32)
    b = (rs.randn(Cc) * 0.3).astype(np.float32)
    W[:, 1] = W[:, 0]
    b[0] = b[1] = 0.4
    seq_len = rs.randint(1, T + 1, N).astype(np.int32)
    seq_len[0], seq_len[1], seq_len[2] = T, 0, 1
    st = dict(t_ptr=np.zeros(N, np.int32), n_sym=np.zeros(N, np.int32),
              decoded_len=np.zeros(N, np.int32), decoded=np.full((N, cap), -1, np.int32))
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in st.items()}
    advance = torch.full((N,), -7, dtype=torch.int32, device='cuda')
    active = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    x_next = torch.full((n_pad, Cc - 1), SENTINEL, device='cuda')
    encd, Wd, bd = torch.from_numpy(enc).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda()
    sld = torch.from_numpy(seq_len).cuda()
    ties = 0
    for it in range(iters):
        g = rs.randn(n_pad, 12).astype(np.float32)
        g[N:] = np.nan
        want_adv, want_x, want_active = RO.greedy_step(enc, g, W, b, seq_len, N, st, max_symbols,
                                                       cap)
        ops.rnnt_greedy_step(encd, torch.from_numpy(g).cuda(), Wd, bd, sld, N, J, dev['t_ptr'],
                             dev['n_sym'], dev['decoded'], dev['decoded_len'], advance, x_next,
                             active, max_symbols=max_symbols)
        torch.cuda.synchronize()
        for k in st:
            assert np.array_equal(dev[k].cpu().numpy(), st[k]), (it, k)
        assert np.array_equal(advance.cpu().numpy(), want_adv), it
        assert np.array_equal(x_next.cpu().numpy()[:N], want_x), it
        assert int(active.item()) == want_active, it
        ties += int(want_x[:, 0].sum())
        assert not want_x[:, 1].any()                        # class 1 never wins its tie
    assert ties > 0 and st['decoded_len'].max() > 0
    assert st['t_ptr'][1] == 0 and st['decoded_len'][1] == 0 and st['t_ptr'][2] <= 1
    if max_symbols == 1:                                     # at most one label per frame
        assert (st['decoded_len'] <= np.minimum(st['t_ptr'] + 1, seq_len)).all()
