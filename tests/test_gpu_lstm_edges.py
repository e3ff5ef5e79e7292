"""-m gpu: the BiLSTM recurrence kernels at every template edge and launch split -- the table of
tests/lstm_cases.py through the C ABI against the float64 oracle (oracle/lstm.py).

Every call starts from sentinel-filled outputs and EVERY one of the n_pad rows is compared: the
oracle sees x = 0 in the rows beyond N, which is what the bias-only padding rows of the packed
input are, so an element a kernel did not write shows wherever it lies; dz of the padding must be
exactly 0.  Bounds (tests/test_gpu_lstm.py): h, c, gates 1e-4 absolute (scaled by max(1, max|c|)
under an unbounded `activation`, as there); every gradient slab, and h@U of the multiplicative
cell, 1e-4 * max(1, max|oracle|)."""
import functools

import numpy as np
import pytest
import torch

from tests import lstm_cases as LC
from tests.gpu_util import to_dev, report

pytestmark = pytest.mark.gpu

SENTINEL = dict(y=3.0, cell=3.0, gates=3.0, dz=5.0, uh=7.0, dwx=7.0, dmi=9.0, db_part=9.0, hl=3.0)
PROBE_N_PAD = 272        # a batch large enough that chains_per_launch is not capped by it


def _env(monkeypatch, case, **extra):
    for k, v in dict(case.env, **extra).items():
        monkeypatch.setenv(k, v)


def _run(D, mode=None, ranges=(None,), zx=None, dy=None, mask=None, absmax=True, max_dz=None):
    """Forward + BPTT of a case from sentinel-filled outputs -> dict of numpy arrays."""
    from asr_study_amd import ops
    c, T, n_pad, H = D.case, D.T, D.n_pad, D.H
    dev = 'cuda:0'
    mode = c.mode if mode is None else mode
    full = lambda shape, v: torch.full(shape, v, dtype=torch.float32, device=dev)
    zx_d, U_d = to_dev(D.zx if zx is None else zx), to_dev(D.U)
    mk = D.mask if mask is None else mask
    kw = dict(mask_u=to_dev(mk) if mk is not None else None, mode=mode,
              mi=to_dev(D.mi) if D.mi is not None else None,
              zone_c=to_dev(D.zone_c) if D.zone_c is not None else None,
              zone_h=to_dev(D.zone_h) if D.zone_h is not None else None, act=D.act)
    use_mi = D.mi is not None
    y = full((T, n_pad, 2 * H), SENTINEL['y'])
    cell = full((T, n_pad, 2, H), SENTINEL['cell'])
    gates = full((T, n_pad, 2, 4 * H), SENTINEL['gates'])
    kw['uh'] = full((T, n_pad, 2, 4 * H), SENTINEL['uh']) if use_mi else None
    for r in ranges:
        ws = ops.lstm_seq_fwd(zx_d, U_d, y, cell, gates, T, n_pad, H, steps=r,
                              n_valid=c.get('n_valid', 0), units=c.get('units', 0), **kw)
    ops.lstm_status(ws)
    out = dict(y=y.cpu().numpy(), cell=cell.cpu().numpy(), gates=gates.cpu().numpy())
    if use_mi:
        out['uh'] = kw['uh'].cpu().numpy()
    if not c.get('bwd', True):
        return out
    planes = bool(c.get('planes'))
    dz = None if planes else full((T, n_pad, 2, 4 * H), SENTINEL['dz'])
    dbp = full((n_pad // 16, 2, 4 * H), SENTINEL['db_part'])
    am = torch.zeros(1, device=dev) if absmax else None
    dwx = full((T, n_pad, 2, 4 * H), SENTINEL['dwx']) if use_mi else None
    dmi = full((n_pad // 16, 2, 4, 4 * H), SENTINEL['dmi']) if use_mi else None
    pl = bound = None
    if planes:
        # the bound is handed in BEFORE the pass: eight times the oracle's maximum
        pl = ops.HlPlanes(T * n_pad, 8 * H, dev)
        pl.hl.fill_(SENTINEL['hl'])
        bound = full((1,), 8.0 * max_dz)
    for r in ranges:
        ws = ops.lstm_seq_bwd(to_dev(D.dy if dy is None else dy), U_d, cell, gates, dz, T, n_pad, H,
                              steps=r, dz_absmax=am, db_part=dbp, wx=zx_d if use_mi else None,
                              dwx=dwx, dmi=dmi, compact=bool(c.get('compact')), dz_planes=pl,
                              dz_bound=bound, **kw)
    ops.lstm_status(ws)
    if planes:
        out['hl'] = pl.hl.cpu().numpy().reshape(T, n_pad, 8 * H // 16, 2, 16)
        v = out['hl'].astype(np.float64)
        out['dz'] = ((v[:, :, :, 0] + v[:, :, :, 1]) / float(pl.scale.item())).reshape(T, n_pad, 2, 4 * H)
    else:
        out['dz'] = dz.cpu().numpy()
    out['db_part'] = dbp.cpu().numpy()
    if absmax:
        out['absmax'] = float(am.item())
    if use_mi:
        out['dwx'], out['dmi'] = dwx.cpu().numpy(), dmi.cpu().numpy()
    return out


def _check(D, got, tag):
    """All n_pad rows of every output against the oracle; prints and returns the maxima."""
    w, c, N = D.want, D.case, D.N
    errs = {}
    sc = max(1.0, np.abs(w['cell']).max()) if D.act != 'tanh' else 1.0
    for name in ('y', 'cell', 'gates'):
        errs[name] = report('%s %s' % (name, tag), got[name], w[name])
        assert errs[name] < 1e-4 * (1.0 if name == 'gates' else sc), (name, tag)
    if 'uh' in got:
        errs['uh'] = report('uh %s' % tag, got['uh'], w['uh'])
        assert errs['uh'] < 1e-4 * max(1.0, np.abs(w['uh']).max()), tag
    if 'dz' not in got:
        return errs
    names = ['dz', 'db_part'] + (['dwx'] if 'dwx' in got else [])
    for name in names:
        scale = max(1.0, np.abs(w[name]).max())
        errs[name] = report('%s %s' % (name, tag), got[name], w[name]) / scale
        assert errs[name] < 1e-4, (name, tag)
    if 'dmi' in got:
        sums = got['dmi'].astype(np.float64).sum(axis=0)
        for k in range(4):
            scale = max(1.0, np.abs(w['dmi'][:, k]).max())
            errs['dmi%d' % k] = report('dmi[%d] %s' % (k, tag), sums[:, k], w['dmi'][:, k]) / scale
            assert errs['dmi%d' % k] < 1e-4, (k, tag)
    # padding rows received no upstream gradient: exactly zero gate gradients
    assert not got['dz'][:, N:].any(), tag
    if 'dwx' in got:
        assert not got['dwx'][:, N:].any(), tag
    if 'absmax' in got:
        zmax = max(np.abs(w[n]).max() for n in names if n != 'db_part')
        assert abs(got['absmax'] - zmax) < 1e-4 * max(1.0, zmax), tag
        if 'hl' not in got:
            assert got['absmax'] == max(np.abs(got[n]).max() for n in names if n != 'db_part'), tag
    print('[lstm-edges] %s %s worst %.3e' % (c.group, c.name, max(errs.values())))
    return errs


def _same_bits(a, b, names, what):
    for name in names:
        bad = np.argwhere(a[name] != b[name])
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist(), bad[-1].tolist())


def _plan_p(plan):
    return plan['blocks'] // max(1, plan['chains_per_launch'])


# --------------------------------------------------------------------------- a, b
@pytest.mark.parametrize('case', LC.group('edges'), ids=repr)
def test_template_edges_plain_cell(case, monkeypatch):
    """lstm_fwd_kernel_h<4|8|16> / lstm_bwd_kernel_h<1|2|4|8> on both sides of every width at
    which make_plan switches templates, ragged last workgroups (H = 20: four units; 300: P = 19,
    ten of sixteen K slabs) and a one-workgroup chain (H = 4); one batch tile with eleven padding
    rows and two tiles; T = 9: a full tag period of the two-slot hand-off."""
    from asr_study_amd import ops
    _env(monkeypatch, case)
    D = LC.build(case.name)
    t = LC.template(case.H)
    pf, pb = ops.lstm_plan(D.T, D.n_pad, D.H, 0), ops.lstm_plan(D.T, D.n_pad, D.H, 1)
    assert pb['k_per_lane'] == 16 * t['TPW'], pb          # ... or the case ran another template
    assert _plan_p(pf) == t['P'] and _plan_p(pb) == t['P']
    _check(D, _run(D), case.name)


@pytest.mark.parametrize('case', LC.group('variants'), ids=repr)
def test_variant_cells_in_every_template(case, monkeypatch):
    """lstm_fwd_kernel_hv<4|8|16> / lstm_bwd_kernel_hv<1|2|4|8>: multiplicative integration,
    zoneout and `activation` beyond H = 256 (never launched by another test) and at ragged widths:
    h, c, gates, h@U, d(h@U), d(x@W), the MI parameter-gradient sums and the bias partials."""
    from asr_study_amd import ops
    _env(monkeypatch, case)
    D = LC.build(case.name)
    t = LC.template(case.H)
    pb = ops.lstm_plan(D.T, D.n_pad, D.H, 1, activation=D.act)
    assert pb['k_per_lane'] == 16 * t['TPW'] and _plan_p(pb) == t['P'], pb
    _check(D, _run(D), case.name)


# --------------------------------------------------------------------------- c
@pytest.mark.parametrize('case', LC.group('ends'), ids=repr)
def test_sequence_ends(case, monkeypatch):
    """T = 1, 2, 3 as whole calls: the peeled step 0, BPTT's guard of the last step, an exchange
    buffer in which one parity slot is written at most once -- on every kernel family; T = 3 also
    as three one-step slices, bit for bit."""
    from asr_study_amd import ops
    _env(monkeypatch, case)
    D = LC.build(case.name)
    if case.get('compact'):
        assert _plan_p(ops.lstm_plan(D.T, D.n_pad, D.H, 1, compact=True)) == D.H // 32
    if case.get('units'):
        assert _plan_p(ops.lstm_plan(D.T, D.n_pad, D.H, 0, units=8)) == D.H // 8
    got = _run(D)
    if case.get('n_valid'):
        # the single-utterance kernel: row 0 to its own bound (1e-5), the others untouched
        for name in ('y', 'cell', 'gates'):
            assert report('n1 %s %s' % (name, case.name), got[name][:, :1], D.want[name][:, :1]) < 1e-5
            assert np.all(got[name][:, 1:] == SENTINEL[name]), name
    else:
        _check(D, got, case.name)
    if D.T == 3:
        parts = _run(D, ranges=[(0, 1), (1, 1), (2, 1)])
        names = [n for n in ('y', 'cell', 'gates', 'uh', 'dz', 'dwx') if n in got]
        _same_bits(parts, got, names, 'sliced != whole')
        if 'absmax' in got:
            assert parts['absmax'] == got['absmax']


# --------------------------------------------------------------------------- d
@pytest.mark.parametrize('case', LC.group('stepwise'), ids=repr)
def test_stepwise_mode(case, monkeypatch):
    """mode 1 (one launch per step: what the engine falls back to after a timeout) at a ragged
    narrow width, a ragged wide one and H = 512, against the oracle and -- `identical arithmetic`,
    csrc/lstm.hip -- bit for bit against the persistent run of the same instantiation."""
    _env(monkeypatch, case)
    D = LC.build(case.name)
    got = _run(D, mode=1)
    _check(D, got, case.name)
    monkeypatch.setenv('ASR_LSTM_GENERIC', '1')       # (H = 512: persistent on the any-H kernels)
    pers = _run(D, mode=0)
    _check(D, pers, case.name + ' persistent')
    _same_bits(got, pers, ('y', 'cell', 'gates', 'dz'), 'stepwise != persistent')
    assert got['absmax'] == pers['absmax']


# --------------------------------------------------------------------------- e
@functools.lru_cache(maxsize=None)
def _split_shape(name, cpl):
    n_pad = LC.split_n_pad(cpl)
    return LC.build(name, n_pad - 3, n_pad)


@pytest.mark.parametrize('case', LC.group('split'), ids=repr)
def test_launch_split(case, monkeypatch):
    """chains > chains_per_launch: run() cuts the chains into launches and hands chain_begin / nch
    to the kernel, which index the exchange buffer, the XCC table, dc_state, db_part and the chain
    slots with them.  The batch follows from the plan of this machine; every row against the
    oracle, db_part per tile, max|dz|; and the same problem with the batch tiles rotated by one
    (the tiles of the last launch move into the first) must give every sample the same bits."""
    from asr_study_amd import ops
    _env(monkeypatch, case)
    H, T = case.H, case.T
    act = case.get('act') or 'tanh'
    kw = dict(mode=case.mode, compact=bool(case.get('compact')), units=case.get('units', 0),
              activation=act)
    cpl_f = ops.lstm_plan(T, PROBE_N_PAD, H, 0, **kw)['chains_per_launch']
    cpl_b = ops.lstm_plan(T, PROBE_N_PAD, H, 1, **kw)['chains_per_launch']
    D = _split_shape(case.name, max(cpl_f, cpl_b))
    n_pad = D.n_pad
    pf, pb = ops.lstm_plan(T, n_pad, H, 0, **kw), ops.lstm_plan(T, n_pad, H, 1, **kw)
    print('split', case.name, 'n_pad', n_pad, 'fwd', pf, 'bwd', pb)
    assert 2 * n_pad // 16 > pf['chains_per_launch'] and 2 * n_pad // 16 > pb['chains_per_launch']
    assert n_pad <= PROBE_N_PAD
    assert (_plan_p(pf), _plan_p(pb)) == LC.split_plan_p(case)
    if case.get('planes'):
        assert ops.lstm_dz_hl_supported(T, n_pad, H)
    max_dz = float(np.abs(D.want['dz']).max())
    got = _run(D, max_dz=max_dz)
    _check(D, got, case.name)
    # placement independence: tile b -> b + 1 (mod NB)
    roll = lambda a, ax: None if a is None else np.roll(a, 16, axis=ax)
    moved = _run(D, zx=roll(D.zx, 1), dy=roll(D.dy, 1), mask=roll(D.mask, 1), max_dz=max_dz)
    back = {k: np.roll(v, -16, axis=1) for k, v in moved.items()
            if k in ('y', 'cell', 'gates', 'uh', 'dz', 'dwx', 'hl')}
    _same_bits(back, got, sorted(back), 'rotated tiles != original')
    assert moved['absmax'] == got['absmax']


# --------------------------------------------------------------------------- f
@functools.lru_cache(maxsize=None)
def _isolation_runs(name):
    D = LC.build(name)
    base = _run(D, absmax=False)
    zx, dy = D.zx.copy(), D.dy.copy()
    zx[:, 16:32] = np.nan
    dy[:, 16:32] = np.nan
    return D, base, _run(D, zx=zx, dy=dy, absmax=False)      # (no dz_absmax: a global maximum)


@pytest.mark.parametrize('case', LC.group('isolation'), ids=repr)
def test_tiles_are_isolated(case):
    """Three batch tiles, the middle one's zx and dy all NaN: the other two tiles' outputs are,
    bit for bit, those of the run in which that tile holds ordinary data."""
    D, base, poisoned = _isolation_runs(case.name)
    _check(D, base, case.name)
    for rows in (slice(0, 16), slice(32, 48)):
        for name in ('y', 'cell', 'gates', 'dz'):
            assert np.array_equal(poisoned[name][:, rows], base[name][:, rows]), (name, rows)
    for tile in (0, 2):
        assert np.array_equal(poisoned['db_part'][tile], base['db_part'][tile]), tile


@pytest.mark.parametrize('case', LC.group('isolation'), ids=repr)
def test_a_nan_tile_comes_out_as_nan(case):
    """... and the NaN tile's own outputs are NaN, not the sentinel and not a finite number:
    v_min_f32 / v_max_f32 return the operand that is not a NaN, so the clamps of the gate
    activations alone would hand on (0, 0, -1, 0), c = 0, h = 0 -- the forward kernels test the
    pre-activations themselves (nan_lanes / poison, lstm_common.h)."""
    D, base, poisoned = _isolation_runs(case.name)
    share = {}
    for name in ('y', 'cell', 'gates', 'dz'):
        mid = poisoned[name][:, 16:32]
        assert not np.any(mid == SENTINEL[name]), name
        share[name] = float(np.isnan(mid).mean())
    print('[lstm-edges] NaN share of the poisoned tile %s: %s' % (case.name, share))
    assert all(v == 1.0 for v in share.values()), share
