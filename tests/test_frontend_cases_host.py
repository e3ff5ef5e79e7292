"""tests/frontend_cases.py is sharp: every length has the frame count it is in the table for, the
strided counts and the column blockings are the ones the notes claim, the 'gap' signals reach both
eps substitutions, and the oracle is finite over the whole table.  No GPU."""
import numpy as np
import pytest

from oracle import frontend as OF
from oracle import gen_golden
from tests import frontend_cases as FC

_WANT = {}


def _want(name, case):
    if (name, case) not in _WANT:
        _WANT[name, case] = FC.want(name, FC.signal(name, case))
    return _WANT[name, case]


def test_tables_agree():
    assert tuple(gen_golden.EDGE_CONFIGS) == FC.EDGE_CONFIGS
    assert set(FC.FULL_LADDER + FC.SIGNAL_CONFIGS + FC.BATCH_CONFIGS) <= set(FC.CONFIGS)
    assert set(FC.SHARED_DELTA_CONFIGS) <= set(FC.BATCH_CONFIGS)
    for raw in ('mfcc39', 'lfb41_d_dd_s3c1', 'mfcc39_s2c2'):
        kw = dict(FC.CONFIGS[raw + '_raw'].kw)
        assert kw.pop('mean_norm') is False and kw.pop('var_norm') is False
        assert kw == FC.CONFIGS[raw].kw and FC.is_raw(raw + '_raw') and not FC.is_raw(raw)


@pytest.mark.parametrize('name', list(FC.CONFIGS))
def test_lengths_give_the_intended_frame_counts(name):
    L, S = FC.framing(name)
    assert 0 < L <= FC.NFFT and S > 0
    for T in FC.LADDER_T + FC.STRIDE_T[2] + FC.STRIDE_T[3]:
        n = FC.full_len(T, L, S)
        assert OF.num_frames(n, L, S) == T and OF.num_frames(n + 1, L, S) == T + 1
        assert T == 1 or OF.num_frames(n - 1, L, S) == T
    assert OF.num_frames(2, L, S) == 1 and OF.num_frames(L - 1, L, S) == 1
    for case in FC.cases(name):
        assert OF.num_frames(case.n, L, S) == case.T and case.n >= 2
        assert len(FC.signal(name, case)) == case.n


@pytest.mark.parametrize('name', list(FC.CONFIGS))
def test_coverage_floor(name):
    c = FC.CONFIGS[name]
    L, S = FC.framing(name)
    cs = FC.cases(name)
    assert len(set(cs)) == len(cs)
    Ts = set(case.T for case in cs)
    plus_one = [case for case in cs if case.T > 1 and case.n == FC.full_len(case.T - 1, L, S) + 1]
    context = c.kw.get('num_context', 0) > 0 and not FC.is_raw(name)
    if name in FC.FULL_LADDER:
        for T in FC.LADDER_T:
            assert FC.Case(FC.full_len(T, L, S), T, 'noise') in cs
            assert FC.Case(FC.full_len(T, L, S) + 1, T + 1, 'noise') in cs
        assert FC.Case(2, 1, 'noise') in cs and FC.Case(L - 1, 1, 'noise') in cs
    elif context:
        assert min(Ts) == FC.MIN_CONTEXT_T        # (why: the docstring of FC.cases)
        assert Ts & {16, 17} and max(Ts) >= 65 and plus_one
    else:
        assert Ts & {2, 3, 4, 5} and Ts & {15, 16, 17} and max(Ts) >= 65 and plus_one
        assert {3, 4, 5} <= Ts                    # the delta clamps meet and part
    if name == 'mfcc_nomean':
        assert min(Ts) == 2
    stride = c.kw.get('stride', 1)
    if stride > 1:
        # both sides of every point at which a row walker gains a trip
        hit = set(FC.strided(T, stride) for T in Ts)
        assert set(FC.WALKER_EDGES) <= hit, sorted(hit)
        for edge in (64, 128):
            assert {edge * stride - stride + 1, edge * stride, edge * stride + 1} <= Ts
    if name in FC.SIGNAL_CONFIGS:
        for kind in FC.SIGNAL_KINDS:
            assert set(FC.SIGNAL_T) <= set(case.T for case in cs if case.kind == kind)
    else:
        assert all(case.kind == 'noise' for case in cs)


def test_walker_edges_at_stride_one():
    """Ts on both sides of the second trip of the 64 walkers of fe_finalize_kernel<16> (lfb80)
    and of the 128 of <8> (mfcc39)."""
    assert FC.walkers(80) == 64 and FC.walkers(39) == 128 and FC.walkers(63) == 128
    assert set(FC.WALKER_EDGES) <= set(FC.LADDER_T)
    assert {4, 5, 15, 16, 17, 31, 32, 33} <= set(FC.LADDER_T)      # waves and workgroups of frames
    assert FC.FRAMES_PER_BLOCK == 16


def _f_out(c):
    """Output width from the kwargs, as Feature.num_feats of the reference counts it."""
    kw = c.kw
    if c.cls == 'MFCC':
        base = kw.get('num_cep', 13)
        d, dd = kw.get('d', True), kw.get('dd', True)
    else:
        base = kw.get('num_filt', 40) + bool(kw.get('append_energy', False))
        d, dd = kw.get('d', False), kw.get('dd', False)
    return base * (1 + bool(d) + bool(d and dd)) * (2 * kw.get('num_context', 0) + 1)


@pytest.mark.parametrize('name', list(FC.CONFIGS))
def test_column_blocking_is_the_one_in_the_table(name):
    c = FC.CONFIGS[name]
    assert _f_out(c) == c.f_out
    assert FC.cx_of(c.f_out) == c.cx and FC.last_block(c.f_out) == c.last
    assert _want(name, FC.cases(name)[-1]).shape[1] == c.f_out
    assert c.kw.get('num_filt', 40) <= FC.MEL_LIMIT


def test_the_widths_the_notes_name():
    C = FC.CONFIGS
    assert C['lfb21_d_dd'].f_out == FC.CX_SWITCH - 1 and C['lfb64'].f_out == FC.CX_SWITCH
    assert C['lfb41_d_dd_s3c1'].f_out == 23 * 16 + 1 and C['mfcc39_s2c2'].f_out == 12 * 16 + 3
    assert C['mfcc39'].f_out == 4 * 8 + 7
    assert C['lfb64'].kw['num_filt'] == FC.MEL_LANES and C['lfb65'].kw['num_filt'] == FC.MEL_LANES + 1
    assert C['lfb128_full'].kw['num_filt'] == FC.MEL_LIMIT
    # lfb21_d_dd: delta-delta columns 42..62 read delta columns 21..41; with 8 columns a block
    # some pair lies in two workgroups (the same for the wide strided configurations)
    for name in FC.SHARED_DELTA_CONFIGS:
        c = C[name]
        ffull = c.f_out // (2 * c.kw.get('num_context', 0) + 1)
        fb = ffull // 3
        assert any((col % ffull) >= 2 * fb and (col // c.cx) != ((col - fb) // c.cx)
                   for col in range(c.f_out)), name
    # top edge of the full-band bank is bin 256; the 80-filter bank has the empty filters 1 and 7
    b = OF.mel_bins(128, 512, 16e3, 0, 8000)
    assert b[-1] == 256 and b[0] == 0
    fb80 = OF.get_filterbanks(80)
    assert np.where(fb80.sum(1) == 0)[0].tolist() == [1, 7]


@pytest.mark.parametrize('name', FC.SIGNAL_CONFIGS)
def test_gap_signals_reach_both_eps_substitutions(name):
    L, S = FC.framing(name)
    kw = {k: v for k, v in FC.CONFIGS[name].kw.items() if k in OF._FB_KEYS}
    eps64 = np.finfo(float).eps
    n_gap = 0
    for case in FC.cases(name):
        if case.kind != 'gap':
            continue
        n_gap += 1
        x = FC.signal(name, case)
        z0, zl = FC.gap_span(L, S)
        assert z0 % S and not x[z0:z0 + zl].any() and x[z0 - 1] != 0 and x[z0 + zl] != 0
        zf = FC.zero_frames(x, L, S)
        assert len(zf) >= 3 and zf[0] > 0 and zf[-1] < case.T - 1, zf
        feat, energy = OF.fbank(x, **kw)
        assert np.all(np.log(energy[zf] + 1e-8) == np.log(eps64 + 1e-8))      # esum == 0 -> eps
        assert np.all(feat[zf] == eps64)                                      # acc == 0 -> eps
        others = [f for f in range(case.T) if f not in zf]
        assert np.all(energy[others] > 1e-6)
        if name == 'mfcc39':
            raw = OF.mfcc_raw(x)
            assert np.all(raw[zf, 0] == np.log(eps64 + 1e-8))
    assert n_gap >= len(FC.SIGNAL_T)
    for key in FC.edge_keys(name):
        if key.startswith('gap'):
            assert len(FC.zero_frames(FC.edge_input(name, key), L, S)) >= 3


@pytest.mark.parametrize('name', FC.EDGE_CONFIGS)
def test_edge_fixture_gaps_hold_silent_frames(name):
    L, S = FC.framing(name)
    keys = FC.edge_keys(name)
    assert len(keys) == 12 and sum(k.startswith('gap') for k in keys) == 2
    for key in keys:
        x = FC.edge_input(name, key)
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
        if key.startswith('gap'):
            assert len(FC.zero_frames(x, L, S)) >= 3 and OF.num_frames(len(x), L, S) >= 16


def test_signal_kinds():
    L, S = 400, 160
    n = FC.full_len(17, L, S)
    for kind in FC.KINDS:
        x = FC.make_signal(kind, n, 3, L, S)
        assert x.shape == (n,) and np.array_equal(x, x.astype(np.float32).astype(np.float64))
        assert np.array_equal(x, FC.make_signal(kind, n, 3, L, S))           # seeded
    pcm = FC.make_signal('pcm', n, 3, L, S)
    assert np.array_equal(pcm, np.round(pcm)) and 3000 < np.abs(pcm).max() < 32768
    tone = FC.make_signal('tone', 16000, 3, L, S)
    spec = np.abs(np.fft.rfft(tone))
    assert abs(int(np.argmax(spec)) - 1000) <= 1 and spec.max() > 100 * np.median(spec)
    assert not FC.make_signal('silence', n, 3, L, S).any()


@pytest.mark.parametrize('name', list(FC.CONFIGS))
def test_oracle_is_finite_over_the_table(name):
    for case in FC.cases(name):
        y = _want(name, case)
        assert y.shape == (FC.strided(case.T, FC.CONFIGS[name].kw.get('stride', 1)),
                           FC.CONFIGS[name].f_out), case
        assert np.isfinite(y).all(), case
        if case.kind == 'silence':
            # every column is constant: the reference is 0 up to the rounding of its mean
            assert np.abs(y).max() <= 1e-4, (case, np.abs(y).max())
