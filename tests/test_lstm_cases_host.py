"""CPU: the BiLSTM edge-case table (tests/lstm_cases.py) reaches every generic-kernel template
on both sides of every width at which make_plan switches templates, its oracle results are finite,
and its inputs drive a visible share of the hard-sigmoid gates into both saturated branches
(slope 0: the branch a kernel gets wrong without the unsaturated cases noticing)."""
import numpy as np
import pytest

from tests import lstm_cases as LC


def test_template_choice_restates_make_plan():
    """NKK = 4 / 8 / 16 for H <= 128 / 256 / 512; TPW = 1 / 2 / 4 / 8 for H <= 64 / 128 / 256 /
    512 (P = ceil(H / 16) <= 4 / 8 / 16 / 32)."""
    for H in range(4, 516, 4):
        t = LC.template(H)
        assert t['P'] == -(-H // 16)
        assert t['NKK'] == (4 if H <= 128 else 8 if H <= 256 else 16)
        assert t['TPW'] == (1 if H <= 64 else 2 if H <= 128 else 4 if H <= 256 else 8)
        assert 32 * t['NKK'] >= H and 64 * t['TPW'] >= H
    assert LC.template(300) == dict(P=19, NKK=16, TPW=8)
    assert LC.chains_per_launch(32) == 8 and LC.split_n_pad(8) == 80
    assert LC.chains_per_launch(19) == 13 and LC.split_n_pad(13) == 112


def test_table_reaches_every_generic_instantiation():
    reached = set()
    for c in LC.CASES:
        reached |= c.instantiations()
    want = {('fwd', nkk, v) for nkk in (4, 8, 16) for v in (False, True)} | \
           {('bwd', tpw, v) for tpw in (1, 2, 4, 8) for v in (False, True)}
    assert reached == want, sorted(want - reached)
    # the persistent plain-cell table alone reaches the plain ones, the variant group the others
    assert {i for c in LC.group('edges') for i in c.instantiations()} == {i for i in want if not i[2]}
    assert {i for c in LC.group('variants') for i in c.instantiations()} == {i for i in want if i[2]}
    # stepwise mode meets a ragged width in the narrow and in the widest templates
    assert {LC.template(c.H)['TPW'] for c in LC.group('stepwise')} == {2, 8}


@pytest.mark.parametrize('lo,hi', [(64, 68), (128, 132), (256, 260)])
def test_both_sides_of_every_template_boundary_are_present(lo, hi):
    widths = {c.H for c in LC.group('edges') if c.generic}
    assert lo in widths and hi in widths
    a, b = LC.template(lo), LC.template(hi)
    assert a['TPW'] != b['TPW'] and (a['NKK'] != b['NKK'] or lo == 64)
    # ... under both batch shapes: one tile with eleven padding rows, two tiles
    for H in (lo, hi):
        assert {c.N for c in LC.group('edges') if c.H == H} == {5, 20}


def test_split_cases_exceed_one_launch_on_a_256_cu_part():
    for c in LC.group('split'):
        for P in LC.split_plan_p(c):
            cpl = LC.chains_per_launch(P)
            n_pad = LC.split_n_pad(max(LC.chains_per_launch(q) for q in LC.split_plan_p(c)))
            assert 2 * n_pad // 16 > cpl and n_pad <= 272, c


def _data(c):
    if c.N is not None:
        return LC.build(c.name)
    n_pad = LC.split_n_pad(max(LC.chains_per_launch(q) for q in LC.split_plan_p(c)))
    return LC.build(c.name, n_pad - 3, n_pad)


# the share of hard-sigmoid gates (i, f, o over all steps, rows, units, directions) that a case
# must have at exactly 0 and at exactly 1: one in a hundred is "visible" for the smallest case
# too (H = 4, T = 1: 384 gates); the table's biases aim at a quarter each (lstm_cases.table_bias).
MIN_SHARE = 0.01


@pytest.mark.parametrize('case', LC.CASES, ids=repr)
def test_oracle_is_finite_and_saturates_the_hard_sigmoid(case):
    D = _data(case)
    for name, a in D.want.items():
        assert np.isfinite(a).all(), name
    assert np.abs(D.want['y']).max() > 0.05 and np.abs(D.want['dz'][:, :D.N]).max() > 1e-3
    assert not D.want['dz'][:, D.N:].any()            # no upstream gradient: exactly zero
    assert D.knee_margin >= LC.KNEE_MARGIN, D.knee_margin
    assert D.share_at_0 >= MIN_SHARE, D.share_at_0
    assert D.share_at_1 >= MIN_SHARE, D.share_at_1
