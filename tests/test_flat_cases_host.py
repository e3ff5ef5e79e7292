"""CPU: the case table of the flat kernels (tests/flat_cases.py) against the index models of
tests/flat_kernel_model.py.  The walk as written visits every element of every case exactly once
(with the right segment), and every seeded defect breaks at least one case: the table is sharp
where such kernels go wrong, shown without a GPU."""
import numpy as np
import pytest

from tests import flat_cases as FC
from tests import flat_kernel_model as KM

VEC_TAIL = ('mul', 'axpby', 'swish', 'absmax')
SCALAR = ('activation',)
UPDATE = ('adam', 'sgd')


def _layout(n, name):
    return FC.layouts(n)[name]


def _norm_vecs(n):
    """Both alignments below the cap and at the largest size; the 16-byte path in between."""
    return (1, 0) if n < FC.cap('norm') - 1 or n == FC.NORM_N else (1,)


def _cases(kernel):
    """(label, callable(defect) -> True if the walk is right) for every case of a kernel."""
    out = []
    if kernel in VEC_TAIL:
        for n in FC.sizes(kernel):
            out.append(('n=%d' % n, lambda d, n=n: _once(KM.vec_tail(kernel, n, d))))
    elif kernel == 'random':
        for n in FC.sizes(kernel):
            out.append(('n=%d' % n, lambda d, n=n: _once(KM.random(n, d))))
    elif kernel in SCALAR:
        for n in FC.sizes(kernel):
            out.append(('n=%d' % n, lambda d, n=n: _once(KM.scalar(kernel, n, d))))
    elif kernel == 'glu':
        for case in FC.GLU_CASES:
            for items in FC.glu_items(*case):
                out.append(('items=%d' % items, lambda d, items=items: _once(KM.glu(items, d))))
    elif kernel in UPDATE:
        for n, name in FC.update_cases(kernel):
            segs = _layout(n, name)
            out.append(('n=%d %s' % (n, name), lambda d, n=n, segs=segs: _once_seg(
                KM.update(kernel, n, segs, d), segs, n)))
    elif kernel == 'norm':
        for n, name in FC.norm_cases():
            segs = _layout(n, name)
            for vec in _norm_vecs(n):
                out.append(('n=%d %s vec=%d' % (n, name, vec),
                            lambda d, n=n, segs=segs, vec=vec: _once_seg(
                                KM.norm(n, segs, vec, d), segs, n)))
    elif kernel == 'colsum':
        for M in FC.COLSUM_M:
            out.append(('M=%d' % M, lambda d, M=M: _once(KM.colsum(M, d))))
    return out


def _once(r):
    visits, oob = r
    return oob == 0 and bool((visits == 1).all())


def _once_seg(r, segs, n):
    visits, oob, used = r
    return oob == 0 and bool((visits == 1).all()) and \
        bool(np.array_equal(used, FC.segment_index(segs, n)))


KERNELS = VEC_TAIL + ('random',) + SCALAR + ('glu',) + UPDATE + ('norm', 'colsum')
# which seeded defects a kernel's walk can have
APPLIES = {
    'no_tail': VEC_TAIL + ('random', 'norm', 'colsum'),
    'le_chunk_end': KERNELS,
    'short_stride': VEC_TAIL + ('random', 'glu') + SCALAR + UPDATE,
    'vec_off_by_one': ('random', 'norm'),
    'seg_stuck': UPDATE + ('norm',),
    'slices_16': ('colsum',),
    'no_wrap': VEC_TAIL + ('random', 'glu') + SCALAR + UPDATE,
}


def test_the_table_restates_the_launch_geometry():
    """The caps of the issue's table, and the classes every kernel's sizes must hold."""
    assert FC.cap('random') == 2097152 and FC.cap('mul') == FC.cap('axpby') == 4194304
    assert FC.cap('swish') == 4194304 and FC.cap('activation') == 1048576
    assert FC.cap('adam') == FC.cap('sgd') == 524288 and FC.cap('norm') == 2097152
    assert FC.cap('absmax') == 262144 and FC.cap('glu') == 4096 * 256
    for k in KERNELS:
        if k in ('glu', 'colsum'):
            continue
        s, c = FC.sizes(k), FC.cap(k)
        assert {1, 2, 3, c, c + 4 * 256 * 3 + 5} <= set(s)
        assert {n % 4 for n in s if 4 < n < c} >= {1, 2, 3}
        assert max(s) <= 4.3e6
    assert {FC.cap('norm') - 1, FC.cap('norm') + 1} <= set(FC.sizes('norm'))
    fwd, bwd = zip(*[FC.glu_items(*c) for c in FC.GLU_CASES])
    assert FC.cap('glu') in fwd and FC.cap('glu') in bwd and max(fwd) > FC.cap('glu')


def test_the_layouts_put_boundaries_where_the_issue_asks():
    for n in (FC.OPTIM_N, FC.NORM_N):
        lay = FC.layouts(n)
        chunk = FC.norm_chunk(n)
        for name, segs in lay.items():
            assert segs[0][0] == 0 and sum(ln for _, ln, _ in segs) == n
            assert all(a[0] + a[1] == b[0] for a, b in zip(segs, segs[1:]))
            assert all(ln > 0 for _, ln, _ in segs)
        offs = {o for o, _, _ in lay['edges']}
        assert any(o % 4 for o in offs)                              # inside a float4 group
        for mark in (1024, 2048, chunk, chunk + 1024):
            assert {mark - 1, mark + 1} <= offs, mark
        l2s = [l for _, _, l in lay['edges']]
        assert set(l2s[::2]) == {0.0} and set(l2s[1::2]) == {FC.L2}
        assert len(lay['single']) == 1 and len(lay['many']) >= 300
        pos, k = FC.probes(n, lay['edges'])
        assert len(pos) == k * k and pos[0] == 0 and pos[-1] == n - 1
        for o in offs - {0}:
            assert o in pos and o - 1 in pos
        for mark in range(1024, n, 1024):
            assert mark in pos and mark - 1 in pos
    assert FC.norm_chunk(FC.OPTIM_N) == 2048 and FC.norm_chunk(FC.NORM_N) == 4096


@pytest.mark.parametrize('kernel', KERNELS)
def test_the_walk_as_written_visits_every_element_once(kernel):
    cases = _cases(kernel)
    assert cases
    for label, run in cases:
        assert run(None), (kernel, label)


@pytest.mark.parametrize('defect', KM.DEFECTS)
def test_every_seeded_defect_breaks_a_case(defect):
    for kernel in APPLIES[defect]:
        caught = [label for label, run in _cases(kernel) if not run(defect)]
        print('[flat] %-14s %-10s caught by %d case(s): %s'
              % (defect, kernel, len(caught), ', '.join(caught[:4])))
        assert caught, (defect, kernel)


def test_a_loop_that_does_not_wrap_is_caught_only_past_the_cap():
    """What the suite lacked: below the cap a grid-stride loop may as well be an `if`."""
    for kernel in VEC_TAIL + ('random',) + SCALAR + UPDATE:
        for label, run in _cases(kernel):
            n = int(label.split()[0][2:])
            assert run('no_wrap') == (n <= FC.cap(kernel)), (kernel, label)
