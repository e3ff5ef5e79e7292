"""Pins the flat-parameter layout (offsets, l2 segments, Keras names and shapes, the padded
embedding of every tensor) against tests/golden/param_layout.json, which was recorded before
the per-kind code of ``_layout`` / ``set_weights`` / ``_unpack`` / ``keras_layers`` became the
parameter table of core/params.py (tests/golden/gen_param_layout.py).  Host only."""
import importlib.util
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('gen_param_layout',
                                               os.path.join(GOLDEN, 'gen_param_layout.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, 'param_layout.json')) as _f:
    LAYOUT = json.load(_f)


def test_every_case_is_pinned():
    assert sorted(LAYOUT) == sorted(name for name, _, _ in gen.CASES)


@pytest.mark.parametrize('name,factory,kwargs', gen.CASES, ids=[c[0] for c in gen.CASES])
def test_layout_matches_the_fixture(name, factory, kwargs):
    m = gen.build(factory, kwargs)
    epoch = m._weights_epoch
    got, w2 = gen.record(m)
    want = LAYOUT[name]
    assert sorted(got) == sorted(want)
    for key in sorted(want):        # (key by key: a mismatch names what moved)
        assert got[key] == want[key], key
    assert m._weights_epoch == epoch + 1
    back = m.get_weights()
    assert len(back) == len(w2)
    for (wname, _), a, b in zip(want['names'], w2, back):
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a, b), wname
    # the optimiser-slot view carries the trainable tensors only, in the same order
    trainable = [a for (wname, _), a in zip(want['names'], w2) if '_running_' not in wname]
    slots = m._unpack(m.params.detach().cpu().numpy())
    assert len(slots) == len(trainable)
    assert all(np.array_equal(a, b) for a, b in zip(trainable, slots))


@pytest.mark.parametrize('name,factory,kwargs', gen.CASES, ids=[c[0] for c in gen.CASES])
def test_wrong_shape_names_the_tensor(name, factory, kwargs):
    m = gen.build(factory, kwargs)
    names = [n for n, _ in LAYOUT[name]['names']]
    w = m.get_weights()
    for i in sorted(set((0, len(w) // 2, len(w) - 1))):
        bad = list(w)
        bad[i] = np.zeros(tuple(d + 1 for d in w[i].shape), np.float32)
        with pytest.raises((AssertionError, ValueError)) as e:
            m.set_weights(bad)
        assert names[i].rsplit(':', 1)[0] in str(e.value)
        assert all(np.array_equal(a, b) for a, b in zip(w, m.get_weights()))
