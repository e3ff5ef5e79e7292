"""Pins what ``Model._layout`` leaves on every ``Stage`` (and the ``Model`` attributes it reduces
over the stage list) against tests/golden/stage_table_parent.json, which was recorded before the
per-kind chains of ``_layout`` / ``forward`` / ``backward`` became the stage-kind table of
core/stages.py (tests/golden/gen_stage_table.py).  Host only."""
import importlib.util
import inspect
import json
import os
import re

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('gen_stage_table',
                                               os.path.join(GOLDEN, 'gen_stage_table.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, 'stage_table_parent.json')) as _f:
    TABLE = json.load(_f)


def test_every_case_is_pinned_and_every_kind_is_covered():
    assert sorted(TABLE) == sorted(name for name, _, _ in gen.CASES)
    assert set(s['kind'] for c in TABLE.values() for s in c['stages']) == set(gen.KINDS)


@pytest.mark.parametrize('name,factory,kwargs', gen.CASES, ids=[c[0] for c in gen.CASES])
def test_stages_match_the_fixture(name, factory, kwargs):
    m = gen.build(factory, kwargs)
    got, want = gen.record(m), TABLE[name]
    assert sorted(got) == sorted(want)
    assert len(got['stages']) == len(want['stages'])
    for i, (g, w) in enumerate(zip(got['stages'], want['stages'])):
        assert g == w, (i, w['kind'])       # (stage by stage: a mismatch names what moved)
    for key in sorted(want):
        assert got[key] == want[key], key
    # the derived fact that replaced the hand-kept list of kinds with weights
    assert [s.first for s in m.stages] == want['first']
    assert [s.first for s in m.stages] == [not any(p.tensors for p in m.stages[:i])
                                           for i in range(len(m.stages))]


def test_kinds_with_tensors_are_the_list_backward_kept_by_hand():
    with_tensors = set(s.kind for _, factory, kw in gen.CASES
                       for s in gen.build(factory, kw).stages if s.tensors)
    assert with_tensors == set(gen._WEIGHTED_AT_PARENT)


def test_every_spec_type_has_a_table_entry():
    """Every ``type`` core/models.py writes into a spec for the classes of core/layers.py."""
    from asr_study_amd.core import models, stages
    src = inspect.getsource(models.ctc_model) + inspect.getsource(models._elementwise_spec)
    emitted = set(re.findall(r"'type': '(\w+)'", src))
    assert emitted == set(gen.KINDS) == set(stages.KINDS)
    for kind in stages.KINDS.values():
        assert callable(kind.build) and callable(kind.forward) and callable(kind.backward)


def test_unknown_type_raises():
    from asr_study_amd.core.engine import Model
    with pytest.raises(ValueError) as e:
        Model([{'type': 'noise', 'value': 0.0}, {'type': 'nonesuch'}], 8, device='cpu')
    assert 'nonesuch' in str(e.value)
