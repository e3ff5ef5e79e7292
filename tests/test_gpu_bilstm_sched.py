"""-m gpu: the two-direction LSTM stage (core/bilstm.py) keeps the schedule and the bits it had
while its two bodies were methods of ``Model``.  tests/golden/bilstm_sched_parent.json holds, per
case and step, every ``ops`` call the engine makes TOGETHER WITH every event record, event wait
and stream wait (which stream, which event, in which order), the SHA-256 of the logits and of
every gradient array, and the model's compact-launch and measuring-pass counters, recorded on the
commit before (tests/golden/gen_bilstm_sched.py, which says what a case is and which branch of
the bodies it is there for); every case is recorded again and compared for equality.  This is
the pin test_gpu_engine_trace.py cannot be: a wait that is dropped or moved shows here.  The
fixture was recorded twice; a case whose bits differed between the two has none in the file.
The two schedules under a process group stay with test_gpu_parallel.py."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('gen_bilstm_sched',
                                               os.path.join(GOLDEN, 'gen_bilstm_sched.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, 'bilstm_sched_parent.json')) as _f:
    PINNED = gen.expand(json.load(_f))


def test_every_case_is_pinned():
    assert sorted(PINNED) == sorted(gen.NAMES)
    for c in gen.CASES:
        assert len(PINNED[c['name']]) == (len(c['infer']) if c['infer'] else c['steps'])


@pytest.mark.parametrize('name', gen.NAMES)
def test_schedule_and_bits_match_the_parent(name):
    got, want = gen.record(name), PINNED[name]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for i, (a, b) in enumerate(zip(g['calls'], w['calls'])):
            assert a == b, (name, k, i)     # (line by line: a mismatch names the first that moved)
        assert len(g['calls']) == len(w['calls']), (name, k)
        if 'bits' in w:
            differ = [a for a in sorted(w['bits']) if g['bits'].get(a) != w['bits'][a]]
            assert not differ and sorted(g['bits']) == sorted(w['bits']), (name, k, differ)
        assert all(g[a] == w[a] for a in w if a not in ('bits', 'calls')), (name, k)
    streams = set(line.split(' ', 1)[0] for st in got for line in st['calls'])
    if name == 'h256_pipeline':
        assert streams == {'main', 'side', 'pipe'}
        assert any(' wait e' in line for line in got[0]['calls'])
    if name == 'h512_compact':
        # the measuring pass of each of the three layers: at step 1, not at step 2, and again
        # behind new weights
        assert [st['compact_launches'] for st in got] == [2, 2, 2]
        assert [st['dz_measure_passes'] for st in got] == [3, 3, 6]
