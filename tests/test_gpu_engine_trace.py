"""Pins the launch sequence of one training step (and of one inference pass of the small models)
against tests/golden/engine_trace_parent.json: which library call the engine makes, in which
order, on which stream, on which buffers.  The fixture was recorded on the GPU before the
per-kind chains of ``Model.forward`` / ``Model.backward`` became the stage-kind table of
core/stages.py; the recorder is the one of tests/golden/gen_engine_trace.py, shared.

Floating-point digests are no safe pin across commits here (the CTC kernels and one BPTT path
accumulate with float atomics); what a pure engine refactor must keep exactly is this sequence.

LIMIT: the recorder sees calls into ``asr_study_amd.ops`` only.  It does not see torch event
records and stream waits (nor torch's own copies and fills).  Those of the BiLSTM schedule
(core/bilstm.py) are pinned by test_gpu_bilstm_sched.py, whose recorder extends this one with the
event and stream-wait lines and which also compares the bits; the schedules under a process group
stay with the bit-identity tests of test_gpu_parallel.py."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('gen_engine_trace',
                                               os.path.join(GOLDEN, 'gen_engine_trace.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, 'engine_trace_parent.json')) as _f:
    TRACE = json.load(_f)


def test_every_case_is_pinned():
    assert sorted(TRACE) == sorted(c[0] for c in gen.CASES)
    assert all(sorted(TRACE[c[0]]) == (['infer', 'train'] if c[5] else ['train'])
               for c in gen.CASES)


@pytest.mark.parametrize('name,factory,kwargs,N,T,infer', gen.CASES, ids=[c[0] for c in gen.CASES])
def test_launch_sequence_matches_the_fixture(name, factory, kwargs, N, T, infer):
    got, m = gen.trace(factory, kwargs, N, T, infer)
    want = TRACE[name]
    assert sorted(got) == sorted(want)
    for phase in sorted(want):
        for i, (g, w) in enumerate(zip(got[phase], want[phase])):
            assert g == w, (phase, i)       # (call by call: a mismatch names the first that moved)
        assert len(got[phase]) == len(want[phase]), phase
    streams = set(line.split(' ', 1)[0] for line in got['train'])
    if name == 'brsmv1_256_pipeline':   # the frame-range pipeline and the side-stream gradients
        assert streams == {'main', 'side', 'pipe'} and m._compact_launches == 0
    if name == 'brsmv1_512_compact':    # as test_compact_bptt_schedule... asserts at T = 11
        assert m._compact_launches == 2 and m.packed and 'side' in streams
