"""-m gpu: the recurrent stage handlers of core/stages.py (SimpleRNN, GRU, RHN and the
one-direction GRU and LSTM, trained and streamed) give the bits, and make the library calls, they
gave before the one- and two-direction forms came to share their handlers and GEMM helpers.
tests/golden/rec_bits_parent.json holds, per case, the SHA-256 of the logits and of every gradient
array and the call skeleton of the step (stream and name of every ``ops`` call, M, N, K of a
gemm), recorded on the commit before (tests/golden/gen_rec_bits.py, which says what a case is);
every case is recorded again and compared for equality.  CTC, whose kernels accumulate with float
atomics, is not part of a case: the fixture was recorded twice and came out the same."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('gen_rec_bits',
                                               os.path.join(GOLDEN, 'gen_rec_bits.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, 'rec_bits_parent.json')) as _f:
    PINNED = json.load(_f)


def test_every_case_is_pinned():
    assert sorted(PINNED) == gen.CASES


@pytest.mark.parametrize('name', gen.CASES)
def test_bits_and_calls_match_the_parent(name):
    got, want = gen.record(name), PINNED[name]
    steps = zip(got, want) if isinstance(want, list) else [(got, want)]
    assert not isinstance(want, list) or len(got) == len(want)
    for k, (g, w) in enumerate(steps):
        assert sorted(g) == sorted(w)
        assert g['calls'] == w['calls'], (name, k)
        differ = [a for a in sorted(w['bits']) if g['bits'].get(a) != w['bits'][a]]
        assert not differ and sorted(g['bits']) == sorted(w['bits']), (name, k, differ)
        assert all(g[a] == w[a] for a in w if a not in ('bits', 'calls')), (name, k)
