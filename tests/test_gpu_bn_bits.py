"""-m gpu: the kernels of csrc/batchnorm.hip give the bits they gave before the BatchNormalization
and the sequence-wise BatchNormalization kernel families became one.  tests/golden/
bn_bits_parent.json holds, per case, the SHA-256 of the inputs and of every returned array as
recorded with the earlier library (tests/golden/gen_bn_bits.py); every case is recorded again and
compared for equality.  The determinism tests of test_gpu_batchnorm.py / test_gpu_seqbn.py show
that repeats are bit-identical, so the hashes are stable."""
import json
import os

import pytest

from tests import bn_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bn_bits_parent.json')


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(bn_cases.BIT_CASES)


@pytest.mark.parametrize('name', sorted(bn_cases.BIT_CASES))
def test_bits_match_the_parent(name, golden):
    arrays, sha = bn_cases.bit_inputs(name)
    # the inputs first: a drift of theirs is not a drift of the kernels
    assert sha == golden[name]['inputs']
    got = bn_cases.bit_outputs(name, arrays)
    want = golden[name]['outputs']
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(got) if got[k] != want[k]]
    assert not differ, differ
