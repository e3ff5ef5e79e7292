"""-m gpu: every entry point of the GEMM family (asr_gemm at both precisions and all eight fast
variants, asr_pack_hl with both kernels, asr_gemm_hl row-major / k-major / batched / segmented /
persistent at both tiles and with split-K, asr_absmax, asr_colsum) writes the bits it wrote before
csrc/gemm.hip was split by kernel family and its repeated pieces were written once.
tests/golden/gemm_bits_parent.json holds, per case, the SHA-256 of the raw bytes of every output
array, recorded on the commit before (tests/golden/gen_gemm_bits.py, which says what a case is);
every case is recorded again and compared for equality.  Nothing in the family accumulates with
float atomics: the fixture was recorded twice and came out the same."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('gen_gemm_bits',
                                               os.path.join(GOLDEN, 'gen_gemm_bits.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, 'gemm_bits_parent.json')) as _f:
    PINNED = json.load(_f)


def test_every_case_is_pinned():
    assert sorted(PINNED) == gen.CASES


@pytest.mark.parametrize('name', gen.CASES)
def test_bits_match_the_parent(name):
    got, want = gen.record(name), PINNED[name]
    differ = [a for a in sorted(want) if got.get(a) != want[a]]
    assert not differ and sorted(got) == sorted(want), (name, differ)
