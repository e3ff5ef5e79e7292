"""Writes tests/golden/bn_bits_parent.json: per case of tests/bn_cases.BIT_CASES the SHA-256 of the
inputs and of the raw bytes of every array the BatchNormalization / sequence-wise
BatchNormalization kernels return (y, stats, dx, dgamma, dbeta, inference y, moments, and for
the sequence form max |dp|), recorded ON THE GPU with the library of the commit BEFORE the two
kernel families of csrc/batchnorm.hip became one (fa842a3): that commit's csrc/ and include/
built with the library's own flags and selected with ASR_LIB_PATH (the C ABI did not change, so
it loads under this tree's Python).  tests/test_gpu_bn_bits.py records every case again and
compares for equality.

Run (needs a GPU):
    ASR_LIB_PATH=<the parent build's libasr_hip.so> python tests/golden/gen_bn_bits.py [dst]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def record():
    from tests import bn_cases
    table = {}
    for name in bn_cases.BIT_CASES:
        arrays, sha = bn_cases.bit_inputs(name)
        table[name] = {'inputs': sha, 'outputs': bn_cases.bit_outputs(name, arrays)}
        print(name, sha[:12], flush=True)
    return table


if __name__ == '__main__':
    from asr_study_amd import _lib
    table = record()
    print('library:', _lib.LIB_PATH)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'bn_bits_parent.json')
    with open(dst, 'w') as f:
        json.dump(table, f, sort_keys=True, indent=0)
        f.write('\n')
