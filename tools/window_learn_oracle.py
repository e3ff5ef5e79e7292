#!/usr/bin/env python
"""Re-derives ORACLE_LER0_STEP of tests/test_gpu_window.py on the host (no GPU):

    python tools/window_learn_oracle.py

builds the learning test's model (the transformer of tests/test_gpu_attention.py's learning test
with context=(4, 8, 0)) on the CPU, runs the float64 oracle's train_step
(tests/window_oracle.py) on the test's batch with Adam(lr=3e-3, clipnorm=400) and prints the first
step, counted from 1, at which the greedy decoding of the step's logits equals every label
sequence.  The test allows twice that many steps.  Run it again when the initialisation, the
factory or the oracle changes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_study_amd.core import engine  # noqa: E402

engine.DEFAULT_DEVICE = 'cpu'
from oracle import optim as OO  # noqa: E402
from tests import window_oracle as WO  # noqa: E402
from tests.test_gpu_window import learn_setup  # noqa: E402


def main(max_steps=2000):
    model, x, lab = learn_setup(device='cpu')
    stages = WO.stages_from_model(model)
    assert [st['window'] for st in stages if st['type'] == 'mha'] == [(4, 8, 0)] * 2
    x64 = x.transpose(1, 0, 2).astype(np.float64)
    lens = np.full(len(lab), x.shape[1])
    opt = OO.Adam(lr=3e-3, clipnorm=400.0)
    for step in range(1, max_steps + 1):
        out = WO.train_step(stages, x64, lab, lens, opt)
        done = WO.greedy(out['logits'], lens) == [[int(v) for v in l] for l in lab]
        if done or step % 20 == 0:
            print('step %d: mean ctc %.4f%s' % (step, float(np.mean(out['ctc'])),
                                                ', greedy LER 0' if done else ''), flush=True)
        if done:
            return step
    return None


if __name__ == '__main__':
    print('ORACLE_LER0_STEP = %s' % main())
