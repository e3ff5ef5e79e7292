#!/usr/bin/env python
"""``python -m extras.make_lm --dataset data.h5 --subset train --order 3 --output_file lm.npz``
-- estimates the character n-gram language model eval.py / predict.py take as ``--lm``; ``--text
file`` adds (or replaces the dataset by) one sentence per line."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_study_amd.cli import make_lm_main as main  # noqa: E402

if __name__ == '__main__':
    main()
