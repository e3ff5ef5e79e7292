#!/usr/bin/env python
"""``python align.py --model best.h5 --dataset data.h5 [--subset test] [--save out.jsonl]`` or
``--file utterance.wav --text "the transcript"`` -- where each character of a known transcript
lies in its audio (CTC forced alignment)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asr_study_amd.cli import align_main as main  # noqa: E402

if __name__ == '__main__':
    main()
