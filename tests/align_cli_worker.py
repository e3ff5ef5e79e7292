"""Child process of the align.py tests.  ``gpu``: the command lines from a dummy dataset through a
few training steps to ``align.py --save`` (tests/test_gpu_ctc_align.py).  ``cpu``: the same
command line on a machine without a GPU (tests/test_ctc_align_host.py): the network's forward pass
has no host form, so the model is built on device 'cpu' and its forward pass is REPLACED by
fixed random logits, one frame per audio sample -- everything else (checkpoint, dataset, label
parser, Model.align on the library's host form, the JSON lines) is the real thing.  Prints one
line ``RESULT <json>``."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _gpu(work):
    import train
    from extras import make_dataset
    from asr_study_amd.datasets import h5lite
    data = os.path.join(work, 'dummy.h5' if h5lite.available() else 'dummy.npz')
    make_dataset.main(['--parser', 'dummy', '--parser_params', 'num_speakers', '4',
                       'num_utterances_per_speaker', '6', 'max_duration', '1.2', 'min_duration',
                       '0.6', 'max_label_length', '8', 'split', '[0.5, 0.25]', 'seed', '3',
                       '--input_parser', 'mfcc', '--input_parser_params', 'dd', 'False',
                       '--output_file', data])
    run = os.path.join(work, 'run')
    train.main(['--dataset', data, '--model', 'graves2006', '--model_params', 'num_hiddens', '16',
                'std', '0.0', '--num_epochs', '1', '--batch_size', '4', '--save', run, '--seed',
                '1', '--lr', '0.01'])
    return os.path.join(run, 'best.h5'), data


def _cpu(work):
    import numpy as np
    import torch
    from asr_study_amd.core import callbacks, engine, models
    from asr_study_amd.datasets.dummy import Dummy
    from asr_study_amd.preprocessing import text
    engine.DEFAULT_DEVICE = 'cpu'
    data = os.path.join(work, 'dummy.npz')
    Dummy(num_speakers=3, num_utterances_per_speaker=4, max_duration=0.02, min_duration=0.01,
          max_label_length=6, split=[0.5, 0.25], seed=1, fs=16e3) \
        .to_h5(data, input_parser=None, label_parser=text.simple_char_parser, fmt='npz')
    model = models.graves2006(num_features=1, num_hiddens=8, num_classes=28, std=0.0)
    best = os.path.join(work, 'best.h5')
    callbacks.save_model(model, best, meta={
        'training_args': {'model': 'graves2006', 'input_parser': None, 'input_parser_params': [],
                          'label_parser': 'simple_char_parser', 'label_parser_params': []},
        'epochs': [0]})

    def to_slab(self, x):                        # (N, samples) raw audio: a frame per sample
        x = torch.as_tensor(np.asarray(x, np.float32))
        slab = torch.zeros((x.shape[1], 16, 1))
        slab[:, :x.shape[0], 0] = x.t()
        return slab

    def forward(self, slab, **kwargs):
        g = torch.Generator().manual_seed(slab.shape[0])
        return 3.0 * torch.randn((slab.shape[0], slab.shape[1], 28), generator=g)

    engine.Model.to_slab, engine.Model.forward = to_slab, forward
    return best, data


def main(work, mode):
    import align
    from asr_study_amd.preprocessing import text
    best, data = _gpu(work) if mode == 'gpu' else _cpu(work)
    out = os.path.join(work, 'out.jsonl')
    res = align.main(['--model', best, '--dataset', data, '--save', out])
    refused = False
    try:
        align.main(['--model', best, '--dataset', data, '--save', out])
    except IOError:
        refused = True
    align.main(['--model', best, '--dataset', data, '--save', out, '--override'])
    with open(out) as f:
        lines = [json.loads(ln) for ln in f]
    file_lines = []
    if mode == 'gpu':
        # one audio file with --text: the features are extracted here, so win_step is known and
        # the characters get times in seconds (a stored-feature dataset has none: null)
        import numpy as np
        from scipy.io import wavfile
        wav = os.path.join(work, 'utt.wav')
        rs = np.random.RandomState(0)
        wavfile.write(wav, 16000, (3000 * rs.randn(16000)).astype(np.int16))
        out2 = os.path.join(work, 'file.jsonl')
        align.main(['--model', best, '--file', wav, '--text', 'Hello, world', '--input_parser',
                    'mfcc', '--input_parser_params', 'dd', 'False', '--save', out2])
        with open(out2) as f:
            file_lines = [json.loads(ln) for ln in f]
    print('RESULT ' + json.dumps({
        'lines': lines, 'file_lines': file_lines, 'returned': len(res), 'refused': refused,
        'sanitised': [text.simple_char_parser._sanitize(r['label']) for r in lines]}))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
