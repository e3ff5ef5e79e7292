"""Child process of tests/test_gpu_beam_lm.py::test_command_lines_end_to_end: the command lines
from a dummy dataset to transcriptions with a character language model, then the same decode
through core/ctc_utils.decode.  Prints one line ``RESULT <json>``."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(work):
    import numpy as np
    import train
    import eval as eval_cli
    import predict as predict_cli
    from extras import make_dataset, make_lm
    from asr_study_amd.core import ctc_utils
    from asr_study_amd.datasets import h5lite
    from asr_study_amd.datasets.dataset_generator import DatasetGenerator
    from asr_study_amd.lm import CharLM
    from asr_study_amd.preprocessing import text
    from asr_study_amd.utils.core_utils import load_model
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
    best = os.path.join(run, 'best.h5')
    lm_file = os.path.join(work, 'lm.npz')
    make_lm.main(['--dataset', data, '--subset', 'train', '--order', '3', '--output_file',
                  lm_file])
    lm = CharLM.load(lm_file)
    lm_args = ['--lm', lm_file, '--lm_alpha', '0.9', '--lm_beta', '0.4']
    values = eval_cli.main(['--model', best, '--dataset', data, '--beam_width', '20'] + lm_args)
    os.environ['ASR_BEAM'] = 'device'
    res = predict_cli.main(['--model', best, '--dataset', data, '--beam_width', '10'] + lm_args)
    # the same decode, called directly on the same model's logits, on the host decoder
    os.environ['ASR_BEAM'] = 'host'
    model = load_model(best, mode='predict', decoder=False)
    flow = DatasetGenerator(None, text.simple_char_parser, batch_size=1, seed=0, mode='predict',
                            shuffle=False).flow_from_fname(data, datasets='test')
    direct = []
    for _ in range(flow.len):
        x, lens = flow.next()
        slab = x[1] if isinstance(x, tuple) else model.to_slab(x)
        logits = model.forward(slab, training=False, need_grad=False, n_valid=1)
        hyp = ctc_utils.decode((logits, model.out_lengths(np.asarray(lens).reshape(-1))),
                               is_greedy=False, beam_width=10, lm=lm_file, lm_alpha=0.9,
                               lm_beta=0.4)
        direct.append(text.simple_char_parser.imap(hyp[0]))
    print('RESULT ' + json.dumps({
        'eval': [float(v) for v in values], 'lm_order': lm.order, 'lm_labels': lm.num_labels,
        'predicted': [r['best'] for r in res], 'direct': direct}))


if __name__ == '__main__':
    main(sys.argv[1])
