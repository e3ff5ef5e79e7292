"""Writes relattention_parent_models.json next to this file: the spec, the Keras config text and
the factory record of the default brsmv1(), deep_speech2(), transformer() and conformer().  It was
run once, from a checkout of the commit before relative positional attention, with that checkout
first on the module path:

    PYTHONPATH=<that checkout> python tests/golden/gen_relattention_parent_models.py

tests/test_relattention_host.py::test_existing_models_unchanged compares the current tree with
the file.  Host only, no device.
"""
import json
import os

NAMES = ('brsmv1', 'deep_speech2', 'transformer', 'conformer')


def record():
    from asr_study_amd.core import models
    from asr_study_amd.utils import keras_config as K
    out = {}
    for name in NAMES:
        m = getattr(models, name)(device='cpu')
        out[name] = {'spec': m.spec, 'model_config': K.model_config(m),
                     'kwargs': json.loads(json.dumps(m.config['kwargs']))}
    return out


if __name__ == '__main__':
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        'relattention_parent_models.json')
    with open(path, 'w') as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write('\n')
