"""Writes tests/golden/param_layout.json: the flat-parameter layout of one small model per
variant of the parameter table (asr_study_amd/core/params.py), recorded from the commit BEFORE
the table existed, when ``Model._layout`` / ``set_weights`` / ``_unpack`` still spelled every
stage kind out by hand.  tests/test_param_layout_host.py rebuilds every case and compares.

Recorded per case: n_params; per stage its kind, p_lo, p_hi and whichever offset attributes it
has; the sorted l2 segments; the (Keras name, shape) list; and, after ``set_weights`` of seeded
normal arrays, the sha256 of the params and bn_running bytes, the lengths of the three unpacked
lists and which gradients are all zero.  The digests come from seeded inputs, never from the
initial values: those go through LAPACK's SVD and need not be bit-stable across machines.

Run: python tests/golden/gen_param_layout.py   (builds on device='cpu', no GPU needed)"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

OFFSETS = ('oW', 'oU', 'ob', 'omi', 'ocell', 'og', 'obeta', 'orun', 'omom')
_BRSM = dict(num_features=13, num_classes=12, num_layers=2)
_DS2 = dict(num_features=16, num_classes=12, num_hiddens=10, num_layers=2, conv_filters=4,
            conv_kernels=((5, 7), (3, 5)))
_RHN = dict(num_features=13, num_classes=12, num_hiddens=10, num_layers=2)
CASES = [
    ('graves2006', 'graves2006', dict(num_features=26, num_hiddens=10, num_classes=12)),
    ('eyben', 'eyben', dict(num_features=13, num_hiddens=[10, 6, 7], num_classes=12)),
    ('maas', 'maas', dict(num_features=13, num_hiddens=10, num_classes=12)),
    ('deep_speech', 'deep_speech', dict(num_features=13, num_hiddens=12, num_classes=12)),
    ('brsmv1', 'brsmv1', dict(_BRSM, num_hiddens=10)),
    ('brsmv1_mi', 'brsmv1', dict(_BRSM, num_hiddens=10, mi=[1.0, 0.5, 0.5])),
    ('brsmv1_ln', 'brsmv1', dict(_BRSM, num_hiddens=12, layer_norm=[1.0, 0.0])),
    ('brsmv1_mi_ln_res', 'brsmv1', dict(_BRSM, num_hiddens=12, mi=[1.0, 0.5, 0.5],
                                        layer_norm=[1.0, 0.0], residual='sum')),
    ('deep_speech2', 'deep_speech2', dict(_DS2)),
    ('deep_speech2_bn', 'deep_speech2', dict(_DS2, batch_norm=True)),
    ('deep_speech2_gru', 'deep_speech2', dict(_DS2, rnn_type='gru')),
    ('deep_speech2_gru_bn', 'deep_speech2', dict(_DS2, rnn_type='gru', batch_norm='recurrent')),
    ('rhn_d2', 'rhn', dict(_RHN, depth=2)),
    ('rhn_d3_uncoupled_sum', 'rhn', dict(_RHN, depth=3, coupling=False, merge_mode='sum')),
]


def build(factory, kwargs):
    from asr_study_amd.core import models
    return getattr(models, factory)(device='cpu', **kwargs)


def seeded_weights(m):
    rs = np.random.RandomState(1)
    return [rs.standard_normal(w.shape).astype(np.float32) for w in m.get_weights()]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def record(m):
    """(the layout of a freshly built model as JSON-able data, the seeded weights it now holds)"""
    from asr_study_amd.core.callbacks import keras_layers
    out = {'n_params': int(m.n_params), 'stages': []}
    for s in m.stages:
        st = {'kind': s.kind, 'p_lo': int(s.p_lo), 'p_hi': int(s.p_hi)}
        for k in OFFSETS:
            if hasattr(s, k):
                v = getattr(s, k)
                st[k] = None if v is None else int(v)
        out['stages'].append(st)
    out['segments'] = [[int(o), int(n), float(c)] for o, n, c in m._segments]
    out['names'] = [[n, list(a.shape)] for _, ws in keras_layers(m, m.get_weights())
                    for n, a in ws]
    w2 = seeded_weights(m)
    m.set_weights(w2)
    out['params_sha256'] = _sha(m.params)
    out['bn_running_sha256'] = _sha(m.bn_running)
    grads = m.get_gradients()
    out['len_unpack'] = len(m._unpack(m.params.detach().cpu().numpy()))
    out['len_weights'] = len(m.get_weights())
    out['len_gradients'] = len(grads)
    out['zero_gradients'] = [bool(not g.any()) for g in grads]
    return out, w2


if __name__ == '__main__':
    layout = {name: record(build(factory, kw))[0] for name, factory, kw in CASES}
    with open(os.path.join(HERE, 'param_layout.json'), 'w') as f:     # one case per line
        f.write('{\n%s\n}\n' % ',\n'.join('%s: %s' % (json.dumps(name), json.dumps(layout[name],
                                                                                 sort_keys=True))
                                          for name in sorted(layout)))
