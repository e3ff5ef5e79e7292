"""Writes tests/golden/stage_table_parent.json: every attribute ``Model._layout`` leaves on the
``Stage`` objects of one small model per stage kind, recorded from the commit BEFORE the
stage-kind table of asr_study_amd/core/stages.py existed (8426f04), when ``_layout`` still spelled
every kind out in one ``if s.kind == ...`` chain.  The JSON was written by running this file on
that commit, before the engine was touched; tests/test_stage_table_host.py rebuilds every case
and compares for equality.

Recorded per case: for every stage all of ``vars(s)`` except ``tensors`` (the parameter table,
pinned by param_layout.json) and ``first`` (new with the table); ``first`` as the expression of
the old ``Model.backward`` gave it (no stage before this one is of a kind in its hand-kept list
of kinds with weights); and the ``Model`` attributes that were reduced over kind lists.

Run: python tests/golden/gen_stage_table.py   (builds on device='cpu', no GPU needed)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

_TF = dict(num_features=16, num_classes=6, d_model=32, num_heads=2, num_layers=1)
_DS2 = dict(num_features=16, num_classes=6, num_hiddens=8, num_layers=1, conv_filters=4,
            batch_norm=True)
_RHN = dict(num_features=13, num_classes=6, num_hiddens=10, num_layers=1)
CASES = [
    ('transformer', 'transformer', dict(_TF)),
    ('conformer', 'conformer', dict(_TF)),
    ('conformer_specaug', 'conformer', dict(_TF, spec_augment=True)),
    ('deep_speech2_bn', 'deep_speech2', dict(_DS2)),
    ('deep_speech2_gru_seqbn', 'deep_speech2', dict(_DS2, rnn_type='gru',
                                                    batch_norm='recurrent')),
    ('deep_speech2_gru_ln', 'deep_speech2', dict(_DS2, batch_norm='layer', rnn_type='gru')),
    ('deep_speech', 'deep_speech', dict(num_features=13, num_hiddens=12, num_classes=6)),
    ('rhn', 'rhn', dict(_RHN)),
    ('rhn_d3_uncoupled_sum', 'rhn', dict(_RHN, depth=3, coupling=False, merge_mode='sum')),
    ('brsmv1_mi_ln_res', 'brsmv1', dict(num_features=13, num_classes=6, num_hiddens=12,
                                        num_layers=2, mi=[1.0, .5, .5], layer_norm=[1.0, 0.0],
                                        residual='sum')),
]
KINDS = ('noise', 'dropout', 'reshape', 'specaug', 'act', 'glu', 'posenc', 'merge', 'dense',
         'conv', 'dwconv', 'bn', 'ln', 'mha', 'bilstm', 'birnn', 'bigru', 'birhn')
# the list Model.backward kept by hand at 8426f04: 'kinds that have weights'
_WEIGHTED_AT_PARENT = ('dense', 'bilstm', 'conv', 'birnn', 'bn', 'bigru', 'birhn', 'ln', 'mha',
                       'dwconv')


def build(factory, kwargs):
    from asr_study_amd.core import models
    return getattr(models, factory)(device='cpu', **kwargs)


def encode(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [encode(e) for e in v]
    if isinstance(v, dict):
        return {str(k): encode(e) for k, e in v.items()}
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def record(m):
    out = {'stages': [{k: encode(v) for k, v in vars(s).items() if k not in ('tensors', 'first')}
                      for s in m.stages]}
    out['first'] = [not any(p.kind in _WEIGHTED_AT_PARENT for p in m.stages[:i])
                    for i in range(len(m.stages))]
    for k in ('num_classes', 'time_strides', 'n_params', '_has_rnn', '_has_mha', '_needs_lens',
              '_has_specaug', 'packed'):
        out[k] = encode(getattr(m, k))
    out['_bn'] = [i for i, _ in m._bn]
    out['_seqbn'] = [i for i, _ in m._seqbn]
    return json.loads(json.dumps(out))


if __name__ == '__main__':
    table = {name: record(build(factory, kw)) for name, factory, kw in CASES}
    assert set(s['kind'] for c in table.values() for s in c['stages']) == set(KINDS)
    with open(os.path.join(HERE, 'stage_table_parent.json'), 'w') as f:     # one case per line
        f.write('{\n%s\n}\n' % ',\n'.join('%s: %s' % (json.dumps(name), json.dumps(table[name],
                                                                                 sort_keys=True))
                                          for name in sorted(table)))
