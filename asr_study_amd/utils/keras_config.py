"""Keras-1.2.2 ``model.save()`` metadata for the build's checkpoints.

``keras.models.save_model`` (keras==1.2.2, msc.yaml:89) writes, next to ``/model_weights``,
three things ``keras.models.load_model`` -- the reference's ``utils/core_utils.py:63-64`` --
reads back:

* root attribute ``model_config``: JSON ``{"class_name": "Model", "config": {"name", "layers":
  [{"class_name", "name", "config", "inbound_nodes"}], "input_layers", "output_layers"}}`` of
  the functional graph ``ctc_model`` builds (core/models.py:31-52): the three ``Input``s
  (``inputs``, sparse int32 ``labels``, int32 ``inputs_length``), the chain of
  ``GaussianNoise`` / ``TimeDistributed(Dense)`` / ``Dropout`` / ``Bidirectional(LSTM)`` /
  ``Bidirectional(SimpleRNN)`` ('concat' or 'sum') / ``TimeDistributed(Activation)`` /
  ``TimeDistributed(Dropout)`` / ``BatchNormalization`` / ``Merge`` / ``SpecAugment`` layers and
  the two ``Lambda``s
  ``decoder`` and ``ctc``;
* root attribute ``training_config``: JSON with the optimizer's class and config, the loss /
  metric names and ``loss_weights`` of ``train.py:140-143``;
* group ``optimizer_weights`` (attribute ``weight_names``): ``[iterations, m..., v...]`` for
  Adam / ``[iterations, moments...]`` for SGD, one tensor per trainable weight in
  ``model.trainable_weights`` order and Keras gate layout.

The schema is RESTATED FROM MEMORY of keras 1.2.2 (``engine/topology.py`` ``Container.
get_config``, ``layers/recurrent.py``, ``layers/wrappers.py``, ``models.py`` ``save_model``);
Keras cannot run in this image, so it is unpinned.  Two things a real Keras file carries
cannot be reproduced here and are the documented residue: (1) Keras-1.2.2
serialises a ``Lambda``'s function with ``marshal`` of its Python-2.7 bytecode
(``func_dump``); this writer names the function instead (``function_type: "function"``),
which ``Lambda.from_config`` resolves through ``custom_objects`` -- and
``get_custom_objects()`` (utils/core_utils.py:41-47) passes every function of
``core.ctc_utils`` by name; (2) TF variable names of the optimizer slots (``param_<i>`` is
what Keras itself falls back to when a weight has no name; loading is by position).

The reader side (``topology_from_config``) rebuilds this package's model from such a JSON
when a file has neither the build's own factory record nor ``meta/training_args``.
"""
import json

LAMBDA_MODULE = 'core.ctc_utils'


def _regularizer(l2):
    return None if not l2 else {'name': 'WeightRegularizer', 'l1': 0.0, 'l2': float(l2)}


def _lstm_config(name, s, go_backwards=False):
    """keras.layers.LSTM.get_config() (Recurrent + LSTM) plus the reference override's four
    extra keys (core/layers.py:471-479)."""
    return {
        'name': name, 'trainable': True, 'return_sequences': True, 'go_backwards': go_backwards,
        'stateful': False, 'unroll': False, 'consume_less': 'gpu', 'input_dim': int(s.f_in),
        'input_length': None, 'output_dim': int(s.H), 'init': 'glorot_uniform',
        'inner_init': 'orthogonal', 'forget_bias_init': 'one',
        'activation': getattr(s, 'act', 'tanh'),
        'inner_activation': 'hard_sigmoid', 'W_regularizer': _regularizer(s.l2_W),
        'U_regularizer': _regularizer(s.l2_U), 'b_regularizer': None,
        'dropout_W': float(s.dropout_W), 'dropout_U': float(s.dropout_U),
        'layer_norm': s.ln, 'mi': s.mi, 'zoneout_h': float(s.zoneout_h),
        'zoneout_c': float(s.zoneout_c)}


def _act_name(act):
    """An activation as Keras config text: the clipped ReLU is named (a closure in the
    reference, not serialisable) and its max_value kept beside it."""
    if isinstance(act, (tuple, list)) and act and act[0] == 'clipped_relu':
        return 'clipped_relu', float(act[1])
    return str(act or 'tanh'), None


def _act_from(c):
    from ..core import layers as L
    if c.get('activation') == 'clipped_relu':
        return L.clipped_relu(c.get('max_value', 20.0))
    return c.get('activation', 'tanh')


def _simplernn_config(name, s):
    """keras.layers.SimpleRNN.get_config() (Recurrent + SimpleRNN)."""
    act, mv = _act_name(s.act)
    cfg = {'name': name, 'trainable': True, 'return_sequences': True, 'go_backwards': False,
           'stateful': False, 'unroll': False, 'consume_less': 'cpu', 'input_dim': int(s.f_in),
           'input_length': None, 'output_dim': int(s.H), 'init': s.init,
           'inner_init': 'orthogonal', 'activation': act,
           'W_regularizer': _regularizer(s.l2_W), 'U_regularizer': _regularizer(s.l2_U),
           'b_regularizer': None, 'dropout_W': float(s.dropout_W),
           'dropout_U': float(s.dropout_U)}
    if mv is not None:
        cfg['max_value'] = mv
    return cfg


def _gru_config(name, s):
    """keras.layers.GRU.get_config() (Recurrent + GRU), consume_less='gpu'."""
    act, mv = _act_name(s.act)
    cfg = {'name': name, 'trainable': True, 'return_sequences': True, 'go_backwards': False,
           'stateful': False, 'unroll': False, 'consume_less': 'gpu', 'input_dim': int(s.f_in),
           'input_length': None, 'output_dim': int(s.H), 'init': 'glorot_uniform',
           'inner_init': 'orthogonal', 'activation': act, 'inner_activation': 'hard_sigmoid',
           'W_regularizer': _regularizer(s.l2_W), 'U_regularizer': _regularizer(s.l2_U),
           'b_regularizer': None, 'dropout_W': float(s.dropout_W),
           'dropout_U': float(s.dropout_U)}
    if mv is not None:
        cfg['max_value'] = mv
    if getattr(s, 'bn', False):     # (only then: files of every other model keep their bytes)
        cfg.update(batch_norm=True, bn_epsilon=float(s.bn_eps), bn_momentum=float(s.bn_momentum))
    return cfg


def _rhn_config(name, s):
    """The reference's RHN.get_config() (core/layers.py:331-353) on top of Recurrent's keys."""
    act, mv = _act_name(s.act)
    cfg = {'name': name, 'trainable': True, 'return_sequences': True, 'go_backwards': False,
           'stateful': False, 'unroll': False, 'consume_less': 'gpu', 'input_dim': int(s.f_in),
           'input_length': None, 'output_dim': int(s.H), 'depth': int(s.depth),
           'init': 'glorot_uniform', 'inner_init': 'orthogonal',
           'bias_init': 'highway_bias_initializer', 'activation': act,
           'inner_activation': 'hard_sigmoid', 'coupling': bool(s.coupling), 'layer_norm': False,
           'ln_gain_init': 'one', 'ln_bias_init': 'zero', 'mi': False,
           'W_regularizer': _regularizer(s.l2_W), 'U_regularizer': _regularizer(s.l2_U),
           'b_regularizer': None, 'dropout_W': float(s.dropout_W),
           'dropout_U': float(s.dropout_U)}
    if mv is not None:
        cfg['max_value'] = mv
    return cfg


def _lambda_config(name, function, output_shape, arguments):
    return {'name': name, 'trainable': True, 'function': function, 'function_type': 'function',
            'output_shape': output_shape[0], 'output_shape_type': output_shape[1],
            'arguments': arguments}


def model_config(model):
    """The ``model_config`` JSON string of ``model`` (an engine.Model)."""
    layers = []

    def add(cls, name, config, inbound):
        layers.append({'class_name': cls, 'name': name, 'config': config,
                       'inbound_nodes': [[[n, 0, 0] for n in inbound]] if inbound else []})
    add('InputLayer', 'inputs', {'batch_input_shape': [None, None, int(model.num_features)],
                                 'input_dtype': 'float32', 'sparse': False, 'name': 'inputs'}, [])
    prev = 'inputs'
    out_names = []                      # output layer name per stage (for Merge skips)
    counts = {}

    def nm(kind):
        counts[kind] = counts.get(kind, 0) + 1
        return '%s_%d' % (kind, counts[kind])
    for s in model.stages:
        if s.kind == 'noise':
            name = nm('gaussiannoise')
            add('GaussianNoise', name, {'name': name, 'trainable': True, 'sigma': float(s.value)},
                [prev])
        elif s.kind == 'specaug':
            name = nm('specaugment')
            add('SpecAugment', name, dict({'name': name, 'trainable': True}, **s.policy), [prev])
        elif s.kind == 'dropout' and getattr(s, 'wrapped', False):
            name = nm('timedistributed')
            inner = nm('dropout')
            add('TimeDistributed', name, {'name': name, 'trainable': True, 'layer': {
                'class_name': 'Dropout', 'config': {'name': inner, 'trainable': True,
                                                   'p': float(s.value)}}}, [prev])
        elif s.kind == 'dropout':
            name = nm('dropout')
            add('Dropout', name, {'name': name, 'trainable': True, 'p': float(s.value)}, [prev])
        elif s.kind == 'dense':
            name = nm('timedistributed')
            dname = nm('dense')
            add('TimeDistributed', name, {
                'name': name, 'trainable': True,
                'layer': {'class_name': 'Dense', 'config': {
                    'name': dname, 'trainable': True, 'output_dim': int(s.n_out),
                    'input_dim': int(s.f_in), 'init': 'glorot_uniform', 'activation': 'linear',
                    'W_regularizer': _regularizer(s.l2), 'b_regularizer': None,
                    'activity_regularizer': None, 'W_constraint': None, 'b_constraint': None,
                    'bias': True}}}, [prev])
        elif s.kind == 'bilstm' and getattr(s, 'directions', 2) == 1:
            name = nm('lstm')           # a bare (unidirectional) LSTM: a plain LSTM layer
            add('LSTM', name, _lstm_config(name, s), [prev])
        elif s.kind == 'bilstm':
            name = nm('bidirectional')
            add('Bidirectional', name, {
                'name': name, 'trainable': True, 'merge_mode': 'concat',
                'layer': {'class_name': 'LSTM',
                          'config': _lstm_config('lstm_%d' % counts['bidirectional'], s)}}, [prev])
        elif s.kind == 'act':
            wrapped = getattr(s, 'wrapped', False)
            name = nm('timedistributed') if wrapped else None
            act, mv = _act_name(s.act)
            inner = {'name': nm('activation'), 'trainable': True, 'activation': act}
            if mv is not None:
                inner['max_value'] = mv
            if wrapped:
                add('TimeDistributed', name, {'name': name, 'trainable': True, 'layer': {
                    'class_name': 'Activation', 'config': inner}}, [prev])
            else:
                name = inner['name']
                add('Activation', name, inner, [prev])
        elif s.kind == 'birnn':
            name = nm('bidirectional')
            add('Bidirectional', name, {
                'name': name, 'trainable': True, 'merge_mode': s.merge,
                'layer': {'class_name': 'SimpleRNN', 'config': _simplernn_config(
                    'simplernn_%d' % counts['bidirectional'], s)}}, [prev])
        elif s.kind == 'bigru' and getattr(s, 'directions', 2) == 1:
            name = nm('gru')            # a bare (unidirectional) GRU: a plain Keras GRU layer
            add('GRU', name, _gru_config(name, s), [prev])
        elif s.kind == 'bigru':
            name = nm('bidirectional')
            add('Bidirectional', name, {
                'name': name, 'trainable': True, 'merge_mode': s.merge,
                'layer': {'class_name': 'GRU', 'config': _gru_config(
                    'gru_%d' % counts['bidirectional'], s)}}, [prev])
        elif s.kind == 'birhn':
            name = nm('bidirectional')
            add('Bidirectional', name, {
                'name': name, 'trainable': True, 'merge_mode': s.merge,
                'layer': {'class_name': 'RHN', 'config': _rhn_config(
                    'rhn_%d' % counts['bidirectional'], s)}}, [prev])
        elif s.kind == 'bn':
            name = nm('batchnormalization')
            add('BatchNormalization', name, {
                'name': name, 'trainable': True, 'epsilon': float(s.eps), 'mode': 0, 'axis': -1,
                'momentum': float(s.momentum), 'gamma_regularizer': None,
                'beta_regularizer': None}, [prev])
        elif s.kind == 'ln':
            name = nm('layernormalization')
            add('LayerNormalization', name, {
                'name': name, 'trainable': True, 'epsilon': float(s.eps), 'gain_init': 'one',
                'bias_init': 'zero'}, [prev])
        elif s.kind == 'mha' and getattr(s, 'relative', False):
            name = nm('relativemultiheadattention')
            add('RelativeMultiHeadAttention', name, {
                'name': name, 'trainable': True, 'num_heads': int(s.heads),
                'head_dim': int(s.dh), 'output_dim': int(s.n_out),
                'W_regularizer': _regularizer(s.l2)}, [prev])
            if getattr(s, 'window', None) is not None:    # (only then: every other model's config text is unchanged)
                layers[-1]['config']['context'] = list(s.window)
        elif s.kind == 'mha':
            name = nm('multiheadattention')
            add('MultiHeadAttention', name, {
                'name': name, 'trainable': True, 'num_heads': int(s.heads),
                'head_dim': int(s.dh), 'output_dim': int(s.n_out),
                'W_regularizer': _regularizer(s.l2), 'attention_dropout': 0.0}, [prev])
            if getattr(s, 'window', None) is not None:
                layers[-1]['config']['context'] = list(s.window)
        elif s.kind == 'posenc':
            name = nm('positionalencoding')
            add('PositionalEncoding', name, {'name': name, 'trainable': True}, [prev])
        elif s.kind == 'reshape' and getattr(s, 'time_factor', 0):
            name = nm('timereduction')      # (the 'treduce' variant of the kind)
            add('TimeReduction', name, {'name': name, 'trainable': True,
                                        'factor': int(s.time_factor)}, [prev])
        elif s.kind == 'reshape':
            name = nm('reshape')
            add('Reshape', name, {'name': name, 'trainable': True,
                                  'target_shape': [int(v) for v in s.target]}, [prev])
        elif s.kind == 'conv':
            name = nm('convolution2d')
            add('Convolution2D', name, {
                'name': name, 'trainable': True, 'nb_filter': int(s.C_out), 'nb_row': int(s.kt),
                'nb_col': int(s.kf), 'subsample': [int(s.st), int(s.sf)], 'border_mode': 'same',
                'dim_ordering': 'tf', 'init': 'glorot_uniform',
                # (a Python closure in the reference's style: named, not marshalled)
                'activation': 'clipped_relu' if s.clip > 0 else 'linear',
                'max_value': float(s.clip), 'W_regularizer': _regularizer(s.l2),
                'b_regularizer': None, 'activity_regularizer': None, 'W_constraint': None,
                'b_constraint': None, 'bias': True}, [prev])
        elif s.kind == 'dwconv':
            name = nm('depthwiseconvolution1d')
            add('DepthwiseConvolution1D', name, {
                'name': name, 'trainable': True, 'kernel_size': int(s.k),
                'border_mode': 'same', 'init': 'glorot_uniform',
                'W_regularizer': _regularizer(s.l2), 'bias': True}, [prev])
            if getattr(s, 'pad_left', None) is not None:
                layers[-1]['config']['causal'] = True
        elif s.kind == 'glu':
            name = nm('glu')
            add('GLU', name, {'name': name, 'trainable': True}, [prev])
        elif s.kind == 'merge':
            name = nm('merge')
            cfg = {'name': name, 'mode': s.mode, 'mode_type': 'raw',
                   'concat_axis': -1, 'dot_axes': -1, 'output_shape': None,
                   'output_shape_type': 'raw', 'output_mask': None,
                   'output_mask_type': 'raw', 'arguments': {}}
            if s.scale != 1.0:      # (only then: every other model's config text is unchanged)
                cfg['scale'] = float(s.scale)
            add('Merge', name, cfg, [prev, out_names[s.skip]])
        else:
            raise ValueError(s.kind)
        out_names.append(name)
        prev = name
    add('InputLayer', 'labels', {'batch_input_shape': [None, None], 'input_dtype': 'int32',
                                 'sparse': True, 'name': 'labels'}, [])
    add('InputLayer', 'inputs_length', {'batch_input_shape': [None, None], 'input_dtype': 'int32',
                                        'sparse': False, 'name': 'inputs_length'}, [])
    # (a language model is a decode-time argument, not part of the model file)
    dec = {k: v for k, v in (model.decoder or {'is_greedy': True}).items()
           if k not in ('lm', 'lm_alpha', 'lm_beta')}
    add('Lambda', 'decoder', _lambda_config('decoder', 'decode',
                                             ('decode_output_shape', 'function'),
                                             {k: dec[k] for k in sorted(dec)}),
        [prev, 'inputs_length'])
    add('Lambda', 'ctc', _lambda_config('ctc', 'ctc_lambda_func', ([1], 'raw'), {}),
        [prev, 'labels', 'inputs_length'])
    cfg = {'class_name': 'Model', 'config': {
        'name': 'model_1', 'layers': layers,
        'input_layers': [['inputs', 0, 0], ['labels', 0, 0], ['inputs_length', 0, 0]],
        'output_layers': [['ctc', 0, 0], ['decoder', 0, 0]]}}
    return json.dumps(cfg)


def training_config(model):
    """The ``training_config`` JSON string (train.py:133-143) or None without an optimizer."""
    opt = model.optimizer
    if opt is None:
        return None
    if type(opt).__name__ == 'Adam':
        oc = {'lr': float(opt.lr), 'beta_1': float(opt.beta_1), 'beta_2': float(opt.beta_2),
              'epsilon': float(opt.epsilon), 'decay': float(getattr(opt, 'decay', 0.0))}
    else:
        oc = {'lr': float(opt.lr), 'momentum': float(opt.momentum),
              'decay': float(getattr(opt, 'decay', 0.0)),
              'nesterov': False}
    if opt.clipnorm:
        oc['clipnorm'] = float(opt.clipnorm)
    return json.dumps({
        'optimizer_config': {'class_name': type(opt).__name__, 'config': oc},
        'loss': {'ctc': 'ctc_dummy_loss', 'decoder': 'decoder_dummy_loss'},
        'metrics': {'decoder': 'ler'}, 'sample_weight_mode': None, 'loss_weights': [1, 0]})


def optimizer_weights(model):
    """[(name, array)]: Keras' ``optimizer.get_weights()`` = [iterations] + one slot tensor per
    trainable weight and state (Adam: all m then all v), in get_weights() order / layout."""
    import numpy as np
    opt = model.optimizer
    if opt is None or not getattr(opt, 'state', None):
        return []
    out = [('iterations:0', np.asarray(float(opt.iterations), np.float32))]
    i = 0
    for st in opt.state:
        for a in model._unpack(st.detach().cpu().numpy()):
            out.append(('param_%d' % i, np.ascontiguousarray(a, np.float32)))
            i += 1
    return out


def topology_from_config(text):
    """Rebuilds the build's model from a Keras ``model_config`` JSON (a chain of the layer
    kinds core/models.py uses, with optional residual Merges): -> engine.Model."""
    from ..core import layers as L
    from ..core.models import ctc_model
    cfg = json.loads(text)
    if cfg.get('class_name') != 'Model':
        raise ValueError('model_config: expected a functional Model, got %r' % cfg.get('class_name'))
    by_name = {l['name']: l for l in cfg['config']['layers']}
    dec = by_name.get('decoder', {}).get('config', {}).get('arguments', {}) or {}
    # the acoustic output feeds the ctc Lambda as its first input
    ctc_in = by_name['ctc']['inbound_nodes'][0][0][0]
    order, cur = [], ctc_in
    while by_name[cur]['class_name'] != 'InputLayer':
        order.append(cur)
        cur = by_name[cur]['inbound_nodes'][0][0][0]
    inp = by_name[cur]['config']
    x = L.Input(name=inp['name'], shape=tuple(inp['batch_input_shape'][1:]))
    syms = {cur: x}
    o = x

    def reg(c):
        return L.l2(c['l2']) if c else None
    for name in reversed(order):
        l = by_name[name]
        c = l['config']
        kind = l['class_name']
        if kind == 'GaussianNoise':
            o = L.GaussianNoise(c['sigma'])(o)
        elif kind == 'SpecAugment':
            o = L.SpecAugment(**{k: c[k] for k in L.SpecAugment.POLICY if k in c})(o)
        elif kind == 'Reshape':
            o = L.Reshape(tuple(c['target_shape']))(o)
        elif kind == 'Convolution2D':
            act = L.clipped_relu(c.get('max_value', 20.0)) if c.get('activation') == 'clipped_relu' \
                else None
            o = L.Convolution2D(c['nb_filter'], c['nb_row'], c['nb_col'],
                                subsample=tuple(c['subsample']), border_mode=c['border_mode'],
                                activation=act, W_regularizer=reg(c.get('W_regularizer')),
                                dim_ordering=c.get('dim_ordering', 'tf'))(o)
        elif kind == 'Dropout':
            o = L.Dropout(c['p'])(o)
        elif kind == 'Activation':
            o = L.Activation(_act_from(c))(o)
        elif kind == 'BatchNormalization':
            o = L.BatchNormalization(epsilon=c.get('epsilon', 1e-3), mode=c.get('mode', 0),
                                     axis=c.get('axis', -1), momentum=c.get('momentum', 0.99))(o)
        elif kind == 'LayerNormalization':
            o = L.LayerNormalization(epsilon=c.get('epsilon', 1e-5),
                                     gain_init=c.get('gain_init', 'one'),
                                     bias_init=c.get('bias_init', 'zero'))(o)
        elif kind == 'MultiHeadAttention':
            o = L.MultiHeadAttention(c['num_heads'], head_dim=c.get('head_dim'),
                                     output_dim=c.get('output_dim'),
                                     W_regularizer=reg(c.get('W_regularizer')),
                                     attention_dropout=c.get('attention_dropout', 0.),
                                     context=c.get('context'))(o)
        elif kind == 'RelativeMultiHeadAttention':
            o = L.RelativeMultiHeadAttention(c['num_heads'], head_dim=c.get('head_dim'),
                                             output_dim=c.get('output_dim'),
                                             W_regularizer=reg(c.get('W_regularizer')),
                                             context=c.get('context'))(o)
        elif kind == 'PositionalEncoding':
            o = L.PositionalEncoding()(o)
        elif kind == 'DepthwiseConvolution1D':
            o = L.DepthwiseConvolution1D(c['kernel_size'],
                                         W_regularizer=reg(c.get('W_regularizer')),
                                         causal=c.get('causal', False))(o)
        elif kind == 'GLU':
            o = L.GLU()(o)
        elif kind == 'TimeReduction':
            o = L.TimeReduction(c['factor'])(o)
        elif kind == 'TimeDistributed' and c['layer']['class_name'] == 'Activation':
            o = L.TimeDistributed(L.Activation(_act_from(c['layer']['config'])))(o)
        elif kind == 'TimeDistributed' and c['layer']['class_name'] == 'Dropout':
            o = L.TimeDistributed(L.Dropout(c['layer']['config']['p']))(o)
        elif kind == 'Bidirectional' and c['layer']['class_name'] == 'SimpleRNN':
            r = c['layer']['config']
            o = L.Bidirectional(L.SimpleRNN(
                r['output_dim'], init=r.get('init', 'glorot_uniform'),
                inner_init=r.get('inner_init', 'orthogonal'), activation=_act_from(r),
                W_regularizer=reg(r.get('W_regularizer')), U_regularizer=reg(r.get('U_regularizer')),
                dropout_W=r.get('dropout_W', 0.), dropout_U=r.get('dropout_U', 0.)),
                merge_mode=c.get('merge_mode', 'concat'))(o)
        elif kind == 'Bidirectional' and c['layer']['class_name'] == 'GRU':
            r = c['layer']['config']
            o = L.Bidirectional(L.GRU(
                r['output_dim'], init=r.get('init', 'glorot_uniform'),
                inner_init=r.get('inner_init', 'orthogonal'), activation=_act_from(r),
                inner_activation=r.get('inner_activation', 'hard_sigmoid'),
                W_regularizer=reg(r.get('W_regularizer')), U_regularizer=reg(r.get('U_regularizer')),
                dropout_W=r.get('dropout_W', 0.), dropout_U=r.get('dropout_U', 0.),
                consume_less=r.get('consume_less', 'gpu'),
                batch_norm=bool(r.get('batch_norm', False)), bn_epsilon=r.get('bn_epsilon', 1e-3),
                bn_momentum=r.get('bn_momentum', 0.99)),
                merge_mode=c.get('merge_mode', 'concat'))(o)
        elif kind == 'GRU':
            o = L.GRU(
                c['output_dim'], init=c.get('init', 'glorot_uniform'),
                inner_init=c.get('inner_init', 'orthogonal'), activation=_act_from(c),
                inner_activation=c.get('inner_activation', 'hard_sigmoid'),
                W_regularizer=reg(c.get('W_regularizer')), U_regularizer=reg(c.get('U_regularizer')),
                dropout_W=c.get('dropout_W', 0.), dropout_U=c.get('dropout_U', 0.),
                consume_less=c.get('consume_less', 'gpu'))(o)
        elif kind == 'LSTM':
            o = L.LSTM(
                c['output_dim'], zoneout_h=c.get('zoneout_h', 0.), zoneout_c=c.get('zoneout_c', 0.),
                layer_norm=c.get('layer_norm'), mi=c.get('mi'),
                W_regularizer=reg(c.get('W_regularizer')), U_regularizer=reg(c.get('U_regularizer')),
                dropout_W=c.get('dropout_W', 0.), dropout_U=c.get('dropout_U', 0.),
                activation=c.get('activation', 'tanh'),
                inner_activation=c.get('inner_activation', 'hard_sigmoid'))(o)
        elif kind == 'Bidirectional' and c['layer']['class_name'] == 'RHN':
            r = c['layer']['config']
            o = L.Bidirectional(L.RHN(
                r['output_dim'], depth=r.get('depth', 1), init=r.get('init', 'glorot_uniform'),
                inner_init=r.get('inner_init', 'orthogonal'),
                bias_init=r.get('bias_init', 'highway_bias_initializer'),
                activation=_act_from(r),
                inner_activation=r.get('inner_activation', 'hard_sigmoid'),
                coupling=r.get('coupling', True), layer_norm=r.get('layer_norm', False),
                mi=r.get('mi', False),
                W_regularizer=reg(r.get('W_regularizer')), U_regularizer=reg(r.get('U_regularizer')),
                dropout_W=r.get('dropout_W', 0.), dropout_U=r.get('dropout_U', 0.)),
                merge_mode=c.get('merge_mode', 'concat'))(o)
        elif kind == 'TimeDistributed':
            d = c['layer']['config']
            o = L.TimeDistributed(L.Dense(d['output_dim'], W_regularizer=reg(d.get('W_regularizer')),
                                          activation=d.get('activation')))(o)
        elif kind == 'Bidirectional':
            r = c['layer']['config']
            o = L.Bidirectional(L.LSTM(
                r['output_dim'], zoneout_h=r.get('zoneout_h', 0.), zoneout_c=r.get('zoneout_c', 0.),
                layer_norm=r.get('layer_norm'), mi=r.get('mi'),
                W_regularizer=reg(r.get('W_regularizer')), U_regularizer=reg(r.get('U_regularizer')),
                dropout_W=r.get('dropout_W', 0.), dropout_U=r.get('dropout_U', 0.),
                activation=r.get('activation', 'tanh'),
                inner_activation=r.get('inner_activation', 'hard_sigmoid')),
                merge_mode=c.get('merge_mode', 'concat'))(o)
        elif kind == 'Merge':
            other = l['inbound_nodes'][0][1][0]
            o = L.merge([o, syms[other]], mode=c['mode'], scale=c.get('scale', 1.0))
        else:
            raise NotImplementedError('model_config: layer class %r' % kind)
        syms[name] = o
    return ctc_model(x, o, **{k: v for k, v in dec.items()
                              if k in ('is_greedy', 'beam_width', 'merge_repeated', 'top_paths')})
