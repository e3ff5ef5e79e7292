"""Model factories with the reference's names and hyper-parameters
(core/models.py): ``ctc_model``, ``graves2006``, ``eyben``, ``maas``, ``deep_speech``,
``brsmv1``, plus this build's ``deep_speech2`` (BiLSTM or, with ``rnn_type='gru'``, BiGRU) and
``rhn`` (brsmv1's topology on the reference's own RHN cell) and ``transformer`` (a pre-LN
self-attention encoder, csrc/attention.hip) and ``conformer`` (arXiv 2005.08100, csrc/dwconv.hip).
The last three take ``spec_augment`` (a SpecAugment layer behind Input, csrc/specaug.hip).

``train.py`` resolves them by name -- ``get_from_module('core.models', 'brsmv1')
(**hparams)`` (train.py:127-129) -- and gets back an object with the Keras
``compile / fit_generator / evaluate_generator / metrics_names / optimizer.lr``
surface; here that object is core.engine.Model, which runs on the HIP kernels.
``maas`` and ``deep_speech`` are dead code in the reference (they use ``Activation`` and
``SimpleRNN`` without importing them); here they run on the SimpleRNN kernels of csrc/rnn.hip
with the reference's signatures, defaults and layer sequence.
"""
from . import ctc_utils
from .engine import Model
from .layers import (Input, GaussianNoise, TimeDistributed, Dense, LSTM, Bidirectional,
                     Dropout, Merge, merge, l2, Reshape, Convolution2D, clipped_relu, SimpleRNN,
                     Activation, BatchNormalization, GRU, RHN, LayerNormalization,
                     MultiHeadAttention, RelativeMultiHeadAttention, PositionalEncoding,
                     DepthwiseConvolution1D, GLU, SpecAugment, TimeReduction)


def ctc_model(inputs, output, **kwargs):
    """Given the symbolic input and the (N, T, C) logit tensor of a user-built
    topology, returns the trainable CTC model: inputs ``[inputs, labels,
    inputs_length]``, outputs ``[ctc, decoder]`` (core/models.py:31-52).

    kwargs: ``is_greedy`` / ``beam_width`` / ``merge_repeated`` for the decoder
    (core/ctc_utils.py:8-52) and ``lm`` / ``lm_alpha`` / ``lm_beta`` for a character language
    model in the beam search (asr_study_amd.lm), ``device``, ``seed``.
    """
    root, chain = output.chain()
    if root is not inputs:
        raise ValueError('output is not connected to inputs')
    spec = []
    # outputs[i] = the symbolic tensor stage i produces (to resolve merge() skip inputs)
    outputs, cur = [], output
    while cur.producer is not None:
        outputs.append(cur)
        cur = cur.parent
    outputs = outputs[::-1]
    for layer in chain:
        if isinstance(layer, Merge):
            if layer.skip is inputs:
                raise NotImplementedError('merge with the raw model input')
            src = [i for i, t in enumerate(outputs) if t is layer.skip]
            if not src:
                raise ValueError('merge: the skip input is not on the path from inputs')
            spec.append({'type': 'merge', 'mode': layer.mode, 'skip': src[0]})
            if layer.scale != 1.0:  # (only then: the spec of every other model is unchanged)
                spec[-1]['scale'] = layer.scale
        elif isinstance(layer, TimeReduction):
            # batch major, stacking k frames is Reshape((-1, k F)) of an utterance's (T, F) block:
            # the 'treduce' variant of the kind (the key only then, as for merge)
            spec.append({'type': 'reshape', 'target': [-1, outputs[len(spec)].features],
                         'time_factor': layer.factor})
        elif isinstance(layer, Reshape):
            spec.append({'type': 'reshape', 'target': list(layer.target)})   # a view: no data moves
        elif isinstance(layer, Convolution2D):
            spec.append({'type': 'conv', 'F_in': layer.in_fc[0], 'C_in': layer.in_fc[1],
                         'C_out': layer.nb_filter, 'kt': layer.kt, 'kf': layer.kf,
                         'st': layer.st, 'sf': layer.sf, 'clip': layer.clip, 'l2': layer.l2})
        elif isinstance(layer, GaussianNoise):
            spec.append({'type': 'noise', 'value': layer.sigma})
        elif isinstance(layer, SpecAugment):
            spec.append(dict({'type': 'specaug'}, **layer.policy()))
        elif isinstance(layer, BatchNormalization):
            spec.append({'type': 'bn', 'epsilon': layer.epsilon, 'momentum': layer.momentum,
                         'fc': None if layer.in_fc is None else list(layer.in_fc)})
        elif isinstance(layer, LayerNormalization):
            spec.append({'type': 'ln', 'epsilon': layer.epsilon})
        elif isinstance(layer, MultiHeadAttention):
            spec.append({'type': 'mha', 'heads': layer.num_heads, 'dh': layer.head_dim,
                         'n_out': layer.output_dim, 'l2': layer.l2})
            if isinstance(layer, RelativeMultiHeadAttention):   # (only then: as for merge)
                spec[-1]['relative'] = True
            if layer.context is not None:
                spec[-1]['context'] = list(layer.context)
        elif isinstance(layer, PositionalEncoding):
            spec.append({'type': 'posenc'})
        elif isinstance(layer, DepthwiseConvolution1D):
            spec.append({'type': 'dwconv', 'k': layer.kernel_size, 'l2': layer.l2})
            if layer.causal:
                spec[-1]['causal'] = True
        elif isinstance(layer, GLU):
            spec.append({'type': 'glu'})
        elif isinstance(layer, TimeDistributed) and layer.dense is None:
            spec.append(_elementwise_spec(layer.layer, wrapped=True))
        elif isinstance(layer, (Dropout, Activation)):
            spec.append(_elementwise_spec(layer))
        elif isinstance(layer, TimeDistributed):
            spec.append({'type': 'dense', 'n_out': layer.dense.output_dim, 'l2': layer.dense.l2})
        elif isinstance(layer, Bidirectional) and isinstance(layer.lstm, SimpleRNN):
            r = layer.lstm
            spec.append({'type': 'birnn', 'H': r.output_dim, 'merge_mode': layer.merge_mode,
                         'activation': r.activation, 'init': r.init, 'dropout_W': r.dropout_W,
                         'dropout_U': r.dropout_U, 'l2_W': r.l2_W, 'l2_U': r.l2_U})
        elif isinstance(layer, Bidirectional) and isinstance(layer.lstm, GRU):
            r = layer.lstm
            spec.append({'type': 'bigru', 'H': r.output_dim, 'merge_mode': layer.merge_mode,
                         'activation': r.activation, 'dropout_W': r.dropout_W,
                         'dropout_U': r.dropout_U, 'l2_W': r.l2_W, 'l2_U': r.l2_U})
            if r.batch_norm:        # (only then: the spec of every other model is unchanged)
                spec[-1].update(batch_norm=True, bn_epsilon=r.bn_epsilon,
                                bn_momentum=r.bn_momentum)
        elif isinstance(layer, GRU):
            # a bare GRU: the one-direction variant of the kind (the key only then, and no
            # merge_mode: there is nothing to merge)
            spec.append({'type': 'bigru', 'H': layer.output_dim, 'activation': layer.activation,
                         'dropout_W': layer.dropout_W, 'dropout_U': layer.dropout_U,
                         'l2_W': layer.l2_W, 'l2_U': layer.l2_U, 'directions': 1})
        elif isinstance(layer, LSTM):
            # a bare LSTM (K29): the one-direction variant of the kind (the key only then; the
            # variant keys mi / zoneout / layer_norm are left out: LSTM.__call__ refused them)
            spec.append({'type': 'bilstm', 'H': layer.output_dim, 'dropout_W': layer.dropout_W,
                         'dropout_U': layer.dropout_U, 'l2_W': layer.l2_W, 'l2_U': layer.l2_U,
                         'activation': layer.activation, 'directions': 1})
        elif isinstance(layer, Bidirectional) and isinstance(layer.lstm, RHN):
            r = layer.lstm
            spec.append({'type': 'birhn', 'H': r.output_dim, 'depth': r.depth,
                         'coupling': r.coupling, 'merge_mode': layer.merge_mode,
                         'activation': r.activation, 'dropout_W': r.dropout_W,
                         'dropout_U': r.dropout_U, 'l2_W': r.l2_W, 'l2_U': r.l2_U})
        elif isinstance(layer, Bidirectional):
            r = layer.lstm
            spec.append({'type': 'bilstm', 'H': r.output_dim, 'dropout_W': r.dropout_W,
                         'dropout_U': r.dropout_U, 'l2_W': r.l2_W, 'l2_U': r.l2_U,
                         'mi': r.mi, 'zoneout_c': r.zoneout_c, 'zoneout_h': r.zoneout_h,
                         'layer_norm': r.layer_norm, 'activation': r.activation})
        else:
            raise NotImplementedError(type(layer).__name__)
    model = Model(spec, inputs.features, device=kwargs.get('device'),
                  seed=kwargs.get('seed', 0))
    model.decoder = ctc_utils.decoder_config(**{k: v for k, v in kwargs.items()
                                                if k in ('is_greedy', 'beam_width',
                                                         'merge_repeated', 'top_paths', 'lm',
                                                         'lm_alpha', 'lm_beta')})
    return model


def _elementwise_spec(layer, wrapped=False):
    """Dropout / Activation, bare or inside TimeDistributed (``wrapped``: kept for the Keras
    config writer; the arithmetic is the same)."""
    if isinstance(layer, Dropout):
        return {'type': 'dropout', 'value': layer.p, 'wrapped': wrapped}
    return {'type': 'act', 'activation': layer.activation, 'wrapped': wrapped}


def _spec_augment(o, spec_augment):
    """The ``spec_augment`` argument of a factory, applied to the symbolic input ``o``: False /
    None (no layer), True (SpecAugment() with its defaults, the Conformer paper's policy) or a
    dict of its keyword arguments."""
    if spec_augment is False or spec_augment is None:
        return o
    if spec_augment is not True and not isinstance(spec_augment, dict):
        raise ValueError('spec_augment=%r: False, True or a dict of SpecAugment arguments'
                         % (spec_augment,))
    return SpecAugment(**({} if spec_augment is True else spec_augment))(o)


def _record_spec_augment(model, spec_augment):
    """... and recorded in the factory record only when set (a default model keeps its config)."""
    if spec_augment is not False and spec_augment is not None:
        model.config['kwargs']['spec_augment'] = (True if spec_augment is True
                                                  else dict(spec_augment))


def _attention_layer(factory, positions):
    """The ``positions`` argument of a factory: the attention layer class of its blocks."""
    if positions not in ('absolute', 'relative'):
        raise ValueError("%s(positions=%r): 'absolute' or 'relative'" % (factory, positions))
    return RelativeMultiHeadAttention if positions == 'relative' else MultiHeadAttention


def _record_positions(model, positions):
    """... recorded in the factory record only when not the default, like spec_augment."""
    if positions != 'absolute':
        model.config['kwargs']['positions'] = positions


def _record_context(model, context, causal_conv=False):
    """... and so are the attention window (as the layer normalised it: a list of three integers)
    and the causal convolution."""
    if context is not None:
        model.config['kwargs']['context'] = list(MultiHeadAttention._check_context(context))
    if causal_conv:
        model.config['kwargs']['causal_conv'] = True


def _time_reduction(factory, time_reduction, num_layers):
    """The ``time_reduction`` argument of a recurrent factory, [[after_layer, factor], ...], as
    {after_layer: factor}: after_layer = 0 puts the TimeReduction in front of the first
    recurrent layer, i behind recurrent layer i; 0 <= i < num_layers, strictly increasing."""
    if time_reduction is None:
        return {}
    try:
        pairs = [(a, f) for a, f in time_reduction]
        ok = bool(pairs) and all(not isinstance(v, bool) and int(v) == v for p in pairs for v in p)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('%s(time_reduction=%r): None or a list of [after_layer, factor] pairs '
                         'of integers' % (factory, time_reduction))
    last = -1
    for a, f in pairs:
        if not last < a < num_layers:
            raise ValueError('%s(time_reduction=%r): after_layer %d (0: in front of the first '
                             'recurrent layer, i: behind layer i; 0 <= i < num_layers = %d, '
                             'strictly increasing)' % (factory, time_reduction, a, num_layers))
        last = a
    return {int(a): int(f) for a, f in pairs}


def _single_factor(factory, time_reduction):
    """The ``time_reduction`` argument of transformer / conformer: one integer factor."""
    if isinstance(time_reduction, bool) or not isinstance(time_reduction, int):
        raise ValueError('%s(time_reduction=%r): None or one integer factor (the stage goes in '
                         'front of the input projection)' % (factory, time_reduction))
    return time_reduction


def _record_time_reduction(model, time_reduction):
    """... recorded in the factory record only when set (a default checkpoint keeps its bytes)."""
    if time_reduction is not None:
        model.config['kwargs']['time_reduction'] = (
            int(time_reduction) if isinstance(time_reduction, int)
            else [[int(a), int(f)] for a, f in time_reduction])


def graves2006(num_features=26, num_hiddens=100, num_classes=28, std=.6, **kw):
    """Graves et al. 2006 (core/models.py:55-73)."""
    x = Input(name='inputs', shape=(None, num_features))
    o = x
    o = GaussianNoise(std)(o)
    o = Bidirectional(LSTM(num_hiddens, return_sequences=True, consume_less='gpu'))(o)
    o = TimeDistributed(Dense(num_classes))(o)
    model = ctc_model(x, o, **kw)
    model.config = {'name': 'graves2006', 'kwargs': dict(
        num_features=num_features, num_hiddens=num_hiddens, num_classes=num_classes, std=std)}
    return model


def eyben(num_features=39, num_hiddens=[78, 120, 27], num_classes=28, **kw):
    """Eyben et al. 2009 (core/models.py:76-103)."""
    assert len(num_hiddens) == 3
    x = Input(name='inputs', shape=(None, num_features))
    o = x
    if num_hiddens[0]:
        o = TimeDistributed(Dense(num_hiddens[0]))(o)
    if num_hiddens[1]:
        o = Bidirectional(LSTM(num_hiddens[1], return_sequences=True, consume_less='gpu'))(o)
    if num_hiddens[2]:
        o = Bidirectional(LSTM(num_hiddens[2], return_sequences=True, consume_less='gpu'))(o)
    o = TimeDistributed(Dense(num_classes))(o)
    model = ctc_model(x, o, **kw)
    model.config = {'name': 'eyben', 'kwargs': dict(
        num_features=num_features, num_hiddens=list(num_hiddens), num_classes=num_classes)}
    return model


def maas(num_features=81, num_classes=29, num_hiddens=1824, dropout=0.1, max_value=20, **kw):
    """Maas et al. 2015, "Lexicon-free conversational speech recognition with neural networks"
    (core/models.py:106-145): two clipped-ReLU Dense layers, a summed Bidirectional SimpleRNN
    with input dropout, two more clipped-ReLU Dense layers, the output Dense."""
    x = Input(name='inputs', shape=(None, num_features))
    act = clipped_relu(max_value)
    o = x
    for _ in range(2):
        o = TimeDistributed(Dense(num_hiddens))(o)
        o = TimeDistributed(Activation(act))(o)
    o = Bidirectional(SimpleRNN(num_hiddens, return_sequences=True, dropout_W=dropout,
                                activation=act, init='he_normal'), merge_mode='sum')(o)
    for _ in range(2):
        o = TimeDistributed(Dense(num_hiddens))(o)
        o = TimeDistributed(Activation(act))(o)
    o = TimeDistributed(Dense(num_classes))(o)
    model = ctc_model(x, o, **kw)
    model.config = {'name': 'maas', 'kwargs': dict(
        num_features=num_features, num_classes=num_classes, num_hiddens=num_hiddens,
        dropout=dropout, max_value=max_value)}
    return model


def deep_speech(num_features=81, num_classes=29, num_hiddens=2048, dropout=0.1, max_value=20,
                **kw):
    """Hannun et al. 2014, "Deep Speech: scaling up end-to-end speech recognition"
    (core/models.py:148-214): three clipped-ReLU Dense layers with dropout, a summed
    Bidirectional SimpleRNN with input dropout and dropout behind it, one more clipped-ReLU
    Dense layer with dropout, the output Dense."""
    x = Input(name='inputs', shape=(None, num_features))
    act = clipped_relu(max_value)
    o = x
    for _ in range(3):
        o = TimeDistributed(Dense(num_hiddens))(o)
        o = TimeDistributed(Activation(act))(o)
        o = TimeDistributed(Dropout(dropout))(o)
    o = Bidirectional(SimpleRNN(num_hiddens, return_sequences=True, dropout_W=dropout,
                                activation=act, init='he_normal'), merge_mode='sum')(o)
    o = TimeDistributed(Dropout(dropout))(o)
    o = TimeDistributed(Dense(num_hiddens))(o)
    o = TimeDistributed(Activation(act))(o)
    o = TimeDistributed(Dropout(dropout))(o)
    o = TimeDistributed(Dense(num_classes))(o)
    model = ctc_model(x, o, **kw)
    model.config = {'name': 'deep_speech', 'kwargs': dict(
        num_features=num_features, num_classes=num_classes, num_hiddens=num_hiddens,
        dropout=dropout, max_value=max_value)}
    return model


def brsmv1(num_features=39, num_classes=28, num_hiddens=256, num_layers=5,
           dropout=0.2, zoneout=0., input_dropout=False, input_std_noise=.0,
           weight_decay=1e-4, residual=None, layer_norm=None, mi=None,
           activation='tanh', bidirectional=True, time_reduction=None, **kw):
    """BRSM v1.0 (core/models.py:217-281), same defaults.

    time_reduction=[[after_layer, factor], ...] (no reference counterpart, K33): a
    TimeReduction(factor) in front of the first recurrent layer (after_layer = 0) or behind
    recurrent layer ``after_layer`` (0 <= after_layer < num_layers, strictly increasing): the
    layers behind it, the logits and CTC run on ceil(T / factor) frames of factor times the
    width -- the pyramid of arXiv 1508.01211 with [[1, 2], [2, 2]], the time-reduction layer of
    RNN-T encoders with [[2, 2]], stacked input frames with [[0, 3]].  ``inputs_length`` is mapped
    inside the model.  With ``residual`` the stage is followed by a TimeDistributed(Dense) of the
    recurrent width, so that the skip widths agree (no skip spans the stage).

    bidirectional=False (no reference counterpart, K29): every layer is a bare, unidirectional
    LSTM(num_hiddens) on csrc/lstm_uni.hip and the ``residual`` Dense is num_hiddens wide; zoneout,
    mi and layer_norm are refused.  Such a model has no look-ahead: Model.stream runs it chunk by
    chunk."""
    if not bidirectional:
        for name, on in (('zoneout', zoneout and zoneout > 0), ('mi', mi is not None),
                         ('layer_norm', layer_norm is not None)):
            if on:
                raise NotImplementedError('brsmv1: bidirectional=False with %s: the unidirectional '
                                          'LSTM is the plain cell only' % name)
    width = num_hiddens * 2 if bidirectional else num_hiddens
    reduce_at = _time_reduction('brsmv1', time_reduction, num_layers)
    x = Input(name='inputs', shape=(None, num_features))
    o = x
    if input_std_noise is not None:
        o = GaussianNoise(input_std_noise)(o)
    if residual is not None:
        o = TimeDistributed(Dense(width, W_regularizer=l2(weight_decay)))(o)
    if input_dropout:
        o = Dropout(dropout)(o)
    for i, _ in enumerate(range(num_layers)):
        if i in reduce_at:
            o = TimeReduction(reduce_at[i])(o)
            if residual is not None:
                o = TimeDistributed(Dense(width, W_regularizer=l2(weight_decay)))(o)
        cell = LSTM(num_hiddens,
                    return_sequences=True,
                    W_regularizer=l2(weight_decay),
                    U_regularizer=l2(weight_decay),
                    dropout_W=dropout,
                    dropout_U=dropout,
                    zoneout_c=zoneout,
                    zoneout_h=zoneout,
                    mi=mi,
                    layer_norm=layer_norm,
                    activation=activation)
        new_o = Bidirectional(cell)(o) if bidirectional else cell(o)
        if residual is not None:
            o = merge([new_o, o], mode=residual)
        else:
            o = new_o
    o = TimeDistributed(Dense(num_classes, W_regularizer=l2(weight_decay)))(o)
    model = ctc_model(x, o, **kw)
    model.config = {'name': 'brsmv1', 'kwargs': dict(
        num_features=num_features, num_classes=num_classes, num_hiddens=num_hiddens,
        num_layers=num_layers, dropout=dropout, zoneout=zoneout, input_dropout=input_dropout,
        input_std_noise=input_std_noise, weight_decay=weight_decay, residual=residual,
        layer_norm=layer_norm, mi=mi, activation=activation)}
    if not bidirectional:   # (only then: default checkpoints keep their bytes)
        model.config['kwargs']['bidirectional'] = False
    _record_time_reduction(model, time_reduction)
    return model


def deep_speech2(num_features=80, num_classes=28, num_hiddens=512, num_layers=5,
                 conv_filters=32, conv_kernels=((11, 41), (11, 21)), conv_strides=((2, 2), (1, 2)),
                 max_value=20, dropout=0.2, weight_decay=1e-4, input_std_noise=.0,
                 batch_norm=False, rnn_type='lstm', spec_augment=False, bidirectional=True,
                 time_reduction=None, **kw):
    """BASELINE.json configs[2]: "DeepSpeech2-style 5xBiLSTM(512) + 2 conv front-end, 80-dim
    log-mel".  NO REFERENCE COUNTERPART: the reference lists Deep Speech 2 as TODO
    (README.md:118) and its ``deep_speech`` factory (core/models.py:148-214) is dead code
    (un-imported Keras names) without convolutions.  Built from the reference's own pieces:
    brsmv1's recurrent stack and regularisers (core/models.py:217-281), the ``clipped_relu``
    of its Deep Speech factories (:116-117), and two Keras Convolution2D layers over (time,
    frequency) with DeepSpeech2's filter shapes -- 32 x (11 x 41) stride (2, 2) and
    32 x (11 x 21) stride (1, 2), 'same' padding -- so the recurrent stack sees T/2 frames of
    F/4 * 32 features.  ``inputs_length`` is mapped to ceil(len / 2) inside the model.

    batch_norm=True: each Convolution2D becomes linear and is followed by BatchNormalization
    (per channel) and Activation(clipped_relu(max_value)); a BatchNormalization also goes in
    front of every Bidirectional(LSTM).  That normalises the layer INPUT x, not the input
    projection W x of the published Deep Speech 2 (sequence-wise BN inside the recurrent layer),
    and its statistics include the time-padding frames, as Keras sees the zero-padded batch.

    batch_norm='recurrent' (with rnn_type='gru' only): the convolution blocks as with
    batch_norm=True, no BatchNormalization in front of the recurrent layers, and every
    GRU(batch_norm=True): the published form, sequence-wise batch normalisation of the input
    projection W x inside the layer, its statistics taken over the valid frames of every utterance
    (the time-padding frames count for nothing; arXiv 1510.01378).

    batch_norm='layer' (with either rnn_type): LayerNormalization where batch_norm=True puts
    BatchNormalization -- behind each (linear) Convolution2D, over the whole F * C vector of a
    frame, followed by Activation(clipped_relu(max_value)), and in front of every recurrent
    layer.  Per frame: no batch statistics, no running state, the same result at any batch size.

    rnn_type='gru': every Bidirectional(LSTM) becomes a Bidirectional(GRU) (the cell of the
    published Deep Speech 2; Keras-1.2.2 GRU on csrc/gru.hip) with the same regularisers and
    dropouts; it composes with batch_norm.

    spec_augment=True (or a dict of its arguments): a SpecAugment layer directly behind Input.

    bidirectional=False (with rnn_type='gru' only): every recurrent layer is a bare, unidirectional
    GRU of width num_hiddens (the deployment form of Deep Speech 2) and the Dense reads num_hiddens
    features; batch_norm False, True and 'layer' compose as above.  Such a model has no look-ahead
    behind its convolutions: with batch_norm=False, Model.stream runs it chunk by chunk.

    time_reduction=[[after_layer, factor], ...]: brsmv1's argument -- a TimeReduction(factor) in
    front of the first recurrent layer (0; in front of its normalisation, if any) or behind
    recurrent layer ``after_layer``, on top of the front-end's time stride; the statistics of a
    GRU(batch_norm=True) behind it run over the valid frames of its own, reduced axis."""
    if rnn_type not in ('lstm', 'gru'):
        raise ValueError("deep_speech2: rnn_type %r ('lstm' or 'gru')" % (rnn_type,))
    if not bidirectional and rnn_type != 'gru':
        raise ValueError("deep_speech2: bidirectional=False needs rnn_type='gru': this factory "
                         "wires only the GRU one-directionally (the unidirectional LSTM is a "
                         "bare LSTM layer, brsmv1(bidirectional=False))")
    if batch_norm not in (False, True, 'recurrent', 'layer'):
        raise ValueError("deep_speech2: batch_norm %r (False, True, 'recurrent' or 'layer')"
                         % (batch_norm,))
    recurrent_bn = batch_norm == 'recurrent'
    norm = LayerNormalization if batch_norm == 'layer' else BatchNormalization
    if recurrent_bn and rnn_type != 'gru':
        raise ValueError("deep_speech2: batch_norm='recurrent' needs rnn_type='gru': only the GRU "
                         "layer normalises its input projection (LSTM has no batch_norm argument)")
    if not bidirectional and recurrent_bn:
        raise NotImplementedError("deep_speech2: bidirectional=False with batch_norm='recurrent': "
                                  "a bare GRU has no sequence-wise batch normalisation")
    cell = GRU if rnn_type == 'gru' else LSTM
    cell_kw = dict(batch_norm=True) if recurrent_bn else {}
    reduce_at = _time_reduction('deep_speech2', time_reduction, num_layers)
    x = Input(name='inputs', shape=(None, num_features))
    o = _spec_augment(x, spec_augment)
    if input_std_noise is not None:
        o = GaussianNoise(input_std_noise)(o)
    o = Reshape((-1, num_features, 1))(o)
    for (kt, kf), (st, sf) in zip(conv_kernels, conv_strides):
        o = Convolution2D(conv_filters, kt, kf, subsample=(st, sf), border_mode='same',
                          activation=None if batch_norm else clipped_relu(max_value),
                          W_regularizer=l2(weight_decay))(o)
        if batch_norm:
            o = norm()(o)
            o = Activation(clipped_relu(max_value))(o)
    o = Reshape((-1, o.features))(o)
    for i in range(num_layers):
        if i in reduce_at:
            o = TimeReduction(reduce_at[i])(o)
        if batch_norm and not recurrent_bn:
            o = norm()(o)
        rec = cell(num_hiddens, return_sequences=True,
                   W_regularizer=l2(weight_decay), U_regularizer=l2(weight_decay),
                   dropout_W=dropout, dropout_U=dropout, **cell_kw)
        o = Bidirectional(rec)(o) if bidirectional else rec(o)
    o = TimeDistributed(Dense(num_classes, W_regularizer=l2(weight_decay)))(o)
    model = ctc_model(x, o, **kw)
    model.config = {'name': 'deep_speech2', 'kwargs': dict(
        num_features=num_features, num_classes=num_classes, num_hiddens=num_hiddens,
        num_layers=num_layers, conv_filters=conv_filters,
        conv_kernels=[list(k) for k in conv_kernels], conv_strides=[list(k) for k in conv_strides],
        max_value=max_value, dropout=dropout, weight_decay=weight_decay,
        input_std_noise=input_std_noise)}
    if batch_norm:          # (only then: default checkpoints keep their config byte for byte)
        model.config['kwargs']['batch_norm'] = batch_norm if isinstance(batch_norm, str) else True
    if rnn_type != 'lstm':  # (likewise)
        model.config['kwargs']['rnn_type'] = rnn_type
    if not bidirectional:   # (likewise)
        model.config['kwargs']['bidirectional'] = False
    _record_spec_augment(model, spec_augment)
    _record_time_reduction(model, time_reduction)
    return model



def rhn(num_features=39, num_classes=28, num_hiddens=256, num_layers=5, depth=2, coupling=True,
        dropout=0.2, input_dropout=False, input_std_noise=.0, weight_decay=1e-4,
        merge_mode='concat', activation='tanh', **kw):
    """brsmv1's topology on the reference's Recurrent Highway Network cell.  NO REFERENCE
    COUNTERPART: the reference defines the ``RHN`` layer (core/layers.py:92-353) and routes it
    through ``recurrent(model='rhn')``, but none of its factories uses it.  Built from the
    reference's own pieces: brsmv1's noise / dropout / regularisers / output Dense
    (core/models.py:217-281) with every Bidirectional(LSTM) replaced by
    Bidirectional(RHN(num_hiddens, depth, coupling), merge_mode) -- W and every U_l l2
    ``weight_decay``, dropout_W = dropout_U = ``dropout``.  Runs on csrc/rhn.hip."""
    x = Input(name='inputs', shape=(None, num_features))
    o = x
    if input_std_noise is not None:
        o = GaussianNoise(input_std_noise)(o)
    if input_dropout:
        o = Dropout(dropout)(o)
    for _ in range(num_layers):
        o = Bidirectional(RHN(num_hiddens, depth=depth, coupling=coupling,
                              return_sequences=True, W_regularizer=l2(weight_decay),
                              U_regularizer=l2(weight_decay), dropout_W=dropout,
                              dropout_U=dropout, activation=activation),
                          merge_mode=merge_mode)(o)
    o = TimeDistributed(Dense(num_classes, W_regularizer=l2(weight_decay)))(o)
    model = ctc_model(x, o, **kw)
    model.config = {'name': 'rhn', 'kwargs': dict(
        num_features=num_features, num_classes=num_classes, num_hiddens=num_hiddens,
        num_layers=num_layers, depth=depth, coupling=coupling, dropout=dropout,
        input_dropout=input_dropout, input_std_noise=input_std_noise,
        weight_decay=weight_decay, merge_mode=merge_mode, activation=activation)}
    return model


def transformer(num_features=80, num_classes=28, d_model=256, num_heads=4, num_layers=6,
                d_ff=1024, dropout=0.1, conv=True, conv_filters=32,
                conv_kernels=((11, 41), (11, 21)), weight_decay=0., spec_augment=False,
                positions='absolute', context=None, time_reduction=None, **kw):
    """A CTC-trained pre-LN transformer encoder (arXiv 1706.03762, 2002.04745).  NO REFERENCE
    COUNTERPART.  conv=True: deep_speech2's front-end first -- Reshape, two Convolution2D with
    clipped ReLU (strides (2, 2) and (1, 2): time stride 2), Reshape.  Then
    TimeDistributed(Dense(d_model)), PositionalEncoding, Dropout, and ``num_layers`` blocks

        x = merge([Dropout(MultiHeadAttention(num_heads)(LayerNormalization(x))), x], 'sum')
        x = merge([Dropout(Dense(d_model)(relu(Dense(d_ff)(LayerNormalization(x))))), x], 'sum')

    a final LayerNormalization and TimeDistributed(Dense(num_classes)).  The attention keys of an
    utterance are its valid frames (the strided lengths).  weight_decay: l2 on every matrix.
    spec_augment=True (or a dict of its arguments): a SpecAugment layer directly behind Input.
    positions='relative': RelativeMultiHeadAttention in every block and no PositionalEncoding.
    context: None, 'causal' or a (chunk, left, right) window in strided frames, the ``context`` of
    MultiHeadAttention, given to every block: an encoder with a bounded look-ahead.  A block looks
    chunk - 1 + right frames ahead; with right = 0 that is the look-ahead of the whole stack,
    chunk - 1, not multiplied by the depth (every layer stays inside the chunk); with a non-zero
    right the blocks add up, num_layers * right for chunk = 1 and at most num_layers * (chunk - 1
    + right) otherwise (a frame seen past the chunk brings its own chunk along).  conv=True adds the fixed look-ahead of the two
    'same'-padded Convolution2D: the first reads kt1 - 1 - p1 input frames past input frame 2 t,
    p1 = (kt1 - 1) // 2 for an odd and (kt1 - 2) // 2 for an even number of input frames
    (TensorFlow's 'same' rule at stride 2), the second (kt2 - 1) // 2 strided frames; a strided
    frame t with an encoder look-ahead of A strided frames reads the input frames up to
    2 (t + A + (kt2 - 1) // 2) + kt1 - 1 - p1, which is 2 (t + A) + 16 with the default kernels
    and an even number of input frames.
    time_reduction=k (2 .. 8): one TimeReduction(k) directly in front of the input projection
    Dense(d_model): 2k x with the convolution front-end (4 x with k = 2, the papers' rate).  The
    encoder, its positions and a ``context`` window are then in frames of the REDUCED axis (one
    is 2k input frames), and the look-ahead stated above in strided frames multiplies by k."""
    attention = _attention_layer('transformer', positions)
    reg = l2(weight_decay)
    x = Input(name='inputs', shape=(None, num_features))
    o = _spec_augment(x, spec_augment)
    if conv:
        o = Reshape((-1, num_features, 1))(o)
        for (kt, kf), (st, sf) in zip(conv_kernels, ((2, 2), (1, 2))):
            o = Convolution2D(conv_filters, kt, kf, subsample=(st, sf), border_mode='same',
                              activation=clipped_relu(20), W_regularizer=reg)(o)
        o = Reshape((-1, o.features))(o)
    if time_reduction is not None:
        o = TimeReduction(_single_factor('transformer', time_reduction))(o)
    o = TimeDistributed(Dense(d_model, W_regularizer=reg))(o)
    if positions == 'absolute':
        o = PositionalEncoding()(o)
    o = Dropout(dropout)(o)
    for _ in range(num_layers):
        y = LayerNormalization()(o)
        y = attention(num_heads, W_regularizer=reg, context=context)(y)
        o = merge([Dropout(dropout)(y), o], mode='sum')
        y = LayerNormalization()(o)
        y = TimeDistributed(Dense(d_ff, W_regularizer=reg))(y)
        y = Activation('relu')(y)
        y = TimeDistributed(Dense(d_model, W_regularizer=reg))(y)
        o = merge([Dropout(dropout)(y), o], mode='sum')
    o = LayerNormalization()(o)
    o = TimeDistributed(Dense(num_classes, W_regularizer=reg))(o)
    model = ctc_model(x, o, **kw)
    model.config = {'name': 'transformer', 'kwargs': dict(
        num_features=num_features, num_classes=num_classes, d_model=d_model,
        num_heads=num_heads, num_layers=num_layers, d_ff=d_ff, dropout=dropout, conv=conv,
        conv_filters=conv_filters, conv_kernels=[list(k) for k in conv_kernels],
        weight_decay=weight_decay)}
    _record_spec_augment(model, spec_augment)
    _record_positions(model, positions)
    _record_context(model, context)
    _record_time_reduction(model, time_reduction)
    return model


def conformer(num_features=80, num_classes=28, d_model=256, num_heads=4, num_layers=6,
              d_ff=1024, kernel_size=31, conv_norm='batch', dropout=0.1, conv=True,
              conv_filters=32, conv_kernels=((11, 41), (11, 21)), weight_decay=0.,
              spec_augment=False, positions='absolute', context=None, causal_conv=False,
              time_reduction=None, **kw):
    """A CTC-trained Conformer encoder (arXiv 2005.08100).  NO REFERENCE COUNTERPART.  The
    front-end and input projection of ``transformer`` (conv=True: deep_speech2's two strided
    Convolution2D; then TimeDistributed(Dense(d_model)), PositionalEncoding, Dropout), then
    ``num_layers`` blocks, with FFN(x) = Dense(d_model)(swish(Dense(d_ff)(LN(x)))):

        x = merge([Dropout(FFN(x)), x], 'sum', scale=0.5)               half-step feed-forward
        x = merge([Dropout(MultiHeadAttention(num_heads)(LN(x))), x], 'sum')
        x = merge([Dropout(Dense(d_model)(swish(Norm(DepthwiseConvolution1D(kernel_size)(
                   GLU(Dense(2 d_model)(LN(x)))))))), x], 'sum')          convolution module
        x = merge([Dropout(FFN(x)), x], 'sum', scale=0.5)
        x = LN(x)

    and TimeDistributed(Dense(num_classes)).  conv_norm: 'batch' (the paper: BatchNormalization,
    with this library's semantics: training statistics over every frame of the real samples, time
    padding included) or 'layer' (LayerNormalization).  The attention keys and the depthwise
    convolution's input of an utterance are its valid frames (the strided lengths).  positions:
    'absolute' (the sinusoidal table added once, PositionalEncoding) or 'relative' (the paper's
    relative positional attention: RelativeMultiHeadAttention in every block and no
    PositionalEncoding layer).
    weight_decay: l2 on every matrix and depthwise filter.  spec_augment=True (or a dict of its
    arguments): a SpecAugment layer directly behind Input; its defaults are the paper's policy
    (section 3.2) without the time warp.
    context: None, 'causal' or a (chunk, left, right) window in strided frames, the ``context`` of
    the attention layer, given to every block; causal_conv=True: DepthwiseConvolution1D(causal=
    True) in every block.  Together they bound the look-ahead of the encoder, in strided frames:
    chunk - 1 when right = 0 (not multiplied by the depth: every layer stays inside the chunk);
    with a non-zero right the blocks add up (num_layers * right for chunk = 1, at most num_layers
    * (chunk - 1 + right) otherwise); plus (kernel_size - 1) / 2 per convolution module that is
    not causal; plus, with conv=True, the fixed look-ahead of the two
    'same'-padded Convolution2D of the front-end as ``transformer`` states it: with an encoder
    look-ahead of A strided frames the strided frame t reads the input frames up to
    2 (t + A + (kt2 - 1) // 2) + kt1 - 1 - p1.  With conv_norm='batch' the bound holds at inference only: the training statistics
    run over all frames.
    time_reduction=k (2 .. 8): one TimeReduction(k) directly in front of the input projection
    Dense(d_model), as in ``transformer``: 2k x with the convolution front-end.  ``context``
    windows, kernel_size and the look-ahead are then in frames of the REDUCED axis."""
    if conv_norm not in ('batch', 'layer'):
        raise ValueError("conformer(conv_norm=%r): 'batch' or 'layer'" % (conv_norm,))
    attention = _attention_layer('conformer', positions)
    reg = l2(weight_decay)
    x = Input(name='inputs', shape=(None, num_features))
    o = _spec_augment(x, spec_augment)
    if conv:
        o = Reshape((-1, num_features, 1))(o)
        for (kt, kf), (st, sf) in zip(conv_kernels, ((2, 2), (1, 2))):
            o = Convolution2D(conv_filters, kt, kf, subsample=(st, sf), border_mode='same',
                              activation=clipped_relu(20), W_regularizer=reg)(o)
        o = Reshape((-1, o.features))(o)
    if time_reduction is not None:
        o = TimeReduction(_single_factor('conformer', time_reduction))(o)
    o = TimeDistributed(Dense(d_model, W_regularizer=reg))(o)
    if positions == 'absolute':
        o = PositionalEncoding()(o)
    o = Dropout(dropout)(o)

    def ffn(o):
        y = LayerNormalization()(o)
        y = TimeDistributed(Dense(d_ff, W_regularizer=reg))(y)
        y = Activation('swish')(y)
        y = TimeDistributed(Dense(d_model, W_regularizer=reg))(y)
        return merge([Dropout(dropout)(y), o], mode='sum', scale=0.5)

    for _ in range(num_layers):
        o = ffn(o)
        y = LayerNormalization()(o)
        y = attention(num_heads, W_regularizer=reg, context=context)(y)
        o = merge([Dropout(dropout)(y), o], mode='sum')
        y = LayerNormalization()(o)
        y = TimeDistributed(Dense(2 * d_model, W_regularizer=reg))(y)
        y = GLU()(y)
        y = DepthwiseConvolution1D(kernel_size, W_regularizer=reg, causal=causal_conv)(y)
        y = BatchNormalization()(y) if conv_norm == 'batch' else LayerNormalization()(y)
        y = Activation('swish')(y)
        y = TimeDistributed(Dense(d_model, W_regularizer=reg))(y)
        o = merge([Dropout(dropout)(y), o], mode='sum')
        o = ffn(o)
        o = LayerNormalization()(o)
    o = TimeDistributed(Dense(num_classes, W_regularizer=reg))(o)
    model = ctc_model(x, o, **kw)
    model.config = {'name': 'conformer', 'kwargs': dict(
        num_features=num_features, num_classes=num_classes, d_model=d_model,
        num_heads=num_heads, num_layers=num_layers, d_ff=d_ff, kernel_size=kernel_size,
        conv_norm=conv_norm, dropout=dropout, conv=conv, conv_filters=conv_filters,
        conv_kernels=[list(k) for k in conv_kernels], weight_decay=weight_decay)}
    _record_spec_augment(model, spec_augment)
    _record_positions(model, positions)
    _record_context(model, context, causal_conv)
    _record_time_reduction(model, time_reduction)
    return model


def transducer(num_features=80, num_classes=28, encoder='lstm', num_hiddens=512, num_layers=5,
               joint_dim=512, pred_hiddens=512, pred_layers=1, dropout=0.2, weight_decay=1e-4,
               **encoder_kw):
    """An RNN-Transducer (arXiv 1211.3711; core/transducer.py, csrc/rnnt.hip).  NO REFERENCE
    COUNTERPART.  ``encoder``: 'lstm' (brsmv1's unidirectional stack), 'gru' (the unidirectional
    deep_speech2 form) or 'conformer' (which takes ``context=`` and ``causal_conv=``), each with
    its final Dense ``joint_dim`` wide instead of the classes; further keyword arguments go to
    that factory (``bidirectional=True`` is allowed for training: only streaming needs a bounded
    context; ``time_reduction=[[2, 2]]`` -- for 'conformer' an integer -- shortens the encoder
    output and with it the T x U lattice of the loss and the frames the greedy decode walks:
    ``inputs_length`` is mapped to the reduced axis inside the encoder).  The predictor is
    ``pred_layers`` bare LSTM(pred_hiddens), Dense(joint_dim), on the
    one-hot rows of the label history; the joint is tanh(f_t + g_u) W_out + b_out over the
    ``num_classes`` classes (blank last), like the CTC models' output."""
    from .transducer import TransducerModel
    kw = dict(encoder_kw)
    device, seed = kw.pop('device', None), kw.pop('seed', 0)
    decoder_kw = {k: kw.pop(k) for k in ('is_greedy', 'beam_width', 'merge_repeated', 'top_paths',
                                         'lm', 'lm_alpha', 'lm_beta') if k in kw}
    if joint_dim % 4:
        raise ValueError('transducer: joint_dim %d must be a multiple of 4' % joint_dim)
    common = dict(num_features=num_features, num_classes=joint_dim, device=device, seed=seed)
    if encoder == 'lstm':
        enc = brsmv1(num_hiddens=num_hiddens, num_layers=num_layers, dropout=dropout,
                     weight_decay=weight_decay,
                     **dict(dict(common, bidirectional=False), **kw))
    elif encoder == 'gru':
        enc = deep_speech2(num_hiddens=num_hiddens, num_layers=num_layers, dropout=dropout,
                           weight_decay=weight_decay,
                           **dict(dict(common, rnn_type='gru', bidirectional=False), **kw))
    elif encoder == 'conformer':
        enc = conformer(num_layers=num_layers, dropout=dropout, weight_decay=weight_decay,
                        **dict(common, **kw))
    else:
        raise ValueError("transducer(encoder=%r): 'lstm', 'gru' or 'conformer'" % (encoder,))
    classes = num_classes               # blank included (the last class), as in every factory
    x = Input(name='labels_onehot', shape=(None, classes - 1))
    o = x
    for _ in range(pred_layers):
        o = LSTM(pred_hiddens, return_sequences=True, consume_less='gpu', dropout_W=dropout,
                 dropout_U=dropout, W_regularizer=l2(weight_decay),
                 U_regularizer=l2(weight_decay))(o)
    o = TimeDistributed(Dense(joint_dim, W_regularizer=l2(weight_decay)))(o)
    o = TimeDistributed(Dense(classes, W_regularizer=l2(weight_decay)))(o)
    pred = ctc_model(x, o, device=device, seed=seed + 1)
    model = TransducerModel(enc, pred)
    model.decoder = ctc_utils.decoder_config(**decoder_kw)
    model.config = {'name': 'transducer', 'kwargs': dict(
        num_features=num_features, num_classes=num_classes, encoder=encoder,
        num_hiddens=num_hiddens, num_layers=num_layers, joint_dim=joint_dim,
        pred_hiddens=pred_hiddens, pred_layers=pred_layers, dropout=dropout,
        weight_decay=weight_decay, **kw)}
    return model


def aed(num_features=80, num_classes=28, encoder='blstm', num_hiddens=512, num_layers=5,
        d_att=256, num_heads=4, pred_hiddens=512, pred_layers=1, label_smoothing=0.0,
        dropout=0.2, weight_decay=1e-4, **encoder_kw):
    """An attention encoder-decoder (arXiv 1508.01211 with the multi-head attention of arXiv
    1706.03762; core/aed.py, csrc/cross_attention.hip, csrc/aed.hip).  NO REFERENCE COUNTERPART:
    the reference lists "Encoder-decoder models with attention mechanism" as TODO.  ``encoder``:
    'blstm' (brsmv1, bidirectional: the persistent BiLSTM stack), 'lstm' (brsmv1's unidirectional
    stack), 'gru' (deep_speech2 with rnn_type='gru'), 'conformer' or 'transformer', each with its
    final Dense ``2 d_att`` wide: the [K | V] of the decoder's cross-attention; further keyword
    arguments go to that factory: ``time_reduction=[[1, 2], [2, 2]]`` makes the 'blstm' encoder the
    pyramid of arXiv 1508.01211 (an integer for 'conformer' / 'transformer'), and the decoder
    then attends over the reduced frames, with key lengths on that axis.  The predictor is
    ``pred_layers`` bare LSTM(pred_hiddens), Dense(d_att) = the queries, on the one-hot rows of the label history; the output layer is
    tanh(ctx_u + q_u) W_out + b_out over the ``num_classes`` classes, EOS last (where the CTC
    models have blank).  ``label_smoothing`` is the eps of the cross-entropy; ``max_labels``
    (default 255) caps the greedy decode."""
    from .aed import AttentionDecoderModel, MAX_LABELS
    kw = dict(encoder_kw)
    device, seed = kw.pop('device', None), kw.pop('seed', 0)
    max_labels = kw.pop('max_labels', MAX_LABELS)
    decoder_kw = {k: kw.pop(k) for k in ('is_greedy', 'beam_width', 'merge_repeated', 'top_paths',
                                         'lm', 'lm_alpha', 'lm_beta') if k in kw}
    common = dict(num_features=num_features, num_classes=2 * d_att, device=device, seed=seed)
    if encoder in ('blstm', 'lstm'):
        enc = brsmv1(num_hiddens=num_hiddens, num_layers=num_layers, dropout=dropout,
                     weight_decay=weight_decay,
                     **dict(dict(common, bidirectional=encoder == 'blstm'), **kw))
    elif encoder == 'gru':
        enc = deep_speech2(num_hiddens=num_hiddens, num_layers=num_layers, dropout=dropout,
                           weight_decay=weight_decay, **dict(dict(common, rnn_type='gru'), **kw))
    elif encoder in ('conformer', 'transformer'):
        factory = conformer if encoder == 'conformer' else transformer
        enc = factory(num_layers=num_layers, dropout=dropout, weight_decay=weight_decay,
                      **dict(common, **kw))
    else:
        raise ValueError("aed(encoder=%r): 'blstm', 'lstm', 'gru', 'conformer' or 'transformer'"
                         % (encoder,))
    classes = num_classes               # EOS included (the last class), as blank in every factory
    x = Input(name='labels_onehot', shape=(None, classes - 1))
    o = x
    for _ in range(pred_layers):
        o = LSTM(pred_hiddens, return_sequences=True, consume_less='gpu', dropout_W=dropout,
                 dropout_U=dropout, W_regularizer=l2(weight_decay),
                 U_regularizer=l2(weight_decay))(o)
    o = TimeDistributed(Dense(d_att, W_regularizer=l2(weight_decay)))(o)
    o = TimeDistributed(Dense(classes, W_regularizer=l2(weight_decay)))(o)
    pred = ctc_model(x, o, device=device, seed=seed + 1)
    model = AttentionDecoderModel(enc, pred, num_heads=num_heads,
                                  label_smoothing=label_smoothing, max_labels=max_labels)
    model.decoder = ctc_utils.decoder_config(**decoder_kw)
    model.config = {'name': 'aed', 'kwargs': dict(
        num_features=num_features, num_classes=num_classes, encoder=encoder,
        num_hiddens=num_hiddens, num_layers=num_layers, d_att=d_att, num_heads=num_heads,
        pred_hiddens=pred_hiddens, pred_layers=pred_layers, label_smoothing=label_smoothing,
        dropout=dropout, weight_decay=weight_decay, **kw)}
    if max_labels != MAX_LABELS:        # (only then: a default model's config names no cap)
        model.config['kwargs']['max_labels'] = max_labels
    return model
