"""Layer descriptors with the Keras-1.2.2 names the reference's model factories use.

The reference builds a Keras functional graph (core/models.py:247-281:
Input -> GaussianNoise -> [TimeDistributed(Dense)] -> [Dropout] ->
N x Bidirectional(LSTM) -> TimeDistributed(Dense)) and hands its two ends to
``ctc_model(inputs, output)``.  Here the same calls build a tiny symbolic chain
(no tensors, no math); ``ctc_model`` turns the chain into the list of stages the
HIP engine (core/engine.py) executes.  ``LSTM`` keeps the reference override's
signature (core/layers.py:366-386: zoneout_h/zoneout_c/layer_norm/mi on top of the
Keras LSTM arguments); of the optional variants the residual ``merge``, multiplicative
integration, zoneout and layer normalisation are implemented.
``SimpleRNN`` (Bidirectional, 'concat' or 'sum'), ``Activation`` and ``recurrent()`` serve the
maas / deep_speech factories (core/models.py).  ``GRU`` (Keras 1.2.2, consume_less='gpu' layout,
hard_sigmoid gates, Bidirectional 'concat' or 'sum') runs on csrc/gru.hip and is deep_speech2's
``rnn_type='gru'`` cell.  ``RHN`` (the reference's Recurrent Highway Network layer) runs on
csrc/rhn.hip and is the cell of the ``rhn`` factory.  ``BatchNormalization`` (mode 0, axis -1) runs
bare or on the (N, T, F, C) image of the convolution front-end (csrc/batchnorm.hip).
``LayerNormalization`` (the reference's fourth layer class, core/layers.py:24-89) normalises every
frame over its features on csrc/layernorm.hip.
``MultiHeadAttention`` and ``PositionalEncoding`` (no reference counterpart) run on
csrc/attention.hip and make the ``transformer`` factory.
``RelativeMultiHeadAttention`` (relative sinusoidal positions inside the scores) runs on
csrc/rel_attention.hip; ``positions='relative'`` of transformer / conformer uses it.
``DepthwiseConvolution1D``, ``GLU``, ``Activation('swish')`` and ``merge(..., scale=)`` (no
reference counterpart either) run on csrc/dwconv.hip and make the ``conformer`` factory.
``SpecAugment`` (no reference counterpart) augments the input slab on csrc/specaug.hip; the
``spec_augment`` argument of deep_speech2 / transformer / conformer puts it behind ``Input``.
``TimeReduction`` (no reference counterpart) stacks consecutive frames on csrc/timestack.hip; the
``time_reduction`` argument of brsmv1 / deep_speech2 / transformer / conformer places it.
"""


class l2(object):
    """keras.regularizers.l2: adds l * sum(w^2) to the loss."""

    def __init__(self, l=0.01):
        self.l2 = float(l)


class Sym(object):
    """A symbolic (N, T, features) tensor: knows the stage that produced it.  ``fc`` is set
    while the tensor is viewed as an (N, T, F, C) image (between ``Reshape`` and the flattening
    ``Reshape`` of the convolution front-end): features = F * C, channel minor."""

    def __init__(self, features, producer=None, parent=None, name=None, fc=None):
        self.features = features
        self.producer = producer
        self.parent = parent
        self.name = name
        self.fc = fc

    def chain(self):
        out, cur = [], self
        while cur.producer is not None:
            out.append(cur.producer)
            cur = cur.parent
        return cur, out[::-1]


def Input(name=None, shape=None, dtype='float32', sparse=False):
    """keras.layers.Input(name='inputs', shape=(None, num_features))."""
    return Sym(shape[-1] if shape else None, name=name)


class Layer(object):
    def __call__(self, x):
        return Sym(self.out_features(x.features), producer=self, parent=x, fc=self.out_fc(x))

    def out_fc(self, x):
        return x.fc

    def out_features(self, f):
        return f


class GaussianNoise(Layer):
    """Adds N(0, sigma) in the training phase only (identity at sigma = 0, which
    is brsmv1's default: core/models.py:250-251)."""

    def __init__(self, sigma):
        self.sigma = float(sigma or 0.0)


class SpecAugment(Layer):
    """SpecAugment (arXiv 1904.08779) of the model INPUT, in the training phase only, on
    csrc/specaug.hip: per utterance a piecewise-linear time warp of at most ``time_warp`` frames
    (0: none), ``freq_masks`` frequency masks of width 0 .. ``freq_width`` and ``time_masks`` time
    masks of width 0 .. min(``time_width`` (0: no absolute cap), ``time_ratio`` * length), set to
    ``mask_value``.  The defaults are the Conformer paper's policy (arXiv 2005.08100, section 3.2:
    two frequency masks of up to 27 channels, ten time masks of up to 5 % of the utterance).
    Drawn per utterance from the library's Philox streams (seed, stage, step, rank), within each
    utterance's own length.  It augments data: it goes directly behind ``Input``, in front of
    every trainable layer.  No parameters; identity at inference.  Not built: the paper's sparse
    image warp (the piecewise-linear form replaces it), mask values other than a constant."""

    def __init__(self, time_warp=0, freq_masks=2, freq_width=27, time_masks=10, time_width=0,
                 time_ratio=0.05, mask_value=0.0, **kwargs):
        if kwargs:
            raise NotImplementedError('SpecAugment: unknown arguments %s' % sorted(kwargs))
        from .. import ops
        ops.specaug_check(time_warp, freq_masks, freq_width, time_masks, time_width, time_ratio)
        self.time_warp, self.freq_masks = int(time_warp), int(freq_masks)
        self.freq_width, self.time_masks = int(freq_width), int(time_masks)
        self.time_width, self.time_ratio = int(time_width), float(time_ratio)
        self.mask_value = float(mask_value)

    POLICY = ('time_warp', 'freq_masks', 'freq_width', 'time_masks', 'time_width', 'time_ratio',
              'mask_value')

    def policy(self):
        return {k: getattr(self, k) for k in self.POLICY}


class Dropout(Layer):
    """Plain (per-element) inverted dropout on the layer input, training only."""

    def __init__(self, p):
        self.p = float(p)


class Dense(object):
    def __init__(self, output_dim, W_regularizer=None, activation=None, **kwargs):
        if activation not in (None, 'linear'):
            raise NotImplementedError('Dense activation %r' % (activation,))
        self.output_dim = int(output_dim)
        self.l2 = W_regularizer.l2 if W_regularizer is not None else 0.0


class TimeDistributed(Layer):
    """TimeDistributed(Dense(n)): a row-wise affine map (core/models.py:278-279);
    TimeDistributed(Activation(...)) and TimeDistributed(Dropout(p)) act per element, exactly as
    the bare layers do (the Deep Speech factories wrap both)."""

    def __init__(self, layer):
        if not isinstance(layer, (Dense, Activation, Dropout)):
            raise NotImplementedError('TimeDistributed(%s): Dense, Activation or Dropout only'
                                      % type(layer).__name__)
        self.dense = layer if isinstance(layer, Dense) else None
        self.layer = layer

    def out_features(self, f):
        return self.dense.output_dim if self.dense is not None else f


class LSTM(object):
    """core/layers.py:356-479 (reference override of keras.layers.LSTM).

    Implemented: consume_less='gpu' fused layout, hard_sigmoid inner activation, the
    ``activation`` of the cell candidate and output (core/layers.py:452, :463: tanh by default;
    relu, sigmoid, hard_sigmoid, linear, softsign, softplus run on the variant kernels),
    variational dropout_W / dropout_U, W/U l2 regularisers,
    multiplicative integration (mi=[alpha, beta1, beta2] inits), zoneout_c / zoneout_h and
    layer_norm=[gain_init, bias_init] (LN of h@U, x@W and the output cell state).

    Used bare, ``LSTM(H, ...)(x)``, it is a UNIDIRECTIONAL layer (frames in order, output width H)
    on the stepwise kernels of csrc/lstm_uni.hip (K29): the plain cell with any ``activation``,
    dropout_W / dropout_U and the l2 regularisers.  It trains like the wrapped layer and, its
    state being two (N, H) vectors, streams chunk by chunk (core/stream.py).  Keras names of the
    unwrapped layer: lstm_k_W / _U / _b.  mi, zoneout_* and layer_norm are refused there.
    """

    def __init__(self, output_dim, zoneout_h=0., zoneout_c=0., layer_norm=None, mi=None,
                 return_sequences=True, consume_less='gpu', W_regularizer=None,
                 U_regularizer=None, dropout_W=0., dropout_U=0., activation='tanh',
                 inner_activation='hard_sigmoid', **kwargs):
        if layer_norm is not None and len(layer_norm) != 2:
            raise ValueError('layer_norm = [gain_init, bias_init]')
        self.layer_norm = None if layer_norm is None else [float(v) for v in layer_norm]
        if mi is not None and len(mi) != 3:
            raise ValueError('mi = [alpha_init, beta1_init, beta2_init]')
        self.mi = None if mi is None else [float(v) for v in mi]
        self.zoneout_h = float(zoneout_h or 0.0)
        self.zoneout_c = float(zoneout_c or 0.0)
        if inner_activation != 'hard_sigmoid':
            raise NotImplementedError('inner_activation: only hard_sigmoid is implemented')
        if activation not in ('tanh', 'relu', 'sigmoid', 'hard_sigmoid', 'linear', 'softsign',
                              'softplus'):
            raise NotImplementedError('LSTM activation %r (implemented: the Keras-1.2.2 names '
                                      'tanh, relu, sigmoid, hard_sigmoid, linear, softsign, '
                                      'softplus)' % (activation,))
        self.activation = activation
        if not return_sequences:
            raise NotImplementedError('return_sequences=False')
        self.output_dim = int(output_dim)
        self.dropout_W = float(dropout_W or 0.0)
        self.dropout_U = float(dropout_U or 0.0)
        self.l2_W = W_regularizer.l2 if W_regularizer is not None else 0.0
        self.l2_U = U_regularizer.l2 if U_regularizer is not None else 0.0

    def __call__(self, x):
        """Used bare (not inside Bidirectional): a unidirectional layer of width output_dim."""
        for name, on in (('mi', self.mi is not None),
                         ('zoneout_c / zoneout_h', self.zoneout_c > 0 or self.zoneout_h > 0),
                         ('layer_norm', self.layer_norm is not None)):
            if on:
                raise NotImplementedError(
                    'LSTM(%s) outside Bidirectional: the unidirectional kernels are the plain '
                    'cell only' % name)
        return Sym(self.output_dim, producer=self, parent=x, fc=None)


class SimpleRNN(object):
    """keras.layers.SimpleRNN (Keras 1.2.2): h_t = act(x_t W + b + h_{t-1} U), h_0 = 0.

    init: 'glorot_uniform' (default) or 'he_normal' (normal(0, sqrt(2 / fan_in)), not
    truncated); inner_init: 'orthogonal' (x 1.1, as the LSTM's U); b = 0.  activation: 'tanh',
    'relu', 'linear' or ``clipped_relu(max_value)``.  dropout_W / dropout_U: variational
    inverted-dropout masks per (sample, feature), drawn once per sequence and direction.
    Runs on csrc/rnn.hip; only return_sequences=True."""

    def __init__(self, output_dim, init='glorot_uniform', inner_init='orthogonal',
                 activation='tanh', W_regularizer=None, U_regularizer=None, b_regularizer=None,
                 dropout_W=0., dropout_U=0., return_sequences=True, **kwargs):
        if init not in ('glorot_uniform', 'he_normal'):
            raise NotImplementedError('SimpleRNN init %r (implemented: glorot_uniform, he_normal)'
                                      % (init,))
        if inner_init != 'orthogonal':
            raise NotImplementedError('SimpleRNN inner_init %r (implemented: orthogonal)'
                                      % (inner_init,))
        if b_regularizer is not None:
            raise NotImplementedError('SimpleRNN b_regularizer')
        if not return_sequences:
            raise NotImplementedError('return_sequences=False')
        from .. import ops
        ops.rnn_activation_id(activation)           # NotImplementedError for anything else
        self.activation = activation
        self.init, self.inner_init = init, inner_init
        self.output_dim = int(output_dim)
        self.dropout_W = float(dropout_W or 0.0)
        self.dropout_U = float(dropout_U or 0.0)
        self.l2_W = W_regularizer.l2 if W_regularizer is not None else 0.0
        self.l2_U = U_regularizer.l2 if U_regularizer is not None else 0.0


class GRU(object):
    """keras.layers.GRU (Keras 1.2.2) in the fused consume_less='gpu' layout: W (F, 3H), U (H, 3H),
    b (3H) with the column blocks z, r, h; with m = h_prev (.) B_U,
    z = hs(x_z + m U_z), r = hs(x_r + m U_r), hh = act(x_h + (r (.) m) U_h),
    h = z h_prev + (1 - z) hh, h_0 = 0 (the reset gate is applied before the product).

    Implemented: init='glorot_uniform' over the fused shape, inner_init='orthogonal' (x 1.1, as the
    LSTM's U), b = 0; activation 'tanh', 'relu', 'linear' or ``clipped_relu(max_value)``;
    inner_activation='hard_sigmoid'; W_regularizer / U_regularizer l2; variational dropout_W /
    dropout_U (one mask per sample, feature and direction, as Keras' 'gpu' mode uses mask 0 of its
    three); return_sequences=True.  Runs on csrc/gru.hip.

    batch_norm=True (not a Keras argument): sequence-wise batch normalisation of the input
    projection (arXiv 1510.01378), zx = gamma (.) (p - mu) / sqrt(var + bn_epsilon) + beta with
    p = (x (.) B_W) W and mu, var the per-column moments of the batch's VALID frames (t < length);
    padded frames are normalised with them and count for nothing.  beta replaces b: the weights per
    direction are W, U, gamma, beta and the running mean / variance (momentum bn_momentum), which
    inference uses.  Runs on the K18 kernels of csrc/batchnorm.hip.

    Used bare, ``GRU(H, ...)(x)``, it is a UNIDIRECTIONAL layer (frames in order, output width H)
    on the one-direction form of the same kernels (K28): it trains like the wrapped layer and,
    its state being one (N, H) vector, streams chunk by chunk (core/stream.py).  Keras names of
    the unwrapped layer: gru_k_W / _U / _b.  batch_norm=True is refused there."""

    IMPLEMENTED = ("output_dim, init='glorot_uniform', inner_init='orthogonal', activation in "
                   "(tanh, relu, linear, clipped_relu(v)), inner_activation='hard_sigmoid', "
                   "W_regularizer / U_regularizer l2, dropout_W, dropout_U, return_sequences=True, "
                   "consume_less='gpu', batch_norm in (False, True), bn_epsilon > 0, "
                   "0 <= bn_momentum <= 1")

    def __init__(self, output_dim, init='glorot_uniform', inner_init='orthogonal',
                 activation='tanh', inner_activation='hard_sigmoid', W_regularizer=None,
                 U_regularizer=None, b_regularizer=None, dropout_W=0., dropout_U=0.,
                 return_sequences=True, consume_less='gpu', batch_norm=False, bn_epsilon=1e-3,
                 bn_momentum=0.99, **kwargs):
        def refuse(what):
            raise NotImplementedError('GRU %s (implemented: %s)' % (what, self.IMPLEMENTED))
        if init != 'glorot_uniform':
            refuse('init %r' % (init,))
        if inner_init != 'orthogonal':
            refuse('inner_init %r' % (inner_init,))
        if inner_activation != 'hard_sigmoid':
            refuse('inner_activation %r' % (inner_activation,))
        if b_regularizer is not None:
            refuse('b_regularizer')
        if not return_sequences:
            refuse('return_sequences=False')
        if consume_less != 'gpu':
            refuse('consume_less %r' % (consume_less,))
        if kwargs:
            refuse('argument(s) %s' % ', '.join(sorted(kwargs)))
        if not isinstance(batch_norm, bool):
            refuse('batch_norm %r' % (batch_norm,))
        if not float(bn_epsilon) > 0.0:
            refuse('bn_epsilon %r' % (bn_epsilon,))
        if not 0.0 <= float(bn_momentum) <= 1.0:
            refuse('bn_momentum %r' % (bn_momentum,))
        from .. import ops
        try:
            ops.rnn_activation_id(activation)
        except NotImplementedError:
            refuse('activation %r' % (activation,))
        self.activation = activation
        self.batch_norm = batch_norm
        self.bn_epsilon, self.bn_momentum = float(bn_epsilon), float(bn_momentum)
        self.init, self.inner_init, self.inner_activation = init, inner_init, inner_activation
        self.output_dim = int(output_dim)
        self.dropout_W = float(dropout_W or 0.0)
        self.dropout_U = float(dropout_U or 0.0)
        self.l2_W = W_regularizer.l2 if W_regularizer is not None else 0.0
        self.l2_U = U_regularizer.l2 if U_regularizer is not None else 0.0

    def __call__(self, x):
        """Used bare (not inside Bidirectional): a unidirectional layer of width output_dim."""
        if self.batch_norm:
            raise NotImplementedError(
                'GRU(batch_norm=True) outside Bidirectional: the sequence-wise batch '
                'normalisation kernels take the projections of both directions of a layer; '
                'a one-direction form is not built')
        return Sym(self.output_dim, producer=self, parent=x, fc=None)


def highway_bias_initializer(shape, name=None):
    """The reference's bias initialiser of the RHN gates (core/initializers.py): constant -2."""
    import numpy as np
    return np.full(shape, -2.0, np.float32)


class RHN(object):
    """The reference's Recurrent Highway Network layer (core/layers.py:92-353; Zilly et al. 2016):
    one time step is ``depth`` highway micro-layers in sequence, only the first of which sees the
    input.  W (F, C H), U_l (H, C H), b_l (C H), column blocks h | t | [c]; C = 2 with
    ``coupling`` (c = 1 - t), else 3.  With s the state carried in (0 at the first frame):

        for l in 0 .. depth-1:
            a = (l == 0 ? (x B_W) W : 0) + (s B_U[l]) U_l + b_l
            h = act(a_h), t = hs(a_t), c = coupling ? 1 - t : hs(a_c)
            s = h t + s c
        y = s

    Implemented: init='glorot_uniform' over (F, C H), inner_init='orthogonal' (x 1.1, per U_l),
    bias_init=highway_bias_initializer (b_l = [0 | -2 | -2]); activation 'tanh', 'relu', 'linear'
    or ``clipped_relu(max_value)``; inner_activation='hard_sigmoid'; W_regularizer l2; variational
    dropout_W (one mask) / dropout_U (one mask per level); return_sequences=True.  Runs on
    csrc/rhn.hip.

    Three arguments cannot be taken from the reference, which crashes on them:
    * U_regularizer: the reference registers it on ``self.U``, an attribute that does not exist
      (core/layers.py:230-232).  Here it is l2 on every U_l, the evident intent (W_regularizer is
      l2 on W).
    * layer_norm=True: the reference calls an un-imported ``LN`` (:282).  NotImplementedError.
    * mi=True: the reference unpacks one tensor into three for every level above 0 (:200-203,
      :270).  NotImplementedError."""

    IMPLEMENTED = ("output_dim, depth >= 1, init='glorot_uniform', inner_init='orthogonal', "
                   "bias_init=highway_bias_initializer, activation in (tanh, relu, linear, "
                   "clipped_relu(v)), inner_activation='hard_sigmoid', coupling, "
                   "W_regularizer / U_regularizer l2, dropout_W, dropout_U, "
                   "return_sequences=True, consume_less")

    def __init__(self, output_dim, depth=1, init='glorot_uniform', inner_init='orthogonal',
                 bias_init=highway_bias_initializer, activation='tanh',
                 inner_activation='hard_sigmoid', coupling=True, layer_norm=False,
                 ln_gain_init='one', ln_bias_init='zero', mi=False, W_regularizer=None,
                 U_regularizer=None, b_regularizer=None, dropout_W=0., dropout_U=0.,
                 return_sequences=True, stateful=False, consume_less='gpu', **kwargs):
        def refuse(what):
            raise NotImplementedError('RHN %s (implemented: %s)' % (what, self.IMPLEMENTED))
        if int(depth) < 1:
            refuse('depth %r' % (depth,))
        if init != 'glorot_uniform':
            refuse('init %r' % (init,))
        if inner_init != 'orthogonal':
            refuse('inner_init %r' % (inner_init,))
        if bias_init not in (highway_bias_initializer, 'highway_bias_initializer'):
            refuse('bias_init %r' % (bias_init,))
        if inner_activation != 'hard_sigmoid':
            refuse('inner_activation %r' % (inner_activation,))
        if layer_norm:
            refuse('layer_norm=True (the reference calls an un-imported LN there)')
        if mi:
            refuse('mi=True (the reference cannot build it for depth > 1)')
        if b_regularizer is not None:
            refuse('b_regularizer')
        if not return_sequences:
            refuse('return_sequences=False')
        if stateful:
            refuse('stateful=True')
        if kwargs:
            refuse('argument(s) %s' % ', '.join(sorted(kwargs)))
        from .. import ops
        try:
            ops.rnn_activation_id(activation)
        except NotImplementedError:
            refuse('activation %r' % (activation,))
        self.activation = activation
        self.init, self.inner_init, self.inner_activation = init, inner_init, inner_activation
        self.bias_init = 'highway_bias_initializer'
        self.output_dim = int(output_dim)
        self.depth = int(depth)
        self.coupling = bool(coupling)
        self.dropout_W = float(dropout_W or 0.0)
        self.dropout_U = float(dropout_U or 0.0)
        self.l2_W = W_regularizer.l2 if W_regularizer is not None else 0.0
        self.l2_U = U_regularizer.l2 if U_regularizer is not None else 0.0


class Activation(Layer):
    """keras.layers.Activation: 'tanh', 'relu', 'linear', ``clipped_relu(max_value)`` or 'swish'
    (x sigmoid(x); this layer only, no recurrent layer takes it), element-wise (bare or inside
    TimeDistributed)."""

    def __init__(self, activation):
        from .. import ops
        if activation != 'swish':
            ops.rnn_activation_id(activation)       # NotImplementedError for anything else
        self.activation = activation


def recurrent(output_dim, model='keras_lstm', activation='tanh', regularizer=None, dropout=0.,
              **kwargs):
    """The reference's recurrent-layer factory (core/layers.py:482-516): 'rnn' -> SimpleRNN,
    'lstm' / 'keras_lstm' -> LSTM, with W and U regularised by ``regularizer`` and dropout_W =
    dropout_U = ``dropout``.  'gru' is not routed here yet: build the layer with ``GRU(...)``
    (this module) directly, and likewise 'rhn' with ``RHN(...)``."""
    if model == 'gru':
        raise NotImplementedError("recurrent(model='gru') is not routed yet: use "
                                  'layers.GRU(output_dim, ...) directly')
    if model == 'rhn':
        raise NotImplementedError("recurrent(model='rhn') is not routed yet: use "
                                  'layers.RHN(output_dim, depth, ...) directly')
    common = dict(W_regularizer=regularizer, U_regularizer=regularizer, dropout_W=dropout,
                  dropout_U=dropout, activation=activation, return_sequences=True)
    if model == 'rnn':
        return SimpleRNN(output_dim, **dict(common, **kwargs))
    if model in ('lstm', 'keras_lstm'):
        return LSTM(output_dim, **dict(common, **kwargs))
    raise ValueError('recurrent(model=%r): unknown model' % (model,))


class Bidirectional(Layer):
    """keras.layers.Bidirectional: LSTM with merge_mode='concat'; SimpleRNN, GRU and RHN with
    'concat' ([h_f | h_b]) or 'sum' (h_f + h_b)."""

    def __init__(self, layer, merge_mode='concat'):
        assert isinstance(layer, (LSTM, SimpleRNN, GRU, RHN))
        allowed = ('concat', 'sum') if isinstance(layer, (SimpleRNN, GRU, RHN)) else ('concat',)
        if merge_mode not in allowed:
            raise NotImplementedError('merge_mode=%r' % merge_mode)
        self.lstm = layer
        self.merge_mode = merge_mode

    def out_features(self, f):
        return (2 if self.merge_mode == 'concat' else 1) * self.lstm.output_dim


class Merge(Layer):
    """keras.layers.merge([a, b], mode): element-wise 'sum' or 'ave' of two tensors of
    the same width (brsmv1's residual connection, core/models.py:273-276).  ``scale`` (not in
    Keras) weighs the FIRST input of a 'sum': out = scale * a + b, the half-step residual of a
    Conformer's feed-forward modules."""

    def __init__(self, mode, skip, scale=1.0):
        if mode not in ('sum', 'ave'):
            raise NotImplementedError('merge mode %r (implemented: sum, ave)' % (mode,))
        if float(scale) != 1.0 and mode != 'sum':
            raise NotImplementedError("merge(scale=%r): with mode='sum' only" % (scale,))
        self.mode = mode
        self.skip = skip
        self.scale = float(scale)


def merge(inputs, mode=None, scale=1.0):
    a, b = inputs
    if a.features != b.features:
        raise ValueError('merge: widths differ (%s vs %s)' % (a.features, b.features))
    return Merge(mode, b, scale)(a)



def clipped_relu(max_value=20.0):
    """The reference's activation of its (dead) Deep Speech factories: ``relu(x,
    max_value=max_value)`` = min(max(x, 0), max_value) (core/models.py:116-117)."""
    return ('clipped_relu', float(max_value))


class BatchNormalization(Layer):
    """keras.layers.BatchNormalization (Keras 1.2.2), mode 0, axis -1: per feature (per channel on
    the (N, T, F, C) image between the convolution front-end's Reshapes) over every other axis.
    Training: the batch mean and biased variance of the real samples (all frames, time padding
    included); inference: the running moments, updated once per optimisation step as r <-
    momentum r + (1 - momentum) batch (no debias).  Weights: gamma, beta, running_mean,
    running_std (which holds the variance, as Keras names it)."""

    def __init__(self, epsilon=1e-3, mode=0, axis=-1, momentum=0.99, weights=None,
                 beta_init='zero', gamma_init='one', gamma_regularizer=None,
                 beta_regularizer=None, **kwargs):
        if mode != 0:
            raise NotImplementedError('BatchNormalization(mode=%r): mode 0 only' % (mode,))
        if axis != -1:
            raise NotImplementedError('BatchNormalization(axis=%r): axis -1 only' % (axis,))
        if gamma_regularizer is not None or beta_regularizer is not None:
            raise NotImplementedError('BatchNormalization regularizers')
        if beta_init != 'zero' or gamma_init != 'one':
            raise NotImplementedError("BatchNormalization: beta_init='zero', gamma_init='one' only")
        if weights is not None:
            raise NotImplementedError('BatchNormalization(weights=...): use set_weights')
        if not float(epsilon) > 0:
            raise ValueError('BatchNormalization: epsilon must be > 0')
        self.epsilon, self.momentum = float(epsilon), float(momentum)
        self.mode, self.axis = 0, -1
        self.in_fc = None

    def __call__(self, x):
        self.in_fc = x.fc
        return Layer.__call__(self, x)


class LayerNormalization(Layer):
    """The reference's LayerNormalization (core/layers.py:24-89; arXiv 1607.06450), which is dead
    code there (it calls an ``LN`` it never imports): built here as what the class says it is.
    For every frame (n, t) of an (N, T, F) tensor

        y = (x - mu) / sqrt(var + epsilon) * gain + bias

    with mu and the BIASED variance taken over the F features of that one frame, epsilon inside
    the square root (core/layers_utils.py:16-19).  Weights: gain, bias (F each), in that order.

    The axis: the reference's helper takes ``tf.nn.moments(x, [1])``, the feature axis of the
    (N, 4H) step tensors it was written for; read literally on a 3-D layer input that would be
    the time axis.  This layer normalises the FEATURE axis -- what the class docstring says
    ("all of the summed inputs to the neurons in a layer on a single training case"), what the
    paper does and what ``LSTM(layer_norm=...)`` does inside the cell.  On the (N, T, F, C)
    image between the convolution front-end's Reshapes the whole F * C vector of a frame is
    one group (gain / bias have F * C entries; no per-channel grouping).

    No mask: a time-padding frame is a frame like any other (a zero row gives y = bias).  No
    batch statistics, no running state: training and inference are the same computation, and a
    sample's output does not depend on what else is in the batch.  No l2 on gain or bias."""

    def __init__(self, epsilon=1e-5, weights=None, gain_init='one', bias_init='zero', **kwargs):
        if kwargs:
            raise NotImplementedError('LayerNormalization: unknown arguments %s' % sorted(kwargs))
        if gain_init != 'one' or bias_init != 'zero':
            raise NotImplementedError("LayerNormalization: gain_init='one', bias_init='zero' only")
        if weights is not None:
            raise NotImplementedError('LayerNormalization(weights=...): use set_weights')
        if not float(epsilon) > 0:
            raise ValueError('LayerNormalization: epsilon must be > 0')
        self.epsilon = float(epsilon)
        self.gain_init, self.bias_init = 'one', 'zero'


class MultiHeadAttention(Layer):
    """Multi-head self-attention over the frames of an utterance (arXiv 1706.03762) on
    csrc/attention.hip.  For an (N, T, F) input, D = num_heads * head_dim:

        [Q | K | V] = x W_qkv + b_qkv               (F, 3D): one projection, head h in columns
                                                    h * head_dim .. of each block
        P_h = softmax(Q_h K_h^T / sqrt(head_dim))   over the utterance's VALID frames (the keys
                                                    past its length carry probability 0)
        y = concat_h(P_h V_h) W_o + b_o             (D, output_dim)

    Every frame is a query, time-padding frames included (a frame like any other, as everywhere in
    this library); only keys are masked, by the utterance lengths the model is called with.
    Weights: W_qkv, b_qkv, W_o, b_o, in that order; W_regularizer (l2) applies to both matrices.
    head_dim defaults to features / num_heads, output_dim to the input width.  head_dim must be a
    multiple of 16 in 16 .. 128 (the kernel's tile).

    context: None (the whole utterance), 'causal' (= (1, -1, 0)) or a (chunk, left, right) window
    in frames, chunk >= 1, left >= -1 (-1: unlimited), right >= 0.  For query frame t, with
    c0 = (t // chunk) * chunk, key u is visible iff lo(t) <= u < hi(t) and u is a valid frame,

        hi(t) = c0 + chunk + right        lo(t) = 0 if left < 0 else max(0, c0 - left)

    chunk 1, right 0 is the causal mask (a finite left: a sliding window); chunk 1, right R a
    symmetric window; chunk C chunk-wise attention, whose look-ahead of chunk - 1 + right frames
    per layer does not grow with the number of layers when right = 0.  A time-padding query that sees no
    valid key (lo(t) at or past the utterance's length) gives a zero attention output and passes
    no gradient.  The kernels visit only the 64 x 64 tiles that hold a visible pair.

    Not built: dropout on the probabilities (use Dropout behind the layer), cross-attention,
    cached chunk-by-chunk inference.  Relative positions are RelativeMultiHeadAttention."""

    def __init__(self, num_heads, head_dim=None, output_dim=None, W_regularizer=None,
                 attention_dropout=0., context=None, **kwargs):
        if kwargs:
            raise NotImplementedError('MultiHeadAttention: unknown arguments %s' % sorted(kwargs))
        if attention_dropout:
            raise NotImplementedError('MultiHeadAttention(attention_dropout=%r): dropout on the '
                                      'attention probabilities is not implemented; put Dropout '
                                      'behind the layer' % (attention_dropout,))
        if int(num_heads) != num_heads or num_heads < 1:
            raise NotImplementedError('MultiHeadAttention: num_heads %r (an integer >= 1)'
                                      % (num_heads,))
        self.num_heads = int(num_heads)
        self.head_dim = None if head_dim is None else self._check_dh(head_dim)
        self.output_dim = None if output_dim is None else int(output_dim)
        self.l2 = W_regularizer.l2 if W_regularizer is not None else 0.0
        self.attention_dropout = 0.0
        self.context = self._check_context(context)

    @classmethod
    def _check_context(cls, context):
        """None, or the (chunk, left, right) triple of ``context``."""
        if context is None:
            return None
        if isinstance(context, str):
            if context != 'causal':
                raise NotImplementedError("%s(context=%r): None, 'causal' or (chunk, left, right)"
                                          % (cls.__name__, context))
            return (1, -1, 0)
        try:
            w = tuple(context)
            ok = len(w) == 3 and all(not isinstance(v, bool) and int(v) == v for v in w)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise NotImplementedError("%s(context=%r): None, 'causal' or three integers (chunk, "
                                      'left, right)' % (cls.__name__, context))
        w = tuple(int(v) for v in w)
        if w[0] < 1 or w[1] < -1 or w[2] < 0:
            raise ValueError('%s(context=%r): chunk >= 1, left >= -1 (-1: unlimited), right >= 0'
                             % (cls.__name__, context))
        return w

    @staticmethod
    def _check_dh(dh):
        if int(dh) != dh or dh < 16 or dh > 128 or int(dh) % 16:
            raise NotImplementedError('MultiHeadAttention: head_dim %r is not implemented (a '
                                      'multiple of 16 in 16 .. 128: the tile of the asr_attn_* '
                                      'kernels)' % (dh,))
        return int(dh)

    def __call__(self, x):
        if self.head_dim is None:
            if x.features % self.num_heads:
                raise NotImplementedError('MultiHeadAttention: %d heads do not divide the %d '
                                          'input features (pass head_dim)'
                                          % (self.num_heads, x.features))
            self.head_dim = self._check_dh(x.features // self.num_heads)
        if self.output_dim is None:
            self.output_dim = int(x.features)
        return Layer.__call__(self, x)

    def out_features(self, f):
        return self.output_dim


class RelativeMultiHeadAttention(MultiHeadAttention):
    """Multi-head self-attention with the relative sinusoidal positions of Transformer-XL
    (arXiv 1901.02860 section 3.3), as the Conformer uses it (arXiv 2005.08100 section 2.1), on
    csrc/rel_attention.hip.  For an (N, T, F) input, D = num_heads * head_dim:

        [Q | K | V] = x W_qkv + b_qkv
        pe[r, 2i] = sin(r 10000^(-2i / D)), pe[r, 2i + 1] = cos(r 10000^(-2i / D)),
                    r = -(T - 1) .. T - 1;   Pos = pe W_pos   (D, D), no bias
        s[t, u] = ((q_t + pos_bias_u[h]) . k_u + (q_t + pos_bias_v[h]) . pos_{t - u}) / sqrt(dh)
        y = concat_h(softmax_u(s) V_h) W_o + b_o

    The relative index is t - u, query frame minus key frame.  Everything else is
    MultiHeadAttention's: every frame is a query, only keys are masked by the utterance lengths.
    No PositionalEncoding layer is needed in front.  Weights: W_qkv, b_qkv, W_pos, pos_bias_u,
    pos_bias_v (num_heads, head_dim), W_o, b_o, in that order; W_regularizer (l2) applies to the
    three matrices.  head_dim must be a multiple of 16 in 16 .. 64 (the kernels stage a band of
    Pos rows beside the tiles of MultiHeadAttention, which leaves no LDS for more).  context:
    MultiHeadAttention's window (None, 'causal' or (chunk, left, right)); the positions a row uses
    are then the relative indices -(chunk - 1 + right) .. left + chunk - 1 only.  Not built:
    dropout on the probabilities, cross-attention, learned relative tables, cached chunk-by-chunk
    inference."""

    MAX_HEAD_DIM = 64

    def __init__(self, num_heads, head_dim=None, output_dim=None, W_regularizer=None,
                 context=None, **kwargs):
        if kwargs:
            raise NotImplementedError('RelativeMultiHeadAttention: unknown arguments %s'
                                      % sorted(kwargs))
        MultiHeadAttention.__init__(self, num_heads, head_dim=head_dim, output_dim=output_dim,
                                    W_regularizer=W_regularizer, context=context)

    @staticmethod
    def _check_dh(dh):
        if int(dh) != dh or dh < 16 or dh > RelativeMultiHeadAttention.MAX_HEAD_DIM or \
                int(dh) % 16:
            raise NotImplementedError('RelativeMultiHeadAttention: head_dim %r is not implemented '
                                      '(a multiple of 16 in 16 .. %d: the limit of the '
                                      'asr_relattn_* kernels, whose band tiles fill the LDS)'
                                      % (dh, RelativeMultiHeadAttention.MAX_HEAD_DIM))
        return int(dh)


class PositionalEncoding(Layer):
    """Adds the sinusoidal position table of arXiv 1706.03762 to an (N, T, F) tensor:
    pe[t, 2i] = sin(t / 10000^(2i / F)), pe[t, 2i + 1] = cos(t / 10000^(2i / F)); t counts the
    frames of the tensor it is applied to (behind a time-strided front-end: the strided frames).
    No parameters; the gradient passes through."""

    def __init__(self, **kwargs):
        if kwargs:
            raise NotImplementedError('PositionalEncoding: unknown arguments %s' % sorted(kwargs))


class DepthwiseConvolution1D(Layer):
    """A depthwise convolution over the time axis of an (N, T, C) tensor (the convolution of a
    Conformer's convolution module, arXiv 2005.08100) on csrc/dwconv.hip: one filter of
    ``kernel_size`` taps per channel, cross-correlation with 'same' padding,

        y[t, c] = b[c] + sum_j W[j, c] x[t + j - (k - 1) / 2, c]

    where the frames at or past the utterance's length (the lengths the model is called with)
    count as the zero padding, like the frames before 0: an utterance's valid frames do not
    depend on how far its batch is padded.  Every frame is an output.  Weights: W (k, C), b (C);
    W_regularizer (l2) applies to W.  kernel_size is odd, in 1 .. 63; the input width is a
    multiple of 4.  Straight in front of a BatchNormalization the bias has no effect on the
    training output (the batch mean takes it out); its gradient is then exactly zero and b keeps
    its value.  causal=True pads k - 1 frames on the left and none on the right,

        y[t, c] = b[c] + sum_j W[j, c] x[t + j - (k - 1), c]

    so that no output frame reads a later input frame.  Not built: strides, dilation, a depth
    multiplier."""

    MAX_KERNEL = 63

    def __init__(self, kernel_size, W_regularizer=None, causal=False, **kwargs):
        if kwargs:
            raise NotImplementedError('DepthwiseConvolution1D: unknown arguments %s'
                                      % sorted(kwargs))
        if (int(kernel_size) != kernel_size or kernel_size < 1 or kernel_size > self.MAX_KERNEL
                or int(kernel_size) % 2 == 0):
            raise NotImplementedError('DepthwiseConvolution1D: kernel_size %r (an odd integer in '
                                      "1 .. %d: 'same' padding, the tile of asr_dwconv1d_*)"
                                      % (kernel_size, self.MAX_KERNEL))
        if not isinstance(causal, (bool, int)) or causal not in (0, 1):
            raise NotImplementedError('DepthwiseConvolution1D(causal=%r): True or False'
                                      % (causal,))
        self.kernel_size = int(kernel_size)
        self.l2 = W_regularizer.l2 if W_regularizer is not None else 0.0
        self.causal = bool(causal)

    def __call__(self, x):
        if x.features % 4:
            raise NotImplementedError('DepthwiseConvolution1D over %d channels: the width must '
                                      'be a multiple of 4' % x.features)
        return Layer.__call__(self, x)


class GLU(Layer):
    """Gated linear unit over the feature axis (arXiv 1612.08083): y = a * sigmoid(g) with
    [a | g] the two halves of the input.  No weights; the width halves.  The input width must
    be a multiple of 8."""

    def __init__(self, **kwargs):
        if kwargs:
            raise NotImplementedError('GLU: unknown arguments %s' % sorted(kwargs))

    def __call__(self, x):
        if x.features % 8:
            raise NotImplementedError('GLU over %d features: the width must be a multiple of 8 '
                                      '(two halves of whole 16-byte groups)' % x.features)
        return Layer.__call__(self, x)

    def out_features(self, f):
        return f // 2


class TimeReduction(Layer):
    """Time reduction by frame stacking (no reference counterpart) on csrc/timestack.hip: ``factor``
    consecutive frames of an (N, T, F) tensor are concatenated into one frame,

        y[n, to, j F + f] = x[n, to * factor + j, f]        j < factor, To = ceil(T / factor)

    the pyramid step of "Listen, Attend and Spell" (arXiv 1508.01211), the time-reduction layer
    of RNN-T encoders, and -- directly behind Input -- the stacked input frames of LSTM-CTC.  The
    frames at or past an utterance's length (the lengths the model is called with) count as zeros,
    so the last, partial group of an utterance is zero-filled and its valid output frames do not
    depend on how far its batch is padded; the lengths behind the layer are ceil(len / factor).
    No parameters; the output width is factor * F; factor is an integer in 2 .. 8.  Not built:
    pooling (mean, max) in place of the concatenation, streaming through the layer."""

    MIN_FACTOR, MAX_FACTOR = 2, 8

    def __init__(self, factor, **kwargs):
        if kwargs:
            raise NotImplementedError('TimeReduction: unknown arguments %s' % sorted(kwargs))
        if (isinstance(factor, bool) or int(factor) != factor
                or not self.MIN_FACTOR <= factor <= self.MAX_FACTOR):
            raise NotImplementedError('TimeReduction: factor %r (an integer in %d .. %d: the '
                                      'limits of asr_time_stack_*)'
                                      % (factor, self.MIN_FACTOR, self.MAX_FACTOR))
        self.factor = int(factor)

    def out_features(self, f):
        return self.factor * f

    def out_fc(self, x):
        return None


class Reshape(Layer):
    """keras.layers.Reshape on the feature axes only: ``Reshape((-1, F, C))`` views the
    (N, T, F*C) features as an (N, T, F, C) image for Convolution2D, ``Reshape((-1, F*C))``
    flattens it again.  Channel-minor memory order either way: no data moves."""

    def __init__(self, target_shape):
        self.target = tuple(int(v) for v in target_shape)
        if len(self.target) not in (2, 3) or self.target[0] != -1:
            raise NotImplementedError('Reshape(%r): only (-1, F, C) and (-1, F*C)' % (target_shape,))

    def out_features(self, f):
        n = int(np_prod(self.target[1:]))
        if n != f:
            raise ValueError('Reshape: %d features into %r' % (f, self.target))
        return f

    def out_fc(self, x):
        return (self.target[1], self.target[2]) if len(self.target) == 3 else None


def np_prod(t):
    out = 1
    for v in t:
        out *= int(v)
    return out


class Convolution2D(Layer):
    """keras.layers.Convolution2D(nb_filter, nb_row, nb_col, subsample=(st, sf),
    border_mode='same', dim_ordering='tf', activation=clipped_relu(...)) over (time, frequency)
    of an (N, T, F, C) tensor.  NO REFERENCE COUNTERPART (README.md:118 lists Deep Speech 2 as
    TODO): the layer of BASELINE.json configs[2]'s "2 conv front-end", defined in
    include/asr_hip.h (K13) and oracle/conv.py."""

    def __init__(self, nb_filter, nb_row, nb_col, subsample=(1, 1), border_mode='same',
                 activation=None, W_regularizer=None, dim_ordering='tf', **kwargs):
        if border_mode != 'same' or dim_ordering != 'tf':
            raise NotImplementedError("Convolution2D: border_mode='same', dim_ordering='tf' only")
        if activation is None or activation == 'linear':
            self.clip = 0.0
        elif isinstance(activation, tuple) and activation[0] == 'clipped_relu':
            self.clip = float(activation[1])
        else:
            raise NotImplementedError('Convolution2D activation %r' % (activation,))
        self.nb_filter, self.kt, self.kf = int(nb_filter), int(nb_row), int(nb_col)
        self.st, self.sf = int(subsample[0]), int(subsample[1])
        self.l2 = W_regularizer.l2 if W_regularizer is not None else 0.0

    def out_fc(self, x):
        if x.fc is None:
            raise ValueError('Convolution2D needs an (N, T, F, C) input: Reshape((-1, F, C)) first')
        return (-(-x.fc[0] // self.sf), self.nb_filter)

    def __call__(self, x):
        fc = self.out_fc(x)
        self.in_fc = x.fc
        return Sym(fc[0] * fc[1], producer=self, parent=x, fc=fc)

