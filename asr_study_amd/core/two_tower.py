"""``TwoTowerModel``: what the label-synchronous models share -- ``TransducerModel``
(core/transducer.py) and ``AttentionDecoderModel`` (core/aed.py).  Two ``engine.Model`` towers:

  encoder    any stage list the engine builds, ending in a Dense stage
  predictor  bare ``LSTM(pred_hiddens)`` x ``pred_layers``, a Dense stage, fed by the one-hot slab of
             the labels (a one-hot row times W is the embedding), and behind them a
             ``Dense(num_classes)`` stage that is never RUN: it only owns ``W_out`` / ``b_out`` in
             the predictor's flat buffers, so they get l2, optimiser state and a place in
             ``get_weights()`` like any Dense (``_joint_free`` hides it from forward / backward).

Here: the weights of both towers as one list, ``compile``, the ONE clip and update over both flat
buffers (the two norms are combined on the device, so ``clipnorm`` bounds the norm over all
parameters as for every other model, with no host synchronisation), the batch preparation, both
forwards, the metrics, one step of the predictor from a carried state, the generators, and the
refusals the two models have in common.  A subclass states its loss (``loss_and_grads``,
``_eval_loss``) and its decode (``_greedy``).
"""
import contextlib

import numpy as np
import torch

from .. import ops
from . import optimizers as _opt
from .engine import Model
from .stages import KINDS, Pass, _nd


@contextlib.contextmanager
def _joint_free(pred):
    """The predictor without its last stage, the parameter-only joint output layer."""
    full = pred.stages
    pred.stages = full[:-1]
    try:
        yield
    finally:
        pred.stages = full


class TwoTowerModel(object):
    _tag = None             # the factory's name, as the messages about a batch's labels say it
    _max_labels = None      # labels of one utterance the loss kernels take
    _beam_reason = None     # why is_greedy=False is refused

    def __init__(self, encoder, predictor):
        self.encoder, self.predictor = encoder, predictor
        self.towers = (encoder, predictor)
        self.device = encoder.device
        self.joint = predictor.stages[-1]
        self.joint_dim, self.num_classes = self.joint.f_in, self.joint.n_out
        self.num_features = encoder.num_features
        self.optimizer = None
        # the model's loss sits in the ctc_loss slot: callbacks and command lines keep working
        self.metrics_names = ['loss', 'ctc_loss', 'decoder_loss', 'decoder_ler']
        self.decoder = dict(is_greedy=True)
        self.greedy_only = True
        self.stop_training = False
        self.config = None
        self._state = None

    def _check_predictor(self):
        for s in self.predictor.stages[:-2]:
            if s.kind != 'bilstm' or _nd(s) != 1:
                raise ValueError('the predictor is a stack of bare LSTM layers')

    # ------------------------------------------------------------------ weights
    def get_weights(self):
        return self.encoder.get_weights() + self.predictor.get_weights()

    def set_weights(self, weights):
        k = len(self.encoder.get_weights())
        self.encoder.set_weights(weights[:k])
        self.predictor.set_weights(weights[k:])

    def get_gradients(self):
        return self.encoder.get_gradients() + self.predictor.get_gradients()

    def count_params(self):
        return self.encoder.count_params() + self.predictor.count_params()

    def keras_layers(self, weights):
        """The checkpoint's layer groups (core/callbacks.py): each tower's own Keras names under
        the prefixes ``encoder_`` and ``predictor_``."""
        from .callbacks import keras_layers
        k = len(self.encoder.get_weights())
        return ([('encoder_' + n, ws) for n, ws in keras_layers(self.encoder, weights[:k])] +
                [('predictor_' + n, ws) for n, ws in keras_layers(self.predictor, weights[k:])])

    @property
    def _step(self):
        return self.encoder._step

    @_step.setter
    def _step(self, v):         # (utils/core_utils.load_model: a resumed run continues the streams)
        for m in self.towers:
            m._step = int(v)

    def _joint_params(self, grads=False):
        s, p = self.joint, self.predictor
        flat = p.grads if grads else p.params
        return (flat[s.oW:s.oW + self.joint_dim * self.num_classes],
                flat[s.ob:s.ob + self.num_classes])

    # ------------------------------------------------------------------ compile / update
    def compile(self, loss=None, optimizer=None, metrics=None, loss_weights=None):
        if isinstance(optimizer, str):
            optimizer = _opt.get(optimizer)
        self.optimizer = optimizer
        if optimizer is not None:
            self._state = [[torch.zeros_like(m.params) for _ in range(optimizer.n_state)]
                           for m in self.towers]
            # (what the checkpoint saves and restores: Optimizer.get_state / set_state)
            optimizer.state = [t for st in self._state for t in st]

    def _update(self):
        """One clip and update over ALL parameters: each tower's norm of (g + 2 l2 w) and l2
        penalty, combined on the device and handed to both towers' update launches."""
        opt = self.optimizer
        lr = opt.lr / (1.0 + opt.decay * opt.iterations) if opt.decay else opt.lr
        opt.iterations += 1
        for m in self.towers:
            ops.grad_norm(m.params, m.grads, m._segs_dev, m._nseg, m._norm)
        e, p = self.encoder._norm, self.predictor._norm
        e[0] = torch.hypot(e[0], p[0])
        e[1] = e[1] + p[1]
        p.copy_(e)
        for m, st in zip(self.towers, self._state):
            # (the timeout words of every recurrent workspace of the process: both towers')
            ops.optim_guard(m._norm, m.params.device, None)
            if isinstance(opt, _opt.Adam):
                ops.adam_step(m.params, m.grads, st[0], st[1], m._segs_dev, m._nseg, m._norm,
                              opt.clipnorm, lr, opt.iterations, opt.beta_1, opt.beta_2,
                              opt.epsilon)
            else:
                ops.sgd_step(m.params, m.grads, st[0], m._segs_dev, m._nseg, m._norm,
                             opt.clipnorm, lr, opt.momentum)

    # ------------------------------------------------------------------ batches
    to_slab = Model.to_slab
    _unpack_inputs = Model._unpack_inputs

    def _prep(self, labels, lens, T):
        """labels (N, l_max), label_len, seq_len (on the encoder output's time axis), in_len."""
        enc = self.encoder
        N = len(labels)
        l_max = max([len(l) for l in labels] + [1])
        if l_max > self._max_labels:
            raise ValueError('%s: %d labels in one utterance (at most %d)'
                             % (self._tag, l_max, self._max_labels))
        lab = np.zeros((N, l_max), np.int32)
        for n, l in enumerate(labels):
            lab[n, :len(l)] = np.asarray(l, np.int64).reshape(-1)
        if lab.size and (lab.min() < 0 or lab.max() >= self.num_classes - 1):
            raise ValueError('%s: labels must lie in 0 .. %d' % (self._tag, self.num_classes - 2))
        lens = np.asarray(lens).reshape(-1)
        sl = enc._key_lens(enc.out_lengths(lens), T)
        dev = self.device
        return (torch.from_numpy(lab).to(dev),
                torch.tensor([len(l) for l in labels], dtype=torch.int32, device=dev),
                torch.as_tensor(np.asarray(sl, np.int32)).to(dev),
                torch.as_tensor(np.asarray(lens, np.int32)).to(dev))

    def _forward(self, slab, lab, lab_len, sl, in_len, N, training):
        enc, pred = self.encoder, self.predictor
        f = enc.forward(slab, training=training, need_grad=training, n_real=N,
                        n_valid=0 if training else N,
                        seq_len=sl if (training or enc._needs_lens) else None,
                        in_len=in_len if ((training and enc._has_specaug) or enc._treduce)
                        else None)
        x = ops.onehot_rows(lab, lab_len, N, slab.shape[1], self.num_classes - 1,
                            out=pred._buf('onehot', (lab.shape[1] + 1, slab.shape[1],
                                                     pred.f_in_pad0)), ld=pred.f_in_pad0)
        with _joint_free(pred):
            g = pred.forward(x, training=training, need_grad=training, n_real=N,
                             n_valid=0 if training else N)
        return f.contiguous(), g.contiguous()

    def _refuse_world(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError(
                '%s: data-parallel training (world size %d) is not built: the two '
                'towers\' gradients would need one all-reduce with shared veto flags'
                % (type(self).__name__, dist.get_world_size()))

    def train_on_batch(self, inputs, outputs=None, sync=True):
        assert self.optimizer is not None, 'compile() first'
        self._refuse_world()
        slab, labels, lens = self._unpack_inputs(inputs)
        N = len(labels)
        loss, f, sl = self.loss_and_grads(slab, labels, lens, training=True)
        for m in self.towers:
            m._step += 1
        self._update()
        for m in self.towers:
            m._bn_update()
        dec, dlen = self._greedy(f, sl, N)
        res = (loss.clone(), dec, dlen, self.encoder._norm[1:2].clone(),
               ops.lstm_timeout_flags(self.device))
        return self._metrics(res, labels) if sync else res

    def _lagged(self, pending):
        res, labels, _ = pending
        return self._metrics(res, labels)

    def _metrics(self, res, labels):
        loss, dec, dlen, pen, flags = res
        loss_h = loss.cpu().numpy().astype(np.float64)
        if bool(flags.any().item()):
            from .._lib import AsrHipError
            raise AsrHipError('%s: a persistent recurrent kernel of the encoder gave '
                              'up on a bounded spin; the update was vetoed on the device.  The '
                              'stepwise retry of engine.Model is not built for two towers: build '
                              'the encoder with lstm_mode=1' % type(self).__name__)
        dec_h, dlen_h = dec.cpu().numpy(), dlen.cpu().numpy()
        hyps = [dec_h[n, :dlen_h[n]].tolist() for n in range(len(labels))]
        ler = float(np.mean(ops.edit_distance_host(hyps, [list(l) for l in labels])))
        mean = float(np.mean(loss_h))
        return [mean + float(pen.item()), mean, 0.0, ler]

    def _penalty(self):
        """l2 penalty of the current weights (what 'loss' reports beside the model's own loss)."""
        if self.optimizer is not None and self.encoder._step > 0:
            return self.encoder._norm[1:2].clone()
        w2 = 0.0
        for m in self.towers:
            for off, n, l2 in m._segments:
                if l2:
                    w2 += l2 * float((m.params[off:off + n].double() ** 2).sum().item())
        return torch.tensor([w2], dtype=torch.float64, device=self.device)

    def test_on_batch(self, inputs, outputs=None):
        slab, labels, lens = self._unpack_inputs(inputs)
        N = len(labels)
        lab, lab_len, sl, in_len = self._prep(labels, lens, slab.shape[0])
        f, g = self._forward(slab, lab, lab_len, sl, in_len, N, training=False)
        loss = self._eval_loss(f, g, lab, lab_len, sl, N)
        self._refuse_beam()
        dec, dlen = self._greedy(f, sl, N)
        return self._metrics((loss, dec, dlen, self._penalty(),
                              ops.lstm_timeout_flags(self.device)), labels)

    fit_generator = Model.fit_generator
    evaluate_generator = Model.evaluate_generator

    # ------------------------------------------------------------------ decoding
    def _refuse_beam(self):
        if not (self.decoder or {}).get('is_greedy', True):
            raise NotImplementedError(
                '%s: beam search (is_greedy=False) is not built: %s; decoding is greedy'
                % (type(self).__name__, self._beam_reason))

    def predict(self, x, inputs_length=None):
        """Greedily decoded label sequences for a batch, as engine.Model.predict takes it."""
        self._refuse_beam()
        if isinstance(x, list) and len(x) == 2 and inputs_length is None:
            x, inputs_length = x
        if isinstance(x, tuple) and x[0] == 'slab':
            x = x[1]
        slab = x if (torch.is_tensor(x) and x.dim() == 3 and x.shape[1] % 16 == 0) \
            else self.to_slab(x)
        N = len(inputs_length) if inputs_length is not None else slab.shape[1]
        lens = np.asarray(inputs_length if inputs_length is not None
                          else [slab.shape[0]] * N).reshape(-1)
        enc = self.encoder
        sl = enc._key_lens(enc.out_lengths(lens), slab.shape[0]).astype(np.int32)
        sl = torch.as_tensor(sl).to(self.device)
        f = enc.forward(slab, training=False, need_grad=False, n_valid=N,
                        seq_len=sl if enc._needs_lens else None,
                        in_len=enc._input_lens(lens)).contiguous()
        dec, dlen = self._greedy(f, sl, N)
        dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
        return [dec[n, :dlen[n]].tolist() for n in range(N)]

    def _predictor_state(self, n_pad):
        """Zero (h, c) pairs, old and new, of every LSTM stage of the predictor."""
        return {si: [[torch.zeros((n_pad, s.Hp), dtype=torch.float32, device=self.device)
                      for _ in range(2)] for _ in range(2)]
                for si, s in enumerate(self.predictor.stages[:-1]) if s.kind == 'bilstm'}

    def _decode_pass(self, N, n_pad):
        return Pass(training=False, masks=None, need_grad=False, n_valid=N, n_real=N, bn_weight=N,
                    seq_len=None, in_len=None, n_pad=n_pad, pipe=False, pre={}, nb=0,
                    stage_masks=lambda i: (None, None))

    def _predictor_step(self, x, state, fp):
        """One frame of the predictor on x (1, n_pad, in): every LSTM stage from its carried
        state (h0, c0) into (h_last, c_last), then the Dense stage."""
        pred, a = self.predictor, x
        for si, s in enumerate(pred.stages[:-1]):
            if s.kind == 'bilstm':
                (h0, h1), (c0, c1) = state[si]
                a = KINDS[s.kind].forward(pred, s, si, a, {}, fp,
                                          dict(h0=h0, h_last=h1, c0=c0, c_last=c1))
            else:
                a = KINDS[s.kind].forward(pred, s, si, a, {}, fp)
        return a
