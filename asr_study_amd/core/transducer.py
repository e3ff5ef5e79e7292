"""``TransducerModel``: an RNN-Transducer (Graves, arXiv 1211.3711) on the kernels of csrc/rnnt.hip
(DESIGN.md 32).  Two ``engine.Model`` towers and the joint's output layer:

  encoder    any stage list the engine builds, ending in ``Dense(joint_dim)``
  predictor  bare ``LSTM(pred_hiddens)`` x ``pred_layers``, ``Dense(joint_dim)``, fed by the one-hot
             slab of the labels (a one-hot row times W is the embedding), and behind them a
             ``Dense(num_classes)`` stage that is never RUN: it only owns ``W_out`` / ``b_out`` in
             the predictor's flat buffers, so they get l2, optimiser state and a place in
             ``get_weights()`` like any Dense (``_joint_free`` hides it from forward / backward).

One training step: both forwards, ``ops.rnnt_loss_grad`` (which writes the gradients of both
tower outputs and of ``W_out`` / ``b_out``), both backwards, then ONE clip and update: the two
flat buffers' norms are combined on the device, so ``clipnorm`` bounds the norm over all
parameters as for every other model, with no host synchronisation.  Decoding is the
frame-synchronous greedy loop: ``ops.rnnt_greedy_step``, one predictor step of one frame through
the stage handlers with ``carry`` (the ``_uni_stream`` mechanism), ``ops.rows_select`` on every
(h, c) pair; the host reads the active-rows word once every 16 iterations.

Refused, each with its reason (follow-ups): data-parallel training, ``stream``, beam search,
``align``.
"""
import torch

from .. import ops
from .two_tower import TwoTowerModel, _joint_free

MAX_SYMBOLS = 10          # labels per frame in greedy decoding


class TransducerModel(TwoTowerModel):
    """(the plumbing both label-synchronous models share is core/two_tower.py's)"""
    _tag = 'transducer'
    _max_labels = ops.RNNT_MAX_LABELS
    _beam_reason = 'a transducer beam keeps a predictor state per hypothesis'

    def __init__(self, encoder, predictor, max_symbols=MAX_SYMBOLS):
        joint = predictor.stages[-1]
        if joint.kind != 'dense' or predictor.stages[-2].kind != 'dense':
            raise ValueError('the predictor ends in Dense(joint_dim), Dense(num_classes)')
        TwoTowerModel.__init__(self, encoder, predictor)
        if encoder.num_classes != self.joint_dim or joint.f_in_pad != self.joint_dim:
            raise ValueError('encoder and predictor must both end %d wide, a multiple of 4 '
                             '(got encoder %d)' % (self.joint_dim, encoder.num_classes))
        if not (self.joint_dim <= ops.RNNT_MAX_J and 2 <= self.num_classes <= ops.RNNT_MAX_C):
            raise ValueError('transducer: joint_dim <= %d and 2 <= classes <= %d'
                             % (ops.RNNT_MAX_J, ops.RNNT_MAX_C))
        if predictor.num_features != self.num_classes - 1:
            raise ValueError('the predictor reads one-hot rows of %d labels' % (self.num_classes - 1))
        self._check_predictor()
        self.max_symbols = int(max_symbols)

    def loss_and_grads(self, slab, labels, lens, training=True):
        """Both forwards, the transducer loss with grad_scale 1 / N, both backwards: the towers'
        ``grads`` hold d(mean loss) / d params.  Returns the per-utterance loss (device), the
        encoder output and its lengths."""
        N = len(labels)
        lab, lab_len, sl, in_len = self._prep(labels, lens, slab.shape[0])
        for m in self.towers:
            m._ar_ref_pad = ops.pad16(N)
        f, g = self._forward(slab, lab, lab_len, sl, in_len, N, training)
        enc, pred = self.encoder, self.predictor
        d_enc, d_pred = enc._buf('d_joint', f.shape), pred._buf('d_joint', g.shape)
        W, b = self._joint_params()
        dW, db = self._joint_params(grads=True)
        loss = ops.rnnt_loss_grad(f, g, W, b, lab, lab_len, sl, N, self.joint_dim,
                                  grads=(d_enc, d_pred, dW, db), grad_scale=1.0 / N)
        enc.backward(d_enc)
        with _joint_free(pred):
            pred.backward(d_pred)
        return loss, f, sl

    def _eval_loss(self, f, g, lab, lab_len, sl, N):
        W, b = self._joint_params()
        return ops.rnnt_loss_grad(f, g, W, b, lab, lab_len, sl, N, self.joint_dim)

    def _greedy(self, f, sl, N):
        """f (T, n_pad, J) encoder output, sl its lengths (device int32) -> decoded (N, cap)
        int32 and decoded_len (N), on the device.  A fresh session per call: nothing is carried
        from one call to the next."""
        pred, dev = self.predictor, self.device
        T, n_pad, J = f.shape
        cap = T * self.max_symbols

        def ints(n, v=0):
            return torch.full((n,), v, dtype=torch.int32, device=dev)
        t_ptr, n_sym, dlen, active = ints(N), ints(N), ints(N), ints(1)
        advance = ints(N, 1)                 # the start-of-sequence step commits every row
        dec = torch.full((N, cap), -1, dtype=torch.int32, device=dev)
        x_next = torch.zeros((n_pad, pred.f_in_pad0), dtype=torch.float32, device=dev)
        g_cur = torch.zeros((n_pad, J), dtype=torch.float32, device=dev)
        state, fp = self._predictor_state(n_pad), self._decode_pass(N, n_pad)
        W, b = self._joint_params()
        for it in range(T * (self.max_symbols + 1)):
            g_new = self._predictor_step(x_next.view(1, n_pad, -1), state, fp)
            for pairs in state.values():     # keep the new state only where a label was emitted
                for old, new in pairs:
                    ops.rows_select(advance, new, old, old, N)
            ops.rows_select(advance, g_new.view(n_pad, J), g_cur, g_cur, N)
            ops.rnnt_greedy_step(f, g_cur, W, b, sl, N, J, t_ptr, n_sym, dec, dlen, advance,
                                 x_next, active, max_symbols=self.max_symbols)
            if it % 16 == 15 and int(active.item()) == 0:
                break
        return dec, dlen

    # ------------------------------------------------------------------ refusals
    def stream(self, *args, **kwargs):
        raise NotImplementedError(
            'TransducerModel.stream is not built: a streaming session would carry the '
            'predictor state and the frame pointer beside the encoder\'s caches')

    def align(self, *args, **kwargs):
        raise NotImplementedError(
            'TransducerModel.align is not built: forced alignment on the transducer lattice '
            'needs a max-plus form of the alpha chain (asr_ctc_align is the CTC lattice)')
