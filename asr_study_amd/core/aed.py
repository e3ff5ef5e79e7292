"""``AttentionDecoderModel``: an attention encoder-decoder ("listen, attend and spell", Chan et al.,
arXiv 1508.01211, with the multi-head dot-product attention of arXiv 1706.03762) on the kernels of
csrc/cross_attention.hip and csrc/aed.hip.  The two towers of core/two_tower.py:

  encoder    any stage list the engine builds, ending in ``Dense(2 d_att)``: its output IS the
             [K | V] slab of the cross-attention, the bidirectional persistent BiLSTM stack
             included (the decoder reads the whole utterance: at the encoder OUTPUT's frame rate,
             the input's unless the encoder has a convolution front-end or TimeReduction stages
             -- ``time_reduction=[[1, 2], [2, 2]]`` is the pyramid of arXiv 1508.01211; the key
             lengths are on that axis, enc.out_lengths)
  predictor  the transducer's: bare ``LSTM(pred_hiddens)`` x ``pred_layers`` on the one-hot label
             history (a zero row is the start of the sequence), ``Dense(d_att)`` which gives Q, and
             the parameter-only ``Dense(num_classes)`` that owns ``W_out`` / ``b_out``.

Decoder row u of utterance n attends with q_u over the encoder's valid frames, and
tanh(ctx_u + q_u) W_out + b_out is scored against label u + 1, row U_n against EOS.  EOS is class
``num_classes - 1``, the slot the CTC models give to blank: ``num_classes`` keeps meaning
"labels + 1" in every data set and command line.

One training step: both forwards, ``ops.attn_cross_fwd`` (q_lens = U_n + 1, k_lens = the encoder's
output lengths), ``ops.aed_loss_grad`` with grad_scale 1 / N (d_ctx, d_q, dW_out, db_out),
``ops.attn_cross_bwd`` (dq of the attention, dkv = the encoder's output gradient), d_q = the
joint's + the attention's, both backwards, then the ONE clip and update of the base class.
Decoding is the label-synchronous greedy loop: one predictor step from the carried state,
``ops.attn_cross_fwd`` with Tq = 1, ``ops.aed_greedy_step``; the host reads the active-rows word
once every 16 iterations; at most ``max_labels`` labels per utterance.

Refused, each with its reason: beam search, ``stream``, ``align``, data-parallel training.  Joint
CTC / attention training is not built.
"""
import torch

from .. import ops
from .two_tower import TwoTowerModel, _joint_free

MAX_LABELS = ops.AED_MAX_LABELS       # labels per utterance in greedy decoding


class AttentionDecoderModel(TwoTowerModel):
    _tag = 'aed'
    _max_labels = ops.AED_MAX_LABELS
    _beam_reason = ('an attention-decoder beam keeps a predictor state per hypothesis and needs '
                    'a length normalisation')

    def __init__(self, encoder, predictor, num_heads=4, label_smoothing=0.0,
                 max_labels=MAX_LABELS):
        joint = predictor.stages[-1]
        if joint.kind != 'dense' or predictor.stages[-2].kind != 'dense':
            raise ValueError('the predictor ends in Dense(d_att), Dense(num_classes)')
        TwoTowerModel.__init__(self, encoder, predictor)
        self.d_att, self.num_heads = self.joint_dim, int(num_heads)
        if self.num_heads < 1 or self.d_att % self.num_heads:
            raise ValueError('aed: d_att %d is no multiple of num_heads %d'
                             % (self.d_att, self.num_heads))
        self.head_dim = self.d_att // self.num_heads
        if self.head_dim % 16 or not 16 <= self.head_dim <= 128:
            raise ValueError('aed: d_att / num_heads = %d must be a multiple of 16 in 16 .. 128 '
                             '(the head sizes of the attention core)' % self.head_dim)
        if encoder.num_classes != 2 * self.d_att or joint.f_in_pad != self.d_att:
            raise ValueError('the encoder must end 2 d_att = %d wide ([K | V]) and the predictor '
                             'd_att = %d wide (got encoder %d)'
                             % (2 * self.d_att, self.d_att, encoder.num_classes))
        if not (self.d_att <= ops.AED_MAX_J and 2 <= self.num_classes <= ops.AED_MAX_C):
            raise ValueError('aed: d_att <= %d and 2 <= classes <= %d'
                             % (ops.AED_MAX_J, ops.AED_MAX_C))
        if predictor.num_features != self.num_classes - 1:
            raise ValueError('the predictor reads one-hot rows of %d labels' % (self.num_classes - 1))
        self._check_predictor()
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError('aed: label_smoothing %r outside [0, 1)' % (label_smoothing,))
        self.label_smoothing = float(label_smoothing)
        self.max_labels = int(max_labels)
        if not 1 <= self.max_labels <= MAX_LABELS:
            raise ValueError('aed: max_labels %d outside 1 .. %d' % (self.max_labels, MAX_LABELS))

    def _attend(self, q, kv, q_lens, sl, N, lse=None, name='ctx'):
        """ctx (like q) of the queries q (Tq, n_pad, d_att) over kv (T, n_pad, 2 d_att)."""
        ctx = self.predictor._buf(name, q.shape)
        ops.attn_cross_fwd(q, kv, ctx, N, self.num_heads, self.head_dim, q_lens=q_lens, k_lens=sl,
                           lse=lse)
        return ctx

    def _lse(self, q):
        return self.predictor._buf('lse', (ops.attn_lse_len(q.shape[0], q.shape[1],
                                                            self.num_heads),))

    def loss_and_grads(self, slab, labels, lens, training=True):
        """Both forwards, the attention, the loss with grad_scale 1 / N, the attention's backward,
        both backwards: the towers' ``grads`` hold d(mean loss) / d params.  Returns the
        per-utterance loss (device), the encoder output [K | V] and its lengths."""
        N = len(labels)
        lab, lab_len, sl, in_len = self._prep(labels, lens, slab.shape[0])
        for m in self.towers:
            m._ar_ref_pad = ops.pad16(N)
        kv, q = self._forward(slab, lab, lab_len, sl, in_len, N, training)
        enc, pred = self.encoder, self.predictor
        q_lens = lab_len + 1
        lse = self._lse(q)
        ctx = self._attend(q, kv, q_lens, sl, N, lse)
        d_ctx, d_q = pred._buf('d_ctx', q.shape), pred._buf('d_joint', q.shape)
        W, b = self._joint_params()
        dW, db = self._joint_params(grads=True)
        loss = ops.aed_loss_grad(ctx, q, W, b, lab, lab_len, N, grads=(d_ctx, d_q, dW, db),
                                 grad_scale=1.0 / N, eps=self.label_smoothing)
        dq_att, dkv = pred._buf('dq_att', q.shape), enc._buf('d_joint', kv.shape)
        ops.attn_cross_bwd(q, kv, ctx, lse, d_ctx, dq_att, dkv, N, self.num_heads, self.head_dim,
                           q_lens=q_lens, k_lens=sl)
        ops.axpby(1.0, d_q, 1.0, dq_att, d_q)           # the joint's + the attention's
        enc.backward(dkv)
        with _joint_free(pred):
            pred.backward(d_q)
        return loss, kv, sl

    def _eval_loss(self, kv, q, lab, lab_len, sl, N):
        ctx = self._attend(q, kv, lab_len + 1, sl, N)
        W, b = self._joint_params()
        return ops.aed_loss_grad(ctx, q, W, b, lab, lab_len, N, eps=self.label_smoothing)

    def _greedy(self, kv, sl, N):
        """kv (T, n_pad, 2 d_att) encoder output, sl its lengths (device int32) -> decoded (N,
        max_labels) int32 and decoded_len (N), on the device.  A fresh session per call."""
        pred, dev = self.predictor, self.device
        n_pad, cap = kv.shape[1], self.max_labels

        def ints(n, v=0):
            return torch.full((n,), v, dtype=torch.int32, device=dev)
        finished, dlen, advance, active = ints(N), ints(N), ints(N), ints(1)
        dec = torch.full((N, cap), -1, dtype=torch.int32, device=dev)
        x_next = torch.zeros((n_pad, pred.f_in_pad0), dtype=torch.float32, device=dev)
        state, fp = self._predictor_state(n_pad), self._decode_pass(N, n_pad)
        W, b = self._joint_params()
        for it in range(cap + 1):
            q = self._predictor_step(x_next.view(1, n_pad, -1), state, fp).contiguous()
            for pairs in state.values():     # every row moves on: a finished row is never read
                for old, new in pairs:
                    old.copy_(new)
            ctx = self._attend(q, kv, None, sl, N, name='ctx_step')
            ops.aed_greedy_step(ctx, q, W, b, N, finished, dec, dlen, advance, x_next, active,
                                max_labels=cap)
            if it % 16 == 15 and int(active.item()) == 0:
                break
        return dec, dlen

    # ------------------------------------------------------------------ refusals
    def stream(self, *args, **kwargs):
        raise NotImplementedError(
            'AttentionDecoderModel.stream is not built: the decoder attends over the whole '
            'utterance, so no label can be emitted before the last frame')

    def align(self, *args, **kwargs):
        raise NotImplementedError(
            'AttentionDecoderModel.align is not built: attention weights are no monotonic '
            'alignment of labels to frames (asr_ctc_align is the CTC lattice)')
