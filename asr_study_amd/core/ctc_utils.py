"""CTC glue with the reference's names (core/ctc_utils.py).

In the reference these are Lambda bodies wrapping tf.nn.ctc_loss /
ctc_greedy_decoder / ctc_beam_search_decoder; here they call the HIP kernels (loss,
gradient, greedy, device beam search) through the C ABI, on time-major logit slabs."""
import numpy as np
import torch

from .. import lm as _lm
from .. import ops


def decoder_config(is_greedy=True, beam_width=100, top_paths=1, merge_repeated=True, lm=None,
                   lm_alpha=1.0, lm_beta=0.0):
    """Decoder kwargs of ``decode`` (core/ctc_utils.py:35-50).  ``lm`` (a CharLM or the path of
    one) with its weight ``lm_alpha`` and per-label bonus ``lm_beta`` turns the beam search into
    the character-LM one; the greedy decoder has no use for it."""
    if top_paths != 1:
        raise NotImplementedError('top_paths != 1')
    cfg = dict(is_greedy=is_greedy, beam_width=beam_width, merge_repeated=merge_repeated)
    if lm is not None:
        if is_greedy:
            raise ValueError('a language model needs the beam decoder: is_greedy=False')
        cfg.update(lm=_lm.resolve(lm), lm_alpha=float(lm_alpha), lm_beta=float(lm_beta))
    return cfg


def lm_of(decoder, num_classes):
    """(CharLM checked against the network's classes, alpha, beta) of a decoder dict, or None."""
    lm = decoder.get('lm')
    if lm is None:
        return None
    if decoder.get('is_greedy', True):
        raise ValueError('a language model needs the beam decoder: is_greedy=False')
    lm = _lm.resolve(lm).check(num_classes)
    return lm, float(decoder.get('lm_alpha', 1.0)), float(decoder.get('lm_beta', 0.0))


def decode(inputs, **kwargs):
    """(y_pred slab (T, n_pad, C) CUDA, seq_len (N,)) -> list of N label lists.
    is_greedy (default True) or beam search (beam_width 100, merge_repeated True), the latter
    with a character LM when ``lm`` (a CharLM or a path), ``lm_alpha``, ``lm_beta`` are given."""
    y_pred, seq_len = inputs
    seq = np.asarray(seq_len).reshape(-1).astype(np.int32)
    N = len(seq)
    lm = lm_of(kwargs, y_pred.shape[2])
    if kwargs.get('is_greedy', True):
        dec, dlen = ops.ctc_greedy(y_pred, torch.as_tensor(seq).to(y_pred.device), N)
        dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
        return [dec[n, :dlen[n]].tolist() for n in range(N)]
    width = int(kwargs.get('beam_width', 100))
    merge = bool(kwargs.get('merge_repeated', True))
    # host or device decoder (same strings, tests/test_gpu_beam.py): ops.beam_decoder_choice
    if ops.beam_decoder_choice(N, width, y_pred.shape[2], y_pred.is_cuda) == 'device':
        sl = torch.as_tensor(seq).to(y_pred.device)
        if lm is None:
            dec, dlen, _ = ops.ctc_beam_search(y_pred, sl, N, width, merge)
        else:
            model, alpha, beta = lm
            dec, dlen, _ = ops.ctc_beam_search_lm(
                y_pred, sl, N, width, merge, model.fused_device(alpha, beta, y_pred.device),
                model.order)
        dec, dlen = dec.cpu().numpy(), dlen.cpu().numpy()
        return [dec[n, :dlen[n]].tolist() for n in range(N)]
    if lm is None:
        hyps, _ = ops.ctc_beam_search_host(y_pred.cpu().numpy(), seq, N, width, merge)
    else:
        model, alpha, beta = lm
        hyps, _ = ops.ctc_beam_search_lm_host(y_pred.cpu().numpy(), seq, N, width, merge,
                                              model.fused(alpha, beta), model.order)
    return hyps


def ctc_lambda_func(args):
    """(y_pred slab, labels list, inputs_length) -> per-sample CTC loss (N,) CUDA."""
    y_pred, labels, inputs_length = args
    N = len(labels)
    lmax = max([len(l) for l in labels] + [1])
    lab = np.zeros((N, lmax), np.int32)
    for n, l in enumerate(labels):
        lab[n, :len(l)] = l
    dev = y_pred.device
    return ops.ctc_loss_grad(
        y_pred, torch.from_numpy(lab).to(dev),
        torch.tensor([len(l) for l in labels], dtype=torch.int32, device=dev),
        torch.as_tensor(np.asarray(inputs_length, np.int32).reshape(-1)).to(dev), N)


def ctc_dummy_loss(y_true, y_pred):
    """Keras needed a loss callable; the model output already IS the loss."""
    return y_pred


def decoder_dummy_loss(y_true, y_pred):
    return 0.0
