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


def _pack_labels(labels):
    lmax = max([len(l) for l in labels] + [1])
    lab = np.zeros((len(labels), lmax), np.int32)
    for n, l in enumerate(labels):
        lab[n, :len(l)] = np.asarray(l, np.int32).reshape(-1)
    return lab, np.array([len(l) for l in labels], np.int32)


def align_paths(y_pred, lab, lab_len, seq_len, N):
    """K19 on whichever side the logits are: the device kernel for a CUDA slab, the library's
    host form otherwise.  -> (path (N, T), score (N,)) numpy arrays."""
    if y_pred.is_cuda:
        dev = y_pred.device
        path, score = ops.ctc_align(y_pred, torch.as_tensor(lab).to(dev),
                                    torch.as_tensor(lab_len).to(dev),
                                    torch.as_tensor(seq_len).to(dev), N)
        return path.cpu().numpy(), score.cpu().numpy()
    lab, lab_len, seq_len = [a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
                             for a in (lab, lab_len, seq_len)]
    return ops.ctc_align_host(y_pred.detach().numpy(), lab, lab_len, seq_len, N)


def align(args):
    """(y_pred slab (T, n_pad, C), labels list, inputs_length) -> list of N (segments, score):
    the most probable CTC alignment of each KNOWN transcript, as ops.ctc_segments entries
    (label_index, label, start_frame, end_frame_exclusive) and its natural-log probability
    ([] and -inf for a transcript that does not fit its frames)."""
    y_pred, labels, inputs_length = args
    N = len(labels)
    lab, lab_len = _pack_labels(labels)
    seq = np.asarray(inputs_length, np.int32).reshape(-1)
    path, score = align_paths(y_pred, lab, lab_len, seq, N)
    return [(ops.ctc_segments(path[n], labels[n]), float(score[n])) for n in range(N)]


def ctc_dummy_loss(y_true, y_pred):
    """Keras needed a loss callable; the model output already IS the loss."""
    return y_pred


def decoder_dummy_loss(y_true, y_pred):
    return 0.0
