"""Command-line front ends: the flag sets of the reference's ``train.py`` (:46-88),
``eval.py`` (:26-49) and ``extras/make_dataset.py`` (:31-48) over this package.

Flags are declared in tables so the three tools share one implementation of
"resolve a plugin by name" (model factory, feature extractor, label parser,
dataset parser) and of "merge stored / explicit arguments" on resume and eval."""
import argparse
import datetime
import logging
import os

from .utils import generic_utils as utils
from .utils.hparams import HParams

_PLUGIN_FLAGS = [
    ('--input_parser', dict(type=str, default=None)),
    ('--input_parser_params', dict(nargs='+', default=[])),
    ('--label_parser', dict(type=str, default='simple_char_parser')),
    ('--label_parser_params', dict(nargs='+', default=[])),
]
_DEVICE_FLAGS = [
    ('--gpu', dict(default='0', type=str)),
    ('--allow_growth', dict(default=False, action='store_true')),
]
_LM_FLAGS = [                                           # no --lm: today's beam search, exactly
    ('--lm', dict(default=None, type=str)),             # a CharLM file (extras/make_lm.py)
    ('--lm_alpha', dict(default=1.0, type=float)),      # weight of log P(label | context)
    ('--lm_beta', dict(default=0.0, type=float)),       # bonus per label
]
TRAIN_FLAGS = [
    ('--load', dict(default=None, type=str)),
    ('--model', dict(default='brsmv1', type=str)),
    ('--model_params', dict(nargs='+', default=[])),
    ('--num_epochs', dict(default=100, type=int)),
    ('--lr', dict(default=0.001, type=float)),
    ('--momentum', dict(default=0.9, type=float)),
    ('--clipnorm', dict(default=400, type=float)),
    ('--batch_size', dict(default=32, type=int)),
    ('--opt', dict(default='adam', type=str, choices=['sgd', 'adam'])),
    ('--dataset', dict(default=None, type=str, nargs='+')),
] + _PLUGIN_FLAGS + [
    ('--lr_schedule', dict(default=None)),
    ('--lr_params', dict(nargs='+', default=[])),
    ('--save', dict(default=None, type=str)),
] + _DEVICE_FLAGS + [
    ('--verbose', dict(default=0, type=int)),
    ('--seed', dict(default=None, type=float)),
]
EVAL_FLAGS = [
    ('--model', dict(required=True, type=str)),
    ('--dataset', dict(required=True, type=str)),
    ('--subset', dict(type=str, default='test')),
    ('--batch_size', dict(default=32, type=int)),
] + _PLUGIN_FLAGS + _DEVICE_FLAGS + [
    ('--save_transcriptions', dict(default=None, type=str)),
    ('--beam_width', dict(default=400, type=int)),      # utils/core_utils.py:70-71
] + _LM_FLAGS
PREDICT_FLAGS = [
    ('--model', dict(required=True, type=str)),
    ('--dataset', dict(default=None, type=str)),
    ('--file', dict(default=None, type=str)),
    ('--subset', dict(type=str, default='test')),
] + _PLUGIN_FLAGS + [
    ('--no_decoder', dict(action='store_true', default=False)),
    # chunk-by-chunk inference (Model.stream): feed every utterance in pieces of this many
    # milliseconds of features; the decoder is then the greedy one
    ('--stream', dict(default=None, type=float)),
    # ... unless --stream_beam: the session then decodes with the device beam search at
    # --beam_width, with --lm* where given (Model.stream(beam=True))
    ('--stream_beam', dict(action='store_true', default=False)),
    # the pieces of --stream are raw samples, not features: the front-end runs inside the
    # session (Model.stream(feature=...)); the model's input parser must be norm='running'
    ('--stream_audio', dict(action='store_true', default=False)),
] + _DEVICE_FLAGS + [
    ('--save', dict(default=None, type=str)),
    ('--override', dict(default=False, action='store_true')),
    ('--beam_width', dict(default=400, type=int)),
] + _LM_FLAGS
ALIGN_FLAGS = [
    ('--model', dict(required=True, type=str)),
    ('--dataset', dict(default=None, type=str)),
    ('--file', dict(default=None, type=str)),
    ('--text', dict(default=None, type=str)),            # the transcript of --file
    ('--subset', dict(type=str, default='test')),
] + _PLUGIN_FLAGS + _DEVICE_FLAGS + [
    ('--save', dict(default=None, type=str)),            # JSON lines, one utterance per line
    ('--override', dict(default=False, action='store_true')),
]
MAKE_LM_FLAGS = [
    ('--dataset', dict(default=None, type=str)),
    ('--subset', dict(type=str, default='train')),
    ('--text', dict(default=None, type=str)),           # a text file, one sentence per line
    ('--label_parser', dict(type=str, default='simple_char_parser')),
    ('--label_parser_params', dict(nargs='+', default=[])),
    ('--order', dict(default=3, type=int)),
    ('--output_file', dict(type=str, default='lm.npz')),
]
MAKE_DATASET_FLAGS = [
    ('--parser', dict(type=str, default='dummy')),
    ('--parser_params', dict(nargs='+', default=[])),
    ('--output_file', dict(type=str, default=None)),
    ('--override', dict(action='store_true')),
] + _PLUGIN_FLAGS


def make_parser(description, table):
    ap = argparse.ArgumentParser(description=description)
    for flag, kw in table:
        ap.add_argument(flag, **kw)
    return ap


def resolve_plugins(args):
    """(feature extractor or None, label parser) named on the command line."""
    feature = utils.get_from_module('preprocessing.audio', args.input_parser,
                                    params=args.input_parser_params)
    labels = utils.get_from_module('preprocessing.text', args.label_parser,
                                   params=args.label_parser_params)
    return feature, labels


def merged_args(parsed, stored, explicit):
    """defaults < arguments stored in the checkpoint < arguments given explicitly.
    (The reference keeps only the last two, dropping un-stored defaults such as
    ``--subset``: eval.py:60.)"""
    return HParams(**vars(parsed)).update(stored).update(vars(explicit))


# ------------------------------------------------------------------ train
def _open_flows(args, data_gen):
    paths = args.dataset
    if len(paths) == 1:
        train, valid, test = data_gen.flow_from_fname(paths[0], datasets=['train', 'valid', 'test'])
        return train, valid, test
    train = data_gen.flow_from_fname(paths[0])
    valid = data_gen.flow_from_fname(paths[1])
    test = data_gen.flow_from_fname(paths[2]) if len(paths) == 3 else None
    return train, valid, test


def _new_model(args):
    from .core import optimizers
    factory = utils.get_from_module('core.models', args.model)
    model = factory(**(HParams().parse(args.model_params).values()))
    if args.opt.strip().lower() == 'sgd':
        opt = optimizers.SGD(lr=args.lr, momentum=args.momentum, clipnorm=args.clipnorm)
    else:
        opt = optimizers.Adam(lr=args.lr, clipnorm=args.clipnorm)
    # loss / metrics / loss_weights are accepted for signature parity (train.py:140-143)
    model.compile(loss={'ctc': 'ctc_dummy_loss', 'decoder': 'decoder_dummy_loss'}, optimizer=opt,
                  metrics={'decoder': 'ler'}, loss_weights=[1, 0])
    return model


def train_main(argv=None):
    parser = make_parser('Training an ASR system.', TRAIN_FLAGS)
    args = parser.parse_args(argv)
    utils.setup_logging()
    log = logging.getLogger('train')
    from . import parallel
    from .core.callbacks import MetaCheckpoint
    from .datasets.dataset_generator import DatasetGenerator
    from .utils.core_utils import setup_gpu, load_model
    rank, world = parallel.init_from_env()
    if world == 1:
        setup_gpu(args.gpu, args.allow_growth, log_device_placement=args.verbose > 1)

    first_epoch, meta = 0, None
    if args.load:
        explicit = utils.parse_nondefault_args(args, parser.parse_args([]), argv)
        model, meta = load_model(args.load, return_meta=True)
        args = merged_args(args, meta['training_args'], explicit)
        first_epoch = len(meta['epochs'])
        if explicit.lr:
            model.optimizer.lr = args.lr
    else:
        model = _new_model(args)
    if world > 1:
        parallel.broadcast_parameters(model)
    lr_callbacks = []
    if args.lr_schedule:
        # train.py:165-172: the class is looked up by name among the Keras callbacks
        from .core import callbacks as _cb
        fn = {k.lower(): getattr(_cb, k) for k in ('ReduceLROnPlateau', 'EarlyStopping')} \
            .get(str(args.lr_schedule).lower())
        if fn is None:
            raise ValueError('Learning rate schedule unrecognized')
        lr_callbacks.append(fn(**HParams().parse(args.lr_params).values()))

    out_dir = args.save or os.path.join('results', '%s_%s' % (args.model, datetime.datetime.now()))
    callbacks = []
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        callbacks = [MetaCheckpoint(os.path.join(out_dir, name), training_args=args, meta=meta)
                     for name in ('model.h5', 'best.h5')]
    callbacks = callbacks + lr_callbacks          # (every rank adjusts its own optimizer.lr)

    feature, labels = resolve_plugins(args)
    gen = DatasetGenerator(feature, labels, batch_size=args.batch_size, seed=args.seed)
    train_flow, valid_flow, test_flow = _open_flows(args, gen)
    if world > 1:       # every rank draws the same global batch and keeps its shard
        train_flow = parallel.ShardedFlow(train_flow, rank, world)
    if rank == 0:
        print(str(args.values() if isinstance(args, HParams) else vars(args)))
    model.fit_generator(train_flow, samples_per_epoch=train_flow.len, nb_epoch=args.num_epochs,
                        validation_data=valid_flow, nb_val_samples=valid_flow.len, max_q_size=10,
                        nb_worker=1, callbacks=callbacks, verbose=int(rank == 0),
                        initial_epoch=first_epoch)
    if test_flow is not None and rank == 0:
        best = load_model(os.path.join(out_dir, 'best.h5'), mode='eval')
        m = best.evaluate_generator(test_flow, test_flow.len, max_q_size=10, nb_worker=1)
        report = 'Total loss: %.4f\nCTC Loss: %.4f\nLER: %.2f%%' % (m[0], m[1], m[3] * 100)
        log.info(report)
        with open(os.path.join(out_dir, 'results.txt'), 'w') as f:
            f.write(report)
        print(report)
    parallel.finalize()


def _check_lm(model, label_parser):
    """A --lm counted over other symbols than the label parser's is refused before decoding
    (its label count is checked against the network's classes at the first batch)."""
    lm = (model.decoder or {}).get('lm')
    if lm is not None:
        lm.check(label_parser=label_parser)


# ------------------------------------------------------------------ eval
def eval_main(argv=None):
    parser = make_parser('Evaluating an ASR system.', EVAL_FLAGS)
    args = parser.parse_args(argv)
    explicit = utils.parse_nondefault_args(
        args, parser.parse_args(['--model', args.model, '--dataset', args.dataset]), argv)
    from .datasets.dataset_generator import DatasetGenerator
    from .utils.core_utils import setup_gpu, load_model
    setup_gpu(args.gpu, args.allow_growth)
    model, meta = load_model(args.model, return_meta=True, mode='eval', beam_width=args.beam_width,
                             lm=args.lm, lm_alpha=args.lm_alpha, lm_beta=args.lm_beta)
    args = merged_args(args, meta['training_args'], explicit)
    feature, labels = resolve_plugins(args)
    _check_lm(model, labels)
    flow = DatasetGenerator(feature, labels, batch_size=args.batch_size, seed=0) \
        .flow_from_fname(args.dataset, datasets=args.subset)
    values = model.evaluate_generator(flow, flow.len, max_q_size=10, nb_worker=1)
    for name, v in zip(model.metrics_names, values):
        print('%s: %4f' % (name, v))
    return values


# ------------------------------------------------------------------ predict
def predict_main(argv=None):
    """predict.py: transcribe one audio file or a dataset split, one utterance per
    forward pass (batch_size=1, the reference's latency path); ``--no_decoder`` saves the
    per-frame network outputs instead (HDF5: predictions vlen-f32 + num_labels, labels).
    ``--stream MS`` feeds each utterance to a Model.stream session in pieces of MS milliseconds of
    features and prints the growing greedy hypothesis per piece and the final one, which is the
    non-streaming greedy result (under a convolution front-end: of the utterance with one zero
    frame appended where its number of frames is odd, StreamSession.finish); a model that cannot
    stream is refused with the session's message.  With ``--stream_beam`` the session decodes
    with the device beam search of width ``--beam_width`` (and ``--lm``): per piece it prints the
    committed text, which no later frame changes, and the tentative tail in brackets; the final
    hypothesis is the whole-utterance beam decode of the streamed network outputs.
    With ``--stream_audio`` the pieces are MS milliseconds of raw samples (``--file``, or a dataset
    whose input parser runs on the fly): the front-end runs inside the session, resumed piece by
    piece (FeatureStream); the model's stored input parser must be ``norm='running'``."""
    import numpy as np
    parser = make_parser('Predicting with an ASR system.', PREDICT_FLAGS)
    args = parser.parse_args(argv)
    if args.stream_beam and (args.stream is None or args.no_decoder):
        raise ValueError('--stream_beam decodes a stream: it needs --stream MS and a decoder')
    if args.stream_audio and args.stream is None:
        raise ValueError('--stream_audio feeds raw samples to a stream: it needs --stream MS')
    if args.dataset is None and args.file is None:
        raise ValueError('dataset or file args must be set.')
    if args.dataset and args.file:
        print('Both dataset and file args was set. Ignoring file args.')
    explicit = utils.parse_nondefault_args(args, parser.parse_args(['--model', args.model]), argv)
    from .datasets.dataset_generator import DatasetGenerator, DatasetIterator
    from .utils.core_utils import setup_gpu, load_model
    setup_gpu(args.gpu, args.allow_growth)
    model, meta = load_model(args.model, return_meta=True, mode='predict',
                             decoder=(not args.no_decoder), beam_width=args.beam_width,
                             lm=None if args.no_decoder else args.lm, lm_alpha=args.lm_alpha,
                             lm_beta=args.lm_beta,
                             is_greedy=args.stream is not None and not args.stream_beam)
    session = None
    if args.stream is not None and not args.stream_audio:
        session = model.stream(1, beam=True) if args.stream_beam else model.stream(1)
    # only the feature / label plugins are inherited from the training run (the reference
    # overlays every stored argument, predict.py:60, which would also import its --save)
    stored = {k: v for k, v in meta['training_args'].items()
              if k in ('input_parser', 'input_parser_params', 'label_parser',
                       'label_parser_params')}
    args = merged_args(args, stored, explicit)
    feature, labels = resolve_plugins(args)
    _check_lm(model, labels)
    if args.stream_audio:
        if getattr(feature, 'norm', None) != 'running':
            raise ValueError(
                "--stream_audio: the model's input parser (%s) standardises with the statistics "
                "of the whole utterance, which a live signal does not have: build the dataset "
                "(extras/make_dataset.py) or train (train.py) with --input_parser_params norm "
                "running" % (feature,))
        session = model.stream(1, beam=True if args.stream_beam else None, feature=feature)
    if args.dataset is not None:
        flow = DatasetGenerator(feature, labels, batch_size=1, seed=0, mode='predict',
                                shuffle=False).flow_from_fname(args.dataset, datasets=args.subset)
    else:
        flow = DatasetIterator(np.array([args.file]), None, input_parser=feature,
                               label_parser=labels, mode='predict', shuffle=False, batch_size=1)
        flow.labels = np.array([u''])
    truth = list(flow.labels) if flow.labels is not None else [u''] * flow.len
    results = []
    for index in range(flow.len):
        if args.stream_audio:
            out = [_predict_streamed_audio(session, _raw_samples(flow, index, feature),
                                           args.stream, feature,
                                           None if args.no_decoder else labels)]
        elif session is not None:
            out = [_predict_streamed(session, flow.next(), args.stream, feature,
                                     None if args.no_decoder else labels)]
        else:
            out = model.predict(flow.next())
        best = out[0] if args.no_decoder else labels.imap(out[0])
        results.append({'label': truth[index], 'best': best})
        print('Ground Truth: %s' % labels._sanitize(truth[index]))
        print('   Predicted: %s\n\n' % (best if not args.no_decoder else 'array%s' % (best.shape,)))
    if args.save is not None:
        if os.path.exists(args.save):
            if not args.override:
                raise IOError('Unable to create file')
            os.remove(args.save)
        if not args.no_decoder:
            raise ValueError('save param must be set if no_decoder is True')
        from .datasets import h5lite
        with h5lite.File(args.save, 'w') as f:
            f.write_vlen_float('predictions', [r['best'].reshape(-1).astype('float32')
                                               for r in results],
                               attrs={'num_labels': int(results[0]['best'].shape[-1])})
            f.write_strings('labels', [str(r['label']) for r in results])
    return results


def _predict_streamed(session, batch, ms, feature, labels):
    """One utterance through a StreamSession in pieces of ``ms`` milliseconds of features (the
    input parser's ``win_step`` per frame, 10 ms where it has none): prints the hypothesis as it
    grows (labels: the label parser; None: the logits' frame count) and returns the whole."""
    import numpy as np
    x, lens = batch
    if isinstance(x, tuple) and x[0] == 'slab':     # (features extracted on the device)
        x = x[1][:, :1].permute(1, 0, 2)
    else:
        x = np.asarray(x, np.float32)
    T = int(np.asarray(lens).reshape(-1)[0])
    piece = max(1, int(round(ms / 1000.0 / float(getattr(feature, 'win_step', None) or 0.01))))
    session.reset()
    parts = []
    for pos in range(0, T, piece):
        end = min(T, pos + piece)
        parts.append(session.feed(x[:, pos:end], ended=[T] if end == T else None))
        _print_partial(parts, labels, end, session)
    parts.append(session.finish())
    if labels is None:
        return np.concatenate([p[0] for p in parts], 0)
    return [l for p in parts for l in p[0]]


def _raw_samples(flow, index, feature):
    """Utterance ``index`` of the flow as samples: a dataset whose input parser runs on the fly
    holds file names or sample arrays; stored features cannot be streamed as audio."""
    if getattr(flow, 'num_feats', None) is not None:
        raise ValueError('--stream_audio: the dataset stores features (%d columns), not audio; '
                         'give --file, or a dataset whose input parser runs on the fly'
                         % flow.num_feats)
    item = flow.inputs[[index]][0]
    if isinstance(item, bytes):
        item = item.decode('utf-8')
    if isinstance(item, str):
        return feature._load_file(item)
    return item


def _predict_streamed_audio(session, samples, ms, feature, labels):
    """One utterance through a session made with ``feature=``, in pieces of ``ms`` milliseconds
    of RAW SAMPLES: the front-end runs inside the session (feed_audio).  Prints and returns as
    _predict_streamed."""
    import numpy as np
    x = np.asarray(samples, np.float32).reshape(1, -1)
    n = x.shape[1]
    piece = max(1, int(round(ms / 1000.0 * float(feature.fs))))
    session.reset()
    parts = []
    for pos in range(0, n, piece):
        end = min(n, pos + piece)
        parts.append(session.feed_audio(x[:, pos:end], ended=[n] if end == n else None))
        _print_partial(parts, labels, session.frames_in, session)
    parts.append(session.finish_audio())
    if labels is None:
        return np.concatenate([p[0] for p in parts], 0)
    return [l for p in parts for l in p[0]]


def _print_partial(parts, labels, frames, session=None):
    if labels is None:
        print('  %6d frames in: %d frames out' % (frames, sum(p.shape[1] for p in parts)))
    elif session is not None and session.beam is not None:
        done = [l for p in parts for l in p[0]]
        print('  %6d frames in: %s[%s]' % (frames, labels.imap(done),
                                           labels.imap(session.hypothesis()[0][0][len(done):])))
    else:
        print('  %6d frames in: %s' % (frames, labels.imap([l for p in parts for l in p[0]])))


# ------------------------------------------------------------------ align
def align_main(argv=None):
    """align.py: where in its utterance each character of a KNOWN transcript lies (CTC forced
    alignment, Model.align), for a dataset split (its stored transcripts) or one audio file with
    ``--text``.  One utterance per forward pass, as predict.py.  Each result -- and each line of
    ``--save`` (JSON lines) -- holds ``label`` (the transcript), ``score`` (log-probability of
    the alignment) and ``chars``: per character ``char``, ``label`` (class id), ``start_frame`` /
    ``end_frame`` (exclusive) in frames of the network's output and ``start`` / ``end`` in seconds
    (frame x ``time_stride`` x the feature extractor's ``win_step``; null when the input parser
    has none)."""
    import json
    import numpy as np
    parser = make_parser('Aligning transcripts with an ASR system.', ALIGN_FLAGS)
    args = parser.parse_args(argv)
    if args.dataset is None and args.file is None:
        raise ValueError('dataset or file args must be set.')
    if args.dataset and args.file:
        print('Both dataset and file args was set. Ignoring file args.')
    if args.dataset is None and args.text is None:
        raise ValueError('text arg must be set with file.')
    if args.save is not None and os.path.exists(args.save) and not args.override:
        raise IOError('Unable to create file')
    explicit = utils.parse_nondefault_args(args, parser.parse_args(['--model', args.model]), argv)
    from .datasets.dataset_generator import DatasetGenerator, DatasetIterator
    from .utils.core_utils import setup_gpu, load_model
    setup_gpu(args.gpu, args.allow_growth)
    model, meta = load_model(args.model, return_meta=True, mode='predict', decoder=False)
    stored = {k: v for k, v in meta['training_args'].items()
              if k in ('input_parser', 'input_parser_params', 'label_parser',
                       'label_parser_params')}
    args = merged_args(args, stored, explicit)
    feature, labels = resolve_plugins(args)
    if args.dataset is not None:
        flow = DatasetGenerator(feature, labels, batch_size=1, seed=0, mode='predict',
                                shuffle=False).flow_from_fname(args.dataset, datasets=args.subset)
        truth = list(flow.labels[list(range(flow.len))])
    else:
        flow = DatasetIterator(np.array([args.file]), None, input_parser=feature,
                               label_parser=labels, mode='predict', shuffle=False, batch_size=1)
        truth = [args.text]
    truth = [t.decode('utf-8') if isinstance(t, bytes) else str(t) for t in truth]
    win_step = getattr(feature, 'win_step', None)
    results = []
    for index in range(flow.len):
        x, lens = flow.next()
        ids = labels(truth[index])
        out = model.align(x, [ids], lens)
        stride, al = out['time_stride'], out['alignments'][0]
        chars = []
        for q, lab, lo, hi in al['segments']:
            chars.append({'char': labels.imap([lab]), 'label': int(lab), 'start_frame': int(lo),
                          'end_frame': int(hi),
                          'start': None if win_step is None else float(lo * stride * win_step),
                          'end': None if win_step is None else float(hi * stride * win_step)})
        results.append({'label': truth[index], 'score': al['score'], 'time_stride': stride,
                        'chars': chars})
        print('%s  (log p = %.3f)' % (labels._sanitize(truth[index]), al['score']))
        print('   ' + ' '.join('%s[%d:%d]' % (c['char'], c['start_frame'], c['end_frame'])
                               for c in chars) + '\n')
    if args.save is not None:
        with open(args.save, 'w') as f:
            for r in results:
                f.write(json.dumps(r) + '\n')
    return results


# ------------------------------------------------------------------ make_dataset
def make_dataset_main(argv=None):
    """extras/make_dataset.py: crawl a corpus with a DatasetParser and write the HDF5
    the H5Iterator reads; features are computed on the GPU a chunk at a time."""
    parser = make_parser('Generates a preprocessed dataset (hdf5 file).', MAKE_DATASET_FLAGS)
    args = parser.parse_args(argv)
    corpus = utils.get_from_module('datasets*', args.parser, params=args.parser_params,
                                   regex=True)
    feature, labels = resolve_plugins(args)
    fmt = 'npz' if (args.output_file or '').endswith('.npz') else 'h5'
    out = corpus.to_h5(fname=args.output_file, input_parser=feature, label_parser=labels,
                       override=args.override, fmt=fmt)
    print('dataset written to', out)
    return out


# ------------------------------------------------------------------ make_lm
def make_lm_main(argv=None):
    """extras/make_lm.py: count the label sequences the label parser yields for one split of a
    dataset and / or the lines of a text file, estimate a character n-gram model
    (asr_study_amd.lm.CharLM: interpolated Witten-Bell) and write it for eval.py / predict.py
    ``--lm``."""
    parser = make_parser('Estimates a character n-gram language model (npz file).', MAKE_LM_FLAGS)
    args = parser.parse_args(argv)
    if args.dataset is None and args.text is None:
        raise ValueError('dataset or text args must be set.')
    from .lm import CharLM, parser_vocab
    labels = utils.get_from_module('preprocessing.text', args.label_parser,
                                   params=args.label_parser_params)
    sentences = []
    if args.dataset is not None:
        from .datasets.dataset_generator import DatasetGenerator
        flow = DatasetGenerator(None, labels, batch_size=1, shuffle=False) \
            .flow_from_fname(args.dataset, datasets=args.subset)
        sentences += [t.decode('utf-8') if isinstance(t, bytes) else str(t)
                      for t in flow.labels[list(range(flow.len))]]
    if args.text is not None:
        import io
        with io.open(args.text, encoding='utf-8') as f:
            sentences += [line.strip() for line in f if line.strip()]
    symbols = parser_vocab(labels)
    num_labels = len(symbols) if symbols is not None else None
    if num_labels is None:
        raise ValueError('the label parser %s has no symbol table' % args.label_parser)
    model = CharLM.estimate([labels(t) for t in sentences], num_labels, args.order, vocab=symbols)
    model.save(args.output_file)
    print('order-%d language model over %d labels from %d sentences written to %s'
          % (model.order, model.num_labels, len(sentences), args.output_file))
    return args.output_file
