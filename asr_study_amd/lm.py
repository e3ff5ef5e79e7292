"""Character n-gram language model for the prefix beam decoders (K9 with an LM).

``CharLM`` is a dense table of natural-log probabilities over the K = C - 1 labels of the
label parser (the CTC blank is not a symbol of it and there is no end-of-sentence symbol):

* order n (1 .. 5), history length h = n - 1; the extra symbol K stands for "before the
  sentence";
* the context index is the history read as base-(K+1) digits, oldest first:
  ``n_ctx = (K+1)**h``, ``root = n_ctx - 1`` (all "before"), ``next(ctx, label) =
  (ctx * (K+1) + label) % n_ctx``; for h = 0 there is one context;
* ``logp`` is (n_ctx, K) float32 with backoff already resolved, so a decoder does one table
  look-up per label and no arithmetic on the model.

``fused(alpha, beta)`` = float32(alpha) * logp + float32(beta), computed once by NumPy in
float32, is the ONLY thing the decoders see (csrc/decode_host.cpp, csrc/beam.hip and the test
oracle read the same float32 values).

``estimate`` is interpolated Witten-Bell smoothing in float64: P_0(c) = 1/K and, for k = 1..n
with g the last k-1 symbols of the padded history, N(g) the number of followers counted after g
and D(g) the number of distinct ones,

    P_k(c | g) = (c(g, c) + D(g) * P_{k-1}(c | g')) / (N(g) + D(g))   if N(g) > 0
               = P_{k-1}(c | g')                                       otherwise

where g' is g without its oldest symbol.  Every row sums to 1 and every entry is positive."""
import numpy as np

MAX_ORDER = 5


class CharLM(object):
    def __init__(self, logp, num_labels, order, vocab=None):
        order, K = int(order), int(num_labels)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError('CharLM: order must be 1 .. %d, got %d' % (MAX_ORDER, order))
        if K < 1:
            raise ValueError('CharLM: num_labels must be positive, got %d' % K)
        n_ctx = (K + 1) ** (order - 1)
        if n_ctx * K > np.iinfo(np.int32).max:
            raise ValueError('CharLM: a table of %d contexts x %d labels does not fit an int32 '
                             'index' % (n_ctx, K))
        logp = np.ascontiguousarray(logp, dtype=np.float32)
        if logp.shape != (n_ctx, K):
            raise ValueError('CharLM: logp has shape %s, order %d over %d labels needs %s'
                             % (logp.shape, order, K, (n_ctx, K)))
        self.order, self.num_labels, self.logp = order, K, logp
        self.vocab = None if vocab is None else str(vocab)
        self._fused = {}
        self._device = {}

    # ------------------------------------------------------------------ contexts
    @property
    def n_ctx(self):
        return (self.num_labels + 1) ** (self.order - 1)

    @property
    def root(self):
        return self.n_ctx - 1

    def next(self, ctx, label):
        return (int(ctx) * (self.num_labels + 1) + int(label)) % self.n_ctx

    # ------------------------------------------------------------------ estimation
    @classmethod
    def estimate(cls, sequences, num_labels, order, vocab=None):
        """Interpolated Witten-Bell estimate from label sequences (iterables of ints in
        [0, num_labels)); float64 throughout, deterministic."""
        order, K = int(order), int(num_labels)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError('CharLM: order must be 1 .. %d, got %d' % (MAX_ORDER, order))
        base = K + 1
        if base ** (order - 1) * K > np.iinfo(np.int32).max:
            raise ValueError('CharLM: order %d over %d labels does not fit an int32 index'
                             % (order, K))
        seqs = [np.asarray(list(s), dtype=np.int64).reshape(-1) for s in sequences]
        for s in seqs:
            if s.size and (s.min() < 0 or s.max() >= K):
                raise ValueError('CharLM.estimate: label outside [0, %d)' % K)
        # flat (context, follower) indices at the full history length, per position
        hist, foll = [], []
        for s in seqs:
            padded = np.concatenate([np.full(order - 1, K, np.int64), s])
            ctx = np.zeros(len(s), np.int64)
            for j in range(order - 1):                     # oldest digit first
                ctx = ctx * base + padded[j:j + len(s)]
            hist.append(ctx)
            foll.append(s)
        hist = np.concatenate(hist) if hist else np.zeros(0, np.int64)
        foll = np.concatenate(foll) if foll else np.zeros(0, np.int64)
        p = np.full((1, K), 1.0 / K, np.float64)           # P_0
        for k in range(1, order + 1):
            n_k = base ** (k - 1)                          # contexts of length k - 1
            counts = np.bincount((hist % n_k) * K + foll, minlength=n_k * K) \
                .astype(np.float64).reshape(n_k, K)
            total = counts.sum(axis=1, keepdims=True)
            distinct = (counts > 0).sum(axis=1, keepdims=True).astype(np.float64)
            lower = p[np.arange(n_k) % p.shape[0]]         # g' = g without its oldest symbol
            seen = total > 0
            p = np.where(seen, (counts + distinct * lower) / np.where(seen, total + distinct, 1.0),
                         lower)
        return cls(np.log(p).astype(np.float32), K, order, vocab=vocab)

    # ------------------------------------------------------------------ what the decoders read
    def fused(self, alpha=1.0, beta=0.0):
        """float32(alpha) * logp + float32(beta), (n_ctx, K) float32, computed once."""
        key = (float(np.float32(alpha)), float(np.float32(beta)))
        w = self._fused.get(key)
        if w is None:
            w = np.ascontiguousarray(np.float32(alpha) * self.logp + np.float32(beta),
                                     dtype=np.float32)
            w.setflags(write=False)
            self._fused[key] = w
        return w

    def fused_device(self, alpha, beta, device):
        """The fused table as a tensor on ``device``, cached per (alpha, beta, device)."""
        import torch
        key = (float(np.float32(alpha)), float(np.float32(beta)), str(torch.device(device)))
        w = self._device.get(key)
        if w is None:
            w = self._device[key] = torch.from_numpy(np.array(self.fused(alpha, beta))).to(device)
        return w

    # ------------------------------------------------------------------ file
    def save(self, path):
        fields = dict(order=np.int32(self.order), num_labels=np.int32(self.num_labels),
                      logp=self.logp)
        if self.vocab is not None:
            fields['vocab'] = np.array(self.vocab)
        with open(path, 'wb') as f:                        # (np.savez would append '.npz')
            np.savez(f, **fields)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            vocab = str(z['vocab'][()]) if 'vocab' in z.files else None
            return cls(z['logp'], int(z['num_labels']), int(z['order']), vocab=vocab)

    def check(self, num_classes=None, label_parser=None):
        """ValueError unless the model fits a network with ``num_classes`` outputs (blank
        included) and, where both are known, the label parser's symbols."""
        if num_classes is not None and self.num_labels != int(num_classes) - 1:
            raise ValueError('the language model has %d labels, the network %d (its %d classes '
                             'less the blank)' % (self.num_labels, int(num_classes) - 1,
                                                  int(num_classes)))
        if label_parser is not None:
            symbols = parser_vocab(label_parser)
            if self.vocab is not None and symbols is not None and self.vocab != symbols:
                raise ValueError('the language model was counted over the symbols %r, the label '
                                 'parser has %r' % (self.vocab, symbols))
        return self


def parser_vocab(label_parser):
    """The label parser's symbols in id order as one string, one character per label id below
    the blank's (None if it has no table; an id no symbol maps to reads as NUL)."""
    inv = getattr(label_parser, '_inv_vocab', None)
    if inv is None:
        return None
    return ''.join(inv.get(i, '\0') for i in range(max(inv)))    # (the last id is the blank)


def resolve(lm):
    """A CharLM, a path to one, or None."""
    if lm is None or isinstance(lm, CharLM):
        return lm
    return CharLM.load(lm)
