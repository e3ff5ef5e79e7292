"""Oracle for the character-LM prefix beam search.  TEST INFRASTRUCTURE ONLY.

* ``beam_search_lm_one``: oracle/decode.py's float64 restatement of TensorFlow's
  CTCBeamSearchDecoder with its two scorer hooks filled in: every tree entry carries the LM
  context of its prefix and the constant w_e = w[ctx(parent), label]; w_e is added to what the
  parent feeds a branch's label path and to a child's first offer.  With w = None it IS
  oracle.decode.beam_search_decode_one(dtype=float64).
* ``estimate``: interpolated Witten-Bell written a second way (dictionaries of follower counts
  and a recursion over the history, not dense tables).
* ``bruteforce``: every labelling's CTC score (oracle.decode.beam_search_bruteforce) plus the
  sum of w along the labelling.
* ``lexicon_corpus``: the fixed-seed toy task on which the LM must help.
"""
import numpy as np

from oracle.decode import LOG_ZERO, _Entry, _lse, beam_search_bruteforce


def n_ctx(K, order):
    return (K + 1) ** (order - 1)


def next_ctx(ctx, label, K, order):
    return (ctx * (K + 1) + label) % n_ctx(K, order)


def beam_search_lm_one(logits, beam_width, w=None, order=1, merge_repeated=True):
    """logits (T, C) float (already cut to seq_len); w (n_ctx, C - 1) float32 or None.
    Returns (top label list, its log-score)."""
    best = _search(logits, beam_width, w, order)
    return best.label_seq(merge_repeated), float(best.nt)


def beam_search_lm_both(logits, seq_len, beam_width, w=None, order=1):
    """One search per utterance (merge_repeated only collapses the emitted string):
    (strings with merge_repeated, strings without, scores)."""
    logits = np.asarray(logits)
    best = [_search(logits[:int(seq_len[n]), n], beam_width, w, order)
            for n in range(logits.shape[1])]
    return ([b.label_seq(True) for b in best], [b.label_seq(False) for b in best],
            [float(b.nt) for b in best])


def _search(logits, beam_width, w, order):
    """The best leaf after the last frame."""
    x = np.asarray(logits, dtype=np.float64)
    T, C = x.shape
    K, blank = C - 1, C - 1
    counter = [0]
    ctx_of, w_of = {}, {}

    def new_entry(parent, label):
        counter[0] += 1
        e = _Entry(parent, label, counter[0])
        if parent is None:
            ctx_of[e] = n_ctx(K, order) - 1
            w_of[e] = 0.0
        else:
            ctx_of[e] = next_ctx(ctx_of[parent], label, K, order)
            w_of[e] = 0.0 if w is None else float(w[ctx_of[parent], label])
        return e

    root = new_entry(None, -1)
    root.nt, root.nb, root.nl = 0.0, 0.0, LOG_ZERO
    leaves = [root]

    cache = [None]                                  # the bottom, until the leaves change

    def bottom(lv):
        if cache[0] is None:
            cache[0] = min(lv, key=lambda e: (e.nt, -e.order))
        return cache[0]

    for t in range(T):
        inp = x[t] - np.max(x[t])
        branches = sorted(leaves, key=lambda e: (-e.nt, e.order))
        leaves = []
        for b in branches:
            b.ob, b.ol, b.ot = b.nb, b.nl, b.nt
        for b in branches:
            if b.parent is not None:
                if b.parent.active():
                    prev = b.parent.ob if b.label == b.parent.label else b.parent.ot
                    if prev != LOG_ZERO:
                        prev = prev + w_of[b]
                    b.nl = _lse(b.nl, prev)
                b.nl = b.nl + inp[b.label]
            b.nb = b.ot + inp[blank]
            b.nt = _lse(b.nb, b.nl)
            leaves.append(b)
        cache[0] = None

        def is_candidate(total):
            return total > LOG_ZERO and (len(leaves) < beam_width or
                                         total > bottom(leaves).nt)

        for b in branches:
            if not is_candidate(b.ot):
                continue
            if b.children is None:
                b.children = [new_entry(b, c) for c in range(C) if c != blank]
            for c in b.children:
                if c.active():
                    continue
                c.nb = LOG_ZERO
                prev = b.ob if c.label == b.label else b.ot
                c.nl = inp[c.label] + (prev + w_of[c]) if prev != LOG_ZERO else LOG_ZERO
                c.nt = c.nl
                if is_candidate(c.nt):
                    if len(leaves) == beam_width:
                        bt = bottom(leaves)
                        leaves.remove(bt)
                        bt.nb = bt.nl = bt.nt = LOG_ZERO
                    leaves.append(c)
                    cache[0] = None
                else:
                    c.ob = c.ol = c.ot = LOG_ZERO
                    c.nb = c.nl = c.nt = LOG_ZERO
    return min(leaves, key=lambda e: (-e.nt, e.order))


def beam_search_lm(logits, seq_len, beam_width, w=None, order=1, merge_repeated=True):
    """logits (T, N, C) -> (list of N label lists, list of N scores)."""
    logits = np.asarray(logits)
    out = [beam_search_lm_one(logits[:int(seq_len[n]), n], beam_width, w, order, merge_repeated)
           for n in range(logits.shape[1])]
    return [o[0] for o in out], [o[1] for o in out]


def estimate(sequences, K, order):
    """(n_ctx, K) float64 probabilities, interpolated Witten-Bell, by recursion on the history."""
    followers = {}                                  # history tuple (any length < order) -> counts
    for s in sequences:
        padded = [K] * (order - 1) + [int(c) for c in s]
        for i in range(order - 1, len(padded)):
            for k in range(order):
                g = tuple(padded[i - k:i])
                followers.setdefault(g, {})
                followers[g][padded[i]] = followers[g].get(padded[i], 0) + 1

    def prob(c, g):                                 # P_{len(g)+1}(c | g)
        lower = prob(c, g[1:]) if g else 1.0 / K
        cnt = followers.get(g)
        if not cnt:
            return lower
        n, d = sum(cnt.values()), len(cnt)
        return (cnt.get(c, 0) + d * lower) / (n + d)

    table = np.zeros((n_ctx(K, order), K), np.float64)
    for ctx in range(table.shape[0]):
        g, r = [], ctx
        for _ in range(order - 1):
            g.append(r % (K + 1))
            r //= K + 1
        g = tuple(g[::-1])                          # oldest first
        for c in range(K):
            table[ctx, c] = prob(c, g)
    return table


def bruteforce(logits, w, order):
    """dict labelling -> CTC log-score + sum of w along the labelling (tiny T, C)."""
    x = np.asarray(logits, dtype=np.float64)
    K = x.shape[1] - 1
    out = {}
    for lab, s in beam_search_bruteforce(x).items():
        ctx, tot = n_ctx(K, order) - 1, s
        for c in lab:
            tot += float(w[ctx, c])
            ctx = next_ctx(ctx, c, K, order)
        out[lab] = tot
    return out


# --------------------------------------------------------------------------- the toy task
LEXICON = [[0, 1, 2], [1, 3], [2, 0, 3, 1], [3, 3, 0], [1, 0, 2, 2]]     # letters 0..3
SPACE, TOY_K = 4, 5                                                       # 4 letters + space


def lexicon_corpus(seed=7, n_train=300, n_test=64):
    """(training label sequences, test truths, test logits (T, n_test, 6), test lengths).
    Sentences are 2-4 lexicon words joined by spaces; an utterance holds each label for 1-2
    frames, then 1-2 blanks, with +3.0 on the true class and 1.5 * N(0, 1) noise everywhere."""
    rs = np.random.RandomState(seed)

    def sentence():
        words = [LEXICON[rs.randint(len(LEXICON))] for _ in range(rs.randint(2, 5))]
        out = []
        for i, wd in enumerate(words):
            out += ([SPACE] if i else []) + list(wd)
        return out

    train = [sentence() for _ in range(n_train)]
    truths = [sentence() for _ in range(n_test)]
    C = TOY_K + 1
    frames = []
    for s in truths:
        f = []
        for c in s:
            f += [c] * rs.randint(1, 3) + [C - 1] * rs.randint(1, 3)
        frames.append(f)
    lens = np.array([len(f) for f in frames], np.int32)
    T = int(lens.max())
    x = (1.5 * rs.randn(T, n_test, C)).astype(np.float32)
    for n, f in enumerate(frames):
        x[np.arange(len(f)), n, f] += 3.0
    return train, truths, x, lens
