"""Float64 NumPy oracle of CTC forced alignment (K19) and the fixture set its tests share.

The lattice of a transcript of L labels has S = 2 L + 1 states: even s is a blank, odd s is label
(s - 1) / 2.  With e_t(s) the log-softmax of frame t at the class of state s,

    v_0(0) = e_0(0), v_0(1) = e_0(1), everything else -inf
    v_t(s) = e_t(s) + max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2))

the last term only for odd s whose label differs from label (s - 3) / 2; the path ends in state
2 L or 2 L - 1.  Ties: the smaller move wins (stay, then -1, then -2), and 2 L ends the path when
its value is >= that of 2 L - 1.  Written from this definition; vectorised over s."""
import numpy as np


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _lattice(label, blank):
    label = [int(l) for l in label]
    S = 2 * len(label) + 1
    cls = np.full(S, blank, np.int64)
    cls[1::2] = label
    skip = np.zeros(S, bool)                     # the move -2 INTO state s is legal
    for s in range(3, S, 2):
        skip[s] = cls[s] != cls[s - 2]
    return cls, skip


def viterbi(logp, label, blank, dtype=np.float64):
    """logp (T, C) log-softmax rows -> (score, path (T,) int array or None, gap).  ``gap`` is the
    distance from the best alignment to the best one that differs from it anywhere (inf when
    there is no other); score -inf, path None, gap nan when no alignment exists.  ``dtype``
    float32 runs the same recursion in single precision (the E32 measurement)."""
    logp = np.asarray(logp, dtype)
    T = logp.shape[0]
    cls, skip = _lattice(label, blank)
    S = len(cls)
    e = logp[:, cls]                             # (T, S)
    ninf = dtype(-np.inf)
    v = np.full((T, S), ninf, dtype)
    bp = np.zeros((T, S), np.int8)
    v[0, 0] = e[0, 0]
    if S > 1:
        v[0, 1] = e[0, 1]
    for t in range(1, T):
        a = v[t - 1]
        b = np.concatenate(([ninf], a[:-1]))
        c = np.where(skip, np.concatenate(([ninf, ninf], a[:-2]))[:S], ninf)
        best, k = a.copy(), np.zeros(S, np.int8)
        m = b > best
        best[m], k[m] = b[m], 1
        m = c > best
        best[m], k[m] = c[m], 2
        v[t] = best + e[t]
        bp[t] = k
    if S == 1 or v[T - 1, S - 1] >= v[T - 1, S - 2]:
        s = S - 1
    else:
        s = S - 2
    score = v[T - 1, s]
    if not score > ninf:
        return float('-inf'), None, float('nan')
    path = np.zeros(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        if t > 0:
            s -= int(bp[t, s])
    # backward Viterbi: w_t(s) = best completion from state s at frame t, emission of t excluded
    w = np.full((T, S), ninf, dtype)
    w[T - 1, S - 1] = 0
    if S > 1:
        w[T - 1, S - 2] = 0
    for t in range(T - 2, -1, -1):
        x = w[t + 1] + e[t + 1]
        x1 = np.concatenate((x[1:], [ninf]))
        x2 = np.concatenate((np.where(skip, x, ninf)[2:], [ninf, ninf]))[:S]
        w[t] = np.maximum(np.maximum(x, x1), x2)
    through = (v + w).astype(np.float64)
    through[np.arange(T), path] = -np.inf
    rest = through.max()
    return float(score), path, float(score) - float(rest)


def check_path(label, path):
    """Raises AssertionError unless ``path`` is a valid alignment of ``label``."""
    path = np.asarray(path, np.int64)
    L = len(label)
    assert path.ndim == 1 and len(path) >= 1, 'empty path'
    assert path[0] in (0, 1) and path[0] <= 2 * L, ('start', int(path[0]))
    assert path[-1] in (2 * L, 2 * L - 1) and path[-1] >= 0, ('end', int(path[-1]), L)
    mv = np.diff(path)
    assert np.all((mv >= 0) & (mv <= 2)), 'a move outside {0, 1, 2}'
    for t in np.nonzero(mv == 2)[0]:
        s = int(path[t + 1])
        assert s % 2 == 1 and s >= 3 and int(label[(s - 1) // 2]) != int(label[(s - 3) // 2]), \
            ('illegal skip into state', s, 'at frame', int(t) + 1)


def path_score(logp, label, path, blank=None):
    """Validates ``path`` and returns its float64 log-probability under ``logp`` (T, C)."""
    logp = np.asarray(logp, np.float64)
    blank = logp.shape[1] - 1 if blank is None else blank
    check_path(label, path)
    assert len(path) == logp.shape[0], (len(path), logp.shape[0])
    cls, _ = _lattice(label, blank)
    return float(logp[np.arange(len(path)), cls[np.asarray(path, np.int64)]].sum())


def paths_valid(path, labels, label_len, seq_len):
    """Vectorised validity of a whole (N, T) path array (labels (N, l_max) padded): True per row."""
    path = np.asarray(path, np.int64)
    N, T = path.shape
    ok = np.ones(N, bool)
    t = np.arange(T)[None, :]
    inside = t < np.asarray(seq_len)[:, None]
    ok &= np.all((path >= 0) == inside, axis=1)
    L = np.asarray(label_len, np.int64)
    last = path[np.arange(N), np.asarray(seq_len) - 1]
    ok &= (path[:, 0] <= 1) & (path[:, 0] <= 2 * L) & ((last == 2 * L) | (last == 2 * L - 1))
    mv = np.diff(path, axis=1)
    live = inside[:, 1:]
    ok &= np.all(~live | ((mv >= 0) & (mv <= 2)), axis=1)
    lab = np.asarray(labels, np.int64)
    lab = np.concatenate((lab, np.full((N, 2), -1, np.int64)), axis=1)
    s = np.where(live, path[:, 1:], 3)
    q = np.clip((s - 1) // 2, 1, lab.shape[1] - 1)
    rows = np.arange(N)[:, None]
    legal = (s % 2 == 1) & (s >= 3) & (lab[rows, q] != lab[rows, np.maximum(q - 1, 0)])
    ok &= np.all(~(live & (mv == 2)) | legal, axis=1)
    return ok


def brute_force(logp, label, blank):
    """Every alignment of a tiny case: (best score, its path) under the same tie rule, or
    (-inf, None).  Among equal scores the end state 2 L goes before 2 L - 1, then the path whose
    moves, read from the LAST frame backwards, are smallest wins -- what a backtrace that
    prefers small moves returns."""
    logp = np.asarray(logp, np.float64)
    T = logp.shape[0]
    cls, skip = _lattice(label, blank)
    S = len(cls)
    found = []

    def grow(path):
        if len(path) == T:
            if path[-1] in (S - 1, S - 2):
                found.append(tuple(path))
            return
        s = path[-1]
        for m in (0, 1, 2):
            if s + m < S and (m < 2 or skip[s + m]):
                grow(path + [s + m])

    for s0 in range(min(2, S)):
        grow([s0])
    best = (float('-inf'), None, None)
    for path in found:
        sc = float(sum(logp[t, cls[s]] for t, s in enumerate(path)))
        key = (-path[-1],) + tuple(path[i + 1] - path[i] for i in range(T - 1))[::-1]
        if sc > best[0] or (sc == best[0] and key < best[2]):
            best = (sc, np.array(path, np.int64), key)
    return best[0], best[1]


# --------------------------------------------------------------------------- fixtures
GAP_MIN = 1e-2          # nats: below it an utterance is left out of the exact-path comparison
SEED = 20240


def repeats(label):
    label = np.asarray(label)
    return int(np.sum(label[1:] == label[:-1])) if len(label) else 0


def random_label(rs, L, C, n_repeats=0):
    """L labels in [0, C-2] with exactly ``n_repeats`` adjacent equal pairs."""
    lab = []
    for _ in range(L - n_repeats):
        c = int(rs.randint(0, C - 1))
        while lab and c == lab[-1]:
            c = int(rs.randint(0, C - 1))
        lab.append(c)
    twice = set(rs.choice(len(lab), size=n_repeats, replace=False).tolist()) if n_repeats else ()
    return [c for i, c in enumerate(lab) for _ in range(2 if i in twice else 1)]


def random_alignment(rs, label, T):
    """A random valid state path of T frames for ``label`` (needs L + repeats <= T)."""
    L = len(label)
    states = []
    for q in range(L):
        forced = q > 0 and label[q] == label[q - 1]
        states.append([2 * q, forced])
        states.append([2 * q + 1, True])
    states.append([2 * L, L == 0])
    need = sum(1 for _, f in states if f)
    assert need <= T, (need, T)
    optional = [i for i, (_, f) in enumerate(states) if not f]
    rs.shuffle(optional)
    for i in optional[:min(len(optional), int(rs.randint(0, T - need + 1)))]:
        states[i][1] = True
    seq = [s for s, f in states if f]
    extra = T - len(seq)
    dur = np.ones(len(seq), np.int64)
    if extra:
        dur += np.bincount(rs.randint(0, len(seq), size=extra), minlength=len(seq))
    return np.repeat(seq, dur)


def _case(name, logits, labels, seq_len, n_pad, l_max=None):
    l_max = max([len(l) for l in labels] + [1]) if l_max is None else l_max
    return dict(name=name, logits=logits, labels=[list(l) for l in labels],
                seq_len=np.asarray(seq_len, np.int32), n_pad=n_pad, l_max=int(l_max),
                N=len(labels), T=logits.shape[0], C=logits.shape[2])


def _slab(rs, T, n_pad, C, labels=None, seq_len=None, plant=0.0):
    x = 3.0 * rs.randn(T, n_pad, C)
    if plant:
        for n, lab in enumerate(labels):
            Tn = int(seq_len[n])
            cls, _ = _lattice(lab, C - 1)
            x[np.arange(Tn), n, cls[random_alignment(rs, lab, Tn)]] += plant
    return x.astype(np.float32)


_F = None


def fixtures():
    """The fixture set F: a list of calls, each a dict (name, logits (T, n_pad, C) float32,
    labels, seq_len, n_pad, l_max, N, T, C).  Built once, never modified."""
    global _F
    if _F is not None:
        return _F
    rs = np.random.RandomState(SEED)
    F = []
    F.append(_case('T1', _slab(rs, 1, 16, 5), [[], [2]], [1, 1], 16))
    F.append(_case('T5', _slab(rs, 5, 16, 5), [[], [3, 0], [1, 1, 2], [0, 1, 2, 3, 0]],
                   [5, 5, 5, 5], 16))
    labs = [random_label(rs, 10, 29), random_label(rs, 24, 29), random_label(rs, 24, 29, 3)]
    F.append(_case('T50', _slab(rs, 50, 16, 29), labs, [50, 37, 26], 16))
    x70 = _slab(rs, 70, 16, 29)
    for k, L in enumerate((63, 64)):
        lab = random_label(rs, L, 29, 1)
        xs = x70.copy()
        xs[:, 0] = x70[:, k]
        F.append(_case('T70_L%d' % L, xs, [lab], [70], 16))
    for T, pair in ((140, (127, 128)), (270, (255, 256))):
        labs = [random_label(rs, L, 29, 2) for L in pair]
        xp = _slab(rs, T, 16, 29, labs, [T, T], plant=8.0)
        for k, L in enumerate(pair):
            xs = xp.copy()
            xs[:, 0] = xp[:, k]
            F.append(_case('T%d_L%d' % (T, L), xs, [labs[k]], [T], 16))
    labs = [random_label(rs, 511, 29, 2), random_label(rs, 511, 29, 3)]
    F.append(_case('T520_L511', _slab(rs, 520, 16, 29, labs, [520, 517], plant=8.0), labs,
                   [520, 517], 16))
    labs = [random_label(rs, int(rs.randint(0, 20)), 29, 0) for _ in range(17)]
    seq = [int(rs.randint(len(l) + 8, 51)) for l in labs]
    F.append(_case('T50_N17', _slab(rs, 50, 32, 29, labs, seq, plant=4.0), labs, seq, 32))
    _F = F
    return F


_REF = None


def reference():
    """Per call of F the oracle's (score, path, gap) per utterance, float64.  Computed once."""
    global _REF
    if _REF is None:
        _REF = []
        for c in fixtures():
            rows = []
            for n in range(c['N']):
                Tn = int(c['seq_len'][n])
                lp = log_softmax(c['logits'][:Tn, n])
                rows.append(viterbi(lp, c['labels'][n], c['C'] - 1))
            _REF.append(rows)
    return _REF


_E32 = None


def e32():
    """Largest relative deviation of the float32 recursion's score from the float64 one on F."""
    global _E32
    if _E32 is None:
        worst = 0.0
        for c, rows in zip(fixtures(), reference()):
            for n in range(c['N']):
                Tn = int(c['seq_len'][n])
                lp = log_softmax(c['logits'][:Tn, n]).astype(np.float32)
                s32, _, _ = viterbi(lp, c['labels'][n], c['C'] - 1, dtype=np.float32)
                worst = max(worst, abs(s32 - rows[n][0]) / max(1.0, abs(rows[n][0])))
        _E32 = worst
    return _E32


def tolerance(best):
    return 4.0 * e32() * max(1.0, abs(best))


def packed(case):
    """(labels (N, l_max) int32, label_len (N,) int32) of a call."""
    lab = np.zeros((case['N'], case['l_max']), np.int32)
    for n, l in enumerate(case['labels']):
        lab[n, :len(l)] = l
    return lab, np.array([len(l) for l in case['labels']], np.int32)


def compare(case, ref_rows, path, score, report=None):
    """The pass conditions of one call: every path valid, its float64 score and the returned
    float32 score within tolerance(best); exact path where the oracle's gap >= GAP_MIN.
    Returns (worst |path score - best| / tol, worst |score - best| / tol, utterances compared
    exactly)."""
    w1 = w2 = 0.0
    exact = 0
    for n in range(case['N']):
        best, want, gap = ref_rows[n]
        Tn = int(case['seq_len'][n])
        assert np.all(path[n, Tn:] == -1), (case['name'], n, 'frames past seq_len')
        if want is None:
            assert np.all(path[n] == -1) and score[n] == -np.inf, (case['name'], n, 'infeasible')
            continue
        lp = log_softmax(case['logits'][:Tn, n])
        got = path_score(lp, case['labels'][n], path[n, :Tn])
        tol = tolerance(best)
        d1, d2 = abs(got - best), abs(float(score[n]) - best)
        w1, w2 = max(w1, d1 / tol), max(w2, d2 / tol)
        if report is not None:
            report.append((case['name'], n, best, gap, d1, d2, tol))
        assert d1 <= tol, (case['name'], n, 'path score', got, best, tol)
        assert d2 <= tol, (case['name'], n, 'score', float(score[n]), best, tol)
        if gap >= GAP_MIN:
            exact += 1
            assert np.array_equal(path[n, :Tn], want), (case['name'], n, 'path', gap)
    return w1, w2, exact
