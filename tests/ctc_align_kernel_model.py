"""The K19 kernels of csrc/ctc.hip as a sequential NumPy model: the same lane geometry (lane k
owns the PPL state pairs k PPL .. k PPL + PPL - 1), the same float32 base-2 arithmetic, wave
shift, strict-greater tie rule, 4-bit back-pointer fields, per-group re-centring with a float64
offset, end-state rule and group-staged backtrace.  It exists so that the kernel's LOGIC (bit
layout, indexing, ties) is checked against the oracle on a machine without a GPU; the kernel
itself is checked by tests/test_gpu_ctc_align.py."""
import numpy as np

LOG2E = np.float32(1.4426950408889634)
LN2 = 0.6931471805599453
NINF = np.float32(-np.inf)
BT_GROUP = 64


def pick_ppl(l_max):
    pairs = l_max + 1
    for ppl, cap in ((1, 64), (2, 128), (4, 256), (8, 512)):
        if pairs <= cap:
            return ppl
    return 0


def lane_init(labels_row, L, C, ppl):
    """CtcLane<PPL>::init for all 64 lanes: lab, valid, diffp of shape (64, PPL)."""
    blank = C - 1
    lab = np.full((64, ppl), blank, np.int64)
    valid = np.zeros((64, ppl), bool)
    diffp = np.zeros((64, ppl), bool)
    for lane in range(64):
        for p in range(ppl):
            q = lane * ppl + p
            valid[lane, p] = q < L
            raw = int(labels_row[q]) if valid[lane, p] else blank
            prev = int(labels_row[q - 1]) if (q >= 1 and q - 1 < L) else -1
            diffp[lane, p] = valid[lane, p] and (q == 0 or raw != prev)
            lab[lane, p] = blank if (raw < 0 or raw >= C) else raw
    return lab, valid, diffp


def viterbi_step(sb, sl, eb, el, valid, diffp):
    """One frame for the whole wave; returns the 64 back-pointer words."""
    ppl = sb.shape[1]
    lprev = np.concatenate(([NINF], sl[:-1, ppl - 1]))          # wave_shift_up, fill -inf
    nsb, nsl = np.empty_like(sb), np.empty_like(sl)
    w = np.zeros(64, np.uint32)
    for p in range(ppl):
        lp1 = lprev if p == 0 else sl[:, p - 1]
        b1 = lp1 > sb[:, p]
        nsb[:, p] = np.maximum(sb[:, p], lp1) + eb
        l1 = sb[:, p] > sl[:, p]
        m1 = np.maximum(sl[:, p], sb[:, p])
        l2 = diffp[:, p] & (lp1 > m1)
        nsl[:, p] = np.where(l2, lp1, m1) + np.where(valid[:, p], el[:, p], NINF)
        field = b1.astype(np.uint32) | np.where(l2, 8, np.where(l1, 4, 0)).astype(np.uint32)
        w |= field << np.uint32(4 * p)
    return nsb, nsl, w


def align_one(logits, labels_row, L, Tn, l_max):
    """logits (T, C) float32 of one utterance -> (path (T,) int32, score float32)."""
    T, C = logits.shape
    ppl = pick_ppl(l_max)
    unr = {1: 16, 2: 8}.get(ppl, 4)
    Tn = min(max(int(Tn), 1), T)
    L = min(max(int(L), 0), l_max)
    lab, valid, diffp = lane_init(labels_row, L, C, ppl)
    x = logits.astype(np.float32)
    m = x.max(axis=1)
    with np.errstate(over='ignore'):
        lse = (m + np.log(np.exp(x - m[:, None]).sum(axis=1, dtype=np.float32))).astype(np.float32)
    sb = np.full((64, ppl), NINF, np.float32)
    sl = np.full((64, ppl), NINF, np.float32)
    sb[0, 0] = 0
    off = 0.0
    word_bits = {1: 8, 2: 8, 4: 16, 8: 32}[ppl]
    bp = np.full((T, 64), 0xFFFFFFFF >> (32 - word_bits), np.uint32)    # dirty workspace
    for t in range(Tn):
        if t % unr == 0:                                             # recentre once per group
            mx = max(sb.max(), sl.max())
            if mx > NINF:
                sb, sl = sb - mx, sl - mx
                off += float(mx)
        eb = (x[t, C - 1] - lse[t]) * LOG2E
        el = (x[t, lab] - lse[t]) * LOG2E
        with np.errstate(invalid='ignore'):
            sb, sl, w = viterbi_step(sb, sl, np.float32(eb), el.astype(np.float32), valid, diffp)
        assert int(w.max()) < (1 << word_bits)
        bp[t] = w
    fin = np.stack((sb, sl), axis=2).reshape(-1)                      # fin[2 q], fin[2 q + 1]
    e1 = fin[2 * L]
    e2 = fin[2 * (L - 1) + 1] if L > 0 else NINF
    last_blank = e1 >= e2
    best = e1 if last_blank else e2
    path = np.full(T, -1, np.int32)
    if not best > NINF:
        return path, NINF
    score = np.float32((float(best) + off) * LN2)
    s = 2 * L if last_blank else 2 * L - 1
    ngroups = (Tn + BT_GROUP - 1) // BT_GROUP
    for g in range(ngroups - 1, -1, -1):
        lo, hi = g * BT_GROUP, min(Tn, (g + 1) * BT_GROUP)
        rows = bp[[min(lo + j, Tn - 1) for j in range(BT_GROUP)]]    # the staged group
        for t in range(hi - 1, lo - 1, -1):
            path[t] = s
            q = s >> 1
            word = int(rows[t - lo, q // ppl])
            mv = (word >> (4 * (q % ppl) + 2 * (s & 1))) & 3
            s = max(s - mv, 0) if t > 0 else s
    return path, score


def align(logits, labels, label_len, seq_len, N):
    """The call as ops.ctc_align_host takes it -> (path (N, T) int32, score (N,) float32)."""
    T = logits.shape[0]
    path = np.empty((N, T), np.int32)
    score = np.empty(N, np.float32)
    for n in range(N):
        path[n], score[n] = align_one(logits[:, n], labels[n], label_len[n], seq_len[n],
                                      labels.shape[1])
    return path, score
