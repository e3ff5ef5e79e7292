"""The loss/gradient kernels of csrc/ctc.hip (K7) as a sequential NumPy float32 model of one
utterance: base-2 log space with lse2 as max + log2(1 + 2^(min - max)), emissions as
(logit - lse) * log2 e, the alpha~ / beta~ chains re-centred on the row maximum once per prefetch
group of UNR frames (the removed amount of the alpha chain summed in float64 for the loss), a
checkpoint of both every 16 frames, and the gradient of frame t from rows re-derived from the
nearest checkpoints (or from the virtual frame Tn), the posteriors normalised by their own sum.

The cross-lane shift only moves a value to the neighbouring state pair, so the model keeps the
64 * PPL pairs in flat arrays; what depends on PPL is the alpha_step formula (PPL == 1: a
three-way sum, PPL > 1: the blank's sum re-used) and UNR.  It exists to show, without a GPU and
independently of the kernel, that the tolerance of tests/test_gpu_ctc.py is reachable in float32
on the inputs of tests/ctc_cases.py (tests/test_ctc_loss_model_host.py)."""
import numpy as np

from tests.ctc_align_kernel_model import pick_ppl

F32 = np.float32
LOG2E = F32(1.4426950408889634)
LN2 = 0.6931471805599453
NINF = F32(-np.inf)
FLOOR = F32(-3.0e38)
CK = 16


def unr_of(ppl):
    return {1: 16, 2: 8}.get(ppl, 4)


def lse2(a, b):
    m = np.maximum(a, b)
    d = np.minimum(a, b) - np.maximum(m, FLOOR)
    return (m + np.log2(F32(1) + np.exp2(d))).astype(F32)


def lse3(a, b, c):
    m = np.maximum(np.maximum(a, b), c)
    f = np.maximum(m, FLOOR)
    mn = np.minimum(np.minimum(a, b), c)
    md = np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c))
    return (m + np.log2(F32(1) + np.exp2(md - f) + np.exp2(mn - f))).astype(F32)


class Lane(object):
    """CtcLane<PPL> for the whole wave: lab / valid / diffp of the 64 * PPL state pairs."""

    def __init__(self, labels_row, L, C, ppl):
        self.ppl, self.P = ppl, 64 * ppl
        blank = C - 1
        q = np.arange(self.P)
        self.valid = q < L
        lab = np.full(self.P, blank, np.int64)
        lab[:L] = np.asarray(labels_row[:L], np.int64)
        prev = np.concatenate(([-1], lab[:-1]))
        self.diffp = self.valid & ((q == 0) | (lab != prev))
        self.lab = np.where((lab < 0) | (lab >= C), blank, lab)

    def alpha_step(self, sb, sl, eb, el):
        lp1 = np.concatenate(([NINF], sl[:-1]))
        x = lse2(sb, lp1)
        e = np.where(self.valid, el, NINF)
        if self.ppl == 1:
            nsl = lse3(sl, sb, np.where(self.diffp, lp1, NINF)) + e
        else:
            nsl = lse2(sl, np.where(self.diffp, x, sb)) + e
        return (x + eb).astype(F32), nsl.astype(F32)

    def beta_step(self, sb, sl, eb, el):
        xb = (sb + eb).astype(F32)
        xl = np.where(self.valid, sl + el, NINF).astype(F32)
        y = lse2(xb, np.where(self.diffp, xl, NINF))
        yn = np.concatenate((y[1:], [NINF]))
        return lse2(xb, xl), np.where(self.valid, lse2(xl, yn), NINF).astype(F32)


def row_lse(x):
    """ctc_lse_kernel: float32 max, sum of exponentials and natural log."""
    m = x.max(axis=1)
    return (m + np.log(np.exp(x - m[:, None]).sum(axis=1, dtype=F32))).astype(F32)


def _recentre(sb, sl):
    m = max(sb.max(), sl.max())
    if m > NINF:
        return sb - m, sl - m, float(m)
    return sb, sl, 0.0


def loss_grad_one(logits, labels_row, L, Tn, l_max, scale=1.0, return_rows=False):
    """logits (T, C) float32 of one utterance -> (loss float32, grad (T, C) float32)."""
    x = np.asarray(logits, F32)
    T, C = x.shape
    blank = C - 1
    ppl = pick_ppl(l_max)
    unr = unr_of(ppl)
    Tn = min(max(int(Tn), 1), T)
    L = min(max(int(L), 0), l_max)
    ln = Lane(labels_row, L, C, ppl)
    lse = row_lse(x)
    with np.errstate(invalid='ignore', over='ignore'):
        eb_all = ((x[:, blank] - lse) * LOG2E).astype(F32)
        el_all = ((x[:, ln.lab] - lse[:, None]) * LOG2E).astype(F32)
        zero_l = np.zeros(ln.P, F32)

        # ---- alpha chain
        sb = np.full(ln.P, NINF, F32)
        sl = np.full(ln.P, NINF, F32)
        sb[0] = 0
        off = 0.0
        alpha_ck = {}
        for t in range(Tn):
            if t % unr == 0:
                sb, sl, m = _recentre(sb, sl)
                off += m
            sb, sl = ln.alpha_step(sb, sl, eb_all[t], el_all[t])
            if t % CK == 0:
                alpha_ck[t] = (sb, sl)
        e1 = sb[L]
        e2 = sl[L - 1] if L > 0 else NINF
        lz = float(lse2(e1, e2)) + off
        loss = F32(-lz * LN2)
        grad = np.zeros((T, C), F32)
        if not lz > -1.0e300:
            return (loss, grad, {}, {}) if return_rows else (loss, grad)

        # ---- beta chain: group g covers t = Tn - 1 - g UNR - u, emissions of frame t + 1
        def beta_em(t):
            return (F32(0), zero_l) if t + 1 >= Tn else (eb_all[t + 1], el_all[t + 1])

        sb = np.full(ln.P, NINF, F32)
        sl = np.full(ln.P, NINF, F32)
        sb[L] = 0
        beta_ck = {}
        for k in range(Tn):
            t = Tn - 1 - k
            if k % unr == 0:
                sb, sl, _ = _recentre(sb, sl)
            sb, sl = ln.beta_step(sb, sl, *beta_em(t))
            if t % CK == 0:
                beta_ck[t] = (sb, sl)

        # ---- gradient: the rows of frame t from the nearest checkpoints.  All frames of a
        # 16-frame block walk the same sequence of steps, so one walk per block serves them.
        a_rows, b_rows = {}, {}
        for t0 in range(0, Tn, CK):
            ab, al = alpha_ck[t0]
            a_rows[t0] = (ab, al)
            for f in range(t0 + 1, min(t0 + CK, Tn)):
                ab, al = ln.alpha_step(ab, al, eb_all[f], el_all[f])
                a_rows[f] = (ab, al)
            b_rows[t0] = beta_ck[t0]
            t1 = t0 + CK
            if t1 <= Tn - 1:
                bb, bl = beta_ck[t1]
                tau = t1
            else:
                bb = np.full(ln.P, NINF, F32)
                bl = np.full(ln.P, NINF, F32)
                bb[L] = 0
                tau = Tn
            for f in range(tau - 1, t0, -1):
                bb, bl = ln.beta_step(bb, bl, *beta_em(f))
                b_rows[f] = (bb, bl)
        q = np.arange(ln.P)
        for t in range(Tn):
            vb = np.where(q <= L, a_rows[t][0] + b_rows[t][0], NINF).astype(F32)
            vl = np.where(q < L, a_rows[t][1] + b_rows[t][1], NINF).astype(F32)
            vmax = max(vb.max(), vl.max())
            if not vmax > NINF:
                continue
            pb = np.exp2(vb - vmax).astype(F32)
            pl = np.exp2(vl - vmax).astype(F32)
            zsum = F32(pb.sum(dtype=F32) + pl.sum(dtype=F32))
            if not zsum > 0:
                continue
            inv = F32(1) / zsum
            bins = np.zeros(C, F32)
            np.add.at(bins, ln.lab[:L], (pl[:L] * inv).astype(F32))
            bins[blank] += (pb * inv).sum(dtype=F32)
            grad[t] = F32(scale) * (np.exp(x[t] - lse[t]).astype(F32) - bins)
    if return_rows:
        return loss, grad, a_rows, b_rows
    return loss, grad


def loss_grad(logits, labels, seq_len, scale=1.0):
    """A batch as tests/ctc_cases.py builds it -> (loss (N,), grad (T, N, C)) float32."""
    T, N, C = logits.shape
    l_max = max([len(l) for l in labels] + [1])
    loss = np.empty(N, F32)
    grad = np.zeros((T, N, C), F32)
    for n in range(N):
        loss[n], grad[:, n] = loss_grad_one(logits[:, n], labels[n], len(labels[n]), seq_len[n],
                                            l_max, scale)
    return loss, grad
