"""tests/beam_device_model.py with the character-LM hooks of csrc/beam.hip's LM = true
instantiations.  TEST INFRASTRUCTURE ONLY: the CPU suite checks with it, without a GPU, that the
kernel's phase structure stays the same function as the oracle (tests/clm_oracle.py) when
w_e = w[ctx(parent), label] is added at the two scorer hooks -- in particular with w_e > 0, when a
child can outscore its parent while the turn loop still ends at the first branch whose ORIGINAL
old total does not beat the bottom of a full beam.

What is modelled on top of beam_device_model: ``block_ctx`` (the context of the node that owns a
child block, written at the block's first expansion), ``b_ctx`` (the context of every branch of
the frame, handed over in phase E: a surviving branch keeps its own, a new child gets
next(block_ctx[its block], its label)), the one float of phase B and the row of phase D.
"""
import numpy as np

NEG = -np.inf


def _lse(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + np.log(np.exp(a - m) + np.exp(b - m))


def beam_device_lm_model(logits, W, w, order, merge_repeated=True):
    x = np.asarray(logits, np.float32)
    T, C = x.shape
    K, blank = C - 1, C - 1
    children = {0: -1}                  # node -> child block (rec[].children)
    turn = {0: 0}                       # node -> branch index (rec[].turn), -1 / absent = not in beam
    block_parent, block_ctx = [], []
    n_ctx = C ** (order - 1)
    b_ctx = [n_ctx - 1]
    # branch table
    b_node, b_par = [0], [-1]
    b_ob, b_ol, b_ot = [0.0], [NEG], [0.0]
    for t in range(T):
        inp = x[t].astype(np.float64) - np.float64(x[t].max())
        nb = len(b_node)
        b_ot0 = list(b_ot)
        b_nb, b_nl, b_nt = [NEG] * nb, [NEG] * nb, [NEG] * nb
        b_pt, b_nkids, b_evicted = [-1] * nb, [0] * nb, [False] * nb
        # phase B: every branch in parallel
        for q in range(nb):
            node, par = b_node[q], b_par[q]
            nl = b_ol[q]
            if par >= 0:
                label = (node - 1) % K
                pt = turn.get(par, -1)
                b_pt[q] = pt
                if pt >= 0:
                    plabel = -1 if par == 0 else (par - 1) % K
                    prev = b_ob[pt] if label == plabel else b_ot[pt]
                    nl = _lse(nl, prev + float(w[b_ctx[pt], label]))
                    b_nkids[pt] += 1
                nl = nl + inp[label]
            b_nb[q] = b_ot[q] + inp[blank]
            b_nl[q] = nl
            b_nt[q] = _lse(b_nb[q], nl)
        # phase C: rank sort into the beam array
        hn = nb
        h = [None] * nb
        for q in range(nb):
            p = sum(1 for j in range(nb)
                    if b_nt[j] > b_nt[q] or (b_nt[j] == b_nt[q] and b_node[j] < b_node[q]))
            h[p] = [b_nt[q], b_node[q], b_par[q], q]
        # phase D: branch turns
        for r in range(nb):
            full = hn == W
            theta = h[W - 1][0] if full else NEG
            if full and not (b_ot0[r] > theta):
                break
            ot = b_ot[r]
            if not (ot > NEG and (not full or ot > theta)):
                continue
            ob, node = b_ob[r], b_node[r]
            blk = children[node]
            if blk < 0:
                blk = len(block_parent)
                block_parent.append(node)
                block_ctx.append(b_ctx[r])
                children[node] = blk
                for c in range(K):
                    children[1 + blk * K + c] = -1
            base = 1 + blk * K
            blabel = -1 if node == 0 else (node - 1) % K
            kid = [-1] * K
            if b_nkids[r] > 0:
                for j in range(nb):
                    if b_pt[j] == r:
                        kid[(b_node[j] - 1) % K] = j
            v = []
            for c in range(K):
                prev = ob if c == blabel else ot
                v.append(NEG if prev == NEG else inp[c] + (prev + float(w[b_ctx[r], c])))
            undecided = set(range(K))
            while undecided:
                fullk = hn == W
                th = h[W - 1][0] if fullk else NEG
                cand = []
                for c in sorted(undecided):
                    active = kid[c] >= 0 and not b_evicted[kid[c]]
                    if active:
                        continue
                    if v[c] > NEG and (not fullk or v[c] > th):
                        cand.append(c)
                    else:
                        if kid[c] >= 0:
                            b_ob[kid[c]] = b_ol[kid[c]] = b_ot[kid[c]] = NEG
                        undecided.discard(c)
                if not cand:
                    break
                cs = cand[0]
                undecided = {c for c in undecided if c > cs}
                if fullk:
                    rb = h[W - 1][3]
                    if rb >= 0:
                        b_evicted[rb] = True
                    hn = W - 1
                    h.pop()
                vs, nid = v[cs], base + cs
                p = sum(1 for j in range(hn) if h[j][0] > vs or (h[j][0] == vs and h[j][1] < nid))
                h.insert(p, [vs, nid, node, -1])
                hn += 1
        # phase E: the beam becomes the next frame's branch table
        for q in range(nb):
            turn[b_node[q]] = -1
        nb2 = hn
        n_node, n_par, n_ob, n_ol, n_ot, n_ctxs = [], [], [], [], [], []
        for j in range(nb2):
            nt, node, par, ref = h[j]
            n_node.append(node)
            n_par.append(par)
            n_ob.append(b_nb[ref] if ref >= 0 else NEG)
            n_ol.append(b_nl[ref] if ref >= 0 else nt)
            n_ot.append(nt)
            n_ctxs.append(b_ctx[ref] if ref >= 0 else
                          (block_ctx[(node - 1) // K] * C + (node - 1) % K) % n_ctx)
            turn[node] = j
        b_node, b_par, b_ob, b_ol, b_ot, b_ctx = n_node, n_par, n_ob, n_ol, n_ot, n_ctxs
    best, score = b_node[0], b_ot[0]
    out, prev, c = [], -1, best
    while c != 0:
        label = (c - 1) % K
        if not merge_repeated or label != prev:
            out.append(label)
        prev = label
        c = block_parent[(c - 1) // K]
    return out[::-1], float(score)
