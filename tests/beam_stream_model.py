"""Resumable restatement of tests/beam_device_model.py: the model of the STREAM form of the device
beam-search kernel (csrc/beam.hip, K27).  TEST INFRASTRUCTURE ONLY.

The frame step is beam_device_model's, phase by phase; what changes is that everything a frame
hands to the next is explicit state of a ``BeamStream`` -- the branch table (b_node, b_par, b_ob,
b_ol, b_ot), the tree (children, turn, block_parent), frames_done and stable_node -- so frames can
arrive in chunks.  After a chunk the model also gives what the kernel gives: the best hypothesis,
its score, and the STABLE PREFIX: the labels on the path from the root to the deepest common
ancestor of all beam entries, computed as the kernel computes it (ids grow from parent to child,
two nodes meet by replacing the larger id by its parent, every walk stops at the stable node of
the chunk before)."""
import numpy as np

from tests.beam_device_model import NEG, _lse


class BeamStream(object):
    def __init__(self, C, W, merge_repeated=True):
        self.C, self.K, self.W, self.merge = C, C - 1, W, merge_repeated
        self.children = {0: -1}
        self.turn = {0: 0}
        self.block_parent = []
        self.b_node, self.b_par = [0], [-1]
        self.b_ob, self.b_ol, self.b_ot = [0.0], [NEG], [0.0]
        self.frames_done = 0
        self.stable_node = 0

    # ------------------------------------------------------------------ one frame
    def _frame(self, row):
        K, blank, W = self.K, self.C - 1, self.W
        children, turn, block_parent = self.children, self.turn, self.block_parent
        b_node, b_par, b_ob, b_ol, b_ot = self.b_node, self.b_par, self.b_ob, self.b_ol, self.b_ot
        inp = row.astype(np.float64) - np.float64(row.max())
        nb = len(b_node)
        b_ot0 = list(b_ot)
        b_nb, b_nl, b_nt = [NEG] * nb, [NEG] * nb, [NEG] * nb
        b_pt, b_nkids, b_evicted = [-1] * nb, [0] * nb, [False] * nb
        for q in range(nb):                                             # phase B
            node, par = b_node[q], b_par[q]
            nl = b_ol[q]
            if par >= 0:
                label = (node - 1) % K
                pt = turn.get(par, -1)
                b_pt[q] = pt
                if pt >= 0:
                    plabel = -1 if par == 0 else (par - 1) % K
                    nl = _lse(nl, b_ob[pt] if label == plabel else b_ot[pt])
                    b_nkids[pt] += 1
                nl = nl + inp[label]
            b_nb[q] = b_ot[q] + inp[blank]
            b_nl[q] = nl
            b_nt[q] = _lse(b_nb[q], nl)
        hn = nb                                                         # phase C
        h = [None] * nb
        for q in range(nb):
            p = sum(1 for j in range(nb)
                    if b_nt[j] > b_nt[q] or (b_nt[j] == b_nt[q] and b_node[j] < b_node[q]))
            h[p] = [b_nt[q], b_node[q], b_par[q], q]
        for r in range(nb):                                             # phase D
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
                v.append(NEG if prev == NEG else inp[c] + prev)
            undecided = set(range(K))
            while undecided:
                fullk = hn == W
                th = h[W - 1][0] if fullk else NEG
                cand = []
                for c in sorted(undecided):
                    if kid[c] >= 0 and not b_evicted[kid[c]]:
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
        for q in range(nb):                                             # phase E
            turn[b_node[q]] = -1
        n_node, n_par, n_ob, n_ol, n_ot = [], [], [], [], []
        for j in range(hn):
            nt, node, par, ref = h[j]
            n_node.append(node)
            n_par.append(par)
            n_ob.append(b_nb[ref] if ref >= 0 else NEG)
            n_ol.append(b_nl[ref] if ref >= 0 else nt)
            n_ot.append(nt)
            turn[node] = j
        self.b_node, self.b_par, self.b_ob, self.b_ol, self.b_ot = n_node, n_par, n_ob, n_ol, n_ot

    # ------------------------------------------------------------------ the calls
    def parent(self, c):
        return self.block_parent[(c - 1) // self.K]

    def feed(self, chunk):
        """chunk (t, C), t >= 0 frames -> (best labels, score, stable_len)."""
        chunk = np.asarray(chunk, np.float32).reshape(-1, self.C)
        for row in chunk:
            self._frame(row)
        self.frames_done += len(chunk)
        # the stable node, as the kernel walks: each entry against the best one
        best, stop = self.b_node[0], self.stable_node
        lo = best
        for a in self.b_node:
            b = best
            while a != b and a != stop and b != stop:
                if a > b:
                    a = self.parent(a)
                else:
                    b = self.parent(b)
            lo = min(lo, a, b)
        self.stable_node = lo
        labels, score = self.best()
        return labels, score, len(self.merged(self.path(lo)))

    def path(self, c):
        """The unmerged labels root -> c."""
        out = []
        while c != 0:
            out.append((c - 1) % self.K)
            c = self.parent(c)
        return out[::-1]

    def merged(self, labels):
        if not self.merge:
            return list(labels)
        return [l for i, l in enumerate(labels) if i == 0 or l != labels[i - 1]]

    def best(self):
        return self.merged(self.path(self.b_node[0])), float(self.b_ot[0])

    def table(self):
        """The branch table as the kernel's state record holds it."""
        return dict(nb=len(self.b_node), nblocks=len(self.block_parent),
                    frames_done=self.frames_done, stable_node=self.stable_node,
                    b_node=list(self.b_node), b_par=list(self.b_par), b_ob=list(self.b_ob),
                    b_ol=list(self.b_ol), b_ot=list(self.b_ot))


def beam_stream_model(logits, W, splits, merge_repeated=True):
    """logits (T, C) fed in chunks of ``splits`` frames -> (BeamStream, [(labels, score,
    stable_len) after every chunk])."""
    x = np.asarray(logits, np.float32)
    assert sum(splits) == len(x)
    st, outs, pos = BeamStream(x.shape[1], W, merge_repeated), [], 0
    for s in splits:
        outs.append(st.feed(x[pos:pos + s]))
        pos += s
    return st, outs
