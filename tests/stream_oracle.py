"""float64 NumPy restatement of cached chunk-by-chunk inference (K26, asr_study_amd/core/stream.py)
for models without a front-end: the stage chains of tests/window_oracle.py run on a few new frames
at a time, carrying EXPLICIT state -- per attention stage the lists of all keys and values so far,
per depthwise convolution the last k - 1 input frames, for the greedy decoder the last label.
Every stage kind that is per-frame at inference is delegated, frame block by frame block, to
window_oracle.model_forward.  What it must equal is window_oracle.model_forward on the whole
utterance (tests/test_stream_host.py, 1e-12).  Test infrastructure only.
"""
import numpy as np

from tests import attention_oracle as AO
from tests import relattention_oracle as RO
from tests import window_oracle as WO

NO_END = 1 << 30


def ring_rows(window, max_tq, tile=WO.TILE, horizon=None):
    """Brute force: the smallest multiple of `tile` that holds, for every first new frame t0 and
    max_tq new frames, everything from the key tile of lo(t0) to the last new frame."""
    return -(-(ring_span(window, tile, horizon) + max_tq) // tile) * tile


def ring_span(window, tile=WO.TILE, horizon=None):
    """max over t0 < horizon of t0 - lo(t0) // tile * tile: what a ring holds before the new
    frames.  The default horizon spans every residue of lo(t0) % tile: lo advances by `chunk`, so
    tile chunks past the first chunk with c0 >= left repeat."""
    chunk, left, right = window
    assert left >= 0 and right == 0
    horizon = horizon or (left + (tile + 2) * chunk + tile)
    t0 = np.arange(horizon)
    lo = np.maximum(0, t0 // chunk * chunk - left)
    return int((t0 - lo // tile * tile).max())


def attn_chunk(q, K, V, t0, heads, window, lens, pos=None, bias_u=None, bias_v=None):
    """q (Tq, N, D): the queries t0 .. t0 + Tq - 1; K, V (t0 + Tq, N, D): every key and value so
    far; lens (N) absolute.  pos: None (K21) or the projected (2P - 1, D) table (K24).  Query by
    query, the definition: key u is visible iff lo(t) <= u < hi(t), u < lens[n], u < t0 + Tq."""
    Tq, N, D = q.shape
    dh = D // heads
    chunk, left, _ = window
    scale = 1.0 / np.sqrt(dh)
    out = np.zeros((Tq, N, D))
    P = None if pos is None else (pos.shape[0] + 1) // 2
    for i in range(Tq):
        t = t0 + i
        c0 = t // chunk * chunk
        lo = max(0, c0 - left)
        for n in range(N):
            hi = min(c0 + chunk, int(lens[n]), t0 + Tq)
            if hi <= lo:
                continue                    # no visible key: out = 0
            for h in range(heads):
                cs = slice(h * dh, (h + 1) * dh)
                qt, k, v = q[i, n, cs], K[lo:hi, n, cs], V[lo:hi, n, cs]
                if pos is None:
                    s = k @ qt
                else:
                    rel = pos[t - np.arange(lo, hi) + P - 1][:, cs]
                    s = k @ (qt + bias_u[cs]) + rel @ (qt + bias_v[cs])
                s = scale * s
                p = np.exp(s - s.max())
                out[i, n, cs] = (p / p.sum()) @ v
    return out


def dwconv_chunk(x, tail, w, b, t0, lens):
    """x (Tq, N, C): the input frames t0 .. t0 + Tq - 1, tail (k - 1, N, C): the k - 1 masked
    frames before them (zeros before the stream) -> y (Tq, N, C), the new tail."""
    Tq, N, C = x.shape
    k = w.shape[0]
    m = (t0 + np.arange(Tq))[:, None] < np.asarray(lens)[None, :]
    xm = np.concatenate([tail, np.where(m[:, :, None], x, 0.0)], 0)
    y = np.zeros((Tq, N, C)) + b
    for j in range(k):
        y += w[j] * xm[j:j + Tq]
    return y, xm[xm.shape[0] - (k - 1):]


def greedy_chunk(logits, chunk_len, last):
    """logits (Tq, N, C), chunk_len (N) valid frames of this chunk, last (N) the arg-max of the
    stream's last valid frame (-1: none) -> labels added per stream, the new last."""
    Tq, N, C = logits.shape
    out, last = [[] for _ in range(N)], list(last)
    for n in range(N):
        for t in range(int(chunk_len[n])):
            best = int(np.argmax(logits[t, n]))         # (first maximum)
            if best != C - 1 and best != last[n]:
                out[n].append(best)
            last[n] = best
    return out, last


class Stream(object):
    """The session's schedule without a front-end: whole steps of `step` frames as the input
    allows, the remainder at finish()."""

    def __init__(self, stages, N, step):
        self.stages, self.N, self.step = stages, N, step
        self.lens = np.full(N, NO_END, np.int64)
        self.t0 = 0
        self.pend = None
        self.state = {}
        self.last = [-1] * N

    def feed(self, x, ended=None):
        """x (t, N, F) -> logits (new, N, C) of the steps the input now allows."""
        self._ended(ended)
        self.pend = x if self.pend is None else np.concatenate([self.pend, x], 0)
        outs = []
        while self.pend.shape[0] >= self.step:
            outs.append(self._step(self.pend[:self.step]))
            self.pend = self.pend[self.step:]
        return self._cat(outs)

    def finish(self):
        total = self.t0 + (0 if self.pend is None else self.pend.shape[0])
        self.lens = np.minimum(self.lens, total)
        outs = [self._step(self.pend)] if self.pend is not None and self.pend.shape[0] else []
        self.pend = None
        return self._cat(outs)

    def _ended(self, ended):
        for n, e in enumerate(ended or []):
            if e is not None:
                self.lens[n] = e

    def _cat(self, outs):
        return np.concatenate(outs, 0) if outs else None

    def _step(self, a):
        t0, Tq = self.t0, a.shape[0]
        m = (t0 + np.arange(Tq))[:, None] < self.lens[None, :]
        a = np.where(m[:, :, None], a, 0.0)             # an ended stream is fed zeros
        outs = []
        for si, st in enumerate(self.stages):
            t = st['type']
            if t in ('mha', 'relmha'):
                a = self._mha(si, st, a, t0)
            elif t == 'dwconv':
                tail = self.state.get(si)
                if tail is None:
                    tail = np.zeros((st['W'].shape[0] - 1,) + a.shape[1:])
                a, self.state[si] = dwconv_chunk(a, tail, st['W'], st['b'], t0, self.lens)
            elif t == 'posenc':
                a = a + AO.posenc(t0 + Tq, a.shape[2])[t0:, None, :]
            elif t == 'merge':
                a = st['coef'] * (st['scale'] * a + outs[st['skip']])
            else:                                       # per frame at inference
                a, _ = WO.model_forward([st], a, None, training=False)
            outs.append(a)
        self.t0 += Tq
        return a

    def _mha(self, si, st, a, t0):
        D = st['W_o'].shape[0]
        qkv = a @ st['W_qkv'] + st['b_qkv']
        K, V = self.state.get(si, (np.zeros((0,) + a.shape[1:2] + (D,)),) * 2)
        K = np.concatenate([K, qkv[:, :, D:2 * D]], 0)
        V = np.concatenate([V, qkv[:, :, 2 * D:3 * D]], 0)
        self.state[si] = (K, V)
        kw = {}
        if st['type'] == 'relmha':
            chunk, left, _ = st['window']
            pe = RO.relpos(left + chunk, st['W_pos'].shape[0])
            kw = dict(pos=pe @ st['W_pos'], bias_u=st['bias_u'].reshape(-1),
                      bias_v=st['bias_v'].reshape(-1))
        ctx = attn_chunk(qkv[:, :, :D], K, V, t0, st['heads'], st['window'], self.lens, **kw)
        return ctx @ st['W_o'] + st['b_o']


def model_stream(stages, x, lens, pieces, step, ended_at=None):
    """x (T, N, F) fed in `pieces` frames at a time -> logits (T, N, C).  lens (N) are told to
    the stream with the piece that carries each stream's last frame (ended_at: the index of that
    piece per stream, worked out here when None)."""
    T, N = x.shape[0], x.shape[1]
    assert sum(pieces) == T
    s = Stream(stages, N, step)
    ends = np.cumsum(pieces)
    outs, pos = [], 0
    for i, p in enumerate(pieces):
        ended = None
        if lens is not None:
            ended = [int(lens[n]) if pos < lens[n] <= ends[i] else None for n in range(N)]
        o = s.feed(x[pos:pos + p], ended)
        if o is not None:
            outs.append(o)
        pos += p
    o = s.finish()
    if o is not None:
        outs.append(o)
    return np.concatenate(outs, 0)
