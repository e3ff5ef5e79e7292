"""float64 NumPy restatement of the UNIDIRECTIONAL LSTM (a bare ``layers.LSTM``: K29,
csrc/lstm_uni.hip): ``oracle.lstm.lstm_forward`` / ``lstm_backward`` (plain cell, reverse=False)
restated with an initial state (h0, c0) and the last state returned, the stage list of a model
whose LSTM stages have one direction, and the chunked restatement of a streaming session.  Test
infrastructure only.

The loops follow oracle/lstm.py operation by operation (z = x W + h U + b in that order, one
matmul per frame), so that with a zero state they give its numbers EXACTLY
(tests/test_lstm_uni_host.py).  Everything is gate-major as there: column blocks i, f, c, o of H.
What differs from oracle/lstm.py:
* the state: ``h0`` / ``c0`` (None: zeros) in front of frame 0; BPTT starts from the zero state;
* the hard-sigmoid slopes of BPTT are read from the SAVED gates (0.2 on 0 < gate < 1, else 0), as
  the kernels do, not from the pre-activations -- the same numbers off the two kinks; with
  ``sides`` (another computation's saved gates) the saturation side of every gate entry, and of a
  relu candidate, is read from there (the mechanism of tests/gru_oracle.py);
* a 'bilstm' stage (a model with a Bidirectional(LSTM) beside a bare LSTM) is two runs of the same
  loop, the second over the reversed frames.
"""
import numpy as np

from oracle import ctc as _ctc
from oracle import lstm as OL
from tests import window_oracle as WO

hard_sigmoid = OL.hard_sigmoid


def hs_slope(g):
    return np.where((g > 0.0) & (g < 1.0), 0.2, 0.0)


# ---------------------------------------------------------------- the recurrence
def _run(wx, b, U, act, BU, h0, c0):
    """wx (T, N, 4H) = x @ W per frame; -> hs, cs (T, N, H), gates (T, N, 4H) post-activation."""
    fact = OL.ACTIVATIONS[act][0]
    T, N, _ = wx.shape
    H = U.shape[0]
    h = np.zeros((N, H), wx.dtype) if h0 is None else np.asarray(h0, wx.dtype)
    c = np.zeros((N, H), wx.dtype) if c0 is None else np.asarray(c0, wx.dtype)
    hs, cs = np.zeros((T, N, H), wx.dtype), np.zeros((T, N, H), wx.dtype)
    gates = np.zeros((T, N, 4 * H), wx.dtype)
    for t in range(T):
        hm = h if BU is None else h * BU
        z = wx[t] + hm @ U + b
        i = hard_sigmoid(z[:, :H])
        f = hard_sigmoid(z[:, H:2 * H])
        g = fact(z[:, 2 * H:3 * H])
        o = hard_sigmoid(z[:, 3 * H:])
        c = f * c + i * g
        h = o * fact(c)
        hs[t], cs[t] = h, c
        gates[t] = np.concatenate([i, f, g, o], axis=1)
    return hs, cs, gates


def recurrence_forward(zx, U, act='tanh', BU=None, h0=None, c0=None):
    """zx (T, N, 4H) = x @ W + b, U (H, 4H), state (N, H) each or None -> h, cell, gates; the last
    state is (h[-1], cell[-1])."""
    assert (h0 is None) == (c0 is None)
    return _run(zx, 0.0, U, act, BU, h0, c0)


def lstm_forward(x, W, U, b, BW=None, BU=None, act='tanh', h0=None, c0=None):
    """oracle.lstm.lstm_forward(reverse=False) from a state: -> hs, cache (cache['last'] = the
    state behind the last frame)."""
    assert (h0 is None) == (c0 is None)
    xs = x if BW is None else x * BW[None]
    wx = np.stack([xs[t] @ W for t in range(x.shape[0])])
    hs, cs, gates = _run(wx, b, U, act, BU, h0, c0)
    return hs, dict(x=x, xs=xs, W=W, U=U, BW=BW, BU=BU, hs=hs, cs=cs, gates=gates, act=act,
                    last=(hs[-1], cs[-1]), sides=None)


def _bptt(dhs, U, cs, gates, act, BU, sides, per_frame=None):
    """BPTT from the zero state: -> dzs (T, N, 4H).  per_frame(t, dz) is called frame by frame,
    T - 1 down to 0: the order in which oracle.lstm.lstm_backward accumulates."""
    fact, dact = OL.ACTIVATIONS[act]
    T, N, H = dhs.shape
    src = gates if sides is None else sides
    dzs = np.zeros((T, N, 4 * H), dhs.dtype)
    dh_next = np.zeros((N, H), dhs.dtype)
    dc_next = np.zeros((N, H), dhs.dtype)
    for t in range(T - 1, -1, -1):
        c_prev = cs[t - 1] if t > 0 else np.zeros((N, H), dhs.dtype)
        i, f = gates[t][:, :H], gates[t][:, H:2 * H]
        g, o = gates[t][:, 2 * H:3 * H], gates[t][:, 3 * H:]
        dh = dhs[t] + dh_next
        tc = fact(cs[t])
        dcl = dh * o * dact(tc)
        do = dh * tc
        dc = dc_next + dcl
        di, dg, df = dc * g, dc * i, dc * c_prev
        dc_next = dc * f
        sg = src[t][:, 2 * H:3 * H] if act == 'relu' else g
        dz = np.concatenate([
            di * hs_slope(src[t][:, :H]),
            df * hs_slope(src[t][:, H:2 * H]),
            dg * dact(sg),
            do * hs_slope(src[t][:, 3 * H:])], axis=1)
        dzs[t] = dz
        if per_frame is not None:
            per_frame(t, dz)
        dhm = dz @ U.T
        dh_next = dhm if BU is None else dhm * BU
    return dzs


def recurrence_backward(dy, U, cell, gates, act='tanh', BU=None, sides=None):
    """dy (T, N, H) -> dz (T, N, 4H): what asr_lstm_uni_seq_bwd computes from the saved cell and
    gates."""
    return _bptt(dy, U, cell, gates, act, BU, sides)


def lstm_backward(dhs, cache):
    """oracle.lstm.lstm_backward for the caches of lstm_forward (zero state): dx, dW, dU, db."""
    xs, W, U, BW, BU = cache['xs'], cache['W'], cache['U'], cache['BW'], cache['BU']
    hs = cache['hs']
    T, N, H = hs.shape
    dW, dU, db = np.zeros_like(W), np.zeros_like(U), np.zeros(4 * H, hs.dtype)
    dxs = np.zeros_like(xs)

    def per_frame(t, dz):
        h_prev = hs[t - 1] if t > 0 else np.zeros((N, H), hs.dtype)
        hm = h_prev if BU is None else h_prev * BU
        dW[...] += xs[t].T @ dz
        dU[...] += hm.T @ dz
        db[...] += dz.sum(axis=0)
        dxs[t] = dz @ W.T

    cache['dzs'] = _bptt(dhs, U, cache['cs'], cache['gates'], cache['act'], BU,
                         cache.get('sides'), per_frame)
    dx = dxs if BW is None else dxs * BW[None]
    return dx, dW, dU, db


def side_share(own, other):
    """Share of the i, f, o entries (gate-major slabs) whose saturation side differs."""
    H = own.shape[-1] // 4
    keep = np.r_[0:2 * H, 3 * H:4 * H]
    return float(np.mean(hs_slope(own[..., keep]) != hs_slope(other[..., keep])))


# ---------------------------------------------------------------- models
def stages_from_model(model):
    """The oracle's stage list (float64 weights) of a model of noise (0), dropout, dense, causal
    dwconv (inference chains), bare LSTM ('lstm') and Bidirectional(LSTM) ('bilstm', plain cell)
    stages."""
    it = iter([w.astype(np.float64) for w in model.get_weights()])
    out = []
    for s in model.stages:
        if s.kind in ('noise', 'reshape'):
            out.append(dict(type='pass'))
        elif s.kind == 'dropout':
            out.append(dict(type='dropout', p=s.value))
        elif s.kind == 'dense':
            out.append(dict(type='dense', W=next(it), b=next(it), l2=s.l2))
        elif s.kind == 'dwconv':
            out.append(dict(type='dwconv', W=next(it), b=next(it), pad_left=s.pad_left))
        elif s.kind == 'bilstm' and getattr(s, 'directions', 2) == 1:
            out.append(dict(type='lstm', W=next(it), U=next(it), b=next(it), act=s.act,
                            l2_W=s.l2_W, l2_U=s.l2_U))
        elif s.kind == 'bilstm':
            assert s.mi is None and s.ln is None and not (s.zoneout_c or s.zoneout_h)
            dirs = [dict(W=next(it), U=next(it), b=next(it)) for _ in range(2)]
            out.append(dict(type='bilstm', dirs=dirs, act=s.act, l2_W=s.l2_W, l2_U=s.l2_U))
        else:
            raise NotImplementedError(s.kind)
    return out


def model_forward(stages, x, masks=None, sides=None, lens=None):
    """x (T, N, F) real rows -> logits (T, N, C), caches.  masks: {stage index: (B_W (N, F), B_U
    (N, H))} of an lstm stage, (B_W (2, N, F), B_U (2, N, H)) of a bilstm stage; sides: {stage
    index: saved gates (T, N, 4H)} (bilstm: (T, N, 2, 4H), frames in time order)."""
    masks, sides = masks or {}, sides or {}
    a, caches = x, []
    for i, st in enumerate(stages):
        t, c = st['type'], None
        if t == 'dense':
            c = a
            a = a @ st['W'] + st['b']
        elif t == 'dwconv':
            a, c = WO.dwconv_forward(a, st['W'], st['b'], st['pad_left'], lens)
        elif t == 'lstm':
            BW, BU = masks.get(i, (None, None))
            a, c = lstm_forward(a, st['W'], st['U'], st['b'], BW, BU, st['act'])
            c['sides'] = sides.get(i)
        elif t == 'bilstm':
            BW, BU = masks.get(i, (None, None))
            outs, c = [], []
            for d, p in enumerate(st['dirs']):
                xin = a if d == 0 else a[::-1]
                hs, cd = lstm_forward(xin, p['W'], p['U'], p['b'], None if BW is None else BW[d],
                                      None if BU is None else BU[d], st['act'])
                if sides.get(i) is not None:
                    sd = sides[i][:, :, d]
                    cd['sides'] = sd if d == 0 else sd[::-1]
                outs.append(hs if d == 0 else hs[::-1])
                c.append(cd)
            a = np.concatenate(outs, axis=-1)
        caches.append(c)
    return a, caches


def stage_gates(stages, caches):
    """{stage index: the oracle's own gates in the layout of ``sides``}."""
    out = {}
    for i, (st, c) in enumerate(zip(stages, caches)):
        if st['type'] == 'lstm':
            out[i] = c['gates']
        elif st['type'] == 'bilstm':
            out[i] = np.stack([c[0]['gates'], c[1]['gates'][::-1]], axis=2)
    return out


def model_backward(stages, caches, dlogits):
    """-> gradients in get_weights() order (training chains: dense, lstm, bilstm)."""
    da, out = dlogits, []
    for st, c in zip(reversed(stages), reversed(caches)):
        t = st['type']
        if t == 'dense':
            out = [np.einsum('tnf,tnc->fc', c, da), da.sum(axis=(0, 1))] + out
            da = da @ st['W'].T
        elif t == 'lstm':
            da, dW, dU, db = lstm_backward(da, c)
            out = [dW, dU, db] + out
        elif t == 'bilstm':
            H = st['dirs'][0]['U'].shape[0]
            dx, g = 0.0, []
            for d in range(2):
                dy = np.ascontiguousarray(da[..., d * H:(d + 1) * H])
                dxd, dW, dU, db = lstm_backward(dy if d == 0 else dy[::-1], c[d])
                dx = dx + (dxd if d == 0 else dxd[::-1])
                g += [dW, dU, db]
            da, out = dx, g + out
        elif t == 'dwconv':
            raise NotImplementedError('dwconv in a training chain')
    return out


def loss_and_grads(stages, x, labels, seq_len, masks=None, sides=None):
    """Mean CTC over the batch (no l2) and its gradients: dict(ctc (N,), logits, grads, caches)."""
    logits, caches = model_forward(stages, x, masks, sides)
    N = logits.shape[1]
    ctc_n, dlog = _ctc.ctc_loss_grad(logits, labels, seq_len, dtype=np.float64)
    grads = model_backward(stages, caches, dlog / N)
    return dict(ctc=ctc_n, logits=logits, grads=grads, caches=caches)


def trainable(stages):
    """(holder, key, l2) of every array Adam updates, get_weights() order."""
    out = []
    for st in stages:
        if st['type'] == 'dense':
            out += [(st, 'W', st['l2']), (st, 'b', 0.0)]
        elif st['type'] == 'lstm':
            out += [(st, 'W', st['l2_W']), (st, 'U', st['l2_U']), (st, 'b', 0.0)]
        elif st['type'] == 'bilstm':
            for p in st['dirs']:
                out += [(p, 'W', st['l2_W']), (p, 'U', st['l2_U']), (p, 'b', 0.0)]
    return out


def weights(stages):
    return [holder[k] for holder, k, _ in trainable(stages)]


def train_step(stages, x, labels, seq_len, opt, masks=None, sides=None):
    """One optimisation step of the oracle: gradients + l2, then the optimiser (oracle.optim, in
    place).  Returns the step's loss_and_grads dict."""
    out = loss_and_grads(stages, x, labels, seq_len, masks, sides)
    tr = trainable(stages)
    g = [gi + 2.0 * l2 * holder[k] if l2 else gi
         for gi, (holder, k, l2) in zip(out['grads'], tr)]
    opt.step([holder[k] for holder, k, _ in tr], g)
    return out


# ---------------------------------------------------------------- a session, restated
def model_stream(stages, x, lens, pieces):
    """x (T, N, F) run ``pieces`` frames at a time with explicit state: (h, c) per lstm stage, the
    last k - 1 masked input frames per causal dwconv (as tests/gru_uni_oracle.py) -> logits."""
    assert sum(pieces) == x.shape[0]
    state, outs, t0 = {}, [], 0
    for p in pieces:
        a = x[t0:t0 + p]
        for i, st in enumerate(stages):
            t = st['type']
            if t == 'lstm':
                h0, c0 = state.get(i, (None, None))
                a, c = lstm_forward(a, st['W'], st['U'], st['b'], None, None, st['act'], h0, c0)
                state[i] = c['last']
            elif t == 'dwconv':
                sub = {} if state.get(i) is None else {0: state[i]}
                a = _dwconv_piece(st, a, lens, t0, sub)
                state[i] = sub[0]
            elif t == 'bilstm':
                raise NotImplementedError('a bidirectional stage has no chunked restatement')
            else:
                a, _ = model_forward([st], a)
        outs.append(a)
        t0 += p
    return np.concatenate(outs, 0)


def _dwconv_piece(st, a, lens, t0, state):
    """One piece of a causal depthwise convolution; state[0]: the last k - 1 masked inputs."""
    k, p = st['W'].shape[0], a.shape[0]
    assert st['pad_left'] == k - 1
    tail = state.get(0)
    if tail is None:
        tail = np.zeros((k - 1,) + a.shape[1:])
    m = (t0 + np.arange(p))[:, None] < np.asarray(lens)[None, :]
    xm = np.concatenate([tail, np.where(m[:, :, None], a, 0.0)], 0)
    out = np.zeros(a.shape) + st['b']
    for j in range(k):
        out = out + st['W'][j] * xm[j:j + p]
    state[0] = xm[xm.shape[0] - (k - 1):]
    return out
