"""Thin torch-tensor level wrappers over the C ABI (libasr_hip.so).

torch is used ONLY as a device-memory / stream provider: every function here takes
``tensor.data_ptr()`` and the current HIP stream handle and calls the C ABI through
ctypes.  No torch.nn, no torch math on the hot path.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_f32(*ts):
    for t in ts:
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), \
                'expected contiguous float32 CUDA tensor'


class _Workspaces(object):
    """Caller-owned scratch buffers, grown on demand, one per op family."""

    def __init__(self):
        self.bufs = {}

    def get(self, name, nbytes, device):
        key = (name, str(device))
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            # zero-filled: the recurrent kernels keep a sticky timeout flag in the first
            # bytes of their workspace (asr_lstm_status); a workspace that grows in the
            # middle of a step (a wider layer, a larger batch) inherits the flag
            new = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            if buf is not None:
                new[:256].copy_(buf[:256])
            buf = self.bufs[key] = new
        return buf


WS = _Workspaces()


def pad16(n):
    return (int(n) + 15) // 16 * 16


# --------------------------------------------------------------------------- GEMM
def _resolve_split(split_k, M, N, K, tile=128):
    if split_k == 'auto':
        # long-K / small-output GEMMs (dW, dU): split K until ~1024 workgroups' worth of
        # `tile` x `tile` tiles exist (256 workgroups of the 256 x 256 kernel)
        tiles = ((int(M) + tile - 1) // tile) * ((int(N) + tile - 1) // tile)
        split_k = max(1, min(64, (1024 + tiles - 1) // tiles, int(K) // 256))
    return int(split_k)


def _resolve_split_hl(split_k, M, N, K, tile=0, batch=1):
    """'auto' for asr_gemm_hl: split K until the launch fills the chip ONCE -- a workgroup of the
    256 x 256 kernel has a CU to itself (256 slots), the 128 x 128 kernel runs two per CU.  (A
    launch a little over one round costs two: 312 workgroups of a 640 x 2048 weight gradient.)"""
    slots_cap = 0
    if isinstance(split_k, str) and split_k.startswith('auto:'):
        # 'auto:<CUs>': a launch that shares the chip (the side stream beside a compact BPTT
        # has half of the CUs): one round of THAT many workgroups
        slots_cap = int(split_k[5:])
        split_k = 'auto'
    if split_k != 'auto':
        return int(split_k)
    big = int(tile) != 128 and int(M) >= 256 and int(N) >= 256
    tl, slots = (256, 256) if big else (128, 512)
    if slots_cap:
        slots = slots_cap if big else 2 * slots_cap
    tiles = ((int(M) + tl - 1) // tl) * ((int(N) + tl - 1) // tl) * max(1, int(batch))
    return max(1, min(64, slots // tiles, int(K) // 256))


def gemm(A, B, Cm, M, N, K, trans_a=False, trans_b=False, lda=None, ldb=None, ldc=None,
         alpha=1.0, beta=0.0, bias=None, a_scale=None, a_scale_period=0, c_scale=None,
         c_scale_period=0, split_k=0, a_off=0, b_off=0, c_off=0, ws_name='gemm',
         precision=-1, a_absmax=None, b_absmax=None, a_scale_off=0, a_scale_ld=None):
    """C[M,N] = alpha * opA(A) @ opB(B) + beta*C (+bias), see include/asr_hip.h.

    A/B/Cm are float32 CUDA tensors used as raw storage; *_off are element
    offsets into them (sub-matrix views without torch slicing semantics)."""
    lib = L.load()
    a = L.GemmArgs()
    a.M, a.N, a.K = int(M), int(N), int(K)
    a.trans_a, a.trans_b = int(bool(trans_a)), int(bool(trans_b))
    a.A = A.data_ptr() + 4 * int(a_off)
    a.B = B.data_ptr() + 4 * int(b_off)
    a.C = Cm.data_ptr() + 4 * int(c_off)
    a.lda = int(lda if lda is not None else (M if trans_a else K))
    a.ldb = int(ldb if ldb is not None else (K if trans_b else N))
    a.ldc = int(ldc if ldc is not None else N)
    a.alpha, a.beta = float(alpha), float(beta)
    a.bias = bias.data_ptr() if bias is not None else None
    a.a_scale = a_scale.data_ptr() + 4 * int(a_scale_off) if a_scale is not None else None
    a.a_scale_period = int(a_scale_period)
    a.a_scale_ld = int(a_scale_ld if a_scale_ld is not None else a_scale.shape[-1]) \
        if a_scale is not None else 0
    a.c_scale = c_scale.data_ptr() if c_scale is not None else None
    a.c_scale_period = int(c_scale_period)
    a.c_scale_ld = int(c_scale.shape[-1]) if c_scale is not None else 0
    a.split_k = _resolve_split(split_k, M, N, K)
    a.precision = int(precision)
    a.a_absmax = a_absmax.data_ptr() if a_absmax is not None else None
    a.b_absmax = b_absmax.data_ptr() if b_absmax is not None else None
    nbytes = lib.asr_gemm_workspace_bytes(C.byref(a))
    ws = WS.get(ws_name, nbytes, Cm.device) if nbytes else None
    L.check(lib.asr_gemm(C.byref(a), _ptr(ws), nbytes, _stream()), 'asr_gemm')


_GATE_ROLES = {'fwd': 0, 'dgrad': 1, 'wgrad': 2}


def gate_gemm(role, rows, n_pad, in_dim, gate_dim, W, w_off, ldw, ldz, x=None, x_off=0,
              ldx=None, bias=None, mask_w=None, zx=None, dz=None, z_off=0, dz_absmax=None,
              dx=None, dx_off=0, dx_beta=0.0, dW=None, dw_off=0, db=None, split_k=0,
              precision=-1, ws_name='gemm'):
    """One of the three GEMMs of an LSTM layer's input projection (asr_gemm_gate_fwd /
    _dgrad / _wgrad, include/asr_hip.h): tensors are raw float32 storage, *_off element
    offsets into them (x_off into x, z_off into zx or dz, w_off into W, dw_off into dW)."""
    lib = L.load()
    g = L.GateGemmArgs()
    g.rows, g.n_pad, g.in_dim, g.gate_dim = int(rows), int(n_pad), int(in_dim), int(gate_dim)
    g.x = None if x is None else x.data_ptr() + 4 * int(x_off)
    g.ldx = int(ldx if ldx is not None else in_dim)
    g.W = W.data_ptr() + 4 * int(w_off)
    g.ldw, g.ldz = int(ldw), int(ldz)
    g.bias = None if bias is None else bias.data_ptr()
    g.mask_w = None if mask_w is None else mask_w.data_ptr()
    g.zx = None if zx is None else zx.data_ptr() + 4 * int(z_off)
    g.dz = None if dz is None else dz.data_ptr() + 4 * int(z_off)
    g.dz_absmax = None if dz_absmax is None else dz_absmax.data_ptr()
    g.dx = None if dx is None else dx.data_ptr() + 4 * int(dx_off)
    g.dx_beta = float(dx_beta)
    g.dW = None if dW is None else dW.data_ptr() + 4 * int(dw_off)
    g.db = None if db is None else db.data_ptr()
    g.split_k = _resolve_split(split_k, in_dim, gate_dim, rows)
    g.precision = int(precision)
    kind = _GATE_ROLES[role]
    nbytes = lib.asr_gemm_gate_workspace_bytes(C.byref(g), kind)
    ws = WS.get(ws_name, nbytes, W.device) if nbytes else None
    fn = (lib.asr_gemm_gate_fwd, lib.asr_gemm_gate_dgrad, lib.asr_gemm_gate_wgrad)[kind]
    L.check(fn(C.byref(g), _ptr(ws), nbytes, _stream()), 'asr_gemm_gate_' + role)


def absmax(x, out=None):
    """max |x| of a contiguous float32 CUDA tensor -> 1-element float32 tensor."""
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
    L.check(L.load().asr_absmax(_ptr(x), x.numel(), _ptr(out), _stream()), 'asr_absmax')
    return out


def colsum(X, M, N, ldx, out, beta=0.0, x_off=0, ws_name='colsum'):
    lib = L.load()
    nbytes = lib.asr_colsum_workspace_bytes(int(M), int(N))
    ws = WS.get(ws_name, nbytes, out.device)
    L.check(lib.asr_colsum(C.c_void_p(X.data_ptr() + 4 * int(x_off)), int(M), int(N),
                           int(ldx), _ptr(out), float(beta), _ptr(ws), nbytes, _stream()),
            'asr_colsum')


# --------------------------------------------------------------------------- LSTM
# LDS a recurrent workgroup reserves (asr_lstm_args.lds_reserve_kb; 0 = the library's 96 KB:
# no GEMM workgroup fits beside it).
LSTM_LDS_KB = 0


def cu_masked_stream(device, n_cus, total_cus):
    """A torch stream confined to n_cus of the device's total_cus compute units
    (asr_stream_create_cu_mask).  The mask alternates groups of 8 CUs, which selects the same
    number of CUs on every XCD whether the runtime numbers them XCD-interleaved or XCD-major."""
    words = (int(total_cus) + 31) // 32
    bits = [0] * words
    chosen = 0
    for pass_ in range(2):                      # even groups of 8 first, then odd ones
        for i in range(int(total_cus)):
            if chosen >= n_cus:
                break
            if ((i // 8) % 2 == pass_) and not (bits[i // 32] >> (i % 32)) & 1:
                bits[i // 32] |= 1 << (i % 32)
                chosen += 1
    arr = (C.c_uint32 * words)(*bits)
    out = C.c_void_p()
    L.check(L.load().asr_stream_create_cu_mask(arr, words, C.byref(out)), 'asr_stream_create_cu_mask')
    return torch.cuda.ExternalStream(out.value, device=device)


# asr_lstm_args.activation: the reference LSTM's `activation` hyper-parameter (Keras-1.2.2 names)
ACTIVATION_IDS = {'tanh': 0, 'relu': 1, 'sigmoid': 2, 'hard_sigmoid': 3, 'linear': 4,
                  'softsign': 5, 'softplus': 6}


def activation_id(act):
    if isinstance(act, int):
        return act
    try:
        return ACTIVATION_IDS[act or 'tanh']
    except KeyError:
        raise ValueError('LSTM activation %r: one of %s' % (act, sorted(ACTIVATION_IDS)))


def _lstm_args(T, n_pad, H, U, mask_u=None, zx=None, y=None, cell=None, gates=None,
               dy=None, dz=None, mode=0, dz_absmax=None, steps=None, mi=None, uh=None,
               zone_c=None, zone_h=None, wx=None, dwx=None, dmi=None, db_part=None, act=0):
    a = L.LstmArgs()
    a.activation = activation_id(act)
    a.T, a.n_pad, a.H, a.mode = int(T), int(n_pad), int(H), int(mode)
    a.step_begin, a.step_count = (0, 0) if steps is None else (int(steps[0]), int(steps[1]))
    a.U = U.data_ptr()
    for name, t in (('mask_u', mask_u), ('zx', zx), ('y', y), ('cell', cell),
                    ('gates', gates), ('dy', dy), ('dz', dz), ('dz_absmax', dz_absmax),
                    ('mi', mi), ('uh', uh), ('zone_c', zone_c), ('zone_h', zone_h),
                    ('wx', wx), ('dwx', dwx), ('dmi', dmi), ('db_part', db_part)):
        setattr(a, name, t.data_ptr() if t is not None else None)
    return a


def lstm_seq_fwd(zx, U, y, cell, gates, T, n_pad, H, mask_u=None, mode=0, check=False,
                 steps=None, mi=None, uh=None, zone_c=None, zone_h=None, n_valid=0, act=0,
                 units=0):
    """steps=(begin, count): only that slice of the recurrence (consecutive slices from 0
    on the same stream continue one sequence); None = all T steps."""
    lib = L.load()
    _check_f32(zx, U, y, cell, gates, mask_u)
    a = _lstm_args(T, n_pad, H, U, mask_u, zx=zx, y=y, cell=cell, gates=gates, mode=mode,
                   steps=steps, mi=mi, uh=uh, zone_c=zone_c, zone_h=zone_h, act=act)
    a.n_valid = int(n_valid)            # 1: single-utterance kernel (row 0 only)
    a.fwd_units = int(units)            # 0 = the library decides, 8 / 16 = units per workgroup
    a.lds_reserve_kb = LSTM_LDS_KB
    nbytes = lib.asr_lstm_workspace_bytes(C.byref(a), 0)
    ws = WS.get('lstm_fwd', nbytes, zx.device)
    L.check(lib.asr_lstm_seq_fwd(C.byref(a), _ptr(ws), nbytes, _stream()), 'asr_lstm_seq_fwd')
    if check:
        L.check(lib.asr_lstm_status(_ptr(ws), _stream()), 'asr_lstm_status(fwd)')
    return ws


def lstm_seq_bwd(dy, U, cell, gates, dz, T, n_pad, H, mask_u=None, mode=0, check=False,
                 dz_absmax=None, steps=None, mi=None, uh=None, zone_c=None, zone_h=None,
                 wx=None, dwx=None, dmi=None, db_part=None, compact=False, act=0,
                 dz_planes=None, dz_bound=None):
    """db_part: optional (n_pad/16, 2, 4H) buffer receiving the per-batch-tile sums of dz over
    samples and steps (bias-gradient partials; accumulated across the slices of a sequence).
    compact: H/32 workgroups per chain (half the CUs per layer, asr_lstm_args.compact).
    dz_planes (HlPlanes of (T n_pad, 8H)) + dz_bound (device float): the gate gradients leave
    as packed planes pre-scaled for *dz_bound INSTEAD of the fp32 slab `dz` (may be None then;
    asr_lstm_args.dz_hl, see lstm_dz_hl_supported / lstm_dz_guard)."""
    lib = L.load()
    _check_f32(dy, U, cell, gates, dz, mask_u)
    a = _lstm_args(T, n_pad, H, U, mask_u, cell=cell, gates=gates, dy=dy, dz=dz, mode=mode,
                   dz_absmax=dz_absmax, steps=steps, mi=mi, uh=uh, zone_c=zone_c,
                   zone_h=zone_h, wx=wx, dwx=dwx, dmi=dmi, db_part=db_part, act=act)
    a.lds_reserve_kb = LSTM_LDS_KB
    a.compact = 1 if compact else 0
    if dz_planes is not None:
        assert dz_bound is not None and dz_planes.rows == T * n_pad and dz_planes.ld == 8 * H
        a.dz_hl = dz_planes.hl.data_ptr()
        a.dz_bound = dz_bound.data_ptr()
        a.dz_scale_out = dz_planes.scale.data_ptr()
    nbytes = lib.asr_lstm_workspace_bytes(C.byref(a), 1)
    ws = WS.get('lstm_bwd', nbytes, dy.device)
    L.check(lib.asr_lstm_seq_bwd(C.byref(a), _ptr(ws), nbytes, _stream()), 'asr_lstm_seq_bwd')
    if check:
        L.check(lib.asr_lstm_status(_ptr(ws), _stream()), 'asr_lstm_status(bwd)')
    return ws


# --------------------------------------------------------------------------- SimpleRNN (K14)
# asr_rnn_args.activation: the SimpleRNN / Activation names this build runs
RNN_ACTIVATIONS = {'tanh': 0, 'relu': 1, 'linear': 4,
                   'clipped_relu': L.CONSTANTS['ASR_ACT_CLIPPED_RELU']}
RNN_WS = ('rnn_fwd', 'rnn_bwd')     # workspaces: sticky timeout word in their first bytes


def _rnn_ran(device):
    return (RNN_WS[0], str(device)) in WS.bufs or (RNN_WS[1], str(device)) in WS.bufs


def rnn_activation_id(act):
    """'tanh' / 'relu' / 'linear' / ('clipped_relu', max_value) -> (id, clip)."""
    if isinstance(act, (tuple, list)) and act and act[0] == 'clipped_relu':
        return RNN_ACTIVATIONS['clipped_relu'], float(act[1])
    try:
        return RNN_ACTIVATIONS[act or 'tanh'], 0.0
    except (KeyError, TypeError):
        raise NotImplementedError('activation %r (implemented: tanh, relu, linear, clipped_relu)'
                                  % (act,))


def _rec_args(a, T, n_pad, H, mode, U=None, act=None, mask_u=None, **fields):
    """The fields the args blocks of the recurrent layers share (asr_rnn_args, asr_gru_args,
    asr_rhn_args); `fields`: tensors (or None) stored as pointers.  A plan query gives no U."""
    a.T, a.n_pad, a.H, a.mode = int(T), int(n_pad), int(H), int(mode)
    if U is not None:
        a.activation, a.clip = rnn_activation_id(act)
        fields.update(U=U, mask_u=mask_u)
    for name, t in fields.items():
        setattr(a, name, t.data_ptr() if t is not None else None)
    return a


def _rec_dy(a, H, shared_dy):
    a.dy_ld, a.dy_dir_stride = (int(H), 0) if shared_dy else (2 * int(H), int(H))


def _rec_run(kind, a, backward, ws_name, device, check=False):
    """asr_<kind>_seq_fwd / _bwd on a workspace of the size the library asks for; returns it."""
    lib = L.load()
    fn = 'asr_%s_seq_%s' % (kind, 'bwd' if backward else 'fwd')
    nbytes = getattr(lib, 'asr_%s_workspace_bytes' % kind)(C.byref(a), int(backward))
    if nbytes == 0:
        L.check(-1, 'asr_%s_workspace_bytes' % kind)
    ws = WS.get(ws_name, nbytes, device)
    L.check(getattr(lib, fn)(C.byref(a), _ptr(ws), nbytes, _stream()), fn)
    if check:
        L.check(lib.asr_lstm_status(_ptr(ws), _stream()),
                'asr_%s status (%s)' % (kind, 'bwd' if backward else 'fwd'))
    return ws


def _rec_plan(kind, a, backward):
    per, rows, units, blocks = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    fn = 'asr_%s_plan' % kind
    L.check(getattr(L.load(), fn)(C.byref(a), int(bool(backward)), C.byref(per), C.byref(rows),
                                  C.byref(units), C.byref(blocks)), fn)
    return {'persistent': bool(per.value), 'rows': rows.value, 'units': units.value,
            'blocks': blocks.value}


def rnn_seq_fwd(zx, U, h, T, n_pad, H, act='tanh', mask_u=None, y_sum=None, mode=0, check=False):
    """Both directions of a SimpleRNN layer: h (T, n_pad, 2, H) from zx = x@W + b (same shape),
    U (2, H, H), optional B_U (2, n_pad, H); y_sum (T, n_pad, H) <- h_f + h_b when given.
    mode: 0 = the library's form, 1 = stepwise, 2 = persistent."""
    _check_f32(zx, U, h, mask_u, y_sum)
    a = _rec_args(L.RnnArgs(), T, n_pad, H, mode, U, act, mask_u, zx=zx, h=h, y_sum=y_sum)
    return _rec_run('rnn', a, False, RNN_WS[0], zx.device, check)


def rnn_seq_bwd(dy, U, h, dz, T, n_pad, H, act='tanh', mask_u=None, shared_dy=False, mode=0,
                db_part=None, dz_absmax=None, check=False):
    """BPTT of both directions: dz (T, n_pad, 2, H) = d loss / d pre-activation.  dy is the
    gradient of the layer output: (T, n_pad, 2H) for 'concat', (T, n_pad, H) shared by both
    directions for 'sum' (shared_dy).  db_part (n_pad/16, 2, H): per-batch-tile sums of dz;
    dz_absmax (1,): max |dz|."""
    _check_f32(dy, U, h, dz, mask_u, db_part, dz_absmax)
    a = _rec_args(L.RnnArgs(), T, n_pad, H, mode, U, act, mask_u, h=h, dy=dy, dz=dz,
                  db_part=db_part, dz_absmax=dz_absmax)
    _rec_dy(a, H, shared_dy)
    return _rec_run('rnn', a, True, RNN_WS[1], dy.device, check)


def rnn_plan(T, n_pad, H, backward=False, mode=0):
    """{'persistent': bool, 'rows': batch rows, 'units': units per workgroup, 'blocks':
    workgroups per launch} of the form the library would run (asr_rnn_plan)."""
    return _rec_plan('rnn', _rec_args(L.RnnArgs(), T, n_pad, H, mode), backward)


def activation_fwd(x, y, act):
    """y = act(x), element-wise (the Activation layer)."""
    _check_f32(x, y)
    if act == 'swish':
        return swish_fwd(x, y)
    aid, clip = rnn_activation_id(act)
    L.check(L.load().asr_activation_fwd(_ptr(x), _ptr(y), x.numel(), aid, clip, _stream()),
            'asr_activation_fwd')
    return y


def activation_bwd(dy, y, dx, act, x=None):
    """dx = dy (.) act'(y), the derivative read from the output; 'swish' reads it from the input
    x instead (its derivative is not a function of y)."""
    _check_f32(dy, y, dx)
    if act == 'swish':
        return swish_bwd(x, dy, dx)
    aid, clip = rnn_activation_id(act)
    L.check(L.load().asr_activation_bwd(_ptr(dy), _ptr(y), _ptr(dx), dy.numel(), aid, clip,
                                        _stream()), 'asr_activation_bwd')
    return dx


# --------------------------------------------------------------------------- GRU (K16)
GRU_WS = ('gru_fwd', 'gru_bwd')     # scratch only: the stepwise form has no status words


def gru_seq_fwd(zx, U, h, gates, rm, T, n_pad, H, act='tanh', mask_u=None, y_sum=None, mode=0):
    """Both directions of a GRU layer: h (T, n_pad, 2, H), gates (T, n_pad, 2, 3H) = z | r | hh and
    rm (T, n_pad, 2, H) = r (.) h_prev (.) B_U from zx = x@W + b (T, n_pad, 2, 3H), U (2, H, 3H),
    optional B_U (2, n_pad, H); y_sum (T, n_pad, H) <- h_f + h_b when given.
    mode: 0 = the library's form, 1 = stepwise (the only form there is)."""
    _check_f32(zx, U, h, gates, rm, mask_u, y_sum)
    a = _rec_args(L.GruArgs(), T, n_pad, H, mode, U, act, mask_u, h=h, gates=gates, zx=zx, rm=rm,
                  y_sum=y_sum)
    return _rec_run('gru', a, False, GRU_WS[0], zx.device)


def gru_seq_bwd(dy, U, h, gates, da, T, n_pad, H, act='tanh', mask_u=None, shared_dy=False,
                mode=0, db_part=None, dz_absmax=None):
    """BPTT of both directions: da (T, n_pad, 2, 3H) = da_z | da_r | da_h, the gradient of the
    gate pre-activations.  dy is the gradient of the layer output: (T, n_pad, 2H) for 'concat',
    (T, n_pad, H) shared by both directions for 'sum' (shared_dy).  db_part (n_pad/16, 2, 3H):
    per-batch-tile sums of da; dz_absmax (1,): max |da|."""
    _check_f32(dy, U, h, gates, da, mask_u, db_part, dz_absmax)
    a = _rec_args(L.GruArgs(), T, n_pad, H, mode, U, act, mask_u, h=h, gates=gates, dy=dy, da=da,
                  db_part=db_part, dz_absmax=dz_absmax)
    _rec_dy(a, H, shared_dy)
    return _rec_run('gru', a, True, GRU_WS[1], dy.device)


def gru_plan(T, n_pad, H, backward=False, mode=0):
    """{'persistent': False, 'rows': batch rows, 'units': output columns per workgroup, 'blocks':
    workgroups of the widest launch of a step} (asr_gru_plan)."""
    return _rec_plan('gru', _rec_args(L.GruArgs(), T, n_pad, H, mode), backward)


# --------------------------------------------------------------------------- unidirectional GRU (K28)
GRU_UNI_WS = ('gru_uni_fwd', 'gru_uni_bwd')     # scratch only, as GRU_WS


def gru_uni_seq_fwd(zx, U, h, gates, rm, T, n_pad, H, act='tanh', mask_u=None, h0=None,
                    h_last=None, mode=0):
    """One direction, frames 0 .. T-1: h (T, n_pad, H), gates (T, n_pad, 3H) = z | r | hh and
    rm (T, n_pad, H) from zx (T, n_pad, 3H), U (H, 3H), optional B_U (n_pad, H).  h0 (n_pad, H):
    the state before frame 0 (None: zeros); h_last (n_pad, H) <- h[T-1] when given, never the
    same buffer as h0.  With h0 = None the outputs are direction 0 of gru_seq_fwd bit for bit."""
    _check_f32(zx, U, h, gates, rm, mask_u, h0, h_last)
    a = _rec_args(L.GruUniArgs(), T, n_pad, H, mode, U, act, mask_u, h=h, gates=gates, zx=zx,
                  rm=rm, h0=h0, h_last=h_last)
    return _rec_run('gru_uni', a, False, GRU_UNI_WS[0], zx.device)


def gru_uni_seq_bwd(dy, U, h, gates, da, T, n_pad, H, act='tanh', mask_u=None, dy_ld=None,
                    mode=0, db_part=None, dz_absmax=None):
    """BPTT from the zero state: da (T, n_pad, 3H) = da_z | da_r | da_h.  dy: the gradient of the
    layer output, rows dy_ld floats apart (default H).  db_part (n_pad/16, 3H): per-batch-tile
    sums of da; dz_absmax (1,): max |da|."""
    _check_f32(dy, U, h, gates, da, mask_u, db_part, dz_absmax)
    a = _rec_args(L.GruUniArgs(), T, n_pad, H, mode, U, act, mask_u, h=h, gates=gates, dy=dy,
                  da=da, db_part=db_part, dz_absmax=dz_absmax)
    a.dy_ld = int(H if dy_ld is None else dy_ld)
    return _rec_run('gru_uni', a, True, GRU_UNI_WS[1], dy.device)


def gru_uni_plan(T, n_pad, H, backward=False, mode=0):
    """As gru_plan, for one direction: the same rows and units, half the workgroups
    (asr_gru_uni_plan)."""
    return _rec_plan('gru_uni', _rec_args(L.GruUniArgs(), T, n_pad, H, mode), backward)


# --------------------------------------------------------------------------- unidirectional LSTM (K29)
LSTM_UNI_WS = ('lstm_uni_fwd', 'lstm_uni_bwd')     # scratch only: no status words


def _lstm_uni_args(T, n_pad, H, mode, act=None, **fields):
    a = L.LstmUniArgs()
    a.T, a.n_pad, a.H, a.mode = int(T), int(n_pad), int(H), int(mode)
    a.activation = activation_id(act)
    for name, t in fields.items():
        setattr(a, name, t.data_ptr() if t is not None else None)
    return a


def lstm_uni_seq_fwd(zx, U, h, cell, gates, T, n_pad, H, act='tanh', mask_u=None, h0=None,
                     c0=None, h_last=None, c_last=None, mode=0):
    """One direction, frames 0 .. T-1: h, cell (T, n_pad, H) and gates (T, n_pad, 4H) = the
    post-activation i, f, g, o of every unit, from zx (T, n_pad, 4H), U (H, 4H) (both
    [unit * 4 + gate]), optional B_U (n_pad, H).  (h0, c0) (n_pad, H): the state before frame 0
    (None: zeros); (h_last, c_last) <- (h[T-1], cell[T-1]) when given, never the buffers of
    (h0, c0).  act: a name of ACTIVATION_IDS."""
    _check_f32(zx, U, h, cell, gates, mask_u, h0, c0, h_last, c_last)
    a = _lstm_uni_args(T, n_pad, H, mode, act, U=U, mask_u=mask_u, zx=zx, h=h, cell=cell,
                       gates=gates, h0=h0, c0=c0, h_last=h_last, c_last=c_last)
    return _rec_run('lstm_uni', a, False, LSTM_UNI_WS[0], zx.device)


def lstm_uni_seq_bwd(dy, U, h, cell, gates, dz, T, n_pad, H, act='tanh', mask_u=None, dy_ld=None,
                     mode=0, db_part=None, dz_absmax=None):
    """BPTT from the zero state: dz (T, n_pad, 4H), the gradient of the gate pre-activations.
    dy: the gradient of the layer output, rows dy_ld floats apart (default H).  db_part
    (n_pad/16, 4H): per-batch-tile sums of dz; dz_absmax (1,): max |dz|."""
    _check_f32(dy, U, h, cell, gates, dz, mask_u, db_part, dz_absmax)
    a = _lstm_uni_args(T, n_pad, H, mode, act, U=U, mask_u=mask_u, h=h, cell=cell, gates=gates,
                       dy=dy, dz=dz, db_part=db_part, dz_absmax=dz_absmax)
    a.dy_ld = int(H if dy_ld is None else dy_ld)
    return _rec_run('lstm_uni', a, True, LSTM_UNI_WS[1], dy.device)


def lstm_uni_plan(T, n_pad, H, backward=False, mode=0):
    """{'persistent': False, 'rows', 'units', 'blocks'}: the launch geometry of a frame
    (asr_lstm_uni_plan)."""
    return _rec_plan('lstm_uni', _lstm_uni_args(T, n_pad, H, mode), backward)


# --------------------------------------------------------------------------- RHN (K17)
RHN_WS = ('rhn_fwd', 'rhn_bwd')     # scratch only: the stepwise form has no status words


def _rhn_args(T, n_pad, H, depth, coupling, mode, *rest, **fields):
    a = L.RhnArgs()
    a.depth, a.coupling = int(depth), int(bool(coupling))
    return _rec_args(a, T, n_pad, H, mode, *rest, **fields)


def rhn_seq_fwd(zx, U, b, h, gates, T, n_pad, H, depth, coupling=True, act='tanh', mask_u=None,
                y_sum=None, mode=0):
    """Both directions of an RHN layer (C = 2 column blocks h | t when coupling, else 3 with c):
    states h (L, T, n_pad, 2, H) of every level (slab L-1 is the layer output) and gates
    (L, T, n_pad, 2, C H) = hh | tg | [cg] from zx = x@W (T, n_pad, 2, C H, no bias),
    U (2, L, H, C H), b (2, L, C H), optional B_U (2, L, n_pad, H); y_sum (T, n_pad, H) <- the sum
    of the two directions' outputs when given.
    mode: 0 = the library's form, 1 = stepwise (the only form there is)."""
    _check_f32(zx, U, b, h, gates, mask_u, y_sum)
    a = _rhn_args(T, n_pad, H, depth, coupling, mode, U, act, mask_u, h=h, gates=gates, zx=zx,
                  b=b, y_sum=y_sum)
    return _rec_run('rhn', a, False, RHN_WS[0], zx.device)


def rhn_seq_bwd(dy, U, h, gates, da, T, n_pad, H, depth, coupling=True, act='tanh', mask_u=None,
                shared_dy=False, mode=0, db_part=None, dz_absmax=None):
    """BPTT of both directions: da (L, T, n_pad, 2, C H) = da_h | da_t | [da_c], the gradient of
    every level's pre-activations.  dy is the gradient of the layer output: (T, n_pad, 2H) for
    'concat', (T, n_pad, H) shared by both directions for 'sum' (shared_dy).  db_part
    (n_pad/16, 2, L, C H): per-batch-tile sums of da; dz_absmax (1,): max |da|."""
    _check_f32(dy, U, h, gates, da, mask_u, db_part, dz_absmax)
    a = _rhn_args(T, n_pad, H, depth, coupling, mode, U, act, mask_u, h=h, gates=gates, dy=dy,
                  da=da, db_part=db_part, dz_absmax=dz_absmax)
    _rec_dy(a, H, shared_dy)
    return _rec_run('rhn', a, True, RHN_WS[1], dy.device)


def rhn_plan(T, n_pad, H, depth=1, coupling=True, backward=False, mode=0):
    """{'persistent': False, 'rows': batch rows, 'units': state columns per workgroup, 'blocks':
    workgroups of a launch} (asr_rhn_plan)."""
    return _rec_plan('rhn', _rhn_args(T, n_pad, H, depth, coupling, mode), backward)


# --------------------------------------------------------------------------- BatchNormalization
def bn_stats_len(C):
    """Floats of a stage's stats block: [mean_hi | mean_lo | invstd | var] (C each)."""
    return 4 * int(C)


def bn_moments_len(C):
    """Floats of a stage's moments block for the running update: [w, 0, 0, 0 | w d | w (var +
    d^2)] (asr_bn_fwd_train)."""
    return 4 + 2 * int(C)


def _bn_ws(T, N, n_pad, ld, W, C, device):
    nbytes = L.load().asr_bn_workspace_bytes(int(T), int(N), int(n_pad), int(ld), int(W), int(C))
    if nbytes == 0:
        L.check(-1, 'asr_bn_workspace_bytes (T %d N %d n_pad %d ld %d W %d C %d)'
                % (T, N, n_pad, ld, W, C))
    return WS.get('bn', nbytes, device), nbytes


def bn_fwd_train(x, y, gamma, beta, stats, N, W, C, eps=1e-3, clip=0.0, moments=None,
                 shift=None, weight=0.0):
    """Training-phase BatchNormalization of x (T, n_pad, ld): y (same shape), stats (4C) from
    the batch moments of the N real rows of every frame; moments (4 + 2C, optional) for
    bn_update_running with weight w and shift (None: the batch mean)."""
    _check_f32(x, y, gamma, beta, stats, moments, shift)
    T, n_pad, ld = x.shape
    ws, nbytes = _bn_ws(T, N, n_pad, ld, W, C, x.device)
    L.check(L.load().asr_bn_fwd_train(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(stats),
                                      _ptr(moments), _ptr(shift), float(weight), int(T), int(N),
                                      int(n_pad), int(ld), int(W), int(C), float(eps), float(clip),
                                      _ptr(ws), nbytes, _stream()), 'asr_bn_fwd_train')
    return y


def bn_fwd_infer(x, y, gamma, beta, running_mean, running_var, N, W, C, eps=1e-3, clip=0.0):
    """Inference-phase BatchNormalization on the running moments (one pass)."""
    _check_f32(x, y, gamma, beta, running_mean, running_var)
    T, n_pad, ld = x.shape
    L.check(L.load().asr_bn_fwd_infer(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta),
                                      _ptr(running_mean), _ptr(running_var), int(T), int(N),
                                      int(n_pad), int(ld), int(W), int(C), float(eps), float(clip),
                                      _stream()), 'asr_bn_fwd_infer')
    return y


def bn_bwd(x, dy, gamma, beta, stats, dx, dgamma, dbeta, N, W, C, clip=0.0):
    """dgamma, dbeta (C, written) and dx (same shape as x, or None) from the saved stats."""
    _check_f32(x, dy, gamma, beta, stats, dx, dgamma, dbeta)
    T, n_pad, ld = x.shape
    ws, nbytes = _bn_ws(T, N, n_pad, ld, W, C, x.device)
    L.check(L.load().asr_bn_bwd(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(beta), _ptr(stats),
                                _ptr(dx), _ptr(dgamma), _ptr(dbeta), int(T), int(N), int(n_pad),
                                int(ld), int(W), int(C), float(clip), _ptr(ws), nbytes, _stream()),
            'asr_bn_bwd')
    return dx


def bn_flag_words(device, flags=None):
    """The four flag words the running update's guard reads, as raw device pointers: the
    all-reduced flag slots (data parallel, ``flags`` = Model.veto_flags()) or this process'
    sticky timeout words -- the same words ops.optim_guard reads."""
    if flags is not None:
        base = flags.data_ptr()
        return [C.c_void_p(base + 4 * k) if k < flags.numel() else None for k in range(4)]
    out = [_ptr(WS.get('lstm_fwd', 0, device)), _ptr(WS.get('lstm_bwd', 0, device))]
    out += [_ptr(WS.get(name, 0, device)) for name in RNN_WS] if _rnn_ran(device) else [None,
                                                                                         None]
    return out


def bn_update_running(running_mean, running_var, moments, C, momentum, shift=None, flags=None):
    """EMA of the running moments from a moments block (skipped on the device when a flag word
    is set: bn_flag_words)."""
    _check_f32(running_mean, running_var, moments, shift)
    fw = bn_flag_words(running_mean.device, flags)
    L.check(L.load().asr_bn_update_running(_ptr(running_mean), _ptr(running_var), _ptr(moments),
                                           _ptr(shift), int(C), float(momentum), *fw, _stream()),
            'asr_bn_update_running')


# --------------------------------------------------------------------------- LayerNormalization (K20)
LN_MAX_WIDTH = 4096       # widest slab row (physical columns) of asr_ln_* (asr_ln_max_width())


def ln_stats_len(T, n_pad):
    """Floats of a stage's stats block: (mu, 1 / sqrt(var + eps)) per slab row."""
    return 2 * int(T) * int(n_pad)


def ln_fwd(x, y, gain, bias, N, H, Hp, segs=1, eps=1e-5, stats=None):
    """LayerNormalization of x (T, n_pad, ld) over the real columns of each row (segs blocks of H
    at a stride of Hp) for the N real rows of every frame; stats (ln_stats_len) kept for ln_bwd
    when given.  The same call serves training and inference."""
    _check_f32(x, y, gain, bias, stats)
    T, n_pad, ld = x.shape
    L.check(L.load().asr_ln_fwd(_ptr(x), _ptr(y), _ptr(gain), _ptr(bias), _ptr(stats), int(T),
                                int(N), int(n_pad), int(ld), int(H), int(Hp), int(segs),
                                float(eps), _stream()), 'asr_ln_fwd')
    return y


def ln_bwd(x, dy, gain, stats, dx, dgain, dbias, N, H, Hp, segs=1):
    """dgain, dbias (ld, written) and dx (same shape as x, or None) from the saved stats."""
    _check_f32(x, dy, gain, stats, dx, dgain, dbias)
    T, n_pad, ld = x.shape
    geo = (int(T), int(N), int(n_pad), int(ld), int(H), int(Hp), int(segs))
    nbytes = L.load().asr_ln_workspace_bytes(*geo)
    if nbytes == 0:
        L.check(-1, 'asr_ln_workspace_bytes (T %d N %d n_pad %d ld %d H %d Hp %d segs %d)' % geo)
    ws = WS.get('ln', nbytes, x.device)
    L.check(L.load().asr_ln_bwd(_ptr(x), _ptr(dy), _ptr(gain), _ptr(stats), _ptr(dx),
                                _ptr(dgain), _ptr(dbias), *geo, _ptr(ws), nbytes, _stream()),
            'asr_ln_bwd')
    return dx


# --------------------------------------------------------------------------- self-attention (K21)
def _attn_args(qkv, N, heads, dh, ld_out, scale=None, lens=None, out=None, lse=None, dout=None,
               dqkv=None):
    T, n_pad, ld = qkv.shape
    a = L.AttnArgs()
    a.T, a.N, a.n_pad, a.heads, a.dh = int(T), int(N), int(n_pad), int(heads), int(dh)
    a.ld, a.ld_out = int(ld), int(ld_out)
    a.scale = float(scale if scale is not None else 1.0 / math.sqrt(dh))
    for k, t in (('qkv', qkv), ('lens', lens), ('out', out), ('lse', lse), ('dout', dout),
                 ('dqkv', dqkv)):
        setattr(a, k, None if t is None else t.data_ptr())
    return a


def attn_lse_len(T, n_pad, heads):
    """Floats of the row log-sum-exp block attn_fwd keeps for attn_bwd: (T, n_pad, heads)."""
    return int(T) * int(n_pad) * int(heads)


def attn_plan(T, n_pad, heads, dh, backward=False):
    """{'bq', 'bk': query / key tile lengths, 'blocks': workgroups of a launch, 'lds': bytes of LDS
    per workgroup} of the geometry (asr_attn_plan)."""
    a = L.AttnArgs()
    a.T, a.N, a.n_pad, a.heads, a.dh = int(T), 1, int(n_pad), int(heads), int(dh)
    a.ld, a.ld_out, a.scale = 3 * int(heads) * int(dh), int(heads) * int(dh), 1.0
    v = [C.c_int(0) for _ in range(4)]
    L.check(L.load().asr_attn_plan(C.byref(a), int(bool(backward)), *[C.byref(x) for x in v]),
            'asr_attn_plan')
    return dict(zip(('bq', 'bk', 'blocks', 'lds'), (x.value for x in v)))


def attn_window(window):
    """The asr_attn_window of a (chunk, left, right) triple (K25, csrc/attn_tile.h): for query
    frame t, c0 = (t // chunk) * chunk, key u is visible iff lo(t) <= u < hi(t) and u < lens[n],
    hi(t) = c0 + chunk + right, lo(t) = 0 if left < 0 else max(0, c0 - left).  The library checks
    the values (chunk >= 1, left >= -1, right >= 0)."""
    chunk, left, right = window
    return L.AttnWindow(int(chunk), int(left), int(right))


def attn_win_plan(T, n_pad, heads, dh, window, backward=False):
    """attn_plan under a window, plus 'tile_pairs': the (query tile, key tile) pairs one (sample,
    head) of the forward launch visits without lens (asr_attn_win_plan)."""
    a = L.AttnArgs()
    a.T, a.N, a.n_pad, a.heads, a.dh = int(T), 1, int(n_pad), int(heads), int(dh)
    a.ld, a.ld_out, a.scale = 3 * int(heads) * int(dh), int(heads) * int(dh), 1.0
    v = [C.c_int(0) for _ in range(4)]
    pairs = C.c_longlong(0)
    w = attn_window(window)
    L.check(L.load().asr_attn_win_plan(C.byref(a), C.byref(w), int(bool(backward)),
                                       *[C.byref(x) for x in v], C.byref(pairs)),
            'asr_attn_win_plan')
    return dict(zip(('bq', 'bk', 'blocks', 'lds'), (x.value for x in v)), tile_pairs=pairs.value)


def attn_fwd(qkv, out, N, heads, dh, lens=None, lse=None, scale=None, window=None):
    """out (T, n_pad, ld_out >= heads dh) = softmax(scale Q K^T) V per real sample and head of the
    slab qkv (T, n_pad, ld >= 3 heads dh) = [Q | K | V]; keys u >= lens[n] (device int32,
    1 <= lens <= T) carry probability 0; lse (attn_lse_len) kept for attn_bwd when given.
    window: None, or (chunk, left, right) of attn_window (asr_attn_win_fwd): keys outside a
    query's window carry probability 0 too, a row with no visible key has out = lse = 0."""
    _check_f32(qkv, out, lse)
    _check_lens(lens, N)
    assert qkv.dim() == 3 and out.dim() == 3 and out.shape[:2] == qkv.shape[:2]
    a = _attn_args(qkv, N, heads, dh, out.shape[2], scale, lens, out, lse)
    if window is None:
        L.check(L.load().asr_attn_fwd(C.byref(a), _stream()), 'asr_attn_fwd')
    else:
        w = attn_window(window)
        L.check(L.load().asr_attn_win_fwd(C.byref(a), C.byref(w), _stream()), 'asr_attn_win_fwd')
    return out


def attn_bwd(qkv, out, lse, dout, dqkv, N, heads, dh, lens=None, scale=None, window=None):
    """dqkv (like qkv) = dQ | dK | dV from dout (like out), recomputing p from lse (window: that
    of the forward call)."""
    _check_f32(qkv, out, lse, dout, dqkv)
    _check_lens(lens, N)
    assert dqkv.shape == qkv.shape and dout.shape == out.shape
    a = _attn_args(qkv, N, heads, dh, out.shape[2], scale, lens, out, lse, dout, dqkv)
    nbytes = L.load().asr_attn_workspace_bytes(C.byref(a))
    if nbytes == 0:
        L.check(-1, 'asr_attn_workspace_bytes (T %d N %d n_pad %d heads %d dh %d ld %d ld_out %d)'
                % (a.T, a.N, a.n_pad, a.heads, a.dh, a.ld, a.ld_out))
    ws = WS.get('attn', nbytes, qkv.device)
    if window is None:
        L.check(L.load().asr_attn_bwd(C.byref(a), _ptr(ws), nbytes, _stream()), 'asr_attn_bwd')
    else:
        w = attn_window(window)
        L.check(L.load().asr_attn_win_bwd(C.byref(a), C.byref(w), _ptr(ws), nbytes, _stream()),
                'asr_attn_win_bwd')
    return dqkv


def posenc_table(T, D):
    """The (T, D) sinusoidal table in float64 (host): pe[t, 2i] = sin(t / 10000^(2i / D)),
    pe[t, 2i + 1] = cos(t / 10000^(2i / D))."""
    t = np.arange(int(T), dtype=np.float64)[:, None]
    i2 = (np.arange(int(D)) // 2 * 2).astype(np.float64)[None, :]
    ang = t / np.power(10000.0, i2 / float(D))
    return np.where(np.arange(int(D))[None, :] % 2 == 0, np.sin(ang), np.cos(ang))


_PE = {}


def posenc_get(T, D, device):
    """The table rounded to fp32 on the device, computed and uploaded once per (T, D)."""
    key = (int(T), int(D), str(device))
    pe = _PE.get(key)
    if pe is None:
        if len(_PE) >= 64:
            _PE.clear()
        pe = _PE[key] = torch.from_numpy(posenc_table(T, D).astype(np.float32)).to(device)
    return pe


def posenc_add(x, y, N, D, pe=None):
    """y[t, n, f] = x[t, n, f] + pe[t, f] for n < N, f < D of the slab x (T, n_pad, ld); zeros in
    the pad rows and columns."""
    _check_f32(x, y, pe)
    T, n_pad, ld = x.shape
    if pe is None:
        pe = posenc_get(T, D, x.device)
    assert tuple(pe.shape) == (T, D) and y.shape == x.shape
    L.check(L.load().asr_posenc_add(_ptr(x), _ptr(pe), _ptr(y), int(T), int(N), int(n_pad),
                                    int(D), int(ld), _stream()), 'asr_posenc_add')
    return y


# --------------------------------------------------------------------------- relative attention (K24)
RELATTN_MAX_HEAD_DIM = 64     # of asr_relattn_*: the band tiles leave no LDS for dh 80 .. 128


def relpos_table(T, D):
    """The (2T - 1, D) relative sinusoidal table in float64 (host): row r + T - 1 holds
    pe[r, 2i] = sin(r / 10000^(2i / D)), pe[r, 2i + 1] = cos(r / 10000^(2i / D)) for the relative
    index r = -(T - 1) .. T - 1 (query frame minus key frame)."""
    r = np.arange(-(int(T) - 1), int(T), dtype=np.float64)[:, None]
    i2 = (np.arange(int(D)) // 2 * 2).astype(np.float64)[None, :]
    ang = r * np.power(10000.0, -i2 / float(D))
    return np.where(np.arange(int(D))[None, :] % 2 == 0, np.sin(ang), np.cos(ang))


def relpos_grad_table(T, D):
    """The fp32 table with 1 taken off its cosine columns (float32): what dW_pos = pe^T dpos is
    computed with.  The rows of dS sum to zero, so sum_r dpos_r = 0 and a constant column of pe has
    no gradient: (pe - 1)^T dpos is the same matrix, without the cancellation that would leave
    rounding noise in the rows of the slow cosines (true size ~ (r / 10000)^2 of the others),
    which Adam would normalise into steps of +-lr.  The 1 comes off the ROUNDED cosines, the ones
    the forward pass multiplies with (an exact fp32 difference for cos x >= 1 / 2, the slow
    columns), not off the float64 ones: where cos x - 1 is below 1e-7, the rounding of cos x is
    most of what the forward pass sees of it."""
    pe = relpos_table(T, D).astype(np.float32)
    pe[:, 1::2] -= np.float32(1.0)
    return pe


_RPE = {}


def relpos_get(T, D, device, grad=False):
    """The table (grad: relpos_grad_table) rounded once to fp32 on the device, computed and
    uploaded once per (T, D)."""
    key = (int(T), int(D), str(device), bool(grad))
    pe = _RPE.get(key)
    if pe is None:
        if len(_RPE) >= 64:
            _RPE.clear()
        table = (relpos_grad_table if grad else relpos_table)(T, D)
        pe = _RPE[key] = torch.from_numpy(table.astype(np.float32)).to(device)
    return pe


def _relattn_args(qkv, N, heads, dh, ld_out, ld_pos, scale=None, **tensors):
    T, n_pad, ld = qkv.shape
    a = L.RelAttnArgs()
    a.T, a.N, a.n_pad, a.heads, a.dh = int(T), int(N), int(n_pad), int(heads), int(dh)
    a.ld, a.ld_out, a.ld_pos = int(ld), int(ld_out), int(ld_pos)
    a.scale = float(scale if scale is not None else 1.0 / math.sqrt(dh))
    a.qkv = qkv.data_ptr()
    for k, t in tensors.items():
        setattr(a, k, None if t is None else t.data_ptr())
    return a


def relattn_plan(T, n_pad, heads, dh, backward=False):
    """{'bq', 'bk': query / key tile lengths, 'blocks': workgroups of a launch, 'lds': bytes of LDS
    per workgroup (backward: of the largest pass)} of the geometry (asr_relattn_plan)."""
    a = L.RelAttnArgs()
    a.T, a.N, a.n_pad, a.heads, a.dh = int(T), 1, int(n_pad), int(heads), int(dh)
    a.ld, a.ld_out, a.scale = 3 * int(heads) * int(dh), int(heads) * int(dh), 1.0
    a.ld_pos = a.ld_out
    v = [C.c_int(0) for _ in range(4)]
    L.check(L.load().asr_relattn_plan(C.byref(a), int(bool(backward)), *[C.byref(x) for x in v]),
            'asr_relattn_plan')
    return dict(zip(('bq', 'bk', 'blocks', 'lds'), (x.value for x in v)))


def relattn_win_plan(T, n_pad, heads, dh, window, backward=False):
    """relattn_plan under a window, plus 'tile_pairs' as attn_win_plan (asr_relattn_win_plan)."""
    a = L.RelAttnArgs()
    a.T, a.N, a.n_pad, a.heads, a.dh = int(T), 1, int(n_pad), int(heads), int(dh)
    a.ld, a.ld_out, a.scale = 3 * int(heads) * int(dh), int(heads) * int(dh), 1.0
    a.ld_pos = a.ld_out
    v = [C.c_int(0) for _ in range(4)]
    pairs = C.c_longlong(0)
    w = attn_window(window)
    L.check(L.load().asr_relattn_win_plan(C.byref(a), C.byref(w), int(bool(backward)),
                                          *[C.byref(x) for x in v], C.byref(pairs)),
            'asr_relattn_win_plan')
    return dict(zip(('bq', 'bk', 'blocks', 'lds'), (x.value for x in v)), tile_pairs=pairs.value)


def relattn_fwd(qkv, pos, bias_u, bias_v, out, N, heads, dh, lens=None, lse=None, scale=None,
                window=None):
    """out (T, n_pad, ld_out >= heads dh) of the relative positional attention core on the slab
    qkv (T, n_pad, ld >= 3 heads dh) = [Q | K | V]: s[t, u] = scale ((q_t + bias_u) . k_u +
    (q_t + bias_v) . pos[t - u + T - 1]) over the keys u < lens[n]; pos (2T - 1, ld_pos >= heads
    dh) is the projected table, bias_u / bias_v (heads dh); lse kept for relattn_bwd when given.
    window: None, or (chunk, left, right) as in attn_fwd (asr_relattn_win_fwd)."""
    _check_f32(qkv, pos, bias_u, bias_v, out, lse)
    _check_lens(lens, N)
    assert qkv.dim() == 3 and out.dim() == 3 and out.shape[:2] == qkv.shape[:2]
    assert pos.dim() == 2 and pos.shape[0] == 2 * qkv.shape[0] - 1 and pos.is_contiguous()
    a = _relattn_args(qkv, N, heads, dh, out.shape[2], pos.shape[1], scale, lens=lens, out=out,
                      lse=lse, pos=pos, bias_u=bias_u, bias_v=bias_v)
    if window is None:
        L.check(L.load().asr_relattn_fwd(C.byref(a), _stream()), 'asr_relattn_fwd')
    else:
        w = attn_window(window)
        L.check(L.load().asr_relattn_win_fwd(C.byref(a), C.byref(w), _stream()),
                'asr_relattn_win_fwd')
    return out


def relattn_bwd(qkv, pos, bias_u, bias_v, out, lse, dout, dqkv, dpos, dbias_u, dbias_v, N, heads,
                dh, lens=None, scale=None, window=None):
    """dqkv (like qkv) = dQ | dK | dV, dpos (like pos), dbias_u, dbias_v (heads dh) from dout (like
    out), recomputing p from lse; all four are written, not accumulated (window: that of the
    forward call)."""
    _check_f32(qkv, pos, bias_u, bias_v, out, lse, dout, dqkv, dpos, dbias_u, dbias_v)
    _check_lens(lens, N)
    assert dqkv.shape == qkv.shape and dout.shape == out.shape and dpos.shape == pos.shape
    assert pos.is_contiguous() and dpos.is_contiguous()
    a = _relattn_args(qkv, N, heads, dh, out.shape[2], pos.shape[1], scale, lens=lens, out=out,
                      lse=lse, dout=dout, dqkv=dqkv, pos=pos, bias_u=bias_u, bias_v=bias_v,
                      dpos=dpos, dbias_u=dbias_u, dbias_v=dbias_v)
    nbytes = L.load().asr_relattn_workspace_bytes(C.byref(a))
    if nbytes == 0:
        L.check(-1, 'asr_relattn_workspace_bytes (T %d N %d n_pad %d heads %d dh %d ld %d ld_out '
                '%d ld_pos %d)' % (a.T, a.N, a.n_pad, a.heads, a.dh, a.ld, a.ld_out, a.ld_pos))
    ws = WS.get('relattn', nbytes, qkv.device)
    if window is None:
        L.check(L.load().asr_relattn_bwd(C.byref(a), _ptr(ws), nbytes, _stream()),
                'asr_relattn_bwd')
    else:
        w = attn_window(window)
        L.check(L.load().asr_relattn_win_bwd(C.byref(a), C.byref(w), _ptr(ws), nbytes, _stream()),
                'asr_relattn_win_bwd')
    return dqkv


# --------------------------------------------------------------------------- dwconv, GLU, Swish (K22)
DWCONV_MAX_KERNEL = 63    # taps of asr_dwconv1d_* (odd, 'same' padding)


def dwconv1d_plan(T, n_pad, channels, k, ld=None, N=1, backward=False):
    """{'tile': frames per time tile, 'blocks': workgroups of the forward / weight-gradient launch,
    'lds': bytes of LDS per workgroup} of the geometry (asr_dwconv1d_plan)."""
    v = [C.c_int(0) for _ in range(3)]
    L.check(L.load().asr_dwconv1d_plan(int(T), int(N), int(n_pad), int(channels),
                                       int(ld or channels), int(k), int(bool(backward)),
                                       *[C.byref(x) for x in v]), 'asr_dwconv1d_plan')
    return dict(zip(('tile', 'blocks', 'lds'), (x.value for x in v)))


def dwconv1d_fwd(x, w, b, y, N, k, lens=None, C_=None, pad_left=None):
    """y[t, n, c] = b[c] + sum_j w[j, c] xm[t + j - (k - 1) / 2, n, c] over the slab x (T, n_pad,
    ld >= C), xm = x with the frames >= lens[n] (device int32; None: every frame) as zeros;
    w (k, C) tap major; zeros in the rows n >= N and the columns >= C (C_: default ld).
    pad_left: None, or the left padding 0 .. k - 1 in place of (k - 1) / 2 (asr_dwconv1d_pad_fwd;
    k - 1 is the causal convolution)."""
    _check_f32(x, w, b, y)
    _check_lens(lens, N)
    T, n_pad, ld = x.shape
    Cc = int(C_ or ld)
    assert y.shape == x.shape and w.numel() == k * Cc and b.numel() == Cc
    if pad_left is None:
        L.check(L.load().asr_dwconv1d_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(lens), _ptr(y), int(T),
                                          int(N), int(n_pad), Cc, int(ld), int(k), _stream()),
                'asr_dwconv1d_fwd')
    else:
        L.check(L.load().asr_dwconv1d_pad_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(lens), _ptr(y),
                                              int(T), int(N), int(n_pad), Cc, int(ld), int(k),
                                              int(pad_left), _stream()), 'asr_dwconv1d_pad_fwd')
    return y


def dwconv1d_bwd(x, w, dy, dx, dw, db, N, k, lens=None, C_=None, pad_left=None):
    """dw (k, C), db (C) (written) and dx (like x, or None) of dwconv1d_fwd (pad_left: that of the
    forward call)."""
    _check_f32(x, w, dy, dx, dw, db)
    _check_lens(lens, N)
    T, n_pad, ld = x.shape
    Cc = int(C_ or ld)
    assert dy.shape == x.shape and dw.numel() == k * Cc and db.numel() == Cc
    geo = (int(T), int(N), int(n_pad), Cc, int(ld), int(k))
    nbytes = L.load().asr_dwconv1d_workspace_bytes(*geo)
    if nbytes == 0:
        L.check(-1, 'asr_dwconv1d_workspace_bytes (T %d N %d n_pad %d C %d ld %d k %d)' % geo)
    ws = WS.get('dwconv', nbytes, x.device)
    if pad_left is None:
        L.check(L.load().asr_dwconv1d_bwd(_ptr(x), _ptr(w), _ptr(dy), _ptr(lens), _ptr(dx),
                                          _ptr(dw), _ptr(db), *geo, _ptr(ws), nbytes, _stream()),
                'asr_dwconv1d_bwd')
    else:
        L.check(L.load().asr_dwconv1d_pad_bwd(_ptr(x), _ptr(w), _ptr(dy), _ptr(lens), _ptr(dx),
                                              _ptr(dw), _ptr(db), *geo, int(pad_left), _ptr(ws),
                                              nbytes, _stream()), 'asr_dwconv1d_pad_bwd')
    return dx


def glu_fwd(x, y, C_=None):
    """y[..., c] = x[..., c] * sigmoid(x[..., C + c]) for c < C (default: half of x's last axis),
    zeros in the other columns of y."""
    _check_f32(x, y)
    ld_in, ld_out = x.shape[-1], y.shape[-1]
    Cc = int(C_ or ld_in // 2)
    rows = x.numel() // ld_in
    assert y.numel() // ld_out == rows
    L.check(L.load().asr_glu_fwd(_ptr(x), _ptr(y), rows, Cc, int(ld_in), int(ld_out), _stream()),
            'asr_glu_fwd')
    return y


def glu_bwd(x, dy, dx, C_=None):
    """dx (like x) = [dy sigma(g) | dy a sigma(g) (1 - sigma(g)) | zeros], sigma recomputed."""
    _check_f32(x, dy, dx)
    ld_in, ld_out = x.shape[-1], dy.shape[-1]
    Cc = int(C_ or ld_in // 2)
    rows = x.numel() // ld_in
    assert dx.shape == x.shape and dy.numel() // ld_out == rows
    L.check(L.load().asr_glu_bwd(_ptr(x), _ptr(dy), _ptr(dx), rows, Cc, int(ld_in), int(ld_out),
                                 _stream()), 'asr_glu_bwd')
    return dx


def swish_fwd(x, y):
    """y = x * sigmoid(x), element-wise."""
    _check_f32(x, y)
    L.check(L.load().asr_swish_fwd(_ptr(x), _ptr(y), x.numel(), _stream()), 'asr_swish_fwd')
    return y


def swish_bwd(x, dy, dx):
    """dx = dy * sigma(x) (1 + x (1 - sigma(x))), read from the input x."""
    _check_f32(x, dy, dx)
    L.check(L.load().asr_swish_bwd(_ptr(x), _ptr(dy), _ptr(dx), x.numel(), _stream()),
            'asr_swish_bwd')
    return dx


# --------------------------------------------------------------------------- time reduction (K33)
TIME_STACK_FACTORS = (2, 8)     # k of asr_time_stack_* (inclusive)


def time_stack_frames(T, k):
    """Frames of the stacked slab: ceil(T / k)."""
    return -(-int(T) // int(k))


def time_stack_fwd(x, y, N, F, k, lens=None):
    """y (ceil(T / k), n_pad, ld_out)[to, n, j F + f] = x (T, n_pad, ld_in)[to k + j, n, f] for
    j < k, f < F where to k + j < lens[n] (device int32; None and rows n >= N: every frame), zeros
    elsewhere, the columns k F .. ld_out included (csrc/timestack.hip)."""
    _check_f32(x, y)
    _check_lens(lens, N)
    T, n_pad, ld_in = x.shape
    To, n_pad_y, ld_out = y.shape
    assert To == time_stack_frames(T, k) and n_pad_y == n_pad
    L.check(L.load().asr_time_stack_fwd(_ptr(x), _ptr(lens), _ptr(y), int(T), int(N), int(n_pad),
                                        int(F), int(ld_in), int(ld_out), int(k), _stream()),
            'asr_time_stack_fwd')
    return y


def time_stack_bwd(dy, dx, N, F, k, lens=None):
    """The transpose of time_stack_fwd: dx (T, n_pad, ld_in)[t, n, f] = dy (ceil(T / k), n_pad,
    ld_out)[t // k, n, (t % k) F + f] for f < F where t < lens[n], zeros elsewhere.  Every
    element of dx is written."""
    _check_f32(dy, dx)
    _check_lens(lens, N)
    T, n_pad, ld_in = dx.shape
    To, n_pad_y, ld_out = dy.shape
    assert To == time_stack_frames(T, k) and n_pad_y == n_pad
    L.check(L.load().asr_time_stack_bwd(_ptr(dy), _ptr(lens), _ptr(dx), int(T), int(N), int(n_pad),
                                        int(F), int(ld_in), int(ld_out), int(k), _stream()),
            'asr_time_stack_bwd')
    return dx


# --------------------------------------------------------------------------- sequence-wise BN (K18)
def seqbn_stats_len(W):
    """Floats of a stats block: [mean_hi | mean_lo | invstd | var] (W each) + [|V|, 0, 0, 0]."""
    return 4 * int(W) + 4


def _seqbn_ws(T, N, n_pad, ld, W, device):
    nbytes = L.load().asr_seqbn_workspace_bytes(int(T), int(N), int(n_pad), int(ld), int(W))
    if nbytes == 0:
        L.check(-1, 'asr_seqbn_workspace_bytes (T %d N %d n_pad %d ld %d W %d)'
                % (T, N, n_pad, ld, W))
    return WS.get('bn', nbytes, device), nbytes


def _check_lens(lens, N):
    if lens is not None and (lens.dtype != torch.int32 or not lens.is_contiguous()
                             or lens.numel() < N or not lens.is_cuda):
        raise ValueError('lens: a contiguous CUDA int32 tensor of at least N = %d entries' % N)


def seqbn_fwd_train(p, y, gamma, beta, stats, N, W, lens=None, eps=1e-3, moments=None,
                    shift=None, weight=1.0):
    """Training-phase sequence-wise BatchNormalization of p (T, n_pad, ld): statistics over the
    valid rows (n < N, t < lens[n]; lens None: all frames), y for every real row; stats
    (seqbn_stats_len(W)); moments (bn_moments_len(W), optional) with w = weight * |V|."""
    _check_f32(p, y, gamma, beta, stats, moments, shift)
    _check_lens(lens, N)
    T, n_pad, ld = p.shape
    ws, nbytes = _seqbn_ws(T, N, n_pad, ld, W, p.device)
    L.check(L.load().asr_seqbn_fwd_train(_ptr(p), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(lens),
                                         _ptr(stats), _ptr(moments), _ptr(shift), float(weight),
                                         int(T), int(N), int(n_pad), int(ld), int(W), float(eps),
                                         _ptr(ws), nbytes, _stream()), 'asr_seqbn_fwd_train')
    return y


def seqbn_fwd_infer(p, y, gamma, beta, running_mean, running_var, N, W, eps=1e-3):
    """Inference-phase affine map on the running moments (one pass, no lengths)."""
    _check_f32(p, y, gamma, beta, running_mean, running_var)
    T, n_pad, ld = p.shape
    L.check(L.load().asr_seqbn_fwd_infer(_ptr(p), _ptr(y), _ptr(gamma), _ptr(beta),
                                         _ptr(running_mean), _ptr(running_var), int(T), int(N),
                                         int(n_pad), int(ld), int(W), float(eps), _stream()),
            'asr_seqbn_fwd_infer')
    return y


def seqbn_bwd(p, da, gamma, stats, dp, dgamma, N, W, lens=None, dbeta=None, dp_absmax=None):
    """dgamma (W), optional dbeta (W) -- both over every real row -- dp (same shape as p) with
    the valid / padded split, and max |dp| (1,), from the saved p and stats."""
    _check_f32(p, da, gamma, stats, dp, dgamma, dbeta, dp_absmax)
    _check_lens(lens, N)
    T, n_pad, ld = p.shape
    ws, nbytes = _seqbn_ws(T, N, n_pad, ld, W, p.device)
    L.check(L.load().asr_seqbn_bwd(_ptr(p), _ptr(da), _ptr(gamma), _ptr(lens), _ptr(stats),
                                   _ptr(dp), _ptr(dgamma), _ptr(dbeta), _ptr(dp_absmax), int(T),
                                   int(N), int(n_pad), int(ld), int(W), _ptr(ws), nbytes,
                                   _stream()), 'asr_seqbn_bwd')
    return dp


def lstm_dz_hl_supported(T, n_pad, H, mode=0, compact=False, act=0):
    """Whether lstm_seq_bwd would write packed planes for this geometry (asr_lstm_dz_hl_supported:
    the plain cell on the two-dimensional-split BPTT kernels, persistent mode, split-fp16)."""
    a = L.LstmArgs()
    a.T, a.n_pad, a.H, a.mode = int(T), int(n_pad), int(H), int(mode)
    a.compact = 1 if compact else 0
    a.activation = activation_id(act)
    a.lds_reserve_kb = LSTM_LDS_KB
    return bool(L.load().asr_lstm_dz_hl_supported(C.byref(a)))


def lstm_dz_guard(dz_absmax, dz_bound, planes_used, device=None):
    """Device-side upkeep of a layer's dz bound behind a BPTT pass (asr_lstm_dz_guard): keeps or
    renews *dz_bound from the measured *dz_absmax; with planes_used, a maximum outside the
    planes' safe range raises the BPTT workspace's sticky flag (the step is vetoed and re-run)."""
    ws = WS.get('lstm_bwd', 0, dz_absmax.device) if planes_used else None
    L.check(L.load().asr_lstm_dz_guard(_ptr(dz_absmax), _ptr(dz_bound), 1 if planes_used else 0,
                                       _ptr(ws) if ws is not None else None, _stream()),
            'asr_lstm_dz_guard')


def lstm_status(ws):
    L.check(L.load().asr_lstm_status(_ptr(ws), _stream()), 'asr_lstm_status')


def lstm_timeout_flags(device):
    """The sticky timeout flags of the forward / BPTT workspaces as one int32 tensor of two
    elements on the device (a snapshot enqueued on the current stream, no synchronisation);
    non-zero = a persistent kernel abandoned a bounded spin since the flag was cleared.
    Once a SimpleRNN recurrence has run in this process its workspaces' words are OR-ed in."""
    words = torch.stack([WS.get(name, 0, device)[:4].view(torch.int32)[0]
                         for name in ('lstm_fwd', 'lstm_bwd')])
    if _rnn_ran(device):
        words = torch.bitwise_or(words, torch.stack(
            [WS.get(name, 0, device)[:4].view(torch.int32)[0] for name in RNN_WS]))
    return words


def lstm_fast_chains(ws):
    return L.load().asr_lstm_fast_chains(_ptr(ws), _stream())


def lstm_profile(ws):
    out = (C.c_longlong * 24)()
    L.check(L.load().asr_lstm_profile(_ptr(ws), _stream(), out), 'asr_lstm_profile')
    return [[out[6 * w + i] for i in range(6)] for w in range(4)]


def lstm_plan(T, n_pad, H, backward, mode=0, compact=False, units=0, activation=0):
    """asr_lstm_plan for the form a call with these arguments would take (mode, compact,
    fwd_units and activation of asr_lstm_args; the ASR_LSTM_* switches act as in a call)."""
    lib = L.load()
    a = L.LstmArgs()
    a.T, a.n_pad, a.H, a.mode = int(T), int(n_pad), int(H), int(mode)
    a.compact = 1 if compact else 0
    a.fwd_units = int(units)
    a.activation = activation_id(activation)
    ks, r, blocks, cpl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    L.check(lib.asr_lstm_plan(C.byref(a), int(backward), C.byref(ks), C.byref(r),
                              C.byref(blocks), C.byref(cpl)), 'asr_lstm_plan')
    return dict(k_split=ks.value, k_per_lane=r.value, blocks=blocks.value,
                chains_per_launch=cpl.value)


# --------------------------------------------------------------------------- CTC
def ctc_loss_grad(logits, labels, label_len, seq_len, N, grad=None, grad_scale=1.0,
                  loss=None):
    """logits (T, n_pad, C) float32; labels (N, l_max) int32; returns loss (N,)."""
    lib = L.load()
    T, n_pad, Cc = logits.shape
    l_max = int(labels.shape[1])
    _check_f32(logits, grad)
    if loss is None:
        loss = torch.empty(N, dtype=torch.float32, device=logits.device)
    nbytes = lib.asr_ctc_workspace_bytes(T, int(N), n_pad, Cc, l_max)
    ws = WS.get('ctc', nbytes, logits.device)
    L.check(lib.asr_ctc_loss_grad(_ptr(logits), _ptr(labels), _ptr(label_len), _ptr(seq_len),
                                  T, int(N), n_pad, Cc, l_max, float(grad_scale), _ptr(loss),
                                  _ptr(grad), _ptr(ws), nbytes, _stream()),
            'asr_ctc_loss_grad')
    return loss


def ctc_greedy(logits, seq_len, N):
    lib = L.load()
    T, n_pad, Cc = logits.shape
    dec = torch.empty((int(N), T), dtype=torch.int32, device=logits.device)
    dlen = torch.empty(int(N), dtype=torch.int32, device=logits.device)
    L.check(lib.asr_ctc_greedy(_ptr(logits), _ptr(seq_len), T, int(N), n_pad, Cc, _ptr(dec),
                               _ptr(dlen), _stream()), 'asr_ctc_greedy')
    return dec, dlen


def ctc_greedy_stream(logits, seq_len, state, N):
    """ctc_greedy over one chunk (T, n_pad, C) of a stream's logits (K26, asr_ctc_greedy_stream):
    seq_len (device int32, N) the valid frames of THIS chunk, state (device int32, N) the arg-max
    of the stream's last valid frame (-1: none yet), read and updated.  Returns the labels this
    chunk adds, (N, T) padded with -1, and their counts."""
    T, n_pad, Cc = logits.shape
    dec = torch.empty((int(N), T), dtype=torch.int32, device=logits.device)
    dlen = torch.empty(int(N), dtype=torch.int32, device=logits.device)
    assert state.dtype == torch.int32 and state.numel() >= int(N) and state.is_contiguous()
    L.check(L.load().asr_ctc_greedy_stream(_ptr(logits), _ptr(seq_len), _ptr(state), T, int(N),
                                           n_pad, Cc, _ptr(dec), _ptr(dlen), _stream()),
            'asr_ctc_greedy_stream')
    return dec, dlen


# --------------------------------------------------------------------------- transducer (K31)
RNNT_MAX_J, RNNT_MAX_C, RNNT_MAX_LABELS = 512, 64, 255    # the limits of asr_rnnt_loss_grad


def _check_i32(t, n):
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= n, \
        'expected a contiguous int32 CUDA tensor of at least %d words' % n


def rnnt_loss_grad(enc, pred, W_out, b_out, labels, label_len, seq_len, N, J, grads=None,
                   grad_scale=1.0, loss=None):
    """The transducer loss (include/asr_hip.h K31) of enc (T, n_pad, Jp) and pred (U1, n_pad, Jp)
    through the joint's output layer W_out (J, C), b_out (C); labels (N, U1 - 1) int32, label_len
    and seq_len (N) int32, all on the device.  grads: None (loss only) or the four tensors
    (d_enc, d_pred, dW_out, db_out), which are WRITTEN, scaled by grad_scale.  Returns loss (N)."""
    lib = L.load()
    T, n_pad, Jp = enc.shape
    U1 = int(pred.shape[0])
    J, Cc, N = int(J), int(b_out.numel()), int(N)
    assert pred.shape[1:] == (n_pad, Jp) and Jp == (J + 3) // 4 * 4 and W_out.numel() == J * Cc
    d = tuple(grads) if grads is not None else (None,) * 4
    assert len(d) == 4
    _check_f32(enc, pred, W_out, b_out, *d)
    if d[0] is not None:
        assert d[0].shape == enc.shape and d[1].shape == pred.shape
        assert d[2].numel() == J * Cc and d[3].numel() == Cc
    l_max = U1 - 1
    if l_max:
        _check_i32(labels, N * l_max)
    _check_i32(label_len, N)
    _check_i32(seq_len, N)
    if loss is None:
        loss = torch.empty(N, dtype=torch.float32, device=enc.device)
    nbytes = lib.asr_rnnt_workspace_bytes(int(T), U1, N, int(n_pad), J, Cc)
    ws = WS.get('rnnt', nbytes, enc.device)
    L.check(lib.asr_rnnt_loss_grad(
        _ptr(enc), _ptr(pred), _ptr(W_out), _ptr(b_out), _ptr(labels) if l_max else None,
        _ptr(label_len), _ptr(seq_len), int(T), U1, N, int(n_pad), J, Cc, l_max,
        float(grad_scale), _ptr(loss), _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), _ptr(ws),
        nbytes, _stream()), 'asr_rnnt_loss_grad')
    return loss


def rnnt_greedy_step(enc, g_cur, W_out, b_out, seq_len, N, J, t_ptr, n_sym, decoded, decoded_len,
                     advance, x_next, active, max_symbols=10):
    """One iteration of frame-synchronous greedy transducer decoding (asr_rnnt_greedy_step): enc
    (T, n_pad, Jp), g_cur (n_pad, Jp) the predictor's current output; t_ptr, n_sym, decoded_len,
    advance (N) and active (1) int32, decoded (N, cap) int32, x_next (n_pad, ld) float32 the next
    predictor input, all on the device and updated in place."""
    T, n_pad, Jp = enc.shape
    J, Cc, N = int(J), int(b_out.numel()), int(N)
    _check_f32(enc, g_cur, W_out, b_out, x_next)
    assert g_cur.numel() >= n_pad * Jp and W_out.numel() == J * Cc
    assert x_next.shape[0] >= N and decoded.shape[0] >= N
    for t in (seq_len, t_ptr, n_sym, decoded_len, advance):
        _check_i32(t, N)
    _check_i32(decoded, N)
    _check_i32(active, 1)
    L.check(L.load().asr_rnnt_greedy_step(
        _ptr(enc), _ptr(g_cur), _ptr(W_out), _ptr(b_out), _ptr(seq_len), int(T), N, int(n_pad),
        J, Cc, int(max_symbols), int(decoded.shape[1]), int(x_next.shape[1]), _ptr(t_ptr),
        _ptr(n_sym), _ptr(decoded), _ptr(decoded_len), _ptr(advance), _ptr(x_next), _ptr(active),
        _stream()), 'asr_rnnt_greedy_step')


def onehot_rows(labels, label_len, N, n_pad, width, out=None, ld=None):
    """The predictor's input slab (U1, n_pad, ld) of labels (N, U1 - 1): position 0 (start of the
    sequence) and the padding are zero rows, label y_u is the unit vector at position u
    (asr_onehot_rows)."""
    l_max = int(labels.shape[1])
    ld = int(ld if ld is not None else width)
    if out is None:
        out = torch.empty((l_max + 1, int(n_pad), ld), dtype=torch.float32, device=labels.device)
    _check_f32(out)
    assert out.shape == (l_max + 1, int(n_pad), ld)
    if l_max:
        _check_i32(labels, int(N) * l_max)
    _check_i32(label_len, int(N))
    L.check(L.load().asr_onehot_rows(_ptr(labels) if l_max else None, _ptr(label_len), l_max + 1,
                                     int(N), int(n_pad), l_max, int(width), ld, _ptr(out),
                                     _stream()), 'asr_onehot_rows')
    return out


def rows_select(mask, a, b, out, N):
    """out[n, :] = a[n, :] where mask[n] != 0 (n < N), b[n, :] elsewhere; out may be a or b
    (asr_rows_select)."""
    _check_f32(a, b, out)
    assert a.shape == b.shape == out.shape and a.dim() == 2
    _check_i32(mask, int(N))
    L.check(L.load().asr_rows_select(_ptr(mask), _ptr(a), _ptr(b), _ptr(out), int(N),
                                     int(a.shape[0]), int(a.shape[1]), _stream()),
            'asr_rows_select')
    return out


# --------------------------------------------------------------------------- attention decoder (K32)
AED_MAX_J, AED_MAX_C, AED_MAX_LABELS = 512, 64, 255      # the limits of asr_aed_loss_grad


def _attn_cross_args(q, kv, out, N, heads, dh, scale, **tensors):
    assert q.dim() == 3 and kv.dim() == 3 and out.dim() == 3
    assert kv.shape[1] == q.shape[1] and out.shape[:2] == q.shape[:2]
    a = L.AttnCrossArgs()
    a.Tq, a.Tk, a.N, a.n_pad = int(q.shape[0]), int(kv.shape[0]), int(N), int(q.shape[1])
    a.heads, a.dh = int(heads), int(dh)
    a.ld_q, a.ld_kv, a.ld_out = int(q.shape[2]), int(kv.shape[2]), int(out.shape[2])
    a.scale = float(scale if scale is not None else 1.0 / math.sqrt(dh))
    for k, t in dict(tensors, q=q, kv=kv, out=out).items():
        setattr(a, k, None if t is None else t.data_ptr())
    return a


def attn_cross_fwd(q, kv, out, N, heads, dh, q_lens=None, k_lens=None, lse=None, scale=None):
    """out (Tq, n_pad, ld_out >= heads dh) = softmax(scale Q K^T) V per real sample and head: Q the
    first heads dh columns of q (Tq, n_pad, ld_q), [K | V] the first 2 heads dh columns of kv (Tk,
    n_pad, ld_kv).  Keys u >= k_lens[n] carry probability 0; a query row t >= q_lens[n] has out =
    lse = 0 (device int32 (N), both optional).  lse (attn_lse_len(Tq, ..)) is kept for
    attn_cross_bwd when given (asr_attn_cross_fwd: the kernels of attn_fwd)."""
    _check_f32(q, kv, out, lse)
    _check_lens(q_lens, N)
    _check_lens(k_lens, N)
    a = _attn_cross_args(q, kv, out, N, heads, dh, scale, q_lens=q_lens, k_lens=k_lens, lse=lse)
    L.check(L.load().asr_attn_cross_fwd(C.byref(a), _stream()), 'asr_attn_cross_fwd')
    return out


def attn_cross_bwd(q, kv, out, lse, dout, dq, dkv, N, heads, dh, q_lens=None, k_lens=None,
                   scale=None):
    """dq (like q) and dkv (like kv) = dK | dV from dout (like out), recomputing p from lse; both
    are WRITTEN, pad columns and padding rows as zeros (asr_attn_cross_bwd)."""
    _check_f32(q, kv, out, lse, dout, dq, dkv)
    _check_lens(q_lens, N)
    _check_lens(k_lens, N)
    assert dq.shape == q.shape and dkv.shape == kv.shape and dout.shape == out.shape
    a = _attn_cross_args(q, kv, out, N, heads, dh, scale, q_lens=q_lens, k_lens=k_lens, lse=lse,
                         dout=dout, dq=dq, dkv=dkv)
    nbytes = L.load().asr_attn_cross_workspace_bytes(C.byref(a))
    if nbytes == 0:
        L.check(-1, 'asr_attn_cross_workspace_bytes (Tq %d Tk %d N %d n_pad %d heads %d dh %d '
                'ld_q %d ld_kv %d ld_out %d)' % (a.Tq, a.Tk, a.N, a.n_pad, a.heads, a.dh, a.ld_q,
                                                 a.ld_kv, a.ld_out))
    ws = WS.get('attn', nbytes, q.device)
    L.check(L.load().asr_attn_cross_bwd(C.byref(a), _ptr(ws), nbytes, _stream()),
            'asr_attn_cross_bwd')
    return dq, dkv


def aed_loss_grad(ctx, q, W_out, b_out, labels, label_len, N, grads=None, grad_scale=1.0,
                  eps=0.0, loss=None):
    """The attention decoder's loss (include/asr_hip.h K32): the label-smoothed cross-entropy of
    tanh(ctx + q) W_out + b_out, ctx and q (U1, n_pad, J), W_out (J, C), b_out (C); labels (N,
    U1 - 1) int32 and label_len (N) int32 on the device; row u of utterance n is scored against
    label u, row label_len[n] against EOS = C - 1.  grads: None (loss only) or the four tensors
    (d_ctx, d_q, dW_out, db_out), which are WRITTEN, scaled by grad_scale (d_ctx and d_q get the
    same values).  Returns loss (N)."""
    lib = L.load()
    U1, n_pad, J = (int(v) for v in ctx.shape)
    Cc, N = int(b_out.numel()), int(N)
    assert q.shape == ctx.shape and W_out.numel() == J * Cc
    d = tuple(grads) if grads is not None else (None,) * 4
    assert len(d) == 4
    _check_f32(ctx, q, W_out, b_out, *d)
    if d[0] is not None:
        assert d[0].shape == ctx.shape and d[1].shape == ctx.shape
        assert d[2].numel() == J * Cc and d[3].numel() == Cc
    l_max = U1 - 1
    if l_max:
        _check_i32(labels, N * l_max)
    _check_i32(label_len, N)
    if loss is None:
        loss = torch.empty(N, dtype=torch.float32, device=ctx.device)
    nbytes = lib.asr_aed_workspace_bytes(U1, N, n_pad, J, Cc)
    ws = WS.get('aed', nbytes, ctx.device)
    L.check(lib.asr_aed_loss_grad(
        _ptr(ctx), _ptr(q), _ptr(W_out), _ptr(b_out), _ptr(labels) if l_max else None,
        _ptr(label_len), U1, N, n_pad, J, Cc, l_max, float(eps), float(grad_scale), _ptr(loss),
        _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), _ptr(ws), nbytes, _stream()),
        'asr_aed_loss_grad')
    return loss


def aed_greedy_step(ctx, q, W_out, b_out, N, finished, decoded, decoded_len, advance, x_next,
                    active, max_labels=AED_MAX_LABELS):
    """One iteration of label-synchronous greedy decoding (asr_aed_greedy_step): ctx, q (n_pad, J)
    the current context and query rows; finished, decoded_len, advance (N) and active (1) int32,
    decoded (N, cap) int32, x_next (n_pad, ld) float32 the next predictor input, all on the device
    and updated in place."""
    n_pad, J = int(ctx.shape[-2]), int(ctx.shape[-1])
    Cc, N = int(b_out.numel()), int(N)
    _check_f32(ctx, q, W_out, b_out, x_next)
    assert ctx.numel() == n_pad * J and q.numel() == n_pad * J and W_out.numel() == J * Cc
    assert x_next.shape[0] >= N and decoded.shape[0] >= N
    for t in (finished, decoded_len, advance):
        _check_i32(t, N)
    _check_i32(decoded, N)
    _check_i32(active, 1)
    L.check(L.load().asr_aed_greedy_step(
        _ptr(ctx), _ptr(q), _ptr(W_out), _ptr(b_out), N, n_pad, J, Cc, int(max_labels),
        int(decoded.shape[1]), int(x_next.shape[1]), _ptr(finished), _ptr(decoded),
        _ptr(decoded_len), _ptr(advance), _ptr(x_next), _ptr(active), _stream()),
        'asr_aed_greedy_step')


# --------------------------------------------------------------------------- streaming (K26)
def attn_stream_plan(window, max_tq):
    """Rows of the smallest [K | V] ring (a multiple of 64) that is valid for every call of up to
    max_tq new frames under the window (chunk, left >= 0, 0) (asr_attn_stream_plan; the ring
    convention is stated once in csrc/attn_tile.h)."""
    rows = C.c_int(0)
    w = attn_window(window)
    L.check(L.load().asr_attn_stream_plan(C.byref(w), int(max_tq), C.byref(rows)),
            'asr_attn_stream_plan')
    return rows.value


def ring_put(src, ring, t0, col0=0, cols=None):
    """Rows [0, Tq) of the columns [col0, col0 + cols) of the slab src (Tq, n_pad, ld) into the
    columns [0, cols) of the ring rows (t0 + i) % R of ring (R, n_pad, ld_ring) (asr_ring_put)."""
    _check_f32(src, ring)
    Tq, n_pad, ld = src.shape
    assert ring.dim() == 3 and ring.shape[1] == n_pad
    cols = int(ld - col0 if cols is None else cols)
    L.check(L.load().asr_ring_put(_ptr(src), _ptr(ring), int(Tq), int(n_pad), int(ld), int(col0),
                                  cols, int(ring.shape[2]), int(ring.shape[0]), int(t0),
                                  _stream()), 'asr_ring_put')
    return ring


def _attn_stream_args(q, ring, kv_len, out, N, heads, dh, t0, scale):
    Tq, n_pad, ld = q.shape
    assert ring.dim() == 3 and ring.shape[1] == n_pad and out.shape[:2] == q.shape[:2]
    assert kv_len.dtype == torch.int32 and kv_len.numel() >= int(N)
    a = L.AttnStreamArgs()
    a.Tq, a.N, a.n_pad, a.heads, a.dh = int(Tq), int(N), int(n_pad), int(heads), int(dh)
    a.ld, a.ld_kv, a.ld_out = int(ld), int(ring.shape[2]), int(out.shape[2])
    a.R, a.t0 = int(ring.shape[0]), int(t0)
    a.scale = float(scale if scale is not None else 1.0 / math.sqrt(dh))
    a.q, a.ring, a.kv_len, a.out = q.data_ptr(), ring.data_ptr(), kv_len.data_ptr(), out.data_ptr()
    return a


def attn_stream_fwd(q, ring, kv_len, out, N, heads, dh, t0, window, scale=None):
    """attn_fwd under `window` for the queries [t0, t0 + Tq) of a stream: q (Tq, n_pad, ld >= heads
    dh) holds Q in its first columns (the chunk's qkv slab serves), ring (R, n_pad, >= 2 heads dh)
    the [K | V] of the absolute frames u at rows u % R, the new ones already put (ring_put);
    kv_len (device int32, N): the absolute frames valid so far.  The rows of the whole-utterance
    call, bit for bit (asr_attn_stream_fwd)."""
    _check_f32(q, ring, out)
    a = _attn_stream_args(q, ring, kv_len, out, N, heads, dh, t0, scale)
    w = attn_window(window)
    L.check(L.load().asr_attn_stream_fwd(C.byref(a), C.byref(w), _stream()),
            'asr_attn_stream_fwd')
    return out


def relattn_stream_fwd(q, ring, kv_len, pos, bias_u, bias_v, out, N, heads, dh, t0, window,
                       scale=None):
    """relattn_fwd under `window` for the queries [t0, t0 + Tq) of a stream (as attn_stream_fwd);
    pos (2P - 1, ld_pos) is the projected table of the relative indices -(P - 1) .. P - 1,
    P >= left + chunk (asr_relattn_stream_fwd)."""
    _check_f32(q, ring, out, pos, bias_u, bias_v)
    assert pos.dim() == 2 and pos.shape[0] % 2 == 1
    a = _attn_stream_args(q, ring, kv_len, out, N, heads, dh, t0, scale)
    a.P, a.ld_pos = (int(pos.shape[0]) + 1) // 2, int(pos.shape[1])
    a.pos, a.bias_u, a.bias_v = pos.data_ptr(), bias_u.data_ptr(), bias_v.data_ptr()
    w = attn_window(window)
    L.check(L.load().asr_relattn_stream_fwd(C.byref(a), C.byref(w), _stream()),
            'asr_relattn_stream_fwd')
    return out


def dwconv1d_stream_fwd(ring, w, b, lens, y, N, k, t0, C_=None):
    """The causal dwconv1d_fwd (pad_left = k - 1) for the output frames [t0, t0 + Tq) of a stream:
    y (Tq, n_pad, ld); ring (Rc >= k - 1 + Tq, n_pad, ld) holds the input's absolute frame u at
    row u % Rc; lens (device int32, N): absolute lengths (asr_dwconv1d_stream_fwd)."""
    _check_f32(ring, w, b, y)
    Tq, n_pad, ld = y.shape
    Cc = int(C_ or ld)
    assert ring.shape[1:] == y.shape[1:] and w.numel() == k * Cc and b.numel() == Cc
    assert lens.dtype == torch.int32 and lens.numel() >= int(N)
    L.check(L.load().asr_dwconv1d_stream_fwd(_ptr(ring), _ptr(w), _ptr(b), _ptr(lens), _ptr(y),
                                             int(Tq), int(N), int(n_pad), Cc, int(ld), int(k),
                                             int(ring.shape[0]), int(t0), _stream()),
            'asr_dwconv1d_stream_fwd')
    return y


def _check_align_labels(labels, label_len, N, Cc):
    """Host-side argument checks of ctc_align / ctc_align_host (numpy views of the labels)."""
    if labels.ndim != 2 or labels.shape[0] < N or labels.shape[1] < 1 or len(label_len) < N:
        raise ValueError('ctc_align: labels must be (N, l_max >= 1) with N label lengths, got %s '
                         'and %d lengths for N = %d' % (tuple(labels.shape), len(label_len), N))
    if N and (label_len[:N].min() < 0 or label_len[:N].max() > labels.shape[1]):
        raise ValueError('ctc_align: label lengths must lie in [0, %d]' % labels.shape[1])
    used = np.arange(labels.shape[1])[None, :] < label_len[:N, None]
    bad = used & ((labels[:N] < 0) | (labels[:N] > Cc - 2))
    if bad.any():
        n, q = np.argwhere(bad)[0]
        raise ValueError('ctc_align: label %d of utterance %d is %d, outside [0, %d] (the blank '
                         'is %d)' % (q, n, labels[n, q], Cc - 2, Cc - 1))


def ctc_align(logits, labels, label_len, seq_len, N):
    """K19 forced alignment on the device (asr_ctc_align).  logits (T, n_pad, C) float32, labels
    (N, l_max) int32, label_len / seq_len (N,) int32, all DEVICE tensors as ctc_loss_grad takes
    them -> (path (N, T) int32, score (N,) float32) device tensors: path[n, t] is the state of
    the CTC lattice at frame t (even: a blank, odd s: label (s - 1) // 2), -1 past seq_len[n] and
    on the whole row when the transcript does not fit; score is the natural-log probability of
    the path (-inf then).  Labels outside [0, C - 2] raise ValueError."""
    lib = L.load()
    T, n_pad, Cc = logits.shape
    N = int(N)
    _check_f32(logits)
    _check_align_labels(labels.cpu().numpy(), label_len.cpu().numpy(), N, Cc)
    l_max = int(labels.shape[1])
    dev = logits.device
    labels = labels.to(dev, torch.int32).contiguous()
    label_len = label_len.to(dev, torch.int32).contiguous()
    seq_len = seq_len.to(dev, torch.int32).contiguous()
    path = torch.empty((N, T), dtype=torch.int32, device=dev)
    score = torch.empty(N, dtype=torch.float32, device=dev)
    nbytes = lib.asr_ctc_align_workspace_bytes(T, N, n_pad, Cc, l_max)
    key = ('ctc_align', str(dev))
    ws = WS.bufs.get(key)                       # (never read before it is written: no zero fill)
    if ws is None or ws.numel() < nbytes:
        ws = WS.bufs[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    L.check(lib.asr_ctc_align(_ptr(logits), _ptr(labels), _ptr(label_len), _ptr(seq_len), T, N,
                              n_pad, Cc, l_max, _ptr(path), _ptr(score), _ptr(ws), nbytes,
                              _stream()), 'asr_ctc_align')
    return path, score


def ctc_align_host(logits_host, labels, label_len, seq_len, N):
    """ctc_align on the host (asr_ctc_align_host: float32, one utterance per host thread): numpy
    arrays in, (path (N, T) int32, score (N,) float32) numpy arrays out."""
    lib = L.load()
    logits_host = np.ascontiguousarray(logits_host, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    label_len = np.ascontiguousarray(label_len, dtype=np.int32).reshape(-1)
    seq = np.ascontiguousarray(seq_len, dtype=np.int32).reshape(-1)
    if logits_host.ndim != 3:
        raise ValueError('ctc_align_host: logits must be (T, n_pad, C)')
    T, n_pad, Cc = logits_host.shape
    N = int(N)
    _check_align_labels(labels, label_len, N, Cc)
    if len(seq) < N:
        raise ValueError('ctc_align_host: %d sequence lengths for N = %d' % (len(seq), N))
    path = np.empty((N, T), dtype=np.int32)
    score = np.empty(N, dtype=np.float32)
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.check(lib.asr_ctc_align_host(as_p(logits_host), as_p(labels), as_p(label_len), as_p(seq), T,
                                   N, n_pad, Cc, int(labels.shape[1]), as_p(path), as_p(score)),
            'asr_ctc_align_host')
    return path, score


def ctc_segments(path_row, labels_row):
    """One row of an alignment path -> [(label_index, label, start_frame, end_frame_exclusive)],
    one entry per label of the transcript, in order; blank frames belong to no entry.  A row of
    -1 (no alignment) gives []; a path that does not spell ``labels_row`` raises ValueError."""
    path_row = np.asarray(path_row).reshape(-1)
    labels_row = [int(l) for l in np.asarray(labels_row).reshape(-1)]
    segs = []
    for t, s in enumerate(path_row.tolist()):
        if s < 0:
            break
        if s & 1:
            q = (s - 1) // 2
            if segs and segs[-1][0] == q and segs[-1][3] == t:
                segs[-1][3] = t + 1
            else:
                segs.append([q, labels_row[q] if q < len(labels_row) else -1, t, t + 1])
    if not segs and (len(path_row) == 0 or path_row[0] < 0):
        return []
    if [g[0] for g in segs] != list(range(len(labels_row))):
        raise ValueError('ctc_segments: the path visits labels %s, the transcript has %d'
                         % ([g[0] for g in segs], len(labels_row)))
    return [tuple(g) for g in segs]


def ctc_beam_search(logits, seq_len, N, beam_width=100, merge_repeated=True):
    """K9 on the device: logits (T, n_pad, C) float32 and seq_len (N,) int32 DEVICE tensors ->
    (decoded (N, T) int32 padded with -1, decoded_len (N,), log_score (N,)) device tensors; same
    results as ctc_beam_search_host (asr_ctc_beam_device).  The prefix-tree workspace is sized
    for the hard bound (T * width child blocks per utterance) and is not initialised."""
    lib = L.load()
    T, n_pad, Cc = logits.shape
    _check_f32(logits)
    dev = logits.device
    dec = torch.empty((int(N), T), dtype=torch.int32, device=dev)
    dlen = torch.empty(int(N), dtype=torch.int32, device=dev)
    score = torch.empty(int(N), dtype=torch.float32, device=dev)
    nbytes = lib.asr_ctc_beam_device_workspace_bytes(T, int(N), Cc, int(beam_width))
    key = ('beam', str(dev))
    ws = WS.bufs.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = WS.bufs[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    L.check(lib.asr_ctc_beam_device(_ptr(logits), _ptr(seq_len), T, int(N), n_pad, Cc,
                                    int(beam_width), int(bool(merge_repeated)), _ptr(dec),
                                    _ptr(dlen), _ptr(score), _ptr(ws), nbytes, _stream()),
            'asr_ctc_beam_device')
    return dec, dlen, score


def _lm_table_shape(w, Cc, order):
    order = int(order)
    if not 1 <= order <= 5:
        raise ValueError('ctc_beam_search_lm: order must be 1 .. 5, got %d' % order)
    want = (int(Cc) ** (order - 1), int(Cc) - 1)
    if tuple(w.shape) != want:
        raise ValueError('ctc_beam_search_lm: the fused table has shape %s, order %d over %d '
                         'classes needs %s' % (tuple(w.shape), order, Cc, want))
    return order


def ctc_beam_search_lm(logits, seq_len, N, beam_width, merge_repeated, w, order):
    """K9 with a character LM on the device (asr_ctc_beam_lm_device): as ctc_beam_search, plus
    ``w`` -- the FUSED table CharLM.fused(alpha, beta) as a float32 DEVICE tensor (n_ctx, C - 1)
    -- and the model's ``order``.  Same results as ctc_beam_search_lm_host."""
    lib = L.load()
    T, n_pad, Cc = logits.shape
    _check_f32(logits, w)
    order = _lm_table_shape(w, Cc, order)
    if w.device != logits.device or not w.is_contiguous():
        raise ValueError('ctc_beam_search_lm: the fused table must be contiguous on %s'
                         % logits.device)
    dev = logits.device
    dec = torch.empty((int(N), T), dtype=torch.int32, device=dev)
    dlen = torch.empty(int(N), dtype=torch.int32, device=dev)
    score = torch.empty(int(N), dtype=torch.float32, device=dev)
    nbytes = lib.asr_ctc_beam_lm_device_workspace_bytes(T, int(N), Cc, int(beam_width))
    key = ('beam_lm', str(dev))
    ws = WS.bufs.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = WS.bufs[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    L.check(lib.asr_ctc_beam_lm_device(_ptr(logits), _ptr(seq_len), T, int(N), n_pad, Cc,
                                       int(beam_width), int(bool(merge_repeated)), _ptr(w),
                                       order, _ptr(dec), _ptr(dlen), _ptr(score), _ptr(ws),
                                       nbytes, _stream()),
            'asr_ctc_beam_lm_device')
    return dec, dlen, score


class BeamStreamState(object):
    """What ctc_beam_stream carries between the chunks of N streams (K27): ``rec``, the state
    records (a zero-filled uint8 tensor: fresh streams), and the prefix-tree workspace, which
    belongs to THIS object -- two sessions never share a tree -- and is allocated at the first
    call: asr_ctc_beam_stream_workspace_bytes, about max_frames * width * (C - 1) * 8 bytes per
    stream, never filled.  ``lm``: None or (fused table as a float32 device tensor, order)."""
    HEADER = ('nb', 'nblocks', 'frames_done', 'stable_node', 'overflow')

    def __init__(self, N, num_classes, width, max_frames, lm=None, device='cuda:0'):
        self.N, self.C, self.width = int(N), int(num_classes), int(width)
        self.max_frames, self.lm = int(max_frames), lm
        lib = L.load()
        flag = int(lm is not None)
        self.rec_bytes = int(lib.asr_ctc_beam_stream_state_bytes(self.N, self.C, self.width, flag))
        self.ws_bytes = int(lib.asr_ctc_beam_stream_workspace_bytes(self.max_frames, self.N,
                                                                    self.C, self.width, flag))
        if self.rec_bytes == 0 or self.ws_bytes == 0:
            raise ValueError('beam stream: %d streams, %d classes (2 .. 64), width %d (1 .. 1024), '
                             'max_frames %d (>= 1, max_frames * width * (classes - 1) < 2^31)'
                             % (self.N, self.C, self.width, self.max_frames))
        if lm is not None:
            _lm_table_shape(lm[0], self.C, lm[1])
        self.rec = torch.zeros(self.rec_bytes, dtype=torch.uint8, device=device)
        self.ws = None

    def zero_(self):
        """Fresh streams; the tree is left as it is (blocks are initialised when allocated)."""
        self.rec.zero_()

    def counters(self, stream=0):
        """The work counters at the head of a stream's tree, summed over its calls since the
        record was fresh (synchronises): seconds in the frame phases and in the stable-prefix
        walk, and the event counts (asr_ctc_beam_device_counters)."""
        per = self.ws_bytes // self.N
        v = self.ws[stream * per:stream * per + 64].cpu().numpy().view(np.int64)
        out = {k: float(v[i]) * 1e-8 for i, k in enumerate(('branch_s', 'rank_s', 'turns_s',
                                                              'handover_s'))}
        out.update(turns=int(v[4]), inserts=int(v[5]), blocks=int(v[6]), walk_s=float(v[7]) * 1e-8)
        return out

    def header(self):
        """The records' header fields as host integers (synchronises): {name: (N,) array}."""
        h = self.rec.view(self.N, -1)[:, :32].contiguous().cpu().numpy().view(np.int32)
        return {k: h[:, i].copy() for i, k in enumerate(self.HEADER)}


def ctc_beam_stream(logits, chunk_len, state, N, width, merge, max_frames, lm=None):
    """K27: the device beam search over one chunk (Tq, n_pad, C) of the logits of N streams
    (asr_ctc_beam_stream / asr_ctc_beam_lm_stream).  chunk_len (device int32, N): the valid frames
    of this chunk; state: a BeamStreamState of the same N, width, max_frames and lm, read and
    updated.  -> (decoded (N, max_frames) padded with -1, decoded_len, stable_len, log_score):
    the current best hypothesis of every stream and how many of its labels are final."""
    lib = L.load()
    Tq, n_pad, Cc = logits.shape
    _check_f32(logits)
    if (state.N, state.C, state.width, state.max_frames) != (int(N), Cc, int(width),
                                                             int(max_frames)):
        raise ValueError('ctc_beam_stream: the state was made for %r'
                         % ((state.N, state.C, state.width, state.max_frames),))
    # the table is the state's: a stream cannot change its LM between two chunks
    if lm is not None and (state.lm is None or lm[0] is not state.lm[0]
                           or int(lm[1]) != int(state.lm[1])):
        raise ValueError('ctc_beam_stream: lm is not the table the state was made with')
    lm = state.lm
    dev = logits.device
    if not (torch.is_tensor(chunk_len) and chunk_len.dtype == torch.int32
            and chunk_len.device == dev and chunk_len.is_contiguous()
            and chunk_len.numel() >= int(N)):
        raise ValueError('ctc_beam_stream: chunk_len must be a contiguous int32 tensor of %d '
                         'entries on %s' % (int(N), dev))
    if state.rec.device != dev or n_pad < int(N):
        raise ValueError('ctc_beam_stream: the state lives on %s, the logits (%d rows for %d '
                         'streams) on %s' % (state.rec.device, n_pad, int(N), dev))
    if state.ws is None:
        state.ws = torch.empty(state.ws_bytes, dtype=torch.uint8, device=dev)
    dec = torch.empty((int(N), int(max_frames)), dtype=torch.int32, device=dev)
    dlen = torch.empty(int(N), dtype=torch.int32, device=dev)
    stable = torch.empty(int(N), dtype=torch.int32, device=dev)
    score = torch.empty(int(N), dtype=torch.float32, device=dev)
    head = (_ptr(logits), _ptr(chunk_len), Tq, int(N), n_pad, Cc, int(width), int(bool(merge)))
    tail = (int(max_frames), _ptr(state.rec), state.rec_bytes, _ptr(state.ws), state.ws_bytes,
            _ptr(dec), _ptr(dlen), _ptr(stable), _ptr(score), _stream())
    if lm is None:
        L.check(lib.asr_ctc_beam_stream(*(head + tail)), 'asr_ctc_beam_stream')
    else:
        w, order = lm
        _check_f32(w)
        order = _lm_table_shape(w, Cc, order)
        if w.device != dev or not w.is_contiguous():
            raise ValueError('ctc_beam_stream: the fused table must be contiguous on %s' % dev)
        L.check(lib.asr_ctc_beam_lm_stream(*(head + (_ptr(w), order) + tail)),
                'asr_ctc_beam_lm_stream')
    return dec, dlen, stable, score


def ctc_beam_lm_counters(logits_shape, N, beam_width, utterance=0, device='cuda:0'):
    """ctc_beam_counters for the last ctc_beam_search_lm call of that shape."""
    lib = L.load()
    T, n_pad, Cc = logits_shape
    ws = WS.bufs[('beam_lm', str(torch.device(device)))]
    out = (C.c_longlong * 7)()
    L.check(lib.asr_ctc_beam_lm_device_counters(_ptr(ws), int(T), int(N), int(Cc),
                                                int(beam_width), int(utterance), out, _stream()),
            'asr_ctc_beam_lm_device_counters')
    return dict(update_s=out[0] * 1e-8, rank_s=out[1] * 1e-8, turns_s=out[2] * 1e-8,
                handover_s=out[3] * 1e-8, turns=out[4], insertions=out[5], blocks=out[6])


def ctc_beam_search_lm_host(logits_host, seq_len_host, N, beam_width, merge_repeated, w, order):
    """ctc_beam_search_host with a character LM: ``w`` is the fused float32 table (n_ctx, C - 1)
    as a numpy array (asr_ctc_beam_lm_host)."""
    lib = L.load()
    logits_host = np.ascontiguousarray(logits_host, dtype=np.float32)
    seq = np.ascontiguousarray(seq_len_host, dtype=np.int32)
    T, n_pad, Cc = logits_host.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    order = _lm_table_shape(w, Cc, order)
    dec = np.empty((int(N), T), dtype=np.int32)
    dlen = np.empty(int(N), dtype=np.int32)
    score = np.empty(int(N), dtype=np.float32)
    L.check(lib.asr_ctc_beam_lm_host(
        logits_host.ctypes.data_as(C.c_void_p), seq.ctypes.data_as(C.c_void_p), T, int(N),
        n_pad, Cc, int(beam_width), int(bool(merge_repeated)), w.ctypes.data_as(C.c_void_p),
        order, dec.ctypes.data_as(C.c_void_p), dlen.ctypes.data_as(C.c_void_p),
        score.ctypes.data_as(C.c_void_p)), 'asr_ctc_beam_lm_host')
    return [dec[n, :dlen[n]].tolist() for n in range(int(N))], score


HOST_BEAM_MAX_UTTERANCES = 64


def beam_decoder_choice(N, width, classes, on_device=True):
    """Which K9 decoder serves a batch of N utterances: 'host' (decode_host.cpp: one utterance
    per host thread, after a D2H copy of the logits) or 'device' (beam.hip: one wave per
    utterance, logits stay in HBM).  Both give the same strings (tests/test_gpu_beam.py); the
    default is decided on measurements (profiles/r6_beam_crossover.md, tools/beam_crossover.py:
    N x 999 frames x 28 classes on a 256-thread host).  The device decoder's time is FLAT in N up
    to one wave per CU (0.118 s at 64, 256 and 0.126 s at 512 utterances, width 100) while the
    host decoder's grows faster than N once more than ~64 threads decode at once (0.08 s at 64,
    0.82 s at 256, 2.1 s at 512; on 8 host threads 0.35 s at 64): ASR_BEAM=auto (default) takes
    the host decoder for N <= min(USABLE host threads, 64) and the device decoder beyond -- the
    BASELINE eval batch (64 utterances) decodes on the host of a many-core box, larger batches and
    small hosts on the device; ASR_BEAM=device / host force one.  The device kernel handles
    widths <= 1024 and <= 64 classes."""
    import os
    mode = os.environ.get('ASR_BEAM', 'auto')
    device_ok = on_device and int(width) <= 1024 and int(classes) <= 64
    if mode == 'host' or not device_ok:
        return 'host'
    if mode == 'device':
        return 'device'
    return 'host' if int(N) <= min(usable_host_threads(), HOST_BEAM_MAX_UTTERANCES) else 'device'


def usable_host_threads():
    """Host threads this PROCESS may run on: the affinity mask where the platform has one (a
    container or a taskset limits it below os.cpu_count()), else the CPU count."""
    import os
    try:
        return max(1, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        return os.cpu_count() or 1


def ctc_beam_counters(logits_shape, N, beam_width, utterance=0, device='cuda:0'):
    """Work counters of the last ctc_beam_search call of that shape (see
    asr_ctc_beam_device_counters): dict of seconds per phase and event counts."""
    lib = L.load()
    T, n_pad, Cc = logits_shape
    ws = WS.bufs[('beam', str(torch.device(device)))]
    out = (C.c_longlong * 7)()
    L.check(lib.asr_ctc_beam_device_counters(_ptr(ws), int(T), int(N), int(Cc), int(beam_width),
                                             int(utterance), out, _stream()),
            'asr_ctc_beam_device_counters')
    return dict(update_s=out[0] * 1e-8, rank_s=out[1] * 1e-8, turns_s=out[2] * 1e-8,
                handover_s=out[3] * 1e-8, turns=out[4], insertions=out[5], blocks=out[6])


def ctc_beam_search_host(logits_host, seq_len_host, N, beam_width=100, merge_repeated=True):
    """logits_host: (T, n_pad, C) float32 numpy array (already on the host)."""
    lib = L.load()
    logits_host = np.ascontiguousarray(logits_host, dtype=np.float32)
    seq = np.ascontiguousarray(seq_len_host, dtype=np.int32)
    T, n_pad, Cc = logits_host.shape
    dec = np.empty((int(N), T), dtype=np.int32)
    dlen = np.empty(int(N), dtype=np.int32)
    score = np.empty(int(N), dtype=np.float32)
    L.check(lib.asr_ctc_beam(
        logits_host.ctypes.data_as(C.c_void_p), seq.ctypes.data_as(C.c_void_p), T, int(N),
        n_pad, Cc, int(beam_width), int(bool(merge_repeated)),
        dec.ctypes.data_as(C.c_void_p), dlen.ctypes.data_as(C.c_void_p),
        score.ctypes.data_as(C.c_void_p)), 'asr_ctc_beam')
    return [dec[n, :dlen[n]].tolist() for n in range(int(N))], score


def edit_distance_host(hyps, truths):
    """Lists of int lists -> per-sample normalised Levenshtein (numpy float32)."""
    lib = L.load()
    N = len(hyps)

    def pack(seqs):
        ld = max([len(s) for s in seqs] + [1])
        a = np.zeros((N, ld), np.int32)
        ln = np.zeros(N, np.int32)
        for i, s in enumerate(seqs):
            a[i, :len(s)] = s
            ln[i] = len(s)
        return a, ln, ld

    h, hl, hld = pack(hyps)
    t, tl, tld = pack(truths)
    out = np.empty(N, np.float32)
    L.check(lib.asr_edit_distance(
        h.ctypes.data_as(C.c_void_p), hl.ctypes.data_as(C.c_void_p), hld,
        t.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p), tld, N,
        out.ctypes.data_as(C.c_void_p)), 'asr_edit_distance')
    return out


# --------------------------------------------------------------------------- optimiser
def make_segments(entries, device):
    """entries: list of (offset, length, l2) -> device buffer of asr_segment."""
    arr = (L.Segment * len(entries))()
    for i, (off, ln, l2) in enumerate(entries):
        arr[i].offset, arr[i].len, arr[i].l2, arr[i].reserved = int(off), int(ln), float(l2), 0.0
    raw = np.frombuffer(memoryview(arr), dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(device), len(entries)


def grad_norm(params, grads, segs, n_seg, norm_out):
    lib = L.load()
    n = params.numel()
    nbytes = lib.asr_optim_workspace_bytes(n)
    ws = WS.get('optim', nbytes, params.device)
    L.check(lib.asr_grad_norm(_ptr(params), _ptr(grads), n, _ptr(segs), n_seg, _ptr(norm_out),
                              _ptr(ws), nbytes, _stream()), 'asr_grad_norm')


def adam_step(params, grads, m, v, segs, n_seg, norm, clipnorm, lr, step, beta1=0.9,
              beta2=0.999, eps=1e-8):
    L.check(L.load().asr_adam_step(_ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel(),
                                   _ptr(segs), n_seg, _ptr(norm), float(clipnorm), float(lr),
                                   float(beta1), float(beta2), float(eps), int(step),
                                   _stream()), 'asr_adam_step')


def clip_adam_step(params, grads, m, v, segs, n_seg, norm_out, clipnorm, lr, step, beta1=0.9,
                   beta2=0.999, eps=1e-8):
    """Global norm (-> norm_out, two float64) + clipped Adam update in one library call."""
    lib = L.load()
    n = params.numel()
    nbytes = lib.asr_optim_workspace_bytes(n)
    ws = WS.get('optim', nbytes, params.device)
    L.check(lib.asr_clip_adam_step(_ptr(params), _ptr(grads), _ptr(m), _ptr(v), n, _ptr(segs),
                                   n_seg, _ptr(norm_out), float(clipnorm), float(lr),
                                   float(beta1), float(beta2), float(eps), int(step), _ptr(ws),
                                   nbytes, _stream()), 'asr_clip_adam_step')


def optim_guard(norm, device, flags=None):
    """Vetoes the update that follows if a persistent recurrent kernel has flagged a timeout;
    device-side only.  flags=None: the sticky words at the head of this process' lstm_fwd /
    lstm_bwd workspaces; data parallel: a 2-element device tensor holding the all-reduced
    flags (any non-zero bit pattern vetoes), so every rank skips the same update."""
    if flags is None:
        a, b = WS.get('lstm_fwd', 0, device), WS.get('lstm_bwd', 0, device)
        pa, pb = _ptr(a), _ptr(b)
    else:
        assert flags.numel() >= 2 and flags.element_size() == 4 and flags.is_contiguous()
        pa, pb = C.c_void_p(flags.data_ptr()), C.c_void_p(flags.data_ptr() + 4)
    L.check(L.load().asr_optim_guard(_ptr(norm), pa, pb, _stream()), 'asr_optim_guard')
    # the SimpleRNN workspaces' words (own process) / slots 2, 3 (all-reduced), where present
    if flags is None and _rnn_ran(device):
        pa, pb = [_ptr(WS.get(name, 0, device)) for name in RNN_WS]
    elif flags is not None and flags.numel() >= 4:
        pa, pb = C.c_void_p(flags.data_ptr() + 8), C.c_void_p(flags.data_ptr() + 12)
    else:
        return
    L.check(L.load().asr_optim_guard(_ptr(norm), pa, pb, _stream()), 'asr_optim_guard')


def collect_timeout_flags(out, device):
    """out[0:2] (float32, device) <- 1.0 where the forward / BPTT workspace's sticky timeout
    word is set, else 0.0 (asr_timeout_flags): the form that travels through the gradient
    all-reduce."""
    L.check(L.load().asr_timeout_flags(_ptr(WS.get('lstm_fwd', 0, device)),
                                       _ptr(WS.get('lstm_bwd', 0, device)), _ptr(out), _stream()),
            'asr_timeout_flags')
    if _rnn_ran(device) and out.numel() >= 4:      # SimpleRNN words -> out[2:4]
        L.check(L.load().asr_timeout_flags(_ptr(WS.get(RNN_WS[0], 0, device)),
                                           _ptr(WS.get(RNN_WS[1], 0, device)),
                                           C.c_void_p(out.data_ptr() + 8), _stream()),
                'asr_timeout_flags')


def debug_occupy(blocks, lds_bytes, seconds):
    """Tests only: holds `blocks` 256-thread workgroups (lds_bytes of LDS each) on the device
    for `seconds` on the current stream (asr_debug_occupy)."""
    L.check(L.load().asr_debug_occupy(int(blocks), int(lds_bytes), float(seconds), _stream()),
            'asr_debug_occupy')


def clear_timeout_flags(device):
    for name in ('lstm_fwd', 'lstm_bwd') + (RNN_WS if _rnn_ran(device) else ()):
        WS.get(name, 0, device)[:4].zero_()


def clip_sgd_step(params, grads, vel, segs, n_seg, norm_out, clipnorm, lr, momentum=0.9):
    lib = L.load()
    n = params.numel()
    nbytes = lib.asr_optim_workspace_bytes(n)
    ws = WS.get('optim', nbytes, params.device)
    L.check(lib.asr_clip_sgd_step(_ptr(params), _ptr(grads), _ptr(vel), n, _ptr(segs), n_seg,
                                  _ptr(norm_out), float(clipnorm), float(lr), float(momentum),
                                  _ptr(ws), nbytes, _stream()), 'asr_clip_sgd_step')


def sgd_step(params, grads, vel, segs, n_seg, norm, clipnorm, lr, momentum=0.9):
    L.check(L.load().asr_sgd_step(_ptr(params), _ptr(grads), _ptr(vel), params.numel(),
                                  _ptr(segs), n_seg, _ptr(norm), float(clipnorm), float(lr),
                                  float(momentum), _stream()), 'asr_sgd_step')


# --------------------------------------------------------------------------- front-end
def frontend_features(cfg, audio, offsets, lengths, host_lengths, n_pad, tables, t_out):
    """cfg: _lib.FrontendCfg; audio float32 CUDA (concatenated); offsets/lengths
    int32 CUDA; tables: dict(window, mel, mel_range, dct) CUDA tensors.
    Returns (out (t_out, n_pad, F) float32, out_frames int32 (n_utt,))."""
    lib = L.load()
    n_utt = len(host_lengths)
    hl = (C.c_int * n_utt)(*[int(x) for x in host_lengths])
    ffull = lib.asr_frontend_num_feats(C.byref(cfg))
    f_out = ffull * (2 * cfg.num_context + 1)
    max_frames = max(lib.asr_frontend_num_frames(int(x), cfg.frame_len, cfg.frame_step)
                     for x in host_lengths)
    nbytes = lib.asr_frontend_workspace_bytes(C.byref(cfg), n_utt, max_frames)
    ws = WS.get('frontend', nbytes, audio.device)
    out = torch.empty((int(t_out), int(n_pad), f_out), dtype=torch.float32, device=audio.device)
    frames = torch.empty(n_utt, dtype=torch.int32, device=audio.device)
    head = (C.byref(cfg), _ptr(audio), _ptr(offsets), _ptr(lengths), hl, n_utt, int(n_pad),
            _ptr(tables['window']), _ptr(tables['mel']), _ptr(tables['mel_range']))
    tail = (_ptr(out), int(t_out), _ptr(frames), _ptr(ws), nbytes, _stream())
    if cfg.kind == 0:
        L.check(lib.asr_frontend_mfcc_batch(*(head + (_ptr(tables['dct']),) + tail)),
                'asr_frontend_mfcc_batch')
    else:
        L.check(lib.asr_frontend_logfbank_batch(*(head + tail)), 'asr_frontend_logfbank_batch')
    return out, frames


class FrontendStreamState(object):
    """What asr_frontend_stream carries from call to call for ``n_streams`` streams: the device
    state (carry, base-row ring, running statistics, tables) and the host's counts."""

    def __init__(self, cfg, n_streams, tables, device):
        lib = L.load()
        self.cfg, self.n_streams, self.tables = cfg, int(n_streams), tables
        nbytes = lib.asr_frontend_stream_state_bytes(C.byref(cfg), self.n_streams)
        if nbytes == 0:
            raise ValueError('frontend stream: n_streams %d' % self.n_streams)
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.host = (C.c_longlong * lib.asr_frontend_stream_host_ints(self.n_streams))()
        self.reset()

    def reset(self):
        L.check(L.load().asr_frontend_stream_reset(
            C.byref(self.cfg), _ptr(self.state), C.cast(self.host, C.c_void_p), self.n_streams,
            _ptr(self.tables['mel']), _ptr(self.tables['mel_range']), _stream()),
            'asr_frontend_stream_reset')


def frontend_stream(st, audio, ended, ended_host, n_pad, rows):
    """One call of asr_frontend_stream.  st: FrontendStreamState; audio (n_streams, s) float32
    CUDA, s >= 0; ended: int32 CUDA (n_streams,) of -1 / total lengths with its host mirror
    ended_host (a list), or both None; rows: the kept rows the call emits (FrameSchedule).
    Returns (out (rows, n_pad, F) float32, first kept row, one past the last)."""
    lib = L.load()
    cfg, N = st.cfg, st.n_streams
    _check_f32(audio)
    assert audio.dim() == 2 and audio.shape[0] == N
    s = int(audio.shape[1])
    f_out = lib.asr_frontend_num_feats(C.byref(cfg))
    nbytes = lib.asr_frontend_stream_workspace_bytes(C.byref(cfg), N, s)
    ws = WS.get('frontend', nbytes, audio.device)
    out = torch.empty((int(rows), int(n_pad), f_out), dtype=torch.float32, device=audio.device)
    eh = None if ended_host is None else (C.c_int * N)(*[int(e) for e in ended_host])
    lo, hi = C.c_int(0), C.c_int(0)
    t = st.tables
    L.check(lib.asr_frontend_stream(
        C.byref(cfg), _ptr(st.state), C.cast(st.host, C.c_void_p),
        _ptr(audio) if s else None, s, _ptr(ended), eh, N, int(n_pad), _ptr(t['window']),
        _ptr(t['mel']), _ptr(t['mel_range']), _ptr(t.get('dct')), _ptr(out) if rows else None,
        int(rows), C.byref(lo), C.byref(hi), _ptr(ws), nbytes, _stream()), 'asr_frontend_stream')
    return out, lo.value, hi.value


def axpby(a, x, b, y, out=None):
    """out = a * x + b * y over contiguous float32 CUDA tensors of equal size (the residual
    merge of brsmv1 and its gradient); out defaults to a new tensor."""
    _check_f32(x, y, out)
    assert x.numel() == y.numel()
    if out is None:
        out = torch.empty_like(x)
    L.check(L.load().asr_axpby(x.numel(), float(a), _ptr(x), float(b), _ptr(y), _ptr(out),
                               _stream()), 'asr_axpby')
    return out


# --------------------------------------------------------------------------- LN cell
def _lstm_ln_args(T, n_pad, H, U, cellp, wx, uh, y, cell, gates, has_mi, mask_u=None,
                  zone_c=None, zone_h=None, dy=None, duh=None, dwx=None, dparams=None):
    a = L.LstmLnArgs()
    a.T, a.n_pad, a.H, a.has_mi = int(T), int(n_pad), int(H), int(bool(has_mi))
    for name, t in (('U', U), ('mask_u', mask_u), ('cellp', cellp), ('zone_c', zone_c),
                    ('zone_h', zone_h), ('wx', wx), ('uh', uh), ('y', y), ('cell', cell),
                    ('gates', gates), ('dy', dy), ('duh', duh), ('dwx', dwx),
                    ('dparams', dparams)):
        setattr(a, name, t.data_ptr() if t is not None else None)
    return a


def lstm_ln_seq_fwd(wx, U, cellp, uh, y, cell, gates, T, n_pad, H, has_mi=False, mask_u=None,
                    zone_c=None, zone_h=None, act=0):
    """Layer-normalised cell, forward over the whole sequence (include/asr_hip.h K5-LN)."""
    _check_f32(wx, U, cellp, uh, y, cell, gates, mask_u, zone_c, zone_h)
    a = _lstm_ln_args(T, n_pad, H, U, cellp, wx, uh, y, cell, gates, has_mi, mask_u, zone_c,
                      zone_h)
    a.activation = activation_id(act)
    L.check(L.load().asr_lstm_ln_seq_fwd(C.byref(a), _stream()), 'asr_lstm_ln_seq_fwd')


def lstm_ln_seq_bwd(dy, wx, U, cellp, uh, y, cell, gates, duh, dwx, dparams, T, n_pad, H,
                    has_mi=False, mask_u=None, zone_c=None, zone_h=None, act=0):
    _check_f32(dy, wx, U, cellp, uh, y, cell, gates, duh, dwx, dparams, mask_u, zone_c, zone_h)
    a = _lstm_ln_args(T, n_pad, H, U, cellp, wx, uh, y, cell, gates, has_mi, mask_u, zone_c,
                      zone_h, dy=dy, duh=duh, dwx=dwx, dparams=dparams)
    a.activation = activation_id(act)
    lib = L.load()
    nbytes = lib.asr_lstm_ln_workspace_bytes(C.byref(a))
    ws = WS.get('lstm_ln', nbytes, dy.device)
    L.check(lib.asr_lstm_ln_seq_bwd(C.byref(a), _ptr(ws), nbytes, _stream()),
            'asr_lstm_ln_seq_bwd')


# --------------------------------------------------------------------------- packed operands
class HlPlanes(object):
    """The two fp16 planes (hi, lo) of a matrix with ``ld`` reduction indices per row,
    interleaved in groups of 16 -- ``hl[row, g, 0]`` = hi[16g:16g+16], ``hl[row, g, 1]`` = lo --
    so that a 32-deep slab of a row is one 128-byte line; plus the device float holding the
    power-of-two scale they were packed with (include/asr_hip.h, asr_pack_hl)."""

    def __init__(self, rows, k, device):
        self.rows, self.k = int(rows), int(k)
        self.ld = (self.k + 31) // 32 * 32
        self.hl = torch.empty((self.rows, self.ld // 16, 2, 16), dtype=torch.float16,
                              device=device)
        self.scale = torch.ones(1, dtype=torch.float32, device=device)

    @property
    def hi(self):
        """(rows, ld) view-copy of the hi plane (tests / debugging)."""
        return self.hl[:, :, 0, :].reshape(self.rows, self.ld)

    @property
    def lo(self):
        return self.hl[:, :, 1, :].reshape(self.rows, self.ld)

    def ptr(self, row=0, k=0):
        """Address of (row, reduction index k); k a multiple of 16."""
        assert k % 16 == 0
        return self.hl.data_ptr() + 2 * (int(row) * 2 * self.ld + (int(k) // 16) * 32)


def pack_hl(src, rows, cols, ld=None, src_off=0, mask=None, mask_period=0, absmax=None,
            r=None, c=None, mask2=None, r2=None):
    """src (rows, cols) float32 (row stride ld, element offset src_off) [* mask[(row % period)]]
    -> r planes (rows, cols as K) and / or c planes (cols, rows as K); both get the same scale.
    mask2 / r2: a second set of row planes of the same source under another mask, written in the
    same pass (the source is read once)."""
    lib = L.load()
    a = L.PackArgs()
    a.src = src.data_ptr() + 4 * int(src_off)
    a.rows, a.cols, a.ld = int(rows), int(cols), int(ld if ld is not None else cols)
    a.mask = mask.data_ptr() if mask is not None else None
    a.mask_period = int(mask_period)
    a.mask_ld = int(mask.shape[-1]) if mask is not None else 0
    a.absmax = absmax.data_ptr() if absmax is not None else None
    first = r if r is not None else c
    a.scale_out = first.scale.data_ptr()
    if r is not None:
        assert r.rows >= rows and r.k == cols
        a.r_hl, a.ldk_r = r.hl.data_ptr(), r.ld
    if c is not None:
        assert c.rows >= cols and c.k == rows
        a.c_hl, a.ldk_c = c.hl.data_ptr(), c.ld
    if r2 is not None:
        assert r is not None and mask is not None and mask2 is not None
        assert r2.rows >= rows and r2.k == cols and mask2.shape[-1] == mask.shape[-1]
        a.mask2, a.r2_hl = mask2.data_ptr(), r2.hl.data_ptr()
    L.check(lib.asr_pack_hl(C.byref(a), _stream()), 'asr_pack_hl')
    if r2 is not None:
        r2.scale = r.scale                # one scale for both sets
    if r is not None and c is not None:
        c.scale = r.scale               # one scale for both orientations
    return r, c


def gemm_hl(A, B, Cm, M, N, K, a_row=0, a_k=0, b_row=0, b_k=0, c_off=0, ldc=None, alpha=1.0,
            beta=0.0, bias=None, c_scale=None, c_scale_period=0, split_k=0, ws_name='gemm',
            tile=0, k_major=False, a_seg_k=0, a_seg_rows=None, batch_rows=None):
    """C[M,N] (float32 storage Cm, element offset c_off) = alpha * A @ B^T (+bias)(*c_scale)
    + beta*C from packed planes: A rows [a_row, a_row+M), reduction range [a_k, a_k+K) of its
    planes; B rows [b_row, b_row+N), range [b_k, b_k+K).
    k_major: C = alpha * A^T @ B from planes whose ROWS are the reduction index: A plane rows
    [a_row, a_row+K), columns [a_k, a_k+M); B rows [b_row, b_row+K), columns [b_k, b_k+N)."""
    lib = L.load()
    g = L.GemmHlArgs()
    g.M, g.N, g.K = int(M), int(N), int(K)
    g.a_hl, g.lda = A.ptr(a_row, a_k), A.ld
    g.b_hl, g.ldb = B.ptr(b_row, b_k), B.ld
    g.a_scale, g.b_scale = A.scale.data_ptr(), B.scale.data_ptr()
    g.C = Cm.data_ptr() + 4 * int(c_off)
    g.ldc = int(ldc if ldc is not None else N)
    g.alpha, g.beta = float(alpha), float(beta)
    g.bias = bias.data_ptr() if bias is not None else None
    g.c_scale = c_scale.data_ptr() if c_scale is not None else None
    g.c_scale_period = int(c_scale_period)
    g.c_scale_ld = int(c_scale.shape[-1]) if c_scale is not None else 0
    g.split_k = _resolve_split_hl(split_k, M, N, K, tile,
                                  len(batch_rows) if batch_rows is not None else 1)
    g.tile = int(tile)
    g.k_major = 1 if k_major else 0
    if batch_rows is not None:      # k_major batch sharing B: C_b = A_b^T B, rows b*M.. of Cm
        g.batch = len(batch_rows)
        for i, r in enumerate(batch_rows):
            g.a_batch_row[i] = int(r)
    if a_seg_k:         # segmented reduction range of A (include/asr_hip.h): K = len(rows) * a_seg_k
        g.a_seg_k = int(a_seg_k)
        for i, r in enumerate(a_seg_rows):
            g.a_seg_row[i] = int(r)
    nbytes = lib.asr_gemm_hl_workspace_bytes(C.byref(g))
    ws = WS.get(ws_name, nbytes, Cm.device) if nbytes else None
    L.check(lib.asr_gemm_hl(C.byref(g), _ptr(ws), nbytes, _stream()), 'asr_gemm_hl')


# --------------------------------------------------------------------------- conv front-end
class Conv2d(object):
    """One layer of the 2-D convolution front-end (K13, include/asr_hip.h asr_conv2d_*) on
    time-major slabs: x (T_in, n_pad, F_in * C_in) -> y (T_out, n_pad, F_out * C_out),
    'same' padding, strides (st, sf), clipped ReLU.  Owns its workspace (the packed planes of x
    and of dz live there between the forward and the backward calls of a step)."""

    def __init__(self, T_in, n_pad, F_in, C_in, C_out, kt, kf, st, sf, clip, device):
        lib = L.load()
        a = self.args = L.Conv2dArgs()
        a.T_in, a.n_pad, a.F_in, a.C_in = int(T_in), int(n_pad), int(F_in), int(C_in)
        a.C_out, a.kt, a.kf, a.st, a.sf = int(C_out), int(kt), int(kf), int(st), int(sf)
        a.clip = float(clip)
        t, f = C.c_int(), C.c_int()
        L.check(lib.asr_conv2d_out_shape(C.byref(a), C.byref(t), C.byref(f)), 'asr_conv2d_out_shape')
        self.T_out, self.F_out = t.value, f.value
        self.ws_bytes = lib.asr_conv2d_workspace_bytes(C.byref(a))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.device = device

    def _call(self, fn, name, **ptrs):
        a = self.args
        for k in ('x', 'W', 'bias', 'z', 'y', 'dy', 'dx', 'dW', 'db', 'x_absmax'):
            t = ptrs.get(k)
            setattr(a, k, t.data_ptr() if t is not None else None)
        a.reuse_x, a.reuse_dz = int(ptrs.get('reuse_x', 0)), int(ptrs.get('reuse_dz', 0))
        L.check(fn(C.byref(a), _ptr(self.ws), self.ws_bytes, _stream()), name)

    def fwd(self, x, W, bias, z, y, x_absmax=None):
        """z=None (clip > 0): the clipped ReLU is applied in the GEMM epilogue and only y is
        written -- pass y as `z` to dgrad / wgrad then (the mask 0 < z < clip reads the same
        from y).  x_absmax: 1-element device tensor >= max|x| (skips the measuring pass)."""
        _check_f32(x, W, bias, z, y, x_absmax)
        self._call(L.load().asr_conv2d_fwd, 'asr_conv2d_fwd', x=x, W=W, bias=bias, z=z, y=y,
                   x_absmax=x_absmax)
        return y

    def dgrad(self, dy, z, W, dx, reuse_dz=False):
        _check_f32(dy, z, W, dx)
        self._call(L.load().asr_conv2d_dgrad, 'asr_conv2d_dgrad', dy=dy, z=z, W=W, dx=dx,
                   reuse_dz=reuse_dz)
        return dx

    def wgrad(self, x, dy, z, dW, db, reuse_x=False, reuse_dz=False, x_absmax=None):
        _check_f32(x, dy, z, dW, db, x_absmax)
        self._call(L.load().asr_conv2d_wgrad, 'asr_conv2d_wgrad', x=x, dy=dy, z=z, dW=dW, db=db,
                   reuse_x=reuse_x, reuse_dz=reuse_dz, x_absmax=x_absmax)


# --------------------------------------------------------------------------- random streams
def dropout_masks(out, p, scale, seed, stream_id, step):
    """out (any shape, contiguous float32) <- keep mask of the stream (seed, stream_id, step):
    scale where u >= p, else 0 (include/asr_hip.h K12)."""
    _check_f32(out)
    L.check(L.load().asr_dropout_masks(_ptr(out), out.numel(), float(p), float(scale),
                                       int(seed) & (2 ** 64 - 1), int(stream_id), int(step),
                                       _stream()), 'asr_dropout_masks')
    return out


def dropout_apply(x, out, mask_out, p, scale, seed, stream_id, step):
    _check_f32(x, out, mask_out)
    L.check(L.load().asr_dropout_apply(_ptr(x), _ptr(out), _ptr(mask_out), x.numel(), float(p),
                                       float(scale), int(seed) & (2 ** 64 - 1), int(stream_id),
                                       int(step), _stream()), 'asr_dropout_apply')
    return out


def gaussian_noise(x, out, sigma, seed, stream_id, step):
    """out = x + sigma * N(0, 1) (x may be None: pure noise)."""
    _check_f32(x, out)
    L.check(L.load().asr_gaussian_noise(_ptr(x), _ptr(out), out.numel(), float(sigma),
                                        int(seed) & (2 ** 64 - 1), int(stream_id), int(step),
                                        _stream()), 'asr_gaussian_noise')
    return out


SPECAUG_MAX_MASKS = 64    # frequency + time masks of one asr_specaug_apply call


def specaug_check(time_warp, freq_masks, freq_width, time_masks, time_width, time_ratio):
    """The limits of asr_specaug_apply on a policy (csrc/specaug.hip), as a ValueError: what the
    SpecAugment layer and the engine's stage refuse when the model is built."""
    ints = dict(time_warp=time_warp, freq_masks=freq_masks, freq_width=freq_width,
                time_masks=time_masks, time_width=time_width)
    for k, v in ints.items():
        if isinstance(v, bool) or int(v) != v or v < 0 or v >= 2 ** 31:
            raise ValueError('SpecAugment: %s %r (a non-negative integer)' % (k, v))
    if freq_masks + time_masks > SPECAUG_MAX_MASKS:
        raise ValueError('SpecAugment: %d frequency + %d time masks (at most %d together)'
                         % (freq_masks, time_masks, SPECAUG_MAX_MASKS))
    if not 0.0 <= float(time_ratio) <= 1.0:
        raise ValueError('SpecAugment: time_ratio %r (in [0, 1])' % (time_ratio,))


def specaug_params_len(freq_masks, time_masks):
    """int32 words per sample of asr_specaug_apply's params_out: (c, c', f, f0, ..., tau, t0, ...)."""
    return 2 + 2 * (int(freq_masks) + int(time_masks))


def specaug_apply(x, out, N, F, seed, stream_id, step, lens=None, time_warp=0, freq_masks=2,
                  freq_width=27, time_masks=10, time_width=0, time_ratio=0.05, mask_value=0.0,
                  params_out=None):
    """SpecAugment of the (T, n_pad, ld) slab x into out (another buffer) on the stream (seed,
    stream_id, step): include/asr_hip.h K23.  N real samples of F <= ld real columns; lens: device
    int32 (N) lengths on x's time axis or None (every frame); params_out: device int32
    (N, specaug_params_len(...)) or None."""
    _check_f32(x, out)
    T, n_pad, ld = x.shape
    assert out.shape == x.shape
    for t, n in ((lens, N), (params_out, N * specaug_params_len(freq_masks, time_masks))):
        if t is not None:
            assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= n
    L.check(L.load().asr_specaug_apply(
        _ptr(x), _ptr(out), _ptr(lens), int(T), int(N), int(n_pad), int(F), int(ld),
        int(time_warp), int(freq_masks), int(freq_width), int(time_masks), int(time_width),
        float(time_ratio), float(mask_value), int(seed) & (2 ** 64 - 1), int(stream_id), int(step),
        _ptr(params_out), _stream()), 'asr_specaug_apply')
    return out


def random_words(n, seed, stream_id, step, device):
    out = torch.empty(int(n), dtype=torch.int32, device=device)
    L.check(L.load().asr_random_words(_ptr(out), int(n), int(seed) & (2 ** 64 - 1),
                                      int(stream_id), int(step), _stream()), 'asr_random_words')
    return out


def mul(x, y, out=None):
    _check_f32(x, y, out)
    assert x.numel() == y.numel()
    if out is None:
        out = torch.empty_like(x)
    L.check(L.load().asr_mul(x.numel(), _ptr(x), _ptr(y), _ptr(out), _stream()), 'asr_mul')
    return out
