"""CPU: what the entry points of the flat kernels refuse, through the C ABI with pointers nothing
dereferences.  Every refusal is decided on the host before anything is launched, so none of this
needs a device -- and nothing is ever launched with a misaligned pointer."""
import ctypes as C

import pytest

from asr_study_amd._lib import CONSTANTS

ONE, TWO, THREE, FOUR = (C.c_void_p(16 * k) for k in (1, 2, 3, 4))     # aligned, non-NULL
ODD = C.c_void_p(20)                                                   # 4-byte aligned only
ERR_ARG, ERR_WS = CONSTANTS['ASR_ERR_INVALID'], CONSTANTS['ASR_ERR_WORKSPACE']
SEED = (0x1234 << 32) | 0xBEEF


@pytest.fixture(scope='module')
def lib():
    from asr_study_amd import _lib
    return _lib.load()


def _refused(lib, rc, word, code=ERR_ARG):
    assert rc == code, (rc, word)
    assert word in lib.asr_last_error().decode(), (word, lib.asr_last_error())


def test_error_codes_are_the_header_s():
    assert (ERR_ARG, ERR_WS) == (-1, -2)


def test_axpby_and_mul(lib):
    for bad in ((ODD, TWO, THREE), (ONE, ODD, THREE), (ONE, TWO, ODD)):
        _refused(lib, lib.asr_axpby(8, 1.0, bad[0], 1.0, bad[1], bad[2], None), 'alignment')
        _refused(lib, lib.asr_mul(8, bad[0], bad[1], bad[2], None), 'alignment')
    for bad in ((None, TWO, THREE), (ONE, None, THREE), (ONE, TWO, None)):
        _refused(lib, lib.asr_axpby(8, 1.0, bad[0], 1.0, bad[1], bad[2], None), 'axpby')
        _refused(lib, lib.asr_mul(8, bad[0], bad[1], bad[2], None), 'mul')
    for n in (0, -1, -2 ** 40):
        _refused(lib, lib.asr_axpby(n, 1.0, ONE, 1.0, TWO, THREE, None), 'axpby')
        _refused(lib, lib.asr_mul(n, ONE, TWO, THREE, None), 'mul')


def test_random(lib):
    _refused(lib, lib.asr_dropout_masks(ODD, 8, 0.2, 1.25, SEED, 1, 1, None), 'alignment')
    _refused(lib, lib.asr_random_words(ODD, 8, SEED, 1, 1, None), 'alignment')
    _refused(lib, lib.asr_gaussian_noise(None, ODD, 8, 0.5, SEED, 1, 1, None), 'alignment')
    _refused(lib, lib.asr_gaussian_noise(ODD, TWO, 8, 0.5, SEED, 1, 1, None), 'alignment')
    for bad in ((ODD, TWO, THREE), (ONE, ODD, THREE), (ONE, TWO, ODD), (ONE, ODD, None)):
        _refused(lib, lib.asr_dropout_apply(bad[0], bad[1], bad[2], 8, 0.2, 1.25, SEED, 1, 1,
                                            None), 'alignment')
    for n in (0, -1):
        _refused(lib, lib.asr_dropout_masks(ONE, n, 0.2, 1.25, SEED, 1, 1, None), 'random')
        _refused(lib, lib.asr_dropout_apply(ONE, TWO, None, n, 0.2, 1.25, SEED, 1, 1, None),
                 'random')
        _refused(lib, lib.asr_gaussian_noise(ONE, TWO, n, 0.5, SEED, 1, 1, None), 'random')
        _refused(lib, lib.asr_random_words(ONE, n, SEED, 1, 1, None), 'random')
    _refused(lib, lib.asr_dropout_masks(None, 8, 0.2, 1.25, SEED, 1, 1, None), 'random')
    _refused(lib, lib.asr_dropout_apply(None, TWO, None, 8, 0.2, 1.25, SEED, 1, 1, None),
             'dropout_apply')
    for p in (1.0, 1.5, -0.01, float('nan'), float('inf')):            # p outside [0, 1)
        _refused(lib, lib.asr_dropout_masks(ONE, 8, p, 1.0, SEED, 1, 1, None), 'dropout_masks')
        _refused(lib, lib.asr_dropout_apply(ONE, TWO, None, 8, p, 1.0, SEED, 1, 1, None),
                 'dropout_apply')


def test_activation(lib):
    """tanh 0, relu 1, linear 4 and clipped ReLU 7 are what the entry points run.  n = 0 is an
    accepted no-op that returns before the launch, which shows WHICH ids pass the check without
    a device: the clipped ReLU's id is accepted (with any clip), its neighbours are not."""
    for aid in (2, 3, 5, 6, 8, -1, 100):
        for n in (0, 8):
            _refused(lib, lib.asr_activation_fwd(ONE, TWO, n, aid, 0.0, None), 'activation_fwd')
            _refused(lib, lib.asr_activation_bwd(ONE, TWO, THREE, n, aid, 0.0, None),
                     'activation_bwd')
    for aid, clip in ((0, 0.0), (1, 0.0), (4, 0.0), (7, 20.0), (7, 0.0)):
        assert lib.asr_activation_fwd(ONE, TWO, 0, aid, clip, None) == 0, aid
        assert lib.asr_activation_bwd(ONE, TWO, THREE, 0, aid, clip, None) == 0, aid
    for aid in (0, 1, 4, 7):
        _refused(lib, lib.asr_activation_fwd(ONE, TWO, -1, aid, 20.0, None), 'activation_fwd')
        _refused(lib, lib.asr_activation_bwd(ONE, TWO, THREE, -1, aid, 20.0, None),
                 'activation_bwd')
        _refused(lib, lib.asr_activation_fwd(None, TWO, 0, aid, 20.0, None), 'activation_fwd')
        _refused(lib, lib.asr_activation_fwd(ONE, None, 0, aid, 20.0, None), 'activation_fwd')
        for bad in ((None, TWO, THREE), (ONE, None, THREE), (ONE, TWO, None)):
            _refused(lib, lib.asr_activation_bwd(bad[0], bad[1], bad[2], 0, aid, 20.0, None),
                     'activation_bwd')


def test_python_side_activation_ids():
    from asr_study_amd import ops
    assert ops.rnn_activation_id('tanh') == (0, 0.0) and ops.rnn_activation_id('relu') == (1, 0.0)
    assert ops.rnn_activation_id('linear') == (4, 0.0) and ops.rnn_activation_id(None) == (0, 0.0)
    assert ops.rnn_activation_id(('clipped_relu', 20)) == (7, 20.0)
    for act in ('sigmoid', 'hard_sigmoid', 'softsign', 'softplus', 7, ('clipped_relu',)):
        with pytest.raises((NotImplementedError, IndexError)):
            ops.rnn_activation_id(act)


def test_absmax_and_colsum(lib):
    _refused(lib, lib.asr_absmax(ODD, 8, TWO, None), 'aligned')
    _refused(lib, lib.asr_absmax(None, 8, TWO, None), 'absmax')
    _refused(lib, lib.asr_absmax(ONE, 8, None, None), 'absmax')
    for n in (0, -1):
        _refused(lib, lib.asr_absmax(ONE, n, TWO, None), 'absmax')
    big = 1 << 30
    for M, N, ldx in ((4, 8, 7), (4, 8, 0), (0, 8, 8), (-1, 8, 8), (4, 0, 8), (4, -1, 8)):
        _refused(lib, lib.asr_colsum(ONE, M, N, ldx, TWO, 0.0, THREE, big, None), 'colsum')
    for bad in ((None, TWO, THREE), (ONE, None, THREE), (ONE, TWO, None)):
        _refused(lib, lib.asr_colsum(bad[0], 4, 8, 8, bad[1], 0.0, bad[2], big, None), 'colsum')
    # the workspace: one float64 per slice and column, rounded up to 256 bytes
    for M, N, slices in ((1, 1, 1), (129, 70, 2), (2178, 160, 18), (33000, 160, 256)):
        need = lib.asr_colsum_workspace_bytes(M, N)
        assert need == -(-slices * N * 8 // 256) * 256, (M, N, need)
        for ws in (0, need - 1):
            _refused(lib, lib.asr_colsum(ONE, M, N, N, TWO, 0.0, THREE, ws, None), 'workspace',
                     ERR_WS)


def test_optimiser(lib):
    need = lib.asr_optim_workspace_bytes(5138)
    assert need == 1024 * 2 * 8 == lib.asr_optim_workspace_bytes(1 << 22)
    args = (ONE, TWO, 5138, THREE, 4, FOUR, C.c_void_p(80))
    for ws in (0, need - 1):
        _refused(lib, lib.asr_grad_norm(*args, ws, None), 'workspace', ERR_WS)
    for i in (0, 1, 3, 5, 6):                                          # every pointer
        bad = list(args)
        bad[i] = None
        _refused(lib, lib.asr_grad_norm(*bad, need, None), 'grad_norm')
    for n, n_seg in ((0, 4), (-1, 4), (5138, 0), (5138, -1)):
        _refused(lib, lib.asr_grad_norm(ONE, TWO, n, THREE, n_seg, FOUR, C.c_void_p(80), need,
                                        None), 'grad_norm')
    adam = lambda n=5138, n_seg=4, step=1, p=ONE, g=TWO, m=THREE, v=FOUR, s=C.c_void_p(80): \
        lib.asr_adam_step(p, g, m, v, n, s, n_seg, None, 0.0, 1e-3, 0.9, 0.999, 1e-8, step, None)
    for step in (0, -1):                                               # Adam's step counts from 1
        _refused(lib, adam(step=step), 'adam')
    for kw in (dict(n=0), dict(n=-1), dict(n_seg=0), dict(p=None), dict(g=None), dict(m=None),
               dict(v=None), dict(s=None)):
        _refused(lib, adam(**kw), 'adam')
    sgd = lambda n=5138, n_seg=4, p=ONE, g=TWO, v=THREE, s=FOUR: \
        lib.asr_sgd_step(p, g, v, n, s, n_seg, None, 0.0, 1e-2, 0.9, None)
    for kw in (dict(n=0), dict(n=-1), dict(n_seg=0), dict(p=None), dict(g=None), dict(v=None),
               dict(s=None)):
        _refused(lib, sgd(**kw), 'sgd')
    _refused(lib, lib.asr_optim_guard(None, ONE, TWO, None), 'optim_guard')
