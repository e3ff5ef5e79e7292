"""The case table of the audio front-end (csrc/frontend.hip: fe_prepare_kernel, fe_frames_kernel,
fe_finalize_kernel<8|16>, fe_zero_pad_rows_kernel, driven by asr_frontend_features).

GEOMETRY restates the launch shapes the sizes are derived from; CONFIGS are constructor kwargs of
preprocessing.audio.MFCC / LogFbank (oracle.frontend.extract takes the same kwargs) with the output
width, column-block width and last-block width each is in the table for; cases(name) gives the
(n, T, kind) every configuration runs at.  tests/test_frontend_cases_host.py proves on the CPU that
the table reaches what it claims, tests/test_gpu_frontend.py runs the kernels, and
oracle/gen_golden.py pins the oracle to the reference at EDGE_CONFIGS with edge_input()."""
import collections

import numpy as np

from oracle import frontend as OF

NFFT = 512
# fe_frames_kernel: one wave per frame, FRAMES_PER_WAVE frames in a row with a one-frame-ahead
# prefetch, WAVES waves per workgroup
FRAMES_PER_WAVE, WAVES = 4, 4
FRAMES_PER_BLOCK = FRAMES_PER_WAVE * WAVES
# fe_finalize_kernel<CX>: 1024 threads, CX columns per workgroup, 1024 / CX row walkers per
# column; asr_frontend_features takes CX = 16 from f_out >= CX_SWITCH on
FINALIZE_THREADS, CX_SWITCH = 1024, 64
MEL_LANES, MEL_LIMIT = 64, 128              # lanes take filters lane and lane + 64


def cx_of(f_out):
    return 16 if f_out >= CX_SWITCH else 8


def walkers(f_out):
    return FINALIZE_THREADS // cx_of(f_out)


def last_block(f_out):
    """Live columns of the last column block."""
    return (f_out - 1) % cx_of(f_out) + 1


# T = 1..5: the +-2 clamps of the delta window overlap (1, 2), meet (3, 4) and part (5); 4 | 5 is
# also the wave boundary of the frame kernel; 15..17, 31..33: its workgroup boundary; 63..65 and
# 127..129: a row walker of the CX = 16 and of the CX = 8 finalize kernel gains its second trip;
# 257: a third and a fifth trip
LADDER_T = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
# the T that put Ts = ceil(T / stride) on both sides of 63 | 64 | 65 and 127 | 128 | 129
STRIDE_T = {
    1: (),
    2: (125, 126, 127, 128, 129, 130, 253, 254, 255, 256, 257, 258),
    3: (187, 189, 190, 192, 193, 195, 379, 381, 382, 384, 385, 387),
}
WALKER_EDGES = (63, 64, 65, 127, 128, 129)
# the floor of every configuration that does not run the whole ladder: delta clamps (2, 3, 5 and
# 3, 4, 6 through n + 1), a workgroup boundary of the frame kernel (16 | 17), a second walker trip
# of either finalize kernel (65, 66, 129, 130)
SHORT_T = (2, 3, 5, 16, 65, 129)
SIGNAL_T = (17, 65, 129)
SIGNAL_KINDS = ('pcm', 'tone', 'gap', 'silence')
KINDS = ('noise',) + SIGNAL_KINDS
MIN_CONTEXT_T = 16          # standardised configurations with context: see cases()

Config = collections.namedtuple('Config', 'cls kw f_out cx last note')
_RAW = {'mean_norm': False, 'var_norm': False}
_S3C1 = {'append_energy': True, 'd': True, 'dd': True, 'stride': 3, 'num_context': 1}
_S2C2 = {'stride': 2, 'num_context': 2}

CONFIGS = collections.OrderedDict([
    ('mfcc39', Config('MFCC', {}, 39, 8, 7, 'five column blocks, the last with 7 columns')),
    ('mfcc13', Config('MFCC', {'d': False, 'dd': False}, 13, 8, 5, 'no delta passes, blocks 8 + 5')),
    ('mfcc26', Config('MFCC', {'dd': False}, 26, 8, 2, 'delta pass only')),
    ('lfb80', Config('LogFbank', {'num_filt': 80}, 80, 16, 16,
                     'two mel passes, empty filters 1 and 7')),
    ('lfb64', Config('LogFbank', {'num_filt': 64}, 64, 16, 16,
                     'the first CX = 16 width, one exactly full mel pass')),
    ('lfb21_d_dd', Config('LogFbank', {'num_filt': 21, 'd': True, 'dd': True}, 63, 8, 7,
                          'the last CX = 8 width; delta-delta columns whose delta column is '
                          "another workgroup's")),
    ('lfb65', Config('LogFbank', {'num_filt': 65}, 65, 16, 1,
                     'second mel pass with one live lane')),
    ('lfb128_full', Config('LogFbank', {'num_filt': 128, 'low_freq': 0, 'high_freq': 8000},
                           128, 16, 16, 'the num_filt limit; top edge at bin 256')),
    ('lfb41_d_dd_s3c1', Config('LogFbank', dict(_S3C1), 369, 16, 1, '23 * 16 + 1; stride 3')),
    ('mfcc39_s2c2', Config('MFCC', dict(_S2C2), 195, 16, 3, 'the context slots')),
    ('mfcc26x26', Config('MFCC', {'num_filt': 26, 'num_cep': 26, 'cep_lifter': 0,
                                  'append_energy': False}, 78, 16, 14,
                         'DCT width, no lifter, c0 kept')),
    ('mfcc_w512', Config('MFCC', {'win_len': 0.032}, 39, 8, 7, 'frame_len == NFFT')),
    ('mfcc_w320_s80', Config('MFCC', {'win_len': 0.02, 'win_step': 0.005}, 39, 8, 7,
                             'different framing; many frames per sample count')),
    ('mfcc_8k', Config('MFCC', {'fs': 8e3, 'high_freq': 3800}, 39, 8, 7, 'L = 200, S = 80')),
    ('mfcc_pe0', Config('MFCC', {'pre_emph': 0.0}, 39, 8, 7, 'no pre-emphasis')),
    ('mfcc_nomean', Config('MFCC', {'mean_norm': False}, 39, 8, 7, 's_inv alone')),
    ('mfcc_novar', Config('MFCC', {'var_norm': False}, 39, 8, 7, 's_mean alone')),
    ('mfcc39_raw', Config('MFCC', dict(_RAW), 39, 8, 7, 'placement of the deltas at tiny T')),
    ('lfb41_d_dd_s3c1_raw', Config('LogFbank', dict(_S3C1, **_RAW), 369, 16, 1,
                                   'placement of stride and context at tiny T')),
    ('mfcc39_s2c2_raw', Config('MFCC', dict(_S2C2, **_RAW), 195, 16, 3,
                               'placement of stride and context at tiny T')),
])

FULL_LADDER = ('mfcc39', 'lfb80', 'mfcc39_s2c2_raw', 'lfb41_d_dd_s3c1_raw')
SIGNAL_CONFIGS = ('mfcc39', 'lfb80', 'lfb128_full')
# the configurations oracle/gen_golden.py pins to the reference in tests/golden/frontend_edge_*.npz:
# every row whose parameters no frontend_*.npz of the default table has
EDGE_CONFIGS = tuple(n for n in CONFIGS if n not in ('mfcc39', 'mfcc13', 'mfcc26', 'lfb80',
                                                     'mfcc39_s2c2'))


def oracle_kind(name):
    return {'MFCC': 'mfcc', 'LogFbank': 'logfbank'}[CONFIGS[name].cls]


def framing(name):
    """(frame_len, frame_step) of a configuration, as FBank._cfg and the oracle round them."""
    kw = CONFIGS[name].kw
    fs = kw.get('fs', 16e3)
    return (OF.round_half_up(kw.get('win_len', 0.025) * fs),
            OF.round_half_up(kw.get('win_step', 0.01) * fs))


def is_raw(name):
    kw = CONFIGS[name].kw
    return not kw.get('mean_norm', True) and not kw.get('var_norm', True)


def strided(T, stride):
    return -(-T // stride)


def full_len(T, L, S):
    """The length whose last frame, frame T - 1, is exactly full."""
    return L + S * (T - 1)


Case = collections.namedtuple('Case', 'n T kind')


def _pairs(Ts, L, S):
    out = []
    for T in Ts:
        out += [Case(full_len(T, L, S), T, 'noise'), Case(full_len(T, L, S) + 1, T + 1, 'noise')]
    return out


def cases(name):
    """The cases of one configuration: the whole ladder (every T with its exactly-full length and
    that length + 1, n = 2 and n = L - 1) for FULL_LADDER, SHORT_T for the rest; the T of
    STRIDE_T for a strided one; the four other signal kinds at SIGNAL_T for SIGNAL_CONFIGS.

    A standardised configuration with context runs from T = MIN_CONTEXT_T on only: the reference
    casts the stacked features to float32 BEFORE it standardises them and the kernel does not;
    that cast alone moves the reference by up to 9.8e-5 at T = 3..4 and by <= 1.4e-5 from T = 16
    on (measured with oracle/frontend.py), so below that context and stride are checked in their
    raw form.  mfcc_nomean runs from T = 2: at T = 1 the reference divides the un-shifted value by
    0 + eps."""
    c = CONFIGS[name]
    L, S = framing(name)
    stride = c.kw.get('stride', 1)
    out = _pairs(LADDER_T if name in FULL_LADDER else SHORT_T, L, S)
    out += [Case(2, 1, 'noise'), Case(L - 1, 1, 'noise')]
    if name not in FULL_LADDER:
        out.append(Case(L, 1, 'noise'))
    out += [Case(full_len(T, L, S), T, 'noise') for T in STRIDE_T[stride]]
    if name in SIGNAL_CONFIGS:
        out += [Case(full_len(T, L, S), T, kind) for kind in SIGNAL_KINDS for T in SIGNAL_T]
    lo = 1
    if c.kw.get('num_context', 0) > 0 and not is_raw(name):
        lo = MIN_CONTEXT_T
        out += _pairs((16, 31, 64), L, S)
    elif name == 'mfcc_nomean':
        lo = 2
    seen, uniq = set(), []
    for case in out:
        if case.T >= lo and case not in seen:
            seen.add(case)
            uniq.append(case)
    return uniq


# ------------------------------------------------------------------------------------- signals
def f32(x):
    """Rounded to float32 and back: the oracle and the device see the same samples, so what is
    left of their difference is arithmetic."""
    return np.asarray(x, np.float32).astype(np.float64)


def gap_span(L, S):
    """(start, length) of the run of exact zeros of a 'gap' signal: it starts inside frame 2 and
    covers frames 3, 4 and 5 with the sample in front of each (the pre-emphasis reads it)."""
    return 2 * S + S // 2 + 3, L + 3 * S


def zero_frames(x, L, S):
    """The frames of x that are exact zeros after the pre-emphasis."""
    T = OF.num_frames(len(x), L, S)
    pad = np.concatenate([x, np.zeros(max(0, (T - 1) * S + L - len(x)))])
    return [f for f in range(T)
            if not pad[f * S:f * S + L].any() and (f == 0 or pad[f * S - 1] == 0)]


def make_signal(kind, n, seed, L, S, fs=16e3):
    rs = np.random.RandomState(seed)
    if kind == 'noise':
        x = rs.randn(n)
    elif kind == 'pcm':
        x = np.round(3000.0 * rs.randn(n))                  # int16-scale integers
    elif kind == 'tone':
        t = np.arange(n)
        x = (0.5 * np.sin(2 * np.pi * 1000.0 * t / fs) * (0.6 + 0.4 * np.cos(2 * np.pi * t / 3000.0))
             + 1e-2 * rs.randn(n))
    elif kind == 'gap':
        x = rs.randn(n)
        z0, zl = gap_span(L, S)
        assert z0 + zl < n, 'a gap signal needs T >= 16'
        x[z0:z0 + zl] = 0.0
    elif kind == 'silence':
        x = np.zeros(n)
    else:
        raise ValueError(kind)
    return f32(x)


def signal(name, case):
    """The input of a case: seeded by (T, kind)."""
    L, S = framing(name)
    seed = 1000 * case.T + KINDS.index(case.kind)
    return make_signal(case.kind, case.n, seed, L, S, CONFIGS[name].kw.get('fs', 16e3))


def want(name, x):
    """The float64 oracle's features of x."""
    return OF.extract(oracle_kind(name), x, **CONFIGS[name].kw)


# ------------------------------------------------------------------------------------- fixtures
EDGE_SEEDS = (0, 1)
EDGE_GAP_N = 3000


def edge_keys(name):
    """Keys of tests/golden/frontend_edge_<name>.npz: 'n<samples>_s<seed>' (noise) and
    'gap<samples>_s<seed>'."""
    L, S = framing(name)
    ns = (2, 300, L + 2 * S, L + 2 * S + 1, L + 16 * S + 1)
    return (['n%d_s%d' % (n, s) for n in ns for s in EDGE_SEEDS] +
            ['gap%d_s%d' % (EDGE_GAP_N, s) for s in EDGE_SEEDS])


def edge_input(name, key):
    L, S = framing(name)
    head, seed = key.split('_')
    kind, n = ('gap', int(head[3:])) if head.startswith('gap') else ('noise', int(head[1:]))
    return make_signal(kind, n, int(seed[1:]), L, S, CONFIGS[name].kw.get('fs', 16e3))


# ------------------------------------------------------------------------------------- batches
# one ragged batch: the longest utterance is not the first
BATCH_T = (1, 2, 5, 16, 17, 129, 64)
BATCH_CONFIGS = ('mfcc13', 'lfb64', 'lfb21_d_dd', 'mfcc39_s2c2', 'lfb41_d_dd_s3c1')
SHARED_DELTA_CONFIGS = ('lfb21_d_dd', 'lfb41_d_dd_s3c1', 'mfcc39_s2c2')
# (n_utt, n_pad): no padding rows (the zero-pad kernel is skipped), 15 of them, and 45
BATCH_SHAPES = ((1, 1), (16, 16), (17, 32), (3, 48))
T_OUT_DELTAS = (0, 5, -3)


def batch_signals(name, n_utt):
    """n_utt utterances whose frame counts cycle through BATCH_T (one utterance: 129 frames;
    three: 17, 129 and 2); every other one is a sample longer than exactly full."""
    L, S = framing(name)
    Ts = {1: [129], 3: [17, 129, 2]}.get(n_utt) or [BATCH_T[i % len(BATCH_T)] for i in range(n_utt)]
    sigs = []
    for i, T in enumerate(Ts):
        n = full_len(T, L, S) + (i % 2 if T > 1 else 0)
        sigs.append(make_signal('noise', n, 77000 + 100 * i + T, L, S))
    return sigs
