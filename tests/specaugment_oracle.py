"""Oracle: SpecAugment as csrc/specaug.hip defines it (include/asr_hip.h K23), restated in NumPy
on oracle.rng.philox4x32_10.  TEST INFRASTRUCTURE ONLY.

The draws are integers (rand(word, K) = the high 32 bits of word * K, by 64-bit products: exact);
the warp's source index and the numerator of its fraction are integers too, the interpolation is
float64.  A pure function of (seed, stream id, step, n): sample n owns the B = 1 + ceil((mF + mT)
/ 2) Philox blocks from n * B on, whatever N is."""
import numpy as np

from oracle.rng import philox4x32_10

DEFAULT = dict(time_warp=0, freq_masks=2, freq_width=27, time_masks=10, time_width=0,
               time_ratio=0.05, mask_value=0.0)


def policy(**kw):
    p = dict(DEFAULT)
    p.update(kw)
    return p


def rand(word, k):
    """An integer in [0, k): the high 32 bits of the 64-bit product word * k."""
    return (int(word) * int(k)) >> 32


def blocks_per_sample(mF, mT):
    return 1 + (mF + mT + 1) // 2


def block_words(n, k, mF, mT, seed, stream_id, step):
    """The four words of block k of sample n."""
    b = n * blocks_per_sample(mF, mT) + k
    w = philox4x32_10([b & 0xFFFFFFFF], [stream_id], [step], [b >> 32],
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return [int(v[0]) for v in w]


def draw(n, length, F, seed, stream_id, step, time_warp=0, freq_masks=2, freq_width=27,
         time_masks=10, time_width=0, time_ratio=0.05, mask_value=0.0):
    """The draws of sample n with `length` valid frames (already clamped to 0 .. T) of F columns:
    {'c', 'cp' (-1, -1: no warp), 'freq': [(f, f0)], 'time': [(tau, t0)]}."""
    mF, mT = int(freq_masks), int(time_masks)
    length = int(length)
    args = (mF, mT, seed, stream_id, step)
    c = cp = -1
    wn = min(int(time_warp), (length - 1) // 2 if length > 0 else 0)
    if wn > 0:
        w = block_words(n, 0, *args)
        c = wn + rand(w[0], length - 2 * wn)
        cp = c + rand(w[1], 2 * wn + 1) - wn
    out = {'c': c, 'cp': cp, 'freq': [], 'time': []}
    for m in range(mF + mT):
        w = block_words(n, 1 + m // 2, *args)
        wa, wb = w[2 * (m % 2)], w[2 * (m % 2) + 1]
        if m < mF:
            f = rand(wa, min(int(freq_width), F) + 1)
            out['freq'].append((f, rand(wb, F - f + 1)))
        else:
            ratio = int(np.floor(np.float32(time_ratio) * np.float32(length)))   # fp32 product
            cap = min(int(time_width) if time_width > 0 else length, ratio, length)
            tau = rand(wa, cap + 1)
            out['time'].append((tau, rand(wb, length - tau + 1)))
    return out


def params_row(d):
    """A draw as the kernel's params_out row: (c, c', f_0, f0_0, ..., tau_0, t0_0, ...)."""
    return [d['c'], d['cp']] + [v for pair in d['freq'] + d['time'] for v in pair]


def warp_positions(length, c, cp):
    """Per output frame t < length of a warped utterance: (i, numerator, denominator) of its
    source position i + numerator / denominator, all integers."""
    out = []
    for t in range(length):
        if t < cp:
            base, num, den = 0, t * c, cp
        else:
            base, num, den = c, (t - cp) * (length - c), length - cp
        out.append((base + num // den, num % den, den))
    return out


def warp(x, length, c, cp):
    """x: (T, F) float64 -> the warped frames [0, length) (frames past them untouched)."""
    y = x.copy()
    if c < 0:
        return y
    for t, (i, r, den) in enumerate(warp_positions(length, c, cp)):
        assert 0 <= i < length
        frac = np.float64(np.float32(r) / np.float32(den))      # the kernel's fp32 fraction
        y[t] = x[i] + frac * (x[min(i + 1, length - 1)] - x[i])
    return y


def mask_of(d, T, F, length):
    """Boolean (T, F): the elements the draws d set to mask_value."""
    m = np.zeros((T, F), bool)
    for f, f0 in d['freq']:
        m[:length, f0:f0 + f] = True
    for tau, t0 in d['time']:
        m[t0:t0 + tau, :] = True
    m[length:] = False
    return m


def apply(x, N, F, lens, seed, stream_id, step, **pol):
    """x: (T, n_pad, ld) float array.  Returns (out float64, masked bool, params (N, 2 + 2 (mF +
    mT)) int64, warped bool (T, n_pad, ld): the elements the warp computed).  Where neither holds,
    out is x itself: frames past the length, rows n >= N, columns col >= F."""
    pol = policy(**pol)
    T, n_pad, ld = x.shape
    out = np.array(x, np.float64)
    masked = np.zeros(x.shape, bool)
    warped = np.zeros(x.shape, bool)
    rows = []
    for n in range(N):
        length = T if lens is None else int(min(max(int(lens[n]), 0), T))
        d = draw(n, length, F, seed, stream_id, step, **pol)
        rows.append(params_row(d))
        if d['c'] >= 0:
            out[:, n, :F] = warp(np.array(x[:, n, :F], np.float64), length, d['c'], d['cp'])
            warped[:length, n, :F] = True
        m = mask_of(d, T, F, length)
        out[:, n, :F][m] = pol['mask_value']
        masked[:, n, :F] = m
    width = 2 + 2 * (int(pol['freq_masks']) + int(pol['time_masks']))
    return out, masked, np.asarray(rows, np.int64).reshape(N, width), warped
