"""Float64 NumPy oracle of the running (causal) normalisation and of the resumed front-end
(csrc/frontend.hip: fe_finalize_running_kernel, asr_frontend_stream), placed over
oracle.frontend's mfcc_raw / logfbank_raw / postprocess.  TEST INFRASTRUCTURE ONLY.

running_standardize is the definition; extract_running the whole-signal features; ChunkedModel a
model of the chunked front-end that keeps what the device state keeps -- the carry, the sample in
front of it, the sample count, the base rows -- and emits frames by the la rule."""
import numpy as np
from scipy.fftpack import dct as _dct
from scipy.signal.windows import hamming as _hamming

from oracle import frontend as OF

_FB_KEYS = ('fs', 'win_len', 'win_step', 'num_filt', 'nfft', 'low_freq', 'high_freq', 'pre_emph')

# the configurations of the issue: name -> (oracle kind, class name, constructor kwargs)
CONFIGS = {
    'mfcc39': ('mfcc', 'MFCC', {}),
    'mfcc26': ('mfcc', 'MFCC', {'dd': False}),
    'lfb80': ('logfbank', 'LogFbank', {'num_filt': 80}),
    'lfb40_e': ('logfbank', 'LogFbank', {'num_filt': 40, 'append_energy': True}),
    'mfcc39_s2': ('mfcc', 'MFCC', {'stride': 2}),
    'mfcc39_s3': ('mfcc', 'MFCC', {'stride': 3}),
    'mfcc39_nomean': ('mfcc', 'MFCC', {'mean_norm': False}),
    'mfcc39_novar': ('mfcc', 'MFCC', {'var_norm': False}),
}
# samples -> frames 1, 1, 2, 2, 3, 3, 6, 11, 99 at L = 400, S = 160
LENGTHS = (2, 400, 401, 560, 561, 720, 1041, 1999, 16000)
EMPTY_FILTERS_80 = (1, 7)


def signal(n, seed):
    """Seeded Gaussian noise, rounded to float32 (the device sees the same samples)."""
    return np.asarray(np.random.RandomState(seed).randn(n), np.float32).astype(np.float64)


def lookahead(kw, kind):
    d = kw.get('d', kind == 'mfcc')
    dd = kw.get('dd', kind == 'mfcc')
    return 2 * bool(d) + 2 * bool(d and dd)


def running_standardize(feats, mean_norm=True, var_norm=True, eps=1e-8):
    """Welford's recursion per column over the rows of feats, in order."""
    feats = np.asarray(feats, np.float64)
    out = np.empty_like(feats)
    mean = np.zeros(feats.shape[1])
    m2 = np.zeros(feats.shape[1])
    for t in range(feats.shape[0]):
        n = t + 1
        x = feats[t]
        delta = x - mean
        mean = mean + delta / n
        m2 = m2 + delta * (x - mean)
        sd = np.sqrt(m2 / n)
        out[t] = (x - (mean if mean_norm else 0.0)) / ((sd + eps) if var_norm else 1.0)
    return out


def running_sd(feats):
    """sd_t of every row (the running divisor without eps): (T, F)."""
    feats = np.asarray(feats, np.float64)
    return np.stack([np.std(feats[:t + 1], axis=0) for t in range(feats.shape[0])])


def raw(kind, x, **kw):
    """The (base | delta | delta-delta) rows before stride and normalisation."""
    kw = {k: v for k, v in kw.items() if k not in ('stride', 'mean_norm', 'var_norm', 'norm')}
    fn = {'mfcc': OF.mfcc_raw, 'logfbank': OF.logfbank_raw}[kind]
    return fn(np.asarray(x, np.float64), **kw)


def kept(kind, x, **kw):
    return OF.postprocess(raw(kind, x, **kw), kw.get('stride', 1), 0)


def extract_running(kind, x, **kw):
    return running_standardize(kept(kind, x, **kw), kw.get('mean_norm', True),
                               kw.get('var_norm', True), kw.get('eps', 1e-8))


def extract_running_rowwise(kind, x, **kw):
    """extract_running with the per-frame chain applied to one frame at a time: the oracle's own
    pre-emphasis and framing of the WHOLE signal (OF.preemphasis, OF.framesig), its deltas
    (OF.delta) and stride (OF.postprocess), but rfft / filterbank / log / DCT called per row, as
    ChunkedModel calls them.  NumPy's matrix product and vectorised log round a row differently
    by a few ulp depending on how many rows they are given; this form takes that out, so that the
    chunked model can be compared EXACTLY (rows_raw pins it to the matrix form to 1e-12)."""
    m = ChunkedModel(kind, **kw)
    x = np.asarray(x, np.float64)
    frames = OF.framesig(OF.preemphasis(x, m.pre), m.L, m.S, np.ones(m.L))
    feat = np.array([m._frame_row(f) for f in frames])
    if m.d:
        dl = OF.delta(feat, 2)
        feat = np.hstack([feat, dl] + ([OF.delta(dl, 2)] if m.dd else []))
    feat = OF.postprocess(feat, m.stride, 0)
    return feat, running_standardize(feat, kw.get('mean_norm', True), kw.get('var_norm', True),
                                     m.eps)


class ChunkedModel(object):
    """One stream of the chunked front-end in float64.  feed(samples, ended=None) -> new rows."""

    def __init__(self, kind, **kw):
        self.kind, self.kw = kind, dict(kw)
        fb = {k: kw[k] for k in kw if k in _FB_KEYS}
        self.fs = fb.get('fs', 16e3)
        self.L = OF.round_half_up(fb.get('win_len', 0.025) * self.fs)
        self.S = OF.round_half_up(fb.get('win_step', 0.01) * self.fs)
        self.nfft = fb.get('nfft', 512)
        self.pre = fb.get('pre_emph', 0.97)
        self.window = _hamming(self.L)
        self.fbank = OF.get_filterbanks(fb.get('num_filt', 40), self.nfft, self.fs,
                                        fb.get('low_freq', 20), fb.get('high_freq', 7800))
        self.d = kw.get('d', kind == 'mfcc')
        self.dd = self.d and kw.get('dd', kind == 'mfcc')
        self.la = 2 * bool(self.d) + 2 * bool(self.dd)
        self.stride = kw.get('stride', 1)
        self.eps = kw.get('eps', 1e-8)
        self.carry = np.zeros(0)        # samples from frame `len(self.base)` * S on
        self.prev = None                # the sample in front of the carry
        self.seen = 0
        self.base = []                  # base rows of the frames computed
        self.emitted = 0                # frames (unstrided) emitted
        self.kept_rows = 0
        self.mean = self.m2 = None

    def complete(self, s):
        return 0 if s < self.L else 1 + (s - self.L) // self.S

    def _frame_row(self, frame):
        """frame: L pre-emphasised samples (zero-padded) -> one base row."""
        pspec = OF.powspec((frame * self.window)[None, :], self.nfft)
        energy = np.sum(pspec, 1)
        energy = np.where(energy == 0, np.finfo(float).eps, energy)
        feat = np.dot(pspec, self.fbank.T)
        feat = np.log(np.where(feat == 0, np.finfo(float).eps, feat))
        if self.kind == 'mfcc':
            feat = _dct(feat, type=2, axis=1, norm='ortho')[:, :self.kw.get('num_cep', 13)]
            feat = OF.lifter(feat, self.kw.get('cep_lifter', 22))
            if self.kw.get('append_energy', True):
                feat[:, 0] = np.log(energy + self.eps)
        elif self.kw.get('append_energy', False):
            feat = np.hstack([feat, np.log(energy + self.eps)[:, None]])
        return feat[0]

    def _compute(self, upto, pad):
        """Frames len(base) .. upto - 1 off the carry (pad: zero-pad the last one)."""
        while len(self.base) < upto:
            x = self.carry[:self.L]
            first = self.prev is None
            head = x[:1] if first else x[:1] - self.pre * self.prev
            y = np.concatenate([head, x[1:] - self.pre * x[:-1]])
            if len(y) < self.L:
                assert pad
                y = np.concatenate([y, np.zeros(self.L - len(y))])
            self.base.append(self._frame_row(y))
            if len(self.carry) >= self.S:
                self.prev = self.carry[self.S - 1]
            self.carry = self.carry[self.S:]

    @staticmethod
    def _delta(rows, T, f):
        acc = None
        for n in range(-2, 3):
            term = n * rows(min(max(f + n, 0), T - 1))
            acc = term if acc is None else acc + term
        return acc / 10.0

    def _row(self, f, T):
        base = lambda t: self.base[t]
        parts = [base(f)]
        if self.d:
            dl = lambda t: self._delta(base, T, t)
            parts.append(dl(f))
            if self.dd:
                parts.append(self._delta(dl, T, f))
        return np.concatenate(parts)

    def feed(self, samples, ended=None):
        samples = np.asarray(samples, np.float64)
        if ended is not None:
            samples = samples[:max(0, ended - self.seen)]
        self.carry = np.concatenate([self.carry, samples])
        self.seen += len(samples)
        if ended is None:
            self._compute(self.complete(self.seen), False)
            final = max(0, len(self.base) - self.la)
        else:
            assert self.seen == ended
            self._compute(OF.num_frames(ended, self.L, self.S), True)
            final = len(self.base)
        T = len(self.base)
        out = []
        for f in range(self.emitted, final):
            if f % self.stride:
                continue
            assert ended is not None or f + self.la < T
            x = self._row(f, T)
            if self.mean is None:
                self.mean, self.m2 = np.zeros_like(x), np.zeros_like(x)
            self.kept_rows += 1
            delta = x - self.mean
            self.mean = self.mean + delta / self.kept_rows
            self.m2 = self.m2 + delta * (x - self.mean)
            sd = np.sqrt(self.m2 / self.kept_rows)
            out.append((x - (self.mean if self.kw.get('mean_norm', True) else 0.0)) /
                       ((sd + self.eps) if self.kw.get('var_norm', True) else 1.0))
        self.emitted = max(self.emitted, final)
        return np.array(out) if out else np.zeros((0, 0))


def pieces(n, piece):
    """The split of n samples into feeds of ``piece`` samples (None: one feed)."""
    if piece is None:
        return [(0, n)]
    return [(p, min(n, p + piece)) for p in range(0, n, piece)]
