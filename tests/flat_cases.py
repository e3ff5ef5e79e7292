"""The case table of the flat element-wise and reduction kernels: the optimiser (csrc/optim.hip),
asr_axpby, asr_mul and the Philox kernels (csrc/random.hip), asr_activation_fwd/_bwd
(csrc/rnn.hip), swish / GLU (csrc/dwconv.hip), asr_absmax and asr_colsum (csrc/pack.hip).

They all have one shape: a launch capped at a fixed number of workgroups, a grid-stride loop, a
16-byte fast path and a scalar tail.  GEOMETRY restates each launch (the comment names the line it
is read from); the sizes are derived from it, the smallest n of every class at which such a kernel
can go wrong.  tests/flat_kernel_model.py walks the indices of every case on the CPU
(tests/test_flat_cases_host.py: the table is sharp), tests/test_gpu_flat.py runs the kernels."""
import numpy as np

THREADS = 256

# blocks: the cap on the grid; per_thread: elements of one thread and trip
GEOMETRY = {
    # random.hip launch(): blocks = ((n + 3) / 4 + 255) / 256, capped at 2048; one Philox block of
    # four values per thread and trip
    'random': dict(blocks=2048, per_thread=4),
    # random.hip asr_mul(), optim.hip asr_axpby(): (n / 4 + 255) / 256 in [1, 4096]
    'mul': dict(blocks=4096, per_thread=4),
    'axpby': dict(blocks=4096, per_thread=4),
    # dwconv.hip ew_blocks(n / 4): in [1, 4096]
    'swish': dict(blocks=4096, per_thread=4),
    # rnn.hip asr_activation_fwd/_bwd(): (n + 255) / 256 capped at 4096, one element per thread
    'activation': dict(blocks=4096, per_thread=1),
    # dwconv.hip ew_blocks(rows * (ld / 4)): one item = four columns of a row
    'glu': dict(blocks=4096, per_thread=1),
    # optim.hip grid_for(): (n + 255) / 256 in [1, 2048], one element per thread
    'adam': dict(blocks=2048, per_thread=1),
    'sgd': dict(blocks=2048, per_thread=1),
    # optim.hip asr_grad_norm(): grid_for(n) capped at kNormBlocks = 1024; a workgroup owns one
    # chunk (a multiple of 2048), a trip of its 256 threads is two float4 groups 1024 apart
    'norm': dict(blocks=1024, per_thread=8),
    # pack.hip asr_absmax(): (n / 4 + 255) / 256 in [1, 256]
    'absmax': dict(blocks=256, per_thread=4),
}

NORM_TRIP, NORM_HALF = 2048, 1024
COLSUM_ROWS, COLSUM_MAX_SLICES, COLSUM_UNROLL = 128, 256, 16     # pack.hip colsum_slices()


def cap(kernel):
    """Elements (GLU: items) one full grid covers before the grid-stride loop wraps."""
    g = GEOMETRY[kernel]
    return g['blocks'] * THREADS * g['per_thread']


RAGGED = 4 * 256 * 3        # three workgroups of float4 groups: the suite's 4 * 256 * 3 + 5 style


def sizes(kernel):
    """n = 1; 2, 3; n % 4 in {1, 2, 3} just above a multiple of 4 (more than one workgroup); one
    full grid exactly; one full grid + a ragged second trip + a tail.  The norm also one below,
    at and one above 1024 * 2048, where its chunk grows from one trip to two."""
    c = cap(kernel)
    out = [1, 2, 3, RAGGED + 1, RAGGED + 2, RAGGED + 3, c, c + RAGGED + 5]
    if kernel == 'norm':
        out += [c - 1, c + 1]
    return sorted(set(out))


# ------------------------------------------------------------------------------------- GLU
# (rows, C, ld_in, ld_out): the forward pass has rows * ld_out / 4 items, the backward pass
# rows * ld_in / 4.  The narrowest rows reach the cap with the fewest floats: 8 per row.
GLU_CASES = [
    (1, 4, 8, 4),
    (3, 8, 20, 12),                                   # zero columns behind C and behind 2 C
    (cap('glu') // 2, 4, 8, 4),                       # backward: one full grid exactly
    (cap('glu'), 4, 8, 4),                            # forward: one full grid; backward: two
    (cap('glu') + 3 * 256 + 5, 4, 8, 4),              # both wrap into a ragged trip
]


def glu_items(rows, C, ld_in, ld_out):
    return rows * (ld_out // 4), rows * (ld_in // 4)


# ------------------------------------------------------------------------------------- colsum
COLSUM_M = [1, 4, 127, 129, 2048 + 130, 33000]
COLSUM_N = [1, 64, 70, 160]
COLSUM_BETA = [0.0, 1.0, 0.5]
# (ldx, x_off) as multiples of N: the plain matrix, and the last third of a (M, 3 N) one
COLSUM_LD = [(1, 0), (3, 2)]


def colsum_slices(M):
    return max(1, min(COLSUM_MAX_SLICES, -(-M // COLSUM_ROWS)))


def colsum_rows_per_slice(M):
    rs = colsum_slices(M)
    return -(-M // rs)


assert colsum_slices(127) == 1 and colsum_slices(129) == 2
assert colsum_slices(2048 + 130) > COLSUM_UNROLL and colsum_slices(2048 + 130) % COLSUM_UNROLL
assert colsum_slices(33000) == COLSUM_MAX_SLICES and colsum_rows_per_slice(33000) > COLSUM_ROWS


# ------------------------------------------------------------------------------------- norm
def norm_blocks(n):
    """Workgroups of norm_partial_kernel (optim.hip asr_grad_norm)."""
    return max(1, min(GEOMETRY['norm']['blocks'], -(-n // THREADS)))


def norm_chunk(n):
    """Elements of one workgroup: ceil(n / blocks) rounded up to whole trips."""
    per = -(-n // norm_blocks(n))
    return -(-per // NORM_TRIP) * NORM_TRIP


assert norm_chunk(cap('norm')) == NORM_TRIP and norm_chunk(cap('norm') + 1) == 2 * NORM_TRIP

# the sizes at which the optimiser runs its layouts: the update kernels' wrapping size (the norm
# has chunk == trip there) and the norm's (chunk == two trips)
OPTIM_N = cap('adam') + RAGGED + 5
NORM_N = cap('norm') + RAGGED + 5
L2 = 2.0 ** -7              # a power of two: the probe case's sums are exact


def _segments(n, bounds, l2_of):
    """Boundaries (first elements of the segments after the first) -> [(offset, len, l2)]."""
    offs = [0] + sorted(set(int(b) for b in bounds if 0 < b < n))
    ends = offs[1:] + [n]
    return [(o, e - o, l2_of(i)) for i, (o, e) in enumerate(zip(offs, ends))]


def layouts(n):
    """name -> [(offset, len, l2)] covering [0, n).  'edges': boundaries inside a float4 group, at
    +-1 around a 1024 half-trip, a 2048 trip and a chunk boundary (first, a middle and the last
    workgroup that has elements) and next to the end, l2 alternating between 0 and L2.  'single':
    one segment.  'many': 400 segments, the first 300 one to seven elements long (a thread of
    the norm kernel crosses hundreds of them between its two float4 groups)."""
    chunk = norm_chunk(n)
    last = (n - 1) // chunk
    edges = [5, 6, 4 * 300 + 2]
    for base in sorted({0, chunk, (last // 2) * chunk, last * chunk}):
        for d in (NORM_HALF, NORM_TRIP, chunk, chunk + NORM_HALF):
            edges += [base + d - 1, base + d, base + d + 1]
    edges += [n - 2, n - 1]
    alt = lambda i: L2 if i % 2 else 0.0
    out = {'edges': _segments(n, edges, alt),
           'single': _segments(n, [], lambda i: L2)}
    many, pos = [], 0
    for i in range(300):
        pos += 1 + i % 7
        many.append(pos)
    step = (n - pos) // 100
    many += [pos + k * step + (k % 5) for k in range(1, 100)]
    out['many'] = _segments(n, many, alt)
    return out


def norm_cases():
    """(n, layout): every size of the norm with the edge layout (one segment where n leaves no
    room for a boundary, and at the cap), the 400-segment layout at the two sizes the optimiser
    tests run."""
    out = [(1, 'single'), (cap('norm'), 'single')]
    out += [(n, 'edges') for n in sorted(set(sizes('norm') + [OPTIM_N])) if n > 1]
    return out + [(OPTIM_N, 'many'), (NORM_N, 'many')]


def update_cases(kernel):
    """(n, layout) of adam / sgd: every size with one segment, the layouts at the wrapping size."""
    return [(n, 'single') for n in sizes(kernel)] + [(OPTIM_N, 'edges'), (OPTIM_N, 'many')]


def l2_vector(segs, n):
    v = np.zeros(n, np.float32)
    for o, ln, l2 in segs:
        v[o:o + ln] = l2
    return v


def segment_index(segs, n):
    idx = np.zeros(n, np.int64)
    for i, (o, ln, _) in enumerate(segs):
        idx[o:o + ln] = i
    return idx


def probes(n, segs):
    """Probe positions of the exact norm case: 0, n - 1 and both sides of every trip, half-trip,
    chunk and segment boundary, topped up with a fixed stride of odd elements until their number
    is a perfect square."""
    marks = set(range(NORM_HALF, n, NORM_HALF)) | set(o for o, _, _ in segs[1:])
    pos = {0, n - 1} | marks | set(m - 1 for m in marks)
    pos = set(p for p in pos if 0 <= p < n)
    k = int(np.ceil(np.sqrt(len(pos))))
    extra = 3
    while len(pos) < k * k:
        if extra >= n:                         # tiny n: as many probes as there are elements
            k -= 1
            pos = set(sorted(pos)[:k * k])
            break
        pos.add(extra)
        extra += 37
    return np.array(sorted(pos), np.int64), k


# ------------------------------------------------------------------------------------- absmax
def absmax_positions(n):
    """Where the one maximum is put: first and last element, every tail position, the first and
    last element of the second trip of the grid-stride loop (if there is one)."""
    c = cap('absmax')
    n4 = n // 4 * 4
    pos = {0, n - 1, n4 - 1} | set(range(n4, n))
    if n > c:
        pos |= {c, min(n4, 2 * c) - 1}
    return sorted(p for p in pos if 0 <= p < n)
