"""The index walks of the flat kernels (tests/flat_cases.py names them) as NumPy models: which
elements a launch visits and how often, and for the kernels that look a segment up, which one.
Index-only, no arithmetic: the models show without a GPU, and independently of the kernels'
results, that every case of the table is covered exactly once by the walk as written -- and that
the table is sharp: each seeded defect of DEFECTS breaks at least one case
(tests/test_flat_cases_host.py).

Every model returns (visits, oob): visits[i] = how often element i is read or written, oob = how
many accesses fell outside [0, n).  `defect` selects one deliberate error:

  no_tail        the scalar tail (or the ragged branch) is removed
  le_chunk_end   `<=` for `<` at the end of a thread's range
  short_stride   the grid stride is short by one workgroup
  vec_off_by_one the guard of the 16-byte path admits a group that ends one past the range
  seg_stuck      the segment is not advanced past every boundary (norm: `if` for `while`;
                 update kernels: `<` for `<=` in the search)
  slices_16      colsum's final pass stops after its first unrolled trip of 16 slices
  no_wrap        the grid-stride loop runs once (`if` for `for`): what only a size past the cap sees
"""
import numpy as np

from tests import flat_cases as FC

DEFECTS = ('no_tail', 'le_chunk_end', 'short_stride', 'vec_off_by_one', 'seg_stuck', 'slices_16',
           'no_wrap')
T = FC.THREADS


def _count(n, idx):
    idx = np.asarray(idx, np.int64).reshape(-1)
    ok = (idx >= 0) & (idx < n)
    return np.bincount(idx[ok], minlength=n).astype(np.int64), int((~ok).sum())


def _grid_stride(first_count, total, blocks, defect, le=False):
    """Items i = tid, tid + stride, ... < total (<= total with `le`) of a launch of `blocks`
    workgroups, offset by first_count (the tail loops start at n4 * 4 + tid)."""
    threads = blocks * T
    stride = threads - (T if defect == 'short_stride' else 0)
    if stride <= 0:
        stride = threads
    tid = np.arange(threads, dtype=np.int64) + first_count
    end = total + (1 if le else 0)
    out = []
    while True:
        tid = tid[tid < end]
        if not tid.size:
            break
        out.append(tid)
        if defect == 'no_wrap':
            break
        tid = tid + stride
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def blocks_of(kernel, n):
    """Workgroups the entry point launches (the expressions GEOMETRY's comments name)."""
    cap = FC.GEOMETRY[kernel]['blocks']
    if kernel == 'random':
        items = (n + 3) // 4
    elif kernel in ('mul', 'axpby', 'swish', 'absmax'):
        items = n // 4
    else:
        items = n
    return max(1, min(cap, (items + T - 1) // T))


def vec_tail(kernel, n, defect=None):
    """mul / axpby / swish / absmax: float4 groups i < n / 4, then the tail from n4 * 4 + tid."""
    blocks = blocks_of(kernel, n)
    n4 = n // 4
    le = defect == 'le_chunk_end'
    g = _grid_stride(0, n4, blocks, defect, le)
    idx = [(4 * g[:, None] + np.arange(4)).reshape(-1)]
    if defect != 'no_tail':
        idx.append(_grid_stride(n4 * 4, n, blocks, defect, le))
    return _count(n, np.concatenate(idx))


def random(n, defect=None):
    """random_kernel: Philox blocks b < (n + 3) / 4; a float4 store if e0 + 3 < n, else
    element by element while e0 + j < n."""
    blocks = blocks_of('random', n)
    b = _grid_stride(0, (n + 3) // 4, blocks, defect)
    e0 = 4 * b
    whole = e0 + 3 <= n if defect == 'vec_off_by_one' else e0 + 3 < n
    idx = [(e0[whole][:, None] + np.arange(4)).reshape(-1)]
    if defect != 'no_tail':
        rag = (e0[~whole][:, None] + np.arange(4)).reshape(-1)
        idx.append(rag[rag <= n] if defect == 'le_chunk_end' else rag[rag < n])
    return _count(n, np.concatenate(idx))


def scalar(kernel, n, defect=None):
    """activation fwd / bwd, adam, sgd: one element per thread and trip."""
    return _count(n, _grid_stride(0, n, blocks_of(kernel, n), defect,
                                  defect == 'le_chunk_end'))


def glu(items, defect=None):
    """glu_fwd / glu_bwd: items = rows * (ld / 4) float4 groups, one per thread and trip."""
    return scalar('glu', items, defect)


def search(offsets, idx, defect=None):
    """seg_l2's binary search (optim.hip): the last segment whose offset is <= idx."""
    offsets = np.asarray(offsets, np.int64)
    idx = np.asarray(idx, np.int64)
    lo = np.zeros(idx.shape, np.int64)
    hi = np.full(idx.shape, len(offsets) - 1, np.int64)
    while (lo < hi).any():
        mid = (lo + hi + 1) >> 1
        go = offsets[mid] < idx if defect == 'seg_stuck' else offsets[mid] <= idx
        act = lo < hi
        lo = np.where(act & go, mid, lo)
        hi = np.where(act & ~go, mid - 1, hi)
    return lo


def update(kernel, n, segs, defect=None):
    """adam_kernel / sgd_kernel -> (visits, oob, segment used per element; -1 = never visited)."""
    idx = _grid_stride(0, n, blocks_of(kernel, n), defect, defect == 'le_chunk_end')
    visits, oob = _count(n, idx)
    idx = idx[idx < n]
    used = np.full(n, -1, np.int64)
    used[idx] = search([o for o, _, _ in segs], idx, defect)
    return visits, oob, used


def norm(n, segs, vec=1, defect=None):
    """norm_partial_kernel: workgroup b owns [b * chunk, min(n, (b + 1) * chunk)); thread t walks
    i = b0 + 4 t, + 2048, ... and reads the groups at i and at j = i + 1024 -- as two float4 if
    `vec` and j + 3 < b1, else element by element below b1.  Its segment starts at the binary
    search of its first element and is walked forward, one `while` per element.
    -> (visits, oob, segment used per element)."""
    blocks, chunk = FC.norm_blocks(n), FC.norm_chunk(n)
    offsets = np.array([o for o, _, _ in segs] + [np.iinfo(np.int64).max], np.int64)
    n_seg = len(segs)
    b0 = np.repeat(np.arange(blocks, dtype=np.int64) * chunk, T)
    b1 = np.minimum(b0 + chunk, n)
    first = b0 + 4 * np.tile(np.arange(T, dtype=np.int64), blocks)
    cur = search(offsets[:-1], first)                 # the head search is not a seeded defect
    hits = []
    used = np.full(n, -1, np.int64)
    oob = 0
    le = defect == 'le_chunk_end'
    i = first.copy()
    while True:
        live = i <= b1 if le else i < b1
        if not live.any():
            break
        j = i + FC.NORM_HALF
        if defect == 'vec_off_by_one':
            whole = live & bool(vec) & (j + 3 <= b1)
        else:
            whole = live & bool(vec) & (j + 3 < b1)
        for base in (i, j):
            for k in range(4):
                e = base + k
                inside = e <= b1 if le else e < b1
                take = whole | (live & ~whole & inside & (defect != 'no_tail'))
                ok = take & (e >= 0) & (e < n)
                oob += int((take & ~ok).sum())
                # the forward walk: past every boundary at or below e (`if`: past one at most)
                if defect == 'seg_stuck':
                    cur = np.where(take & (e >= offsets[np.minimum(cur + 1, n_seg)]), cur + 1, cur)
                else:
                    want = np.searchsorted(offsets, np.where(take, e, 0), side='right') - 1
                    cur = np.where(take, np.maximum(cur, want), cur)
                cur = np.minimum(cur, n_seg - 1)
                hits.append(e[ok])
                used[e[ok]] = cur[ok]
        i = i + FC.NORM_TRIP
    return np.bincount(np.concatenate(hits), minlength=n).astype(np.int64), oob, used


def colsum(M, defect=None):
    """colsum_partial_kernel + colsum_final_kernel for one column -> (how often each row reaches
    the result, oob).  Stage 1: slice s owns rows [s rps, min(M, (s + 1) rps)); row phase ry
    walks m = m0 + ry in steps of 8 (rows m and m + 4) while m + 4 < m1, then in steps of 4.
    Stage 2: wave sg takes slices sg, sg + 4, ...: 16 at a time while s + 12 < slices, then one
    at a time."""
    slices, rps = FC.colsum_slices(M), FC.colsum_rows_per_slice(M)
    rows = np.zeros(M, np.int64)
    owner = np.full(M, -1, np.int64)
    oob = 0
    for s in range(slices):
        m0, m1 = s * rps, min(M, (s + 1) * rps)
        for ry in range(4):
            m = m0 + ry
            got = []
            while m + 4 < m1:
                got += [m, m + 4]
                m += 8
            if defect != 'no_tail':
                end = m1 + 1 if defect == 'le_chunk_end' else m1
                while m < end:
                    got.append(m)
                    m += 4
            for r in got:
                if r < M:
                    rows[r] += 1
                    owner[r] = s
                else:
                    oob += 1
    taken = np.zeros(slices, np.int64)
    for sg in range(4):
        s = sg
        while s + 12 < slices:
            for d in (0, 4, 8, 12):
                taken[s + d] += 1
            s += 16
            if defect == 'slices_16':
                s = slices
        while s < slices:
            taken[s] += 1
            s += 4
    return np.where(owner >= 0, rows * taken[np.maximum(owner, 0)], 0), oob
