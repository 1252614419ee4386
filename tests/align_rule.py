"""Mel alignment (include/zerovox_amd.h "mel alignment") restated with Python / numpy integers and ONE float64 operation per step.
Two forms that the tests hold equal at small sizes: align_loops, plain loops over Python integers, and align, vectorised over
anti-diagonals.  The vectorised form takes its costs from a float64 matrix product, which is exact: every dot product of rows with
|q'| <= 2046 over at most 256 channels is below 2^31, far below 2^53."""
import math
import os
import re

import numpy as np

F = np.float32
MAX_FRAMES, MAX_MELS, GROUP_CELLS = 4096, 256, 1 << 27
NONE = 3
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zerovox.cpp_amd", "csrc")


def constant(name: str) -> int:
    """an integer constant of csrc/align.h (ALIGN_DP_ROWS, ALIGN_TILE, ...)"""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(_CSRC, "align.h")).read())
    assert m, name
    return int(m.group(1))


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def scale_of(scale) -> float:
    """the resolved scale as float64: 0 means 64"""
    s = float(F(scale))
    return 64.0 if s == 0.0 else s


def quantise(x, scale) -> np.ndarray:
    """f32 rows -> int64, one float64 operation per line"""
    x = np.ascontiguousarray(x, dtype=F)
    y = np.where(np.isfinite(x), x, F(0.0)).astype(np.float64)
    d = y * np.float64(scale_of(scale))
    d = np.minimum(np.maximum(d, -1023.0), 1023.0)
    d = d + np.where(d >= 0.0, 0.5, -0.5)
    return np.trunc(d).astype(np.int64)


def rows(x, scale, normalise) -> np.ndarray:
    """q' [T, M] of one sequence"""
    q = quantise(x, scale)
    if normalise:
        T = q.shape[0]
        s = q.sum(axis=0)
        mean = (2 * s + T) // (2 * T)                     # numpy's // on integers is a true floor
        q = q - mean[None, :]
    return q


def _walk(c, ch, Ta, Tb, scale):
    i, j, L, acc = Ta - 1, Tb - 1, 0, 0.0
    map_a, map_b = np.full(Ta, -1, np.int32), np.full(Tb, -1, np.int32)
    while True:
        acc = acc + math.sqrt(float(int(c[i][j])))
        L += 1
        map_a[i], map_b[j] = j, i
        k = int(ch[i][j])
        if k == NONE:
            break
        if k != 2:
            i -= 1
        if k != 1:
            j -= 1
    assert (i, j) == (0, 0)
    acc = acc / float(L)
    acc = acc / scale_of(scale)
    return L, acc, map_a, map_b


def align_loops(a, b, scale=0.0, normalise=0):
    """plain loops over Python integers -> (total, distance, path_len, map_a, map_b)"""
    qa, qb = rows(a, scale, normalise).tolist(), rows(b, scale, normalise).tolist()
    Ta, Tb = len(qa), len(qb)
    c = [[sum((x - y) ** 2 for x, y in zip(qa[i], qb[j])) for j in range(Tb)] for i in range(Ta)]
    assert max(map(max, c)) < 1 << 32
    D = [[0] * Tb for _ in range(Ta)]
    ch = [[NONE] * Tb for _ in range(Ta)]
    for i in range(Ta):
        for j in range(Tb):
            best, k = 0, NONE
            if i and j:
                best, k = D[i - 1][j - 1], 0
            if i and (k == NONE or D[i - 1][j] < best):
                best, k = D[i - 1][j], 1
            if j and (k == NONE or D[i][j - 1] < best):
                best, k = D[i][j - 1], 2
            D[i][j], ch[i][j] = c[i][j] + best, k
    L, dist, map_a, map_b = _walk(c, ch, Ta, Tb, scale)
    return D[Ta - 1][Tb - 1], dist, L, map_a, map_b


def costs(a, b, scale=0.0, normalise=0) -> np.ndarray:
    """c [Ta, Tb] as int64, from a float64 matrix product (exact)"""
    qa, qb = rows(a, scale, normalise), rows(b, scale, normalise)
    assert max(np.abs(qa).max(), np.abs(qb).max()) <= 2046
    dot = qa.astype(np.float64) @ qb.astype(np.float64).T
    c = (qa * qa).sum(axis=1)[:, None] + (qb * qb).sum(axis=1)[None, :] - 2 * dot.astype(np.int64)
    assert c.min() >= 0 and c.max() < 1 << 32
    return c


def align(a, b, scale=0.0, normalise=0):
    """vectorised over anti-diagonals -> (total, distance, path_len, map_a, map_b)"""
    c = costs(a, b, scale, normalise)
    Ta, Tb = c.shape
    INF = np.int64(1) << 62
    D = np.full((Ta + 1, Tb + 1), INF, np.int64)          # D[i + 1][j + 1] holds cell (i, j); row 0 and column 0: no predecessor
    ch = np.full((Ta, Tb), NONE, np.uint8)
    D[1, 1] = c[0, 0]
    for d in range(1, Ta + Tb - 1):
        i = np.arange(max(0, d - Tb + 1), min(d, Ta - 1) + 1)
        j = d - i
        diag, up, left = D[i, j], D[i, j + 1], D[i + 1, j]
        best, k = diag.copy(), np.where(diag < INF, 0, NONE).astype(np.uint8)
        m = (up < INF) & ((k == NONE) | (up < best))
        best[m], k[m] = up[m], 1
        m = (left < INF) & ((k == NONE) | (left < best))
        best[m], k[m] = left[m], 2
        D[i + 1, j + 1] = c[i, j] + best
        ch[i, j] = k
    L, dist, map_a, map_b = _walk(c, ch, Ta, Tb, scale)
    return int(D[Ta, Tb]), dist, L, map_a, map_b


def durations(durations_a, map_a, Tb):
    """the timing transfer, written out"""
    da, ma = [int(x) for x in durations_a], [int(x) for x in map_a]
    Ta, n = len(ma), len(da)
    assert all(x >= 0 for x in da) and sum(da) == Ta
    pos = [0] + [ma[sum(da[:p])] if sum(da[:p]) < Ta else Tb for p in range(1, n)] + [Tb]
    return np.array([pos[p + 1] - pos[p] for p in range(n)], np.int32)


def group_ends(Ta, Tb):
    """where the launch groups of a batch end: consecutive pairs while their cells stay within 2^27"""
    ends, cells = [], 0
    for p, (x, y) in enumerate(zip(Ta, Tb)):
        if cells + x * y > GROUP_CELLS and cells:
            ends.append(p)
            cells = 0
        cells += x * y
    return ends + [len(Ta)]


def repeated(A, reps):
    """B = A with row i repeated reps[i] times; -> (B, the run starts, the run index of every row of B)"""
    reps = np.asarray(reps)
    idx = np.repeat(np.arange(len(A)), reps)
    return A[idx], (np.cumsum(reps) - reps).astype(np.int32), idx.astype(np.int32)
