"""Host restatements of include/nsg.h's nsg_mel_cepstra and nsg_dtw (numpy only; no kernel, no torch).

  * dtw64(a, b): the definition as the obvious double loop in fp64 -- the yardstick of accuracy, and exact wherever every
    distance and every partial cost is an integer (the exact probes).
  * dtw32(a, b): the definition operation for operation in fp32 -- what the kernel must return bit for bit.  The distance matrix
    is one fp32 chain per cell over k ascending (numpy rounds every elementwise operation and fuses nothing; its float32 sqrt is
    correctly rounded); the recurrence runs along anti-diagonals, whose cells are independent.
  * cepstra32(mel, table, frames): nsg_mel_cepstra's fp32 chain over the bands in order; cepstra64 / dct_table64: fp64.

Both dtw functions return (cost, steps, path): path (steps, 2) int32, the cells from (0, 0) to (la - 1, lb - 1).  Ties between
predecessors go to the diagonal, then (i - 1, j), then (i, j - 1): each candidate replaces the best only when strictly smaller."""
import numpy as np


def frame_distances32(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    for k in range(a.shape[1]):
        t = a[:, None, k] - b[None, :, k]
        acc = acc + t * t
    assert acc.dtype == np.float32
    return np.sqrt(acc)


def frame_distances64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]))
    for k in range(a.shape[1]):
        t = a[:, None, k] - b[None, :, k]
        acc = acc + t * t
    return np.sqrt(acc)


def backtrack(direction, la, lb, steps):
    path = np.empty((steps, 2), dtype=np.int32)
    i, j = la - 1, lb - 1
    for p in range(steps - 1, -1, -1):
        path[p] = (i, j)
        dc = direction[i, j]
        i, j = i - (dc != 2), j - (dc != 1)
    assert (i, j) == (-1, -1) or steps == 0, "the path does not start at (0, 0)"
    return path


def dtw64(a, b):
    d = frame_distances64(a, b)
    la, lb = d.shape
    D = np.full((la + 1, lb + 1), np.inf)
    N = np.zeros((la + 1, lb + 1), dtype=np.int64)
    direction = np.zeros((la, lb), dtype=np.uint8)
    for i in range(la):
        for j in range(lb):
            if i == 0 and j == 0:
                D[1, 1], N[1, 1] = d[0, 0], 1
                continue
            best, n, dc = D[i, j], N[i, j], 0
            if D[i, j + 1] < best:
                best, n, dc = D[i, j + 1], N[i, j + 1], 1
            if D[i + 1, j] < best:
                best, n, dc = D[i + 1, j], N[i + 1, j], 2
            D[i + 1, j + 1], N[i + 1, j + 1], direction[i, j] = best + d[i, j], n + 1, dc
    steps = int(N[la, lb])
    return float(D[la, lb]), steps, backtrack(direction, la, lb, steps)


def dtw32(a, b):
    d = frame_distances32(a, b)
    la, lb = d.shape
    D = np.full((la + 1, lb + 1), np.inf, dtype=np.float32)         # row / column 0: the absent predecessors
    N = np.zeros((la + 1, lb + 1), dtype=np.int32)
    direction = np.zeros((la, lb), dtype=np.uint8)
    D[1, 1], N[1, 1] = d[0, 0], 1
    for s in range(1, la + lb - 1):
        i = np.arange(max(0, s - lb + 1), min(la - 1, s) + 1)
        j = s - i
        best, n, dc = D[i, j], N[i, j], np.zeros(len(i), dtype=np.uint8)
        for code, (pi, pj) in ((1, (i, j + 1)), (2, (i + 1, j))):
            take = D[pi, pj] < best
            best, n, dc = np.where(take, D[pi, pj], best), np.where(take, N[pi, pj], n), np.where(take, np.uint8(code), dc)
        total = best + d[i, j]
        assert total.dtype == np.float32
        D[i + 1, j + 1], N[i + 1, j + 1], direction[i, j] = total, n + 1, dc
    steps = int(N[la, lb])
    return D[la, lb], steps, backtrack(direction, la, lb, steps)


def dct_table64(n_mels, n_ceps, min_level_db=-100.0):
    """Rows 1 .. n_ceps of the orthonormal DCT-II matrix, times the normalised-mel -> natural-log-amplitude scale, in fp64."""
    t = np.empty((n_ceps, n_mels))
    for k in range(1, n_ceps + 1):
        for j in range(n_mels):
            t[k - 1, j] = np.sqrt(2.0 / n_mels) * np.cos(np.pi * k * (2 * j + 1) / (2.0 * n_mels))
    return t * (-min_level_db * np.log(10.0) / 20.0)


def cepstra32(mel, table, frames=None):
    """mel (n_mels, T) fp32, table (K, n_mels) fp32 -> (T, K) fp32: +0.0 start, bands in order, product and sum rounded."""
    mel, table = np.ascontiguousarray(mel, dtype=np.float32), np.ascontiguousarray(table, dtype=np.float32)
    T = mel.shape[1]
    acc = np.zeros((T, table.shape[0]), dtype=np.float32)
    for j in range(mel.shape[0]):
        acc = acc + mel[j][:, None] * table[:, j][None, :]
    assert acc.dtype == np.float32
    if frames is not None:
        acc[frames:] = 0.0
    return acc


def cepstra64(mel, table64):
    return np.asarray(mel, dtype=np.float64).T @ np.asarray(table64, dtype=np.float64).T
