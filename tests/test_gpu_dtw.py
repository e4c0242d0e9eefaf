"""nsg_dtw across its envelope against the fp32 restatement of include/nsg.h's definition (tests/helpers/dtw_ref.py), bit for
bit: cost as its uint32 pattern, steps, and every cell of the path.  No tolerance anywhere in this file.

Guards: a and b are views into NaN-filled buffers (GUARD floats on either side) and every element past a pair's own length is
NaN as well, so a read past a length poisons the cost; cost, steps and path are views into buffers filled with NaN / a sentinel,
so a missing store, a store past steps[p] rows of the path or a store outside a tensor shows."""
import functools

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, ops
from tests.helpers import dtw_ref as R

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)
DEV = torch.device("cuda:0")

GUARD = 67
SENTINEL = -77
W = ops.DTW_BLOCK_COLS                                   # columns of b one sweep of the wave covers (include/nsg.h)
LENGTHS = [(1, 1), (1, 37), (37, 1), (2, 2), (63, 64), (64, 64), (65, 64), (64, 65), (129, 200), (200, 129)]
KS = [1, 13, 16, 64]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def pair(la, lb, K, seed=0):
    """Features of the magnitude of mel cepstra (a few units), and their restatement's (cost, steps, path)."""
    rs = np.random.RandomState(1000 * seed + 7 * la + 13 * lb + K)
    a, b = (3 * rs.standard_normal((la, K))).astype(np.float32), (3 * rs.standard_normal((lb, K))).astype(np.float32)
    return a, b, R.dtw32(a, b)


def guarded(rows, T, K):
    """The sequences `rows` (each (len, K)) as a (B, T, K) view into a NaN-filled buffer, NaN past each length."""
    B = len(rows)
    buf = torch.full((B * T * K + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    host = np.full((B, T, K), np.nan, dtype=np.float32)
    for p, r in enumerate(rows):
        host[p, :len(r)] = r
    view = buf[GUARD:GUARD + B * T * K].view(B, T, K)
    view.copy_(torch.from_numpy(host))
    return view


def guarded_out(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def run(pairs, Ta, Tb, want_path, device_lengths=False):
    """[(a, b), ...] in one launch -> (cost (B,), steps (B,), path (B, Ta + Tb - 1, 2) or None) as numpy, guards checked."""
    B, K = len(pairs), pairs[0][0].shape[1]
    a, b = guarded([p[0] for p in pairs], Ta, K), guarded([p[1] for p in pairs], Tb, K)
    la, lb = np.array([len(p[0]) for p in pairs], dtype=np.int32), np.array([len(p[1]) for p in pairs], dtype=np.int32)
    if device_lengths:
        la, lb = torch.from_numpy(la).to(DEV), torch.from_numpy(lb).to(DEV)
    cbuf, cost = guarded_out(B, torch.float32, float("nan"))
    sbuf, steps = guarded_out(B, torch.int32, SENTINEL)
    pbuf, path = guarded_out(B * (Ta + Tb - 1) * 2, torch.int32, SENTINEL)
    out = ops.dtw(a, b, la, lb, want_path, out=(cost, steps, path.view(B, Ta + Tb - 1, 2)) if want_path else (cost, steps))
    assert len(out) == (3 if want_path else 2) and out[0] is cost and out[1] is steps
    cw, sw, pw = cbuf.cpu().numpy(), sbuf.cpu().numpy(), pbuf.cpu().numpy()
    assert np.isnan(cw[:GUARD]).all() and np.isnan(cw[GUARD + B:]).all(), "a store outside cost"
    assert (sw[:GUARD] == SENTINEL).all() and (sw[GUARD + B:] == SENTINEL).all(), "a store outside steps"
    assert (pw[:GUARD] == SENTINEL).all() and (pw[GUARD + path.numel():] == SENTINEL).all(), "a store outside path"
    got_path = pw[GUARD:GUARD + path.numel()].reshape(B, Ta + Tb - 1, 2)
    if not want_path:
        assert (got_path == SENTINEL).all(), "path written although none was asked for"
    return cw[GUARD:GUARD + B], sw[GUARD:GUARD + B], got_path if want_path else None


def check(pairs, refs, Ta, Tb, **kw):
    for want_path in (False, True):
        cost, steps, path = run(pairs, Ta, Tb, want_path, **kw)
        for p, (c, n, cells) in enumerate(refs):
            assert bits(cost[p]) == bits(c), (p, want_path, float(cost[p]), float(c))
            assert steps[p] == n, (p, want_path, int(steps[p]), n)
            if want_path:
                assert np.array_equal(path[p, :n], cells), (p, int((path[p, :n] != cells).any(axis=1).sum()))
                assert (path[p, n:] == SENTINEL).all(), "rows of the path past steps were written"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("la,lb", LENGTHS)
def test_single_pair_matches_the_restatement(la, lb, K):
    """Tensors exactly as long as the pair: the last row and column are the tensors' last."""
    a, b, ref = pair(la, lb, K)
    check([(a, b)], [ref], la, lb)


@pytest.mark.parametrize("K", KS)
def test_mixed_lengths_in_one_launch(K):
    """Six pairs of different lengths in one launch, Ta and Tb above every length; once with the lengths already on the device."""
    cases = [pair(la, lb, K, seed=1) for la, lb in ((1, 37), (2, 2), (65, 64), (64, 65), (129, 200), (200, 129))]
    check([(a, b) for a, b, _ in cases], [r for _, _, r in cases], 210, 205)
    if K == 13:
        check([(a, b) for a, b, _ in cases], [r for _, _, r in cases], 210, 205, device_lengths=True)


@pytest.mark.parametrize("la,lb", [(70, W + 1), (150, 2 * W + 1), (W + 1, 37), (3 * 64 + 1, W), (5, 2 * W)])
@pytest.mark.parametrize("K", [13, 64])
def test_across_column_blocks_and_ring_refills(la, lb, K):
    """b one column longer than a block of W columns, and one block plus one: the block's last column is handed on.  a longer
    than 64, 128 and 192 rows: the ring of a's rows in LDS is refilled and wraps.  Whole blocks exactly, too."""
    a, b, ref = pair(la, lb, K, seed=2)
    check([(a, b)], [ref], la + 3, lb + 2)


def test_longest_sequences():
    """NSG_DTW_MAX_FRAMES x NSG_DTW_MAX_FRAMES with a path (K = 5): eight column blocks, the largest workspace and LDS boundary."""
    M = ops.DTW_MAX_FRAMES
    a, b, ref = pair(M, M - 3, 5, seed=3)
    check([(a, b)], [ref], M, M)


def integer_pair(la, lb, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 4, (la, 1)).astype(np.float32), rs.randint(0, 4, (lb, 1)).astype(np.float32)


@pytest.mark.parametrize("la,lb", [(65, 64), (130, 97)])
def test_exact_probe_integer_features(la, lb):
    """K = 1, features in {0, 1, 2, 3}: every distance is a small integer, every D an integer far below 2^24, ties are
    everywhere -- fp64 and fp32 are both exact, so the kernel must equal the fp64 double loop, tie rule and steps included."""
    a, b = integer_pair(la, lb, seed=la)
    c64, n64, p64 = R.dtw64(a, b)
    assert c64 == int(c64) and (np.diff(p64, axis=0) != 1).any()
    check([(a, b)], [(np.float32(c64), n64, p64)], la + 1, lb + 1)


@pytest.mark.parametrize("n,K", [(1, 13), (64, 13), (65, 1), (300, 16)])
def test_identical_sequences(n, K):
    a, _, _ = pair(n, 1, K, seed=4)
    diagonal = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    cost, steps, path = run([(a, a)], n + 2, n + 5, True)
    assert bits(cost[0]) == 0 and steps[0] == n and np.array_equal(path[0, :n], diagonal)      # +0.0 by bit pattern


def test_refusals_launch_nothing():
    """Each refusal carries the library's message; the outputs keep their fill."""
    K = 13
    a, b, _ = pair(20, 30, K)
    ga, gb = guarded([a], 20, K), guarded([b], 30, K)
    cbuf, cost = guarded_out(1, torch.float32, float("nan"))
    sbuf, steps = guarded_out(1, torch.int32, SENTINEL)

    def call(x, y, la, lb):
        return ops.dtw(x, y, la, lb, out=(cost, steps))

    with pytest.raises(_lib.NsgError, match=r"len_a: every length must be in \[1, 20\]"):
        call(ga, gb, [0], [30])
    with pytest.raises(_lib.NsgError, match=r"len_b: every length must be in \[1, 30\]"):
        call(ga, gb, [20], [31])
    M = ops.DTW_MAX_FRAMES
    long = torch.zeros(1, M + 1, K, device=DEV)
    with pytest.raises(_lib.NsgError, match=r"nsg_dtw: sequence lengths \(Ta = %d, Tb = 30\) outside \[1, %d\]" % (M + 1, M)):
        call(long, gb, [M + 1], [30])
    with pytest.raises(_lib.NsgError, match=r"nsg_dtw: K = 65 outside \[1, 64\]"):
        call(torch.zeros(1, 20, 65, device=DEV), torch.zeros(1, 30, 65, device=DEV), [20], [30])
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        call(ga.cpu(), gb, [20], [30])
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        call(ga, gb.cpu(), [20], [30])
    torch.cuda.synchronize()
    assert np.isnan(cbuf.cpu().numpy()).all() and (sbuf.cpu().numpy() == SENTINEL).all()
