"""CPU side of tests/test_gpu_f0_cond_envelope.py (numpy and torch on the host only): the launch geometry of csrc/f0_cond.hip as
functions of its launch constants, the references of nsg_add_cond and nsg_column_sum in the header's order, the bf16 store's
rounding as integer arithmetic, and the inputs of the nsg_f0_bins cases with what include/nsg.h says of them.
tests/test_f0_cond_envelope_host.py checks on the host what the GPU tests rely on: that the probes are exact, that the
order-sensitive data is order-sensitive, and that the references stay inside the stated caps."""
import numpy as np
import torch

from tests.helpers import f0_cond_ref as R

F32, BF16 = torch.float32, torch.bfloat16


def vec(dtype):
    """Channels per 16-byte vector of the narrower side: Width<float, TY>::W and Elem<T>::N."""
    return 8 if dtype == BF16 else 4


# ---- launch geometry --------------------------------------------------------------------------------------------------------
def ew_blocks(n, cap, threads):
    """nsg_common.h: ew_blocks."""
    return min(cap, max(1, -(-n // threads)))


def add_cond_launch(nw, cap, threads, items):
    """add_cond_kernel over nw vectors -> (blocks, trips of the grid-stride loop, threads of the last trip with all `items`
    items, with some of them, with none)."""
    blocks = ew_blocks((nw + 1) // items, cap, threads)
    stride = blocks * threads
    trips = -(-nw // (items * stride))
    left = nw - (trips - 1) * items * stride                   # the last trip: thread t has item u iff t + u * stride < left
    whole = max(0, left - (items - 1) * stride)
    some = min(left, stride) - whole
    return blocks, trips, (whole, some, stride - whole - some)


def column_sum_launch(nv, cap, threads):
    """column_sum_kernel over nv vectors -> (blocks, trips, vectors of the last trip)."""
    blocks = ew_blocks(nv, cap, threads)
    stride = blocks * threads
    trips = -(-nv // stride)
    return blocks, trips, nv - (trips - 1) * stride


def smallest_above(limit, per_w, extra=0):
    """The smallest W with W * per_w > limit (+ extra)."""
    return limit // per_w + 1 + extra


def largest_below(limit, per_w):
    """The largest W with W * per_w < limit."""
    return (limit - 1) // per_w


# ---- nsg_add_cond -----------------------------------------------------------------------------------------------------------
def add_cond_inputs(B, H, W, C, n_rows, K, seed, rows=True):
    """-> dict of CPU tensors: x (B, H, W, C) (rows=True only), code (K, C), idx (B, H, W), clip (B, C), table (n_rows, C), bins
    (B, W); every table row and every code row is named by some index where the grid has room for it."""
    g = torch.Generator().manual_seed(seed)
    d = dict(code=torch.randn(K, C, generator=g), clip=torch.randn(B, C, generator=g), table=torch.randn(n_rows, C, generator=g))
    d["idx"] = (torch.arange(B * H * W) % K)[torch.randperm(B * H * W, generator=g)].view(B, H, W)
    d["bins"] = (torch.arange(B * W) % n_rows)[torch.randperm(B * W, generator=g)].view(B, W)
    if rows:
        d["x"] = torch.randn(B, H, W, C, generator=g)
    return d


def add_cond_ref(src, clip, table, bins, relu, dtype):
    """include/nsg.h: (src + clip) + table[bins], ReLU, the store type's rounding -- torch on the CPU in fp32, out-of-range bins
    clamped as 64-bit values.  src (B, H, W, C) is not modified."""
    want = src + clip[:, None, None, :] if clip is not None else src.clone()
    want += table[bins.clamp(0, table.shape[0] - 1)][:, None, :, :]
    if relu:
        want.relu_()
    return want.to(dtype)


def gather_rows(code, idx):
    return code[idx.clamp(0, code.shape[0] - 1)]


CLAMPED = lambda n: [-1, n, -(2 ** 63), 2 ** 63 - 1, 2 ** 32, 2 ** 32 + 1, -(2 ** 32)]       # noqa: E731
TRUNCATED = lambda n: [-1, n, 0, -1, 0, 1, 0]                                                # noqa: E731  (the same as 32-bit values)


def bf16_bits_rne(x):
    """Round-to-nearest-even of finite fp32 values to bf16 as integer arithmetic on the fp32 pattern: add 0x7fff plus the lowest
    kept bit, drop the low 16 bits (a carry out of the significand moves the exponent on, up to infinity).  -> uint16."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    assert ((b & 0x7F800000) != 0x7F800000).all(), "finite values only"
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


# fp32 patterns of the positive rounding probes, by kind; each is run with both signs
ROUNDING_PROBES = {
    "tie, even lower neighbour": [0x3F808000, 0x42FE8000, 0x00808000, 0x3F7E8000],
    "tie, odd lower neighbour": [0x3F818000, 0x42FF8000, 0x00818000, 0x3F7F8000],          # (0x3F7F8000 carries into the exponent: 1.0)
    "one fp32 ulp below a tie": [0x3F807FFF, 0x3F817FFF, 0x42FE7FFF, 0x42FF7FFF],
    "one fp32 ulp above a tie": [0x3F808001, 0x3F818001, 0x42FE8001, 0x42FF8001],
    "the largest finite bf16 + half a bf16 ulp": [0x7F7F8000],
    "the fp32 value just below it": [0x7F7F7FFF],
    "bf16 subnormals": [0x00008000, 0x00018000, 0x00028000, 0x00008001, 0x00017FFF, 0x00400000, 0x007F8000, 0x007F7FFF, 0x00000001],
}
# what the rule must give for the positive probe (the negative one: the same with the sign bit)
ROUNDING_EXPECTED = {
    "tie, even lower neighbour": [0x3F80, 0x42FE, 0x0080, 0x3F7E],
    "tie, odd lower neighbour": [0x3F82, 0x4300, 0x0082, 0x3F80],
    "one fp32 ulp below a tie": [0x3F80, 0x3F81, 0x42FE, 0x42FF],
    "one fp32 ulp above a tie": [0x3F81, 0x3F82, 0x42FF, 0x4300],
    "the largest finite bf16 + half a bf16 ulp": [0x7F80],
    "the fp32 value just below it": [0x7F7F],
    "bf16 subnormals": [0x0000, 0x0002, 0x0002, 0x0001, 0x0001, 0x0040, 0x0080, 0x007F, 0x0000],
}


def rounding_probes():
    """-> (t, x, clip, table) fp32 numpy, each (P,): (x + clip) + table == t exactly in fp32, t the probes of both signs (padded
    with 1.0 to a multiple of 8).  With hi = t's upper 16 bits as a value: x = clip = hi / 2, table = t - hi -- both adds meet
    operands that are not zero wherever hi is not, and no sum needs a bit fp32 does not have (the host module checks this in
    fp64)."""
    pos = np.array([p for kind in ROUNDING_PROBES.values() for p in kind], dtype=np.uint32)
    bits = np.concatenate((pos, pos | np.uint32(0x80000000)))
    bits = np.concatenate((bits, np.full(-len(bits) % 8, 0x3F800000, dtype=np.uint32)))
    t = bits.view(np.float32)
    hi = (bits & np.uint32(0xFFFF0000)).view(np.float32)
    half = (hi * np.float32(0.5)).astype(np.float32)
    return t, half, half.copy(), (t - hi).astype(np.float32)


# ---- nsg_column_sum ---------------------------------------------------------------------------------------------------------
def order_data(B, H, W, C, seed, dtype=F32, rows=4):
    """Rows of very different magnitudes, so that the order of an fp32 sum shows.
    fp32: randn times 2 ** randint(-10, 11).
    bf16: that draw does not show the order -- a bf16 value has 8 significant bits, so an fp32 sum of two of them is exact unless
    their exponents lie more than 16 apart, and on it the descending sum differs in under 5 % of the outputs at H <= 5.  Instead
    every output has one row of randn's magnitude, drawn among the rows the unrolled trips take (`rows` a trip; any row at
    H < rows), and the others 2 ** (-20 + randint(-2, 3)) times smaller: each of them is rounded as it is added to the large one."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, C, generator=g)
    if dtype == BF16:
        e = torch.randint(-22, -17, (B, H, W, C), generator=g, dtype=F32)
        big = torch.randint(0, rows * (H // rows) if H >= rows else H, (B, 1, W, C), generator=g)
        e += 20.0 * (torch.arange(H).view(1, H, 1, 1) == big)
    else:
        e = torch.randint(-10, 11, (B, H, W, C), generator=g, dtype=F32)
    x *= e.exp2_()
    return x.to(dtype)


def colsum_ascending(x):
    """include/nsg.h: every (b, w, c) adds its H values to 0.f in ascending h in fp32."""
    acc = torch.zeros(x.shape[0], x.shape[2], x.shape[3])
    for h in range(x.shape[1]):
        acc += x[:, h].float()
    return acc


def colsum_descending(x):
    return colsum_ascending(x.flip(1))


def colsum_pairwise(x, rows=4):
    """What a kernel that summed each trip of four rows as (r0 + r1) + (r2 + r3) before adding it would give."""
    H = x.shape[1]
    acc = torch.zeros(x.shape[0], x.shape[2], x.shape[3])
    h = 0
    while h + rows <= H:
        r = [x[:, h + u].float() for u in range(rows)]
        acc += (r[0] + r[1]) + (r[2] + r[3])
        h += rows
    for h in range(h, H):
        acc += x[:, h].float()
    return acc


def integer_data(B, H, W, C, seed, dtype=F32):
    """Integer-valued rows whose every partial sum over h is an integer below 2^24 (fp32: |x| <= 2^20; bf16: |x| <= 128, all of
    them bf16 values): the sum is exact in any order, so only the indexing decides the result."""
    g = torch.Generator().manual_seed(seed)
    lim = 128 if dtype == BF16 else 1 << 20
    return torch.randint(-lim, lim + 1, (B, H, W, C), generator=g).float().to(dtype)


# ---- nsg_f0_bins ------------------------------------------------------------------------------------------------------------
RANGE = (65.0, 500.0)


def one_value_range():
    """(fmin, fmax) with fmin < fmax in fp32 whose fp32 log2 are one value: the first fp32 integer from 100 upwards that shares
    its fl32(log2) with its successor -- a range include/nsg.h refuses for its span."""
    for f in np.arange(100, 120, dtype=np.float32):
        g = np.nextafter(f, np.float32(1e3))
        if np.float32(np.log2(np.float64(f))) == np.float32(np.log2(np.float64(g))):
            return float(f), float(g)
    raise AssertionError("no such pair")


def contours(B, T, seed, unvoiced=0.3, lo=60.0, hi=550.0):
    """(B, T) fp32: uniform in lo .. hi Hz -- a little beyond RANGE on either side --, about 30 % of the frames unvoiced (+0.0)."""
    rs = np.random.RandomState(seed)
    f = rs.uniform(lo, hi, size=(B, T)).astype(np.float32)
    f[rs.uniform(size=(B, T)) < unvoiced] = 0.0
    return f


def must_frames(T, W):
    """Lengths every shape is run with: 0, 1, T, the columns' end 4 W, and one ending at each of the four positions inside a
    column, in the middle of the clip and at its start."""
    w = W // 2
    return [0, 1, T, 4 * W, 4 * w, 4 * w + 1, 4 * w + 2, 4 * w + 3, T - 1, 2, 3, 4]


def frame_sets(B):
    """Sets of B lengths it takes to hold must_frames."""
    return -(-12 // B)


def ragged_frames(B, T, W, k):
    """The k-th set of B clip lengths: its share of must_frames, the rest drawn from 0 .. T."""
    fr = np.random.RandomState(100 + k).randint(0, T + 1, size=B)
    part = must_frames(T, W)[k * B:(k + 1) * B]
    fr[:len(part)] = part
    return fr.astype(np.int64)


def affine_rows(B, seed):
    rs = np.random.RandomState(seed)
    return np.stack((rs.uniform(6.5, 8.0, B), rs.uniform(0.5, 1.5, B), rs.uniform(6.5, 8.0, B)), axis=1).astype(np.float32)


# exact bin edges: fmin = 64, fmax = 512, so lo = 6 and span = 3 exactly; columns of powers of two
EDGE_RANGE = (64.0, 512.0)
EDGE_BINS = (3, 6, 12, 96)
EDGE_COLUMNS = [
    # (four frames, the exact mean log2 F0, what the column is)
    ([64.0] * 4, 6.0, "u = 0: bin 1"),
    ([128.0] * 4, 7.0, "u = n_bins / 3, an integer: the upper bin"),
    ([256.0] * 4, 8.0, "u = 2 n_bins / 3, an integer: the upper bin"),
    ([512.0] * 4, 9.0, "u = n_bins: clamped to n_bins"),
    ([128.0, 256.0, 128.0, 256.0], 7.5, "u = n_bins / 2: as floor gives"),
    ([32.0] * 4, 5.0, "u < 0: bin 1"),
    ([1024.0] * 4, 10.0, "u > n_bins: bin n_bins"),
    ([128.0, 128.0, 0.0, 128.0], 7.0, "three voiced frames: 21 / 3 is exact"),
    ([64.0, 128.0, 256.0, 512.0], 7.5, "four different frames: 30 / 4"),
    ([0.0, 64.0, 0.0, 256.0], 7.0, "two voiced frames: 14 / 2"),
    ([0.0, 0.0, 256.0, 0.0], None, "one voiced frame: unvoiced"),
    # two means that fp32 rounds, a third of a bin or more from every edge at each of EDGE_BINS: u = 2 n_bins / 9 and n_bins / 9,
    # whose fraction is 2/3 in one of the two -- where rounding to nearest would give the next bin
    ([128.0, 128.0, 0.0, 64.0], 20.0 / 3.0, "not exact, 20 / 3"),
    ([64.0, 64.0, 128.0, 0.0], 19.0 / 3.0, "not exact, 19 / 3"),
]
EDGE_EXACT = np.array(["not exact" not in c[2] for c in EDGE_COLUMNS])


def edge_case(n_bins):
    """-> (f0 (2, 4 W) fp32: the columns in order and reversed, mean (2, W) fp64 (NaN: unvoiced), u (2, W) fp64, bins (2, W)) by
    the header's rule in exact arithmetic."""
    cols = np.array([c[0] for c in EDGE_COLUMNS], dtype=np.float32)
    mean = np.array([np.nan if c[1] is None else c[1] for c in EDGE_COLUMNS])
    u = (mean - 6.0) * n_bins / 3.0
    with np.errstate(invalid="ignore"):
        bins = np.where(np.isnan(u), 0, 1 + np.clip(np.floor(u), 0, n_bins - 1)).astype(np.int64)
    two = lambda a: np.stack((a, a[::-1]))                                                   # noqa: E731
    return two(cols).reshape(2, -1), two(mean), two(u), two(bins)


# every voicing pattern: frame t of the column under test holds VOICING_HZ[t] where the mask has bit t; log2: 6, 7, 9, 13 -- the
# mean of every subset of two or more differs from every other's, so logf says which frames were counted
VOICING_HZ = (64.0, 128.0, 512.0, 8192.0)
VOICING_RANGE = (64.0, 16384.0)          # lo = 6, span = 8
VOICING_BINS = 16                        # u = 2 (l - 6)


def voicing_case():
    """80 clips of three columns, T = 13: clip 16 cut + mask ends `cut` frames into column 1 (frames = 4 + cut), whose frames are
    voiced by `mask`; column 0 is whole and voiced, column 2 and frame 12 lie past every clip's end and are voiced in the data.
    -> (f0 (80, 13) fp32, frames (80,), n (80,) counted frames of column 1, mean (80,) fp64 over exactly those (NaN: unvoiced))."""
    f0 = np.zeros((80, 13), dtype=np.float32)
    frames, n, mean = np.zeros(80, dtype=np.int64), np.zeros(80, dtype=np.int64), np.full(80, np.nan)
    for cut in range(5):
        for mask in range(16):
            b = 16 * cut + mask
            f0[b, 0:4] = 128.0
            f0[b, 4:8] = [VOICING_HZ[t] if mask >> t & 1 else 0.0 for t in range(4)]
            f0[b, 8:13] = 256.0
            frames[b] = 4 + cut
            logs = [np.log2(VOICING_HZ[t]) for t in range(4) if mask >> t & 1 and t < cut]
            n[b] = len(logs)
            if len(logs) >= 2:
                mean[b] = sum(logs) / len(logs)
    return f0, frames, n, mean


def not_voiced_case():
    """Values that are not > 0 do not count: -0.0, a negative frequency, NaN.  Row 0: a column of each kind alone (unvoiced);
    row 1: each kind mixed with 128 and 512 Hz (mean 8 over the two).  -> f0 (2, 12) fp32."""
    kinds = np.array([-0.0, -128.0, np.nan], dtype=np.float32)
    f0 = np.zeros((2, 12), dtype=np.float32)
    for w, v in enumerate(kinds):
        f0[0, 4 * w:4 * w + 4] = v
        f0[1, 4 * w:4 * w + 4] = [v, 128.0, v, 512.0]
    return f0


def f0_reference(f0, W, n_bins, fmin, fmax, frames=None, affine=None):
    """The fp64 definition with what the judgement needs: -> dict(b64, l64, u64, voiced, dec, undecided)."""
    b64, l64, u64, voiced = R.bins_f64(f0, W, n_bins, fmin, fmax, frames, affine)
    dec = R.decided(u64)
    return dict(b64=b64, l64=l64, u64=u64, voiced=voiced, dec=dec, undecided=voiced & ~dec)
