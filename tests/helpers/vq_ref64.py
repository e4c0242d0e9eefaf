"""The fp64 yardstick of the vector quantiser's kernels (csrc/vq.hip, vq_bf16.hip, segsum.hip, the one-hot forms of
gemm_wgrad.hip, vq_losses_indexed_kernel of elementwise.hip), their bounds, acceptance rules and case tables: plain torch and
numpy on the CPU.  tests/test_vq_ref_host.py shows that this file is right and sharp (a CPU emulation of the split search stays
inside the bound; every acceptance rule rejects a list of deliberately wrong results); tests/test_gpu_vq_envelope.py checks the
kernels against it.  Nothing here is tuned against the kernels.  Every reference takes its operands AS THE KERNEL SEES THEM:
fp32 tensors are widened, rows given as their sources are first formed in fp32 in the header's order (bnres_rows).

The split search (nsg_vq_forward_bf16x3*), per (row x, code e), A = sum_i |x_i| |e_i|:
  bf16 has unit roundoff 2^-8: hi = bf16(v), lo = bf16(v - hi), so v = hi + lo + rho with |rho| <= 2^-16 |v|.
  x.e = (hx + lx + rx).(he + le + re); the kernel adds lx.he + hx.le + hx.he.  What it drops -- lx.le and the two residual
  terms rx.e and (hx + lx).re -- is at most 3 * 2^-16 * A.  The 3 * DP products (exact in fp32: 8 x 8 significant bits) are
  accumulated in fp32, DP the padded width (16, 32, 64, 128, 256): at most 3 * DP * 2^-24 * A more.
      dot_err = (3 * 2^-16 + 3 * DP * 2^-24) * A
  The computed distance is fma(-2, dot, c2) (production form, HAS_X2 = false) or fma(-2, dot, fl(c2 + x2)) (dmin form):
      bound = 2 * dot_err + (D + 2) * 2^-24 * |e|^2            the fp32 row norm c2 (rowsumsq: D products, < D additions)
                          + 2^-24 * |d|                         the final fma, d the quantity it forms
              and in the dmin form + (D + 2) * 2^-24 * |x|^2 + 2^-24 * (|e|^2 + |x|^2)     x2, and the rounding of c2 + x2
  Acceptance of a picked index p against the fp64 first minimum m (both forms compare the same differences: |x|^2 is constant
  along a row):  dist(p) - dist(m) <= bound(p) + bound(m);  where dmin is requested, |dmin - dist(p)| <= bound(p).
  EVERY row is judged; there is no exclusion (SEARCH_ROWS_LEFT_OUT = 0).
  Integer probe: entries in {-3 .. 3}: hi is the value and lo = 0, every product, norm and c2 + x2 - 2 dot is an integer below
  2^24, exact in bf16 and fp32 (int_exact asserts D * max|v|^2 < 2^23): the kernel must return EXACTLY the first index of the
  integer minimum, and dmin exactly -- the fp32 search and all three bf16x3 forms.

Segment sums (nsg_index_add_rows*): fp64 index_add_ over the rows whose index lies in [0, K), bincount for the counts (exact).
  |got - want| <= gamma(chain) * sum |term| per output element, gamma(n) = n 2^-24 / (1 - n 2^-24), chain the longest chain of
  fp32 additions behind the element, as a function of the code's row count n and of D (sorted_chain, onehot_chain); bf16x2
  adds 2^-16 * sum |term| for the split of the rows.  Integer-valued rows with per-code sums below 2^24 must give EXACT sums.

Losses (nsg_vq_losses_indexed*): the bound classes of tests/test_gpu_elementwise_envelope.py: loss at rtol 1e-6; dz within
  4 * 2^-24 of its terms' magnitudes + 2^-24 max(|z|, |q|) |scale| (the rounding of d = z - q) + 2^-8 |want| when stored as bf16;
  the two BatchNorm sums, taken of dz AS STORED, within 2e-5 * sum |term| (bn_ref64's chain-length bound: losses_chain < 300).

EMA update (nsg_vq_ema_update; formula of include/nsg.h in fp64 with the fp32 values of decay, 1.f - decay and eps widened),
  counting roundings (a, b >= 0 relative; signed sums relative to the sum of magnitudes T):
  v = fl(fl(decay a) + fl(om b)): each term passes 2 roundings: ema_n' within gamma(2) v, ema_s' within gamma(2) T.
  tot = fl32(sum in double of the fp32 v): gamma(3).  nn = fl(fl(fl(v + eps) / fl(tot + fl(K eps))) * tot): v + eps gamma(3),
  K eps gamma(1), tot + K eps gamma(4), the quotient gamma(8), times tot (gamma(3)) and its rounding: gamma(12).
  e = fl(s' / nn): |err| <= gamma(2) T / nn + gamma(13) |e| <= gamma(16) * T / nn  (T / nn >= |e|).
  A total count of 0 is a stated precondition and is not tested."""
import math
import types

import numpy as np
import torch

from tests.helpers import bn_ref64

U32 = 2.0 ** -24                    # unit roundoff of fp32
UBF = 2.0 ** -8                     # ... of bf16
U_SPLIT = 2.0 ** -16                # |v - hi - lo| <= U_SPLIT |v|
SEARCH_ROWS_LEFT_OUT = 0            # the cap on rows a search case may leave out of the acceptance rule
IDX_POISON = -7777                  # what the GPU tests fill an index output with before the call


def f64(t):
    return None if t is None else t.detach().to("cpu").double()


def gamma(n):
    return n * U32 / (1.0 - n * U32)


# ----------------------------------------------------------------------------------------------------------------------
# rows given as their sources
# ----------------------------------------------------------------------------------------------------------------------
def bnres_rows(h, r, mean, invstd, gam, beta):
    """z = ((h - mean) * (invstd * gamma) + beta) + r in fp32 on the CPU, one rounding per operation, no contraction: the
    header's order (include/nsg.h, "Rows given as their SOURCES").  h, r bf16 (N, D); the vectors fp32 (D,)."""
    hf, rf = h.detach().cpu().float(), r.detach().cpu().float()
    mean, invstd, gam, beta = (v.detach().cpu().float() for v in (mean, invstd, gam, beta))
    sc = invstd * gam
    t = hf - mean
    t = t * sc
    t = t + beta
    return t + rf


# ----------------------------------------------------------------------------------------------------------------------
# the search
# ----------------------------------------------------------------------------------------------------------------------
def dp_of(D):
    return 16 if D <= 16 else 32 if D <= 32 else 64 if D <= 64 else 128 if D <= 128 else 256


def search_ref(x, e):
    """fp64 distances (N, K), their first minimum, and the per-(row, code) bounds of the two forms of the split search."""
    x, e = f64(x), f64(e)
    D = x.shape[1]
    x2, e2 = (x * x).sum(1), (e * e).sum(1)
    dot = x @ e.t()
    dist = x2[:, None] + e2[None, :] - 2.0 * dot
    A = x.abs() @ e.abs().t()
    dot_err = (3.0 * U_SPLIT + 3.0 * dp_of(D) * U32) * A
    norm = (D + 2) * U32
    bound_plain = 2.0 * dot_err + norm * e2[None, :] + U32 * (e2[None, :] - 2.0 * dot).abs()
    bound_dmin = 2.0 * dot_err + norm * (e2[None, :] + x2[:, None]) + U32 * (e2[None, :] + x2[:, None]) + U32 * dist.abs()
    return types.SimpleNamespace(N=x.shape[0], K=e.shape[0], D=D, dist=dist, argmin=first_argmin(dist), dmin=dist.min(1).values,
                                 bound_plain=bound_plain, bound_dmin=bound_dmin)


def first_argmin(d):
    """The FIRST index of the minimum of each row (torch.argmin promises no tie rule)."""
    K = d.shape[1]
    m = d.min(1, keepdim=True).values
    pos = torch.arange(K).expand_as(d)
    return torch.where(d == m, pos, torch.full_like(pos, K)).min(1).values


def last_argmin(d):
    m = d.min(1, keepdim=True).values
    pos = torch.arange(d.shape[1]).expand_as(d)
    return torch.where(d == m, pos, torch.full_like(pos, -1)).max(1).values


def search_violations(ref, idx, dmin=None):
    """-> bool (N,): rows whose picked index (and reported distance) the acceptance rule rejects.  idx int64 (N,); dmin fp32 (N,)
    selects the dmin form's bound.  An index outside [0, K) and a non-finite distance are violations."""
    idx = idx.detach().cpu().long()
    bound = ref.bound_plain if dmin is None else ref.bound_dmin
    bad = (idx < 0) | (idx >= ref.K)
    p = idx.clamp(0, ref.K - 1)[:, None]
    m = ref.argmin[:, None]
    excess = ref.dist.gather(1, p) - ref.dist.gather(1, m)
    slack = bound.gather(1, p) + bound.gather(1, m)
    bad |= ~(excess <= slack)[:, 0]
    if dmin is not None:
        err = (dmin.detach().cpu().double()[:, None] - ref.dist.gather(1, p)).abs()
        bad |= ~(err <= bound.gather(1, p))[:, 0]
    return bad


def search_ratio(ref, idx, dmin=None):
    """The largest (excess / slack) and (distance error / bound) over the rows: what the GPU suite reports."""
    idx = idx.detach().cpu().long().clamp(0, ref.K - 1)[:, None]
    bound = ref.bound_plain if dmin is None else ref.bound_dmin
    m = ref.argmin[:, None]
    r_idx = float(((ref.dist.gather(1, idx) - ref.dist.gather(1, m)) / (bound.gather(1, idx) + bound.gather(1, m)).clamp_min(1e-300)).max())
    r_d = 0.0
    if dmin is not None:
        r_d = float(((dmin.detach().cpu().double()[:, None] - ref.dist.gather(1, idx)).abs() / bound.gather(1, idx).clamp_min(1e-300)).max())
    return r_idx, r_d


def int_exact(x, e):
    """The integer probe: asserts its exactness preconditions, -> (first index of the exact minimum (N,), that minimum as fp32)."""
    x, e = f64(x), f64(e)
    assert bool((x == x.round()).all()) and bool((e == e.round()).all()), "integer probe: non-integer entries"
    vmax = max(float(x.abs().max()), float(e.abs().max()), 1.0)
    assert x.shape[1] * vmax * vmax < 2 ** 23, "integer probe: D * max|v|^2 must stay below 2^23"
    assert vmax <= 127, "integer probe: entries must be exact in bf16"
    dist = (x * x).sum(1)[:, None] + (e * e).sum(1)[None, :] - 2.0 * (x @ e.t())
    assert bool((dist == dist.round()).all()) and float(dist.abs().max()) < 2 ** 24
    return first_argmin(dist), dist.min(1).values.float()


def int_violations(x, e, idx, dmin=None):
    want, wd = int_exact(x, e)
    bad = idx.detach().cpu().long() != want
    if dmin is not None:
        bad |= ~(dmin.detach().cpu().float() == wd)
    return bad


def split_bf16(v):
    hi = v.float().bfloat16().float()
    lo = (v.float() - hi).bfloat16().float()
    return hi, lo


def emulate_split_search(x, e, has_x2):
    """A CPU emulation of the split search: hi / lo split, the three products accumulated in fp32 (small terms first), fp32
    row norms, the final expression rounded once.  -> (computed distances fp32 (N, K) as the kernel compares them -- WITHOUT
    |x|^2 when not has_x2 -- and their first minimum)."""
    x, e = x.detach().cpu().float(), e.detach().cpu().float()
    xh, xl = split_bf16(x)
    eh, el = split_bf16(e)
    acc = xl @ eh.t()
    acc = acc + xh @ el.t()
    acc = acc + xh @ eh.t()
    c2 = (e * e).sum(1)
    base = c2[None, :] + (x * x).sum(1)[:, None] if has_x2 else c2[None, :].expand(x.shape[0], -1)
    d = (base.double() - 2.0 * acc.double()).float()          # -2 acc is exact: one rounding, as the fma
    return d, first_argmin(d)


def codes_bf16_ref(e, idx, clip_rows=None, rows_per_clip=0, relu=False, clip_shift=0):
    """bf16( relu?( e[idx] + clip_rows[row // rows_per_clip] ) ), the sum in fp32 on the CPU.  clip_shift != 0 (host test only):
    the neighbouring clip's row, a deliberately wrong result."""
    v = e.detach().cpu().float()[idx.detach().cpu().long()]
    if clip_rows is not None:
        c = clip_rows.detach().cpu().float()
        clip = (torch.arange(v.shape[0]) // rows_per_clip + clip_shift) % c.shape[0]
        v = v + c[clip]
    if relu:
        v = v.clamp_min(0.0)
    return v.bfloat16()


# ---- the exact search's slices (nsg_vq_slices, vq.hip), restated -----------------------------------------------------------
SEARCH_CUS = 256


def vq_slices(N, D, K):
    slots = SEARCH_CUS * (1 if D > 128 else 2)
    nb = -(-N // 128)
    if nb <= 0:
        return 1
    best, best_eff, S = 1, 0.0, 1
    while S <= 8:
        if S > 1 and (-(-K // 32)) // S < 16:
            break
        units = nb * S
        eff = units / float(-(-units // slots) * slots)
        if eff > best_eff * 1.05:
            best_eff, best = eff, S
        S *= 2
    return best


def slice_tiles(K, S):
    return -(-(-(-K // 32)) // S)          # code tiles per slice


# ---- the search's inputs ------------------------------------------------------------------------------------------------------
SEARCH_N = (1, 127, 128, 129, 257)
SEARCH_K = (1, 31, 32, 33, 100, 1000)
SEARCH_D = (8, 16, 24, 40, 64, 72, 120, 128, 136, 248, 256)
SEARCH_DATA = ("gauss", "fresh", "int")


def _search_cases():
    """33 cases: 5, 6 and 11 are pairwise coprime, so over i = 0 .. 32 every D meets three N, three K and all three kinds of
    data, every (N, K) pair occurs, and every padded width is met with D < DP and with D = DP; K = 8192 once, at D = 256."""
    out = []
    for i in range(33):
        out.append((SEARCH_N[i % 5], SEARCH_K[i % 6], SEARCH_D[i % 11], SEARCH_DATA[(i // 11 + i % 11) % 3]))
    out.append((129, 8192, 256, "gauss"))
    out += [(128, 33, 32, "gauss"), (257, 100, 32, "int")]          # D = 32, the one padded width the list above meets only below it
    return out


SEARCH_CASES = _search_cases()


def search_case_id(c):
    return f"{c[0]}x{c[2]}-K{c[1]}-{c[3]}"


def tail_start(D):
    """The first channel of the last k-step of 16 (the half of it that D % 16 == 8 leaves is behind the kernel's d0 < D guard)."""
    return 16 * ((D - 1) // 16)


def plant(e, x, data):
    """Code rows planted from the rows they are to be nearest to (in place; e (K, D), x (N, D) fp32), from the last row back:
      row N-1 = code K-1                      the last row of the last 128-row block is nearest to the last code of the last tile
      row N-2 = code K-2, and code a < K-2 = that row with the channels from tail_start(D) on NEGATED (the same norm): a kernel
                that ignores those channels sees a tie and takes a, whose true distance is 4 |those channels|^2
      row N-3 = codes 1 and 5                 exact duplicates in one 32-code tile
      row N-4 = codes 3 and K-4               ... in different tiles
    -> {name: (row, code the first minimum must be)} of what fitted."""
    N, K = x.shape[0], e.shape[0]
    D = x.shape[1]
    w = {}
    e[K - 1] = x[N - 1]
    w["last"] = (N - 1, K - 1)
    if N >= 2 and K >= 3:
        b = K - 2
        a = max(0, b - 33)
        e[b] = x[N - 2]
        e[a] = x[N - 2]
        e[a, tail_start(D):] = 0.0 - x[N - 2, tail_start(D):]          # (0 - x: no -0.0, whose sign max(0, .) need not keep)
        w["tail"] = (N - 2, b)
    if N >= 3 and K >= 8:
        e[1] = x[N - 3]
        e[5] = x[N - 3]
        w["dup_tile"] = (N - 3, 1)
    if N >= 4 and K >= 40:
        e[3] = x[N - 4]
        e[K - 4] = x[N - 4]
        w["dup_far"] = (N - 4, 3)
    return w


def make_sources(N, D, data, g):
    """bf16 h, r and the fp32 vectors of a BnResRows.  int: mean 1, invstd 2, gamma 0.5, beta -1, so z = h - 2 + r exactly,
    with r in {0, 1} and z in {-3 .. 3}."""
    if data == "int":
        z = torch.randint(-3, 4, (N, D), generator=g).float()
        r = torch.randint(0, 2, (N, D), generator=g).float()
        h = z - r + 2.0
        mean, invstd, gam, beta = torch.ones(D), torch.full((D,), 2.0), torch.full((D,), 0.5), torch.full((D,), -1.0)
    else:
        h = torch.randn(N, D, generator=g) * 1.3 + 0.4
        r = torch.randn(N, D, generator=g).clamp_min(0.0) * 0.5
        mean = torch.randn(D, generator=g) * 0.2 + 0.4
        invstd = 1.0 / (1.3 * (0.8 + 0.4 * torch.rand(D, generator=g)))
        gam = 0.8 + 0.4 * torch.rand(D, generator=g)
        beta = torch.randn(D, generator=g) * 0.2 + (0.5 if data == "fresh" else 0.0)
    return h.bfloat16(), r.bfloat16(), mean, invstd, gam, beta


def make_search_inputs(N, K, D, data):
    """One case's operands (one generator, fixed draw order).  x: the fp32 rows of the two fp32-row forms; src: the sources of
    the third form and z = bnres_rows(*src), its rows as the kernel forms them; e_x / e_z: one codebook with the codes plant()
    derives from x / from z.
      gauss  x ~ N(0, 1), e ~ N(0, 1)
      fresh  the codebook of a fresh model, e ~ U(-1/K, 1/K), against rows of order 1 with a non-zero mean (0.7 randn + 0.5)
      int    entries in {-3 .. 3} (ties are frequent), with planted duplicates"""
    g = torch.Generator().manual_seed(7919 * N + 104729 * K + 31 * D + SEARCH_DATA.index(data))
    if data == "int":
        x = torch.randint(-3, 4, (N, D), generator=g).float()
        e = torch.randint(-3, 4, (K, D), generator=g).float()
    elif data == "gauss":
        x = torch.randn(N, D, generator=g)
        e = torch.randn(K, D, generator=g)
    else:
        x = torch.randn(N, D, generator=g) * 0.7 + 0.5
        e = (torch.rand(K, D, generator=g) * 2.0 - 1.0) / K
    src = make_sources(N, D, data, g)
    z = bnres_rows(*src)
    e_x, e_z = e.clone(), e.clone()
    wx, wz = plant(e_x, x, data), plant(e_z, z, data)
    return types.SimpleNamespace(N=N, K=K, D=D, data=data, x=x, e_x=e_x, src=src, z=z, e_z=e_z, planted_x=wx, planted_z=wz)


# clip rows of the bf16 code output: (rows per clip, clips): a 128-row block spans three clips / is one clip / has the boundary
# at row 129 (its second block begins one row before the second clip)
CLIP_CASES = ((50, 3), (128, 2), (129, 2))

# the exact search: (N, D, K, S the slices nsg_vq_slices picks, what it reaches)
EXACT_CASES = [
    (130, 128, 1000, 2, "two slices of 16 tiles; 1000 is no multiple of 64: the last tile holds 8 codes"),
    (130, 64, 2100, 4, "four slices of 17 tiles, 15 in the last, 20 codes in the last tile"),
    (130, 256, 4100, 8, "eight slices of 17 tiles, 10 in the last, 4 codes in the last tile: no multiple of 32 * 8"),
    (130, 256, 4096, 8, "eight even slices of 16 tiles"),
    (130, 1, 1, 1, "K = 1, D = 1"),
    (130, 17, 1, 1, "K = 1 at an odd width"),
    (130, 17, 1000, 2, "an odd width (scalar loads) through two slices"),
    (130, 255, 4100, 8, "the widest odd width through eight ragged slices"),
    (130, 255, 1, 1, "K = 1 at the widest odd width"),
]


def make_exact_inputs(N, D, K, S):
    """Gaussian x and e with the nearest code of a few rows planted TWICE (bit-identical code rows), the two copies in different
    slices (and, without slices, in different tiles where K allows): the lower index must win.
    -> x, e (numpy fp32), {row: the index that must be returned}."""
    g = torch.Generator().manual_seed(15485863 + 1009 * D + K)
    x = torch.randn(N, D, generator=g)
    e = torch.randn(K, D, generator=g)
    must = {}
    per = 32 * slice_tiles(K, S)          # codes per slice
    if S > 1:
        # slices 0 and 1;  the first code and the last one (the ragged last tile of the last slice);  a middle slice and the last
        for row, a, b in ((0, 5, per + 5), (64, 0, K - 1), (129, (S // 2) * per + 1, (S - 1) * per + 1)):
            if a < b:
                e[a] = x[row]
                e[b] = x[row]
                must[row] = a
    return x.numpy(), e.numpy(), must


# ----------------------------------------------------------------------------------------------------------------------
# segment sums
# ----------------------------------------------------------------------------------------------------------------------
SEG_ROWS, SEG_CH, SEG_SCAN_PASS = 1024, 512, 8 * 96          # segsum.hip


def seg_ref(idx, g, K):
    """fp64 sums (K, D) over the rows whose index lies in [0, K), the sums of |term|, and the counts (int64 (K,))."""
    idx = idx.detach().cpu().long()
    g = f64(g)
    ok = (idx >= 0) & (idx < K)
    rows, ids = g[ok], idx[ok]
    D = g.shape[1]
    sums = torch.zeros(K, D, dtype=torch.float64).index_add_(0, ids, rows)
    absum = torch.zeros(K, D, dtype=torch.float64).index_add_(0, ids, rows.abs())
    counts = torch.bincount(ids, minlength=K)
    return types.SimpleNamespace(sums=sums, absum=absum, counts=counts, K=K, D=D, N=idx.numel())


def sorted_supported(N, D, K):
    """The one rule of include/nsg.h, nsg_index_add_rows_sorted and ops.index_add_sorted_supported."""
    return D % 4 == 0 and K <= 8192 and N < 2 ** 31 and (D % 256 == 0 if D > 256 else (D // 4) & (D // 4 - 1) == 0)


def sorted_chain(n, D):
    """The longest chain of fp32 additions behind one element of a code's sum in the sorted form, n (numpy int array) rows on
    the code.  seg_sum: a chunk is 512 rows, a wave takes a quarter (128 rows); D / 4 = ppr pieces per row, rpi = 64 / ppr rows
    per wave-wide load: a lane adds ceil(min(n, 128) / rpi) rows, the rpi sub-rows are added (rpi - 1), then the four waves (4).
    Wide rows (ppr > 64): one thread adds a chunk's min(n, 512) rows.  seg_final: ceil(n / 512) chunks over G = 256 / P groups
    (P = min(ppr, 256) pieces; one group for P > 64): ceil(chunks / G) per group, then the G groups (G additions from zero)."""
    n = np.asarray(n, dtype=np.int64)
    ppr = D // 4
    chunks = -(-n // SEG_CH)
    P = min(ppr, 256)
    G = 256 // P if P <= 64 else 1
    final = -(-chunks // G) + G
    if ppr <= 64:
        rpi = 64 // ppr
        return -(-np.minimum(n, 128) // rpi) + (rpi - 1) + 4 + final
    return np.minimum(n, SEG_CH) + final


WG_KP = 32          # gemm_wgrad.hip: pixels per chunk; slab rows are a multiple of it


def onehot_plan(N, K, D):
    """plan_slabs of gemm_wgrad.hip for the one-hot GEMM (one tap, A = K, C = D) -> (slabs, rows per slab)."""
    tiles = -(-K // 128) * -(-D // (128 if D > 32 else 32))
    want = max(1, min(512 // tiles, -(-N // 256), 512))
    rows = -(-(-(-N // want)) // WG_KP) * WG_KP
    return -(-N // rows), rows


def onehot_chain(n, N, K, D, bf16x2):
    """The one-hot forms: within a slab the matrix pipe adds one product per row in row order (the rows of other codes add an
    exact 0): min(n, slab rows) additions -- twice that on the bf16 pipe, which adds the lo and the hi part of each row; then
    the slabs, in at most `split` shares: chunk + split <= slabs + 1 additions."""
    nslab, rows = onehot_plan(N, K, D)
    n = np.minimum(np.asarray(n, dtype=np.int64), rows)
    return (2 if bf16x2 else 1) * n + nslab + 1


def bf16x2_runs_bf16(D):
    """nsg_index_add_rows_bf16x2 falls back to the fp32 kernel for D % 8 != 0 or D <= 32."""
    return D % 8 == 0 and D > 32


def seg_bound(impl, ref):
    n = ref.counts.numpy()
    if impl in ("sorted", "sorted_bnres"):
        chain = sorted_chain(n, ref.D)
        extra = 0.0
    else:
        bf = impl == "bf16x2" and bf16x2_runs_bf16(ref.D)
        chain = onehot_chain(n, ref.N, ref.K, ref.D, bf)
        extra = U_SPLIT if bf else 0.0
    rel = torch.from_numpy(chain.astype(np.float64) * U32 / (1.0 - chain.astype(np.float64) * U32)) + extra
    return rel[:, None] * ref.absum


def seg_violations(impl, ref, sums, counts, exact=False):
    """-> number of elements the rule rejects: sums outside the bound (exact: unequal), counts != bincount, non-finite values."""
    got = sums.detach().cpu().double()
    if exact:
        bad = int((~(got == ref.sums)).sum())
    else:
        bad = int((~((got - ref.sums).abs() <= seg_bound(impl, ref))).sum())
    if counts is not None:
        bad += int((~(counts.detach().cpu().double() == ref.counts.double())).sum())
    return bad


SEG_N = (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025)
SEG_K = (1, 7, 8192)
SEG_D = (4, 8, 16, 32, 64, 128, 256, 512)
SEG_BIG_N = SEG_SCAN_PASS * SEG_ROWS + 1025          # 770 blocks of 1024 rows: seg_scan_blk's second pass carries the sum
BAD_INDICES = (-1, "K", "K+5", 2 ** 32 + 3, -2 ** 32 + 1, 2 ** 32)          # 2^32 itself: modulo 2^32 it is code 0, for K = 1


def _seg_cases():
    """(N, K, D, index kind, data).  i = 0 .. 39: 10 N x 8 D x 3 K, pairwise through coprime periods (10 against 3; D advances by
    one and shifts by one each round of 10, so every N meets four widths); the index kinds and the two kinds of data alternate.
    Then the multi-pass scan, skewed and collapsed, and batches with every index out of range."""
    kinds = ("uniform", "skew", "oob_mixed", "collapsed")
    out = []
    for i in range(40):
        out.append((SEG_N[i % 10], SEG_K[i % 3], SEG_D[(i + i // 10) % 8], kinds[(i + i // 4) % 4], ("gauss", "int")[(i + i // 10) % 2]))
    out += [(SEG_BIG_N, 7, 4, "skew", "gauss"), (SEG_BIG_N, 7, 4, "collapsed", "int"), (SEG_BIG_N, 7, 4, "oob_mixed", "int"),
            (1, 7, 8, "oob_all", "gauss"), (1025, 7, 64, "oob_all", "int"), (513, 8192, 16, "oob_all", "gauss")]
    return out


SEG_CASES = _seg_cases()
# the chains a few cases are claimed to have (test_vq_ref_host.py asserts them): (N, K, D, kind) -> (form, longest chain)
SEG_CHAIN_CLAIMS = {
    (SEG_BIG_N, 7, 4, "collapsed"): ("sorted", 2 + 63 + 4 + 5 + 256),          # 524 971 rows on code 3: 1026 chunks over 256 groups
    (1025, 7, 64, "oob_all"): ("sorted", 0 + 3 + 4 + 0 + 16),                  # no row anywhere: the fixed part alone
}


def seg_case_id(c):
    return f"{c[0]}x{c[2]}-K{c[1]}-{c[3]}-{c[4]}"


def bad_index_values(K):
    return [K if v == "K" else K + 5 if v == "K+5" else v for v in BAD_INDICES]


def make_seg_index(N, K, kind, g):
    if kind == "uniform":
        idx = torch.randint(0, K, (N,), generator=g)
    elif kind == "skew":          # most rows on a few codes, a tail on the rest
        idx = (torch.rand(N, generator=g) ** 4 * K).long().clamp(0, K - 1)
    elif kind == "collapsed":     # all rows on two codes
        idx = torch.full((N,), min(3, K - 1), dtype=torch.int64)
        idx[1::3] = max(K - 2, 0)
    elif kind == "oob_mixed":     # a valid batch with the bad values at its first and last rows and spread through it
        idx = torch.randint(0, K, (N,), generator=g)
        bad = bad_index_values(K)
        pos = sorted({0, N - 1} | {int(p) for p in torch.randint(0, N, (2 * len(bad),), generator=g)})
        for j, p in enumerate(pos):
            idx[p] = bad[j % len(bad)]
    else:                         # oob_all
        bad = torch.tensor(bad_index_values(K), dtype=torch.int64)
        idx = bad[torch.arange(N) % bad.numel()]
    return idx


def make_seg_inputs(N, K, D, kind, data):
    """idx int64 (N,), g fp32 (N, D) and the sources of the _bnres form with z = bnres_rows(*src), its rows.  int: entries in
    {-3 .. 3}: every per-code sum stays below 3 N < 2^24, so every fp32 partial sum is exact."""
    g_ = torch.Generator().manual_seed(2750159 + 613 * N + 7 * K + D + 3 * len(kind) + (1 if data == "int" else 0))
    idx = make_seg_index(N, K, kind, g_)
    g = torch.randint(-3, 4, (N, D), generator=g_).float() if data == "int" else torch.randn(N, D, generator=g_) + 0.3
    src = make_sources(N, D, "int" if data == "int" else "gauss", g_)
    assert 3 * N < 2 ** 24
    return types.SimpleNamespace(N=N, K=K, D=D, kind=kind, data=data, idx=idx, g=g, src=src, z=bnres_rows(*src))


def bnres_sorted_supported(D):
    """nsg_index_add_rows_sorted_bnres: D a power of two, 4 <= D <= 256."""
    return 4 <= D <= 256 and D & (D - 1) == 0


# ----------------------------------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------------------------------
def clamp_index(idx, K):
    return idx.clamp(0, K - 1)


def losses_ref(z, e, idx, dz_scale, dz_add=None, clamp=True):
    """-> loss64 (float), dz64 (N, D), the magnitudes of dz's terms, max(|z|, |q|), and the scale.  clamp=False (host test only):
    a bad index wraps modulo K instead, a deliberately wrong result."""
    z, e = f64(z), f64(e)
    K = e.shape[0]
    idx = idx.detach().cpu().long()
    q = e[clamp_index(idx, K) if clamp else idx % K]
    d = z - q
    n = z.numel()
    zs = float(dz_scale) * 2.0 / n
    add = f64(dz_add) if dz_add is not None else torch.zeros(1, dtype=torch.float64)
    return types.SimpleNamespace(loss=float((d * d).sum()) / n, dz=d * zs + add, terms=(d * zs).abs() + add.abs(),
                                 dmax=torch.maximum(z.abs(), q.abs()), zs=zs)


def dz_bound(ref, bf16):
    b = 4 * U32 * ref.terms + U32 * ref.dmax * abs(ref.zs)
    return b + UBF * ref.dz.abs() if bf16 else b


def bn_sums_ref(dz_stored, x, mean, invstd):
    """The BatchNorm backward sums of dz AS STORED: -> dgamma64, dbeta64 and the sums of |term| of each."""
    g, x = f64(dz_stored), f64(x)
    xhat = (x - f64(mean)) * f64(invstd)
    return (g * xhat).sum(0), g.sum(0), (g * xhat).abs().sum(0), g.abs().sum(0)


BN_SUM_TOL = 2e-5


def losses_chain(N, D):
    """A thread takes 8 channels whatever the gradient's type (NsgSlabMap<8>): bn_ref64's chain at the bf16 map."""
    return bn_ref64.chain_length(N, D, True)


def losses_violations(ref, loss, dz, bf16):
    bad = 0 if abs(float(loss) - ref.loss) <= 1e-6 * abs(ref.loss) else 1
    return bad + int((~((dz.detach().cpu().double() - ref.dz).abs() <= dz_bound(ref, bf16))).sum())


# (N, D, what it reaches); K = LOSS_K throughout; the _bnres form where D <= 1024
LOSS_K = 37
LOSS_CASES = [
    (1, 8, "one row, one slab; 255 of 256 threads idle"),
    (1, 2048, "one row at the widest _bn width: one row group, every thread busy"),
    (63, 96, "one slab short of full; 12 column groups, 21 row groups, 252 threads"),
    (63, 1024, "the widest _bnres width: its constants fill the whole reduction buffer; two row groups"),
    (64, 128, "exactly one slab of 64 rows"),
    (64, 8, "one slab, 256 row groups for 64 rows"),
    (65, 1024, "the 64 / 65 boundary at the widest _bnres width: slabs of 33 and 32 rows"),
    (65, 2048, "the boundary at the widest _bn width"),
    (4097, 96, "65 slabs of 64 rows, one row in the last"),
    (4097, 1024, "65 slabs at the widest _bnres width"),
    (65536 + 65, 8, "above 65 536 rows the slabs grow: 1010 slabs of 65 rows"),
    (65536 + 65, 128, "... at the model's width"),
]
LOSS_BAD_INDICES = (-1, "K", 2 ** 32 + 3, -2 ** 40)


def make_loss_inputs(N, D):
    """z fp32, the codebook, indices with a few outside [0, K) (at the first row, the last row and in between, N allowing),
    dz_add in both types, and the sources with z_src = bnres_rows(*src)."""
    K = LOSS_K
    g = torch.Generator().manual_seed(32452843 + 977 * N + D)
    z = torch.randn(N, D, generator=g) + 0.2
    e = torch.randn(K, D, generator=g) * 0.8
    idx = torch.randint(0, K, (N,), generator=g)
    bad = [K if v == "K" else v for v in LOSS_BAD_INDICES]
    for j, p in enumerate(sorted({0, N - 1, N // 2, N // 3})):
        idx[p] = bad[j % len(bad)]
    add = torch.randn(N, D, generator=g) * 1e-3
    x = torch.randn(N, D, generator=g) * 1.3 + 0.4          # the BatchNorm input of the _bn form
    mean, invstd = x.mean(0), 1.0 / torch.sqrt(x.var(0, unbiased=False) + 1e-5)
    src = make_sources(N, D, "gauss", g)
    return types.SimpleNamespace(N=N, D=D, K=K, z=z, e=e, idx=idx, add=add, x=x, mean=mean, invstd=invstd, src=src, z_src=bnres_rows(*src))


# ----------------------------------------------------------------------------------------------------------------------
# EMA update
# ----------------------------------------------------------------------------------------------------------------------
EMA_CASES = [(1, 8), (48, 16), (513, 24), (8192, 256)]          # 8192 x 256 / 256 threads = 8192 blocks > the 2048-block grid
EMA_DECAY, EMA_EPS = 0.99, 1e-5


def make_ema_inputs(K, D):
    """Codes 1, 7, 14, ... have a running count of 0 AND a batch count of 0 (K > 1: the total stays positive); their running sum
    is 0 as it would be -- but for code 1, which keeps a non-zero sum over its tiny denominator."""
    g = torch.Generator().manual_seed(49979687 + 131 * K + D)
    ema_n = torch.rand(K, generator=g) * 20.0 + 0.5
    n = torch.randint(0, 30, (K,), generator=g).float()
    ema_s = torch.randn(K, D, generator=g) * ema_n[:, None]
    s = torch.randn(K, D, generator=g) * n[:, None]
    e = torch.randn(K, D, generator=g)
    dead = torch.zeros(K, dtype=torch.bool)
    if K > 1:
        dead[1::7] = True
        dead[1] = True
        ema_n[dead], n[dead] = 0.0, 0.0
        s[dead] = 0.0
        keep = ema_s[1].clone()
        ema_s[dead] = 0.0
        ema_s[1] = keep
    return types.SimpleNamespace(K=K, D=D, e=e, ema_n=ema_n, ema_s=ema_s, n=n, s=s, dead=dead)


def ema_ref(ema_n, ema_s, n, s, decay=EMA_DECAY, eps=EMA_EPS):
    """-> e64, ema_n64, ema_s64 and their bounds (module docstring)."""
    dec = float(np.float32(decay))
    om = float(np.float32(1.0) - np.float32(decay))
    ep = float(np.float32(eps))
    K = ema_n.numel()
    vn = dec * f64(ema_n) + om * f64(n)
    vs = dec * f64(ema_s) + om * f64(s)
    T = (dec * f64(ema_s)).abs() + (om * f64(s)).abs()
    tot = vn.sum()
    assert float(tot) > 0.0, "a total count of 0 is outside the contract"
    nn = (vn + ep) / (tot + K * ep) * tot
    e = vs / nn[:, None]
    return types.SimpleNamespace(e=e, ema_n=vn, ema_s=vs, b_e=gamma(16) * T / nn[:, None], b_n=gamma(2) * vn, b_s=gamma(2) * T)


assert math.isclose(U32, 5.9604644775390625e-08)
