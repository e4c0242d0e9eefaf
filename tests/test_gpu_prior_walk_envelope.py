"""GPU tests of the incremental sampler's column walk (nsg_prior_walk) across the envelope include/nsg.h states: dim % 16 == 0
and <= 128, any input_dim <= 1024, any n_layers >= 1 whose 4-clip state fits the LDS.  The teacher-forced logits are held to
the fp64 oracle at widths that are not powers of two, at input_dim not a multiple of 4 (the head's padding), at 1024 (the
k-slice buffer exactly full), at one layer and at the deepest model admitted, with partly filled 4-clip workgroups.  The
pick of the code is held to the fp64 inverse CDF of known logits at and around every prefix boundary: a code of zero
probability is never returned."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import ops  # noqa: E402
from neural_sound_generation_amd._lib import NsgError  # noqa: E402
from neural_sound_generation_amd.prior import GatedPixelCNN  # noqa: E402
from tests.test_gpu_prior_sampling import _close, _fp64_logits, _inverse_cdf  # noqa: E402

DEV = "cuda:0"
N_CLASSES = 10
DEEPEST = None      # n_layers: the deepest model the walk admits at that (input_dim, dim), found by deepest_layers

# (input_dim, dim, n_layers) of the teacher-forced cases (tests/test_abi.py checks the blob size at the same widths)
WIDTHS = [(1, 16, 1), (3, 48, 2), (65, 32, 3), (1000, 96, 4), (1023, 112, 2), (1024, 128, 3), (512, 80, 5),
          (1024, 128, DEEPEST), (512, 64, DEEPEST)]


def deepest_layers(input_dim, dim):
    """The largest n_layers for which nsg_prior_walk_weight_floats is non-zero (the LDS check decides)."""
    assert ops.prior_walk_weight_floats(dim, 1, input_dim) > 0
    for L in range(2, 1024):
        if ops.prior_walk_weight_floats(dim, L, input_dim) == 0:
            return L - 1
    raise AssertionError(f"no depth limit below 1024 layers at input_dim={input_dim}, dim={dim}")


def _model(input_dim, dim, n_layers):
    torch.manual_seed(input_dim * 7 + dim * 3 + n_layers)
    m = GatedPixelCNN(input_dim, dim, n_layers, N_CLASSES)
    st = {k: v.clone() for k, v in m.state_dict().items()}
    return m.to(DEV), st


# 1. teacher-forced logits across the envelope.  Every width runs at B = 5 on 4 x 37 (the layer-0 ring wraps, the second
# workgroup holds one clip); B = 1 and 9 and the grids 1 x 1, 2 x 3 and 5 x 7 appear twice each.
CASES = [w + (5, (4, 37)) for w in WIDTHS] + [
    (1, 16, 1, 1, (1, 1)), (3, 48, 2, 9, (2, 3)), (65, 32, 3, 1, (5, 7)),
    (1023, 112, 2, 9, (1, 1)), (1000, 96, 4, 1, (2, 3)), (512, 80, 5, 9, (5, 7))]


@pytest.mark.parametrize("input_dim,dim,n_layers,B,hw", CASES,
                         ids=[f"{k}x{d}x{'Lmax' if n is None else n}-B{b}-{h}x{w}" for k, d, n, b, (h, w) in CASES])
def test_teacher_forced_logits_across_the_envelope(input_dim, dim, n_layers, B, hw):
    torch.set_num_threads(16)
    L = deepest_layers(input_dim, dim) if n_layers is DEEPEST else n_layers
    model, st = _model(input_dim, dim, L)
    assert model.walk_supported()
    H, W = hw
    g = torch.Generator().manual_seed(input_dim + 1000 * B + H * W)
    x = torch.randint(0, input_dim, (B, H, W), generator=g)
    label = torch.randint(0, N_CLASSES, (B,), generator=g)
    got = model.incremental_logits(x.to(DEV), label.to(DEV)).cpu()
    assert tuple(got.shape) == (B, H, W, input_dim)
    want = _fp64_logits(st, x, label, L)
    for b in range(B):                                          # every clip on its own scale, the idle slots' neighbours included
        _close(got[b], want[b], what=f"clip {b}: incremental vs fp64 oracle")
    with torch.no_grad():
        if input_dim % 4 == 0:
            full = model.forward_nhwc(x.to(DEV), label.to(DEV)).cpu()
            for b in range(B):
                _close(got[b], full[b], what=f"clip {b}: incremental vs forward_nhwc")
        else:                                                   # the fp32 conv path needs C_out % 4 == 0: only the walk serves
            with pytest.raises(NsgError):
                model.forward_nhwc(x.to(DEV), label.to(DEV))
            with pytest.raises(NsgError):
                model.generate(label.to(DEV), shape=(H, W), batch_size=B)


# 2. the envelope's edges: the walk refuses, generate serves where its conv path does
def _assert_walk_refused(model, generate_serves=True):
    model = model.to(DEV)
    assert not model.walk_supported()
    B, H, W = 2, 2, 3
    label = torch.tensor([1, 7], device=DEV)
    with pytest.raises(NotImplementedError):
        model.sample(label, shape=(H, W), batch_size=B)
    with pytest.raises(NotImplementedError):
        model.sample(label, shape=(H, W), batch_size=B, u=torch.rand(B, H, W, device=DEV))
    with pytest.raises(NotImplementedError):
        model.incremental_logits(torch.zeros(B, H, W, dtype=torch.int64, device=DEV), label)
    K = model.embedding.num_embeddings
    if generate_serves:
        s = model.generate(label, shape=(H, W), batch_size=B)
        assert tuple(s.shape) == (B, H, W) and int(s.min()) >= 0 and int(s.max()) < K
    else:
        with pytest.raises(NsgError):
            model.generate(label, shape=(H, W), batch_size=B)


@pytest.mark.parametrize("input_dim,dim", [(1024, 128), (512, 64)], ids=lambda v: str(v))
def test_one_layer_past_the_deepest_is_refused(input_dim, dim):
    L = deepest_layers(input_dim, dim) + 1
    assert ops.prior_walk_weight_floats(dim, L, input_dim) == 0
    torch.manual_seed(L)
    _assert_walk_refused(GatedPixelCNN(input_dim, dim, L, N_CLASSES))


@pytest.mark.parametrize("input_dim,dim", [(64, 8), (64, 20), (64, 136), (1025, 16)], ids=lambda v: str(v))
def test_widths_outside_the_envelope_are_refused(input_dim, dim):
    assert ops.prior_walk_weight_floats(dim, 2, input_dim) == 0
    torch.manual_seed(dim)
    # input_dim 1025: the output conv's C_out % 4 != 0, so generate cannot serve it either
    _assert_walk_refused(GatedPixelCNN(input_dim, dim, 2, N_CLASSES), generate_serves=input_dim % 4 == 0)


# 3. the inverse CDF against known logits.  With output_conv[2]'s weight zero every position's logits are its bias exactly,
# so the u grid can be placed at and around every fp64 prefix boundary of a known distribution.
KS = [1, 3, 65, 100, 512, 1000, 1024]
PATTERNS = ["random", "dead_lanes", "equal", "one_hot"]
DEAD = -300.0            # exp(-300) is 0 in fp32: a code of zero probability
TIE = 2.0 ** -16         # u * S nearer than TIE * S to a prefix boundary may fall on either side of it


def _known_logits(pattern, K):
    """fp32 logits: every code at max or within 20 below it (p > 0), or at DEAD below it (p == 0 in fp32)."""
    rng = np.random.RandomState(K * 10 + PATTERNS.index(pattern))
    if pattern == "equal":
        return np.zeros(K, np.float32)
    if pattern == "one_hot":
        l = np.full(K, DEAD, np.float32)
        l[rng.randint(K)] = 0.0
        return l
    l = rng.uniform(-20.0, 0.0, K).astype(np.float32)
    if pattern == "random":                                     # about half the codes dead, anywhere
        l[rng.rand(K) < 0.5] = DEAD
        if not (l > DEAD).any():
            l[rng.randint(K)] = 0.0
    else:                                                       # dead runs that fill whole lanes of the walk's pick (ceil(K / 64) codes each)
        ck = -(-K // 64)
        lanes = -(-K // ck)
        dead = rng.rand(lanes) < 0.5
        if lanes > 1:
            dead[0], dead[1] = False, True                      # at least one live lane followed by a dead one
        for ln in np.nonzero(dead)[0]:
            l[ln * ck:(ln + 1) * ck] = DEAD
    return l


def _u_grid(bounds):
    """The float32 nearest each boundary fraction and 1..4 ulps either side of it, 0 and the largest float below 1."""
    f = bounds.astype(np.float32)
    vals = [f, np.array([0.0, np.nextafter(np.float32(1), np.float32(0))], np.float32)]
    up = dn = f
    for _ in range(4):
        up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
        vals += [up, dn]
    v = np.concatenate(vals)
    return np.unique(v[(v >= 0) & (v < 1)])


def _fp64_distribution(l):
    """Of fp32 logits l: the live codes (p > 0 in fp32), the fp64 logits with the dead ones at -inf (p exactly 0), the prefix
    boundaries bnd (bnd[m] separates live codes P[m - 1] and P[m]; bnd[0] = 0, bnd[-1] = S) and S."""
    live = l >= l.max() - 30
    P = np.nonzero(live)[0]
    l64 = torch.from_numpy(np.where(live, l.astype(np.float64), -np.inf))
    _, pre, S = _inverse_cdf(l64, torch.zeros(1))
    return P, l64, np.concatenate([[0.0], pre.numpy()[P]]), float(S)


def known_logits_u(l):
    """The u values of the inverse CDF test: the boundary grid (sorted, unique), then the regular grid (m + 1/2) / 16384."""
    _, _, bnd, S = _fp64_distribution(l)
    return _u_grid(bnd[1:] / S), ((np.arange(16384) + 0.5) / 16384).astype(np.float32)


def check_inverse_cdf(l, u_b, u_reg, c):
    """Asserts that the codes c picked under u = [u_b, u_reg] are the inverse CDF of softmax(l) (see the test)."""
    P, l64, bnd, S = _fp64_distribution(l)
    u_all = np.concatenate([u_b, u_reg])
    N, K = len(u_all), len(l)
    y64 = _inverse_cdf(l64, torch.from_numpy(u_all))[0].numpy()
    dead = ~np.isin(c, P)
    assert not dead.any(), (f"{int(dead.sum())} of {N} codes picked have zero probability, e.g. u = {u_all[dead][0]!r} -> code "
                            f"{c[dead][0]} (logit {l[c[dead][0]]} vs max {l.max()})")
    order = np.argsort(u_all, kind="stable")
    assert (np.diff(c[order]) >= 0).all(), "the code decreases as u grows"
    assert c[u_all == 0][0] == P[0], "u = 0 does not give the first code of positive probability"
    if S - bnd[-2] > 2 * TIE * S:                               # the last live code's interval is wider than the tie band
        assert c[u_all == u_all.max()][0] == P[-1], "the largest u does not give the last code of positive probability"
    t = u_all.astype(np.float64) * S
    lo = np.searchsorted(bnd, t - TIE * S, "left")
    hi = np.searchsorted(bnd, t + TIE * S, "right")             # bnd[lo:hi] are the boundaries within TIE * S of u * S
    far = lo == hi
    bad = far & (c != y64)
    assert not bad.any(), f"{int(bad.sum())} codes away from every boundary differ from the fp64 inverse CDF, e.g. u = {u_all[bad][0]!r}"
    ordinal = np.searchsorted(P, c)                             # near boundary m: live code P[m - 1] or P[m]
    ok = (ordinal >= np.maximum(lo - 1, 0)) & (ordinal <= np.minimum(hi - 1, len(P) - 1))
    bad = ~far & ~ok
    assert not bad.any(), f"{int(bad.sum())} codes near a boundary are not a live code beside it, e.g. u = {u_all[bad][0]!r}"
    # the regular grid: each code's share is its fp64 interval's, within one point at each boundary
    reg = slice(len(u_b), N)
    cum_got = np.cumsum(np.bincount(c[reg], minlength=K))
    cum_want = np.cumsum(np.bincount(y64[reg], minlength=K))
    assert np.abs(cum_got - cum_want).max() <= 1, "the regular grid's counts differ from the fp64 intervals' by more than one"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_sampling_is_the_inverse_cdf_of_known_logits(pattern, K):
    """Logits = output_conv[2]'s bias, bit for bit.  Then, under u at and around every fp64 prefix boundary and on a regular
    grid: no code of zero probability; codes non-decreasing in u; u = 0 gives the first live code and the largest u the last;
    away from the boundaries (more than 2^-16 S) the fp64 inverse CDF exactly; near one, a live code on either side of it;
    on the regular grid each code's count is its fp64 interval's within one at each boundary."""
    torch.set_num_threads(16)
    l = _known_logits(pattern, K)
    torch.manual_seed(K)
    model = GatedPixelCNN(K, 16, 1, N_CLASSES)
    with torch.no_grad():
        model.output_conv[2].weight.zero_()
        model.output_conv[2].bias.copy_(torch.from_numpy(l))
    model = model.to(DEV)
    g = torch.Generator().manual_seed(K + 1)
    x = torch.randint(0, K, (2, 2, 5), generator=g).to(DEV)
    lab = torch.randint(0, N_CLASSES, (2,), generator=g).to(DEV)
    got = model.incremental_logits(x, lab).cpu()
    bias_bits = torch.from_numpy(l).view(torch.int32)
    assert torch.equal(got.view(torch.int32), bias_bits.expand(got.shape)), "the teacher-forced logits are not the bias bit for bit"

    u_b, u_reg = known_logits_u(l)
    N = len(u_b) + len(u_reg)
    H, W = 2, 64
    B = -(-N // (H * W))
    u = np.full(B * H * W, 0.5, np.float32)
    u[:N] = np.concatenate([u_b, u_reg])
    codes = model.sample(lab[:1].repeat(B), shape=(H, W), batch_size=B, u=torch.from_numpy(u).view(B, H, W).to(DEV))
    check_inverse_cdf(l, u_b, u_reg, codes.reshape(-1)[:N].cpu().numpy())


# 4. batch independence at a non-production width: a partly filled last workgroup, every clip checked
@pytest.mark.parametrize("B", [5, 9])
def test_batch_independence_at_a_non_production_width(B):
    model, _ = _model(1000, 128, 3)
    H, W = 4, 37
    g = torch.Generator().manual_seed(B)
    label = torch.randint(0, N_CLASSES, (B,), generator=g).to(DEV)
    u = torch.rand(B, H, W, generator=g).to(DEV)
    a = model.sample(label, shape=(H, W), batch_size=B, u=u)
    assert torch.equal(a, model.sample(label, shape=(H, W), batch_size=B, u=u)), "two calls with the same u differ"
    assert int(a.min()) >= 0 and int(a.max()) < 1000
    for b in range(B):
        alone = model.sample(label[b:b + 1], shape=(H, W), batch_size=1, u=u[b:b + 1])
        assert torch.equal(alone[0], a[b]), f"clip {b}: sampled alone differs from its row in the batch"
