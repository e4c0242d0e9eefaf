"""GPU tests of the sampler's controls (nsg_prior_walk_ctl through GatedPixelCNN.sample): temperature, top-k, top-p and kept
(primed) codes.  The rule is the one include/nsg.h states; the references here evaluate it in fp64 on the fp32 logits.

Neutral controls are the plain walk bit for bit; known logits are held to the filtered fp64 inverse CDF at and around every
prefix boundary; on the production model top-k is checked exactly and temperature / top-p against the GPU's own logits;
priming is checked by replay; determinism, batch independence, validation and continue_mels close the list."""
import itertools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import models as M  # noqa: E402
from neural_sound_generation_amd.evaluate import continue_mels, sample_mels  # noqa: E402
from neural_sound_generation_amd.prior import GatedPixelCNN  # noqa: E402
from tests.test_gpu_prior_sampling import INPUT_DIM, N_CLASSES, _inverse_cdf, _production  # noqa: E402
from tests.test_gpu_prior_walk_envelope import DEAD, KS, PATTERNS, TIE, _known_logits, _model, _u_grid  # noqa: E402

DEV = "cuda:0"
NEUTRAL = (1.0, 0, 1.0)
NEAR_TIE = 1e-4          # the near-tie criterion of test_gpu_prior_sampling._agree_up_to_near_ties
MARGIN = 1e-4            # a top-p case whose nucleus turns on a candidate mass nearer than this (x S_A) to the goal is not run


# ----------------------------------------------------------------------------------------------------------------------
# the rule in fp64
# ----------------------------------------------------------------------------------------------------------------------
def filter64(l32, T, top_k, top_p):
    """The header's steps 1-3 in fp64 on fp32 logits l32 (..., K): the filtered logits (l - mx) / T with -inf outside the
    kept set N, and per position the distance (as a share of S_A) of the nearest candidate mass from top_p * S_A (inf
    without top-p).  Live codes: scaled logit above -100 (exp(-103.3) is the smallest fp32 can hold; the inputs of these
    tests keep live codes within 30 of the maximum and dead ones 150 or more below it)."""
    assert l32.dtype == torch.float32
    K = l32.shape[-1]
    l = l32.double()
    s = (l - l.amax(-1, keepdim=True)) / T
    keep = s > -100.0
    if top_k >= 1:
        nlive = keep.sum(-1, keepdim=True)
        ranked = torch.where(keep, l, torch.full_like(l, -math.inf)).sort(-1, descending=True).values
        kth = ranked[..., min(top_k, K) - 1:min(top_k, K)]            # the top_k-th largest live logit (-inf: fewer live codes)
        keep = keep & ((l >= kth) | (nlive <= top_k))
    margin = torch.full(l.shape[:-1], math.inf, dtype=torch.float64)
    if top_p < 1:
        p = torch.where(keep, torch.exp(s), torch.zeros_like(s))
        ps = p.sort(-1, descending=True).values
        mass = ps.cumsum(-1)
        goal = top_p * mass[..., -1:]
        first = (mass >= goal).int().argmax(-1, keepdim=True)        # ps[first]: the largest v whose mass of p >= v reaches the goal
        keep = keep & (p >= ps.gather(-1, first))
        last_of_value = torch.cat([ps[..., :-1] != ps[..., 1:], torch.ones_like(ps[..., :1], dtype=torch.bool)], -1) & (ps > 0)
        dist = torch.where(last_of_value, (mass - goal).abs(), torch.full_like(mass, math.inf))
        margin = dist.amin(-1) / mass[..., -1]
    return torch.where(keep, s, torch.full_like(s, -math.inf)), margin


def pick_status(x, filt, u):
    """Per position: 0 where x is the fp64 inverse CDF of the filtered logits filt under u, 1 where it is a near-tie (u * S
    within NEAR_TIE * S of a prefix boundary between the two codes), 2 otherwise or where x has zero probability."""
    y, pre, S = _inverse_cdf(filt, u)
    status = (x != y).long()
    p = torch.exp(filt).gather(-1, x[..., None])[..., 0]
    for idx in torch.nonzero(x != y).tolist():
        idx = tuple(idx)
        lo, hi = sorted((int(x[idx]), int(y[idx])))
        gap = (pre[idx][lo:hi] - float(u[idx]) * float(S[idx])).abs().min()
        if float(gap) > NEAR_TIE * float(S[idx]):
            status[idx] = 2
    status[p < 2.0 ** -149] = 2
    return status


def assert_filtered_inverse_cdf(x, l32, u, T, top_k, top_p, where=None, max_ambiguous=0.05, max_near_clips=3):
    """x (B, H, W) sampled under u from the GPU's own logits l32 (B, H, W, K): at the positions `where` (all by default) x
    is the fp64 filtered inverse CDF or a near-tie of it.  A position is ambiguous if its nucleus differs between
    top_p (1 - 1e-5) and top_p (1 + 1e-5); there either nucleus may serve.  Caps: the ambiguous share, the clips that use the
    near-tie allowance."""
    x, l32, u = x.cpu(), l32.cpu(), u.cpu()
    where = torch.ones_like(x, dtype=torch.bool) if where is None else where.cpu()
    if top_p < 1:
        f_lo, _ = filter64(l32, T, top_k, top_p * (1 - 1e-5))
        f_hi, _ = filter64(l32, T, top_k, top_p * (1 + 1e-5))
        ambiguous = (torch.isfinite(f_lo) != torch.isfinite(f_hi)).any(-1)
        status = torch.minimum(pick_status(x, f_lo, u), pick_status(x, f_hi, u))
    else:
        f, _ = filter64(l32, T, top_k, top_p)
        ambiguous = torch.zeros_like(where)
        status = pick_status(x, f, u)
    share = float((ambiguous & where).sum()) / max(int(where.sum()), 1)
    print(f"T={T} top_k={top_k} top_p={top_p}: ambiguous share {share:.4%}, near-ties {int(((status == 1) & where).sum())}, "
          f"failures {int(((status == 2) & where).sum())} of {int(where.sum())} positions")
    assert share <= max_ambiguous, f"{share:.2%} of the positions have an ambiguous nucleus"
    bad = (status == 2) & where
    assert not bool(bad.any()), (f"{int(bad.sum())} sampled codes are neither the fp64 filtered inverse CDF nor a near-tie "
                                 f"(or have zero probability), first at {torch.nonzero(bad)[0].tolist()}")
    near_clips = int(((status == 1) & where).flatten(1).any(1).sum())
    assert near_clips <= max_near_clips, f"{near_clips} of {x.shape[0]} clips needed the near-tie allowance"


def walk(model, label, shape, u, ctl=NEUTRAL, given=None, keep=None, want_logits=False):
    """The sampler forced through nsg_prior_walk_ctl (GatedPixelCNN.sample takes the plain walk when nothing is set)."""
    B, (H, W) = label.shape[0], shape
    codes = torch.empty((B, H, W), dtype=torch.int64, device=DEV)
    logits = torch.empty((B, H, W, model.embedding.num_embeddings), dtype=torch.float32, device=DEV) if want_logits else None
    with torch.no_grad():
        model._walk_rows(label, B, H, W, u=u, codes=codes, x_in=given, keep=keep, logits=logits, ctl=ctl)
    return (codes, logits) if want_logits else codes


def _inputs(B, H, W, seed, n_classes=N_CLASSES):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_classes, (B,), generator=g).to(DEV), torch.rand(B, H, W, generator=g).to(DEV)


# ----------------------------------------------------------------------------------------------------------------------
# 1. neutral controls are the plain sampler, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["production_64x20x256", "65x32x3_5x4x37"])
def test_neutral_controls_are_the_plain_sampler_bit_for_bit(which):
    if which.startswith("production"):
        (model, _), (B, H, W) = _production(), (64, 20, 256)
    else:
        (model, _), (B, H, W) = _model(65, 32, 3), (5, 4, 37)
    label, u = _inputs(B, H, W, 11)
    plain = model.sample(label, shape=(H, W), batch_size=B, u=u)
    none_kept = torch.zeros((B, H, W), dtype=torch.bool, device=DEV)
    anything = torch.randint(0, model.embedding.num_embeddings, (B, H, W), device=DEV)
    assert torch.equal(walk(model, label, (H, W), u), plain), "nsg_prior_walk_ctl with neutral controls differs from nsg_prior_walk"
    assert torch.equal(walk(model, label, (H, W), u, given=anything, keep=none_kept), plain), "an all-false keep changes the codes"
    # the public dispatch: neutral values, and top_k >= input_dim, are the plain sampler
    assert torch.equal(model.sample(label, shape=(H, W), batch_size=B, u=u, temperature=1.0, top_k=0, top_p=1.0), plain)
    if W < 256:
        assert torch.equal(model.sample(label, shape=(H, W), batch_size=B, u=u, top_k=10 ** 6), plain)
        assert torch.equal(model.sample(label, shape=(H, W), batch_size=B, u=u, given=anything, keep=none_kept), plain)


# ----------------------------------------------------------------------------------------------------------------------
# 2. known logits
# ----------------------------------------------------------------------------------------------------------------------
TEMPERATURES = [0.5, 0.8, 1.25, 2.0]
TOP_KS = [0, 1, 7, 64]
TOP_PS = [1.0, 0.9, 0.5]
CONTROLS = list(itertools.product(TEMPERATURES, TOP_KS, TOP_PS))      # the full product: 48 settings per (K, pattern)


def _logits_for(pattern, K, T):
    """The envelope test's known logits; at T = 0.5 the live ones halved (drawn from [-10, 0]), so that after the division
    by T every live code stays within 30 of the maximum, where `live` means the same to the kernel and to the reference."""
    l = _known_logits(pattern, K)
    if T == 0.5:
        l = np.where(l > DEAD, l * np.float32(0.5), np.float32(DEAD)).astype(np.float32)
    s = (l.astype(np.float64) - float(l.max())) / T
    assert ((s >= -30) | (s <= -140)).all()
    return l


def _filtered_distribution(l, T, top_k, top_p):
    """Of fp32 logits l under the controls: the kept codes N (indices), the filtered fp64 logits, the prefix boundaries
    (bnd[m] separates kept codes N[m - 1] and N[m]; bnd[0] = 0, bnd[-1] = S), S and the top-p margin."""
    filt, margin = filter64(torch.from_numpy(l), T, top_k, top_p)
    N = np.nonzero(torch.isfinite(filt).numpy())[0]
    _, pre, S = _inverse_cdf(filt, torch.zeros(1))
    return N, filt, np.concatenate([[0.0], pre.numpy()[N]]), float(S), float(margin)


def check_filtered_inverse_cdf(N_, filt, bnd, S, u_b, u_reg, c, what):
    """check_inverse_cdf of tests/test_gpu_prior_walk_envelope.py, assertion for assertion, against the filtered distribution."""
    u_all = np.concatenate([u_b, u_reg])
    n, K = len(u_all), filt.shape[-1]
    y64 = _inverse_cdf(filt, torch.from_numpy(u_all))[0].numpy()
    out = ~np.isin(c, N_)
    assert not out.any(), f"{what}: {int(out.sum())} of {n} codes picked lie outside the kept set, e.g. u = {u_all[out][0]!r} -> code {c[out][0]}"
    order = np.argsort(u_all, kind="stable")
    assert (np.diff(c[order]) >= 0).all(), f"{what}: the code decreases as u grows"
    assert c[u_all == 0][0] == N_[0], f"{what}: u = 0 does not give the first kept code"
    if S - bnd[-2] > 2 * TIE * S:
        assert c[u_all == u_all.max()][0] == N_[-1], f"{what}: the largest u does not give the last kept code"
    t = u_all.astype(np.float64) * S
    lo = np.searchsorted(bnd, t - TIE * S, "left")
    hi = np.searchsorted(bnd, t + TIE * S, "right")
    far = lo == hi
    bad = far & (c != y64)
    assert not bad.any(), f"{what}: {int(bad.sum())} codes away from every boundary differ from the fp64 inverse CDF, e.g. u = {u_all[bad][0]!r}"
    ordinal = np.searchsorted(N_, c)
    ok = (ordinal >= np.maximum(lo - 1, 0)) & (ordinal <= np.minimum(hi - 1, len(N_) - 1))
    bad = ~far & ~ok
    assert not bad.any(), f"{what}: {int(bad.sum())} codes near a boundary are not a kept code beside it, e.g. u = {u_all[bad][0]!r}"
    reg = slice(len(u_b), n)
    cum_got = np.cumsum(np.bincount(c[reg], minlength=K))
    cum_want = np.cumsum(np.bincount(y64[reg], minlength=K))
    assert np.abs(cum_got - cum_want).max() <= 1, f"{what}: the regular grid's counts differ from the fp64 intervals' by more than one"


def test_the_margin_filter_leaves_out_at_most_one_percent_of_the_top_p_cases():
    """The input filter of the known-logits test: a top-p case is run only if, in fp64, every candidate mass is at least
    1e-4 S_A away from top_p S_A (about 100x the fp32 summation error of <= 1024 terms), so the kernel's order of summation
    cannot decide its nucleus.  At most 1 % of the top-p cases may be left out."""
    run = left_out = 0
    for K, pattern, (T, top_k, top_p) in itertools.product(KS, PATTERNS, CONTROLS):
        if top_p < 1:
            run += 1
            if _filtered_distribution(_logits_for(pattern, K, T), T, top_k, top_p)[4] < MARGIN:
                left_out += 1
                print("left out:", (K, pattern, T, top_k, top_p))
    assert run == len(KS) * len(PATTERNS) * len(TEMPERATURES) * len(TOP_KS) * 2
    assert left_out <= 0.01 * run, f"{left_out} of {run} top-p cases left out"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_controlled_sampling_is_the_filtered_inverse_cdf_of_known_logits(pattern, K):
    """Logits = output_conv[2]'s bias.  Under every (temperature, top_k, top_p) of the product, with u at and 1..4 ulps around
    every fp64 prefix boundary of the FILTERED distribution and on the regular 16384-grid: no code outside the kept set;
    codes non-decreasing in u; u = 0 gives the first kept code; farther than 2^-16 S from every boundary the fp64 pick
    exactly, nearer a kept code beside the boundary; the grid's counts within one.  `equal` keeps all K codes under any
    top_k (ties are kept); `one_hot` returns its code under every setting."""
    torch.set_num_threads(16)
    torch.manual_seed(K)
    model = GatedPixelCNN(K, 16, 1, N_CLASSES)
    with torch.no_grad():
        model.output_conv[2].weight.zero_()
    model = model.to(DEV)
    lab = torch.randint(0, N_CLASSES, (1,), generator=torch.Generator().manual_seed(K + 1)).to(DEV)
    u_reg = ((np.arange(16384) + 0.5) / 16384).astype(np.float32)
    ran = 0
    for T, top_k, top_p in CONTROLS:
        what = f"K={K} {pattern} T={T} top_k={top_k} top_p={top_p}"
        l = _logits_for(pattern, K, T)
        N_, filt, bnd, S, margin = _filtered_distribution(l, T, top_k, top_p)
        if margin < MARGIN:                                     # counted and capped by the test above
            continue
        if pattern == "equal":
            assert len(N_) == K, what
        if pattern == "one_hot":
            assert len(N_) == 1, what
        with torch.no_grad():
            model.output_conv[2].bias.copy_(torch.from_numpy(l))
        u_b = _u_grid(bnd[1:] / S)
        n = len(u_b) + len(u_reg)
        H, W = 2, 64
        B = -(-n // (H * W))
        u = np.full(B * H * W, 0.5, np.float32)
        u[:n] = np.concatenate([u_b, u_reg])
        codes = model.sample(lab.repeat(B), shape=(H, W), batch_size=B, u=torch.from_numpy(u).view(B, H, W).to(DEV),
                             temperature=T, top_k=top_k, top_p=top_p)
        c = codes.reshape(-1)[:n].cpu().numpy()
        if pattern == "equal":
            assert len(np.unique(c)) == K, f"{what}: {len(np.unique(c))} of {K} equally likely codes returned"
        check_filtered_inverse_cdf(N_, filt, bnd, S, u_b, u_reg, c, what)
        ran += 1
    assert ran >= len(CONTROLS) - 2


# ----------------------------------------------------------------------------------------------------------------------
# 3. exact top-k facts on the production model
# ----------------------------------------------------------------------------------------------------------------------
def test_top_k_is_exact_on_the_production_model():
    model, _ = _production()
    B, H, W = 4, 20, 64
    label, u = _inputs(B, H, W, 3)
    for top_k in (1, 32):
        x, walked = walk(model, label, (H, W), u, ctl=(1.0, top_k, 1.0), want_logits=True)
        assert torch.equal(x, model.sample(label, shape=(H, W), batch_size=B, u=u, top_k=top_k))
        l32 = model.incremental_logits(x, label)
        assert torch.equal(walked.view(torch.int32), l32.view(torch.int32)), "the sampling walk's logits are not the teacher-forced ones"
        ranked = l32.sort(-1, descending=True).values
        if top_k == 1:
            unique_max = ranked[..., 0] > ranked[..., 1]
            assert float(unique_max.float().mean()) > 0.9
            assert torch.equal(x[unique_max], l32.argmax(-1)[unique_max]), "top_k = 1 is not the argmax where the maximum is unique"
            tied = l32.gather(-1, x[..., None])[..., 0] == ranked[..., 0]
            assert bool(tied.all()), "top_k = 1 returned a code below the maximum"
        else:
            assert bool((l32.gather(-1, x[..., None])[..., 0] >= ranked[..., top_k - 1]).all()), "a sampled code lies below the 32nd largest logit"


# ----------------------------------------------------------------------------------------------------------------------
# 4. temperature and top-p on the production model, against the GPU's own logits
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,top_k,top_p", [(0.7, 0, 1.0), (1.0, 0, 0.9), (0.7, 32, 0.5), (1.3, 0, 0.5)])
def test_temperature_and_top_p_on_the_production_model(T, top_k, top_p):
    torch.set_num_threads(16)
    model, _ = _production()
    B, H, W = 4, 20, 64
    label, u = _inputs(B, H, W, 4)
    x = model.sample(label, shape=(H, W), batch_size=B, u=u, temperature=T, top_k=top_k, top_p=top_p)
    assert_filtered_inverse_cdf(x, model.incremental_logits(x, label), u, T, top_k, top_p)


# ----------------------------------------------------------------------------------------------------------------------
# 5. priming
# ----------------------------------------------------------------------------------------------------------------------
def _masks(B, H, W, seed):
    rows = torch.zeros((B, H, W), dtype=torch.bool)
    rows[:, :3] = True
    cols = torch.zeros((B, H, W), dtype=torch.bool)
    cols[:, :, :17] = True
    rand = torch.rand((B, H, W), generator=torch.Generator().manual_seed(seed)) < 0.5
    return {"rows": rows.to(DEV), "columns": cols.to(DEV), "random": rand.to(DEV)}


def test_priming_keeps_everything_or_nothing():
    model, _ = _production()
    B, H, W = 4, 20, 64
    label, u = _inputs(B, H, W, 5)
    given = torch.randint(0, INPUT_DIM, (B, H, W), generator=torch.Generator().manual_seed(50)).to(DEV)
    everything = torch.ones((B, H, W), dtype=torch.bool, device=DEV)
    x, walked = walk(model, label, (H, W), u, given=given, keep=everything, want_logits=True)
    assert torch.equal(x, given)
    assert torch.equal(walked.view(torch.int32), model.incremental_logits(given, label).view(torch.int32))
    assert torch.equal(model.sample(label, shape=(H, W), batch_size=B, u=u, given=given, keep=everything, temperature=0.7, top_p=0.5), given)
    assert torch.equal(model.sample(label, shape=(H, W), batch_size=B, u=u, given=given, keep=~everything),
                       model.sample(label, shape=(H, W), batch_size=B, u=u))


@pytest.mark.parametrize("ctl", [NEUTRAL, (0.8, 64, 0.95)], ids=["neutral", "controls"])
def test_priming_replays_a_draw(ctl):
    """Keeping any part of a draw and sampling the rest under the same u and controls returns the draw: every position sees
    the inputs it saw before."""
    model, _ = _production()
    B, H, W = 4, 20, 64
    label, u = _inputs(B, H, W, 6)
    controls = dict(temperature=ctl[0], top_k=ctl[1], top_p=ctl[2])
    a = model.sample(label, shape=(H, W), batch_size=B, u=u, **controls)
    for name, m in _masks(B, H, W, 60).items():
        again = model.sample(label, shape=(H, W), batch_size=B, u=u, given=a, keep=m, **controls)
        assert torch.equal(again, a), f"keep = {name}: {int((again != a).sum())} codes moved"
        scrambled = torch.where(m, a, (a + 1) % INPUT_DIM)      # what is not kept is not read
        assert torch.equal(model.sample(label, shape=(H, W), batch_size=B, u=u, given=scrambled, keep=m, **controls), a), name


def test_priming_with_other_codes_holds_them_and_samples_the_rest():
    torch.set_num_threads(16)
    model, _ = _production()
    B, H, W = 4, 20, 64
    label, u = _inputs(B, H, W, 7)
    given = torch.randint(0, INPUT_DIM, (B, H, W), generator=torch.Generator().manual_seed(70)).to(DEV)
    m = _masks(B, H, W, 0)["columns"]
    x = model.sample(label, shape=(H, W), batch_size=B, u=u, given=given, keep=m)
    assert torch.equal(x[m], given[m])
    assert not torch.equal(x, model.sample(label, shape=(H, W), batch_size=B, u=u)), "the kept codes did not change the rest"
    assert_filtered_inverse_cdf(x, model.incremental_logits(x, label), u, *NEUTRAL, where=~m)


def test_continue_codes():
    model, _ = _production()
    B, H, W0, width = 3, 20, 9, 24
    label, u = _inputs(B, H, width, 8)
    prefix = torch.randint(0, INPUT_DIM, (B, H, W0), generator=torch.Generator().manual_seed(80)).to(DEV)
    out = model.continue_codes(prefix, label, width, u=u, temperature=0.9, top_k=100)
    assert tuple(out.shape) == (B, H, width) and out.dtype == torch.int64
    assert torch.equal(out[:, :, :W0], prefix)
    keep = torch.zeros((B, H, width), dtype=torch.bool, device=DEV)
    keep[:, :, :W0] = True
    given = torch.zeros((B, H, width), dtype=torch.int64, device=DEV)
    given[:, :, :W0] = prefix
    assert torch.equal(out, model.sample(label, shape=(H, width), batch_size=B, u=u, given=given, keep=keep, temperature=0.9, top_k=100))
    assert torch.equal(model.continue_codes(prefix, label, W0), prefix)
    drawn = model.continue_codes(prefix, label, width, generator=torch.Generator(device=DEV).manual_seed(1))
    assert torch.equal(drawn[:, :, :W0], prefix) and int(drawn.min()) >= 0 and int(drawn.max()) < INPUT_DIM


# ----------------------------------------------------------------------------------------------------------------------
# 6. determinism and batch independence with controls and a mask on
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["production_64x20x256", "1000x128x3_5x4x37"])
def test_determinism_and_batch_independence_with_controls_and_a_mask(which):
    if which.startswith("production"):
        (model, _), (B, H, W), alone = _production(), (64, 20, 256), (0, 31, 63)
    else:
        (model, _), (B, H, W), alone = _model(1000, 128, 3), (5, 4, 37), range(5)
    K = model.embedding.num_embeddings
    label, u = _inputs(B, H, W, 9)
    g = torch.Generator().manual_seed(90)
    given = torch.randint(0, K, (B, H, W), generator=g).to(DEV)
    keep = (torch.rand((B, H, W), generator=g) < 0.3).to(DEV)
    controls = dict(temperature=0.8, top_k=64, top_p=0.95)
    a = model.sample(label, shape=(H, W), batch_size=B, u=u, given=given, keep=keep, **controls)
    assert torch.equal(a, model.sample(label, shape=(H, W), batch_size=B, u=u, given=given, keep=keep, **controls)), "two calls differ"
    assert torch.equal(a[keep], given[keep]) and int(a.min()) >= 0 and int(a.max()) < K
    assert not torch.equal(a, model.sample(label, shape=(H, W), batch_size=B, u=u, given=given, keep=keep)), "the controls changed nothing"
    for c in alone:
        one = model.sample(label[c:c + 1], shape=(H, W), batch_size=1, u=u[c:c + 1], given=given[c:c + 1], keep=keep[c:c + 1], **controls)
        assert torch.equal(one[0], a[c]), f"clip {c}: sampled alone differs from its row in the batch"


# ----------------------------------------------------------------------------------------------------------------------
# 7. validation
# ----------------------------------------------------------------------------------------------------------------------
def test_controls_and_priming_are_validated():
    model, _ = _model(65, 32, 3)
    B, H, W = 2, 3, 5
    label, u = _inputs(B, H, W, 10)
    args = dict(shape=(H, W), batch_size=B, u=u)
    for bad in (dict(temperature=0.0), dict(temperature=-0.5), dict(temperature=math.nan), dict(temperature=math.inf),
                dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5)):
        with pytest.raises(ValueError):
            model.sample(label, **args, **bad)
    given = torch.zeros((B, H, W), dtype=torch.int64, device=DEV)
    keep = torch.ones((B, H, W), dtype=torch.bool, device=DEV)
    for bad in (dict(given=given), dict(keep=keep), dict(given=given[:, :, :4], keep=keep), dict(given=given, keep=keep[:1]),
                dict(given=given.int(), keep=keep), dict(given=given, keep=keep.long()),
                dict(given=given - 1, keep=keep), dict(given=given + 65, keep=keep)):
        with pytest.raises(ValueError):
            model.sample(label, **args, **bad)
    out_of_range_but_not_kept = model.sample(label, **args, given=given + 65, keep=~keep)
    assert torch.equal(out_of_range_but_not_kept, model.sample(label, **args))
    with pytest.raises(ValueError):
        model.continue_codes(torch.zeros((B, H, W + 1), dtype=torch.int64, device=DEV), label, W)
    narrow = GatedPixelCNN(32, 12, 2, 4).to(DEV)                  # dim % 16 != 0: outside the walk's envelope
    lab = torch.tensor([0, 3], device=DEV)
    with pytest.raises(NotImplementedError):
        narrow.sample(lab, shape=(3, 4), batch_size=2, temperature=0.8, top_k=5, top_p=0.9)
    with pytest.raises(NotImplementedError):
        narrow.sample(lab, shape=(3, 4), batch_size=2, u=torch.rand(2, 3, 4, device=DEV), top_k=5)
    with pytest.raises(NotImplementedError):
        narrow.continue_codes(torch.zeros((2, 3, 2), dtype=torch.int64, device=DEV), lab, 4)


# ----------------------------------------------------------------------------------------------------------------------
# 8. mels
# ----------------------------------------------------------------------------------------------------------------------
def test_continue_mels_and_sample_mels_controls():
    torch.manual_seed(2)
    vqvae = M.VQVAE(1, 32, 64).to(DEV).eval()
    prior = GatedPixelCNN(64, 16, 2, 4).to(DEV)
    B, keep_frames, frames = 3, 18, 48
    label = torch.tensor([0, 2, 3], device=DEV)
    mel = torch.rand(B, 1, 80, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    codes, out = continue_mels(vqvae, prior, mel, label, keep_frames, frames, generator=torch.Generator(device=DEV).manual_seed(7),
                               temperature=0.9, top_p=0.9)
    assert tuple(codes.shape) == (B, 20, frames // 4) and codes.dtype == torch.int64
    assert tuple(out.shape) == (B, 1, 80, frames)
    with torch.no_grad():
        known = vqvae.encode(mel)
        assert torch.equal(codes[:, :, :keep_frames // 4], known[:, :, :keep_frames // 4])
        assert torch.equal(out, vqvae.decode(codes))
    with pytest.raises(ValueError):
        continue_mels(vqvae, prior, mel, label, 36, frames)                  # more frames kept than the mel has
    a, mel_a = sample_mels(vqvae, prior, label, frames, generator=torch.Generator(device=DEV).manual_seed(1), top_k=1)
    b, mel_b = sample_mels(vqvae, prior, label, frames, generator=torch.Generator(device=DEV).manual_seed(2), top_k=1)
    assert torch.equal(a, b) and torch.equal(mel_a, mel_b), "top_k = 1 depends on the random numbers"
