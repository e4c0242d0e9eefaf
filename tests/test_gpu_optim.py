"""GPU: the optimiser's extensions -- nsg_grad_sumsq and nsg_adamw_step (csrc/optim.hip) over the envelope of
tests/test_gpu_elementwise_envelope.py, FlatAdam's options through both fused train steps, the epoch driver and a checkpoint.

Bounds (none is tuned against the kernels; U = 2^-24):
  neutral step         every option neutral (or clipping with max_norm above the norm: the coefficient is exactly 1): the bits of
                       nsg_adam_step on p, m and v
  sum of squares       (double)g * (double)g is exact and the sum is double (error ~ n 2^-53): |norm - norm64| <= 2 U norm64 covers
                       the one rounding to fp32 with room for the square root; integer gradients with a sum below 2^53: equality
  coefficient          norm + 1e-6, the quotient and the norm's own rounding: |coef - coef64| <= 4 U coef64
  m, v                 against torch.optim.AdamW on CPU doubles fed (g * grad_scale) * the kernel's own coefficient: the existing
                       Adam check's 4 U relative + the smallest normal, unchanged (gradients of one sign per element, as there)
  p                    that check's U |p64| + 8 U |update64|, plus U |p64| where a segment decays (the decay rounds once at |p|)
  shadow               against s0 - omd (s0 - p') in doubles, p' the stored parameter and omd the same float:
                       U |s64| + 3 U |omd (s0 - p')| (the difference, the product and the final subtraction round once each)
  guard                p, m, v and the shadow bit-unchanged, finite flag 0, skipped count + 1
  end to end           fused step against autograd + clip_grad_norm_ + torch.optim.AdamW + a hand-rolled shadow: the bound
                       tests/test_gpu_model.py puts on parameters after a fused and an autograd step, rtol 0 and atol 5e-6, held
                       here over three steps and for the shadow too, on the elements whose gradient is above 1e-5 in every step
                       and outside the biases in front of a BatchNorm (Adam turns a round-off-sized gradient into a step of
                       +-lr: that file's rule).  A purely relative 1e-4 is not a bound a correct step can keep: a weight that
                       three steps of ~1e-3 carry across zero is a difference of nearly equal numbers.  Measured: every
                       |fused - autograd| of both models <= 2.4e-7, and in the VQ-VAE case 1 element of 2304 in encoder.4.block.1.weight, at
                       |p| = 1.5e-5 with a difference of 3.5e-9, is 2.4e-4 of its own size (each tensor's figures are printed)"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import ops, optim  # noqa: E402
from neural_sound_generation_amd.optim import FlatAdam  # noqa: E402
from tests.test_gpu_elementwise_envelope import DEV, GRID, TINY32, U32, assert_bits, gpu, mis, within  # noqa: E402

LENGTHS = [1, 3, 1001, 4096, GRID + 77, 4 * (GRID + 300)]
STEPS = (1, 2, 3, 10000)
VIEWS = pytest.mark.parametrize("view", [False, True], ids=["aligned", "from-element-1"])
LR, B1, B2, EPS = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))          # as the C ABI receives them


def f32(x):
    return float(np.float32(x))


def same(t):
    return t


# ----------------------------------------------------------------------------------------------------------------------
# bit identity with the plain step
# ----------------------------------------------------------------------------------------------------------------------
@VIEWS
@pytest.mark.parametrize("n", LENGTHS)
def test_neutral_adamw_step_gives_adam_steps_bits(n, view):
    """Three states from the same start: adam_step; adamw_step with every option neutral; adamw_step with the sum of squares,
    the statistics block and a max_norm far above the norm (coefficient exactly 1.0f, and multiplying by it is exact)."""
    gen = torch.Generator().manual_seed(n)
    f = mis if view else same
    p0 = torch.randn(n, generator=gen) * 1.1
    states = [[f(gpu(p0)), f(torch.zeros(n, device=DEV)), f(torch.zeros(n, device=DEV))] for _ in range(3)]
    stats = ops.new_adamw_stats(DEV)
    for step, gs in zip(STEPS, (1.0, 0.25, 1.0, 0.25)):
        grad = f(gpu(torch.randn(n, generator=gen) * 10.0 ** (-1.0 - 5.0 * torch.rand(n, generator=gen))))
        ops.adam_step(states[0][0], grad, states[0][1], states[0][2], step, grad_scale=gs)
        ops.adamw_step(states[1][0], grad, states[1][1], states[1][2], step, grad_scale=gs)
        ops.adamw_step(states[2][0], grad, states[2][1], states[2][2], step, grad_scale=gs, sumsq=ops.grad_sumsq(grad), max_norm=1e30,
                       skip_nonfinite=True, stats=stats)
        for k in (1, 2):
            for a, b, name in zip(states[0], states[k], "pmv"):
                assert_bits(b, a, f"n={n} step={step} variant {k}: {name}")
        norm, coef, finite, skipped = ops.read_adamw_stats(stats)
        assert coef == 1.0 and finite == 1 and skipped == 0 and norm > 0


def test_default_flat_adam_takes_the_old_entry_point(monkeypatch):
    calls = {"adam": 0, "adamw": 0, "sumsq": 0}
    real = {"adam": ops.adam_step, "adamw": ops.adamw_step, "sumsq": ops.grad_sumsq}

    def counted(name):
        def fn(*a, **k):
            calls[name] += 1
            return real[name](*a, **k)
        return fn
    monkeypatch.setattr(ops, "adam_step", counted("adam"))
    monkeypatch.setattr(ops, "adamw_step", counted("adamw"))
    monkeypatch.setattr(ops, "grad_sumsq", counted("sumsq"))
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(33, 7, device=DEV)), torch.nn.Parameter(torch.randn(50, device=DEV))]
    opt = FlatAdam(ps, lr=1e-3)
    opt.flat_grad.normal_()
    opt.step()
    opt.step(grad_scale=0.5)
    assert calls == {"adam": 2, "adamw": 0, "sumsq": 0}
    assert opt.stats() == {"grad_norm": None, "clip_coef": None, "skipped_steps": 0, "lr": 1e-3}
    # each option leaves it; the norm is taken only where clipping or the guard needs it
    for kw, sumsq in ((dict(weight_decay=0.01), 0), (dict(weight_ema_decay=0.9), 0), (dict(lr_schedule=optim.noam_learning_rate_decay(4)), 0),
                      (dict(max_grad_norm=1.0), 1), (dict(skip_nonfinite=True), 1)):
        for k in calls:
            calls[k] = 0
        o = FlatAdam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1e-3, **kw)
        o.flat_grad.normal_()
        o.step()
        assert calls == {"adam": 0, "adamw": 1, "sumsq": sumsq}, kw
    # a decay assigned to the group after construction (the usual torch idiom) reaches the device table at the next step
    for k in calls:
        calls[k] = 0
    o = FlatAdam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1e-3)
    assert o.plain and o.seg_wd is None
    o.param_groups[0]["weight_decay"] = 0.25
    o.flat_grad.normal_()
    o.step()
    assert calls == {"adam": 0, "adamw": 1, "sumsq": 0} and not o.plain and o.seg_wd.tolist() == [0.25, 0.0]


# ----------------------------------------------------------------------------------------------------------------------
# sum of squares
# ----------------------------------------------------------------------------------------------------------------------
@VIEWS
@pytest.mark.parametrize("n", LENGTHS)
def test_grad_sumsq(n, view):
    gen = torch.Generator().manual_seed(n + 1)
    f = mis if view else same
    g = f(gpu(torch.randn(n, generator=gen) * 10.0 ** (-4.0 * torch.rand(n, generator=gen))))
    a, b = ops.grad_sumsq(g), ops.grad_sumsq(g)
    assert a.dtype == torch.float64 and a.is_cuda and a.data_ptr() != b.data_ptr()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "two runs on the same input differ"
    norm64 = float(g.double().cpu().pow(2).sum().sqrt())
    norm = float(np.float32(np.sqrt(float(a))))
    print(f"n={n}: norm {norm!r} norm64 {norm64!r} error / bound {abs(norm - norm64) / (2 * U32 * norm64):.3f}")
    assert abs(norm - norm64) <= 2 * U32 * norm64
    # integer gradients: every product and every partial sum is an integer below 2^53, so the double is exact
    gi = torch.randint(-2000, 2001, (n,), generator=gen)
    want = int((gi * gi).sum())
    assert want < 2 ** 53
    out = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    assert ops.grad_sumsq(f(gpu(gi.float())), out=out) is out and float(out) == float(want)


# ----------------------------------------------------------------------------------------------------------------------
# the full step restated in fp64
# ----------------------------------------------------------------------------------------------------------------------
def _segments(case):
    """(n, segment lengths, decay per segment)."""
    if case == "S=1":
        return [4096], [f32(0.01)]
    if case == "S=2":
        return [64, 128 * 9], [0.0, f32(0.1)]
    if case == "grid":                                   # the 16-byte path with a grid stride, the boundary inside the second pass
        n = 4 * (GRID + 300)
        return [64 * 50000, n - 64 * 50000], [f32(0.003), f32(0.1)]
    lens = [(64, 128, 64 * 5, 64 * 17)[i % 4] for i in range(300)]       # a block of 1024 floats spans up to 16 segments
    wds = [(0.0, f32(0.01), f32(0.1), f32(0.003), f32(0.05))[i % 5] for i in range(300)]
    return lens, wds


def _adamw64(p0, m0, v0, gs, step, lr, lens, wds):
    """One torch.optim.AdamW step on CPU doubles, one parameter per segment, one group per decay -> (p64, m64, v64)."""
    ps = [torch.nn.Parameter(t.clone()) for t in p0.split(lens)]
    groups = {}
    for p, wd in zip(ps, wds):
        groups.setdefault(wd, []).append(p)
    opt = torch.optim.AdamW([dict(params=v, weight_decay=k) for k, v in groups.items()], lr=lr, betas=(B1, B2), eps=EPS)
    for p, g, m, v in zip(ps, gs.split(lens), m0.split(lens), v0.split(lens)):
        p.grad = g.clone()
        opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    return (torch.cat([p.detach() for p in ps]), torch.cat([opt.state[p]["exp_avg"] for p in ps]),
            torch.cat([opt.state[p]["exp_avg_sq"] for p in ps]))


# (the 4 M-element case costs a second per combination on the host: two of the four)
FULL = [(c, gs, clip) for c in ("S=1", "S=2", "S=300", "S=300-from-element-1") for gs in (1.0, 0.25) for clip in ("below", "above")] + [
    ("grid", 1.0, "below"), ("grid", 0.25, "above")]


@pytest.mark.parametrize("case,grad_scale,clip", FULL)
def test_full_step_against_adamw_in_fp64(case, grad_scale, clip):
    """Each step on its own, from the kernel's fp32 state of the step before (the existing Adam check's scheme and gradients:
    magnitudes 10^-1 .. 10^-6, one sign per element for all steps).  max_norm is 0.37 or 2 times the step's own norm."""
    lens, wds = _segments(case.replace("-from-element-1", ""))
    view = case.endswith("from-element-1")
    n, f = sum(lens), (mis if view else same)
    gen = torch.Generator().manual_seed(n + int(100 * grad_scale) + len(clip))
    p, m, v = f(gpu(torch.randn(n, generator=gen) * 1.1)), f(torch.zeros(n, device=DEV)), f(torch.zeros(n, device=DEV))
    shadow = f(gpu(torch.randn(n, generator=gen)))
    seg_end = gpu(torch.tensor(lens, dtype=torch.int64).cumsum(0))
    seg_wd = gpu(torch.tensor(wds, dtype=torch.float32))
    wd_el = torch.repeat_interleave(torch.tensor(wds, dtype=torch.float64), torch.tensor(lens))
    omd = f32(1.0 - 0.999)
    stats, sumsq = ops.new_adamw_stats(DEV), torch.zeros(1, dtype=torch.float64, device=DEV)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    for step in STEPS:
        grad = sign * 10.0 ** (-1.0 - 5.0 * torch.rand(n, generator=gen))
        gin = f(gpu(grad / grad_scale))          # (1 and 0.25: exact)
        g64 = gin.double().cpu()
        norm64 = grad_scale * float(g64.pow(2).sum().sqrt())
        max_norm = f32((0.37 if clip == "below" else 2.0) * norm64)
        p0, m0, v0, s0 = (t.double().cpu() for t in (p, m, v, shadow))
        ops.grad_sumsq(gin, out=sumsq)
        ops.adamw_step(p, gin, m, v, step, lr=LR, beta1=B1, beta2=B2, eps=EPS, grad_scale=grad_scale, seg_end=seg_end, seg_wd=seg_wd,
                       sumsq=sumsq, max_norm=max_norm, skip_nonfinite=True, shadow=shadow, one_minus_decay=omd, stats=stats)
        norm, coef, finite, skipped = ops.read_adamw_stats(stats)
        what = f"{case} step={step} grad_scale={grad_scale} clip={clip}"
        coef64 = min(1.0, max_norm / (norm64 + 1e-6))
        print(f"{what}: norm {norm!r} / {norm64!r}, coef {coef!r} / {coef64!r}")
        assert (finite, skipped) == (1, 0), what
        assert abs(norm - norm64) <= 2 * U32 * norm64, what
        assert abs(coef - coef64) <= 4 * U32 * coef64, what
        assert (coef == 1.0) if clip == "above" else (0.3 < coef < 0.4), what
        gs = g64 * grad_scale * coef                                              # the kernel's own coefficient
        p64, m64, v64 = _adamw64(p0, m0, v0, gs, step, LR, lens, wds)
        within("adamw m, v", m, m64, 4 * U32 * m64.abs() + TINY32, what + " m")
        within("adamw m, v", v, v64, 4 * U32 * v64.abs() + TINY32, what + " v")
        upd64 = p0 * (1.0 - LR * wd_el) - p64
        within("adamw p", p, p64, U32 * p64.abs() + 8 * U32 * upd64.abs() + U32 * p64.abs() * (wd_el != 0), what + " p")
        pk = p.double().cpu()
        d64 = omd * (s0 - pk)
        within("adamw shadow", shadow, s0 - d64, U32 * (s0 - d64).abs() + 3 * U32 * d64.abs(), what + " shadow")


@VIEWS
@pytest.mark.parametrize("n", LENGTHS)
def test_shadow_with_decay_zero_is_the_parameters(n, view):
    gen = torch.Generator().manual_seed(n)
    f = mis if view else same
    p, m, v = f(gpu(torch.randn(n, generator=gen) * 1e-3)), f(torch.zeros(n, device=DEV)), f(torch.zeros(n, device=DEV))
    shadow = f(gpu(torch.randn(n, generator=gen) * 1e4))
    for step in (1, 2, 3):
        ops.adamw_step(p, f(gpu(torch.randn(n, generator=gen))), m, v, step, shadow=shadow, one_minus_decay=1.0)
        assert_bits(shadow, p, f"decay 0, step {step}")


# ----------------------------------------------------------------------------------------------------------------------
# the non-finite guard
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")], ids=["inf", "-inf", "nan"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@VIEWS
@pytest.mark.parametrize("n", LENGTHS)
def test_guard_leaves_everything_untouched(n, view, where, bad):
    """(At n = 1 first, middle and last are the one element: those three cases repeat one another.)"""
    gen = torch.Generator(device=DEV).manual_seed(n)
    f = mis if view else same
    p, m, v, shadow = (f(torch.randn(n, generator=gen, device=DEV)) for _ in range(4))
    v.abs_()
    before = [t.clone() for t in (p, m, v, shadow)]
    grad = f(torch.randn(n, generator=gen, device=DEV))
    seg_end, seg_wd = gpu(torch.tensor([n], dtype=torch.int64)), gpu(torch.tensor([0.01]))
    stats = ops.new_adamw_stats(DEV)
    args = dict(lr=LR, seg_end=seg_end, seg_wd=seg_wd, max_norm=1.0, skip_nonfinite=True, shadow=shadow, one_minus_decay=0.1, stats=stats)
    ops.adamw_step(p, grad, m, v, 1, sumsq=ops.grad_sumsq(grad), **args)          # a finite step first: everything moves
    assert ops.read_adamw_stats(stats)[2:] == (1, 0)
    for t, b in zip((p, m, v, shadow), before):
        assert not torch.equal(t, b)
    before = [t.clone() for t in (p, m, v, shadow)]
    grad[{"first": 0, "middle": n // 2, "last": n - 1}[where]] = bad
    for k in (1, 2):
        ops.adamw_step(p, grad, m, v, 1 + k, sumsq=ops.grad_sumsq(grad), **args)
        norm, coef, finite, skipped = ops.read_adamw_stats(stats)
        assert finite == 0 and skipped == k and not np.isfinite(norm)
        for t, b, name in zip((p, m, v, shadow), before, ("p", "m", "v", "shadow")):
            assert_bits(t, b, f"guard n={n} {where} {bad}: {name}")


# ----------------------------------------------------------------------------------------------------------------------
# FlatAdam: data-parallel identity in one process
# ----------------------------------------------------------------------------------------------------------------------
def _opt(seed=0, **kw):
    torch.manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in ((40, 33), (70,), (8, 3, 4, 4), (5,))]
    kw = dict(dict(lr=1e-3, weight_decay=0.01, max_grad_norm=0.5, skip_nonfinite=True, weight_ema_decay=0.99,
                   lr_schedule=optim.noam_learning_rate_decay(2)), **kw)
    return FlatAdam(ps, **kw)


def test_data_parallel_identity_in_one_process():
    """Two shards' buckets summed + step(grad_scale = 1/2) against one step on the averaged gradient: the same bits, and the
    reported norm is the averaged gradient's."""
    a, b = _opt(), _opt()
    gen = torch.Generator(device=DEV).manual_seed(3)
    for step in range(1, 4):
        shards = []
        for _ in range(2):
            g = torch.zeros_like(a.flat_grad)
            for p, off in zip(a._params, a.offsets):
                g[off:off + p.numel()].normal_(generator=gen)
            shards.append(g)
        a.flat_grad.copy_(shards[0] + shards[1])
        b.flat_grad.copy_((shards[0] + shards[1]) * 0.5)
        a.step(grad_scale=0.5)
        b.step()
        for name in ("flat_param", "exp_avg", "exp_avg_sq", "shadow"):
            assert_bits(getattr(a, name), getattr(b, name), f"step {step}: {name}")
        sa, sb = a.stats(), b.stats()
        norm64 = float(b.flat_grad.double().cpu().pow(2).sum().sqrt())
        assert sa == sb and abs(sa["grad_norm"] - norm64) <= 2 * U32 * norm64 and sa["clip_coef"] < 1.0 and sa["skipped_steps"] == 0
        assert sa["lr"] == pytest.approx(1e-3 * optim.noam_learning_rate_decay(2)(step), rel=1e-15)
    # a reserved tail (the EMA codebook's statistics behind the gradients) stays outside the norm
    tail = a.reserve_tail(100)
    tail.fill_(1e6)
    a.flat_grad.copy_(b.flat_grad)
    a.step()
    b.step()
    assert a.stats() == b.stats() and torch.equal(a.flat_param, b.flat_param)
    # a NaN gradient: skipped, counted, the host's step count still advances
    before = a.flat_param.clone(), a.shadow.clone()
    a.flat_grad[7] = float("nan")
    a.step()
    st = a.stats()
    assert st["skipped_steps"] == 1 and not np.isfinite(st["grad_norm"]) and a.step_count == b.step_count + 1
    assert torch.equal(a.flat_param, before[0]) and torch.equal(a.shadow, before[1])


# ----------------------------------------------------------------------------------------------------------------------
# end to end, tiny shapes
# ----------------------------------------------------------------------------------------------------------------------
WD, DECAY, WARMUP = 0.01, 0.9, 2


def _options(max_norm):
    return dict(lr=1e-3, weight_decay=WD, max_grad_norm=max_norm, skip_nonfinite=True, weight_ema_decay=DECAY,
                lr_schedule=optim.noam_learning_rate_decay(WARMUP))


def _autograd_run(model, loss_fn, no_decay, max_norm, steps=3):
    """clip_grad_norm_ + torch.optim.AdamW (ndim < 2 and no_decay exempt) + the shadow of src/dataloader.py:254-257 by hand
    -> (parameters, shadow, per-step |gradient|, per-step coefficient)."""
    params = list(model.parameters())
    exempt = {id(p) for p in params if p.ndim < 2} | {id(p) for p in no_decay}
    opt = torch.optim.AdamW([dict(params=[p for p in params if id(p) not in exempt], weight_decay=WD),
                             dict(params=[p for p in params if id(p) in exempt], weight_decay=0.0)], lr=1e-3)
    shadow = [p.detach().clone() for p in params]
    sched = optim.noam_learning_rate_decay(WARMUP)
    gmin, coefs = None, []
    for step in range(1, steps + 1):
        opt.zero_grad()
        loss_fn(model).backward()
        norm = torch.nn.utils.clip_grad_norm_(params, float("inf"))
        coefs.append(min(1.0, max_norm / (float(norm) + 1e-6)))
        g = [p.grad.detach().abs().clone() for p in params]
        gmin = g if gmin is None else [torch.minimum(a, b) for a, b in zip(gmin, g)]
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        for group in opt.param_groups:
            group["lr"] = 1e-3 * sched(step)
        opt.step()
        with torch.no_grad():
            for s, p in zip(shadow, params):
                s.sub_((1.0 - DECAY) * (s - p))
    return params, shadow, gmin, coefs


def _compare(names, fused_opt, params, shadow, gmin, skip=lambda k: False):
    compared = 0
    for i, (k, off) in enumerate(zip(names, fused_opt.offsets)):
        if skip(k):
            continue
        n = params[i].numel()
        big = (gmin[i].reshape(-1) > 1e-5).cpu().numpy()
        compared += int(big.sum())
        for what, got, want in (("parameter", fused_opt.flat_param, params[i]), ("shadow", fused_opt.shadow, shadow[i])):
            got, want = got[off:off + n].cpu().numpy()[big], want.detach().reshape(-1).cpu().numpy()[big]
            if got.size:
                err = np.abs(got - want)
                print(f"{k} {what}: max |fused - autograd| {float(err.max()):.3e}, max relative "
                      f"{float((err / np.maximum(np.abs(want), 1e-30)).max()):.3e} over {got.size} of {n}")
            np.testing.assert_allclose(got, want, rtol=0, atol=5e-6, err_msg=f"{k} {what}")
    print(f"compared {compared} of {fused_opt.total} bucket elements")
    assert compared >= 1000


def _norm_of_first_gradient(model, loss_fn):
    loss_fn(model).backward()
    return float(torch.nn.utils.clip_grad_norm_(list(model.parameters()), float("inf")))


def test_fused_vqvae_step_with_every_option(golden_dir, tmp_path):
    from neural_sound_generation_amd import evaluate as E
    from neural_sound_generation_amd.train import FusedTrainStep, vqvae_loss_terms
    from tests.test_gpu_model import build, golden, is_noise_bias
    g = golden(golden_dir, "model_tiny.npz")
    c = torch.from_numpy(g["s0.c"]).to(DEV)

    def loss_fn(model):
        l3 = vqvae_loss_terms(c, *model(c))
        return l3[0] + l3[1] + l3[2]
    max_norm = 0.5 * _norm_of_first_gradient(build(g).train(), loss_fn)          # so that the first step, at least, is clipped
    ma = build(g).train()
    params, shadow, gmin, coefs = _autograd_run(ma, loss_fn, [ma.codebook.embedding.weight], max_norm)
    assert coefs[0] == pytest.approx(0.5, rel=1e-3)

    def fresh():
        m = build(g).train()
        opt = FlatAdam(m.parameters(), no_decay=[m.codebook.embedding.weight], **_options(max_norm))
        return m, FusedTrainStep(m, beta=1.0, optimizer=opt)
    runs = []
    for _ in range(2):
        m, st = fresh()
        seen = []
        for _ in range(3):
            st.step(c)
            seen.append(st.opt.stats())
        runs.append((m, st, seen))
    m1, s1, seen = runs[0]
    print("fused coefficients", [s["clip_coef"] for s in seen], "autograd", coefs)
    for s, want, step in zip(seen, coefs, (1, 2, 3)):
        assert s["clip_coef"] == pytest.approx(want, rel=1e-4) and s["skipped_steps"] == 0
        assert s["lr"] == pytest.approx(1e-3 * optim.noam_learning_rate_decay(WARMUP)(step), rel=1e-15)
    names = [k for k, _ in m1.named_parameters()]
    assert s1.opt.no_decay == [i for i, (k, p) in enumerate(m1.named_parameters()) if p.ndim < 2 or k == "codebook.embedding.weight"]
    _compare(names, s1.opt, params, shadow, gmin, skip=is_noise_bias)
    for name in ("flat_param", "exp_avg", "exp_avg_sq", "shadow"):                # two fused runs: the same bits
        assert_bits(getattr(runs[1][1].opt, name), getattr(s1.opt, name), "second fused run: " + name)
    assert not torch.equal(s1.opt.shadow, s1.opt.flat_param)
    # a checkpoint after step 2, resumed: step 3 bit for bit, the shadow included; it still loads into torch's optimisers
    m2, s2 = fresh()
    for _ in range(2):
        s2.step(c)
    path = str(tmp_path / "ckpt.pth.tar")
    E.save_checkpoint(None, E.checkpoint_state(2, "vqvae", m2, s2.opt), filename=path)
    m3, s3 = fresh()
    s3.opt.shadow.zero_()
    st = E.load_checkpoint(path, m3, s3.opt, map_location=DEV)
    assert st["epoch"] == 2 and s3.opt.step_count == 2 and torch.equal(s3.opt.shadow, s2.opt.shadow)
    s3.step(c)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m3.state_dict().items()):
        assert torch.equal(a, b), f"{k} differs after checkpoint resume"
    for name in ("exp_avg", "exp_avg_sq", "shadow"):
        assert_bits(getattr(s3.opt, name), getattr(s1.opt, name), "resumed: " + name)
    topt = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in m2.parameters()])
    topt.load_state_dict(torch.load(path, weights_only=True)["optimizer"])
    assert topt.param_groups[0]["weight_decay"] == WD
    # a checkpoint of the plain optimiser (what the code before these options wrote) loads; the average restarts from its weights
    m4 = build(g).train()
    s4 = FusedTrainStep(m4, lr=1e-3, beta=1.0)
    s4.step(c)
    E.save_checkpoint(None, E.checkpoint_state(1, "vqvae", m4, s4.opt), filename=path)
    assert set(torch.load(path, weights_only=True)["optimizer"]) == {"state", "param_groups"}
    m5, s5 = fresh()
    E.load_checkpoint(path, m5, s5.opt, map_location=DEV)
    assert s5.opt.step_count == 1 and torch.equal(s5.opt.flat_param, s4.opt.flat_param) and torch.equal(s5.opt.shadow, s4.opt.flat_param)
    assert s5.opt.param_groups[0]["weight_decay"] == 0 and s5.opt.seg_end is None


def test_fused_prior_step_with_every_option(golden_dir, tmp_path):
    from neural_sound_generation_amd import evaluate as E
    from neural_sound_generation_amd.prior_train import PriorTrainStep
    from tests.test_gpu_prior import build
    from tests.test_gpu_prior_train import _ragged_batch
    g = np.load(os.path.join(golden_dir, "prior_tiny.npz"))
    x, label, lengths = (t.to(DEV) for t in _ragged_batch(int(g["cfg"][0]), int(g["cfg"][3])))

    def loss_fn(model):
        return model.loss(x, label, lengths)
    max_norm = 0.5 * _norm_of_first_gradient(build(g)[0], loss_fn)
    ma = build(g)[0]
    params, shadow, gmin, coefs = _autograd_run(ma, loss_fn, [], max_norm)
    assert coefs[0] == pytest.approx(0.5, rel=1e-3)

    def fresh():
        m = build(g)[0]
        return m, PriorTrainStep(m, optimizer=FlatAdam(m.parameters(), **_options(max_norm)))
    runs = []
    for _ in range(2):
        m, st = fresh()
        seen = []
        for _ in range(3):
            st.step(x, label, lengths)
            seen.append(st.opt.stats())
        runs.append((m, st, seen))
    m1, s1, seen = runs[0]
    print("fused coefficients", [s["clip_coef"] for s in seen], "autograd", coefs)
    for s, want in zip(seen, coefs):
        assert s["clip_coef"] == pytest.approx(want, rel=1e-4) and s["skipped_steps"] == 0
    _compare([k for k, _ in m1.named_parameters()], s1.opt, params, shadow, gmin)
    for name in ("flat_param", "exp_avg", "exp_avg_sq", "shadow"):
        assert_bits(getattr(runs[1][1].opt, name), getattr(s1.opt, name), "second fused run: " + name)
    m2, s2 = fresh()
    for _ in range(2):
        s2.step(x, label, lengths)
    path = str(tmp_path / "prior.pth.tar")
    E.save_checkpoint(None, E.checkpoint_state(2, "pixelcnn", m2, s2.opt), filename=path)
    m3, s3 = fresh()
    s3.opt.shadow.zero_()
    E.load_checkpoint(path, m3, s3.opt, map_location=DEV)
    s3.step(x, label, lengths)
    for name in ("flat_param", "exp_avg", "exp_avg_sq", "shadow"):
        assert_bits(getattr(s3.opt, name), getattr(s1.opt, name), "resumed: " + name)


def test_run_epoch_evaluates_with_the_averaged_weights(tmp_path, monkeypatch):
    from neural_sound_generation_amd import data as Dm, epoch as Ep, evaluate as E, models as M
    monkeypatch.chdir(tmp_path)
    root = str(tmp_path / "ljs")
    # no utterance is longer than max_time_steps: the collate function crops none at a random offset, so every pass over the
    # test loader sees the same batches and the losses of two passes can be compared for equality
    Dm.write_synthetic_data_root(root, n_utts=40, min_frames=48, max_frames=64, with_audio=False, seed=11)
    loaders = Dm.get_data_loaders(root, batch_size=4, max_time_steps=64 * Dm.HOP_SIZE, num_workers=0, frame_multiple=4)
    torch.manual_seed(1)
    model = M.VQVAE(1, 16, 32).to(DEV)
    opt = FlatAdam(model.parameters(), no_decay=[model.codebook.embedding.weight], **_options(1.0))

    class A:
        model, dataset, dim, z_dim, beta, log_interval, sampledir = "vqvae", "ljspeech", 16, 32, 1.0, 1000, str(tmp_path / "samples")
    inside = {}
    real = Ep.test_vqvae

    def spying(*a, **k):
        inside["averaged"], inside["raw"] = opt.flat_param.clone(), opt.shadow.clone()      # (swapped while the block is open)
        return real(*a, **k)
    monkeypatch.setattr(Ep, "test_vqvae", spying)
    r = Ep.run_epoch(A(), model, opt, loaders["train"], loaders["test"], DEV, 1, export_audio=False, eval_with_ema=True)
    monkeypatch.setattr(Ep, "test_vqvae", real)
    assert_bits(opt.flat_param, inside["raw"], "the raw weights after the epoch")
    assert_bits(opt.shadow, inside["averaged"], "the averaged weights after the epoch")
    assert not torch.equal(inside["raw"], inside["averaged"])
    with opt.ema_weights():
        by_hand = E.test_vqvae(A(), model, loaders["test"], DEV, 1)
    raw = E.test_vqvae(A(), model, loaders["test"], DEV, 1)
    assert (r["test_loss_recons"], r["test_loss_vq"]) == tuple(by_hand) and tuple(by_hand) != tuple(raw)
    assert_bits(opt.flat_param, inside["raw"], "the raw weights after ema_weights()")
    # the checkpoint holds the raw weights, and the averaged ones in the optimiser's state
    saved = torch.load(r["checkpoint"], weights_only=True, map_location=DEV)
    for k, p in model.named_parameters():
        assert torch.equal(saved["state_dict"][k], p), k
    for s, p, off in zip(saved["optimizer"]["weight_ema"]["shadow"], opt._params, opt.offsets):
        assert torch.equal(s.reshape(-1), opt.shadow[off:off + p.numel()])
    with pytest.raises(ValueError):
        Ep.run_epoch(A(), model, torch.optim.Adam(model.parameters()), [], loaders["test"], DEV, 2, export_audio=False, eval_with_ema=True)
