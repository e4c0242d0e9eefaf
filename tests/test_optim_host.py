"""CPU: the host side of FlatAdam's options -- the stock learning-rate schedules against their closed forms, the segment table
of the decoupled weight decay, and the state dict (shadow included) with its interchange with torch.optim.AdamW."""
import math

import pytest
import torch

from neural_sound_generation_amd import optim
from neural_sound_generation_amd.optim import FlatAdam


def _params(seed=0):
    torch.manual_seed(seed)
    shapes = [(5, 3), (7,), (2, 3, 4, 4), (70,), (9, 8), ()]
    return [torch.nn.Parameter(torch.randn(s)) for s in shapes]


# ---- schedules ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 7, 4000])
def test_noam_schedule_matches_its_closed_form(w):
    f = optim.noam_learning_rate_decay(warmup_steps=w)
    for s in (1, w, w + 1, 10 * w):
        want = w ** 0.5 * min(s * w ** -1.5, s ** -0.5)
        assert f(s) == pytest.approx(want, rel=1e-15), s
    assert f(w) == pytest.approx(1.0, rel=1e-15)                                 # the peak is the group's lr itself
    assert f(1) == pytest.approx(1.0 / w, rel=1e-15) and f(10 * w) == pytest.approx(10 ** -0.5, rel=1e-15)
    assert f(4 * w) == pytest.approx(0.5, rel=1e-15)
    assert optim.noam_learning_rate_decay().__call__(4000) == pytest.approx(1.0)  # the default is the preset's 4000 steps


@pytest.mark.parametrize("rate,interval", [(0.5, 50000), (0.1, 7), (1.0, 1)])
def test_step_schedule_matches_its_closed_form(rate, interval):
    f = optim.step_learning_rate_decay(anneal_rate=rate, anneal_interval=interval)
    for s in (1, interval - 1, interval, interval + 1, 10 * interval, 10 * interval + 3):
        assert f(max(s, 1)) == rate ** (max(s, 1) // interval), s
    assert optim.step_learning_rate_decay()(49999) == 1.0 and optim.step_learning_rate_decay()(100000) == 0.25


@pytest.mark.parametrize("w,total,floor", [(10, 110, 0.0), (4, 20, 0.1), (0, 8, 0.0)])
def test_warmup_cosine_matches_its_closed_form(w, total, floor):
    f = optim.warmup_cosine(w, total, floor=floor)
    for s in (1, max(w, 1), w + 1, (w + total) // 2, total, 10 * total):
        if s <= w:
            want = s / w
        else:
            want = floor + (1 - floor) * 0.5 * (1 + math.cos(math.pi * min(1.0, (s - w) / (total - w))))
        assert f(s) == pytest.approx(want, rel=1e-15, abs=1e-18), s
    if w:
        assert f(w) == 1.0 and f(1) == 1.0 / w
    assert f(total) == pytest.approx(floor, abs=1e-16) and f(10 * total) == pytest.approx(floor, abs=1e-16)
    for bad in ((5, 5), (6, 5), (-1, 5)):
        with pytest.raises(ValueError):
            optim.warmup_cosine(*bad)


def test_schedule_multiplies_the_groups_lr():
    opt = FlatAdam(_params(), lr=2e-3, lr_schedule=optim.noam_learning_rate_decay(8))
    assert opt._lr_now(1) == pytest.approx(2e-3 / 8) and opt._lr_now(8) == pytest.approx(2e-3) and opt._lr_now(32) == pytest.approx(1e-3)
    assert not opt.plain and FlatAdam(_params(), lr=2e-3).plain
    assert FlatAdam(_params())._lr_now(5) == 1e-3
    assert "lr_schedule" not in str(opt.state_dict().keys())                      # code is not checkpointed


# ---- the segment table ----------------------------------------------------------------------------------------------
def test_segment_table_offsets_and_exempt_tensors():
    ps = _params()
    opt = FlatAdam(ps, weight_decay=0.01)
    assert opt.offsets == [0, 64, 128, 256, 384, 512] and opt.total == 576      # every view starts on a multiple of 64 floats
    ends, wds = opt.segment_table()
    assert ends == [64, 128, 256, 384, 512, 576] and ends == opt.seg_end.tolist()
    assert all(e % 64 == 0 for e in ends) and ends == sorted(ends) and ends[-1] == opt.total
    assert opt.no_decay == [1, 3, 5]                                              # the default rule: ndim < 2
    assert wds == [0.01, 0.0, 0.01, 0.0, 0.01, 0.0]
    assert opt.seg_end.dtype == torch.int64 and opt.seg_wd.dtype == torch.float32
    assert torch.equal(opt.seg_wd, torch.tensor(wds, dtype=torch.float32))
    # no_decay adds to the default rule (the codebook is 2-D)
    ps = _params()
    opt = FlatAdam(ps, weight_decay=0.02, no_decay=[ps[4]])
    assert opt.no_decay == [1, 3, 4, 5] and opt.segment_table()[1] == [0.02, 0.0, 0.02, 0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        FlatAdam(_params(), weight_decay=0.02, no_decay=[torch.zeros(3, 3)])      # not one of the parameters
    # without decay there is no table at all, whatever no_decay lists
    ps = _params()
    opt = FlatAdam(ps, no_decay=[ps[0]])
    assert opt.seg_end is None and opt.seg_wd is None and opt.plain
    for bad in (dict(weight_decay=-1.0), dict(max_grad_norm=0.0), dict(max_grad_norm=-2.0), dict(weight_ema_decay=1.5),
                dict(weight_ema_decay=-0.1)):
        with pytest.raises(ValueError):
            FlatAdam(_params(), **bad)


def test_options_switch_the_plain_path_off_one_by_one():
    for kw in (dict(weight_decay=0.01), dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(weight_ema_decay=0.999),
               dict(lr_schedule=optim.step_learning_rate_decay())):
        assert not FlatAdam(_params(), **kw).plain, kw
    opt = FlatAdam(_params(), weight_ema_decay=0.999)
    assert torch.equal(opt.shadow, opt.flat_param) and opt.shadow.data_ptr() != opt.flat_param.data_ptr()
    assert opt.stats() == {"grad_norm": None, "clip_coef": None, "skipped_steps": 0, "lr": 1e-3}
    with pytest.raises(RuntimeError):
        with FlatAdam(_params()).ema_weights():
            pass


def test_ema_weights_swaps_and_swaps_back_even_on_an_exception():
    ps = _params()
    opt = FlatAdam(ps, weight_ema_decay=0.9)
    raw = opt.flat_param.clone()
    opt.shadow.mul_(0.5)
    avg = opt.shadow.clone()
    versions = [p._version for p in ps]
    with opt.ema_weights():
        assert torch.equal(opt.flat_param, avg) and torch.equal(opt.shadow, raw)
        assert torch.equal(ps[0], avg[:15].view(5, 3))                            # the parameters alias the bucket
        assert all(p._version > v for p, v in zip(ps, versions))
    assert torch.equal(opt.flat_param, raw) and torch.equal(opt.shadow, avg)
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("inside")
    assert torch.equal(opt.flat_param, raw) and torch.equal(opt.shadow, avg)


# ---- state dict -----------------------------------------------------------------------------------------------------
def _fill(opt, steps=3):
    g = torch.Generator().manual_seed(5)
    opt.step_count = steps
    for p, off in zip(opt._params, opt.offsets):                                  # (the padding between the views stays zero)
        opt.exp_avg[off:off + p.numel()].copy_(torch.randn(p.numel(), generator=g))
        opt.exp_avg_sq[off:off + p.numel()].copy_(torch.rand(p.numel(), generator=g))
        if opt.shadow is not None:
            opt.shadow[off:off + p.numel()].copy_(torch.randn(p.numel(), generator=g))


def test_state_dict_round_trip_with_the_shadow():
    ps = _params()
    a = FlatAdam(ps, lr=2e-3, weight_decay=0.03, no_decay=[ps[0]], weight_ema_decay=0.99, max_grad_norm=1.0, skip_nonfinite=True,
                 lr_schedule=optim.noam_learning_rate_decay(10))
    _fill(a)
    sd = a.state_dict()
    assert set(sd) == {"state", "param_groups", "no_decay", "weight_ema"}
    assert sd["param_groups"][0]["weight_decay"] == 0.03 and sd["no_decay"] == [0, 1, 3, 5] and sd["weight_ema"]["decay"] == 0.99
    assert [tuple(t.shape) for t in sd["weight_ema"]["shadow"]] == [tuple(p.shape) for p in ps]
    b = FlatAdam(_params(1), lr=1e-3, weight_ema_decay=0.5)
    b.load_state_dict(sd)
    g = b.param_groups[0]
    assert (g["lr"], g["weight_decay"], b.step_count, b.no_decay) == (2e-3, 0.03, 3, [0, 1, 3, 5])
    assert b.weight_ema_decay == 0.5                                              # the constructor's decay wins; the shadow is data
    for name in ("exp_avg", "exp_avg_sq", "shadow", "seg_end", "seg_wd"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert b.seg_wd.tolist() == [0.0, 0.0, pytest.approx(0.03), 0.0, pytest.approx(0.03), 0.0]
    # an optimiser built without the average takes the checkpoint's, decay included
    c = FlatAdam(_params(2))
    c.load_state_dict(sd)
    assert c.weight_ema_decay == 0.99 and torch.equal(c.shadow, a.shadow)
    # a checkpoint of the plain optimiser (the layout before the options existed): the shadow restarts from the weights
    old = FlatAdam(_params(3))
    _fill(old)
    sd_old = old.state_dict()
    assert set(sd_old) == {"state", "param_groups"} and sd_old["param_groups"][0]["weight_decay"] == 0
    d = FlatAdam(_params(4), weight_decay=0.01, weight_ema_decay=0.9)
    d.shadow.zero_()
    d.load_state_dict(sd_old)
    assert d.param_groups[0]["weight_decay"] == 0 and d.seg_end is None and d.step_count == 3
    assert torch.equal(d.shadow, d.flat_param) and torch.equal(d.exp_avg, old.exp_avg)
    bad = a.state_dict()
    bad["weight_ema"]["shadow"] = bad["weight_ema"]["shadow"][:-1]
    with pytest.raises(ValueError):
        FlatAdam(_params()).load_state_dict(bad)


def test_state_dict_survives_a_tensors_only_load(tmp_path):
    """evaluate.load_checkpoint reads with weights_only=True: the extra keys must be tensors and plain values."""
    a = FlatAdam(_params(), weight_decay=0.03, weight_ema_decay=0.99)
    _fill(a)
    path = str(tmp_path / "opt.pt")
    torch.save({"optimizer": a.state_dict()}, path)
    sd = torch.load(path, weights_only=True)["optimizer"]
    b = FlatAdam(_params(1), weight_ema_decay=0.99)
    b.load_state_dict(sd)
    assert torch.equal(a.shadow, b.shadow) and torch.equal(a.exp_avg_sq, b.exp_avg_sq) and b.no_decay == a.no_decay


def test_state_dict_written_here_loads_into_torch_adamw():
    ps = _params()
    a = FlatAdam(ps, lr=2e-3, weight_decay=0.03, weight_ema_decay=0.99)
    _fill(a)
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for cls in (torch.optim.AdamW, torch.optim.Adam):
        topt = cls(theirs, lr=1e-3)
        topt.load_state_dict(a.state_dict())                                      # the extra top-level keys are ignored
        g = topt.param_groups[0]
        assert g["lr"] == 2e-3 and g["weight_decay"] == 0.03 and g.get("decoupled_weight_decay", True)
        for i, (p, off) in enumerate(zip(ps, a.offsets)):
            st = topt.state[theirs[i]]
            assert float(st["step"]) == 3.0
            assert torch.equal(st["exp_avg"], a.exp_avg[off:off + p.numel()].view_as(p))
            assert torch.equal(st["exp_avg_sq"], a.exp_avg_sq[off:off + p.numel()].view_as(p))
    for p in theirs:
        p.grad = torch.ones_like(p)
    topt.step()                                                                   # and torch can go on from it


def test_torch_adamw_state_dict_with_weight_decay_loads_here():
    ref = _params()
    topt = torch.optim.AdamW(ref, lr=2e-3, weight_decay=0.01)
    for _ in range(3):
        for p in ref:
            p.grad = torch.randn_like(p)
        topt.step()
    mine = FlatAdam([torch.nn.Parameter(p.detach().clone()) for p in ref], lr=1e-3)
    assert mine.seg_end is None
    mine.load_state_dict(topt.state_dict())
    g = mine.param_groups[0]
    assert g["weight_decay"] == 0.01 and g["lr"] == 2e-3 and mine.step_count == 3 and not mine.plain
    assert mine.segment_table()[1] == [0.01, 0.0, 0.01, 0.0, 0.01, 0.0]            # the default exemptions: torch's dict names none
    assert mine.seg_wd.tolist() == [pytest.approx(w) for w in mine.segment_table()[1]]
    for i, (p, off) in enumerate(zip(ref, mine.offsets)):
        assert torch.equal(mine.exp_avg[off:off + p.numel()].view_as(p), topt.state[p]["exp_avg"])
        assert torch.equal(mine.exp_avg_sq[off:off + p.numel()].view_as(p), topt.state[p]["exp_avg_sq"])


def test_amsgrad_and_coupled_decay_still_raise():
    ref = _params()
    for p in ref:
        p.grad = torch.randn_like(p)
    topt = torch.optim.AdamW(ref, lr=2e-3, weight_decay=0.01, amsgrad=True)
    topt.step()
    with pytest.raises(ValueError, match="amsgrad"):
        FlatAdam(_params()).load_state_dict(topt.state_dict())
    sd = torch.optim.Adam(_params(), weight_decay=0.01).state_dict()              # torch.optim.Adam's decay is L2, added to the gradient
    if "decoupled_weight_decay" in sd["param_groups"][0]:
        with pytest.raises(ValueError, match="coupled"):
            FlatAdam(_params()).load_state_dict(sd)
    sd = torch.optim.Adam(_params()).state_dict()                                 # without decay the flag does not matter
    FlatAdam(_params()).load_state_dict(sd)


def test_step_without_a_gpu_still_refuses():
    opt = FlatAdam(_params(), weight_decay=0.01, max_grad_norm=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
