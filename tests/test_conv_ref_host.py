"""tests/helpers/conv_ref64.py held to torch.autograd, its case tables held to the conditions the GPU module relies on, and its
comparison rule held to planted errors -- all on the CPU, with the reference alone (tests/test_gpu_conv_envelope.py holds the
kernels to the reference)."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import conv_ref64 as R

PROBES = R.probe_cases()
ROUNDING = R.all_rounding_cases()


def _by(note, bf16=None, cases=PROBES):
    return [L for L in cases if L.note.startswith(note) and (bf16 is None or L.bf16 == bf16)]


# ---- the reference against autograd ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ROUNDING, ids=lambda L: L.tag)
def test_reference_agrees_with_autograd(L):
    """One differentiable fp64 graph per layer kind (ReLU on the input, bias, crop; the skip gradient and the ReLU mask applied by
    hand) against the three reference functions, which linearise around zero."""
    c = R.rounding_inputs(L)
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()  # noqa: E731
    for relu_in in (0, R.RELU_IN):
        x = nchw(c.x).requires_grad_(True)
        w, b = c.w.clone().requires_grad_(True), c.bias.clone().requires_grad_(True)
        xin = F.relu(x) if relu_in else x
        conv = F.conv_transpose2d if L.transposed else F.conv2d
        y = conv(xin, w, b, stride=L.stride, padding=(L.ph, L.pw))[:, :, :L.OH, :L.OW]
        gx, gw, gb = torch.autograd.grad(y, [xin, w, b], nchw(c.dy))
        r = R.forward(L, c.x, c.w, c.bias, relu_in)
        torch.testing.assert_close(nchw(r.y), y.detach(), rtol=1e-12, atol=1e-12)
        assert R.kind(L) in ("conv_c1", "convt_c1") or torch.equal(R.forward(L, c.x, c.w, c.bias, relu_in | R.RELU_OUT).y, r.y.clamp_min(0.0))
        torch.testing.assert_close(R.forward(L, c.x, c.w, c.bias, relu_in | R.TANH_OUT).y, torch.tanh(r.y), rtol=0, atol=0)
        rw = R.wgrad(L, c.x, c.dy, relu_in)
        torch.testing.assert_close(rw.y, gw, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(rw.dbias, gb, rtol=1e-12, atol=1e-12)
        assert rw.K == L.Mp and float(rw.terms.min()) >= 0.0 and bool((rw.terms + 1e-12 >= rw.y.abs()).all())
        if not relu_in:
            rd = R.dgrad(L, c.dy, c.w)
            torch.testing.assert_close(nchw(rd.y), gx, rtol=1e-12, atol=1e-12)
            re = R.dgrad(L, c.dy, c.w, c.add, c.relu_x)
            torch.testing.assert_close(re.y, (rd.y + c.add) * (c.relu_x > 0), rtol=1e-12, atol=1e-12)
            assert re.K == rd.K + 1 and bool((rd.terms + 1e-12 >= rd.y.abs()).all())
    # the chain length is taps x reduced channels where the whole window is inside
    if R.kind(L) == "conv" and L.OH > L.kh and L.OW > L.kw:
        assert R.forward(L, c.x, c.w, c.bias).K == L.kh * L.kw * L.Ci


@pytest.mark.parametrize("L", ROUNDING, ids=lambda L: L.tag)
def test_rounding_cases_have_short_chains(L):
    c = R.rounding_inputs(L)
    ks = [R.forward(L, c.x, c.w, c.bias, f).K for f in R.fwd_flag_sets(L, False)]
    ks += [R.dgrad(L, c.dy, c.w, c.add if R.has_epilogue(L) else None).K]
    rw = R.wgrad(L, c.x, c.dy)
    assert max(ks + [rw.K, rw.Kb]) <= R.MAX_ROUND_K, (L.tag, ks, rw.K, rw.Kb)
    if L.bf16:          # operands as handed over: bf16 values
        for t in (c.x, c.w, c.dy, c.add, c.relu_x):
            assert torch.equal(R.rb(t), t)


# ---- the probes' exactness conditions ------------------------------------------------------------------------------------------------
def _exact(r, what, want=None, terms=None):
    want, terms = r.y if want is None else want, r.terms if terms is None else terms
    assert float(terms.max()) < R.EXACT_SUM, f"{what}: a partial sum may reach 2^24"
    assert torch.equal(want, want.round()), f"{what}: not integer-valued"
    if r.stored_bf16:
        assert float(want.abs().max()) <= R.EXACT_BF16, f"{what}: a bf16-stored output above 256"
        assert torch.equal(R.store(r, want), want)


@pytest.mark.parametrize("L", PROBES, ids=lambda L: L.tag)
def test_probe_is_exact_in_any_order(L):
    """Every partial sum below 2^24 (sum |a b| bounds it in any order), every bf16-stored output an integer of at most 256."""
    c = R.probe_inputs(L)
    for t in (c.x, c.w, c.dy, c.bias, c.add, c.relu_x):
        assert torch.equal(t.bfloat16().double(), t)
    assert bool((c.relu_x == 0).any()) and bool((c.relu_x > 0).any()) and float(c.relu_x.min()) >= 0.0
    for f in R.fwd_flag_sets(L, True):
        _exact(R.forward(L, c.x, c.w, c.bias, f), f"{L.tag} forward flags={f}")
    _exact(R.dgrad(L, c.dy, c.w), f"{L.tag} dgrad")
    if R.has_epilogue(L):
        _exact(R.dgrad(L, c.dy, c.w, c.add, c.relu_x), f"{L.tag} dgrad + add + mask")
    for f in R.wgrad_flag_sets(L):
        r = R.wgrad(L, c.x, c.dy, f)
        _exact(r, f"{L.tag} dw flags={f}")
        _exact(r, f"{L.tag} dbias", r.dbias, r.dbias_terms)


# ---- every boundary is hit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_gather_cases_reach_every_tile_boundary(bf16):
    cases = R.gather_cases(bf16)
    fw = [R.gemm_params(L, "forward") for L in cases]
    assert all(R.patch_kind(p) < 0 for p in fw), "a gemm_gather case goes to the patch kernel"
    rows = {p.M for p in fw}
    assert {1, R.GATHER_BM - 1, R.GATHER_BM, R.GATHER_BM + 1} <= rows
    cm = 8 if bf16 else 4
    for e in R.GATHER_BN:
        assert {e, e + cm} <= {L.Co for L in cases}
    assert {R.gather_tile(L.Co, bf16)[1] for L in cases} == set(R.GATHER_BN)
    assert 2 * R.GATHER_BN[-1] in {L.Co for L in cases}                   # two column tiles
    kc = R.gather_tile(8, bf16)[2]
    assert {kc - cm, kc, kc + cm} <= {L.Ci for L in cases}
    assert (kc, cm) == ((64, 8) if bf16 else (32, 4))
    sq = {(L.kh, L.ph) for L in cases if not L.transposed and L.stride == 1 and L.kh == L.kw and (L.OH, L.OW) == (L.FH, L.FW)}
    assert {(1, 0), (2, 1), (3, 0), (3, 1), (3, 2), (5, 2), (7, 3)} <= sq
    assert any(L.kh != L.kw for L in cases) and any((L.OH, L.OW) != (L.FH, L.FW) for L in cases)
    assert {(L.IH % 2, L.IW % 2) for L in cases if not L.transposed and L.stride == 2 and L.IH > 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(R.kind(L) == "convt" for L in cases)
    assert bf16 or {(L.kh, L.ph) for L in cases if R.kind(L) == "convt_s1"} == {(3, 0), (5, 2)}
    assert {p.mode for p in fw} == {0, 1} and {R.gemm_params(L, "dgrad").mode for L in cases} == {0, 1}


def test_patch_cases_reach_every_dispatch_boundary():
    cases = R.patch_cases()
    fk = lambda L: R.patch_kind(R.gemm_params(L, "forward"))  # noqa: E731
    dk = lambda L: R.patch_kind(R.gemm_params(L, "dgrad"))  # noqa: E731
    pads = {(L.ph, L.pw) for L in cases if fk(L) == 0 and (L.OH, L.OW) == (L.FH, L.FW)}
    assert pads == {(a, b) for a in (0, 1, 2) for b in (0, 1, 2)}
    assert any(fk(L) == 0 and L.ph == 2 and (L.OH, L.OW) == (L.IH, L.IW) for L in cases)              # pad 2, cropped to the input's extent
    th, tw = R.PATCH_TILE
    tiles = {(p.RH, p.RW) for p in (R.gemm_params(L, "forward") for L in _by("patch-tile", cases=cases))}
    assert tiles == {(a, b) for a in (1, th - 1, th, th + 1) for b in (1, tw - 1, tw, tw + 1)}
    assert (R.patch_max_ci(0), R.patch_max_ci(1), R.patch_max_ci(2)) == (448, 256, 256)
    last, first = _by("patch-last", cases=cases)[0], _by("patch-first-gather", cases=cases)[0]
    assert (last.Ci, fk(last)) == (448, 0) and (first.Ci, fk(first)) == (512, -1)
    assert {(L.Ci, fk(L)) for L in _by("patch-s2", cases=cases) if L.note == "patch-s2"} == {(256, 1), (320, -1)}
    assert {(L.Ci, fk(L)) for L in _by("patch-T", cases=cases)} == {(256, 2), (320, -1)}
    assert {1, 2} <= {dk(L) for L in cases} and any(dk(L) == 2 and L.Co == 256 for L in cases)        # the data gradients reach both forms
    assert any(fk(L) == 0 and L.Co == 256 for L in cases)
    for ntn in (1, 2):                                                                                # more tiles than workgroups
        assert any(fk(L) == 0 and L.Co == 128 * ntn and R.patch_tiles(R.gemm_params(L, "forward")) ==
                   R.patch_grid(10 ** 6, ntn) + 1 for L in cases)
    assert R.patch_kind(R.gemm_params(cases[0], "forward"), flags=R.RELU_IN) < 0 and R.patch_kind(R.gemm_params(cases[0], "forward"), out_f32=True) < 0


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_wgrad_cases_reach_every_slab_boundary(bf16):
    cases = R.wgrad_cases(bf16)
    routes = [R.wgrad_route(L) for L in cases]
    assert not any(r.strip for r in routes)
    kp, mr = R.WGRAD_KP, R.WGRAD_MIN_ROWS
    assert {1, kp - 1, kp, kp + 1, mr - 1, mr, mr + 1, 289} <= {L.Mp for L in cases}
    split = {(r.nslab, r.split) for r in routes if r.q.ntaps * r.q.A * r.q.C < R.SPLIT_OUTPUTS and r.nslab >= R.SPLIT_SLABS - 1}
    assert split == {(R.SPLIT_SLABS - 1, 1), (R.SPLIT_SLABS, R.SPLIT_WAYS)}
    assert {r.tile for r in routes} == {(128, 32), (64, 64), (128, 128)}
    # a slab that ends inside a 64-pixel chunk of the bf16 kernel (plan_slabs rounds to 32)
    assert any(r.nslab > 1 and r.rows % R.WGRAD_KPB == R.WGRAD_KP for r in routes)
    assert any(L.transposed for L in cases) and any(not L.transposed for L in cases)                  # NSG_RELU_IN lands on either operand


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_strip_cases_reach_every_chunk_boundary(bf16):
    cases = R.strip_cases(bf16)
    routes = [R.wgrad_route(L) for L in cases]
    assert all(r.strip for r in routes) and not any(R.wgrad_route(L, R.RELU_IN).strip for L in cases)
    for k, s in ((3, 1), (4, 2)):
        mine = [(L, r) for L, r in zip(cases, routes) if (L.kh, L.stride) == (k, s) and not L.transposed]
        ns = R.strip_slabs(k * k, 128, 128)
        assert ns == (80 if k == 3 else 64)
        assert {ns - 1, ns, ns + 1, 2 * ns + 1} <= {r.chunks for L, r in mine if L.note == "strip-chunks"}
        assert any(r.per == 2 for _, r in mine) and any(r.per == 3 for _, r in mine)
        sp = R.strip_len(mine[0][1].q)
        assert sp == (32 if (s == 2 and not bf16) else 64)
        assert {1, sp - 1, sp, sp + 1} <= {r.q.PW for _, r in mine}
    assert {0, 1, 2} <= {L.ph for L in cases if L.kh == 3}
    assert any(r.q.A == 256 for r in routes) and any(r.q.C == 256 for r in routes) and any(L.transposed for L in cases)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_stencil_cases_reach_every_tile_boundary(bf16):
    cases = R.stencil_cases(bf16)
    tw = R.C1_TW
    for kd in ("conv_c1", "convt_c1"):
        mine = [L for L in cases if R.kind(L) == kd]
        lw = {(L.OW if kd == "conv_c1" else L.IW) for L in mine}
        assert {1, tw - 1, tw, tw + 1} <= lw
        C = {(L.Co if kd == "conv_c1" else L.Ci) for L in mine}
        assert C >= ({8, 1024} if bf16 else {4, 8, 36, 1020, 1024})
        assert max(R.c1_tiles(L) for L in mine) > max(R.C1_FWD_BLOCKS, R.C1_WGRAD_BLOCKS)
    for lw in (1, tw - 1, tw, tw + 1):
        assert {L.IW % 2 for L in cases if R.kind(L) == "conv_c1" and L.OW == lw} == {0, 1}
    assert (R.C1_FWD_BLOCKS, R.C1_WGRAD_BLOCKS, R.C1_MAX_C) == (2048, 1024, 1024)


def test_pack_layers_pass_the_job_cap_and_sizes_stay_small():
    layers = R.pack_layers()
    assert len(layers) == 17 and R.pack_jobs(layers) == 34 > R.PACK_MAX_JOBS
    assert {R.kind(L) for L in layers} == {"conv", "convt", "conv_c1", "convt_c1", "convt_s1"}
    for L in PROBES + ROUNDING:            # every tensor under 20 MB as the widest type it takes (fp32)
        assert 4 * max(L.B * L.IH * L.IW * L.Ci, L.B * L.OH * L.OW * L.Co, L.kh * L.kw * L.Ci * L.Co) < 20e6, L.tag
    assert len({L.tag for L in PROBES}) == len(PROBES)


def test_the_flag_constants_are_the_header_s():
    lib = pytest.importorskip("neural_sound_generation_amd._lib")
    assert (R.RELU_IN, R.TANH_OUT, R.OUT_F32, R.RELU_OUT) == (lib.NSG_RELU_IN, lib.NSG_TANH_OUT, lib.NSG_OUT_F32, lib.NSG_RELU_OUT)


# ---- planted errors --------------------------------------------------------------------------------------------------------------
def _rejected_somewhere(cases, plant):
    """plant(c) -> [(got, r, extra kwargs)]: the unplanted output must pass, the planted one must fail on at least one case."""
    hits = 0
    for c in cases:
        for got, r, kw in plant(c):
            assert R.accepts(R.store(r, kw.get("want")), r, c.probe, **kw)[0], f"{c.L.tag}: the exact result is refused"
            hits += not R.accepts(got, r, c.probe, **kw)[0]
    return hits


def _square_cases():
    Ls = [R.layer(1, 5, 33, 128, 128, 3, 1, 1, bf16=True), R.layer(2, 5, 7, 8, 8, 3, 1, 1), R.layer(2, 5, 7, 8, 8, 3, 1, 1, bf16=True)]
    return [R.probe_inputs(L) for L in Ls] + [R.rounding_inputs(L) for L in Ls[1:]]


def test_planted_forward_errors_are_rejected():
    cases = _square_cases()

    def one_product_removed(c):
        r = R.forward(c.L, c.x, c.w, c.bias)
        L = c.L
        ci = int((c.x[0, 0, 0, :] * c.w[0, :, L.ph, L.pw]).abs().argmax())         # output (0, 0, 0, 0) reads x(0, 0, 0, :) through the centre tap
        prod = c.x[0, 0, 0, ci] * c.w[0, ci, L.ph, L.pw]
        assert prod != 0
        less = r.y.clone()
        less[0, 0, 0, 0] -= prod
        return [(R.store(r, less), r, {})]

    def with_weights(change):
        def plant(c):
            r = R.forward(c.L, c.x, c.w, c.bias)
            return [(R.store(r, R.forward(c.L, c.x, change(c.w), c.bias).y), r, {})]
        return plant

    def border_tap_shifted(c):
        """Tap (0, 0) reads one column further left than it should."""
        r = R.forward(c.L, c.x, c.w, c.bias)
        w_rest = c.w.clone()
        w_rest[:, :, 0, 0] = 0.0
        w_tap = c.w - w_rest
        x_shift = torch.zeros_like(c.x)
        x_shift[:, :, 1:, :] = c.x[:, :, :-1, :]
        got = R.forward(c.L, c.x, w_rest, c.bias).y + R.forward(c.L, x_shift, w_tap, None).y
        return [(R.store(r, got), r, {})]

    def bias_twice(c):
        r = R.forward(c.L, c.x, c.w, c.bias)
        return [(R.store(r, r.y + c.bias), r, {})]

    def store_toward_zero(c):
        r = R.forward(c.L, c.x, c.w, c.bias)
        if not r.stored_bf16:
            return []
        down = R.rb(r.y)
        ulp = R.bf16_ulp(r.y)
        down = torch.where(down.abs() > r.y.abs(), down - ulp * torch.sign(r.y), down)
        return [(down, r, {})]

    probes, rounding = [c for c in cases if c.probe], [c for c in cases if not c.probe]
    assert _rejected_somewhere(probes, one_product_removed) == len(probes), "a probe let a dropped product pass"
    assert _rejected_somewhere(rounding, one_product_removed) >= 1                                     # (fp32; a bf16 store's 2^-8 can hide one product: the probes' job)
    assert _rejected_somewhere(cases, border_tap_shifted) == len(cases)
    assert _rejected_somewhere(cases, with_weights(lambda w: w.flip(2, 3))) == len(cases)               # taps flipped
    assert _rejected_somewhere(cases, with_weights(lambda w: w.transpose(0, 1).contiguous())) == len(cases)   # in / out swapped
    assert _rejected_somewhere(cases, bias_twice) == len(cases)
    assert _rejected_somewhere(rounding, store_toward_zero) >= 1
    assert _rejected_somewhere(probes, store_toward_zero) == 0                                         # (integers: both roundings are exact)


def test_planted_weight_gradient_errors_are_rejected():
    """One pixel of a slab edge counted twice, and the last pixel of the reduction dropped."""
    Ls = [L for L in R.wgrad_cases(True) + R.wgrad_cases(False) if R.wgrad_route(L).nslab > 1 and not L.transposed][:6]
    Ls += [L for L in R.strip_cases(True) if L.note == "strip-pw"][:4]
    assert len(Ls) >= 8

    def pixel_term(c, pix):
        only = torch.zeros_like(c.dy)
        only.view(-1, c.L.Co)[pix] = c.dy.view(-1, c.L.Co)[pix]
        return R.wgrad(c.L, c.x, only).y

    def edge_twice(c):
        r = R.wgrad(c.L, c.x, c.dy)
        route = R.wgrad_route(c.L)
        pix = route.rows if not route.strip else R.strip_len(route.q) - 1      # the first pixel of the second slab | the last of the first strip
        return [(r.y + pixel_term(c, min(pix, c.L.Mp - 1)), r, {})]

    def last_dropped(c):
        r = R.wgrad(c.L, c.x, c.dy)
        return [(r.y - pixel_term(c, c.L.Mp - 1), r, {})]

    probes = [R.probe_inputs(L) for L in Ls]
    assert _rejected_somewhere(probes, last_dropped) == len(probes)
    assert _rejected_somewhere(probes, edge_twice) >= len(probes) - 2       # (an interior pixel may be all zeros in a 4-channel probe)
