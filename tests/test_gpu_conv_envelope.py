"""The nsg_conv_* family (csrc/gemm_gather.hip, gemm_patch.hip, gemm_wgrad.hip, gemm_wgrad_strip.hip, stencil_c1.hip; the packer,
col2im_c1_kernel and colsum of conv_api.hip) over its envelope, against the fp64 yardstick tests/helpers/conv_ref64.py.

Cases (conv_ref64 derives them from the kernels' constants; tests/test_conv_ref_host.py asserts that every boundary is hit):
    gemm_gather     rows 1 | 127 | 128 | 129; C_out on each side of the 32 / 64 / 128 column tiles; C_in on each side of the K chunk;
                    k = 1, 2, 3, 5, 7, every pad of k = 3, rectangular, cropped, Conv2d 4/2/1 in its four parity classes,
                    ConvTranspose2d 4/2/1 and (fp32) stride 1; fp32 and bf16
    gemm_patch      3x3 with (pad, pad_w) over {0, 1, 2}^2, pad 2 cropped, RH in 1 | 3 | 4 | 5 x RW in 1 | 31 | 32 | 33, C_in = 448 (its
                    last) | 512 (gemm_gather's first), both 4/2/1 forms at 256 | 320, C_out = 256, 513 (257) one-pixel clips past the
                    grid cap; every case again through the diagnostics build with the patch kernel switched off: equal bits
    weight gradient Mp = 1 | 31 | 32 | 33 | 255 | 256 | 257 (bf16: a slab of 160 rows ends mid-chunk) | 289; 63 | 64 slabs (the 8-way closing
                    sum); the three tiles; NSG_RELU_IN on either side; the strip kernels at nslab - 1 | nslab | nslab + 1 | 2 nslab + 1
                    chunks, PW on each side of a strip, pad 0 | 2, A or C = 256, again with the strip kernels switched off
    stencil_c1      LW = 1 | 63 | 64 | 65 with even and odd image width, C = 4 | 8 | 36 | 1020 | 1024, 2049 tiles (past both block caps)
    packer          17 layers in one call (34 jobs > PACK_MAX_JOBS) == 17 single calls
Every case runs forward (each legal flag set, and the _bnstats form), the data gradient (plain, add, mask, add + mask) and the
weight gradient with dbias (with and without NSG_RELU_IN), everything twice with equal bits.

PROBES (sparse ternary operands, integer bias / add / mask) must EQUAL the reference: torch.equal, no tolerance.  ROUNDING cases
(normal operands, chains of at most 288 products) must lie within K 2^-24 sum |a b| (+ 2^-8 |want| for a bf16 store; behind a
tanh + 1e-6 |want| + 1e-7): derived in conv_ref64.py, not measured.  Every output is a view into a NaN-filled buffer with 64 canary
elements on each side, which must keep their bits; no NaN may remain in the output.

Largest error / bound of the rounding cases as measured on an MI355X (also DESIGN.md, "Envelope of the convolution kernels"):
forward 0.988 (bf16 Conv2d(1, 16), 2 x 12 x 24) and data gradient 0.986 (bf16 ConvTranspose2d(64, 1)), both the bf16 store rounding
itself; weight gradient 0.076; dbias 0.012.  Every probe is exact.

Found by this module: nsg_conv_forward_bnstats sized its statistics records by 128-row tiles while gemm_patch.hip writes one per
workgroup, and checked the count after the launch (test_probe[bf16-C3x3s1p1.1-B1-79x3-128to128-strip-chunks]: 20 records into
room for 10, status -3)."""
import math
import types
from ctypes import byref, c_void_p

import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, ops  # noqa: E402
from tests.helpers import conv_ref64 as R  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
BF, F32 = torch.bfloat16, torch.float32
CANARY = 64
WORST = {}
COUNT = {"launches": 0}


def _note(cls, ratio, where):
    if ratio > WORST.get(cls, (-1.0, ""))[0]:
        WORST[cls] = (ratio, where)


def _ints(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _out(shape, dtype):
    """An output over NaN poison between two rows of canaries -> (the view, the whole buffer)."""
    n = math.prod(shape)
    whole = torch.full((n + 2 * CANARY,), NAN, dtype=dtype, device=DEV)
    return whole[CANARY:CANARY + n].view(shape), whole


def _collect(view, whole, what):
    torch.cuda.synchronize()
    iv = _ints(whole).cpu()
    poison = _ints(torch.full((1,), NAN, dtype=whole.dtype))[0]
    assert bool((iv[:CANARY] == poison).all()), f"{what}: elements BEFORE the output were written"
    assert bool((iv[-CANARY:] == poison).all()), f"{what}: elements BEHIND the output were written"
    got = view.detach().cpu()
    assert not bool(torch.isnan(got.float()).any()), f"{what}: poison left in the output (an element the kernel did not write)"
    COUNT["launches"] += 1
    return got


def _desc(L):
    return ops.conv_desc(L.B, L.IH, L.IW, L.Ci, L.Co, (L.kh, L.kw), L.stride, (L.ph, L.pw), transposed=L.transposed, dtype=BF if L.bf16 else F32,
                         out_hw=(L.OH, L.OW))


def _setup(c):
    L = c.L
    act = BF if L.bf16 else F32
    t = types.SimpleNamespace(L=L, d=_desc(L), xdt=F32 if L.Ci == 1 else act, ydt=F32 if L.Co == 1 else act)
    t.w = c.w.float().to(DEV)
    t.wf, t.wd = ops.pack_weights(t.d, t.w)
    t.x, t.dy, t.bias = c.x.to(t.xdt).to(DEV), c.dy.to(t.ydt).to(DEV), c.bias.float().to(DEV)
    t.add, t.relu_x = c.add.to(t.xdt).to(DEV), c.relu_x.to(t.xdt).to(DEV)
    t.fwd_flags = R.fwd_flag_sets(L, c.probe)
    t.wg_flags = R.wgrad_flag_sets(L)
    t.epi = R.has_epilogue(L)
    t.dgrads = [("dgrad", False, False)] + ([("dgrad+add", True, False), ("dgrad+mask", False, True), ("dgrad+add+mask", True, True)] if t.epi else [])
    return t


def _forward(t, flags, stats=False):
    L = t.L
    y, whole = _out((L.B, L.OH, L.OW, L.Co), F32 if (flags & R.OUT_F32) else t.ydt)
    if stats:
        _, mean, invstd = ops.conv_forward_bnstats(t.d, t.x, t.wf, t.bias, flags=flags, out=y)
        return _collect(y, whole, f"{L.tag} forward_bnstats"), mean.cpu(), invstd.cpu()
    ops.conv_forward(t.d, t.x, t.wf, t.bias, flags=flags, out=y)
    return _collect(y, whole, f"{L.tag} forward flags={flags}")


def _dgrad(t, add, mask):
    L = t.L
    dx, whole = _out((L.B, L.IH, L.IW, L.Ci), t.xdt)
    ops.conv_dgrad(t.d, t.dy, t.wd, out=dx, add=t.add if add else None, relu_x=t.relu_x if mask else None)
    return _collect(dx, whole, f"{L.tag} dgrad add={add} mask={mask}")


def _wgrad(t, flags):
    L = t.L
    (dw, dw_all), (db, db_all) = _out(L.wshape, F32), _out((L.Co,), F32)
    ops.conv_wgrad(t.d, t.x, t.dy, L.wshape, flags=flags, dw=dw, dbias=db)
    return _collect(dw, dw_all, f"{L.tag} wgrad flags={flags}"), _collect(db, db_all, f"{L.tag} dbias flags={flags}")


def _run_all(t):
    """Every launch of a case, in a fixed order -> {name: CPU tensor}."""
    out = {}
    for flags in t.fwd_flags:
        out[f"forward flags={flags}"] = _forward(t, flags)
    if t.epi:
        out["bnstats y"], out["bnstats mean"], out["bnstats invstd"] = _forward(t, 0, stats=True)
    for name, add, mask in t.dgrads:
        out[name] = _dgrad(t, add, mask)
    for flags in t.wg_flags:
        out[f"dw flags={flags}"], out[f"dbias flags={flags}"] = _wgrad(t, flags)
    return out


def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(_ints(a[k]), _ints(b[k])), f"{what}: {k}"


def _switched_kernels(L):
    """Does a launch of this case go to gemm_patch.hip or to the strip kernels?"""
    fw, dg = R.gemm_params(L, "forward"), R.gemm_params(L, "dgrad")
    return (R.patch_kind(fw) >= 0 or R.patch_kind(dg) >= 0 or R.strip_applicable(R.wgrad_params(L)))


def _hold(cls, got, r, c, what, want=None, terms=None, K=None):
    ok, ratio = R.accepts(got.double(), r, c.probe, want, terms, K)
    if ratio is not None:
        print(f"[conv envelope] {what}: error / bound = {ratio:.4f}")
        _note(cls, ratio, what)
    want = r.y if want is None else want
    if c.probe:
        bad = int((got.double().reshape(want.shape) != R.store(r, want)).sum())
        assert ok, f"{what}: {bad} of {want.numel()} elements differ from the exact result"
    else:
        assert ok, f"{what}: error / bound = {ratio:.3f}"


def _check_case(c):
    L = c.L
    t = _setup(c)
    first = _run_all(t)
    _same_bits(first, _run_all(t), f"{L.tag}: two runs differ")
    if c.probe and _switched_kernels(L):
        with _lib.use_diag() as lib:        # the same sources with gemm_patch.hip and the strip kernels switched off
            lib.nsg_debug_set_patch_gemm(0)
            lib.nsg_debug_set_wgrad_strip(0)
            try:
                other = _run_all(t)
            finally:
                lib.nsg_debug_set_patch_gemm(1)
                lib.nsg_debug_set_wgrad_strip(3)
        _same_bits({k: v for k, v in first.items() if "bnstats m" not in k and "bnstats i" not in k}, other,
                   f"{L.tag}: gemm_gather.hip / the per-tap kernels give other bits")
    for flags in t.fwd_flags:
        r = R.forward(L, c.x, c.w, c.bias, flags)
        _hold("forward", first[f"forward flags={flags}"], r, c, f"{L.tag} forward flags={flags}")
    if t.epi:
        y = first["bnstats y"]
        assert torch.equal(_ints(y), _ints(first["forward flags=0"])), f"{L.tag}: the _bnstats form stores another y"
        # The statistics are of y before its store rounding (gemm_gather.hip: the fp32 tile in LDS) or as stored (gemm_patch.hip):
        # of y + d with |d| <= the element's bound either way (0 on a probe).  Then |mean' - mean| <= mean |d| and, by Cauchy-Schwarz,
        # |var' - var| <= 2 std e + e^2 with e = rms d; on top, the project's figures for a statistics pass (test_gpu_ops.py).
        r0 = R.forward(L, c.x, c.w, c.bias, 0)
        y64 = r0.y.reshape(-1, L.Co)
        d = torch.zeros_like(y64) if c.probe else R.bound(r0).reshape(-1, L.Co)
        mean, var = y64.mean(0), y64.var(0, unbiased=False)
        std, e = var.sqrt(), (d * d).mean(0).sqrt()
        got_mean, got_invstd = first["bnstats mean"].double(), first["bnstats invstd"].double()
        assert bool(((got_mean - mean).abs() <= d.mean(0) + 1e-5 * mean.abs() + 2e-6 * float(std.max()) + 1e-6).all()), f"{L.tag}: bnstats mean"
        invstd = 1.0 / torch.sqrt(var + ops.BN_EPS)
        x = ((2.0 * std * e + e * e) / (var + ops.BN_EPS)).clamp_max(0.5)
        rel = 2e-5 + (1.0 / torch.sqrt(1.0 - x) - 1.0)
        assert bool(((got_invstd - invstd).abs() <= rel * invstd).all()), f"{L.tag}: bnstats invstd"
    for name, add, mask in t.dgrads:
        r = R.dgrad(L, c.dy, c.w, c.add if add else None, c.relu_x if mask else None)
        _hold("dgrad", first[name], r, c, f"{L.tag} {name}")
    for flags in t.wg_flags:
        r = R.wgrad(L, c.x, c.dy, flags)
        _hold("wgrad", first[f"dw flags={flags}"], r, c, f"{L.tag} dw flags={flags}")
        _hold("dbias", first[f"dbias flags={flags}"], r, c, f"{L.tag} dbias flags={flags}", want=r.dbias, terms=r.dbias_terms, K=r.Kb)


@pytest.mark.parametrize("L", R.probe_cases(), ids=lambda L: L.tag)
def test_probe(L):
    """Integer-valued operands: every entry point must reproduce the reference exactly."""
    _check_case(R.probe_inputs(L))


@pytest.mark.parametrize("L", R.all_rounding_cases(), ids=lambda L: L.tag)
def test_rounding(L):
    """Real-valued operands over short chains: fp32 accumulation, round-to-nearest-even stores, bias and tanh applied once."""
    _check_case(R.rounding_inputs(L))


def test_out_f32_skips_the_store_rounding():
    """NSG_OUT_F32 of a bf16 layer must hold the fp32 accumulator, not a bf16 value widened: most of its values are not
    representable in bf16, and rounding them gives the bf16 output's bits."""
    L = R.rounding_cases(True)[0]
    c = R.rounding_inputs(L)
    t = _setup(c)
    y32, y16 = _forward(t, R.OUT_F32), _forward(t, 0)
    assert y32.dtype == F32 and y16.dtype == BF
    assert float((y32.bfloat16().float() != y32).float().mean()) > 0.9, "the fp32 output holds bf16 values"
    assert torch.equal(_ints(y32.bfloat16()), _ints(y16)), "the bf16 output is not the fp32 output rounded to nearest even"


def test_packer_batch_equals_single_calls():
    layers = R.pack_layers()
    assert R.pack_jobs(layers) > R.PACK_MAX_JOBS
    g = torch.Generator().manual_seed(5)
    jobs = []
    for L in layers:
        jobs.append((_desc(L), torch.randn(*L.wshape, generator=g).to(DEV), True, True))
    batch = ops.pack_weights_batch(jobs)
    torch.cuda.synchronize()

    def single(d, w, fill):
        n = _lib.query("nsg_packed_weight_floats", byref(d))
        wf, wd = (torch.full((n,), fill, dtype=ops.torch_dtype(d.dtype), device=DEV) for _ in range(2))
        _lib.call("nsg_pack_conv_weights", byref(d), ops._p(w), ops._p(wf), ops._p(wd), ops._stream())
        return wf, wd

    for i, ((d, w, _, _), images) in enumerate(zip(jobs, batch)):
        # a buffer of nsg_packed_weight_floats(d) elements is not written everywhere (only one of a layer's two images may carry the
        # fragment-ordered twin): what a single call writes is where its results over two different fills agree
        for got, a, b in zip(images, single(d, w, 0.0), single(d, w, NAN)):
            written = _ints(a) == _ints(b)
            assert int(written.sum()) >= layers[i].kh * layers[i].kw * layers[i].Ci * layers[i].Co
            assert got.numel() == a.numel() and torch.equal(_ints(got)[written], _ints(a)[written]), f"layer {i} ({layers[i].tag}): images differ"


# ---- rejections ------------------------------------------------------------------------------------------------------------------
def _raw(B, IH, IW, Ci, OH, OW, Co, k, stride, pad, tr=0, bf=0, k_w=0, pad_w=0):
    return _lib.ConvDesc(B, IH, IW, Ci, OH, OW, Co, k, stride, pad, tr, ops.NSG_BF16 if bf else ops.NSG_F32, k_w, pad_w)


# (what, descriptor, status): conv_api.hip classify()
REFUSED_DESCRIPTORS = [
    ("C_in = 6 in fp32", _raw(1, 8, 8, 6, 8, 8, 8, 3, 1, 1), R.E_UNSUPPORTED),
    ("C_out = 12 in bf16", _raw(1, 8, 8, 8, 8, 8, 12, 3, 1, 1, bf=1), R.E_UNSUPPORTED),
    ("stride 3", _raw(1, 8, 8, 8, 3, 3, 8, 3, 3, 1), R.E_UNSUPPORTED),
    ("k = 8", _raw(1, 8, 8, 8, 7, 7, 8, 8, 1, 3), R.E_UNSUPPORTED),
    ("pad >= k", _raw(1, 8, 8, 8, 12, 12, 8, 3, 1, 3), R.E_UNSUPPORTED),
    ("stride 2 with k = 3", _raw(1, 8, 8, 8, 4, 4, 8, 3, 2, 1), R.E_UNSUPPORTED),
    ("OH above the full extent", _raw(1, 8, 8, 8, 9, 8, 8, 3, 1, 1), R.E_INVALID),
    ("transposed extent that does not match", _raw(1, 4, 4, 8, 8, 9, 8, 4, 2, 1, tr=1), R.E_INVALID),
    ("stride-1 transposed extent that does not match", _raw(1, 4, 4, 8, 6, 7, 8, 3, 1, 0, tr=1), R.E_INVALID),
    ("stride-1 transposed in bf16", _raw(1, 4, 4, 8, 6, 6, 8, 3, 1, 0, tr=1, bf=1), R.E_UNSUPPORTED),
    ("rectangular with C_in = 1", _raw(1, 8, 8, 1, 4, 4, 8, 4, 2, 1, k_w=3, pad_w=1), R.E_INVALID),      # (stride 2: the extent check comes first)
    ("rectangular stride 1 with C_in = 1", _raw(1, 8, 8, 1, 8, 8, 8, 3, 1, 1, k_w=5, pad_w=2), R.E_UNSUPPORTED),
    ("C_in = 1 with k = 3", _raw(1, 8, 8, 1, 8, 8, 8, 3, 1, 1), R.E_UNSUPPORTED),
    ("C = 1028 on Conv2d(1, C)", _raw(1, 4, 4, 1, 2, 2, R.C1_MAX_C + 4, 4, 2, 1), R.E_UNSUPPORTED),
    ("C = 1028 on ConvTranspose2d(C, 1)", _raw(1, 2, 2, R.C1_MAX_C + 4, 4, 4, 1, 4, 2, 1, tr=1), R.E_UNSUPPORTED),
]


class _Arena:
    """Operands far larger than any tensor the descriptors above imply, outputs over poison."""

    def __init__(self):
        n = 1 << 18
        self.inp = torch.zeros(n, device=DEV)
        self.outs = [torch.full((n,), NAN, device=DEV) for _ in range(2)]
        self.ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)

    def untouched(self, what):
        torch.cuda.synchronize()
        for o in self.outs:
            assert bool(torch.isnan(o).all()), f"{what}: a refused call wrote to an output"


@pytest.fixture(scope="module")
def arena():
    return _Arena()


@pytest.mark.parametrize("what,d,status", REFUSED_DESCRIPTORS, ids=[r[0] for r in REFUSED_DESCRIPTORS])
def test_refused_descriptor_launches_nothing(arena, what, d, status):
    lib, p, a = _lib.load(), ops._p, arena
    s = ops._stream()
    nb = a.ws.numel()
    assert lib.nsg_conv_workspace_bytes(byref(d)) == 0
    assert lib.nsg_conv_forward(byref(d), p(a.inp), p(a.inp), p(a.inp), p(a.outs[0]), 0, p(a.ws), nb, s) == status, what
    assert lib.nsg_conv_forward_bnstats(byref(d), p(a.inp), p(a.inp), p(a.inp), p(a.outs[0]), 0, 1e-5, 0.1, p(a.outs[1]), p(a.outs[1]), None, None,
                                        p(a.ws), nb, s) == status, what
    assert lib.nsg_conv_dgrad(byref(d), p(a.inp), p(a.inp), p(a.outs[0]), 0, p(a.ws), nb, s) == status, what
    assert lib.nsg_conv_dgrad_relu_add(byref(d), p(a.inp), p(a.inp), p(a.inp), p(a.inp), p(a.outs[0]), 0, p(a.ws), nb, s) == status, what
    assert lib.nsg_conv_wgrad(byref(d), p(a.inp), p(a.inp), p(a.outs[0]), p(a.outs[1]), 0, p(a.ws), nb, s) == status, what
    assert lib.nsg_pack_conv_weights(byref(d), p(a.inp), p(a.outs[0]), p(a.outs[1]), s) == status, what
    a.untouched(what)


def test_refused_calls_launch_nothing(arena):
    """The NSG_REQUIREs of the four entry points on descriptors classify() accepts."""
    lib, p, a = _lib.load(), ops._p, arena
    s = ops._stream()
    conv = _desc(R.layer(1, 8, 8, 8, 8, 3, 1, 1))
    conv_bf = _desc(R.layer(1, 8, 8, 8, 8, 3, 1, 1, bf16=True))
    c1 = _desc(R.layer(1, 8, 8, 1, 8, 4, 2, 1))
    c1t = _desc(R.layer(1, 4, 4, 8, 1, 4, 2, 1, transposed=True))
    nb = {id(d): lib.nsg_conv_workspace_bytes(byref(d)) for d in (conv, conv_bf, c1, c1t)}
    assert all(0 < v <= a.ws.numel() for v in nb.values())
    o0, o1, x, ws = p(a.outs[0]), p(a.outs[1]), p(a.inp), p(a.ws)
    off = lambda t, nbytes: c_void_p(t.data_ptr() + nbytes)  # noqa: E731

    def fwd(d, xx=x, ww=x, y=o0, flags=0, nbytes=None):
        return lib.nsg_conv_forward(byref(d), xx, ww, x, y, flags, ws, nb[id(d)] if nbytes is None else nbytes, s)

    def stats(d, flags=0, nbytes=None):
        return lib.nsg_conv_forward_bnstats(byref(d), x, x, x, o0, flags, 1e-5, 0.1, o1, o1, None, None, ws, nb[id(d)] if nbytes is None else nbytes, s)

    def dgr(d, dy=x, ww=x, add=None, mask=None, dx=o0, nbytes=None):
        return lib.nsg_conv_dgrad_relu_add(byref(d), dy, ww, add, mask, dx, 0, ws, nb[id(d)] if nbytes is None else nbytes, s)

    def wgr(d, xx=x, dy=x, flags=0, nbytes=None):
        return lib.nsg_conv_wgrad(byref(d), xx, dy, o0, o1, flags, ws, nb[id(d)] if nbytes is None else nbytes, s)

    checks = [
        ("NSG_TANH_OUT with _bnstats", lambda: stats(conv, R.TANH_OUT), R.E_UNSUPPORTED),
        ("NSG_RELU_OUT with _bnstats", lambda: stats(conv, R.RELU_OUT), R.E_UNSUPPORTED),
        ("_bnstats on a single-channel output", lambda: stats(c1t), R.E_UNSUPPORTED),
        ("add on Conv2d(1, C)", lambda: dgr(c1, add=x), R.E_UNSUPPORTED),
        ("relu_x on ConvTranspose2d(C, 1)", lambda: dgr(c1t, mask=x), R.E_UNSUPPORTED),
        ("NSG_RELU_IN on the C_in = 1 weight gradient", lambda: wgr(c1, flags=R.RELU_IN), R.E_UNSUPPORTED),
        ("a fused activation on the C_in = 1 forward", lambda: fwd(c1, flags=R.RELU_IN), R.E_UNSUPPORTED),
        ("forward: x off 16-byte alignment", lambda: fwd(conv, xx=off(a.inp, 4)), R.E_INVALID),
        ("forward: w off 16-byte alignment", lambda: fwd(conv_bf, ww=off(a.inp, 2)), R.E_INVALID),
        ("forward: y of the stencil layer off alignment", lambda: fwd(c1, y=off(a.outs[0], 4)), R.E_INVALID),
        ("dgrad: dy off alignment", lambda: dgr(conv, dy=off(a.inp, 8)), R.E_INVALID),
        ("dgrad + add: add off alignment", lambda: dgr(conv, add=off(a.inp, 4)), R.E_UNSUPPORTED),
        ("dgrad: dx of the stencil layer off alignment", lambda: dgr(c1t, dx=off(a.outs[0], 4)), R.E_INVALID),
        ("wgrad: x off alignment", lambda: wgr(conv, xx=off(a.inp, 4)), R.E_INVALID),
        ("wgrad: dy off alignment", lambda: wgr(conv_bf, dy=off(a.inp, 2)), R.E_INVALID),
        ("wgrad: dy of the stencil layer off alignment", lambda: wgr(c1, dy=off(a.inp, 4)), R.E_INVALID),
        ("a null operand", lambda: lib.nsg_conv_forward(byref(conv), None, x, x, o0, 0, ws, nb[id(conv)], s), R.E_INVALID),
        ("wgrad: workspace one byte short", lambda: wgr(conv, nbytes=nb[id(conv)] - 1), R.E_WORKSPACE),
        ("wgrad (stencil): workspace one byte short", lambda: wgr(c1, nbytes=nb[id(c1)] - 1), R.E_WORKSPACE),
        ("forward (ConvTranspose2d(C, 1)): workspace one byte short", lambda: fwd(c1t, nbytes=nb[id(c1t)] - 1), R.E_WORKSPACE),
        ("dgrad (Conv2d(1, C)): workspace one byte short", lambda: dgr(c1, nbytes=nb[id(c1)] - 1), R.E_WORKSPACE),
        ("_bnstats: workspace one byte short", lambda: stats(conv, nbytes=nb[id(conv)] - 1), R.E_WORKSPACE),
    ]
    for what, fn, status in checks:
        assert fn() == status, what
        a.untouched(what)


def test_report_worst_ratios():
    """Not a check: the largest error / bound each entry point's rounding cases met in this module's run (pytest -s)."""
    for cls in sorted(WORST):
        print(f"[conv envelope summary] {cls}: largest error / bound = {WORST[cls][0]:.4f} at {WORST[cls][1]}")
    print(f"[conv envelope summary] {COUNT['launches']} outputs checked for canaries and poison")
