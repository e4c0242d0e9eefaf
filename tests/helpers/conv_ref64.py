"""The fp64 yardstick of the nsg_conv_* family (csrc/gemm_gather.hip, gemm_patch.hip, gemm_wgrad.hip, gemm_wgrad_strip.hip,
stencil_c1.hip and the packer / col2im_c1_kernel / colsum of conv_api.hip): torch.nn.functional.conv2d / conv_transpose2d and
torch.autograd.grad on fp64 CPU tensors, the library's NHWC layout handled at the edges.  tests/test_conv_ref_host.py holds this
file to itself and to the case tables' conditions; tests/test_gpu_conv_envelope.py holds the kernels to it.

Every function returns, next to the value, per output element `terms` = sum |a b| (the same convolution over the operands'
magnitudes) and the chain length K = the most products any one element sums (the same convolution over ones: taps x reduced
channels in the interior, fewer on a border; lowres pixels B OH OW for a weight gradient; + 1 for the fused `add`).

Two kinds of input.  PROBES: sparse ternary {-1, 0, 1} operands (a quarter non-zero), small integer bias / add / mask: every
product and partial sum is an integer below 2^24 in any order and every bf16-stored output an integer of at most 256, so a
kernel must EQUAL the reference (test_conv_ref_host.py asserts both conditions from the reference alone).  ROUNDING cases:
normal operands (pre-rounded to bf16 in the bf16 mode), chains of at most MAX_ROUND_K products, bound
fused_ref64.mfma_bound(want, terms, 0, K, stored_bf16) = K 2^-24 sum |a b| (+ 2^-8 |want| for a bf16 store), and behind a tanh
(derivative <= 1) + TANH_RTOL |want| + TANH_ATOL.

The dispatch of the launchers is restated below as plain functions of named constants, each with the source line it mirrors;
the case tables are DERIVED from them, so a changed constant moves the cases (or fails the host test's coverage asserts)."""
import types

import torch
import torch.nn.functional as F

from tests.helpers.fused_ref64 import TANH_ATOL, TANH_RTOL, U32, UB, bf16_ulp, cdiv, f64, mfma_bound, rb  # noqa: F401

RELU_IN, TANH_OUT, OUT_F32, RELU_OUT = 1, 2, 8, 16      # include/nsg.h:56-60
E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3      # include/nsg.h:45-47
MAX_ROUND_K = 288
EXACT_SUM, EXACT_BF16 = 2.0 ** 24, 256.0                # the probes' two conditions

# ---- the kernels' constants ------------------------------------------------------------------------------------------------------
GATHER_BM = 128                         # gemm_gather.hip:490-492 launch_typed: 128 rows by
GATHER_BN = (32, 64, 128)               #   32 (C_out <= 32) | 64 (<= 64) | 128 columns
GATHER_KC = {False: 32, True: 64}       # gemm_gather.hip:43 KC = 8 * EPV channels per K chunk (fp32 | bf16)
PG_MAX_JOBS, PG_MAX_TAPS = 16, 64       # gemm_patch.hip:45-46
PATCH_TILE = (4, 32)                    # gemm_patch.hip:658-659 tiles_y = cdiv(RH, 4), tiles_x = cdiv(RW, 32)
PATCH_GRID_CAP = 512                    # gemm_patch.hip:33 g_patch_grid_cap
PATCH_CI, PATCH_CO = 64, 128            # gemm_patch.hip:615 C_in % 64, C_out % 128
WGRAD_KP, WGRAD_KPB = 32, 64            # gemm_wgrad.hip:33 (fp32 chunk), :293 (bf16 chunk)
WGRAD_ROUND, WGRAD_MIN_ROWS, WGRAD_MAX_SLABS = 512, 256, 512      # gemm_wgrad.hip:705-709 plan_slabs
SPLIT_SLABS, SPLIT_OUTPUTS, SPLIT_WAYS = 64, 512 * 256, 8         # nsg_common.h:150 nsg_slab_split
STRIP_CUS, STRIP_SP, STRIP_SP_F32_S2 = 256, 64, 32      # gemm_wgrad_strip.hip:410, :24, :432
C1_TW, C1_FWD_BLOCKS, C1_WGRAD_BLOCKS = 64, 2048, 1024  # c1_geom.h:9, stencil_c1.hip:598, :585 (NSG_MAX_SLABS)
C1_MAX_C = 1024                         # stencil_c1.hip:589 nsg_c1_stencil_supported
PACK_MAX_JOBS = 32                      # conv_api.hip:23


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def layer(B, IH, IW, Ci, Co, k, stride=1, pad=0, transposed=False, bf16=False, out_hw=None, note=""):
    """One nn.Conv2d / nn.ConvTranspose2d(Ci, Co, k, stride, pad) on a (B, IH, IW) input; k / pad may be (rows, columns)."""
    (kh, kw), (ph, pw) = _pair(k), _pair(pad)
    if transposed:
        FH, FW = (IH - 1) * stride - 2 * ph + kh, (IW - 1) * stride - 2 * pw + kw
    else:
        FH, FW = (IH + 2 * ph - kh) // stride + 1, (IW + 2 * pw - kw) // stride + 1
    OH, OW = out_hw if out_hw is not None else (FH, FW)
    L = types.SimpleNamespace(B=B, IH=IH, IW=IW, Ci=Ci, Co=Co, kh=kh, kw=kw, stride=stride, ph=ph, pw=pw, transposed=transposed, bf16=bf16,
                              OH=OH, OW=OW, FH=FH, FW=FW, note=note)
    L.wshape = (Ci, Co, kh, kw) if transposed else (Co, Ci, kh, kw)
    L.Mp = B * IH * IW if transposed else B * OH * OW        # conv_api.hip:375 lowres_pixels
    L.tag = (f"{'bf16' if bf16 else 'f32'}-{'T' if transposed else 'C'}{kh}x{kw}s{stride}p{ph}.{pw}-B{B}-{IH}x{IW}-{Ci}to{Co}"
             + (f"-crop{OH}x{OW}" if (OH, OW) != (FH, FW) else "") + (f"-{note}" if note else ""))
    return L


def kind(L):
    """conv_api.hip:324 classify(), for the layers it accepts."""
    if not L.transposed:
        return "conv_c1" if L.Ci == 1 else "conv"
    if L.stride == 1:
        return "convt_s1"
    return "convt_c1" if L.Co == 1 else "convt"


def fwd_stored_bf16(L, flags=0):
    return L.bf16 and L.Co > 1 and not (flags & OUT_F32)


def dx_stored_bf16(L):
    return L.bf16 and L.Ci > 1


# ----------------------------------------------------------------------------------------------------------------------
# the reference: NHWC in, NHWC out
# ----------------------------------------------------------------------------------------------------------------------
def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _conv(L, x4, w, b):
    if L.transposed:
        y = F.conv_transpose2d(x4, w, b, stride=L.stride, padding=(L.ph, L.pw))
    else:
        y = F.conv2d(x4, w, b, stride=L.stride, padding=(L.ph, L.pw))
    return y[:, :, :L.OH, :L.OW]


def forward(L, x, w, bias, flags=0):
    """nsg_conv_forward -> namespace(y, pre (before RELU_OUT / TANH_OUT), terms, K, stored_bf16)."""
    x4, w, b = _nchw(f64(x)), f64(w), f64(bias)
    if flags & RELU_IN:
        x4 = x4.clamp_min(0.0)
    pre = _conv(L, x4, w, b)
    terms = _conv(L, x4.abs(), w.abs(), None if b is None else b.abs())
    K = int(_conv(L, torch.ones_like(x4), torch.ones_like(w), None).max())
    y = pre.clamp_min(0.0) if flags & RELU_OUT else pre
    y = torch.tanh(y) if flags & TANH_OUT else y
    return types.SimpleNamespace(y=_nhwc(y), pre=_nhwc(pre), terms=_nhwc(terms), K=K, stored_bf16=fwd_stored_bf16(L, flags), tanh=bool(flags & TANH_OUT))


def dgrad(L, dy, w, add=None, relu_x=None):
    """nsg_conv_dgrad / nsg_conv_dgrad_relu_add: dx = (autograd's data gradient + add) * (relu_x > 0)."""
    w = f64(w)

    def g(dy4, ww):
        x0 = torch.zeros(L.B, L.Ci, L.IH, L.IW, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(_conv(L, x0, ww, None), x0, dy4)[0]

    dy4 = _nchw(f64(dy))
    dx, terms = _nhwc(g(dy4, w)), _nhwc(g(dy4.abs(), w.abs()))
    K = int(g(torch.ones_like(dy4), torch.ones_like(w)).max())
    if add is not None:
        dx, terms, K = dx + f64(add), terms + f64(add).abs(), K + 1
    if relu_x is not None:
        dx = torch.where(f64(relu_x) > 0, dx, torch.zeros_like(dx))
    return types.SimpleNamespace(y=dx, terms=terms, K=K, stored_bf16=dx_stored_bf16(L), tanh=False)


def wgrad(L, x, dy, flags=0):
    """nsg_conv_wgrad -> namespace(y = dw (reference layout), terms, K = lowres pixels, dbias, dbias_terms, Kb = B OH OW)."""
    x4, dy4 = _nchw(f64(x)), _nchw(f64(dy))
    if flags & RELU_IN:
        x4 = x4.clamp_min(0.0)

    def g(xx, dd):
        w0 = torch.zeros(L.wshape, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(_conv(L, xx, w0, None), w0, dd)[0]

    return types.SimpleNamespace(y=g(x4, dy4), terms=g(x4.abs(), dy4.abs()), K=L.Mp, dbias=dy4.sum((0, 2, 3)), dbias_terms=dy4.abs().sum((0, 2, 3)),
                                 Kb=L.B * L.OH * L.OW, stored_bf16=False, tanh=False)


def bound(r, want=None, terms=None, K=None):
    """The derived bound of a rounding case, per element."""
    want, terms, K = r.y if want is None else want, r.terms if terms is None else terms, r.K if K is None else K
    b = mfma_bound(want, terms, 0.0, K, r.stored_bf16)
    return b + TANH_RTOL * want.abs() + TANH_ATOL if r.tanh else b


def store(r, want=None):
    """What an exact kernel stores: the value, through bf16 (round to nearest even) where the output is bf16."""
    want = r.y if want is None else want
    return rb(want) if r.stored_bf16 else want


def accepts(got, r, probe, want=None, terms=None, K=None):
    """THE comparison rule of both kinds of case, on fp64 CPU tensors: a probe must equal the stored reference, a rounding case
    must lie within bound().  -> (ok, largest error / bound or None)."""
    want = r.y if want is None else want
    got = got.reshape(want.shape)
    if not bool(torch.isfinite(got).all()):
        return False, float("inf")
    if probe:
        return bool(torch.equal(got, store(r, want))), None
    ratio = float(((got - want).abs() / bound(r, want, terms, K).clamp_min(1e-300)).max())
    return ratio <= 1.0, ratio


# ----------------------------------------------------------------------------------------------------------------------
# the dispatch, restated
# ----------------------------------------------------------------------------------------------------------------------
def gemm_params(L, role):
    """The GatherGemmParams of a forward (conv_api.hip:552-567) or data-gradient (conv_api.hip:635-656) launch, or None where the
    launch is not a gather GEMM over the layer's own geometry (the single-channel layers)."""
    kd = kind(L)
    if kd in ("conv_c1", "convt_c1"):
        return None
    p = types.SimpleNamespace(B=L.B, KH=L.kh, KW=L.kw, bf16=L.bf16)
    if role == "forward":
        p.CI, p.CO, p.stride = L.Ci, L.Co, L.stride
        if kd == "conv":
            p.mode, p.pad, p.pad_w, p.RH, p.RW = 0, L.ph, L.pw, L.OH, L.OW
        elif kd == "convt_s1":
            p.mode, p.pad, p.pad_w, p.RH, p.RW = 0, L.kh - 1 - L.ph, L.kh - 1 - L.ph, L.OH, L.OW
        else:
            p.mode, p.pad, p.pad_w, p.RH, p.RW = 1, L.ph, L.pw, L.IH, L.IW
    else:
        p.CI, p.CO = L.Co, L.Ci
        if kd == "conv" and L.stride == 1:
            p.mode, p.stride, p.pad, p.pad_w, p.RH, p.RW = 0, 1, L.kh - 1 - L.ph, L.kw - 1 - L.pw, L.IH, L.IW
        elif kd == "convt_s1":
            p.mode, p.stride, p.pad, p.pad_w, p.RH, p.RW = 0, 1, L.ph, L.ph, L.IH, L.IW
        elif kd == "conv":
            p.mode, p.stride, p.pad, p.pad_w, p.RH, p.RW = 1, 2, 1, 1, (L.IH + 1) // 2, (L.IW + 1) // 2
        else:
            p.mode, p.stride, p.pad, p.pad_w, p.RH, p.RW = 0, 2, 1, 1, L.IH, L.IW
    p.M = p.B * p.RH * p.RW
    return p


def gather_tile(CO, bf16):
    """gemm_gather.hip:490-492 -> rows, columns, channels per K chunk."""
    bn = GATHER_BN[2] if CO > GATHER_BN[1] else (GATHER_BN[1] if CO > GATHER_BN[0] else GATHER_BN[0])
    return GATHER_BM, bn, GATHER_KC[bool(bf16)]


def patch_kind(p, flags=0, out_f32=False, stats=False, epi=False):
    """gemm_patch.hip:608 patch_kind -> 0 (3x3 stride 1), 1 (4/2/1), 2 (transposed 4/2/1) or -1: gemm_gather.hip runs it."""
    if p is None or not p.bf16 or out_f32 or flags & (RELU_IN | TANH_OUT):
        return -1
    if stats and (epi or flags & RELU_OUT):
        return -1
    if p.CI % PATCH_CI or p.CO % PATCH_CO:
        return -1
    chunks = p.CI // PATCH_CI
    if p.mode == 1:
        k = 2
    elif (p.KH, p.KW, p.stride) == (3, 3, 1) and 0 <= p.pad <= 2 and 0 <= p.pad_w <= 2:
        k = 0
    elif (p.KH, p.KW, p.stride, p.pad, p.pad_w) == (4, 4, 2, 1, 1):
        k = 1
    else:
        return -1
    njobs, ntaps = (chunks, 9) if k == 0 else (4 * chunks, 4)
    if njobs > PG_MAX_JOBS or njobs * ntaps > PG_MAX_TAPS:
        return -1
    return k


def patch_tiles(p):
    return p.B * cdiv(p.RH, PATCH_TILE[0]) * cdiv(p.RW, PATCH_TILE[1])


def patch_grid(ntiles, ntn):
    """gemm_patch.hip:39 patch_grid: workgroups along x; more tiles than that are walked with a grid stride."""
    return min(ntiles, max(PATCH_GRID_CAP // ntn, 1))


def patch_max_ci(k):
    """The widest C_in the patch kernel takes for kind k (gemm_patch.hip:622-624)."""
    per, taps = (1, 9) if k == 0 else (4, 4)
    return PATCH_CI * min(PG_MAX_JOBS // per, PG_MAX_TAPS // (per * taps))


def wgrad_params(L):
    """conv_api.hip:704-714 -> namespace(A, C, PH, PW, Mp, ntaps, KW, stride, relu side)."""
    if kind(L) in ("conv_c1", "convt_c1"):
        return None
    if kind(L) == "conv":
        A, C, PH, PW = L.Co, L.Ci, L.OH, L.OW
    else:
        A, C, PH, PW = L.Ci, L.Co, L.IH, L.IW
    return types.SimpleNamespace(A=A, C=C, PH=PH, PW=PW, B=L.B, Mp=L.Mp, ntaps=L.kh * L.kw, KH=L.kh, KW=L.kw, stride=L.stride, bf16=L.bf16)


def plan_slabs(Mp, ntaps, A, C):
    """gemm_wgrad.hip:700 plan_slabs -> nslab, rows per slab."""
    tiles = cdiv(A, 128) * cdiv(C, 128 if C > 32 else 32) * ntaps
    want = max(1, min(WGRAD_ROUND // tiles, cdiv(Mp, WGRAD_MIN_ROWS), WGRAD_MAX_SLABS))
    rows = cdiv(cdiv(Mp, want), WGRAD_KP) * WGRAD_KP
    return cdiv(Mp, rows), rows


def slab_split(nslab, outputs):
    """nsg_common.h:150 nsg_slab_split: shares of the closing sum over the slabs."""
    return SPLIT_WAYS if (nslab >= SPLIT_SLABS and outputs < SPLIT_OUTPUTS) else 1


def wgrad_tile(A, C):
    """gemm_wgrad.hip:844-853 -> (rows, columns) of the per-tap kernels' tile."""
    return (128, 32) if C <= 32 else ((64, 64) if (A <= 64 and C <= 64) else (128, 128))


def strip_slabs(ntaps, A, C):
    """gemm_wgrad_strip.hip:406 nsg_wgrad_strip_slabs."""
    kh = 4 if ntaps == 16 else 3
    n = (STRIP_CUS // (kh * max((A >> 7) * (C >> 7), 1))) & ~7
    return max(n, 8)


def strip_applicable(q, flags=0):
    """gemm_wgrad_strip.hip:415-425 nsg_wgrad_strip_shape + nsg_wgrad_strip_applicable."""
    if q is None or flags & RELU_IN or q.A % 128 or q.C % 128:
        return False
    return (q.KH, q.KW, q.stride) in ((3, 3, 1), (4, 4, 2))


def strip_len(q):
    """gemm_wgrad_strip.hip:432: pixels of a strip chunk."""
    return STRIP_SP_F32_S2 if (not q.bf16 and q.stride == 2) else STRIP_SP


def strip_plan(q):
    """gemm_wgrad_strip.hip:438-445 -> chunks, slabs run, chunks per slab."""
    nch = q.B * q.PH * cdiv(q.PW, strip_len(q))
    nslab = min(strip_slabs(q.ntaps, q.A, q.C), nch)
    per = cdiv(nch, nslab)
    return nch, cdiv(nch, per), per


def wgrad_route(L, flags=0):
    """-> namespace(strip, nslab, rows, split, tile): what nsg_launch_wgrad (gemm_wgrad.hip:812) does with the layer."""
    q = wgrad_params(L)
    if q is None:
        return None
    r = types.SimpleNamespace(strip=strip_applicable(q, flags), q=q)
    r.nslab, r.rows = plan_slabs(q.Mp, q.ntaps, q.A, q.C)
    r.tile = wgrad_tile(q.A, q.C)
    if r.strip:
        r.chunks, r.nslab, r.per = strip_plan(q)
    r.split = slab_split(r.nslab, q.ntaps * q.A * q.C)
    return r


def c1_tiles(L):
    """c1_geom.h:33: tiles of TW low-resolution pixels of one row (the multi-channel side's grid)."""
    LH, LW = (L.OH, L.OW) if kind(L) == "conv_c1" else (L.IH, L.IW)
    return L.B * LH * cdiv(LW, C1_TW)


def pack_jobs(layers):
    """conv_api.hip:504-532: two images per layer."""
    return 2 * len(layers)


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def _seed(L, salt):
    return hash((L.B, L.IH, L.IW, L.Ci, L.Co, L.kh, L.kw, L.stride, L.ph, L.pw, L.transposed, L.bf16, L.OH, L.OW, salt)) % (2 ** 31)


def probe_inputs(L):
    """Sparse ternary x, w, dy (a quarter non-zero; the first and the last pixel of x and dy non-zero in every channel, so a lost or
    doubled edge pixel changes every sum it feeds); integer bias in -2 .. 2, add in -3 .. 3, relu_x in 0 .. 2."""
    g = torch.Generator().manual_seed(_seed(L, 1))

    def tern(*shape):
        r = torch.randint(0, 8, shape, generator=g)
        return (r == 0).double() - (r == 1).double()

    c = types.SimpleNamespace(L=L, probe=True)
    c.x, c.w, c.dy = tern(L.B, L.IH, L.IW, L.Ci), tern(*L.wshape), tern(L.B, L.OH, L.OW, L.Co)
    for t, v in ((c.x, 1.0), (c.dy, -1.0)):
        t[0, 0, 0, :], t[-1, -1, -1, :] = v, -v
    c.bias = torch.randint(-2, 3, (L.Co,), generator=g).double()
    c.add = torch.randint(-3, 4, (L.B, L.IH, L.IW, L.Ci), generator=g).double()
    c.relu_x = torch.randint(0, 3, (L.B, L.IH, L.IW, L.Ci), generator=g).double()
    c.relu_x.view(-1)[0], c.relu_x.view(-1)[-1] = 0.0, 2.0             # zeros and positives in the smallest tensor too (C >= 4)
    return c


def rounding_inputs(L):
    """Normal operands, pre-rounded to bf16 in the bf16 mode (the values the kernels are handed; bias stays fp32)."""
    g = torch.Generator().manual_seed(_seed(L, 2))
    q = (lambda t: t.bfloat16().double()) if L.bf16 else (lambda t: t.double())
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    c = types.SimpleNamespace(L=L, probe=False)
    c.x, c.w, c.dy = q(rn(L.B, L.IH, L.IW, L.Ci)), q(rn(*L.wshape) * 0.2), q(rn(L.B, L.OH, L.OW, L.Co))
    c.bias = (rn(L.Co) * 0.1).double()
    c.add, c.relu_x = q(rn(L.B, L.IH, L.IW, L.Ci)), q(rn(L.B, L.IH, L.IW, L.Ci).clamp_min(0.0))
    return c


def fwd_flag_sets(L, probe):
    """The flag sets a case's forward runs (tanh has no exact values: rounding cases only)."""
    kd = kind(L)
    if kd == "conv_c1":
        sets = [0]
    elif kd == "convt_c1":
        sets = [0, RELU_IN] + ([] if probe else [TANH_OUT, RELU_IN | TANH_OUT])
    else:
        sets = [0, RELU_IN, RELU_OUT, RELU_IN | RELU_OUT] + ([] if probe else [TANH_OUT])
        if L.bf16:
            sets += [OUT_F32, RELU_IN | RELU_OUT | OUT_F32] + ([] if probe else [TANH_OUT | OUT_F32])
    return sets


def wgrad_flag_sets(L):
    return [0] if kind(L) == "conv_c1" else [0, RELU_IN]


def has_epilogue(L):
    return kind(L) not in ("conv_c1", "convt_c1")


# ----------------------------------------------------------------------------------------------------------------------
# the case tables, derived from the constants above
# ----------------------------------------------------------------------------------------------------------------------
def _cm(bf16):
    return 8 if bf16 else 4                 # conv_api.hip:330 channel granularity


def _sides(edges, step):
    """step, then each edge and one step past it."""
    out = [step]
    for e in edges:
        out += [e, e + step]
    return out


def gather_cases(bf16):
    cm, cases = _cm(bf16), []
    c0 = cm
    for M in (1, GATHER_BM - 1, GATHER_BM, GATHER_BM + 1):                                   # rows on each side of the tile
        cases.append(layer(1, 1, M, c0, c0, 3, 1, 1, bf16=bf16, note="rows"))
    for co in _sides(GATHER_BN, cm) + [2 * GATHER_BN[2]]:                                   # 4 | 32, 36 | 64, 68 | 128, 132 | 256
        cases.append(layer(2, 5, 7, c0, co, 3, 1, 1, bf16=bf16, note="cols"))
    kc = GATHER_KC[bf16]
    for ci in (cm, kc - cm, kc, kc + cm):                                                    # the K chunk
        cases.append(layer(2, 5, 7, ci, c0, 3, 1, 1, bf16=bf16, note="kchunk"))
    for k in (1, 2, 5, 7):
        cases.append(layer(2, 6, 9, c0, 2 * c0, k, 1, k // 2, bf16=bf16, note="k"))
    for pad in (0, 1, 2):
        cases.append(layer(2, 6, 9, c0, 2 * c0, 3, 1, pad, bf16=bf16, note="pad"))
    cases.append(layer(2, 6, 9, c0, 2 * c0, (2, 3), 1, (1, 1), bf16=bf16, out_hw=(6, 9), note="rect"))     # the prior's masked stacks: pad, then crop
    cases.append(layer(2, 6, 9, 2 * c0, c0, (1, 7), 1, (0, 3), bf16=bf16, note="rect"))
    cases.append(layer(2, 6, 9, c0, 2 * c0, 3, 1, 2, bf16=bf16, out_hw=(6, 9), note="crop"))
    cases.append(layer(2, 6, 9, c0, 2 * c0, 5, 1, 2, bf16=bf16, out_hw=(4, 5), note="crop"))
    for ih, iw in ((6, 8), (7, 9), (6, 9), (7, 8)):                                          # the data gradient's four parity classes; odd: rows outside
        cases.append(layer(2, ih, iw, c0, 2 * c0, 4, 2, 1, bf16=bf16, note="s2"))
    cases.append(layer(1, 2, 2, c0, c0, 4, 2, 1, bf16=bf16, note="s2"))                      # OH = OW = 1
    cases.append(layer(2, 3, 5, 2 * c0, c0, 4, 2, 1, transposed=True, bf16=bf16, note="T"))
    cases.append(layer(1, 1, 1, c0, 2 * c0, 4, 2, 1, transposed=True, bf16=bf16, note="T"))
    if not bf16:
        cases.append(layer(2, 4, 6, c0, 2 * c0, 3, 1, 0, transposed=True, note="Ts1"))
        cases.append(layer(2, 4, 6, 2 * c0, c0, 5, 1, 2, transposed=True, note="Ts1"))
    return cases


def patch_cases():
    ci, co, cases = PATCH_CI, PATCH_CO, []
    th, tw = PATCH_TILE
    for ph in (0, 1, 2):
        for pw in (0, 1, 2):
            cases.append(layer(2, th + 1, tw + 1, ci, co, 3, 1, (ph, pw), bf16=True, note="patch-pad"))
    cases.append(layer(2, th + 1, tw + 1, ci, co, 3, 1, 2, bf16=True, out_hw=(th + 1, tw + 1), note="patch-crop"))
    for rh in (1, th - 1, th, th + 1):
        for rw in (1, tw - 1, tw, tw + 1):
            cases.append(layer(1, rh, rw, ci, co, 3, 1, 1, bf16=True, note="patch-tile"))
    top = patch_max_ci(0)
    cases.append(layer(1, th + 1, tw + 1, top, co, 3, 1, 1, bf16=True, note="patch-last"))                 # 448: the last shape it takes
    cases.append(layer(1, th + 1, tw + 1, top + ci, co, 3, 1, 1, bf16=True, note="patch-first-gather"))    # 512: gemm_gather's
    top2 = patch_max_ci(1)
    for c in (top2, top2 + ci):                                                                            # 256 | 320, both 4/2/1 forms
        cases.append(layer(1, 2 * th + 2, 2 * tw + 2, c, co, 4, 2, 1, bf16=True, note="patch-s2"))
        cases.append(layer(1, th + 1, tw + 1, c, co, 4, 2, 1, transposed=True, bf16=True, note="patch-T"))
    cases.append(layer(1, 7, 9, co, top2, 4, 2, 1, bf16=True, note="patch-s2-dgrad"))                      # odd input: the data gradient (kind 2) at C_in = 256
    cases.append(layer(1, th + 1, tw + 1, ci, 2 * co, 3, 1, 1, bf16=True, note="patch-co256"))
    cases.append(layer(PATCH_GRID_CAP + 1, 1, 1, co, co, 3, 1, 1, bf16=True, note="patch-cap"))            # 513 one-pixel clips
    cases.append(layer(PATCH_GRID_CAP // 2 + 1, 1, 1, 2 * co, 2 * co, 3, 1, 1, bf16=True, note="patch-cap"))  # 257 at C_out = 256 (cap 256)
    return cases


def _first_mp(ntaps, A, C, want_nslab):
    """The smallest reduction length at which plan_slabs gives want_nslab slabs."""
    Mp = (want_nslab - 1) * WGRAD_MIN_ROWS
    while plan_slabs(Mp, ntaps, A, C)[0] != want_nslab:
        Mp += 1
    return Mp


def wgrad_cases(bf16):
    cm, cases = _cm(bf16), []
    kp = WGRAD_KP
    for Mp in (1, kp - 1, kp, kp + 1, WGRAD_MIN_ROWS - 1, WGRAD_MIN_ROWS, WGRAD_MIN_ROWS + 1):
        cases.append(layer(1, 1, Mp, cm, 2 * cm, 3, 1, 1, bf16=bf16, note="wgrad-mp"))
    cases.append(layer(1, 17, 17, cm, 2 * cm, 3, 1, 1, bf16=bf16, note="wgrad-mp"))                       # 289
    for ns in (SPLIT_SLABS - 1, SPLIT_SLABS):                                                              # 63 | 64 slabs: the 8-way closing sum
        Mp = _first_mp(1, 16, 16, ns)
        cases.append(layer(1, 1, Mp, 16, 16, 1, 1, 0, bf16=bf16, note=f"wgrad-{ns}slabs"))
    cases.append(layer(1, 1, 300, 64, 64, 1, 1, 0, bf16=bf16, note="wgrad-64x64"))
    cases.append(layer(1, 1, 300, 128, 136, 1, 1, 0, bf16=bf16, note="wgrad-128x128"))
    cases.append(layer(1, 3, 100, 128, 128, 5, 1, 2, bf16=bf16, note="wgrad-128x128"))                    # 25 taps: 4 slabs
    cases.append(layer(1, 5, 60, 40, 64, 4, 2, 1, transposed=True, bf16=bf16, note="wgrad-T"))
    return cases


def strip_cases(bf16):
    cases, c = [], 128
    for k, s in ((3, 1), (4, 2)):
        ns = strip_slabs(k * k, c, c)
        sp = STRIP_SP_F32_S2 if (not bf16 and s == 2) else STRIP_SP
        rows = (lambda n: n) if s == 1 else (lambda n: 2 * n)            # input rows for n weight-gradient rows (one chunk per row while PW <= strip)
        for n in (ns - 1, ns, ns + 1, 2 * ns + 1):
            cases.append(layer(1, rows(n), rows(3), c, c, k, s, 1, bf16=bf16, note="strip-chunks"))
        for pw in (1, sp - 1, sp, sp + 1):
            cases.append(layer(2, rows(3), rows(pw), c, c, k, s, 1, bf16=bf16, note="strip-pw"))
    for pad in (0, 2):
        cases.append(layer(2, 5, STRIP_SP + 3, c, c, 3, 1, pad, bf16=bf16, note="strip-pad"))
    cases.append(layer(2, 5, STRIP_SP + 1, c, 2 * c, 3, 1, 1, bf16=bf16, note="strip-a256"))
    cases.append(layer(2, 6, 2 * STRIP_SP + 2, 2 * c, c, 4, 2, 1, bf16=bf16, note="strip-c256"))
    cases.append(layer(2, 3, STRIP_SP + 1, c, c, 4, 2, 1, transposed=True, bf16=bf16, note="strip-T"))
    return cases


def stencil_cases(bf16):
    cm, cases = _cm(bf16), []
    tw = C1_TW
    for lw in (1, tw - 1, tw, tw + 1):
        for odd in (0, 1):                                               # image width 2 LW | 2 LW + 1
            cases.append(layer(2, 5 + odd, 2 * lw + odd, 1, cm, 4, 2, 1, bf16=bf16, note=f"c1-lw{lw}"))
        cases.append(layer(2, 3, lw, cm, 1, 4, 2, 1, transposed=True, bf16=bf16, note=f"c1-lw{lw}"))
    cs = (8, C1_MAX_C) if bf16 else (4, 8, 36, C1_MAX_C - 4, C1_MAX_C)
    for C in cs:
        cases.append(layer(1, 6, 2 * tw + 2, 1, C, 4, 2, 1, bf16=bf16, note="c1-C"))
        cases.append(layer(1, 3, tw + 1, C, 1, 4, 2, 1, transposed=True, bf16=bf16, note="c1-C"))
    tall = max(C1_FWD_BLOCKS, C1_WGRAD_BLOCKS) + 1                        # 2049 tiles from a tall narrow image
    cases.append(layer(1, 2 * tall, 2, 1, cm, 4, 2, 1, bf16=bf16, note="c1-cap"))
    cases.append(layer(1, tall, 1, cm, 1, 4, 2, 1, transposed=True, bf16=bf16, note="c1-cap"))
    return cases


def rounding_cases(bf16):
    """Short chains only (K <= MAX_ROUND_K in every entry point: 3x3 x 32 channels, 16 taps x 16, at most 288 pixels)."""
    cm = _cm(bf16)
    c = 32
    return [layer(2, 9, 16, c, c - cm, 3, 1, 1, bf16=bf16, note="round"),                    # 288 products forward, 288 pixels in the weight gradient
            layer(2, 12, 12, 16, 40, 4, 2, 1, bf16=bf16, note="round"),
            layer(1, 6, 7, 16, 16, 4, 2, 1, transposed=True, bf16=bf16, note="round"),
            layer(2, 9, 16, 40, c, (2, 3), 1, (1, 1), bf16=bf16, out_hw=(9, 16), note="round"),
            layer(2, 12, 24, 1, 16, 4, 2, 1, bf16=bf16, note="round"),
            layer(1, 4, 8, 64, 1, 4, 2, 1, transposed=True, bf16=bf16, note="round")] + (
        [] if bf16 else [layer(2, 8, 9, 8, 8, 5, 1, 2, transposed=True, note="round")])


def pack_layers():
    """17 layers of mixed kinds: 34 packing jobs, past PACK_MAX_JOBS (a second launch)."""
    n = PACK_MAX_JOBS // 2 + 1
    pool = [layer(1, 4, 4, 8, 16, 3, 1, 1), layer(1, 4, 4, 64, 128, 3, 1, 1, bf16=True), layer(1, 4, 4, 16, 8, 4, 2, 1, bf16=True),
            layer(1, 2, 2, 8, 16, 4, 2, 1, transposed=True), layer(1, 4, 4, 1, 8, 4, 2, 1, bf16=True), layer(1, 2, 2, 16, 1, 4, 2, 1, transposed=True, bf16=True),
            layer(1, 2, 2, 8, 4, 3, 1, 0, transposed=True), layer(1, 4, 4, 128, 128, 4, 2, 1, transposed=True, bf16=True),
            layer(1, 4, 4, 8, 8, (2, 3), 1, (1, 1), out_hw=(4, 4)), layer(1, 4, 4, 1, 12, 4, 2, 1)]
    return [pool[i % len(pool)] for i in range(n)]


def probe_cases():
    out = []
    for bf in (False, True):
        out += gather_cases(bf) + wgrad_cases(bf) + strip_cases(bf) + stencil_cases(bf)
    return out + patch_cases()


def all_rounding_cases():
    return rounding_cases(False) + rounding_cases(True)
