"""The fp64 yardstick of the two kernel families with BatchNorm arithmetic folded into a matrix-core operand path: the ResBlock's
1x1 convolution (csrc/gemm_flat.hip, the BatchNorm-on-load operand of csrc/gemm_wgrad.hip) and the fused output layer (second half
of csrc/c1_mfma.hip, the col2im / loss epilogue of csrc/conv_api.hip).  Plain torch on the CPU, written out from include/nsg.h.
tests/test_fused_ref_host.py holds this file to torch.autograd; tests/test_gpu_fused_1x1_envelope.py and
tests/test_gpu_fused_output_envelope.py hold the kernels to it.

Every function takes the operands as the kernel is handed them (bf16 tensors, fp32 statistics and parameters) and widens them.

Documented roundings.  The kernels round some intermediates to bf16 on the way into the MFMA; the reference (round_ops=True)
rounds the same ones and multiplies the rounded values, so what is left between kernel and reference is fp32 accumulation order
and the store rounding:
    1x1 family      a = relu(bn(x)) and w (forward, both weight gradients); dh (stored, then multiplied) and w (data gradient)
    output layer    forward: a and w.  backward: the data gradient da is rebuilt from (hi, lo) bf16 splits of the gradient image and
                    of w (c1_mfma.hip: "h to ~2^-17 relative"), so da takes NO bf16 rounding here and carries DA_SPLIT * sum |term|
                    instead; the weight gradient multiplies bf16(patch of the gradient image) with bf16(a) ("bf16 operands, as
                    every weight gradient of this mode"): both rounded here.  du is rounded where it is stored.

Fragile elements.  A rounded intermediate v is formed in fp32 by the kernel, each rounding at most 2^-24 of the magnitudes v is
formed FROM (`mag`).  a = max(fma(x, fs, off), 0): three roundings (fs = invstd * gamma, off = fma(-mean, fs, beta), the fma), at
most 3 * 2^-24 (|x fs| + |mean fs| + |beta|); its window is WINDOW_A * mag = 4 * 2^-24 * mag.  dh = fma(sc, dy, -fma(k1, h, k2)): 1 /
M, sc, k1 (three products), k2 and the two fmas, at most eight roundings of |sc| (|dy| + |dbeta / M|) + |k1| (|h| + |mean|); its
window is WINDOW * mag = 8 * 2^-24 * mag.  Both are relative to the magnitudes, not to v: they are the same where nothing cancels
(mag is 2 to 3 |a| in an ordinary channel, so the window of a is the 8 * 2^-24 |a| one would grant it there), and in a channel
whose mean dwarfs its spread the fp32 error IS relative to the mean.  Where fp64 puts v within the window of a bf16 rounding midpoint or of
the ReLU threshold, the kernel may round the other way: the element is fragile, it is NOT excluded, and its possible change (one
bf16 ulp plus the window; for a ReLU decision in a backward pass the whole term) times the magnitude of what it is multiplied
with is added to the bound of every output it feeds (`frag`).  Elements with |v| <= 2 * window are "noise": the value is its own
rounding residue (every dh at M = 1, where the BatchNorm backward is identically zero).  They are bounded the same way but are not
counted in the fragile share, which is a statement about the rounding direction of well-defined values."""
import types

import torch
import torch.nn.functional as F

from tests.helpers import bn_ref64 as BN

U32 = 2.0 ** -24                    # unit roundoff of fp32
UB = 2.0 ** -8                      # unit roundoff of bf16 (8 significant bits)
WINDOW = 8.0 * U32               # of dh, du and the backward ReLU decisions
WINDOW_A = 4.0 * U32             # of the staged activation a
DA_SPLIT = 3.0 * 2.0 ** -18 + 52.0 * U32   # the (hi, lo) split product: two representation errors and the dropped lo * lo term, each
#                                            2^-18 of a term; 3 MFMAs of 16 products + the bias add in fp32
MAX_CHAIN = 300                     # 300 * 2^-24 * 1.1 = 1.97e-5 <= the 2e-5 of the fp32 sums' bound
SUM_COEF = 2e-5
MAX_SLABS = 1024                    # nsg_common.h NSG_MAX_SLABS: the output layer's backward passes run at most this many blocks

# ---- geometry of the kernels, restated (tests/test_fused_ref_host.py asserts the case tables against these) -------------------
FLAT_ROWS, FLAT_BLOCKS = 128, 512           # flat_gemm_kernel: rows per tile, persistent blocks (gemm_flat.hip ROWS, FLAT_BLOCKS)
WIDE_ROWS, WIDE_BLOCKS = 64, 256            # flat_wide_kernel (C = 256): WROWS, FLAT_WIDE_BLOCKS
FUSED_ROWS, FUSED_BLOCKS = 128, 256         # flat_bwd_fused_kernel (C = 128): ROWS, FLAT_FUSED_BLOCKS
WAVE_ROWS = 32                              # rows of a tile one wave multiplies
WGRAD_ROUND, WGRAD_MIN_ROWS, WGRAD_KP = 512, 256, 32   # gemm_wgrad.hip plan_slabs: blocks of one round, least rows per slab, chunk
DOTS_ROWS, OUT_TILE = 128, 64               # bnrelu_dots_kernel's row block; the backward passes' pixels per tile (c1_geom.h TW)


def f64(t):
    return None if t is None else t.detach().to("cpu").double()


def cdiv(a, b):
    return -(-a // b)


def rb(t):
    """fp64 -> fp32 -> bf16 (round to nearest even), widened again: what v_cvt_pk_bf16_f32 makes of the kernel's fp32 value."""
    return t.float().bfloat16().double()


def bf16_ulp(v):
    _, e = torch.frexp(v)           # |v| = m 2^e, m in [0.5, 1): 8 significant bits -> ulp 2^(e - 8)
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 8))


def round_fragile(v, mag, relu_t=None, window=WINDOW):
    """-> rounded v, delta (the change a fragile element may show, 0 elsewhere), fragile mask (counted), noise mask (not counted).
    relu_t: the pre-activation when v = max(t, 0): an element within the window of the threshold is fragile too."""
    win = window * mag
    ulp = bf16_ulp(v)
    q = v.abs() / ulp.clamp_min(1e-300)
    dist = (q - torch.floor(q) - 0.5).abs() * ulp
    near = (v != 0) & (dist <= win)
    if relu_t is not None:
        near = near | ((relu_t.abs() <= win) & (win > 0))
    else:
        near = near | ((v == 0) & (mag > 0))
    noise = near & (v.abs() <= 2.0 * win)
    delta = torch.where(near, ulp + 2.0 * win, torch.zeros_like(v))
    return rb(v), delta, near & ~noise, noise


def sum_coef(chain):
    """Coefficient of sum |term| in an fp32 sum's bound: the class figure up to MAX_CHAIN additions, the chain's own beyond."""
    return SUM_COEF if chain < MAX_CHAIN else chain * U32 * 1.1


# ----------------------------------------------------------------------------------------------------------------------
# the staging transform both families share: a = relu((x - mean) * (invstd * gamma) + beta), rounded to bf16
# ----------------------------------------------------------------------------------------------------------------------
def staged_activation(x, mean, invstd, gamma, beta, round_ops=True):
    """x [M][C] -> namespace(a, t, delta, fragile, noise, mag)."""
    x, mean, invstd, gamma, beta = f64(x), f64(mean), f64(invstd), f64(gamma), f64(beta)
    fs = invstd * gamma
    t = (x - mean) * fs + beta
    mag = x.abs() * fs.abs() + (mean * fs).abs() + beta.abs()
    a = t.clamp_min(0.0)
    if not round_ops:
        z = torch.zeros_like(a)
        return types.SimpleNamespace(a=a, t=t, delta=z, fragile=z.bool(), noise=z.bool(), mag=mag)
    a_r, delta, frag, noise = round_fragile(a, mag, relu_t=t, window=WINDOW_A)
    return types.SimpleNamespace(a=a_r, t=t, delta=delta, fragile=frag, noise=noise, mag=mag)


def relu_decision(x, mean, invstd, gamma, beta):
    """-> mask (t > 0 in fp64), fragile (either decision is correct): a backward pass's ReLU mask, as bn_ref64.fragile states it
    (t = (x - mean) * (invstd * gamma) + beta in fp32: within 8 * 2^-24 of the magnitudes it is formed from)."""
    x, mean, invstd, gamma, beta = f64(x), f64(mean), f64(invstd), f64(gamma), f64(beta)
    mag = (x - mean).abs() * invstd * gamma.abs() + beta.abs()
    t = (x - mean) * (invstd * gamma) + beta
    return t > 0.0, (t.abs() <= WINDOW * mag) & (mag > 0)


# ----------------------------------------------------------------------------------------------------------------------
# the ResBlock's 1x1 convolution; tensors [M][C], w [C][C] = [out][in]
# ----------------------------------------------------------------------------------------------------------------------
def conv1x1_forward(x, mean, invstd, gamma, beta, w, bias, round_ops=True):
    """y = a @ w.T + bias -> namespace(y, terms (sum |term| per element), frag (the fragile operands' part of the bound), K
    (products per element + 4), act (staged_activation's namespace))."""
    act = staged_activation(x, mean, invstd, gamma, beta, round_ops)
    C = act.a.shape[1]
    w2 = f64(w).reshape(C, C)
    w2 = rb(w2) if round_ops else w2
    b = torch.zeros(C, dtype=torch.float64) if bias is None else f64(bias)
    y = act.a @ w2.t() + b
    terms = act.a.abs() @ w2.abs().t() + b.abs()
    frag = act.delta @ w2.abs().t()
    return types.SimpleNamespace(y=y, terms=terms, frag=frag, K=C + 4, act=act)


def mfma_bound(want, terms, frag, K, stored_bf16):
    return (UB * want.abs() if stored_bf16 else 0.0) + K * U32 * terms + frag


def conv1x1_backward(h, dy, mean, invstd, gamma, dgamma, dbeta, w, round_ops=True):
    """dh = gamma invstd (dy - dbeta / M - xhat dgamma / M), dx = dh @ w, column sums of dh (of the fp32 values: the kernels sum dh
    before its store rounding).  -> namespace(dh, dh_r (as multiplied), dh_mag, dh_delta, fragile, noise, dx, dx_terms, dx_frag, K,
    colsum, colsum_terms, colsum_own)."""
    h, dy, mean, invstd, gamma, dgamma, dbeta = (f64(t) for t in (h, dy, mean, invstd, gamma, dgamma, dbeta))
    M, C = h.shape
    w2 = f64(w).reshape(C, C)
    sc = gamma * invstd
    k1 = sc * invstd * dgamma / M
    dh = sc * (dy - dbeta / M) - k1 * (h - mean)
    mag = sc.abs() * (dy.abs() + (dbeta / M).abs()) + k1.abs() * (h.abs() + mean.abs())
    if round_ops:
        dh_r, delta, frag, noise = round_fragile(dh, mag)
        w2 = rb(w2)
    else:
        dh_r, delta = dh, torch.zeros_like(dh)
        frag = noise = torch.zeros_like(dh).bool()
    return types.SimpleNamespace(dh=dh, dh_r=dh_r, dh_mag=mag, dh_delta=delta, fragile=frag, noise=noise, dx=dh_r @ w2,
                                 dx_terms=dh_r.abs() @ w2.abs(), dx_frag=delta @ w2.abs(), K=C + 4, colsum=dh.sum(0),
                                 colsum_terms=dh.abs().sum(0), colsum_own=WINDOW * mag.sum(0))


def prev_sums(prev_x, dx, mean, invstd, gamma, beta):
    """The backward sums of the BatchNorm + ReLU in FRONT of the conv over (prev_x, dx): g = dx where the pre-activation is
    positive, dbeta = sum g, dgamma = sum g xhat.  dx: the values the kernel sums, i.e. dx AS STORED (bf16: exact operands, so
    there is no `own` part).  -> namespace(dgamma, dbeta, terms_dgamma, terms_dbeta, flip_dgamma, flip_dbeta): flip = the whole
    terms of the fragile ReLU decisions."""
    x, g, mean, invstd = f64(prev_x), f64(dx), f64(mean), f64(invstd)
    mask, frag = relu_decision(prev_x, mean, invstd, gamma, beta)
    xhat = (x - mean) * invstd
    z = torch.zeros_like(g)
    gm = torch.where(mask, g, z)
    return types.SimpleNamespace(dgamma=(gm * xhat).sum(0), dbeta=gm.sum(0), terms_dgamma=(gm * xhat).abs().sum(0),
                                 terms_dbeta=gm.abs().sum(0), flip_dgamma=torch.where(frag, (g * xhat).abs(), z).sum(0),
                                 flip_dbeta=torch.where(frag, g.abs(), z).sum(0), fragile=frag)


def conv1x1_wgrad(dh_r, dh_delta, act):
    """dw[o][i] = sum_m dh[m][o] a[m][i] over the operands AS MULTIPLIED: dh_r (bf16 values; dh_delta their fragile part or None
    when dh is handed to the kernel as a stored tensor), act = staged_activation of the conv's input.  -> dw, terms, frag."""
    dh_r = f64(dh_r)
    dw = dh_r.t() @ act.a
    terms = dh_r.abs().t() @ act.a.abs()
    frag = dh_r.abs().t() @ act.delta
    if dh_delta is not None:
        frag = frag + dh_delta.t() @ (act.a.abs() + act.delta)
    return dw, terms, frag


# ---- fp32 addition chains of the 1x1 family (the longest chain behind one output; partials are then added in double) ----------
def flat_geom(M, C):
    """-> rows per tile, blocks, tiles of the longest block, threads per channel group (RSTEP), pieces per thread and tile."""
    rows, cap, nt = (WIDE_ROWS, WIDE_BLOCKS, 512) if C == 256 else (FLAT_ROWS, FLAT_BLOCKS, 256)
    tiles = cdiv(M, rows)
    blocks = min(tiles, cap)
    rstep = nt // (C // 8)
    return rows, blocks, cdiv(tiles, blocks), rstep, rows // rstep


def flat_chain(M, C):
    """Column sums of the flat kernels (dh_colsum, prev_*): a thread's pieces over its tiles, then the channel group's threads."""
    _, _, per_block, rstep, pieces = flat_geom(M, C)
    return pieces * per_block + rstep


def fused_geom(M):
    tiles = cdiv(M, FUSED_ROWS)
    blocks = min(tiles, FUSED_BLOCKS)
    return blocks, cdiv(tiles, blocks)


def fused_chain(M):
    """flat_bwd_fused_kernel (512 threads, C = 128: 32 threads per channel group, 4 pieces per tile)."""
    _, per_block = fused_geom(M)
    return 4 * per_block + 32


def fused_dw_chain(M):
    """dw of the one-pass form: the MFMA accumulator runs over all rows of the block's tiles; the block partials are added in fp32."""
    blocks, per_block = fused_geom(M)
    return min(M, FUSED_ROWS * per_block) + blocks


def wgrad_slabs(M, C):
    """gemm_wgrad.hip plan_slabs for the 1x1 weight gradient (one tap, A = C): -> nslab, rows per slab."""
    tiles = cdiv(C, 128) * cdiv(C, 128 if C > 32 else 32)
    want = max(1, min(WGRAD_ROUND // tiles, cdiv(M, WGRAD_MIN_ROWS), 512))
    rows = cdiv(cdiv(M, want), WGRAD_KP) * WGRAD_KP
    return cdiv(M, rows), rows


def wgrad_chain(M, C):
    nslab, rows = wgrad_slabs(M, C)
    return min(M, rows) + nslab         # the accumulator over a slab's rows, then wgrad_reduce_kernel's fp32 sum over the slabs


# ----------------------------------------------------------------------------------------------------------------------
# the fused output layer: u [B][H][W][C], w [C][16] = (C, 1, 4, 4), image [B][2H][2W]
# ----------------------------------------------------------------------------------------------------------------------
def _nchw(t, B, H, W, C):
    return t.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def output_forward(u, mean, invstd, gamma, beta, w, bias, round_ops=True):
    """pre = bias + ConvTranspose2d(C, 1, 4, 2, 1)(a) -> namespace(pre [B][2H][2W], terms, frag, K, act).  K: at most four taps of C
    products reach a pixel, then the taps and the bias are added: 4 C + 4 (+ 4)."""
    B, H, W, C = u.shape
    act = staged_activation(f64(u).reshape(-1, C), mean, invstd, gamma, beta, round_ops)
    w4 = f64(w).reshape(C, 1, 4, 4)
    w4 = rb(w4) if round_ops else w4
    b = torch.zeros(1, dtype=torch.float64) if bias is None else f64(bias).reshape(1)
    ct = lambda a, ww, bb: F.conv_transpose2d(_nchw(a, B, H, W, C), ww, bb, stride=2, padding=1)[:, 0]  # noqa: E731
    pre = ct(act.a, w4, b)
    terms = ct(act.a.abs(), w4.abs(), b.abs())
    frag = ct(act.delta, w4.abs(), None)
    return types.SimpleNamespace(pre=pre, terms=terms, frag=frag, K=4 * C + 8, act=act)


TANH_RTOL, TANH_ATOL = 1e-6, 1e-7       # tests/test_gpu_elementwise_envelope.py's figure for the library's tanh


def mse_epilogue(image, target, grad_scale):
    """The loss epilogue of nsg_bn_relu_c1convt_forward_mse on an image x_tilde [B][2H][2W] (the kernel's STORED image, checked
    by itself): loss = mean((pad(x_tilde) - target)^2) over the target's [B][2H][T], dpre = grad_scale 2 / (B 2H T) (x_tilde -
    target) (1 - x_tilde^2), dbias = sum dpre.  -> loss, dpre, dpre_mag (what dpre is formed from), dbias, sum |dpre|."""
    v, tg = f64(image), f64(target)
    Bn, HH, WW = v.shape
    tg = tg.reshape(Bn, HH, -1)
    T = tg.shape[2]
    pad = torch.zeros_like(tg)
    pad[:, :, :WW] = v
    loss = ((pad - tg) ** 2).mean()
    gs = grad_scale * 2.0 / (Bn * HH * T)
    d = v - tg[:, :, :WW]
    dpre = gs * d * (1.0 - v * v)
    mag = abs(gs) * (v.abs() + tg[:, :, :WW].abs()) * (1.0 + v * v)
    return loss, dpre, mag, dpre.sum(), dpre.abs().sum()


def output_backward(u, mean, invstd, gamma, beta, w, dy, dgamma_used=None, dbeta_used=None, round_ops=True):
    """The chain BatchNorm -> ReLU -> ConvTranspose2d backwards from dy [B][2H][2W] (the gradient at the conv's output).
    da = the conv's data gradient (unrounded: see the module docstring), g = da where the pre-activation is positive, dbeta = sum g,
    dgamma = sum g xhat, du = gamma invstd (g - dbeta / M - xhat dgamma / M) with the dgamma / dbeta THE KERNEL USED when given (its
    second pass reads what its first pass wrote; they are checked by themselves), dw[c][t] = sum bf16(patch(dy))[t] bf16(a)[c].
    -> namespace; *_terms = sum |term|, *_own = roundings of the kernel's own values that a sum adds up, *_flip = whole terms of
    fragile ReLU decisions."""
    B, H, W, C = u.shape
    M = B * H * W
    x = f64(u).reshape(M, C)
    mean, invstd, gamma, beta = f64(mean), f64(invstd), f64(gamma), f64(beta)
    w4 = f64(w).reshape(C, 1, 4, 4)
    dy4 = f64(dy).reshape(B, 1, 2 * H, 2 * W)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(M, C)  # noqa: E731
    da = rows(F.conv2d(dy4, w4, None, stride=2, padding=1))
    da_terms = rows(F.conv2d(dy4.abs(), w4.abs(), None, stride=2, padding=1))
    da_err = DA_SPLIT * da_terms
    act = staged_activation(x, mean, invstd, gamma, beta, round_ops)
    mask, frag = act.t > 0.0, (act.t.abs() <= WINDOW * act.mag) & (act.mag > 0)         # the passes decide the ReLU from fma(u, fs, off), as the forward
    z = torch.zeros_like(da)
    g = torch.where(mask, da, z)
    g_err = torch.where(mask | frag, da_err, z)
    g_flip = torch.where(frag, da.abs(), z)
    xhat = (x - mean) * invstd
    o = types.SimpleNamespace(fragile=frag, da=da)
    o.dbeta, o.dgamma = g.sum(0), (g * xhat).sum(0)
    o.dbeta_terms, o.dgamma_terms = g.abs().sum(0), (g * xhat).abs().sum(0)
    o.dbeta_own, o.dgamma_own = g_err.sum(0), (g_err * xhat.abs()).sum(0)
    o.dbeta_flip, o.dgamma_flip = g_flip.sum(0), (g_flip * xhat.abs()).sum(0)
    dg = o.dgamma if dgamma_used is None else f64(dgamma_used)
    db = o.dbeta if dbeta_used is None else f64(dbeta_used)
    sc = gamma * invstd
    k1 = sc * invstd * dg / M
    o.du = sc * (g - db / M) - k1 * (x - mean)
    mag = sc.abs() * (g.abs() + (db / M).abs()) + k1.abs() * (x.abs() + mean.abs())
    o.du_own = WINDOW * mag + sc.abs() * g_err              # the fp32 expression's roundings and the split product's
    o.du_flip = sc.abs() * g_flip
    o.du_colsum, o.du_colsum_terms = o.du.sum(0), o.du.abs().sum(0)
    o.du_colsum_own, o.du_colsum_flip = o.du_own.sum(0), o.du_flip.sum(0)
    # the weight gradient: both MFMA operands are bf16
    dyr = rb(dy4) if round_ops else dy4

    def wg(a, d):
        ww = torch.zeros(C, 1, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(_nchw(a, B, H, W, C), ww, None, stride=2, padding=1).mul(d).sum().backward()
        return ww.grad.reshape(C, 16)

    o.dw, o.dw_terms, o.dw_frag = wg(act.a, dyr), wg(act.a.abs(), dyr.abs()), wg(act.delta, dyr.abs())
    o.dbias, o.dbias_terms = dy4.sum(), dy4.abs().sum()
    o.act = act
    return o


# ---- geometry and chains of the output layer ---------------------------------------------------------------------------------
def dots_blocks_cap(C):
    return 512 if C > 128 else 1024


def out_tiles(B, H, W):
    return B * H * cdiv(W, OUT_TILE)


def out_chain(B, H, W):
    """The longest fp32 chain of a per-channel sum of the backward passes (dgamma, dbeta, du_colsum): a lane adds at most 32 of a
    tile's pixels (fewer in a narrow row: the rest are zeros, which round nothing), over its block's tiles, then its partner lane."""
    tiles = out_tiles(B, H, W)
    return min(32, W) * cdiv(tiles, min(tiles, MAX_SLABS)) + 1


def out_dw_chain(B, H, W):
    tiles = out_tiles(B, H, W)
    return min(OUT_TILE, W) * cdiv(tiles, min(tiles, MAX_SLABS))


# ----------------------------------------------------------------------------------------------------------------------
# the cases and their inputs (one generator per case, fixed draw order; the GPU tests upload exactly these)
# ----------------------------------------------------------------------------------------------------------------------
HARD_RELU, HARD_MEAN = 1, 2         # channel 1: beta = -8, the ReLU passes almost nothing; channel 2: mean >> std (6 +- 0.2)


def boundary_ms(C):
    """M on each side of every boundary of the flat kernels' geometry at width C, and of the weight gradient's first slab split."""
    rows, blocks = flat_geom(1, C)[0], (WIDE_BLOCKS if C == 256 else FLAT_BLOCKS)
    return [1, WAVE_ROWS - 1, rows - 1, rows, rows + 1, WGRAD_MIN_ROWS, WGRAD_MIN_ROWS + 1, blocks * rows, blocks * rows + 1]


def wgrad_cap_m(C):
    """The first M at which the 1x1 weight gradient runs its most slabs."""
    tiles = cdiv(C, 128) * cdiv(C, 128 if C > 32 else 32)
    return (min(WGRAD_ROUND // tiles, 512) - 1) * WGRAD_MIN_ROWS + 1


RAGGED_M = 3 * FLAT_BLOCKS * FLAT_ROWS + 77         # 196 685 rows: three to four tiles per persistent block, the last one ragged
CASES_1X1 = ([(M, 128) for M in boundary_ms(128) + [FUSED_BLOCKS * FUSED_ROWS, FUSED_BLOCKS * FUSED_ROWS + 1, wgrad_cap_m(128), RAGGED_M]]
             + [(M, 256) for M in boundary_ms(256) + [wgrad_cap_m(256)]]
             + [(M, 32) for M in boundary_ms(32)]
             + [(M, 64) for M in (1, FLAT_ROWS + 1, FLAT_BLOCKS * FLAT_ROWS + 1)])


# seed shifts of the cases whose first draw missed a condition of tests/test_fused_ref_host.py: more than 1e-3 of an intermediate
# next to a rounding decision (a small case holds a few thousand elements: three or four fragile ones are the whole allowance),
# or the fragile part over half of a bound in more than 1 % of the outputs (an image pixel is fed by up to 4 C activations: one in
# six holds a fragile one).  Found on the CPU with the reference alone, before any kernel ran
SEEDS_1X1 = {(31, 128): 3, (256, 128): 3, (130817, 128): 2, (31, 256): 4, (63, 256): 3, (31, 32): 2, (65537, 64): 2,
             (16384, 256): 6, (16385, 256): 7}      # (these two: whole columns of a next to a midpoint -- x is bf16, so a channel's a takes
#                                                       a few hundred values -- put the fragile part over half of dw's bound in 2 % of its entries)
SEEDS_OUT = {((2, 3, 1), 128): 1, ((2, 5, 130), 128): 3, ((1, 2, 64), 128): 1, ((1, 3, 43), 128): 2, ((1, 1, 63), 128): 1,
             ((1, 1, 64), 128): 2, ((1, 1024, 3), 128): 3, ((1, 1025, 3), 128): 9, ((5, 205, 1), 128): 1, ((1, 1, 65), 256): 1,
             ((1, 1024, 3), 256): 3, ((1, 1025, 3), 256): 6, ((5, 205, 1), 256): 2, ((1, 1025, 3), 32): 2, ((5, 205, 1), 32): 6,
             ((2, 5, 130), 64): 3, ((1, 1025, 3), 64): 5, ((2, 5, 130), 96): 19, ((1, 1025, 3), 96): 1}


def inputs_1x1(M, C):
    g = torch.Generator().manual_seed(1000003 * M + 1009 * C + SEEDS_1X1.get((M, C), 1))
    c = types.SimpleNamespace(M=M, C=C, tag=f"M={M} C={C}")

    def tensor():
        t = torch.randn(M, C, generator=g) * 1.3 + 0.4
        t[:, HARD_MEAN] = 6.0 + 0.2 * torch.randn(M, generator=g)
        return t.bfloat16()

    c.x, c.h = tensor(), tensor()
    c.dy = torch.randn(M, C, generator=g).bfloat16()
    c.w = torch.randn(C, C, 1, 1, generator=g) * 0.15
    c.bias = torch.randn(C, generator=g) * 0.1
    c.gamma, c.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    c.beta[HARD_RELU] = -8.0
    c.gamma2 = torch.rand(C, generator=g) + 0.5
    c.rm, c.rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    return c


def probe_1x1(M, C):
    """The integer probe: identity BatchNorm, w = the identity, x and dy small non-negative integers (exact in bf16); the first and
    last row are non-zero in every channel, so a lost or doubled row there changes every sum."""
    g = torch.Generator().manual_seed(7 * M + C)
    c = types.SimpleNamespace(M=M, C=C, tag=f"probe M={M} C={C}")
    c.x = torch.randint(0, 4, (M, C), generator=g).float()
    c.dy = torch.randint(0, 4, (M, C), generator=g).float()
    edge = 1.0 + (torch.arange(C) % 3).float()
    c.x[0], c.x[M - 1], c.dy[0], c.dy[M - 1] = edge, edge.flip(0), edge.flip(0), edge
    c.x, c.dy = c.x.bfloat16(), c.dy.bfloat16()
    c.w = torch.eye(C).reshape(C, C, 1, 1).contiguous()
    c.zero, c.one = torch.zeros(C), torch.ones(C)
    return c


# ---- the output layer: (B, H, W) ----------------------------------------------------------------------------------------------
TILE_EDGE = [(1, 1, OUT_TILE - 1), (1, 1, OUT_TILE), (1, 1, OUT_TILE + 1)]
BWD_CAP = [(1, MAX_SLABS, 3), (1, MAX_SLABS + 1, 3), (5, (MAX_SLABS + 1) // 5, 1)]          # 1024 | 1025 | 1025 tiles
SMALL = [(1, 1, 1), (2, 3, 1), (2, 5, 130), (1, 2, OUT_TILE), (1, 3, 43)]                    # (1, 2, 64): M = 128; (1, 3, 43): M = 129


def fwd_cap(C):
    """M on each side of the dots kernel's block cap: (1, H, 64) with M = cap * 128 rows, and (1, cap * 128 + 1, 1)."""
    m = dots_blocks_cap(C) * DOTS_ROWS
    return [(1, m // OUT_TILE, OUT_TILE), (1, m + 1, 1)]


CASES_OUT = ([(s, 128) for s in SMALL + TILE_EDGE + BWD_CAP + fwd_cap(128)]
             + [(s, 256) for s in TILE_EDGE + BWD_CAP + fwd_cap(256)]
             + [(s, 32) for s in TILE_EDGE + BWD_CAP]
             + [(s, C) for C in (64, 96) for s in ((1, 1, 1), (2, 5, 130), (1, MAX_SLABS + 1, 3))])
MSE_SHAPES = [(2, 3, 1), (1, 1, OUT_TILE + 1), (2, 5, 130)]
MSE_EXTRA = (0, 1, 37)              # T = 2 W + these
PROBE_OUT = [((1, MAX_SLABS + 1, 3), 128), ((1, 1, OUT_TILE + 1), 128), (fwd_cap(128)[1], 128), (fwd_cap(256)[1], 256),
             ((1, MAX_SLABS + 1, 3), 32)]


def inputs_out(shape, C):
    B, H, W = shape
    g = torch.Generator().manual_seed(1000003 * B + 1009 * H + 31 * W + C + SEEDS_OUT.get((shape, C), 0))
    c = types.SimpleNamespace(B=B, H=H, W=W, C=C, M=B * H * W, tag=f"B={B} H={H} W={W} C={C}")
    u = torch.randn(B, H, W, C, generator=g) * 1.5 + 0.5
    u[..., HARD_MEAN] = 6.0 + 0.2 * torch.randn(B, H, W, generator=g)
    c.u = u.bfloat16()
    c.w = torch.randn(C, 1, 4, 4, generator=g) * 0.2
    c.bias = torch.randn(1, generator=g) * 0.1
    c.gamma, c.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    c.beta[HARD_RELU] = -8.0
    c.dy = torch.randn(B, 2 * H, 2 * W, generator=g)
    c.target = torch.rand(B, 2 * H, 2 * W + max(MSE_EXTRA), generator=g)
    return c


def probe_out(shape, C):
    """Identity BatchNorm, u in {0..3}, integer taps on two channels, dy in {-2..2}: every product and partial sum is an integer."""
    B, H, W = shape
    g = torch.Generator().manual_seed(11 * B + 13 * H + 17 * W + C)
    c = types.SimpleNamespace(B=B, H=H, W=W, C=C, M=B * H * W, tag=f"probe B={B} H={H} W={W} C={C}")
    c.u = torch.randint(0, 4, (B, H, W, C), generator=g).float().bfloat16()
    c.w = torch.zeros(C, 16)
    c.w[3] = 1.0 + (torch.arange(16) % 3).float()
    c.w[C - 1] = (torch.arange(16) % 2).float()
    c.w = c.w.reshape(C, 1, 4, 4)
    c.dy = torch.randint(-2, 3, (B, 2 * H, 2 * W), generator=g).float()
    c.zero, c.one = torch.zeros(C), torch.ones(C)
    return c


def host_stats(x):
    """mean, invstd of [M][C] as fp32: the CPU stand-in for what ops.bn_stats hands the kernels."""
    mean, invstd, _ = BN.stats(x)
    return mean.float(), invstd.float()
