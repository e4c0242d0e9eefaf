// Element-wise pieces of the latent prior (the reference's GatedPixelCNN over the code-index grid, src/models.py:219-341,
// SURVEY.md section 8f row 1); its convolutions run on the conv kernels of the main path.
//   gated activation  y = tanh(a) * sigmoid(b),  (a, b) = the two channel halves of x (+ a per-clip conditioning row)
//                     src/models.py:219-226 (GatedActivation) with the class embedding add of :268,:274 folded in;
//                     the training step's forms: the gate of a sum of two tensors (the sum never stored) and a backward
//                     that also forms the per-clip column sums of dx (the gradient of the conditioning rows);
//   cross-entropy     mean over rows of  logsumexp(l) - l[target]  and its gradient (what F.cross_entropy computes on
//                     the prior's logits); the masked form leaves rows with a negative target out and returns per-clip sums.
// fp32, NHWC rows [M][channels]; deterministic (fixed-order reductions).
#include "nsg_reduce.h"
#include <math.h>

namespace {

// The two channel halves of row m at columns c .. c+3:  (x (+ x2)) + cond, in that order of additions (x2: the second
// summand of the gate-of-a-sum forms, so that the result equals nsg_add followed by the plain gate bit for bit).
template <bool SUM>
__device__ __forceinline__ void gate_load(const float *__restrict__ x, const float *__restrict__ x2, const float *__restrict__ cond, int64_t m,
                                          int c, int C, int64_t rows_per_clip, v4f &a, v4f &b)
{
    a = *reinterpret_cast<const v4f *>(x + m * 2 * C + c);
    b = *reinterpret_cast<const v4f *>(x + m * 2 * C + C + c);
    if (SUM) {
        a += *reinterpret_cast<const v4f *>(x2 + m * 2 * C + c);
        b += *reinterpret_cast<const v4f *>(x2 + m * 2 * C + C + c);
    }
    if (cond) {
        const float *cr = cond + (m / rows_per_clip) * 2 * C;
        a += *reinterpret_cast<const v4f *>(cr + c);
        b += *reinterpret_cast<const v4f *>(cr + C + c);
    }
}

// d/da = dy * s * (1 - t^2),  d/db = dy * t * s * (1 - s)
__device__ __forceinline__ void gate_grad(const v4f &a, const v4f &b, const v4f &g, v4f &da, v4f &db)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t = tanhf(a[e]);
        const float s = 1.f / (1.f + expf(-b[e]));
        da[e] = g[e] * s * (1.f - t * t);
        db[e] = g[e] * t * s * (1.f - s);
    }
}

// x (and x2 when SUM) [M][2C], cond [B][2C] or null (row m belongs to clip m / rows_per_clip), y [M][C]
template <bool SUM>
__global__ __launch_bounds__(256) void gated_fwd_kernel(const float *__restrict__ x, const float *__restrict__ x2, const float *__restrict__ cond,
                                                        float *__restrict__ y, int64_t M, int C, int64_t rows_per_clip)
{
    const int C4 = C >> 2;
    const int64_t total = M * C4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / C4;
        const int c = (int)(i - m * C4) * 4;
        v4f a, b;
        gate_load<SUM>(x, x2, cond, m, c, C, rows_per_clip, a, b);
        v4f o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = tanhf(a[e]) * (1.f / (1.f + expf(-b[e])));
        *reinterpret_cast<v4f *>(y + m * C + c) = o;
    }
}

// dx [M][2C] from dy [M][C]
template <bool SUM>
__global__ __launch_bounds__(256) void gated_bwd_kernel(const float *__restrict__ x, const float *__restrict__ x2, const float *__restrict__ cond,
                                                        const float *__restrict__ dy, float *__restrict__ dx, int64_t M, int C,
                                                        int64_t rows_per_clip)
{
    const int C4 = C >> 2;
    const int64_t total = M * C4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / C4;
        const int c = (int)(i - m * C4) * 4;
        v4f a, b, da, db;
        gate_load<SUM>(x, x2, cond, m, c, C, rows_per_clip, a, b);
        gate_grad(a, b, *reinterpret_cast<const v4f *>(dy + m * C + c), da, db);
        *reinterpret_cast<v4f *>(dx + m * 2 * C + c) = da;
        *reinterpret_cast<v4f *>(dx + m * 2 * C + C + c) = db;
    }
}

// The same dx, and while it is written its per-clip column sums (the gradient of cond).  Block (b, sl) owns rows
// [sl * R, (sl + 1) * R) of clip b, R = ceil(rows_per_clip / slabs); thread (rg, cg) walks rows rg, rg + rgroups, ... of the slab
// at column group cg and sums its da / db in double; the row groups are then added in order rg = 0, 1, ... and written to
// partial[b][sl][2C]; gated_colsum_final_kernel adds the slabs in order.  Every order is fixed: no atomics.
template <bool SUM>
__global__ __launch_bounds__(256) void gated_bwd_colsum_kernel(const float *__restrict__ x, const float *__restrict__ x2,
                                                               const float *__restrict__ cond, const float *__restrict__ dy,
                                                               float *__restrict__ dx, int64_t rows_per_clip, int C, int slabs,
                                                               double *__restrict__ partial)
{
    __shared__ double red[256 * 8];
    const int C4 = C >> 2;
    const int rgroups = 256 / C4;
    const int tid = threadIdx.x;
    const int cg = tid % C4, rg = tid / C4;
    const int64_t b = blockIdx.x / slabs;
    const int sl = blockIdx.x % slabs;
    const int64_t R = (rows_per_clip + slabs - 1) / slabs;
    const int64_t r0 = sl * R, r1 = min(rows_per_clip, r0 + R);
    const int c = cg * 4;
    double sa[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0};
    if (rg < rgroups) {
        for (int64_t r = r0 + rg; r < r1; r += rgroups) {
            const int64_t m = b * rows_per_clip + r;
            v4f a, bb, da, db;
            gate_load<SUM>(x, x2, cond, m, c, C, rows_per_clip, a, bb);
            gate_grad(a, bb, *reinterpret_cast<const v4f *>(dy + m * C + c), da, db);
            *reinterpret_cast<v4f *>(dx + m * 2 * C + c) = da;
            *reinterpret_cast<v4f *>(dx + m * 2 * C + C + c) = db;
#pragma unroll
            for (int e = 0; e < 4; ++e) { sa[e] += (double)da[e]; sb[e] += (double)db[e]; }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[tid * 8 + e] = sa[e]; red[tid * 8 + 4 + e] = sb[e]; }
    __syncthreads();
    if (tid < C4) {
        double *out = partial + (size_t)blockIdx.x * 2 * C;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double ta = 0.0, tb = 0.0;
            for (int g = 0; g < rgroups; ++g) { ta += red[(g * C4 + tid) * 8 + e]; tb += red[(g * C4 + tid) * 8 + 4 + e]; }
            out[tid * 4 + e] = ta;
            out[C + tid * 4 + e] = tb;
        }
    }
}
__global__ __launch_bounds__(256) void gated_colsum_final_kernel(const double *__restrict__ partial, int64_t B, int slabs, int C2,
                                                                 float *__restrict__ out)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= B * C2) return;
    const int64_t b = i / C2;
    const int c = (int)(i - b * C2);
    double s = 0.0;
    for (int k = 0; k < slabs; ++k) s += partial[((size_t)b * slabs + k) * C2 + c];
    out[i] = (float)s;
}

// One wave per row of K logits.  With mx = l[a] the row's maximum (a its first index) and s = sum over k != a of
// exp(l[k] - mx):  row_loss[m] = (mx - l[t]) + log1p(s);  dlogits = (softmax - onehot) * gscale (optional), softmax[k] =
// exp(l[k] - mx) / (1 + s).  Nothing is rounded at the scale of mx: the textbook (mx + log(sum)) - l[t] loses the loss of a
// confident row, or of logits that share a large offset, to the rounding of mx + log(sum); and 1 / (1 + s) - 1 at a confident
// target loses its gradient the same way, so that entry is -s / (1 + s).
// MASKED: a row whose target lies outside [0, K) is ignored -- row_loss 0, its dlogits exact zeros, its logits never read --
// and the gradient's scale is read from the device (ce_scale_kernel: grad_scale / n_valid).
template <bool MASKED>
__global__ __launch_bounds__(256) void cross_entropy_kernel(const float *__restrict__ logits, const int64_t *__restrict__ target,
                                                            int64_t M, int K, float gscale, const float *__restrict__ gscale_dev,
                                                            float *__restrict__ row_loss, float *__restrict__ dlogits)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    if (MASKED) gscale = gscale_dev[0];
    for (int64_t m = wave; m < M; m += nw) {
        if (MASKED) {
            const int64_t t64 = target[m];
            if (t64 < 0 || t64 >= K) {
                if (lane == 0) row_loss[m] = 0.f;
                if (dlogits)
                    for (int k = lane; k < K; k += 64) dlogits[m * K + k] = 0.f;
                continue;
            }
        }
        const float *l = logits + m * K;
        float mx = -INFINITY;
        int am = -1;                                   // first index of the maximum (-1: this lane holds no element)
        for (int k = lane; k < K; k += 64) {
            const float v = l[k];
            if (am < 0 || v > mx) { mx = v; am = k; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {     // (max, first index) is a total order: every lane ends with the same pair
            const float ov = __shfl_xor(mx, off, 64);
            const int oi = __shfl_xor(am, off, 64);
            if (oi >= 0 && (am < 0 || ov > mx || (ov == mx && oi < am))) { mx = ov; am = oi; }
        }
        float s = 0.f;
        for (int k = lane; k < K; k += 64)
            if (k != am) s += expf(l[k] - mx);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);     // xor butterfly: the same value, in the same order, on every lane
        const int t = (int)target[m];
        if (lane == 0) row_loss[m] = (t >= 0 && t < K) ? (mx - l[t]) + log1pf(s) : 0.f;
        if (dlogits) {
            const float inv = 1.f / (1.f + s);
            for (int k = lane; k < K; k += 64) {
                float g;
                if (k == am) g = (k == t) ? -s * inv : inv;
                else {
                    const float p = expf(l[k] - mx) * inv;
                    g = (k == t) ? p - 1.f : p;
                }
                dlogits[m * K + k] = g * gscale;
            }
        }
    }
}

// sum of n floats in double, two fixed-order stages
__global__ __launch_bounds__(256) void sum_partial_kernel(const float *__restrict__ v, int64_t n, double *__restrict__ partial)
{
    double acc = 0.0;
    const int64_t per = (n + gridDim.x - 1) / gridDim.x;
    const int64_t i0 = blockIdx.x * per, i1 = min(n, i0 + per);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) acc += (double)v[i];
    nsg_block_sum_walk256(acc, [&](double t) { partial[blockIdx.x] = t; });
}
__global__ void sum_final_kernel(const double *partial, int n, double denom, float *out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < n; ++i) t += partial[i];
        out[0] = (float)(t / denom);
    }
}


// ---- masked cross-entropy: counts, scale, per-clip sums ----
struct CeScalars { int64_t n_valid; float gscale; };

// count[b] = rows of clip b whose target lies in [0, K)
__global__ __launch_bounds__(256) void ce_count_kernel(const int64_t *__restrict__ target, int64_t rows_per_clip, int K, int64_t *__restrict__ count)
{
    __shared__ int red[256];
    const int64_t *t = target + blockIdx.x * rows_per_clip;
    int c = 0;
    for (int64_t r = threadIdx.x; r < rows_per_clip; r += 256) c += (t[r] >= 0 && t[r] < K) ? 1 : 0;
    red[threadIdx.x] = c;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {       // integers: any order gives the same sum
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) count[blockIdx.x] = red[0];
}
// n_valid = sum of the counts; gscale = grad_scale / n_valid (0 when nothing is valid); the counts also go to clip_count
__global__ __launch_bounds__(256) void ce_scale_kernel(const int64_t *__restrict__ count, int64_t B, float grad_scale, CeScalars *__restrict__ sc,
                                                       int64_t *__restrict__ clip_count)
{
    __shared__ long long red[256];
    long long n = 0;
    for (int64_t b = threadIdx.x; b < B; b += 256) {
        n += count[b];
        if (clip_count) clip_count[b] = count[b];
    }
    red[threadIdx.x] = n;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sc->n_valid = red[0];
        sc->gscale = red[0] > 0 ? grad_scale / (float)red[0] : 0.f;
    }
}
// clip_nll[b] = sum of the row losses of clip b (ignored rows hold 0), in double, two fixed-order stages inside one block:
// nothing outside the clip's own rows enters
__global__ __launch_bounds__(256) void ce_clip_nll_kernel(const float *__restrict__ row_loss, int64_t rows_per_clip, float *__restrict__ clip_nll)
{
    const float *v = row_loss + blockIdx.x * rows_per_clip;
    double acc = 0.0;
    for (int64_t r = threadIdx.x; r < rows_per_clip; r += 256) acc += (double)v[r];
    nsg_block_sum_walk256(acc, [&](double t) { clip_nll[blockIdx.x] = (float)t; });
}
__global__ void ce_masked_final_kernel(const double *partial, int n, const CeScalars *sc, float *out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < n; ++i) t += partial[i];
        out[0] = sc->n_valid > 0 ? (float)(t / (double)sc->n_valid) : 0.f;
    }
}

constexpr int SUM_BLOCKS = 256;
// nsg_cross_entropy's workspace: the rows' losses | the block sums
struct CeLayout { float *row_loss; double *partial; size_t bytes; };
inline CeLayout ce_layout(void *ws, int64_t M)
{
    NsgCarver c(ws);
    return {c.take<float>(nsg_align_up((size_t)M * sizeof(float), 256)), c.take<double>(SUM_BLOCKS * sizeof(double)), c.off};
}
struct CeMaskedLayout { size_t partial, count, scalars, bytes; };
inline CeMaskedLayout ce_masked_layout(int64_t M, int64_t B)
{
    CeMaskedLayout L;
    L.partial = nsg_align_up((size_t)M * sizeof(float), 256);
    L.count = L.partial + SUM_BLOCKS * sizeof(double);
    L.scalars = L.count + nsg_align_up((size_t)B * sizeof(int64_t), 256);
    L.bytes = L.scalars + 256;
    return L;
}
// slabs per clip of gated_bwd_colsum_kernel: about 2048 blocks in all, every block at least 4 passes over its row groups
inline int gate_slabs(int64_t B, int64_t rows_per_clip, int C)
{
    const int rgroups = 256 / (C / 4);
    int64_t most = rows_per_clip / (4 * rgroups);
    if (most > 64) most = 64;
    int64_t s = nsg_cdiv(2048, B);
    if (s > most) s = most;
    return (int)(s < 1 ? 1 : s);
}

}  // namespace

extern "C" {

int nsg_gated_activation_forward(const float *x, const float *cond, float *y, int64_t M, int32_t C, int64_t rows_per_clip, void *stream)
{
    NSG_REQUIRE(x && y && M > 0 && C > 0 && C % 4 == 0, NSG_E_INVALID, "nsg_gated_activation_forward: bad argument (C %% 4 == 0)");
    NSG_REQUIRE(!cond || rows_per_clip > 0, NSG_E_INVALID, "nsg_gated_activation_forward: rows_per_clip must be positive with a conditioning row");
    NSG_REQUIRE(nsg_aligned16(x) && nsg_aligned16(y) && (!cond || nsg_aligned16(cond)), NSG_E_INVALID, "nsg_gated_activation_forward: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(gated_fwd_kernel<false>, dim3(ew_blocks(M * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, (const float *)nullptr, cond, y, M, C,
                       cond ? rows_per_clip : 1);
    return nsg_check_launch("gated_fwd_kernel");
}

int nsg_gated_activation_backward(const float *x, const float *cond, const float *dy, float *dx, int64_t M, int32_t C, int64_t rows_per_clip,
                                  void *stream)
{
    NSG_REQUIRE(x && dy && dx && M > 0 && C > 0 && C % 4 == 0, NSG_E_INVALID, "nsg_gated_activation_backward: bad argument (C %% 4 == 0)");
    NSG_REQUIRE(!cond || rows_per_clip > 0, NSG_E_INVALID, "nsg_gated_activation_backward: rows_per_clip must be positive with a conditioning row");
    NSG_REQUIRE(nsg_aligned16(x) && nsg_aligned16(dy) && nsg_aligned16(dx) && (!cond || nsg_aligned16(cond)), NSG_E_INVALID,
                "nsg_gated_activation_backward: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(gated_bwd_kernel<false>, dim3(ew_blocks(M * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, (const float *)nullptr, cond, dy, dx, M, C,
                       cond ? rows_per_clip : 1);
    return nsg_check_launch("gated_bwd_kernel");
}

size_t nsg_cross_entropy_workspace_bytes(int64_t M) { return M > 0 ? ce_layout(nullptr, M).bytes : 0; }

int nsg_cross_entropy(const float *logits, const int64_t *target, int64_t M, int32_t K, float grad_scale, float *loss_out, float *dlogits,
                      void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(logits && target && loss_out && M > 0 && K > 0, NSG_E_INVALID, "nsg_cross_entropy: bad argument");
    const CeLayout L = ce_layout(workspace, M);
    NSG_REQUIRE(workspace && workspace_bytes >= L.bytes, NSG_E_WORKSPACE, "nsg_cross_entropy: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float *row_loss = L.row_loss;
    double *partial = L.partial;
    int64_t blocks = nsg_cdiv(M, 4);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(cross_entropy_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, logits, target, M, K, grad_scale / (float)M, (const float *)nullptr,
                       row_loss, dlogits);
    const int nb = (int)(M < SUM_BLOCKS ? M : SUM_BLOCKS);
    hipLaunchKernelGGL(sum_partial_kernel, dim3(nb), dim3(256), 0, s, row_loss, M, partial);
    hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(64), 0, s, partial, nb, (double)M, loss_out);
    return nsg_check_launch("cross_entropy");
}

size_t nsg_cross_entropy_masked_workspace_bytes(int64_t M, int64_t rows_per_clip)
{
    return (M > 0 && rows_per_clip > 0 && M % rows_per_clip == 0) ? ce_masked_layout(M, M / rows_per_clip).bytes : 0;
}

int nsg_cross_entropy_masked(const float *logits, const int64_t *target, int64_t M, int32_t K, int64_t rows_per_clip, float grad_scale,
                             float *loss_out, float *dlogits, float *clip_nll, int64_t *clip_count, void *workspace, size_t workspace_bytes,
                             void *stream)
{
    NSG_REQUIRE(logits && target && loss_out && M > 0 && K > 0, NSG_E_INVALID, "nsg_cross_entropy_masked: bad argument");
    NSG_REQUIRE(rows_per_clip > 0 && M % rows_per_clip == 0 && M / rows_per_clip < 0x7fffffff, NSG_E_INVALID,
                "nsg_cross_entropy_masked: M must be a whole number of clips of rows_per_clip rows");
    NSG_REQUIRE(workspace && nsg_aligned16(workspace) && workspace_bytes >= nsg_cross_entropy_masked_workspace_bytes(M, rows_per_clip), NSG_E_WORKSPACE,
                "nsg_cross_entropy_masked: workspace too small (or not 16-byte aligned)");
    hipStream_t s = (hipStream_t)stream;
    const int64_t B = M / rows_per_clip;
    const CeMaskedLayout L = ce_masked_layout(M, B);
    char *ws = reinterpret_cast<char *>(workspace);
    float *row_loss = reinterpret_cast<float *>(ws);
    double *partial = reinterpret_cast<double *>(ws + L.partial);
    int64_t *count = reinterpret_cast<int64_t *>(ws + L.count);
    CeScalars *sc = reinterpret_cast<CeScalars *>(ws + L.scalars);
    hipLaunchKernelGGL(ce_count_kernel, dim3((unsigned)B), dim3(256), 0, s, target, rows_per_clip, K, count);
    hipLaunchKernelGGL(ce_scale_kernel, dim3(1), dim3(256), 0, s, count, B, grad_scale, sc, clip_count);
    int64_t blocks = nsg_cdiv(M, 4);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(cross_entropy_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, logits, target, M, K, 0.f, &sc->gscale, row_loss, dlogits);
    const int nb = (int)(M < SUM_BLOCKS ? M : SUM_BLOCKS);            // the same two stages as nsg_cross_entropy
    hipLaunchKernelGGL(sum_partial_kernel, dim3(nb), dim3(256), 0, s, row_loss, M, partial);
    hipLaunchKernelGGL(ce_masked_final_kernel, dim3(1), dim3(64), 0, s, partial, nb, sc, loss_out);
    if (clip_nll) hipLaunchKernelGGL(ce_clip_nll_kernel, dim3((unsigned)B), dim3(256), 0, s, row_loss, rows_per_clip, clip_nll);
    return nsg_check_launch("cross_entropy_masked");
}

int nsg_gated_activation_sum_forward(const float *a, const float *b, const float *cond, float *y, int64_t M, int32_t C, int64_t rows_per_clip,
                                     void *stream)
{
    NSG_REQUIRE(a && b && y && M > 0 && C > 0 && C % 4 == 0, NSG_E_INVALID, "nsg_gated_activation_sum_forward: bad argument (C %% 4 == 0)");
    NSG_REQUIRE(!cond || rows_per_clip > 0, NSG_E_INVALID, "nsg_gated_activation_sum_forward: rows_per_clip must be positive with a conditioning row");
    NSG_REQUIRE(nsg_aligned16(a) && nsg_aligned16(b) && nsg_aligned16(y) && (!cond || nsg_aligned16(cond)), NSG_E_INVALID,
                "nsg_gated_activation_sum_forward: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(gated_fwd_kernel<true>, dim3(ew_blocks(M * (C / 4))), dim3(256), 0, (hipStream_t)stream, a, b, cond, y, M, C, cond ? rows_per_clip : 1);
    return nsg_check_launch("gated_fwd_kernel<sum>");
}

size_t nsg_gated_colsum_workspace_bytes(int64_t M, int32_t C, int64_t rows_per_clip)
{
    if (M <= 0 || C <= 0 || C % 4 != 0 || C > 1024 || rows_per_clip <= 0 || M % rows_per_clip != 0) return 0;
    const int64_t B = M / rows_per_clip;
    return (size_t)B * gate_slabs(B, rows_per_clip, C) * 2 * C * sizeof(double);
}

// the shared launcher of the two backward forms (b == NULL: the plain gate); dcond != NULL selects the column-sum kernel
static int gated_backward_impl(const char *fn, const float *a, const float *b, const float *cond, const float *dy, float *dx, float *dcond, int64_t M,
                               int32_t C, int64_t rows_per_clip, void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(a && dy && dx && M > 0 && C > 0 && C % 4 == 0, NSG_E_INVALID, "%s: bad argument (C %% 4 == 0)", fn);
    NSG_REQUIRE((!cond && !dcond) || rows_per_clip > 0, NSG_E_INVALID, "%s: rows_per_clip must be positive with a conditioning row", fn);
    NSG_REQUIRE(nsg_aligned16(a) && (!b || nsg_aligned16(b)) && nsg_aligned16(dy) && nsg_aligned16(dx) && (!cond || nsg_aligned16(cond)), NSG_E_INVALID,
                "%s: pointers must be 16-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    if (!dcond) {
        if (b) hipLaunchKernelGGL(gated_bwd_kernel<true>, dim3(ew_blocks(M * (C / 4))), dim3(256), 0, s, a, b, cond, dy, dx, M, C, cond ? rows_per_clip : 1);
        else hipLaunchKernelGGL(gated_bwd_kernel<false>, dim3(ew_blocks(M * (C / 4))), dim3(256), 0, s, a, b, cond, dy, dx, M, C, cond ? rows_per_clip : 1);
        return nsg_check_launch("gated_bwd_kernel");
    }
    NSG_REQUIRE(M % rows_per_clip == 0 && M / rows_per_clip <= 0x7fffffff / 64, NSG_E_INVALID, "%s: M must be a whole number of clips of rows_per_clip rows", fn);
    NSG_REQUIRE(C <= 1024, NSG_E_UNSUPPORTED, "%s: the column sums take C <= 1024", fn);
    NSG_REQUIRE(workspace && nsg_aligned16(workspace) && workspace_bytes >= nsg_gated_colsum_workspace_bytes(M, C, rows_per_clip), NSG_E_WORKSPACE,
                "%s: workspace too small (or not 16-byte aligned)", fn);
    const int64_t B = M / rows_per_clip;
    const int slabs = gate_slabs(B, rows_per_clip, C);
    double *partial = reinterpret_cast<double *>(workspace);
    if (b) hipLaunchKernelGGL(gated_bwd_colsum_kernel<true>, dim3((unsigned)(B * slabs)), dim3(256), 0, s, a, b, cond, dy, dx, rows_per_clip, C, slabs, partial);
    else hipLaunchKernelGGL(gated_bwd_colsum_kernel<false>, dim3((unsigned)(B * slabs)), dim3(256), 0, s, a, b, cond, dy, dx, rows_per_clip, C, slabs, partial);
    hipLaunchKernelGGL(gated_colsum_final_kernel, dim3((unsigned)nsg_cdiv(B * 2 * C, 256)), dim3(256), 0, s, partial, B, slabs, 2 * C, dcond);
    return nsg_check_launch("gated_bwd_colsum_kernel");
}

int nsg_gated_activation_sum_backward(const float *a, const float *b, const float *cond, const float *dy, float *dx, float *dcond, int64_t M, int32_t C,
                                      int64_t rows_per_clip, void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(b, NSG_E_INVALID, "nsg_gated_activation_sum_backward: bad argument (second summand)");
    return gated_backward_impl("nsg_gated_activation_sum_backward", a, b, cond, dy, dx, dcond, M, C, rows_per_clip, workspace, workspace_bytes, stream);
}

int nsg_gated_activation_backward_colsum(const float *x, const float *cond, const float *dy, float *dx, float *dcond, int64_t M, int32_t C,
                                         int64_t rows_per_clip, void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(dcond, NSG_E_INVALID, "nsg_gated_activation_backward_colsum: bad argument (dcond)");
    return gated_backward_impl("nsg_gated_activation_backward_colsum", x, nullptr, cond, dy, dx, dcond, M, C, rows_per_clip, workspace, workspace_bytes, stream);
}

}  // extern "C"
