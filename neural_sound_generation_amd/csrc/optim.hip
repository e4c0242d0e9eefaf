// The optimiser's extensions over one flat fp32 bucket: the gradient's sum of squares (double, fixed order) and the extended
// Adam step -- decoupled weight decay per segment, clipping by the global norm, a non-finite guard and a weight EMA folded
// into the one pass.  With every extension neutral the step's arithmetic is adam_kernel's (elementwise.hip), operation for
// operation; the library is built with -ffp-contract=off, so the bits are too.
#include "nsg_reduce.h"
#include <math.h>

namespace {

constexpr int SUMSQ_BLOCKS = 1024;

inline int opt_blocks(int64_t n, int cap)
{
    int64_t b = nsg_cdiv(n, 256);
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// partial[block] = sum of g^2 over the block's grid-stride share: a thread adds its elements in index order, the block's 256
// thread sums go through nsg_block_sum_four_walk.  (double)g * (double)g is exact.
template <int V>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float *__restrict__ g, int64_t nv, double *__restrict__ partial)
{
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        float x[V];
        if constexpr (V == 4) ldw<float, 4>(g + i * 4, x); else x[0] = g[i];
#pragma unroll
        for (int e = 0; e < V; ++e) acc += (double)x[e] * (double)x[e];
    }
    nsg_block_sum_four_walk(acc, partial);
}

__global__ __launch_bounds__(64) void grad_sumsq_final_kernel(const double *__restrict__ partial, int n, double *__restrict__ out)
{
    nsg_wave_close_sum(partial, n, [&](double s) { out[0] = s; });
}

struct AdamwScalars {
    float b1, b2, eps, step_size, bc2_sqrt, gscale, lr, max_norm, one_minus_decay;
    int n_seg, skip_nonfinite;
};

// Every thread forms the norm and the coefficient from the one double at sumsq with the same operations, so all blocks agree
// on them to the bit.  stats (16 bytes: float norm, float coef, int32 finite, int32 skipped steps) is written by thread 0 of
// block 0 alone and read by nobody in this launch.
template <int V>
__global__ __launch_bounds__(256) void adamw_kernel(float *p, const float *g, float *m, float *v, int64_t nv, const AdamwScalars a,
                                                    const int64_t *__restrict__ seg_end, const float *__restrict__ seg_wd,
                                                    const double *__restrict__ sumsq, float *shadow, float *stats)
{
    float norm = -1.0f, coef = 1.0f;
    bool finite = true;
    const bool clip = sumsq && a.max_norm > 0.f;
    if (sumsq) {
        norm = (float)((double)a.gscale * sqrt(sumsq[0]));           // formed in double, rounded once
        finite = __builtin_isfinite(norm);
        if (clip) coef = fminf(1.0f, a.max_norm / (norm + 1e-6f));  // torch.nn.utils.clip_grad_norm_
    }
    const bool scaled = clip && coef != 1.0f;                        // a coefficient of exactly 1 leaves the plain step's bits
    const bool skip = a.skip_nonfinite && !finite;
    if (stats && blockIdx.x == 0 && threadIdx.x == 0) {
        stats[0] = norm;
        stats[1] = coef;
        int *istats = reinterpret_cast<int *>(stats);
        istats[2] = finite ? 1 : 0;
        if (skip) istats[3] = istats[3] + 1;
    }
    if (skip) return;                                                // p, m, v and the shadow stay as they are
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        float gv[V], mv[V], vv[V], pv[V], sv[V];
        if constexpr (V == 4) {
            ldw<float, 4>(g + i * 4, gv); ldw<float, 4>(m + i * 4, mv); ldw<float, 4>(v + i * 4, vv); ldw<float, 4>(p + i * 4, pv);
            if (shadow) ldw<float, 4>(shadow + i * 4, sv);
        } else {
            gv[0] = g[i]; mv[0] = m[i]; vv[0] = v[i]; pv[0] = p[i];
            if (shadow) sv[0] = shadow[i];
        }
        float lrwd = 0.f;
        if (seg_end) {
            // the segment of the group's first element: the smallest s with seg_end[s] > e (segments end on multiples of 4)
            const int64_t e = i * V;
            int lo = 0, hi = a.n_seg;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (seg_end[mid] > e) hi = mid; else lo = mid + 1;
            }
            if (lo < a.n_seg) lrwd = a.lr * seg_wd[lo];
        }
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const float gx = gv[c] * a.gscale;
            float mx = mv[c], vx = vv[c], px = pv[c];
            if (scaled) {
                // the clipped gradient is the exact double product of two floats and is never rounded to fp32 on its own:
                // g c - m and (g c)^2 (1 - b2) round once each, so clipping adds no rounding to m' and v'
                const double gd = (double)gx * (double)coef;
                mx = mx + (float)(gd - (double)mx) * (1.0f - a.b1);
                vx = vx * a.b2 + (float)(gd * gd * (double)(1.0f - a.b2));
            } else {
                mx = mx + (gx - mx) * (1.0f - a.b1);      // from here to the update: adam_kernel's expressions in its order
                vx = vx * a.b2 + gx * gx * (1.0f - a.b2);
            }
            const float den = sqrtf(vx) / a.bc2_sqrt + a.eps;
            if (lrwd != 0.f) px = px - px * lrwd;        // torch.optim.AdamW: p (1 - lr wd), rounded once at the size of p
            px = px - (mx / den) * a.step_size;
            mv[c] = mx; vv[c] = vx; pv[c] = px;
            // decay 0 (one_minus_decay == 1) is a copy: s - (s - p) need not round back to p
            if (shadow) sv[c] = a.one_minus_decay == 1.0f ? px : sv[c] - a.one_minus_decay * (sv[c] - px);
        }
        if constexpr (V == 4) {
            stw<float, 4>(m + i * 4, mv); stw<float, 4>(v + i * 4, vv); stw<float, 4>(p + i * 4, pv);
            if (shadow) stw<float, 4>(shadow + i * 4, sv);
        } else {
            m[i] = mv[0]; v[i] = vv[0]; p[i] = pv[0];
            if (shadow) shadow[i] = sv[0];
        }
    }
}

}  // namespace

extern "C" {

size_t nsg_grad_sumsq_workspace_bytes(int64_t n)
{
    (void)n;
    return (size_t)SUMSQ_BLOCKS * sizeof(double);
}

int nsg_grad_sumsq(const float *g, int64_t n, double *sumsq, void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(sumsq && n >= 0 && (g || n == 0), NSG_E_INVALID, "nsg_grad_sumsq: bad argument");
    NSG_REQUIRE((reinterpret_cast<uintptr_t>(sumsq) & 7u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, NSG_E_INVALID,
                "nsg_grad_sumsq: sumsq and workspace must be 8-byte aligned");
    NSG_REQUIRE(workspace && workspace_bytes >= nsg_grad_sumsq_workspace_bytes(n), NSG_E_WORKSPACE, "nsg_grad_sumsq: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    double *partial = reinterpret_cast<double *>(workspace);
    int nb = 0;
    if (n > 0) {
        if ((n & 3) == 0 && nsg_aligned16(g)) {
            nb = opt_blocks(n / 4, SUMSQ_BLOCKS);
            hipLaunchKernelGGL((grad_sumsq_kernel<4>), dim3(nb), dim3(256), 0, s, g, n / 4, partial);
        } else {
            nb = opt_blocks(n, SUMSQ_BLOCKS);
            hipLaunchKernelGGL((grad_sumsq_kernel<1>), dim3(nb), dim3(256), 0, s, g, n, partial);
        }
    }
    hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(64), 0, s, partial, nb, sumsq);
    return nsg_check_launch("grad_sumsq");
}

int nsg_adamw_step(float *p, const float *g, float *m, float *v, int64_t n, float lr, float beta1, float beta2, float eps,
                   int32_t step, float grad_scale, const int64_t *seg_end, const float *seg_wd, int32_t n_seg, const double *sumsq,
                   float max_norm, int32_t skip_nonfinite, float *shadow, float one_minus_decay, void *stats, void *stream)
{
    NSG_REQUIRE(p && g && m && v && n >= 0, NSG_E_INVALID, "nsg_adamw_step: null pointer or negative size");
    NSG_REQUIRE(step >= 1, NSG_E_INVALID, "nsg_adamw_step: step=%d must be >= 1", step);
    NSG_REQUIRE((seg_end != nullptr) == (seg_wd != nullptr), NSG_E_INVALID, "nsg_adamw_step: seg_end and seg_wd come together");
    NSG_REQUIRE(seg_end ? n_seg >= 1 : n_seg == 0, NSG_E_INVALID, "nsg_adamw_step: n_seg=%d does not match the segment table", n_seg);
    NSG_REQUIRE(!(max_norm > 0.f) || sumsq, NSG_E_INVALID, "nsg_adamw_step: max_norm > 0 needs the sum of squares");
    NSG_REQUIRE(!skip_nonfinite || sumsq, NSG_E_INVALID, "nsg_adamw_step: the non-finite guard needs the sum of squares");
    NSG_REQUIRE(max_norm == max_norm, NSG_E_INVALID, "nsg_adamw_step: max_norm is NaN");
    NSG_REQUIRE(fabsf(one_minus_decay) <= 1.0f, NSG_E_INVALID, "nsg_adamw_step: one_minus_decay=%g outside [-1, 1]", (double)one_minus_decay);
    NSG_REQUIRE(!shadow || (n > 0 ? (shadow < p + n && p < shadow + n) == false : shadow != p), NSG_E_INVALID,
                "nsg_adamw_step: the shadow overlaps the parameters");
    NSG_REQUIRE((!sumsq || (reinterpret_cast<uintptr_t>(sumsq) & 7u) == 0) && (!stats || (reinterpret_cast<uintptr_t>(stats) & 3u) == 0),
                NSG_E_INVALID, "nsg_adamw_step: sumsq must be 8-byte and stats 4-byte aligned");
    if (n == 0) return NSG_OK;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const AdamwScalars a = {beta1, beta2, eps, (float)((double)lr / bc1), (float)sqrt(bc2), grad_scale, lr, max_norm, one_minus_decay,
                            (int)n_seg, skip_nonfinite ? 1 : 0};
    hipStream_t s = (hipStream_t)stream;
    float *st = reinterpret_cast<float *>(stats);
    if ((n & 3) == 0 && nsg_aligned16(p) && nsg_aligned16(g) && nsg_aligned16(m) && nsg_aligned16(v) && (!shadow || nsg_aligned16(shadow)))
        hipLaunchKernelGGL((adamw_kernel<4>), dim3(opt_blocks(n / 4, 4096)), dim3(256), 0, s, p, g, m, v, n / 4, a, seg_end, seg_wd, sumsq, shadow, st);
    else
        hipLaunchKernelGGL((adamw_kernel<1>), dim3(opt_blocks(n, 4096)), dim3(256), 0, s, p, g, m, v, n, a, seg_end, seg_wd, sumsq, shadow, st);
    return nsg_check_launch("adamw_kernel");
}

}  // extern "C"
