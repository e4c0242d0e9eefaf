// The Gaussian bottleneck of the continuous VAE (src/models.py:77,103-112): encoder.10 BatchNorm2d(2Z) -> chunk(2, dim=1) ->
// KL to N(0, I) -> z = mu + exp(.5 logvar) * eps, and its backward.  Rows are NHWC pixels, [M][2Z]: channels [0, Z) are mu,
// [Z, 2Z) logvar.  Both kernels read h, the BatchNorm's INPUT, and form y = (h - mean) * (invstd * gamma) + beta on load with
// bn_apply_kernel's expression (bn.hip; the library is built with -ffp-contract=off), so the BatchNorm's output is never stored.
//
// Traffic per row (fp32): forward reads 2Z (h) + Z (eps) and writes Z (z); backward reads 2Z (h) + Z (eps) + Z (dz) and writes
// 2Z (dy).  The separate operators (bn_apply, chunk, exp, kl, sample; their autograd and bn_backward_sums) move 2Z more each way
// for y and read dy back for the sums.
//
// Reductions (nsg_reduce.h; DESIGN.md "Reduction shapes"): both kernels run one block per slab of nsg_bn_slab_geom(M), the slabs of
// nsg_bn_backward_sums.  The KL sum: a double per thread -> four-then-walk per block -> the one-wave closer.  The BatchNorm sums:
// slab column fold (park / fold) per block -> bn.hip's finaliser, so dgamma / dbeta carry nsg_bn_backward_sums's bits.
#include "nsg_reduce.h"

namespace {

constexpr int W = 4;            // channels per thread = one 16-byte access
constexpr int MAX_Z = 512;      // 2Z / W threads own one row's channel groups: 2Z <= 1024, bn.hip's limit

// z and the block's share of the KL sum.  Thread (cg, rg) of NsgSlabMap<W>(Z): mu channels W cg .., logvar channels Z + W cg ..
__global__ __launch_bounds__(256) void vae_latent_fwd_kernel(const float *__restrict__ h, const float *__restrict__ mean,
                                                             const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, const float *__restrict__ eps,
                                                             float *__restrict__ z, int64_t M, int Z, int slab_rows,
                                                             double *__restrict__ partial)
{
    const NsgSlabMap<W> m(Z, blockIdx.x, slab_rows, M);
    double acc = 0.0;
    if (m.active) {
        const int c = m.cg * W;
        float mu_m[W], sc_m[W], be_m[W], mu_l[W], sc_l[W], be_l[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            mu_m[e] = mean[c + e]; sc_m[e] = invstd[c + e] * gamma[c + e]; be_m[e] = beta[c + e];
            mu_l[e] = mean[Z + c + e]; sc_l[e] = invstd[Z + c + e] * gamma[Z + c + e]; be_l[e] = beta[Z + c + e];
        }
        for (int64_t r = m.r0 + m.rg; r < m.r1; r += m.rgroups) {
            float hm[W], hl[W], ev[W], o[W];
            ldw<float, W>(h + (size_t)r * 2 * Z + c, hm);
            ldw<float, W>(h + (size_t)r * 2 * Z + Z + c, hl);
            ldw<float, W>(eps + (size_t)r * Z + c, ev);
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const float mu = (hm[e] - mu_m[e]) * sc_m[e] + be_m[e];
                const float lv = (hl[e] - mu_l[e]) * sc_l[e] + be_l[e];
                const float sigma = expf(0.5f * lv);
                o[e] = mu + sigma * ev[e];
                acc += 0.5 * ((((double)(mu * mu) + (double)(sigma * sigma)) - 1.0) - (double)lv);
            }
            stw<float, W>(z + (size_t)r * Z + c, o);
        }
    }
    nsg_block_sum_four_walk(acc, partial);
}

// dy and the slab's BatchNorm-backward sums over it.  Thread (cg, rg) of NsgSlabMap<W>(2Z), bn_bwd_partial_kernel's map: the
// channel groups below Z are mu's, the others logvar's (Z % W == 0: no group holds both).
__global__ __launch_bounds__(256) void vae_latent_bwd_kernel(const float *__restrict__ h, const float *__restrict__ mean,
                                                             const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, const float *__restrict__ eps,
                                                             const float *__restrict__ dz, float kl_scale, const float *__restrict__ kl_grad,
                                                             float *__restrict__ dy, int64_t M, int Z, int slab_rows,
                                                             float *__restrict__ partial)
{
    __shared__ float red[2 * 256 * W];
    const int C = 2 * Z;
    const NsgSlabMap<W> m(C, blockIdx.x, slab_rows, M);
    const int tid = threadIdx.x;
    if (m.active) {
        const int c = m.cg * W;
        const bool is_lv = c >= Z;
        const int zc = is_lv ? c - Z : c;
        const float ks = (kl_scale * (kl_grad ? kl_grad[0] : 1.f)) / (float)M;
        float s[2][W], mu[W], is[W], sc[W], be[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            s[0][e] = 0.f; s[1][e] = 0.f;
            mu[e] = mean[c + e]; is[e] = invstd[c + e]; sc[e] = is[e] * gamma[c + e]; be[e] = beta[c + e];
        }
        for (int64_t r = m.r0 + m.rg; r < m.r1; r += m.rgroups) {
            const size_t o = (size_t)r * C + c, oz = (size_t)r * Z + zc;
            float hv[W], g[W], d[W];
            ldw<float, W>(h + o, hv);
            ldw<float, W>(dz + oz, g);
            if (is_lv) {
                float ev[W];
                ldw<float, W>(eps + oz, ev);
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const float lv = (hv[e] - mu[e]) * sc[e] + be[e];
                    const float sigma = expf(0.5f * lv);
                    d[e] = 0.5f * g[e] * sigma * ev[e] + 0.5f * ks * (sigma * sigma - 1.f);
                }
            } else {
#pragma unroll
                for (int e = 0; e < W; ++e) d[e] = g[e] + ks * ((hv[e] - mu[e]) * sc[e] + be[e]);
            }
            stw<float, W>(dy + o, d);
#pragma unroll
            for (int e = 0; e < W; ++e) { s[0][e] += d[e]; s[1][e] += d[e] * ((hv[e] - mu[e]) * is[e]); }     // bn_bwd_partial_kernel's terms
        }
        nsg_slab_park(m, s, red);
    }
    float *dst = partial + (size_t)blockIdx.x * 2 * C;
    nsg_slab_fold<2>(m, red, [&](int e, const float (&t)[2]) {
        dst[tid * W + e] = t[0];
        dst[C + tid * W + e] = t[1];
    });
}

// nsg_vae_latent_*'s workspace: the KL sum's block partials | the BatchNorm-backward sums [slabs][2][2Z]
struct LatentLayout { double *kl_partial; float *bn_partial; int nslab, rows; size_t bytes; };
LatentLayout latent_layout(void *ws, int64_t M, int Z)
{
    int nslab, rows;
    nsg_bn_slab_geom(M, &nslab, &rows);
    NsgCarver c(ws);
    return {c.take<double>(nsg_align_up((size_t)nslab * sizeof(double), 256)), c.take<float>((size_t)nslab * 2 * 2 * Z * sizeof(float)), nslab, rows, c.off};
}

int check_mz(const char *fn, int64_t M, int Z)
{
    NSG_REQUIRE(M >= 1, NSG_E_INVALID, "%s: M must be positive", fn);
    NSG_REQUIRE(Z >= 4 && Z % 4 == 0 && Z <= MAX_Z, NSG_E_UNSUPPORTED, "%s: Z=%d must be a multiple of 4 in 4 ... %d", fn, Z, MAX_Z);
    NSG_REQUIRE(M * 2 * (int64_t)Z < (1ll << 31), NSG_E_UNSUPPORTED, "%s: tensor too large", fn);
    return NSG_OK;
}

}  // namespace

extern "C" {

size_t nsg_vae_latent_workspace_bytes(int64_t M, int32_t Z)
{
    if (M < 1 || Z < 4 || Z % 4 != 0 || Z > MAX_Z || M * 2 * (int64_t)Z >= (1ll << 31)) return 0;
    return latent_layout(nullptr, M, Z).bytes;
}

int nsg_vae_latent_forward(const float *h, const float *mean, const float *invstd, const float *gamma, const float *beta, const float *eps,
                           float *z, float *kl_out, int64_t M, int32_t Z, void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(h && mean && invstd && gamma && beta && eps && z && kl_out, NSG_E_INVALID, "nsg_vae_latent_forward: null pointer");
    if (int rc = check_mz("nsg_vae_latent_forward", M, Z)) return rc;
    NSG_REQUIRE(nsg_aligned16(h) && nsg_aligned16(eps) && nsg_aligned16(z), NSG_E_INVALID, "nsg_vae_latent_forward: pointers must be 16-byte aligned");
    const LatentLayout L = latent_layout(workspace, M, Z);
    NSG_REQUIRE(workspace && workspace_bytes >= L.bytes, NSG_E_WORKSPACE, "nsg_vae_latent_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(vae_latent_fwd_kernel, dim3(L.nslab), dim3(256), 0, s, h, mean, invstd, gamma, beta, eps, z, M, Z, L.rows, L.kl_partial);
    int rc = nsg_check_launch("vae_latent_fwd_kernel");
    if (rc) return rc;
    return nsg_launch_final_mean(L.kl_partial, L.nslab, (double)M, kl_out, s);
}

int nsg_vae_latent_backward(const float *h, const float *mean, const float *invstd, const float *gamma, const float *beta, const float *eps,
                            const float *dz, float kl_scale, const float *kl_grad, float *dy, float *dgamma, float *dbeta, int64_t M, int32_t Z,
                            void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(h && mean && invstd && gamma && beta && eps && dz && dy && dgamma && dbeta, NSG_E_INVALID, "nsg_vae_latent_backward: null pointer");
    if (int rc = check_mz("nsg_vae_latent_backward", M, Z)) return rc;
    NSG_REQUIRE(nsg_aligned16(h) && nsg_aligned16(eps) && nsg_aligned16(dz) && nsg_aligned16(dy), NSG_E_INVALID,
                "nsg_vae_latent_backward: pointers must be 16-byte aligned");
    const LatentLayout L = latent_layout(workspace, M, Z);
    NSG_REQUIRE(workspace && workspace_bytes >= L.bytes, NSG_E_WORKSPACE, "nsg_vae_latent_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(vae_latent_bwd_kernel, dim3(L.nslab), dim3(256), 0, s, h, mean, invstd, gamma, beta, eps, dz, kl_scale, kl_grad, dy, M, Z,
                       L.rows, L.bn_partial);
    int rc = nsg_check_launch("vae_latent_bwd_kernel");
    if (rc) return rc;
    return nsg_launch_bn_bwd_final(L.bn_partial, L.nslab, 2 * Z, dgamma, dbeta, s);
}

}  // extern "C"
