// BatchNorm2d over NHWC activations viewed as [M][C] (M = B*H*W).  Reference call sites:
// src/models.py:151,154,166,180 (nn.BatchNorm2d, training and eval).  HBM-bound kernels:
// 16-byte accesses, each row of C channels is contiguous so a wave reads whole 128-B lines.
// Activations may be stored fp32 or bf16 (templates below); all arithmetic, statistics and
// per-channel parameters are fp32.
//
// Statistics are formed per slab of rows as (count, mean, M2 about the slab mean) in one pass about a
// pivot row, and pooled in double in slab order: no E[x^2]-E[x]^2 cancellation and bitwise
// reproducible (no atomics).
// The backward of a BatchNorm that was followed by a fused ReLU re-derives the ReLU mask from x itself
// ((x-mean)*(invstd*gamma)+beta > 0, the forward's own expression) instead of reading the stored output.
#include "nsg_reduce.h"

namespace {

constexpr int MAX_SLABS = NSG_MAX_SLABS;

struct SlabGeom {
    int nslab;
    int rows;
};
inline SlabGeom slab_geom(int64_t M)
{
    SlabGeom g;
    int64_t n = nsg_cdiv(M, 64);   // >= 64 rows per slab (256 left 320 blocks for the 82 K rows of BASELINE configs[3]: 1.25 per CU)
    if (n > MAX_SLABS) n = MAX_SLABS;
    if (n < 1) n = 1;
    g.rows = (int)nsg_cdiv(M, n);
    g.nslab = (int)nsg_cdiv(M, g.rows);
    return g;
}

// One block per slab, threads by NsgSlabMap.  partial[slab] = { mean[C], M2[C] } (count is implied by the slab geometry).
// ONE pass: sums of d = v - pivot and d^2 with pivot = the slab's first row (a sample of the column, so
// |mean - pivot| is of the order of the column's spread and M2 = S2 - S1^2/n loses no more than a few bits).
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const T *__restrict__ x, int64_t M, int C, int slab_rows,
                                                               float *__restrict__ partial)
{
    constexpr int W = Elem<T>::N;
    __shared__ float red[2 * 256 * W];
    const NsgSlabMap<W> m(C, blockIdx.x, slab_rows, M);
    const int tid = threadIdx.x;
    const int n = (int)(m.r1 - m.r0);

    float pv[W];               // set by the active threads; read by the fold's closing threads (tid < CW, so rg == 0: active)
    if (m.active) {
        float s[2][W];
        ldw<T, W>(x + m.r0 * C + m.cg * W, pv);
#pragma unroll
        for (int e = 0; e < W; ++e) { s[0][e] = 0.f; s[1][e] = 0.f; }
#pragma unroll 4
        for (int64_t r = m.r0 + m.rg; r < m.r1; r += m.rgroups) {
            float v[W];
            ldw<T, W>(x + r * C + m.cg * W, v);
#pragma unroll
            for (int e = 0; e < W; ++e) { const float d = v[e] - pv[e]; s[0][e] += d; s[1][e] += d * d; }
        }
        nsg_slab_park(m, s, red);
    }
    float *dst = partial + (size_t)blockIdx.x * 2 * C;
    const float inv_n = 1.f / (float)n;
    nsg_slab_fold<2>(m, red, [&](int e, const float (&t)[2]) {
        dst[tid * W + e] = pv[e] + t[0] * inv_n;
        dst[C + tid * W + e] = fmaxf(t[1] - t[0] * t[0] * inv_n, 0.f);
    });
}

// Finalisers with one block per 4 channels: thread tid holds the records of slabs tid, tid + 256, ... (PER of them) of an
// array [nslab][stride] at column c0.  The slab index is clamped to the last slab, so every load is unconditional, and all of a
// kernel's slab_records_load calls come before its first add: one memory latency.
constexpr int PER = MAX_SLABS / 256;
__device__ __forceinline__ void slab_records_load(const float *__restrict__ p, size_t stride, int c0, int nslab, int tid, v4f (&a)[PER])
{
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int s = tid + 256 * i;
        a[i] = *reinterpret_cast<const v4f *>(p + (size_t)(s < nslab ? s : nslab - 1) * stride + c0);
    }
}
// sum over all slabs of element e of such records: the thread's live records in index order, then the butterfly block sum
__device__ __forceinline__ double slab_records_sum(const v4f (&a)[PER], int e, int nslab, double *red, int tid)
{
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < PER; ++i) t += (tid + 256 * i < nslab) ? (double)a[i][e] : 0.0;
    return nsg_block_sum_butterfly(t, red, tid);
}

// mean, invstd and the running statistics (as nn.BatchNorm2d: biased variance for invstd, unbiased into running_var) of channel
// c from its mean mu and M2 over M rows; rm0 / rv0 = the running values read before
__device__ __forceinline__ void bn_stats_store(int c, double mu, double m2, int64_t M, float eps, float momentum, float rm0, float rv0,
                                               float *mean, float *invstd, float *running_mean, float *running_var)
{
    const double var_b = m2 / (double)M;
    mean[c] = (float)mu;
    invstd[c] = (float)(1.0 / sqrt(var_b + (double)eps));
    if (running_mean) running_mean[c] = (1.f - momentum) * rm0 + momentum * (float)mu;
    if (running_var) {
        const double var_u = M > 1 ? m2 / (double)(M - 1) : var_b;
        running_var[c] = (1.f - momentum) * rv0 + momentum * (float)var_u;
    }
}

// One block per 4 channels, then two butterfly block sums per channel in double:
//   n = sum n_s,  mean = sum n_s m_s / n,  M2 = sum ( q_s + n_s (m_s - mean)^2 )       (the pooled-variance identity)
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float *__restrict__ partial, int nslab, int slab_rows, int64_t M,
                                                             int C, float eps, float momentum, float *mean, float *invstd,
                                                             float *running_mean, float *running_var)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * 4;
    v4f ms[PER], qs[PER];
    float ns[PER];
    float rm0[4], rv0[4];        // the running statistics travel with the partials (read by every thread: no lane condition on a load)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int cc = c0 + e < C ? c0 + e : C - 1;
        rm0[e] = running_mean ? running_mean[cc] : 0.f;
        rv0[e] = running_var ? running_var[cc] : 0.f;
    }
    slab_records_load(partial, (size_t)2 * C, c0, nslab, tid, ms);
    slab_records_load(partial, (size_t)2 * C, C + c0, nslab, tid, qs);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int64_t r0 = (int64_t)(tid + 256 * i) * slab_rows;
        ns[i] = tid + 256 * i < nslab ? (float)(min(M, r0 + slab_rows) - r0) : 0.f;
    }
    double mu[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < PER; ++i) t += (double)ns[i] * (double)ms[i][e];
        mu[e] = nsg_block_sum_butterfly(t, red, tid) / (double)M;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const double dl = (double)ms[i][e] - mu[e];
            t += ns[i] > 0.f ? (double)qs[i][e] + (double)ns[i] * dl * dl : 0.0;
        }
        const double m2 = nsg_block_sum_butterfly(t, red, tid);
        if (tid == 0 && c0 + e < C) bn_stats_store(c0 + e, mu[e], m2, M, eps, momentum, rm0[e], rv0[e], mean, invstd, running_mean, running_var);
    }
}

// tiles: [ntiles][3][C] = (count n_t, sum S_t, M2_t about the tile mean), written by a producer's epilogue / statistics pass.
// With N = sum n_t, S = sum S_t:  mean = S/N,  M2 = sum_t ( M2_t + S_t^2/n_t ) - S^2/N  (double).
// Two stages, both with a thread per channel (coalesced rows of the tile records): TILE_CHUNKS blocks each fold a
// contiguous run of tiles in tile order into (N, S, Q) per channel, then one block folds the chunks in chunk order.
constexpr int TILE_CHUNKS = 64;
__global__ __launch_bounds__(256) void bn_stats_tiles_fold_kernel(const float *__restrict__ tiles, int ntiles, int C, double *__restrict__ chunks)
{
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    const int cx = tid & 63, ty = tid >> 6;
    const int per = (ntiles + TILE_CHUNKS - 1) / TILE_CHUNKS;
    const int t0 = blockIdx.x * per, t1 = min(ntiles, t0 + per);
    for (int cb = 0; cb < C; cb += 64) {
        const int c = cb + cx;
        double N = 0.0, S = 0.0, Q = 0.0;
        if (c < C)
            for (int t = t0 + ty; t < t1; t += 4) {
                const float *rec = tiles + (size_t)t * 3 * C + c;
                const double n = rec[0];
                if (n == 0.0) continue;
                const double st = rec[C], qt = rec[2 * C];
                N += n;
                S += st;
                Q += qt + st * st / n;
            }
        red[0][tid] = N; red[1][tid] = S; red[2][tid] = Q;
        __syncthreads();
        if (ty == 0 && c < C) {
            double *dst = chunks + (size_t)blockIdx.x * 3 * C;
            dst[c] = ((red[0][cx] + red[0][64 + cx]) + red[0][128 + cx]) + red[0][192 + cx];
            dst[C + c] = ((red[1][cx] + red[1][64 + cx]) + red[1][128 + cx]) + red[1][192 + cx];
            dst[2 * C + c] = ((red[2][cx] + red[2][64 + cx]) + red[2][128 + cx]) + red[2][192 + cx];
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void bn_stats_tiles_final_kernel(const double *__restrict__ chunks, int64_t M, int C, float eps, float momentum,
                                                                   float *mean, float *invstd, float *running_mean, float *running_var)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float rm0 = running_mean ? running_mean[c] : 0.f, rv0 = running_var ? running_var[c] : 0.f;     // (in flight with the chunks)
    double N = 0.0, S = 0.0, Q = 0.0;
    for (int k0 = 0; k0 < TILE_CHUNKS; k0 += 16) {        // 48 loads in flight, added in chunk order
        double n[16], sv[16], q[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            n[k] = chunks[(size_t)(k0 + k) * 3 * C + c];
            sv[k] = chunks[(size_t)(k0 + k) * 3 * C + C + c];
            q[k] = chunks[(size_t)(k0 + k) * 3 * C + 2 * C + c];
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) { N += n[k]; S += sv[k]; Q += q[k]; }
    }
    const double mu = S / N;
    double m2 = Q - S * S / N;
    if (m2 < 0.0) m2 = 0.0;
    bn_stats_store(c, mu, m2, M, eps, momentum, rm0, rv0, mean, invstd, running_mean, running_var);
}

__global__ void bn_eval_stats_kernel(const float *rm, const float *rv, int C, float eps, float *mean, float *invstd)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        mean[c] = rm[c];
        invstd[c] = 1.0f / sqrtf(rv[c] + eps);
    }
}

// y = (x-mean)*invstd*gamma + beta  [relu]  [+ (relu) residual];   x/residual of type TX, y of type TY.
// The grid stride is a multiple of the row length (launcher), so a thread keeps its W channels: their parameters are
// loaded once, not per element (the kernel was instruction-bound on those loads: 3.7 TB/s on tensors beyond the MALL).
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void bn_apply_kernel(const TX *__restrict__ x, const float *__restrict__ mean,
                                                       const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, const TX *__restrict__ residual,
                                                       TY *__restrict__ y, int64_t nw, int CW, int relu, int relu_res)
{
    // relu bit 0: ReLU right after the affine map; bit 1: ReLU of the final value (after the residual add)
    const int relu_bn = relu & 1, relu_out = relu & 2;
    constexpr int W = Width<TX, TY>::W;
    const int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int c = (int)(i0 % CW) * W;
    float mu[W], sc[W], be[W];
#pragma unroll
    for (int e = 0; e < W; ++e) { mu[e] = mean[c + e]; sc[e] = invstd[c + e] * gamma[c + e]; be[e] = beta[c + e]; }
    for (int64_t i = i0; i < nw; i += (int64_t)gridDim.x * blockDim.x) {
        float xv[W], o[W];
        ldw<TX, W>(x + i * W, xv);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            float t = (xv[e] - mu[e]) * sc[e] + be[e];
            if (relu_bn) t = fmaxf(t, 0.f);
            o[e] = t;
        }
        if (residual) {
            float rv[W];
            ldw<TX, W>(residual + i * W, rv);
#pragma unroll
            for (int e = 0; e < W; ++e) o[e] += relu_res ? fmaxf(rv[e], 0.f) : rv[e];
        }
        if (relu_out)
#pragma unroll
            for (int e = 0; e < W; ++e) o[e] = fmaxf(o[e], 0.f);
        stw<TY, W>(y + i * W, o);
    }
}

// per-slab partial sums of dyh and dyh*xhat (dyh = dy masked by the fused ReLU)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const T *__restrict__ x, const T *__restrict__ yrelu,
                                                             const T *__restrict__ dy, const float *__restrict__ mean,
                                                             const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                             const float *__restrict__ relu_beta, int64_t M, int C,
                                                             int slab_rows, float *__restrict__ partial)
{
    constexpr int W = Elem<T>::N;
    __shared__ float red[2 * 256 * W];
    const NsgSlabMap<W> m(C, blockIdx.x, slab_rows, M);
    const int tid = threadIdx.x;
    const int cg = m.cg;
    if (m.active) {
        float s[2][W], mu[W], is[W], sc[W], be[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            s[0][e] = 0.f; s[1][e] = 0.f; mu[e] = mean[cg * W + e]; is[e] = invstd[cg * W + e];
            sc[e] = relu_beta ? is[e] * gamma[cg * W + e] : 0.f;
            be[e] = relu_beta ? relu_beta[cg * W + e] : 0.f;
        }
        for (int64_t r = m.r0 + m.rg; r < m.r1; r += m.rgroups) {
            const size_t o = (size_t)r * C + cg * W;
            float g[W], xv[W];
            ldw<T, W>(dy + o, g);
            ldw<T, W>(x + o, xv);
            if (relu_beta) {          // the forward's own expression (bn_apply_kernel): same rounding, same decision
#pragma unroll
                for (int e = 0; e < W; ++e) g[e] = ((xv[e] - mu[e]) * sc[e] + be[e]) > 0.f ? g[e] : 0.f;
            } else if (yrelu) {
                float yv[W];
                ldw<T, W>(yrelu + o, yv);
#pragma unroll
                for (int e = 0; e < W; ++e) g[e] = yv[e] > 0.f ? g[e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < W; ++e) { s[0][e] += g[e]; s[1][e] += g[e] * ((xv[e] - mu[e]) * is[e]); }
        }
        nsg_slab_park(m, s, red);
    }
    float *dst = partial + (size_t)blockIdx.x * 2 * C;
    nsg_slab_fold<2>(m, red, [&](int e, const float (&t)[2]) {
        dst[tid * W + e] = t[0];
        dst[C + tid * W + e] = t[1];
    });
}

// dbeta[c] = sum_s partial[s][c], dgamma[c] = sum_s partial[s][C + c]: one block per 4 channels, slab_records_sum in double
// colsum_partial != null: out3[c] = sum_s colsum_partial[s][c] in the same launch (slab_sum_final_kernel's job: a producer that
// leaves both kinds of partials, the fused 1x1 backward, pays one finaliser launch instead of two)
__device__ __forceinline__ void bn_bwd_final_body(int bid, const float *__restrict__ partial, int nslab, int C, float *dgamma, float *dbeta,
                                                  const float *__restrict__ colsum_partial, float *out3)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int c0 = bid * 4;
    v4f a[PER], b[PER], c3[PER];
    slab_records_load(partial, (size_t)2 * C, c0, nslab, tid, a);
    slab_records_load(partial, (size_t)2 * C, C + c0, nslab, tid, b);
    if (colsum_partial) slab_records_load(colsum_partial, (size_t)C, c0, nslab, tid, c3);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double s1 = slab_records_sum(a, e, nslab, red, tid);
        const double s2 = slab_records_sum(b, e, nslab, red, tid);
        const double s3 = colsum_partial ? slab_records_sum(c3, e, nslab, red, tid) : 0.0;
        if (tid == 0 && c0 + e < C) {
            dbeta[c0 + e] = (float)s1;
            dgamma[c0 + e] = (float)s2;
            if (colsum_partial) out3[c0 + e] = (float)s3;
        }
    }
}

__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const float *__restrict__ partial, int nslab, int C, float *dgamma, float *dbeta,
                                                           const float *__restrict__ colsum_partial, float *out3)
{
    bn_bwd_final_body(blockIdx.x, partial, nslab, C, dgamma, dbeta, colsum_partial, out3);
}

// bn_bwd_final_kernel in blocks 0 .. C / 4 - 1 and, in the blocks behind them, wdst[e] = nsg_split_slab_sum over the slabs of
// wpartial[slab][e], e < wn (what wgrad_reduce_kernel does for one tap): the two finalisers of the fused 1x1 backward (BatchNorm
// sums in front, the weight gradient's block partials) in ONE launch (a dependent launch costs 4.7 us here whatever it does).
__global__ __launch_bounds__(256) void bn_bwd_final_wreduce_kernel(const float *__restrict__ partial, int nslab, int C, float *dgamma, float *dbeta,
                                                                   const float *__restrict__ colsum_partial, float *out3,
                                                                   const float *__restrict__ wpartial, float *__restrict__ wdst, int wn, int wsplit)
{
    const int nbn = C / 4;
    if ((int)blockIdx.x < nbn) {
        bn_bwd_final_body(blockIdx.x, partial, nslab, C, dgamma, dbeta, colsum_partial, out3);
        return;
    }
    const int per_block = 256 / wsplit;
    const int tid = threadIdx.x;
    const int sub = tid / per_block, loc = tid - sub * per_block;
    const int e = ((int)blockIdx.x - nbn) * per_block + loc;
    const float sacc = nsg_split_slab_sum<false>(wpartial + e, (size_t)wn, nslab, wsplit, e < wn);
    if (sub == 0 && e < wn) wdst[e] = sacc;
}

// dx = gamma*invstd*(dyh - mean(dyh) - xhat*mean(dyh*xhat)), slab-structured; optionally also the per-slab
// column sums of dx (= bias gradient of the convolution in front of this BatchNorm) into `partial`
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T *__restrict__ x, const T *__restrict__ yrelu,
                                                           const T *__restrict__ dy, const float *__restrict__ mean,
                                                           const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                           const float *__restrict__ dgamma, const float *__restrict__ dbeta,
                                                           const float *__restrict__ relu_beta, T *__restrict__ dx, int64_t M, int C,
                                                           int slab_rows, float inv_m, float *__restrict__ partial)
{
    constexpr int W = Elem<T>::N;
    __shared__ float red[256 * W];
    const NsgSlabMap<W> m(C, blockIdx.x, slab_rows, M);
    const int tid = threadIdx.x;
    const int cg = m.cg;
    float s[1][W];
#pragma unroll
    for (int e = 0; e < W; ++e) s[0][e] = 0.f;
    if (m.active) {
        float mu[W], is[W], sc[W], dg[W], db[W], fs[W], be[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const int c = cg * W + e;
            mu[e] = mean[c]; is[e] = invstd[c]; sc[e] = gamma[c] * is[e]; dg[e] = dgamma[c] * inv_m; db[e] = dbeta[c] * inv_m;
            fs[e] = is[e] * gamma[c];                  // the forward's scale, in the forward's operand order
            be[e] = relu_beta ? relu_beta[c] : 0.f;
        }
        for (int64_t r = m.r0 + m.rg; r < m.r1; r += m.rgroups) {
            const size_t o = (size_t)r * C + cg * W;
            float g[W], xv[W], d[W];
            ldw<T, W>(dy + o, g);
            ldw<T, W>(x + o, xv);
            if (relu_beta) {
#pragma unroll
                for (int e = 0; e < W; ++e) g[e] = ((xv[e] - mu[e]) * fs[e] + be[e]) > 0.f ? g[e] : 0.f;
            } else if (yrelu) {
                float yv[W];
                ldw<T, W>(yrelu + o, yv);
#pragma unroll
                for (int e = 0; e < W; ++e) g[e] = yv[e] > 0.f ? g[e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < W; ++e) {
                d[e] = sc[e] * (g[e] - db[e] - ((xv[e] - mu[e]) * is[e]) * dg[e]);
                s[0][e] += d[e];
            }
            stw<T, W>(dx + o, d);
        }
    }
    if (partial == nullptr) return;        // (uniform: a kernel argument)
    if (m.active) nsg_slab_park(m, s, red);
    nsg_slab_fold<1>(m, red, [&](int e, const float (&t)[1]) { partial[(size_t)blockIdx.x * C + tid * W + e] = t[0]; });
}

// out[c] = sum_s partial[s][c]: one block per 4 channels
__global__ __launch_bounds__(256) void slab_sum_final_kernel(const float *__restrict__ partial, int nslab, int C, float *out)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * 4;
    v4f a[PER];
    slab_records_load(partial, (size_t)C, c0, nslab, tid, a);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double sm = slab_records_sum(a, e, nslab, red, tid);
        if (tid == 0 && c0 + e < C) out[c0 + e] = (float)sm;
    }
}


inline int check_mc(const char *fn, int64_t M, int C, int dtype)
{
    if (M <= 0 || C <= 0) return nsg_fail(NSG_E_INVALID, "%s: bad size", fn);
    if (dtype != NSG_F32 && dtype != NSG_BF16) return nsg_fail(NSG_E_INVALID, "%s: unknown dtype %d", fn, dtype);
    const int w = dtype == NSG_BF16 ? 8 : 4;
    if (C % w != 0 || C > 1024) return nsg_fail(NSG_E_UNSUPPORTED, "%s: C=%d must be a multiple of %d and <= 1024", fn, C, w);
    if (M * (int64_t)C >= (1ll << 31)) return nsg_fail(NSG_E_UNSUPPORTED, "%s: tensor too large", fn);
    return NSG_OK;
}

}  // namespace

// The same in ONE launch for up to MAX_SLABS records (the flat 1x1 GEMM writes 256-512): one block per 4 channels, three butterfly
// block sums in double: N, S, T = sum (Q_t + S_t^2 / n_t).
__global__ __launch_bounds__(256) void bn_stats_tiles_onepass_kernel(const float *__restrict__ tiles, int ntiles, int64_t M, int C, float eps,
                                                                     float momentum, float *mean, float *invstd, float *running_mean,
                                                                     float *running_var)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * 4;
    v4f nv[PER], sv[PER], qv[PER];
    float rm0[4], rv0[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        rm0[e] = running_mean ? running_mean[c0 + e] : 0.f;
        rv0[e] = running_var ? running_var[c0 + e] : 0.f;
    }
    slab_records_load(tiles, (size_t)3 * C, c0, ntiles, tid, nv);
    slab_records_load(tiles, (size_t)3 * C, C + c0, ntiles, tid, sv);
    slab_records_load(tiles, (size_t)3 * C, 2 * C + c0, ntiles, tid, qv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        double n = 0.0, sm = 0.0, tq = 0.0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const bool live = tid + 256 * i < ntiles;
            const double ni = live ? (double)nv[i][e] : 0.0, si = live ? (double)sv[i][e] : 0.0, qi = live ? (double)qv[i][e] : 0.0;
            n += ni;
            sm += si;
            tq += ni > 0.0 ? qi + si * si / ni : 0.0;
        }
        const double N = nsg_block_sum_butterfly(n, red, tid), S = nsg_block_sum_butterfly(sm, red, tid), T = nsg_block_sum_butterfly(tq, red, tid);
        if (tid == 0) {
            double m2 = T - S * S / N;
            if (m2 < 0.0) m2 = 0.0;
            bn_stats_store(c0 + e, S / N, m2, M, eps, momentum, rm0[e], rv0[e], mean, invstd, running_mean, running_var);
        }
    }
}

// A tile-statistics buffer: the records [ntiles][3][C] | the finalizer's chunk records (callers size it with nsg_bn_tiles_bytes)
struct BnTilesLayout { float *tiles; double *chunks; size_t bytes; };
static BnTilesLayout bn_tiles_layout(void *buf, int64_t ntiles, int C)
{
    NsgCarver c(buf);
    return {c.take<float>(nsg_align_up((size_t)ntiles * 3 * C, 64) * sizeof(float)),
            c.take<double>((size_t)TILE_CHUNKS * 3 * C * sizeof(double)), c.off + 256};
}

// used by nsg_conv_forward_bnstats (conv_api.hip): merge the per-tile statistics the conv epilogue wrote
int nsg_bn_stats_from_tiles(const float *tiles, int ntiles, int64_t M, int C, float eps, float momentum, float *mean,
                            float *invstd, float *running_mean, float *running_var, hipStream_t s)
{
    if (ntiles <= MAX_SLABS && C % 4 == 0) {
        hipLaunchKernelGGL(bn_stats_tiles_onepass_kernel, dim3(C / 4), dim3(256), 0, s, tiles, ntiles, M, C, eps, momentum, mean, invstd,
                           running_mean, running_var);
        return nsg_check_launch("bn_stats_tiles_onepass_kernel");
    }
    double *chunks = bn_tiles_layout(const_cast<float *>(tiles), ntiles, C).chunks;
    hipLaunchKernelGGL(bn_stats_tiles_fold_kernel, dim3(TILE_CHUNKS), dim3(256), 0, s, tiles, ntiles, C, chunks);
    hipLaunchKernelGGL(bn_stats_tiles_final_kernel, dim3((C + 255) / 256), dim3(256), 0, s, chunks, M, C, eps, momentum, mean, invstd,
                       running_mean, running_var);
    return nsg_check_launch("bn_stats_from_tiles");
}

size_t nsg_bn_tiles_bytes(int64_t ntiles, int C) { return bn_tiles_layout(nullptr, ntiles, C).bytes; }

// the slab structure of nsg_bn_backward_sums over M rows (a producer of dy that forms the same sums itself launches over it)
void nsg_bn_slab_geom(int64_t M, int *nslab, int *rows)
{
    const SlabGeom g = slab_geom(M);
    *nslab = g.nslab;
    *rows = g.rows;
}

// what the one-block-per-4-channels finalisers can take
static int check_slabs(const char *what, int nslab, int C)
{
    if (nslab < 1 || nslab > MAX_SLABS || C % 4) return nsg_fail(NSG_E_INVALID, "%s: %d slabs / %d channels not supported", what, nslab, C);
    return NSG_OK;
}

int nsg_launch_bn_bwd_final(const float *partial, int nslab, int C, float *dgamma, float *dbeta, hipStream_t s)
{
    if (int rc = check_slabs("bn_bwd_final", nslab, C)) return rc;
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(C / 4), dim3(256), 0, s, partial, nslab, C, dgamma, dbeta, (const float *)nullptr, (float *)nullptr);
    return nsg_check_launch("bn_bwd_final_kernel");
}

int nsg_launch_bn_bwd_final_wreduce(const float *partial, const float *colsum_partial, int nslab, int C, float *dgamma, float *dbeta, float *colsum,
                                    const float *wpartial, float *wdst, int wn, hipStream_t s)
{
    if (int rc = check_slabs("bn_bwd_final", nslab, C)) return rc;
    const int split = nsg_slab_split(nslab, wn);
    const int wblocks = (wn + 256 / split - 1) / (256 / split);
    hipLaunchKernelGGL(bn_bwd_final_wreduce_kernel, dim3(C / 4 + wblocks), dim3(256), 0, s, partial, nslab, C, dgamma, dbeta, colsum_partial, colsum,
                       wpartial, wdst, wn, split);
    return nsg_check_launch("bn_bwd_final_wreduce_kernel");
}

int nsg_launch_slab_sum_final(const float *partial, int nslab, int C, float *out, hipStream_t s)
{
    if (int rc = check_slabs("slab_sum_final", nslab, C)) return rc;
    hipLaunchKernelGGL(slab_sum_final_kernel, dim3(C / 4), dim3(256), 0, s, partial, nslab, C, out);
    return nsg_check_launch("slab_sum_final_kernel");
}

// f(T()) with T the storage type of dtype (checked by check_mc): a launch is written once, for T
template <typename F>
static void by_dtype(int dtype, F f)
{
    if (dtype == NSG_BF16) f(bf16_t());
    else f(float());
}

// The backward over [M][C] in its two halves, which nsg_bn_backward runs one after the other.
struct BnBwd {
    const void *x, *y_relu, *dy;
    const float *mean, *invstd, *gamma, *relu_beta;
    int64_t M;
    int C, dtype;
    float *partial;      // the workspace: [nslab][2][C]
    hipStream_t s;
};

// the entry points' shared argument checks; dx: the apply half's output (its null check is the caller's), null for the sums alone
static int bn_bwd_check(const char *fn, const BnBwd &b, const float *dgamma, const float *dbeta, const void *dx, size_t workspace_bytes)
{
    NSG_REQUIRE(b.x && b.dy && b.mean && b.invstd && b.gamma && dgamma && dbeta, NSG_E_INVALID, "%s: null pointer", fn);
    if (int rc = check_mc(fn, b.M, b.C, b.dtype)) return rc;
    NSG_REQUIRE(nsg_aligned16(b.x) && nsg_aligned16(b.dy) && nsg_aligned16(dx) && (!b.y_relu || nsg_aligned16(b.y_relu)), NSG_E_INVALID,
                "%s: pointers must be 16-byte aligned", fn);
    NSG_REQUIRE(b.partial && workspace_bytes >= nsg_bn_workspace_bytes(b.M, b.C), NSG_E_WORKSPACE, "%s: workspace too small", fn);
    return NSG_OK;
}

// dgamma, dbeta <- the per-slab sums and their finaliser
static void bn_bwd_launch_sums(const BnBwd &b, float *dgamma, float *dbeta)
{
    const SlabGeom g = slab_geom(b.M);
    by_dtype(b.dtype, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((bn_bwd_partial_kernel<T>), dim3(g.nslab), dim3(256), 0, b.s, (const T *)b.x, (const T *)b.y_relu, (const T *)b.dy, b.mean,
                           b.invstd, b.gamma, b.relu_beta, b.M, b.C, g.rows, b.partial);
    });
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(b.C / 4), dim3(256), 0, b.s, b.partial, g.nslab, b.C, dgamma, dbeta, (const float *)nullptr, (float *)nullptr);
}

// dx (and dx_colsum) from dgamma, dbeta.  Whatever sat in the workspace has been consumed (stream order): it takes the dx column sums.
static void bn_bwd_launch_apply(const BnBwd &b, const float *dgamma, const float *dbeta, void *dx, float *dx_colsum)
{
    const SlabGeom g = slab_geom(b.M);
    const float inv_m = 1.0f / (float)b.M;
    by_dtype(b.dtype, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T>), dim3(g.nslab), dim3(256), 0, b.s, (const T *)b.x, (const T *)b.y_relu, (const T *)b.dy, b.mean,
                           b.invstd, b.gamma, dgamma, dbeta, b.relu_beta, (T *)dx, b.M, b.C, g.rows, inv_m, dx_colsum ? b.partial : nullptr);
    });
    if (dx_colsum) hipLaunchKernelGGL(slab_sum_final_kernel, dim3(b.C / 4), dim3(256), 0, b.s, b.partial, g.nslab, b.C, dx_colsum);
}

extern "C" {

size_t nsg_bn_workspace_bytes(int64_t M, int32_t C)
{
    if (M <= 0 || C <= 0) return 0;
    return (size_t)slab_geom(M).nslab * 2 * C * sizeof(float);
}

int nsg_bn_stats(const void *x, int64_t M, int32_t C, int32_t dtype, float eps, float momentum, float *mean, float *invstd,
                 float *running_mean, float *running_var, void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(x && mean && invstd, NSG_E_INVALID, "nsg_bn_stats: null pointer");
    int rc = check_mc("nsg_bn_stats", M, C, dtype);
    if (rc) return rc;
    NSG_REQUIRE(nsg_aligned16(x), NSG_E_INVALID, "nsg_bn_stats: x must be 16-byte aligned");
    NSG_REQUIRE(workspace && workspace_bytes >= nsg_bn_workspace_bytes(M, C), NSG_E_WORKSPACE, "nsg_bn_stats: workspace too small");
    const SlabGeom g = slab_geom(M);
    hipStream_t s = (hipStream_t)stream;
    float *partial = reinterpret_cast<float *>(workspace);
    by_dtype(dtype, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((bn_stats_partial_kernel<T>), dim3(g.nslab), dim3(256), 0, s, reinterpret_cast<const T *>(x), M, C, g.rows, partial);
    });
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3(C / 4), dim3(256), 0, s, partial, g.nslab, g.rows, M, C, eps,
                       momentum, mean, invstd, running_mean, running_var);
    return nsg_check_launch("bn_stats");
}

int nsg_bn_eval_stats(const float *running_mean, const float *running_var, int32_t C, float eps, float *mean,
                      float *invstd, void *stream)
{
    NSG_REQUIRE(running_mean && running_var && mean && invstd && C > 0, NSG_E_INVALID, "nsg_bn_eval_stats: bad argument");
    hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, running_mean,
                       running_var, C, eps, mean, invstd);
    return nsg_check_launch("bn_eval_stats");
}

int nsg_bn_apply(const void *x, const float *mean, const float *invstd, const float *gamma, const float *beta,
                 const void *residual, void *y, int64_t M, int32_t C, int32_t relu, int32_t relu_residual, int32_t dtype,
                 int32_t y_dtype, void *stream)
{
    NSG_REQUIRE(x && mean && invstd && gamma && beta && y, NSG_E_INVALID, "nsg_bn_apply: null pointer");
    int rc = check_mc("nsg_bn_apply", M, C, dtype);
    if (rc) return rc;
    NSG_REQUIRE(y_dtype == NSG_F32 || y_dtype == NSG_BF16, NSG_E_INVALID, "nsg_bn_apply: unknown output dtype");
    NSG_REQUIRE(nsg_aligned16(x) && nsg_aligned16(y) && (!residual || nsg_aligned16(residual)), NSG_E_INVALID,
                "nsg_bn_apply: pointers must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int W = (dtype == NSG_BF16 || y_dtype == NSG_BF16) ? 8 : 4;
    NSG_REQUIRE(C % W == 0, NSG_E_UNSUPPORTED, "nsg_bn_apply: C=%d must be a multiple of %d", C, W);
    const int64_t nw = M * C / W;
    // grid stride (blocks * 256) must be a multiple of the row length CW = C / W so that a thread keeps its channels
    int blocks = ew_blocks(nw);
    {
        const int CW = C / W;
        int a = CW, b = 256;
        while (b) { const int t = a % b; a = b; b = t; }      // a = gcd(CW, 256)
        const int mult = CW / a;
        blocks = (blocks + mult - 1) / mult * mult;
    }
    const dim3 grid(blocks), blk(256);
#define NSG_BN_APPLY(TX, TY)                                                                                             \
    hipLaunchKernelGGL((bn_apply_kernel<TX, TY>), grid, blk, 0, s, reinterpret_cast<const TX *>(x), mean, invstd, gamma, \
                       beta, reinterpret_cast<const TX *>(residual), reinterpret_cast<TY *>(y), nw, C / W, relu, relu_residual)
    if (dtype == NSG_F32 && y_dtype == NSG_F32) NSG_BN_APPLY(float, float);
    else if (dtype == NSG_BF16 && y_dtype == NSG_BF16) NSG_BN_APPLY(bf16_t, bf16_t);
    else if (dtype == NSG_BF16 && y_dtype == NSG_F32) NSG_BN_APPLY(bf16_t, float);
    else NSG_BN_APPLY(float, bf16_t);
#undef NSG_BN_APPLY
    return nsg_check_launch("bn_apply_kernel");
}

int nsg_bn_backward(const void *x, const void *y_relu, const void *dy, const float *mean, const float *invstd,
                    const float *gamma, const float *relu_beta, void *dx, float *dgamma, float *dbeta, float *dx_colsum,
                    int64_t M, int32_t C, int32_t dtype, void *workspace, size_t workspace_bytes, void *stream)
{
    const BnBwd b = {x, y_relu, dy, mean, invstd, gamma, relu_beta, M, C, dtype, reinterpret_cast<float *>(workspace), (hipStream_t)stream};
    NSG_REQUIRE(dx, NSG_E_INVALID, "nsg_bn_backward: null pointer");
    if (int rc = bn_bwd_check("nsg_bn_backward", b, dgamma, dbeta, dx, workspace_bytes)) return rc;
    bn_bwd_launch_sums(b, dgamma, dbeta);
    bn_bwd_launch_apply(b, dgamma, dbeta, dx, dx_colsum);
    return nsg_check_launch("bn_backward");
}

/* The apply half of nsg_bn_backward alone: dgamma / dbeta are INPUTS (nsg_bn_backward_sums, or a producer that formed the
 * same sums while it wrote dy). */
int nsg_bn_backward_apply(const void *x, const void *y_relu, const void *dy, const float *mean, const float *invstd, const float *gamma,
                          const float *relu_beta, const float *dgamma, const float *dbeta, void *dx, float *dx_colsum, int64_t M, int32_t C,
                          int32_t dtype, void *workspace, size_t workspace_bytes, void *stream)
{
    const BnBwd b = {x, y_relu, dy, mean, invstd, gamma, relu_beta, M, C, dtype, reinterpret_cast<float *>(workspace), (hipStream_t)stream};
    NSG_REQUIRE(dx, NSG_E_INVALID, "nsg_bn_backward_apply: null pointer");
    if (int rc = bn_bwd_check("nsg_bn_backward_apply", b, dgamma, dbeta, dx, workspace_bytes)) return rc;
    bn_bwd_launch_apply(b, dgamma, dbeta, dx, dx_colsum);
    return nsg_check_launch("bn_backward_apply");
}

/* The reduction half of nsg_bn_backward alone: dgamma, dbeta (what a fused consumer of the apply half needs first). */
int nsg_bn_backward_sums(const void *x, const void *y_relu, const void *dy, const float *mean, const float *invstd, const float *gamma,
                         const float *relu_beta, float *dgamma, float *dbeta, int64_t M, int32_t C, int32_t dtype, void *workspace,
                         size_t workspace_bytes, void *stream)
{
    const BnBwd b = {x, y_relu, dy, mean, invstd, gamma, relu_beta, M, C, dtype, reinterpret_cast<float *>(workspace), (hipStream_t)stream};
    if (int rc = bn_bwd_check("nsg_bn_backward_sums", b, dgamma, dbeta, nullptr, workspace_bytes)) return rc;
    bn_bwd_launch_sums(b, dgamma, dbeta);
    return nsg_check_launch("bn_backward_sums");
}

}  // extern "C"
