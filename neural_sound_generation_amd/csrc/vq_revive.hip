// Codebook usage statistics and dead-code revival (extension: the reference's plain nearest-neighbour codebook has neither; its
// U(-1/K, 1/K) initialisation leaves a handful of live codes, DESIGN.md "Codebook usage and revival").
//
//   nsg_code_usage   every step of a run that asked for it: histogram of the batch's indices, the running window += it, and the
//                    batch's perplexity / number of codes in use.  Reads N * 8 bytes.
//                      usage_hist   per block of 4096 rows: LDS bins (K <= 8192), one integer atomic per non-zero bin -- a batch
//                                   with every row on one code costs one global atomic per block, not one per row
//                      usage_final  one block: window += batch_counts, fp64 entropy in a fixed order
//   nsg_vq_revive(_bnres)   every R-th step: codes the window saw fewer than min_count times take rows of the current z_e.
//                      revive_scan  one block: dead flags of window -> slot[k] = rank among the dead codes (exclusive scan), window = 0
//                      revive_copy  one thread per (code, 16-byte piece): the chosen row -> codebook (and ema_sum), moments zeroed
// Latency-class work (K * D * 4 <= 8 MB written): nothing here is tuned beyond coalesced 16-byte accesses.  Integer atomics
// only, so every result is independent of arrival order.
#include "nsg_common.h"

namespace {

constexpr int USAGE_ROWS = 4096;      // rows per histogram block
constexpr int USAGE_LDS_K = 8192;     // largest K binned in LDS (32 KiB); beyond it the rows add to global memory directly

__global__ __launch_bounds__(256) void usage_hist_kernel(const int64_t *__restrict__ idx, int64_t N, int K, int *__restrict__ batch_counts)
{
    extern __shared__ int bins[];
    const bool lds = K <= USAGE_LDS_K;
    if (lds) {
        for (int k = threadIdx.x; k < K; k += 256) bins[k] = 0;
        __syncthreads();
    }
    const int64_t r0 = (int64_t)blockIdx.x * USAGE_ROWS;
    for (int i = threadIdx.x; i < USAGE_ROWS; i += 256) {
        const int64_t r = r0 + i;
        if (r < N) {
            const int64_t c = idx[r];
            if (c >= 0 && c < K) atomicAdd(lds ? &bins[(int)c] : &batch_counts[(int)c], 1);
        }
    }
    if (lds) {
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += 256) {
            const int v = bins[k];
            if (v) atomicAdd(&batch_counts[k], v);
        }
    }
}

// stats[0] = exp(H), H = ln T - (sum_k c_k ln c_k) / T = -sum_k p_k ln p_k with p_k = c_k / T, T = sum_k c_k; stats[1] = #{c_k > 0}.
// A thread adds its codes k = tid, tid + 1024, ... in that order, the 1024 thread sums meet in a fixed LDS tree.
__global__ __launch_bounds__(1024) void usage_final_kernel(const int *__restrict__ batch_counts, int K, int *__restrict__ window,
                                                          double *__restrict__ stats)
{
    __shared__ double sh[1024];
    __shared__ long long st[1024];
    __shared__ int su[1024];
    const int tid = threadIdx.x;
    double h = 0.0;
    long long t = 0;
    int u = 0;
    for (int k = tid; k < K; k += 1024) {
        const int c = batch_counts[k];
        if (c > 0) {
            window[k] += c;
            h += (double)c * log((double)c);
            t += c;
            ++u;
        }
    }
    sh[tid] = h; st[tid] = t; su[tid] = u;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (tid < off) { sh[tid] += sh[tid + off]; st[tid] += st[tid + off]; su[tid] += su[tid + off]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double T = (double)st[0];
        stats[0] = st[0] > 0 ? exp(log(T) - sh[0] / T) : 0.0;
        stats[1] = (double)su[0];
    }
}

// slot[k] = number of dead codes below k for a dead code, -1 for a live one; window cleared; stats[0] = dead codes, stats[1] += them
__global__ __launch_bounds__(1024) void revive_scan_kernel(int *__restrict__ window, int K, int min_count, int revive_all,
                                                          int *__restrict__ slot, int64_t *__restrict__ stats)
{
    __shared__ int sa[1024];
    const int tid = threadIdx.x;
    const int per = (K + 1023) / 1024;
    const int k0 = min(K, tid * per), k1 = min(K, k0 + per);
    int a = 0;
    for (int k = k0; k < k1; ++k) a += (revive_all || window[k] < min_count) ? 1 : 0;
    sa[tid] = a;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {          // Hillis-Steele inclusive scan (integers: exact)
        const int v = tid >= off ? sa[tid - off] : 0;
        __syncthreads();
        sa[tid] += v;
        __syncthreads();
    }
    int run = sa[tid] - a;
    for (int k = k0; k < k1; ++k) {
        const bool dead = revive_all || window[k] < min_count;
        slot[k] = dead ? run : -1;
        run += dead ? 1 : 0;
        window[k] = 0;
    }
    if (tid == 1023) {
        stats[0] = sa[1023];
        stats[1] += sa[1023];
    }
}

// four bf16 elements (8 bytes) as floats
__device__ __forceinline__ void revive_ld_bf16x4(const bf16_t *p, float *o)
{
    const uint2 u = *reinterpret_cast<const uint2 *>(p);
    o[0] = nsg_bitsf(u.x << 16); o[1] = nsg_bitsf(u.x & 0xffff0000u);
    o[2] = nsg_bitsf(u.y << 16); o[3] = nsg_bitsf(u.y & 0xffff0000u);
}

struct ReviveArgs {
    float *codebook, *adam_m, *adam_v, *ema_count, *ema_sum;   // all but codebook may be null
    const int *slot;
    int64_t N, base_row, stride;
    int K, D;
};

// one thread per (code, 16-byte piece of its row).  BNRES: the row is formed from its sources as bn_apply forms it (BnResLane).
template <bool BNRES>
__global__ __launch_bounds__(256) void revive_copy_kernel(const typename RowArg<BNRES>::T z, const ReviveArgs a)
{
    const int ppr = a.D >> 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)a.K * ppr) return;
    const int k = (int)(t / ppr), pc = (int)(t - (int64_t)k * ppr);
    const int j = a.slot[k];
    if (j < 0) return;                                               // live rows of every array are not written at all
    const int64_t row = (int64_t)(((uint64_t)a.base_row + (uint64_t)j * (uint64_t)a.stride) % (uint64_t)a.N);
    v4f v;
    if constexpr (BNRES) {
        BnResLane<4> lane;
        lane.init(z, pc * 4);
        float hv[4], rv[4], o[4];
        revive_ld_bf16x4(z.h + (size_t)row * a.D + pc * 4, hv);
        revive_ld_bf16x4(z.r + (size_t)row * a.D + pc * 4, rv);
        lane.apply(hv, rv, o);
        v = v4f{o[0], o[1], o[2], o[3]};
    } else {
        v = *reinterpret_cast<const v4f *>(z + (size_t)row * a.D + pc * 4);
    }
    const size_t off = (size_t)k * a.D + pc * 4;
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<v4f *>(a.codebook + off) = v;
    if (a.adam_m) *reinterpret_cast<v4f *>(a.adam_m + off) = zero;
    if (a.adam_v) *reinterpret_cast<v4f *>(a.adam_v + off) = zero;
    if (a.ema_sum) *reinterpret_cast<v4f *>(a.ema_sum + off) = v;
    if (a.ema_count && pc == 0) a.ema_count[k] = 1.0f;
}

// the checks both forms share (what: the entry point's name)
int revive_check(const char *what, const void *codebook, const int32_t *window, const int32_t *slot, const int64_t *stats, int64_t N, int32_t D,
                 int32_t K, int64_t base_row, int64_t stride, const float *adam_m, const float *adam_v, const float *ema_count, const float *ema_sum)
{
    NSG_REQUIRE(codebook && window && slot && stats, NSG_E_INVALID, "%s: null pointer", what);
    NSG_REQUIRE(N >= 1 && N < 0x7fffffffll && K >= 1 && D >= 1, NSG_E_INVALID, "%s: 1 <= N < 2^31, K and D positive", what);
    NSG_REQUIRE(stride >= 1 && stride < 0x7fffffffll, NSG_E_INVALID, "%s: 1 <= stride < 2^31", what);
    NSG_REQUIRE(base_row >= 0 && base_row < N, NSG_E_INVALID, "%s: base_row must lie in [0, N)", what);
    NSG_REQUIRE(D % 4 == 0, NSG_E_UNSUPPORTED, "%s: D %% 4 == 0", what);
    NSG_REQUIRE(nsg_aligned16(codebook) && nsg_aligned16(adam_m) && nsg_aligned16(adam_v) && nsg_aligned16(ema_sum), NSG_E_UNSUPPORTED,
                "%s: 16-byte aligned tensors", what);
    NSG_REQUIRE((adam_m == nullptr) == (adam_v == nullptr) && (ema_count == nullptr) == (ema_sum == nullptr), NSG_E_INVALID,
                "%s: adam_m / adam_v and ema_count / ema_sum are given in pairs", what);
    return NSG_OK;
}

template <bool BNRES>
int revive_launch(const typename RowArg<BNRES>::T z, const ReviveArgs &a, int32_t *window, int32_t min_count, int32_t revive_all, int32_t *slot,
                  int64_t *stats, void *stream, const char *what)
{
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(revive_scan_kernel, dim3(1), dim3(1024), 0, s, window, a.K, min_count, revive_all != 0 ? 1 : 0, slot, stats);
    const int64_t threads = (int64_t)a.K * (a.D >> 2);
    hipLaunchKernelGGL(revive_copy_kernel<BNRES>, dim3((unsigned)nsg_cdiv(threads, 256)), dim3(256), 0, s, z, a);
    return nsg_check_launch(what);
}

}  // namespace

extern "C" {

int nsg_code_usage(const int64_t *idx, int64_t N, int32_t K, int32_t *batch_counts, int32_t *window, double *stats, void *stream)
{
    NSG_REQUIRE(idx && batch_counts && window && stats, NSG_E_INVALID, "nsg_code_usage: null pointer");
    NSG_REQUIRE(N >= 1 && N < 0x7fffffffll && K >= 1, NSG_E_INVALID, "nsg_code_usage: 1 <= N < 2^31 and K >= 1");
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(batch_counts, 0, (size_t)K * 4, s);
    if (e != hipSuccess) return nsg_fail((int)e, "nsg_code_usage: hipMemsetAsync: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(usage_hist_kernel, dim3((unsigned)nsg_cdiv(N, USAGE_ROWS)), dim3(256), K <= USAGE_LDS_K ? (size_t)K * 4 : 0, s, idx, N, K,
                       batch_counts);
    hipLaunchKernelGGL(usage_final_kernel, dim3(1), dim3(1024), 0, s, batch_counts, K, window, stats);
    return nsg_check_launch("nsg_code_usage");
}

int nsg_vq_revive(const float *z, int64_t N, int32_t D, float *codebook, int32_t K, int32_t *window, int32_t min_count, int64_t base_row,
                  int64_t stride, float *adam_m, float *adam_v, float *ema_count, float *ema_sum, int32_t *slot, int64_t *stats,
                  int32_t revive_all, void *stream)
{
    NSG_REQUIRE(z, NSG_E_INVALID, "nsg_vq_revive: null pointer");
    const int rc = revive_check("nsg_vq_revive", codebook, window, slot, stats, N, D, K, base_row, stride, adam_m, adam_v, ema_count, ema_sum);
    if (rc != NSG_OK) return rc;
    NSG_REQUIRE(nsg_aligned16(z), NSG_E_UNSUPPORTED, "nsg_vq_revive: 16-byte aligned tensors");
    const ReviveArgs a = {codebook, adam_m, adam_v, ema_count, ema_sum, slot, N, base_row, stride, K, D};
    return revive_launch<false>(z, a, window, min_count, revive_all, slot, stats, stream, "nsg_vq_revive");
}

int nsg_vq_revive_bnres(const void *h, const void *r, const float *mean, const float *invstd, const float *gamma, const float *beta, int64_t N,
                        int32_t D, float *codebook, int32_t K, int32_t *window, int32_t min_count, int64_t base_row, int64_t stride,
                        float *adam_m, float *adam_v, float *ema_count, float *ema_sum, int32_t *slot, int64_t *stats, int32_t revive_all,
                        void *stream)
{
    NSG_REQUIRE(h && r && mean && invstd && gamma && beta, NSG_E_INVALID, "nsg_vq_revive_bnres: null pointer");
    const int rc = revive_check("nsg_vq_revive_bnres", codebook, window, slot, stats, N, D, K, base_row, stride, adam_m, adam_v, ema_count, ema_sum);
    if (rc != NSG_OK) return rc;
    NSG_REQUIRE(D >= 8 && D <= 256 && (D & (D - 1)) == 0, NSG_E_UNSUPPORTED, "nsg_vq_revive_bnres: D a power of two in 8 ... 256");
    NSG_REQUIRE(nsg_aligned16(h) && nsg_aligned16(r), NSG_E_UNSUPPORTED, "nsg_vq_revive_bnres: 16-byte aligned tensors");
    const BnResRows src = {reinterpret_cast<const bf16_t *>(h), reinterpret_cast<const bf16_t *>(r), mean, invstd, gamma, beta};
    const ReviveArgs a = {codebook, adam_m, adam_v, ema_count, ema_sum, slot, N, base_row, stride, K, D};
    return revive_launch<true>(src, a, window, min_count, revive_all, slot, stats, stream, "nsg_vq_revive_bnres");
}

}  // extern "C"
