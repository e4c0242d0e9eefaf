// The F0-conditioned decoder's kernels (an extension: the reference's VQVAE knows neither the speaker nor the pitch).  include/nsg.h
// states the definitions (nsg_add_cond, nsg_column_sum, nsg_f0_bins, nsg_collate_f0_bins); tests/helpers/f0_cond_ref.py restates them in numpy.
//   * add_cond_kernel: the decoder input in one pass -- latent rows (given, or gathered from the codebook through the code indices)
//     + the clip's speaker row + the column's F0 row, ReLU, the store type's rounding.  HBM-bound on the rows and the output; the two
//     tables and the index vectors stay in L2.  Two 16-byte-vector items per thread and trip: the index loads of both, then the
//     (up to) six row loads of both, are in flight before the first add.
//   * column_sum_kernel: out[b][w][:] = sum over h of x[b][h][w][:], one thread per (b, w, 16-byte channel vector), h ascending in
//     fp32, four rows' loads in flight per trip.  No atomics, no workspace: the order is fixed by construction.
//   * f0_bins_kernel: one thread per latent column: the voiced frames' mean log2 F0, the affine move, the bin (f0_column).
//   * collate_f0_bins_kernel: the same column rule on frames read straight out of a corpus-wide F0 track through the loader's plan
//     rows (nsg_collate_f0_bins; data.ResidentMelCorpus.track_f0): a batch's bins without tracking anything in the training loop.
// None of them takes a workspace.
#include "nsg_common.h"
#include <math.h>

namespace {

__device__ __forceinline__ int64_t clamp_index(int64_t v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

struct CondGeom {
    int CW, HW, Wd;          // 16-byte vectors per row, latent pixels per clip, latent columns
    FastDiv div_cw, div_hw, div_w;
};

// y[row][:] = act((src(row)[:] + clip[b][:]) + table[bins[b][w]][:]), row = (b * H + h) * Wd + w; nw counts vectors of
// W = Width<float, TY> channels (nw < 2^31: the launcher's check, so the divisions are FastDiv's).
template <typename TY, bool GATHER>
__global__ __launch_bounds__(256) void add_cond_kernel(const float *__restrict__ x, const int64_t *__restrict__ idx, const float *__restrict__ clip,
                                                       const float *__restrict__ table, const int64_t *__restrict__ bins, TY *__restrict__ y,
                                                       int64_t nw, const CondGeom g, int K, int n_rows, int relu)
{
    constexpr int W = Width<float, TY>::W;
    constexpr int U = 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < nw; i0 += U * stride) {
        int64_t it[U], xo[U], to[U], co[U];
        int64_t kb[U], kx[U];
        // (an item past the end repeats the last one's loads and stores nothing: the loads stay branch-free)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            it[u] = i0 + u * stride < nw ? i0 + u * stride : nw - 1;
            const int row = nsg_div((int)it[u], g.div_cw);
            const int c = (int)it[u] - row * g.CW;
            const int b = nsg_div(row, g.div_hw);
            const int p = row - b * g.HW;
            const int w = p - nsg_div(p, g.div_w) * g.Wd;
            kb[u] = bins[(int64_t)b * g.Wd + w];
            kx[u] = GATHER ? idx[row] : 0;
            co[u] = ((int64_t)b * g.CW + c) * W;
            to[u] = (int64_t)c * W;
            xo[u] = GATHER ? (int64_t)c * W : it[u] * W;
        }
        float xv[U][W], cv[U][W], tv[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (GATHER) xo[u] += clamp_index(kx[u], K) * g.CW * W;
            to[u] += clamp_index(kb[u], n_rows) * g.CW * W;
            ldw<float, W>(x + xo[u], xv[u]);
            if (clip) ldw<float, W>(clip + co[u], cv[u]);
            ldw<float, W>(table + to[u], tv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (clip)
#pragma unroll
                for (int e = 0; e < W; ++e) xv[u][e] += cv[u][e];
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const float v = xv[u][e] + tv[u][e];
                xv[u][e] = relu ? fmaxf(v, 0.f) : v;
            }
            if (i0 + u * stride < nw) stw<TY, W>(y + it[u] * W, xv[u]);
        }
    }
}

// out[b][w][:] = sum_h x[b][h][w][:]; nv = B * Wd * CW vectors of W = Elem<T>::N channels, WCW = Wd * CW vectors per latent row.
template <typename T>
__global__ __launch_bounds__(256) void column_sum_kernel(const T *__restrict__ x, float *__restrict__ out, int64_t nv, int H, int WCW,
                                                         FastDiv div_wcw)
{
    constexpr int W = Elem<T>::N;
    constexpr int U = 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = nsg_div((int)i, div_wcw);
        const int r = (int)i - b * WCW;
        const T *p = x + ((int64_t)b * H * WCW + r) * W;
        const int64_t step = (int64_t)WCW * W;
        float acc[W];
#pragma unroll
        for (int e = 0; e < W; ++e) acc[e] = 0.f;
        int h = 0;
        for (; h + U <= H; h += U) {
            float v[U][W];
#pragma unroll
            for (int u = 0; u < U; ++u) ldw<T, W>(p + (h + u) * step, v[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < W; ++e) acc[e] += v[u][e];
        }
        for (; h < H; ++h) {
            float v[W];
            ldw<T, W>(p + h * step, v);
#pragma unroll
            for (int e = 0; e < W; ++e) acc[e] += v[e];
        }
        stw<float, W>(out + i * W, acc);
    }
}

// The column rule, stated once (include/nsg.h: nsg_f0_bins): fv = the column's four frames, of which frame `first + t` counts when
// it lies below len and is voiced; row = the clip's affine row or null.  lo = fl(log2 fmin), span = fl(log2 fmax) - lo and
// nb = (float)n_bins come from the launcher; the expressions are include/nsg.h's, in its order (-ffp-contract=off).
__device__ __forceinline__ void f0_column(const float (&fv)[4], int first, int len, const float *__restrict__ row, float lo, float span, float nb,
                                          int64_t &bin, float &lf)
{
    int n = 0;
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (first + t < len && fv[t] > 0.f) {
            sum += (float)log2((double)fv[t]);
            ++n;
        }
    }
    bin = 0;
    lf = 0.f;
    if (n >= 2) {
        lf = sum / (float)n;
        if (row) {
            const float ms = row[0], ratio = row[1], mt = row[2];
            lf = mt + (lf - ms) * ratio;
        }
        const float u = ((lf - lo) * nb) / span;
        bin = 1 + (int64_t)fminf(fmaxf(floorf(u), 0.f), nb - 1.f);
    }
}

// One thread per latent column (b, w): frames 4w .. 4w + 3 of clip b.
__global__ __launch_bounds__(256) void f0_bins_kernel(const float *__restrict__ f0, const int32_t *__restrict__ frames, const float *__restrict__ affine,
                                                      int64_t *__restrict__ bins, float *__restrict__ logf, int B, int T, int Wd, float lo, float span,
                                                      float nb)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * Wd) return;
    const int b = (int)(i / Wd), w = (int)(i - (int64_t)b * Wd);
    int len = frames ? frames[b] : T;
    len = len < 0 ? 0 : (len > T ? T : len);
    const float *row = f0 + (int64_t)b * T + 4 * w;           // (T >= 4 Wd: all four frames lie in the row)
    float fv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) fv[t] = row[t];
    int64_t bin;
    float lf;
    f0_column(fv, 4 * w, len, affine ? affine + 3 * b : nullptr, lo, span, nb, bin, lf);
    bins[i] = bin;
    if (logf) logf[i] = lf;
}

// nsg_f0_bins on rows cropped out of a resident track by nsg_collate_mels' plan, without the rows: one thread per frame quad
// (b, q) -- frames 4q .. 4q + 3 of item b, corpus frames start_b + 4q ..: no alignment, so four scalar loads -- of the Q quads the
// launcher asks for: W (the latent columns) or, where f0_out is wanted, ceil(T / 4) (then the quads past W only copy).  The clamps
// are collate_mels_kernel's: count into [0, T], start to where start + t cannot overflow, a frame outside [0, corpus_frames) reads
// as +0.0 -- whatever the plan holds, no access leaves a buffer.
__global__ __launch_bounds__(256) void collate_f0_bins_kernel(const float *__restrict__ corpus, int64_t corpus_frames, const int64_t *__restrict__ plan,
                                                              const float *__restrict__ affine, int64_t *__restrict__ bins, float *__restrict__ logf,
                                                              float *__restrict__ f0_out, int B, int T, int Wd, int Q, float lo, float span, float nb)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * Q) return;
    const int b = (int)(i / Q), q = (int)(i - (int64_t)b * Q);
    int64_t start = plan[(int64_t)b * 3 + 1], count = plan[(int64_t)b * 3 + 2];
    count = count < 0 ? 0 : (count > T ? T : count);
    start = start < -((int64_t)1 << 31) ? -((int64_t)1 << 31) : (start > corpus_frames ? corpus_frames : start);
    float fv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t f = start + 4 * q + t;                  // |f| <= 2^31 + corpus_frames + T: no overflow
        fv[t] = (4 * q + t < count && f >= 0 && f < corpus_frames) ? corpus[f] : 0.f;
    }
    if (f0_out)
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (4 * q + t < T) f0_out[(int64_t)b * T + 4 * q + t] = fv[t];
    if (q >= Wd) return;                                      // (T >= 4 Wd: a column's four frames lie below T)
    int64_t bin;
    float lf;
    f0_column(fv, 4 * q, (int)count, affine ? affine + 3 * b : nullptr, lo, span, nb, bin, lf);
    bins[(int64_t)b * Wd + q] = bin;
    if (logf) logf[(int64_t)b * Wd + q] = lf;
}

inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int nsg_add_cond(const float *x, const int64_t *idx, const float *clip_rows, const float *table, const int64_t *bins, void *y, int32_t B,
                 int32_t H, int32_t W, int32_t C, int32_t K, int32_t n_rows, int32_t relu, int32_t y_dtype, void *stream)
{
    NSG_REQUIRE(x && table && bins && y, NSG_E_INVALID, "nsg_add_cond: null pointer (x, table, bins and y are required)");
    NSG_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && n_rows > 0 && (!idx || K > 0), NSG_E_INVALID,
                "nsg_add_cond: B, H, W, C, n_rows (and K with idx) must be positive");
    NSG_REQUIRE(y_dtype == NSG_F32 || y_dtype == NSG_BF16, NSG_E_INVALID, "nsg_add_cond: unknown dtype");
    const int V = y_dtype == NSG_BF16 ? 8 : 4;
    NSG_REQUIRE(C % V == 0, NSG_E_INVALID, "nsg_add_cond: C = %d must be a multiple of %d", C, V);
    NSG_REQUIRE(nsg_aligned16(x) && nsg_aligned16(table) && nsg_aligned16(y) && (!clip_rows || nsg_aligned16(clip_rows)) &&
                aligned_to(bins, 8) && (!idx || aligned_to(idx, 8)), NSG_E_INVALID,
                "nsg_add_cond: x, clip_rows, table and y must be 16-byte aligned, idx and bins 8-byte aligned");
    const int64_t rows = (int64_t)B * H * W;
    NSG_REQUIRE(rows * C < (1ll << 31) && (int64_t)n_rows * C < (1ll << 31) && (!idx || (int64_t)K * C < (1ll << 31)), NSG_E_INVALID,
                "nsg_add_cond: B * H * W * C, n_rows * C and K * C must stay below 2^31");
    const int CW = C / V;
    const int64_t nw = rows * CW;
    const CondGeom g = {CW, H * W, W, nsg_fastdiv((uint32_t)CW), nsg_fastdiv((uint32_t)(H * W)), nsg_fastdiv((uint32_t)W)};
    const dim3 grid(ew_blocks((nw + 1) / 2)), block(256);
    hipStream_t s = (hipStream_t)stream;
#define NSG_ADD_COND(TY, GATHER) \
    hipLaunchKernelGGL((add_cond_kernel<TY, GATHER>), grid, block, 0, s, x, idx, clip_rows, table, bins, (TY *)y, nw, g, (int)K, (int)n_rows, (int)relu)
    if (y_dtype == NSG_BF16) { if (idx) NSG_ADD_COND(bf16_t, true); else NSG_ADD_COND(bf16_t, false); }
    else                     { if (idx) NSG_ADD_COND(float, true);  else NSG_ADD_COND(float, false); }
#undef NSG_ADD_COND
    return nsg_check_launch("add_cond_kernel");
}

int nsg_column_sum(const void *x, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, float *out, void *stream)
{
    NSG_REQUIRE(x && out, NSG_E_INVALID, "nsg_column_sum: null pointer");
    NSG_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, NSG_E_INVALID, "nsg_column_sum: B, H, W and C must be positive");
    NSG_REQUIRE(dtype == NSG_F32 || dtype == NSG_BF16, NSG_E_INVALID, "nsg_column_sum: unknown dtype");
    const int V = dtype == NSG_BF16 ? 8 : 4;
    NSG_REQUIRE(C % V == 0, NSG_E_INVALID, "nsg_column_sum: C = %d must be a multiple of %d", C, V);
    NSG_REQUIRE(nsg_aligned16(x) && nsg_aligned16(out), NSG_E_INVALID, "nsg_column_sum: x and out must be 16-byte aligned");
    NSG_REQUIRE((int64_t)B * H * W * C < (1ll << 31), NSG_E_INVALID, "nsg_column_sum: B * H * W * C must stay below 2^31");
    const int WCW = W * (C / V);
    const int64_t nv = (int64_t)B * WCW;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == NSG_BF16)
        hipLaunchKernelGGL((column_sum_kernel<bf16_t>), dim3(ew_blocks(nv)), dim3(256), 0, s, (const bf16_t *)x, out, nv, (int)H, WCW, nsg_fastdiv((uint32_t)WCW));
    else
        hipLaunchKernelGGL((column_sum_kernel<float>), dim3(ew_blocks(nv)), dim3(256), 0, s, (const float *)x, out, nv, (int)H, WCW, nsg_fastdiv((uint32_t)WCW));
    return nsg_check_launch("column_sum_kernel");
}

int nsg_f0_bins(const float *f0, const int32_t *frames, const float *affine, int64_t *bins, float *logf, int32_t B, int32_t T, int32_t W,
                int32_t n_bins, float fmin, float fmax, void *stream)
{
    NSG_REQUIRE(f0 && bins, NSG_E_INVALID, "nsg_f0_bins: null pointer (f0 and bins are required)");
    NSG_REQUIRE(B > 0 && T > 0 && W > 0, NSG_E_INVALID, "nsg_f0_bins: B, T and W must be positive");
    NSG_REQUIRE((int64_t)T >= 4 * (int64_t)W, NSG_E_INVALID, "nsg_f0_bins: T = %d frames do not cover W = %d latent columns (T >= 4 W)", T, W);
    NSG_REQUIRE(n_bins >= 1, NSG_E_INVALID, "nsg_f0_bins: n_bins = %d < 1", n_bins);
    NSG_REQUIRE(fmin > 0.f && fmin < fmax && fmax < INFINITY, NSG_E_INVALID, "nsg_f0_bins: the range must be 0 < fmin < fmax (finite)");
    NSG_REQUIRE(aligned_to(f0, 4) && aligned_to(bins, 8) && (!frames || aligned_to(frames, 4)) && (!affine || aligned_to(affine, 4)) &&
                (!logf || aligned_to(logf, 4)), NSG_E_INVALID, "nsg_f0_bins: misaligned pointer (4 bytes; bins 8 bytes)");
    NSG_REQUIRE((int64_t)B * T < (1ll << 31), NSG_E_INVALID, "nsg_f0_bins: B * T must stay below 2^31");
    const float lo = (float)log2((double)fmin);
    const float span = (float)log2((double)fmax) - lo;
    NSG_REQUIRE(span > 0.f, NSG_E_INVALID, "nsg_f0_bins: fmin and fmax are one value in fp32 log2");
    hipLaunchKernelGGL(f0_bins_kernel, dim3((unsigned)nsg_cdiv((int64_t)B * W, 256)), dim3(256), 0, (hipStream_t)stream, f0, frames, affine, bins, logf,
                       (int)B, (int)T, (int)W, lo, span, (float)n_bins);
    return nsg_check_launch("f0_bins_kernel");
}

int nsg_collate_f0_bins(const float *f0_corpus, int64_t corpus_frames, const int64_t *plan, const float *affine, int64_t *bins, float *logf,
                        float *f0_out, int32_t B, int32_t T, int32_t W, int32_t n_bins, float fmin, float fmax, void *stream)
{
    NSG_REQUIRE(f0_corpus && plan && bins, NSG_E_INVALID, "nsg_collate_f0_bins: null pointer (f0_corpus, plan and bins are required)");
    NSG_REQUIRE(B > 0 && T > 0 && W > 0, NSG_E_INVALID, "nsg_collate_f0_bins: B, T and W must be positive");
    NSG_REQUIRE((int64_t)T >= 4 * (int64_t)W, NSG_E_INVALID, "nsg_collate_f0_bins: T = %d frames do not cover W = %d latent columns (T >= 4 W)", T, W);
    NSG_REQUIRE(n_bins >= 1, NSG_E_INVALID, "nsg_collate_f0_bins: n_bins = %d < 1", n_bins);
    NSG_REQUIRE(fmin > 0.f && fmin < fmax && fmax < INFINITY, NSG_E_INVALID, "nsg_collate_f0_bins: the range must be 0 < fmin < fmax (finite)");
    NSG_REQUIRE(corpus_frames >= 0, NSG_E_INVALID, "nsg_collate_f0_bins: corpus_frames = %lld < 0", (long long)corpus_frames);
    NSG_REQUIRE(aligned_to(f0_corpus, 4) && aligned_to(plan, 8) && aligned_to(bins, 8) && (!affine || aligned_to(affine, 4)) &&
                (!logf || aligned_to(logf, 4)) && (!f0_out || aligned_to(f0_out, 4)), NSG_E_INVALID,
                "nsg_collate_f0_bins: misaligned pointer (4 bytes; plan and bins 8 bytes)");
    NSG_REQUIRE((int64_t)B * T < (1ll << 31), NSG_E_INVALID, "nsg_collate_f0_bins: B * T must stay below 2^31");
    const float lo = (float)log2((double)fmin);
    const float span = (float)log2((double)fmax) - lo;
    NSG_REQUIRE(span > 0.f, NSG_E_INVALID, "nsg_collate_f0_bins: fmin and fmax are one value in fp32 log2");
    const int Q = f0_out ? (int)nsg_cdiv((int64_t)T, 4) : (int)W;      // quads per item: the columns, or all of T where the row is copied out
    hipLaunchKernelGGL(collate_f0_bins_kernel, dim3((unsigned)nsg_cdiv((int64_t)B * Q, 256)), dim3(256), 0, (hipStream_t)stream, f0_corpus,
                       corpus_frames, plan, affine, bins, logf, f0_out, (int)B, (int)T, (int)W, Q, lo, span, (float)n_bins);
    return nsg_check_launch("collate_f0_bins_kernel");
}

}  // extern "C"
