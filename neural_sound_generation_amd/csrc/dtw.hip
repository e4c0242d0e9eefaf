// Mel cepstra and dynamic time warping: the two kernels behind audio.mel_cepstral_distortion (evaluate.test_conversion).
//
// mel_cepstra_kernel: one workgroup owns 64 frames of one clip.  The mel tile [n_mels][64] is loaded along t (lane = frame: whole
// 256-byte row segments of the mel-major input, no transpose pass) into LDS, and so is the table, band-major; a wave forms 4
// coefficients of the 64 frames at a time (lane = frame again; a band's 4 table values are one 16-byte read at a wave-uniform
// address, a broadcast), one fp32 chain per output in the header's order; the 64 x K results go through an LDS tile so that the
// frame-major output leaves as one contiguous run.
//
// dtw_kernel: D(i, j) depends on its left, upper and upper-left neighbours, so the cells of one anti-diagonal are independent
// and nothing else is.  One wave per pair, one pair per workgroup (the LDS a pair needs, below, and not the wave count, bounds
// how many pairs share a CU; a workgroup of one wave has no barrier to wait at).  Lane l owns DTW_STRIP adjacent columns of b and
// walks a's rows one row behind lane l - 1: at step s it is on row s - l, so the wave sweeps an anti-diagonal band.  A lane keeps
// D and n of its strip for the previous row in registers; its left neighbours D(i, first - 1) and D(i - 1, first - 1) are lane
// l - 1's last column of the previous step (one lane shift a step; the second is the value shifted in a step earlier).
//   LDS (floats):  sb [K4][DTW_BS]  b's block of 256 columns, k-major: a lane reads its 4 columns of one k as 16 bytes, the wave
//                                   1 KB contiguous; zero past len_b (never read from memory there).  K4 = K rounded up to 4,
//                                   the rows past K zero here and in sa: the distance loop takes 4 coefficients at a time, its
//                                   8 LDS reads issued together, and (0 - 0)^2 added to a sum leaves its bits as they are
//                  sa [K4][DTW_AS]  a ring of 128 rows of a, k-major, filled 64 rows at a time every 64 steps (the rows s - 63 ..
//                                   s in flight lie in two adjacent chunks); lanes read consecutive addresses
//                  bd [2][Ta]       the block's last column, D then n, for every row: lane 63 writes row i 63 steps after lane
//                                   0 of the NEXT block would read it, so one array serves both blocks
//                  fin              the path length, for the lane that walks the path back
// Sequences b longer than DTW_BLOCK columns run as successive blocks.  With a path wanted, each lane stores the predecessor
// taken at its 4 cells as one 32-bit word of the workspace ([B][Ta][Tb rounded up to 4] bytes) and lane 0 walks it back.
#include "nsg_common.h"

namespace {

constexpr int CEP_FRAMES = 64;
constexpr int CEP_THREADS = 256;
constexpr int CEP_MAX_K = 64, CEP_MAX_MELS = 128;
constexpr int CEP_BATCH = 8;                      // global loads a thread has in flight while staging

inline size_t cep_lds_bytes(int n_mels, int K)
{
    const int K4 = (K + 3) / 4 * 4;
    return ((size_t)n_mels * (K4 + 4) + (size_t)n_mels * CEP_FRAMES + (size_t)CEP_FRAMES * (K | 1)) * sizeof(float);
}

__global__ __launch_bounds__(CEP_THREADS) void mel_cepstra_kernel(const float *__restrict__ mel, const int32_t *__restrict__ frames,
                                                                   const float *__restrict__ table, float *__restrict__ c, int n_mels, int T,
                                                                   int K, int tiles_t, FastDiv div_k, FastDiv div_mels)
{
    extern __shared__ __attribute__((aligned(16))) float cep_lds[];
    const int K4 = (K + 3) / 4 * 4, KS = K4 + 4;        // the table band-major, 4 coefficients of one band = one 16-byte broadcast read
    const int S = K | 1;                                // odd row stride of the result tile: lanes along t meet different banks
    float *tab = cep_lds;                               // [n_mels][KS], zero for K <= k < K4
    float *tile = tab + n_mels * KS;                    // [n_mels][64]
    float *res = tile + n_mels * CEP_FRAMES;            // [64][S]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / tiles_t, t0 = (blockIdx.x - b * tiles_t) * CEP_FRAMES;
    int nf = frames ? frames[b] : T;
    nf = nf < 0 ? 0 : (nf > T ? T : nf);
    const int valid = nf - t0 < 0 ? 0 : (nf - t0 > CEP_FRAMES ? CEP_FRAMES : nf - t0);    // frames of this tile below the clip's count
    const int width = T - t0 > CEP_FRAMES ? CEP_FRAMES : T - t0;                          // frames of this tile inside the tensor
    const float *mb = mel + (int64_t)b * n_mels * T + t0;
    // Both stagings issue CEP_BATCH loads before the first LDS store waits for one: a load a trip costs a memory latency a row.
    for (int e0 = tid; e0 < K * n_mels; e0 += CEP_THREADS * CEP_BATCH) {           // the table as the contiguous run it is
        float v[CEP_BATCH];
#pragma unroll
        for (int u = 0; u < CEP_BATCH; ++u) {
            const int e = e0 + u * CEP_THREADS;
            v[u] = table[e < K * n_mels ? e : 0];
        }
#pragma unroll
        for (int u = 0; u < CEP_BATCH; ++u) {
            const int e = e0 + u * CEP_THREADS, k = nsg_div(e, div_mels);
            if (e < K * n_mels) tab[(e - k * n_mels) * KS + k] = v[u];
        }
    }
    for (int j = tid; j < n_mels; j += CEP_THREADS)
        for (int k = K; k < K4; ++k) tab[j * KS + k] = 0.f;
    const bool live = lane < valid;
    for (int jb = wave; jb < n_mels; jb += CEP_THREADS / 64 * CEP_BATCH) {           // rows jb, jb + 4, ...: 256 bytes of one band each
        float v[CEP_BATCH];
#pragma unroll
        for (int u = 0; u < CEP_BATCH; ++u) {
            const int j = jb + u * (CEP_THREADS / 64);
            v[u] = live ? mb[(int64_t)(j < n_mels ? j : n_mels - 1) * T + lane] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CEP_BATCH; ++u) {
            const int j = jb + u * (CEP_THREADS / 64);
            if (j < n_mels) tile[j * CEP_FRAMES + lane] = v[u];
        }
    }
    __syncthreads();
    for (int kb = wave * 4; kb < K; kb += CEP_THREADS / 64 * 4) {       // a wave forms 4 coefficients of its 64 frames at a time
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < n_mels; ++j) {
            const float m = tile[j * CEP_FRAMES + lane];
            const v4f t = *reinterpret_cast<const v4f *>(tab + j * KS + kb);
            acc[0] = acc[0] + m * t.x;
            acc[1] = acc[1] + m * t.y;
            acc[2] = acc[2] + m * t.z;
            acc[3] = acc[3] + m * t.w;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (kb + u < K) res[lane * S + kb + u] = lane < valid ? acc[u] : 0.f;
    }
    __syncthreads();
    float *cb = c + ((int64_t)b * T + t0) * K;
    for (int e = tid; e < width * K; e += CEP_THREADS) {
        const int t = nsg_div(e, div_k);
        cb[e] = res[t * S + (e - t * K)];
    }
}

constexpr int DTW_STRIP = 4;                      // columns of b a lane owns
constexpr int DTW_BLOCK = 64 * DTW_STRIP;         // columns one sweep of the wave covers
constexpr int DTW_BS = DTW_BLOCK + 4;             // row stride of sb: 16-byte aligned rows, the staging stores 8 banks apart
constexpr int DTW_RING = 128, DTW_AS = DTW_RING + 1;   // rows of a in LDS; the odd stride spreads the staging stores over the banks
constexpr int DTW_MAX_K = 64;
static_assert(DTW_BLOCK == NSG_DTW_BLOCK_COLS, "nsg.h states the block width");

constexpr int DTW_KG = 4;                         // coefficients per group of the distance loop: sb and sa hold zero rows up to a multiple
inline int dtw_k_rows(int K) { return (K + DTW_KG - 1) / DTW_KG * DTW_KG; }
inline size_t dtw_lds_bytes(int K, int Ta) { return ((size_t)dtw_k_rows(K) * (DTW_BS + DTW_AS) + 2 * (size_t)Ta + 4) * sizeof(float); }

// nsg_dtw's workspace: the predecessor taken at each cell, one byte each, [B][Ta][Tb rounded up to a multiple of 4] (0: (i-1, j-1),
// 1: (i-1, j), 2: (i, j-1)); nothing when no path is wanted
struct DtwLayout { uint8_t *dir; size_t bytes; };
inline DtwLayout dtw_layout(void *ws, int B, int Ta, int Tb, int want_path)
{
    NsgCarver c(ws);
    return {c.take<uint8_t>(want_path ? nsg_align_up((size_t)B * Ta * nsg_align_up((size_t)Tb, 4), 256) : 0), c.off};
}

__global__ __launch_bounds__(64) void dtw_kernel(const float *__restrict__ a, const float *__restrict__ b, const int32_t *__restrict__ len_a,
                                                 const int32_t *__restrict__ len_b, float *__restrict__ cost, int32_t *__restrict__ steps,
                                                 int32_t *__restrict__ path, uint8_t *__restrict__ dir, int Ta, int Tb, int Tb4, int K,
                                                 FastDiv div_k)
{
    extern __shared__ __attribute__((aligned(16))) float dtw_lds[];
    const int KR = (K + DTW_KG - 1) / DTW_KG * DTW_KG;  // rows K .. KR - 1 of sb and sa are zero: (0 - 0)^2 added to a sum leaves its bits
    float *sb = dtw_lds;
    float *sa = sb + KR * DTW_BS;
    float *bd_d = sa + KR * DTW_AS;
    int *bd_n = reinterpret_cast<int *>(bd_d + Ta);
    int *fin = bd_n + Ta;
    const int pair = blockIdx.x, lane = threadIdx.x;
    int la = len_a[pair], lb = len_b[pair];
    la = la < 1 ? 1 : (la > Ta ? Ta : la);              // the caller's to get right (nsg.h); clamped so that no access leaves a buffer
    lb = lb < 1 ? 1 : (lb > Tb ? Tb : lb);
    const float *A = a + (int64_t)pair * Ta * K, *Bm = b + (int64_t)pair * Tb * K;
    uint8_t *dr = dir ? dir + (int64_t)pair * Ta * Tb4 : nullptr;
    const float INF = __builtin_inff();
    for (int e = K * DTW_BS + lane; e < KR * DTW_BS; e += 64) sb[e] = 0.f;
    for (int e = K * DTW_AS + lane; e < KR * DTW_AS; e += 64) sa[e] = 0.f;

    for (int c0 = 0; c0 < lb; c0 += DTW_BLOCK) {
        const int ncols = lb - c0 < DTW_BLOCK ? lb - c0 : DTW_BLOCK;
        const int nl = (ncols + DTW_STRIP - 1) / DTW_STRIP;          // lanes with a column below len_b
        __syncthreads();                                             // the block before is done with sb
        for (int e = lane; e < DTW_BLOCK * K; e += 64) {             // b[c0 .. c0 + 256) as one contiguous run; zero past len_b
            const int col = nsg_div(e, div_k), k = e - col * K;
            sb[k * DTW_BS + col] = col < ncols ? Bm[(int64_t)c0 * K + e] : 0.f;
        }
        float pd[DTW_STRIP], left_prev_d = INF;                      // D(i-1, .) of the strip; D(i-1, first-1)
        int pn[DTW_STRIP], left_prev_n = 0;
#pragma unroll
        for (int w = 0; w < DTW_STRIP; ++w) { pd[w] = INF; pn[w] = 0; }
        const int j0 = c0 + DTW_STRIP * lane;
        const int nsteps = la + nl - 1;
        for (int s = 0; s < nsteps; ++s) {
            if ((s & 63) == 0 && s < la) {                           // rows s .. s + 63 of a into their half of the ring
                __syncthreads();
                const int slot = (s & 64), rows = la - s < 64 ? la - s : 64;
                for (int e = lane; e < rows * K; e += 64) {
                    const int r = nsg_div(e, div_k), k = e - r * K;
                    sa[k * DTW_AS + slot + r] = A[(int64_t)s * K + e];
                }
                __syncthreads();
            }
            const int i = s - lane;
            const bool act = i >= 0 && i < la && lane < nl;
            // D(i, first-1), n(i, first-1): lane l-1's last column after its previous step (row i); the block before's for lane 0
            float left_d = __shfl_up(pd[DTW_STRIP - 1], 1);
            int left_n = __shfl_up(pn[DTW_STRIP - 1], 1);
            if (lane == 0) {
                const bool have = c0 > 0 && act;
                left_d = have ? bd_d[have ? i : 0] : INF;
                left_n = have ? bd_n[have ? i : 0] : 0;
            }
            const float *pa = sa + (act ? (i & (DTW_RING - 1)) : 0);
            const float *pb = sb + DTW_STRIP * lane;
            float acc[DTW_STRIP] = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < KR; k += DTW_KG) {                   // a group's LDS reads are issued together, then its arithmetic
                float av[DTW_KG];
                v4f bv[DTW_KG];
#pragma unroll
                for (int u = 0; u < DTW_KG; ++u) {
                    av[u] = pa[(k + u) * DTW_AS];
                    bv[u] = *reinterpret_cast<const v4f *>(pb + (k + u) * DTW_BS);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < DTW_KG; ++u) {
                    const float t0 = av[u] - bv[u].x, t1 = av[u] - bv[u].y, t2 = av[u] - bv[u].z, t3 = av[u] - bv[u].w;
                    acc[0] = acc[0] + t0 * t0;
                    acc[1] = acc[1] + t1 * t1;
                    acc[2] = acc[2] + t2 * t2;
                    acc[3] = acc[3] + t3 * t3;
                }
            }
            if (act) {
                float diag_d = left_prev_d, side_d = left_d;
                int diag_n = left_prev_n, side_n = left_n;
                unsigned dirs = 0;
                const int w_end = lb - 1 - j0;                       // the strip's column that is b's last, if it has it
                float end_d = 0.f;
                int end_n = 0;
#pragma unroll
                for (int w = 0; w < DTW_STRIP; ++w) {
                    const float d = sqrtf(acc[w]);
                    const float up_d = pd[w];
                    const int up_n = pn[w];
                    float best = diag_d;
                    int bn = diag_n;
                    unsigned dc = 0;
                    if (up_d < best) { best = up_d; bn = up_n; dc = 1; }
                    if (side_d < best) { best = side_d; bn = side_n; dc = 2; }
                    const bool origin = i == 0 && j0 + w == 0;
                    const float D = origin ? d : best + d;
                    const int n = origin ? 1 : bn + 1;
                    diag_d = up_d; diag_n = up_n;
                    side_d = D; side_n = n;
                    pd[w] = D; pn[w] = n;
                    dirs |= dc << (8 * w);
                    end_d = w == w_end ? D : end_d;
                    end_n = w == w_end ? n : end_n;
                }
                left_prev_d = left_d; left_prev_n = left_n;
                if (i == la - 1 && w_end >= 0 && w_end < DTW_STRIP) { cost[pair] = end_d; steps[pair] = end_n; fin[0] = end_n; }
                if (dr) *reinterpret_cast<unsigned *>(dr + (int64_t)i * Tb4 + j0) = dirs;
                if (lane == 63) { bd_d[i] = pd[DTW_STRIP - 1]; bd_n[i] = pn[DTW_STRIP - 1]; }
            }
        }
    }
    if (path && dr) {
        __syncthreads();                                             // the wave's stores of dir and fin are visible to lane 0
        if (lane == 0) {
            int32_t *P = path + (int64_t)pair * (Ta + Tb - 1) * 2;
            int i = la - 1, j = lb - 1;
            for (int p = fin[0] - 1; p >= 0 && i >= 0 && j >= 0; --p) {
                P[2 * p] = i; P[2 * p + 1] = j;
                const unsigned dc = dr[(int64_t)i * Tb4 + j];
                if (dc != 2) --i;
                if (dc != 1) --j;
            }
        }
    }
}

}  // namespace

extern "C" {

int nsg_mel_cepstra(const float *mel, const int32_t *frames, const float *table, float *c, int32_t B, int32_t n_mels, int32_t T,
                    int32_t K, void *stream)
{
    NSG_REQUIRE(mel && table && c, NSG_E_INVALID, "nsg_mel_cepstra: null pointer");
    NSG_REQUIRE(B >= 1 && T >= 1, NSG_E_INVALID, "nsg_mel_cepstra: bad size (B = %d, T = %d)", B, T);
    NSG_REQUIRE(K >= 1 && K <= CEP_MAX_K, NSG_E_UNSUPPORTED, "nsg_mel_cepstra: K = %d outside [1, %d]", K, CEP_MAX_K);
    NSG_REQUIRE(n_mels >= 1 && n_mels <= CEP_MAX_MELS, NSG_E_UNSUPPORTED, "nsg_mel_cepstra: n_mels = %d outside [1, %d]", n_mels, CEP_MAX_MELS);
    const int tiles_t = (int)nsg_cdiv(T, CEP_FRAMES);
    NSG_REQUIRE((int64_t)B * tiles_t < 0x7fffffff, NSG_E_INVALID, "nsg_mel_cepstra: too many frames (B * ceil(T / 64) >= 2^31)");
    const size_t lds = cep_lds_bytes(n_mels, K);                // 30 KB at 80 bands and 13 coefficients, 82 KB at 128 and 64
    static LdsOptIn once;
    if (const int rc = nsg_lds_opt_in(once, {reinterpret_cast<const void *>(&mel_cepstra_kernel)}, cep_lds_bytes(CEP_MAX_MELS, CEP_MAX_K), "nsg_mel_cepstra"))
        return rc;
    hipLaunchKernelGGL(mel_cepstra_kernel, dim3((unsigned)(B * tiles_t)), dim3(CEP_THREADS), lds, (hipStream_t)stream, mel, frames, table, c,
                       n_mels, T, K, tiles_t, nsg_fastdiv((uint32_t)K), nsg_fastdiv((uint32_t)n_mels));
    return nsg_check_launch("mel_cepstra_kernel");
}

size_t nsg_dtw_workspace_bytes(int32_t B, int32_t Ta, int32_t Tb, int32_t want_path)
{
    if (B < 1 || Ta < 1 || Tb < 1 || Ta > NSG_DTW_MAX_FRAMES || Tb > NSG_DTW_MAX_FRAMES) return 0;
    return dtw_layout(nullptr, B, Ta, Tb, want_path).bytes;
}

int nsg_dtw(const float *a, const float *b, const int32_t *len_a, const int32_t *len_b, float *cost, int32_t *steps, int32_t *path,
            int32_t B, int32_t Ta, int32_t Tb, int32_t K, void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(a && b && len_a && len_b && cost && steps, NSG_E_INVALID, "nsg_dtw: null pointer");
    NSG_REQUIRE(B >= 1, NSG_E_INVALID, "nsg_dtw: B = %d < 1", B);
    NSG_REQUIRE(K >= 1 && K <= DTW_MAX_K, NSG_E_UNSUPPORTED, "nsg_dtw: K = %d outside [1, %d]", K, DTW_MAX_K);
    NSG_REQUIRE(Ta >= 1 && Ta <= NSG_DTW_MAX_FRAMES && Tb >= 1 && Tb <= NSG_DTW_MAX_FRAMES, NSG_E_UNSUPPORTED,
                "nsg_dtw: sequence lengths (Ta = %d, Tb = %d) outside [1, %d]", Ta, Tb, NSG_DTW_MAX_FRAMES);
    const DtwLayout L = dtw_layout(workspace, B, Ta, Tb, path != nullptr);
    NSG_REQUIRE(!path || (workspace && workspace_bytes >= L.bytes), NSG_E_WORKSPACE, "nsg_dtw: workspace too small");
    static LdsOptIn once;
    if (const int rc = nsg_lds_opt_in(once, {reinterpret_cast<const void *>(&dtw_kernel)}, dtw_lds_bytes(DTW_MAX_K, NSG_DTW_MAX_FRAMES), "nsg_dtw"))
        return rc;
    hipLaunchKernelGGL(dtw_kernel, dim3((unsigned)B), dim3(64), dtw_lds_bytes(K, Ta), (hipStream_t)stream, a, b, len_a, len_b, cost, steps,
                       path, path ? L.dir : nullptr, Ta, Tb, (int)nsg_align_up((size_t)Tb, 4), K, nsg_fastdiv((uint32_t)K));
    return nsg_check_launch("dtw_kernel");
}

}  // extern "C"
