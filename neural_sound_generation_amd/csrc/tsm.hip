// Time-scale modification and noise augmentation of waveforms: the kernels behind audio.tempo (and with audio.resample,
// audio.pitch_shift) and audio.mix_noise.  include/nsg.h states the arithmetic and its order; this file is how it is laid on the
// machine.
//
// tsm_chain_kernel (nsg_audio_tempo, first launch): one workgroup of 256 lanes per clip walks the segments m = 1 .. M - 1 in
// order.  A step compares the O tail samples behind the previous segment with the W candidate positions of this one: W * O
// subtract-square-add triples out of W + O - 1 samples, VALU work fed from LDS.  The loop is nsg_ssd_run (nsg_wave.h), the
// function f0_difference (csrc/f0.hip) calls too, here with every tail (O mod 4 is anything) and compiled with -fno-slp-vectorize
// as that header asks.  A lane owns RUN adjacent candidates delta = RUN g .. RUN g + RUN - 1 (RUN = 2, 4 or 8: the
// least that lets 256 lanes cover W, so that the four SIMDs share the work): four j cost one read of the next four window samples
// (consecutive lanes RUN floats apart) and one 16-byte read of the tail at an address all lanes share (a broadcast), for 4 RUN
// triples.  One fp32 chain per candidate over j in order.  The argmin is the integer minimum of bits(d) << 32 | delta (d >= 0: its
// bits order as integers; equal d: the smallest delta): nsg_wave_min (nsg_reduce.h) inside each wave, then one LDS atomic per wave
// -- exact and order-free.
//   The chain over m runs only through delta*: the window x[n_m .. n_m + W + O - 1) does not depend on earlier steps, and the tail
// x[q_{m-1} + Ho ..) lies inside x[n_{m-1} + Ho .. n_{m-1} + Ho + W + O - 1), which does not either.  So both ranges of step
// m + 1 are loaded from global memory into registers BEFORE step m's search and stored to LDS after it: no global load waits on
// the step before it; what is sequential is an LDS-to-LDS copy of the tail (to a 16-byte aligned row), the search and three
// barriers.
//   LDS (floats):  win  [stride]  x[n_m + i], zero outside the clip and for i >= W + O - 1
//                  twin [stride]  x[n_{m-1} + Ho + i], likewise: the tail is twin[delta*_{m-1} ..]
//                  tail [O4 + 4]  the tail, zero past O (O4 = O rounded up to 4)
//                  key            the 64-bit minimum
//   stride = W + O + 2 RUN + 8 rounded up to 4 covers every read of an active lane (tsm_stride).
// The positions q_m go to `positions` (or, when the caller does not want them, to the workspace); tsm_render_kernel (second
// launch) forms the output from them, a thread per sample, coalesced: it is the cheap part and runs over (clip, tile of 1024).
//
// nsg_audio_mix_noise: mix_energy_kernel (a block per NSG_MIX_PARTIAL = 4096 samples of one clip: the two fp64 sums of squares,
// thread partials then nsg_block_sum_four_walk), mix_scale_kernel (a wave per clip: nsg_wave_close_sum over the partials, then s),
// mix_apply_kernel (two reads and one write a sample, four consecutive samples a thread, 16-byte accesses where they are aligned).
#include "nsg_common.h"
#include "nsg_reduce.h"
#include "nsg_wave.h"

namespace {

constexpr int TSM_THREADS = 256;
constexpr int TSM_MAX_O = 2048, TSM_MAX_S = 8192, TSM_MAX_W = 2048;
constexpr int TSM_MAX_RUN = 8;
constexpr int TSM_MAX_STRIDE = (TSM_MAX_W + TSM_MAX_O + 2 * TSM_MAX_RUN + 8 + 3) / 4 * 4;
constexpr int TSM_NPF = (TSM_MAX_STRIDE + TSM_THREADS - 1) / TSM_THREADS;     // floats of a range a lane carries in registers
constexpr int TSM_TILE = 1024;                                                // output samples of a render block

inline int tsm_run(int W) { return W <= 2 * TSM_THREADS ? 2 : (W <= 4 * TSM_THREADS ? 4 : 8); }
// floats of win / twin: an active lane (RUN g < W) reads up to win[RUN g + O4 + RUN + 3], O4 <= O + 3
inline int tsm_stride(int O, int W, int run) { return (W + O + 2 * run + 8 + 3) / 4 * 4; }
inline int tsm_segments(int L_out, int Ho) { return (int)nsg_cdiv(L_out, Ho); }

// a clip's lengths and factor as the kernels use them: clamped, so that no access leaves a buffer (nsg.h)
struct TsmClip {
    int len, out_len, M;
    double factor;
};
__device__ __forceinline__ TsmClip tsm_clip(const int32_t *lengths, const double *factor, const int32_t *out_lengths, int b, int L, int L_out,
                                            int Ho)
{
    TsmClip c;
    c.len = nsg_clip_len(lengths, b, L);
    const int ol = out_lengths[b];
    c.out_len = ol < 0 ? 0 : (ol > L_out ? L_out : ol);
    c.M = (c.out_len + Ho - 1) / Ho;
    c.factor = factor[b];
    return c;
}
// n_m = floor((double)(m Ho) * factor), one fp64 product; anything not in [0, len) -- only a factor or an out_length that breaks
// the caller's precondition gives one -- is taken as len, where every sample read is zero
__device__ __forceinline__ int64_t tsm_nominal(int m, int Ho, const TsmClip &c)
{
    const double p = (double)((int64_t)m * Ho) * c.factor;
    return (p >= 0.0 && p < (double)c.len) ? (int64_t)p : (int64_t)c.len;
}

// the range x[base + i], i = tid, tid + 256, ... < stride, zero outside the clip and for i >= n: global -> registers ...
__device__ __forceinline__ void tsm_fetch(float (&r)[TSM_NPF], const float *__restrict__ xb, int64_t base, int n, int len, int npf, int tid)
{
#pragma unroll
    for (int k = 0; k < TSM_NPF; ++k) {
        if (k < npf) {
            const int i = k * TSM_THREADS + tid;
            r[k] = nsg_clip_at(xb, base + i, len, i < n);
        }
    }
}
// ... registers -> LDS
__device__ __forceinline__ void tsm_commit(float *dst, const float (&r)[TSM_NPF], int stride, int npf, int tid)
{
#pragma unroll
    for (int k = 0; k < TSM_NPF; ++k) {
        if (k < npf) {
            const int i = k * TSM_THREADS + tid;
            if (i < stride) dst[i] = r[k];
        }
    }
}

// d(delta) of the lane's run, folded to the lane's least key bits(d) << 32 | delta over delta < W
template <int RUN>
__device__ __forceinline__ unsigned long long tsm_search(const float *win, const float *tail, int O, int W, int g)
{
    float acc[RUN];                                    // (O mod 4 != 0: both rows are long enough for the tail's reads)
    nsg_ssd_run<RUN, 0b1111>(acc, win + RUN * g, tail, O);
    unsigned long long best = ~0ull;
#pragma unroll
    for (int r = 0; r < RUN; ++r) {
        const int delta = RUN * g + r;
        const unsigned long long key = (unsigned long long)nsg_fbits(acc[r]) << 32 | (unsigned)delta;
        if (delta < W && key < best) best = key;
    }
    return best;
}

template <int RUN>
__global__ __launch_bounds__(TSM_THREADS) void tsm_chain_kernel(const float *__restrict__ wav, const int32_t *__restrict__ lengths,
                                                                const double *__restrict__ factor, const int32_t *__restrict__ out_lengths,
                                                                int32_t *__restrict__ q, int L, int L_out, int S, int O, int W, int M_max,
                                                                int stride)
{
    extern __shared__ __attribute__((aligned(16))) float tsm_lds[];
    float *win = tsm_lds, *twin = win + stride, *tail = twin + stride;
    const int O4 = (O + 3) / 4 * 4;
    unsigned long long *key = reinterpret_cast<unsigned long long *>(tail + O4 + 4);     // 16-byte aligned: every section is a multiple of 4 floats
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Ho = S - O;
    const TsmClip c = tsm_clip(lengths, factor, out_lengths, b, L, L_out, Ho);
    const float *xb = wav + (int64_t)b * L;
    int32_t *qb = q + (int64_t)b * M_max;
    for (int m = c.M + tid; m < M_max; m += TSM_THREADS) qb[m] = -1;
    if (c.M == 0) return;
    if (tid == 0) qb[0] = 0;
    if (c.M == 1) return;                              // (uniform over the workgroup)

    const int n = W + O - 1;                           // samples of a range
    const int npf = (stride + TSM_THREADS - 1) / TSM_THREADS;
    const int g = tid;
    const bool act = RUN * g < W;
    float rw[TSM_NPF], rt[TSM_NPF];
    tsm_fetch(rw, xb, tsm_nominal(1, Ho, c), n, c.len, npf, tid);
    tsm_fetch(rt, xb, (int64_t)Ho, n, c.len, npf, tid);                                  // q_0 = 0: n_0 + Ho
    tsm_commit(win, rw, stride, npf, tid);
    tsm_commit(twin, rt, stride, npf, tid);
    for (int i = tid; i < O4 + 4; i += TSM_THREADS) tail[i] = 0.f;
    __syncthreads();
    int dprev = 0;                                     // delta* of the step before
    for (int m = 1; m < c.M; ++m) {
        for (int j = tid; j < O; j += TSM_THREADS) tail[j] = twin[dprev + j];
        if (tid == 0) *key = ~0ull;
        __syncthreads();
        const int64_t nm = tsm_nominal(m, Ho, c);
        if (m + 1 < c.M) {                             // step m + 1's ranges, in flight while this step is searched
            tsm_fetch(rw, xb, tsm_nominal(m + 1, Ho, c), n, c.len, npf, tid);
            tsm_fetch(rt, xb, nm + Ho, n, c.len, npf, tid);
        }
        const unsigned long long best = nsg_wave_min(act ? tsm_search<RUN>(win, tail, O, W, g) : ~0ull);
        if ((tid & 63) == 0) atomicMin(key, best);
        __syncthreads();
        dprev = (int)(unsigned)*key;
        if (tid == 0) qb[m] = (int32_t)(nm + dprev);
        if (m + 1 < c.M) {
            tsm_commit(win, rw, stride, npf, tid);
            tsm_commit(twin, rt, stride, npf, tid);
        }
        __syncthreads();
    }
}

// out[b][k] from the positions: a thread per sample of a tile of TSM_TILE
__global__ __launch_bounds__(256) void tsm_render_kernel(const float *__restrict__ wav, const int32_t *__restrict__ lengths,
                                                         const double *__restrict__ factor, const int32_t *__restrict__ out_lengths,
                                                         const int32_t *__restrict__ q, float *__restrict__ out, int L, int L_out, int S, int O,
                                                         int M_max, int tiles, FastDiv div_ho)
{
    const int b = blockIdx.x / tiles, k0 = (blockIdx.x - b * tiles) * TSM_TILE;
    const int Ho = S - O;
    const TsmClip c = tsm_clip(lengths, factor, out_lengths, b, L, L_out, Ho);
    const float *xb = wav + (int64_t)b * L;
    const int32_t *qb = q + (int64_t)b * M_max;
    float *ob = out + (int64_t)b * L_out;
    const float fO = (float)O;
    for (int k = k0 + threadIdx.x; k < k0 + TSM_TILE && k < L_out; k += 256) {
        float v = 0.f;
        if (k < c.out_len) {
            const int m = nsg_div(k, div_ho), j = k - m * Ho;
            v = nsg_clip_at(xb, (int64_t)qb[m] + j, c.len);
            if (m >= 1 && j < O) {
                const float a = nsg_clip_at(xb, (int64_t)qb[m - 1] + Ho + j, c.len);
                const float w = (float)j / fO;
                const float diff = v - a;
                const float sc = w * diff;
                v = a + sc;
            }
        }
        ob[k] = v;
    }
}

// ---- nsg_audio_mix_noise ---------------------------------------------------------------------------------------------------------
constexpr int MIX_PARTIAL = NSG_MIX_PARTIAL;           // samples of a partial: 16 a thread
static_assert(MIX_PARTIAL % 256 == 0, "a thread's samples are 256 apart");

struct MixClip {
    int len;
    unsigned off;
};
__device__ __forceinline__ MixClip mix_clip(const int32_t *lengths, const int32_t *offset, int b, int L, int Ln)
{
    MixClip c;
    c.len = nsg_clip_len(lengths, b, L);
    const int o = offset[b];
    c.off = (unsigned)(o < 0 ? 0 : (o > Ln - 1 ? Ln - 1 : o));      // the caller's to get right (nsg.h); clamped so that no read leaves noise
    return c;
}

// partial [2][B][NP] fp64: the sums of squares of the clips' samples, then of the noise under them, per MIX_PARTIAL samples
__global__ __launch_bounds__(256) void mix_energy_kernel(const float *__restrict__ wav, const int32_t *__restrict__ lengths,
                                                         const float *__restrict__ noise, const int32_t *__restrict__ offset,
                                                         double *__restrict__ partial, int L, int Ln, int NP)
{
    const int b = blockIdx.x / NP, p = blockIdx.x - b * NP;
    const MixClip c = mix_clip(lengths, offset, b, L, Ln);
    const float *xb = wav + (int64_t)b * L;
    const unsigned uLn = (unsigned)Ln, step = 256u % uLn;
    const int i0 = p * MIX_PARTIAL + threadIdx.x;
    unsigned r = (c.off + (unsigned)i0) % uLn;         // off < Ln < 2^31 and i0 < 2^31: no wrap
    double ex = 0.0, en = 0.0;
#pragma unroll 4
    for (int k = 0; k < MIX_PARTIAL / 256; ++k) {
        const int i = i0 + 256 * k;
        if (i < c.len) {
            const double x = (double)xb[i], v = (double)noise[r];
            ex += x * x;
            en += v * v;
        }
        r += step;
        r = r >= uLn ? r - uLn : r;
    }
    nsg_block_sum_four_walk(ex, partial);                               // to [blockIdx.x] = [b][p]
    __syncthreads();
    nsg_block_sum_four_walk(en, partial + (int64_t)gridDim.x);
}

// a wave per clip: the partials' totals, then s = (float)(level * sqrt(E_x / E_n))
__global__ __launch_bounds__(64) void mix_scale_kernel(const double *__restrict__ partial, const int32_t *__restrict__ lengths,
                                                       const float *__restrict__ level, float *__restrict__ scale, double *__restrict__ energy,
                                                       int L, int NP)
{
    __shared__ double tot[2];
    const int b = blockIdx.x;
    const double *pb = partial + (int64_t)b * NP;
    nsg_wave_close_sum(pb, NP, [&](double t) { tot[0] = t; });
    __syncthreads();
    nsg_wave_close_sum(pb + (int64_t)gridDim.x * NP, NP, [&](double t) { tot[1] = t; });
    if (threadIdx.x == 0) {
        const double ex = tot[0], en = tot[1];
        const int len = nsg_clip_len(lengths, b, L);
        float s = 0.f;
        if (len > 0 && en != 0.0) {
            const double ratio = ex / en;
            const double root = sqrt(ratio);
            const double prod = (double)level[b] * root;
            s = (float)prod;
        }
        scale[b] = s;
        if (energy) { energy[2 * b] = ex; energy[2 * b + 1] = en; }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void mix_apply_kernel(const float *__restrict__ wav, const int32_t *__restrict__ lengths,
                                                        const float *__restrict__ noise, const float *__restrict__ gain,
                                                        const float *__restrict__ scale, const int32_t *__restrict__ offset,
                                                        float *__restrict__ out, int L, int Ln, int tiles)
{
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const MixClip c = mix_clip(lengths, offset, b, L, Ln);
    const float *xb = wav + (int64_t)b * L;
    float *ob = out + (int64_t)b * L;
    const float gn = gain[b], s = scale[b];
    const unsigned uLn = (unsigned)Ln;
    const int i0 = t * 1024 + 4 * threadIdx.x;
    if (i0 >= L) return;
    float x[4], y[4];
    const bool whole = i0 + 4 <= L;
    if (VEC && whole && i0 + 4 <= c.len) {
        const v4f v = *reinterpret_cast<const v4f *>(xb + i0);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = nsg_clip_at(xb, i0 + e, c.len);
    }
    unsigned r = (c.off + (unsigned)i0) % uLn;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float gx = gn * x[e];
        const float sv = s * noise[r];
        const float sum = gx + sv;
        y[e] = i0 + e < c.len ? sum : 0.f;
        r = r + 1 == uLn ? 0 : r + 1;
    }
    if (VEC && whole) {
        const v4f v = {y[0], y[1], y[2], y[3]};
        *reinterpret_cast<v4f *>(ob + i0) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < L) ob[i0 + e] = y[e];
    }
}

// the workspace of nsg_audio_mix_noise: partial [2][B][NP] fp64 | scale [B] fp32
struct MixLayout { double *partial; float *scale; size_t bytes; };
inline MixLayout mix_layout(void *ws, int B, int L)
{
    const size_t NP = (size_t)nsg_cdiv(L, MIX_PARTIAL);
    NsgCarver c(ws);
    MixLayout m = {c.take<double>(nsg_align_up((size_t)B * 2 * NP * sizeof(double), 256)), c.take<float>(nsg_align_up((size_t)B * sizeof(float), 256)), 0};
    m.bytes = c.off;
    return m;
}

}  // namespace

extern "C" {

size_t nsg_audio_tempo_workspace_bytes(int32_t B, int32_t L_out, int32_t S, int32_t O)
{
    if (B <= 0 || L_out <= 0 || O <= 0 || S <= O) return 0;
    return nsg_align_up((size_t)B * (size_t)tsm_segments(L_out, S - O) * sizeof(int32_t), 256);
}

int nsg_audio_tempo(const float *wav, const int32_t *lengths, const double *factor, const int32_t *out_lengths, float *out, int32_t *positions,
                    int32_t B, int32_t L, int32_t L_out, int32_t S, int32_t O, int32_t W, void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(wav && factor && out_lengths && out, NSG_E_INVALID, "nsg_audio_tempo: null pointer");
    NSG_REQUIRE(B >= 1 && L >= 1 && L_out >= 1, NSG_E_INVALID, "nsg_audio_tempo: non-positive size (B = %d, L = %d, L_out = %d)", B, L, L_out);
    NSG_REQUIRE(O >= 1 && O <= TSM_MAX_O, NSG_E_UNSUPPORTED, "nsg_audio_tempo: overlap O = %d outside [1, %d]", O, TSM_MAX_O);
    NSG_REQUIRE(S >= 2 * (int64_t)O && S <= TSM_MAX_S, NSG_E_UNSUPPORTED, "nsg_audio_tempo: segment S = %d outside [2 O = %d, %d]", S, 2 * O,
                TSM_MAX_S);
    NSG_REQUIRE(W >= 1 && W <= TSM_MAX_W, NSG_E_UNSUPPORTED, "nsg_audio_tempo: search width W = %d outside [1, %d]", W, TSM_MAX_W);
    NSG_REQUIRE((int64_t)B * L_out < 0x7fffffffLL, NSG_E_UNSUPPORTED, "nsg_audio_tempo: B * L_out = %lld >= 2^31, outside the envelope",
                (long long)B * L_out);
    NSG_REQUIRE((int64_t)L + S + W < 0x7fffffffLL, NSG_E_UNSUPPORTED, "nsg_audio_tempo: L + S + W = %lld >= 2^31, outside the envelope (positions are int32)",
                (long long)L + S + W);
    const int Ho = S - O, M_max = tsm_segments(L_out, Ho);
    int32_t *q = positions;
    if (!q) {
        NSG_REQUIRE(workspace && workspace_bytes >= nsg_audio_tempo_workspace_bytes(B, L_out, S, O), NSG_E_WORKSPACE,
                    "nsg_audio_tempo: workspace too small (without positions the kernels keep them there)");
        q = reinterpret_cast<int32_t *>(workspace);
    }
    hipStream_t s = (hipStream_t)stream;
    const int run = tsm_run(W), stride = tsm_stride(O, W, run);
    const size_t lds = ((size_t)2 * stride + (O + 3) / 4 * 4 + 4 + 4) * sizeof(float);
    auto chain = run == 2 ? tsm_chain_kernel<2> : (run == 4 ? tsm_chain_kernel<4> : tsm_chain_kernel<8>);
    hipLaunchKernelGGL(chain, dim3((unsigned)B), dim3(TSM_THREADS), lds, s, wav, lengths, factor, out_lengths, q, L, L_out, S, O, W, M_max, stride);
    const int tiles = (int)nsg_cdiv(L_out, TSM_TILE);
    hipLaunchKernelGGL(tsm_render_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, s, wav, lengths, factor, out_lengths, q, out, L, L_out, S, O,
                       M_max, tiles, nsg_fastdiv((uint32_t)Ho));
    return nsg_check_launch("tsm_kernels");
}

size_t nsg_audio_mix_noise_workspace_bytes(int32_t B, int32_t L)
{
    if (B <= 0 || L <= 0) return 0;
    return mix_layout(nullptr, B, L).bytes;
}

int nsg_audio_mix_noise(const float *wav, const int32_t *lengths, const float *noise, const float *gain, const float *level, const int32_t *offset,
                        float *out, double *energy, int32_t B, int32_t L, int32_t Ln, void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(wav && noise && gain && level && offset && out, NSG_E_INVALID, "nsg_audio_mix_noise: null pointer");
    NSG_REQUIRE(B >= 1 && L >= 1 && Ln >= 1, NSG_E_INVALID, "nsg_audio_mix_noise: non-positive size (B = %d, L = %d, Ln = %d)", B, L, Ln);
    const int64_t NP = nsg_cdiv(L, MIX_PARTIAL), tiles = nsg_cdiv(L, 1024);
    NSG_REQUIRE((int64_t)B * tiles < 0x7fffffffLL, NSG_E_UNSUPPORTED, "nsg_audio_mix_noise: B * ceil(L / 1024) = %lld >= 2^31, outside the envelope",
                (long long)(B * tiles));
    NSG_REQUIRE(workspace && workspace_bytes >= nsg_audio_mix_noise_workspace_bytes(B, L), NSG_E_WORKSPACE, "nsg_audio_mix_noise: workspace too small");
    const MixLayout m = mix_layout(workspace, B, L);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mix_energy_kernel, dim3((unsigned)(B * NP)), dim3(256), 0, s, wav, lengths, noise, offset, m.partial, L, Ln, (int)NP);
    hipLaunchKernelGGL(mix_scale_kernel, dim3((unsigned)B), dim3(64), 0, s, m.partial, lengths, level, m.scale, energy, L, (int)NP);
    const bool vec = L % 4 == 0 && nsg_aligned16(wav) && nsg_aligned16(out);
    hipLaunchKernelGGL(vec ? mix_apply_kernel<true> : mix_apply_kernel<false>, dim3((unsigned)(B * tiles)), dim3(256), 0, s, wav, lengths, noise, gain,
                       m.scale, offset, out, L, Ln, (int)tiles);
    return nsg_check_launch("mix_noise_kernels");
}

}  // extern "C"
