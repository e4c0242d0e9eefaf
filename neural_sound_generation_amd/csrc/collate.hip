// The loader's batch, built on the device from a corpus that lives in HBM (data.py: ResidentMelCorpus / ResidentMelLoader).
// The corpus is the on-disk layout with the clips concatenated, [frames][n_mels] fp32, frame-major; a batch is the model's
// input, [B][n_mels][T], mel-major.  One kernel does what data.Collate does on the host for the mel case (src/dataloader.py:
// 324-434): the crop (a plan row's start and count), the zero padding to the batch's longest item, and the transpose.
//
// One workgroup owns a tile of CT_FRAMES frames x n_mels of one item.  Its source is ONE contiguous run of CT_FRAMES * n_mels
// floats, loaded coalesced (16 bytes a lane where that is legal) and written to an LDS tile whose row stride is odd
// (n_mels | 1: 81, 41, 13 dwords; 32 x 81 x 4 = 10.4 KB at 80 bands), so the transposed read -- lane = frame, ds_read_b32, banked
// on (addr / 4) % 32 -- meets 32 different banks in each half wave.  Every element of the tile is written to LDS, the zeros of
// the padding included, and every element of `out` is stored exactly once: row segments of 32 consecutive t, two 128-byte
// segments per wave instruction (or 16 bytes a lane, 8 rows per instruction, where that is legal).  A copy: HBM-bound,
// 2 x B x n_mels x T x 4 bytes of compulsory traffic.  32 frames, not 64: at the workload's 128 x 80 x 1024 a 64-frame tile
// (20.7 KB) lets 7 workgroups share a CU, 1 792 slots for 2 048 tiles, and the last 256 tiles run one to a CU; 4 096 tiles of
// 32 frames fill 8 workgroups x 256 CUs exactly twice (measured: 21.0 against 22.1 us, scripts/loader_timing.py).
#include "nsg_common.h"

namespace {

constexpr int CT_FRAMES = 32;          // frames per tile = lanes along t of one stored row segment
constexpr int CT_THREADS = 256;
constexpr int CT_MAX_MELS = 128;
constexpr int CT_MAX_BLOCKS = 1 << 16; // the grid's cap: the workgroups stride over the tiles, so B is not bound by a grid dimension

__global__ __launch_bounds__(CT_THREADS) void collate_mels_kernel(const float *__restrict__ corpus, int64_t corpus_frames, int n_mels,
                                                                   const int64_t *__restrict__ plan, int64_t n_tiles, int tiles_t, int T,
                                                                   float *__restrict__ out, FastDiv div_mels, int vec_load, int vec_store)
{
    extern __shared__ float tile[];             // [CT_FRAMES][S]: tile[r * S + m] = item's frame t0 + r, band m (zero past its count)
    const int tid = threadIdx.x, S = n_mels | 1, n_elem = CT_FRAMES * n_mels;
    for (int64_t w = blockIdx.x; w < n_tiles; w += gridDim.x) {
        const int64_t b = w / tiles_t;
        const int t0 = (int)(w - b * tiles_t) * CT_FRAMES;
        // The plan is the caller's to get right (nsg.h); whatever it holds, no access leaves either buffer: count is clamped to
        // [0, T], start to where start + t cannot overflow, and a frame outside [0, corpus_frames) reads as zero.
        int64_t start = plan[b * 3 + 1], count = plan[b * 3 + 2];
        count = count < 0 ? 0 : (count > T ? T : count);
        start = start < -((int64_t)1 << 31) ? -((int64_t)1 << 31) : (start > corpus_frames ? corpus_frames : start);
        const int64_t f0 = start + t0;                                   // corpus frame of the tile's row 0
        const int valid = count - t0 < 0 ? 0 : (count - t0 > CT_FRAMES ? CT_FRAMES : (int)(count - t0));     // rows below the item's count
        const int64_t e0 = f0 * n_mels;                                  // |f0| <= 2^31 + corpus_frames: no overflow; used only under the guards below
        if (vec_load) {                                                  // n_mels % 4 == 0: a lane's 4 floats lie in one frame
            for (int e = tid * 4; e < n_elem; e += CT_THREADS * 4) {
                const int r = nsg_div(e, div_mels), m = e - r * n_mels;
                const int64_t f = f0 + r;
                v4f v = {0.f, 0.f, 0.f, 0.f};
                if (r < valid && f >= 0 && f < corpus_frames) v = *reinterpret_cast<const v4f *>(corpus + e0 + e);
                float *d = tile + r * S + m;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        } else {
            for (int e = tid; e < n_elem; e += CT_THREADS) {
                const int r = nsg_div(e, div_mels), m = e - r * n_mels;
                const int64_t f = f0 + r;
                tile[r * S + m] = (r < valid && f >= 0 && f < corpus_frames) ? corpus[e0 + e] : 0.f;
            }
        }
        __syncthreads();
        float *ob = out + b * n_mels * (int64_t)T + t0;                  // out[b][0][t0]
        if (vec_store) {                                                 // T % 4 == 0: t0 + 4 q < T implies the whole quad is inside
            for (int i = tid; i < n_mels * (CT_FRAMES / 4); i += CT_THREADS) {
                const int m = i / (CT_FRAMES / 4), q = (i % (CT_FRAMES / 4)) * 4;
                if (t0 + q < T) {
                    const float *s = tile + q * S + m;
                    const v4f v = {s[0], s[S], s[2 * S], s[3 * S]};
                    *reinterpret_cast<v4f *>(ob + (int64_t)m * T + q) = v;
                }
            }
        } else {
            const int lane = tid % CT_FRAMES;
            if (t0 + lane < T)
                for (int m = tid / CT_FRAMES; m < n_mels; m += CT_THREADS / CT_FRAMES) ob[(int64_t)m * T + lane] = tile[lane * S + m];
        }
        __syncthreads();                                                 // the tile is free for the next one
    }
}

// The same batch's waveform from the clips' samples resident beside the mels (data.py: ResidentMelCorpus.keep_audio): row b of
// out is the run corpus[start_b hop : (start_b + count_b) hop] followed by zeros up to T hop -- no transpose, so no LDS: a
// streaming copy, 2 x B x T x hop x 4 bytes of compulsory traffic.  A row is cut into units of W floats (W = 4 where either side
// moves 16 bytes a lane, else 1) and into chunks of CA_THREADS * CA_UNROLL units; a workgroup owns a chunk, and a lane owns
// CA_UNROLL units CA_THREADS apart, so each wave instruction covers one contiguous run.  A chunk that lies wholly inside the
// row's samples (and the corpus), or wholly inside its padding, is straight-line code: CA_UNROLL independent loads in flight,
// then the stores, no predicate and no wait between them (behind per-unit predicates the compiler waits for every earlier
// access, stores included, before each store).  Only the chunk that holds the samples' end or the row's end takes the
// predicated path: a unit past the samples is stored as zeros without a load, one past the row's end is skipped.  No loop's
// trip count depends on the lane.
constexpr int CA_THREADS = 256;
constexpr int CA_UNROLL = 4;
constexpr int CA_MAX_BLOCKS = 1 << 16;   // the workgroups stride over the chunks: neither B nor a row's length is bound by a grid dimension

template <bool V, int W> __device__ __forceinline__ void ca_load(const float *p, float *v)
{
    if (V) Elem<float>::load16(p, v);
    else
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = p[e];
}
template <bool V, int W> __device__ __forceinline__ void ca_store(float *p, const float *v)
{
    if (V) Elem<float>::store16(p, v);
    else
#pragma unroll
        for (int e = 0; e < W; ++e) p[e] = v[e];
}

template <bool VL, bool VS>
__global__ __launch_bounds__(CA_THREADS) void collate_audio_kernel(const float *__restrict__ corpus, int64_t corpus_samples, int64_t corpus_frames,
                                                                    int hop, const int64_t *__restrict__ plan, int64_t n_chunks, int chunks_row,
                                                                    int T, int64_t L, float *__restrict__ out)
{
    constexpr int W = (VL || VS) ? 4 : 1, STEP = CA_THREADS * W, CHUNK = STEP * CA_UNROLL;
    for (int64_t w = blockIdx.x; w < n_chunks; w += gridDim.x) {
        const int64_t b = w / chunks_row;
        // collate_mels_kernel's clamps: whatever the plan holds, no access leaves either buffer
        int64_t start = plan[b * 3 + 1], count = plan[b * 3 + 2];
        count = count < 0 ? 0 : (count > T ? T : count);
        start = start < -((int64_t)1 << 31) ? -((int64_t)1 << 31) : (start > corpus_frames ? corpus_frames : start);
        const int64_t n = count * hop;                                   // the row's samples, <= L < 2^31
        const int64_t s0 = start * hop;                                  // |start| <= 2^31 + corpus_frames and hop < 2^31: no overflow
        const int64_t c0 = (w - b * chunks_row) * CHUNK, c1 = c0 + CHUNK; // the chunk: elements [c0, c1) of the row
        const int64_t i0 = c0 + threadIdx.x * W;
        float *__restrict__ dst = out + b * L;
        float v[CA_UNROLL][W];
        if (c1 <= n && s0 + c0 >= 0 && s0 + c1 <= corpus_samples) {      // n <= L.  (hop % 4 == 0 where VL: s0 + i is a multiple of 4)
#pragma unroll
            for (int u = 0; u < CA_UNROLL; ++u) ca_load<VL, W>(corpus + s0 + i0 + u * STEP, v[u]);
#pragma unroll
            for (int u = 0; u < CA_UNROLL; ++u) ca_store<VS, W>(dst + i0 + u * STEP, v[u]);
        } else if (c0 >= n && c1 <= L) {
#pragma unroll
            for (int e = 0; e < W; ++e) v[0][e] = 0.f;
#pragma unroll
            for (int u = 0; u < CA_UNROLL; ++u) ca_store<VS, W>(dst + i0 + u * STEP, v[0]);
        } else {
#pragma unroll
            for (int u = 0; u < CA_UNROLL; ++u) {
                const int64_t i = i0 + u * STEP, s = s0 + i;
#pragma unroll
                for (int e = 0; e < W; ++e) v[u][e] = 0.f;
                if (i < n) {
                    // where VL, i + 4 <= n and s is a multiple of 4; only a corpus whose end is not can cut a unit
                    if (VL && s >= 0 && s + W <= corpus_samples) {
                        Elem<float>::load16(corpus + s, v[u]);
                    } else {
#pragma unroll
                        for (int e = 0; e < W; ++e)
                            if (i + e < n && s + e >= 0 && s + e < corpus_samples) v[u][e] = corpus[s + e];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < CA_UNROLL; ++u) {
                const int64_t i = i0 + u * STEP;
                if (VS) {                                                // L % 4 == 0: a unit that starts inside the row ends inside it
                    if (i < L) Elem<float>::store16(dst + i, v[u]);
                } else {
#pragma unroll
                    for (int e = 0; e < W; ++e)
                        if (i + e < L) dst[i + e] = v[u][e];
                }
            }
        }
    }
}

}  // namespace

int nsg_collate_audio(const float *corpus, int64_t corpus_samples, int32_t hop, const int64_t *plan, int32_t B, int32_t T, float *out,
                      void *stream)
{
    NSG_REQUIRE(corpus && plan && out, NSG_E_INVALID, "nsg_collate_audio: null pointer");
    NSG_REQUIRE(B >= 1 && T >= 1 && hop >= 1 && corpus_samples >= 0, NSG_E_INVALID,
                "nsg_collate_audio: bad size (B = %d, T = %d, hop = %d, corpus_samples = %lld)", B, T, hop, (long long)corpus_samples);
    const int64_t L = (int64_t)T * hop;
    NSG_REQUIRE(L < ((int64_t)1 << 31), NSG_E_INVALID, "nsg_collate_audio: T * hop = %lld is not below 2^31", (long long)L);
    NSG_REQUIRE((reinterpret_cast<uintptr_t>(corpus) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0 &&
                    (reinterpret_cast<uintptr_t>(plan) & 7u) == 0,
                NSG_E_INVALID, "nsg_collate_audio: a pointer is not aligned to its element (4 bytes; plan 8)");
    // 16 bytes a lane only where every such access is aligned: a row's first sample start_b * hop is a multiple of 4 floats and
    // the corpus starts on 16 bytes; a row of out is a multiple of 16 bytes and out starts on one
    const bool vl = hop % 4 == 0 && nsg_aligned16(corpus), vs = L % 4 == 0 && nsg_aligned16(out);
    const int W = (vl || vs) ? 4 : 1;
    const int chunks_row = (int)nsg_cdiv(nsg_cdiv(L, W), CA_THREADS * CA_UNROLL);
    const int64_t n_chunks = (int64_t)B * chunks_row;
    const dim3 grid((unsigned)(n_chunks < CA_MAX_BLOCKS ? n_chunks : CA_MAX_BLOCKS)), block(CA_THREADS);
    const hipStream_t s = (hipStream_t)stream;
    const int64_t corpus_frames = corpus_samples / hop;
#define NSG_CA_LAUNCH(VL, VS) \
    hipLaunchKernelGGL((collate_audio_kernel<VL, VS>), grid, block, 0, s, corpus, corpus_samples, corpus_frames, hop, plan, n_chunks, chunks_row, T, L, out)
    if (vl && vs) NSG_CA_LAUNCH(true, true);
    else if (vl) NSG_CA_LAUNCH(true, false);
    else if (vs) NSG_CA_LAUNCH(false, true);
    else NSG_CA_LAUNCH(false, false);
#undef NSG_CA_LAUNCH
    return nsg_check_launch("collate_audio_kernel");
}

int nsg_collate_mels(const float *corpus, int64_t corpus_frames, int32_t n_mels, const int64_t *plan, int32_t B, int32_t T, float *out,
                     void *stream)
{
    NSG_REQUIRE(corpus && plan && out, NSG_E_INVALID, "nsg_collate_mels: null pointer");
    NSG_REQUIRE(B >= 1 && T >= 1 && corpus_frames >= 0, NSG_E_INVALID, "nsg_collate_mels: bad size (B = %d, T = %d, corpus_frames = %lld)", B, T,
                (long long)corpus_frames);
    NSG_REQUIRE(n_mels >= 1 && n_mels <= CT_MAX_MELS, NSG_E_INVALID, "nsg_collate_mels: n_mels = %d outside [1, %d]", n_mels, CT_MAX_MELS);
    const int tiles_t = (int)nsg_cdiv(T, CT_FRAMES);
    const int64_t n_tiles = (int64_t)B * tiles_t;
    const int S = n_mels | 1;
    // 16 bytes a lane only where every such access is aligned: a frame is a multiple of 16 bytes and the corpus starts on one;
    // a row of out is a multiple of 16 bytes and out starts on one (tiles start at multiples of 64 floats)
    const int vec_load = n_mels % 4 == 0 && nsg_aligned16(corpus), vec_store = T % 4 == 0 && nsg_aligned16(out);
    hipLaunchKernelGGL(collate_mels_kernel, dim3((unsigned)(n_tiles < CT_MAX_BLOCKS ? n_tiles : CT_MAX_BLOCKS)), dim3(CT_THREADS),
                       (size_t)CT_FRAMES * S * sizeof(float), (hipStream_t)stream, corpus, corpus_frames, n_mels, plan, n_tiles, tiles_t, T, out,
                       nsg_fastdiv((uint32_t)n_mels), vec_load, vec_store);
    return nsg_check_launch("collate_mels_kernel");
}
