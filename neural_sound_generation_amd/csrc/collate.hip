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

}  // namespace

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
