// What stands between a recording and the mel front end in the reference's multi-speaker preprocessing (src/cmu_arctic.py:59-72):
// librosa.core.load(path, sr=22050) resamples (audio_tacotron.py:12-13), librosa.effects.trim(wav, top_db=20) cuts the silent ends.
//   * resample: a band-limited Kaiser-windowed sinc interpolator evaluated exactly per polyphase phase (no interpolation in a
//     filter table).  The host builds the P x 2W coefficient table in fp64 and rounds it once; an output is ONE fp32 fmaf
//     chain over its 2W taps in increasing tap order, its inputs staged in LDS (zeros outside the clip), so a clip's samples
//     do not depend on the batch, the row or the tiling.
//   * trim bounds: librosa.effects.trim's frame energies (centred, reflect-padded frames), the clip's loudest frame as the
//     reference, and the first and last frame within top_db of it.
// fp32, ragged batches as melspectrogram_kernel takes them: a clip's length, the zero-padded read and the reflect map are
// nsg_wave.h's, the wave stages of the frame sums and of the bounds nsg_reduce.h's.  HBM- / L2-bound kernels; nothing here
// touches the matrix pipe.
#include "nsg_common.h"
#include "nsg_reduce.h"
#include "nsg_wave.h"
#include <math.h>

namespace {

constexpr int RS_TILE = 256;                    // outputs per workgroup, one per thread
constexpr int RS_MAX_TABLE = 1 << 20;           // floats: P * 2W
constexpr size_t RS_MAX_LDS = 64 * 1024;        // the staged input span of a tile

// out[b][m] = sum_j x_b[floor(m Q / P) - W + 1 + j] * table[j][m mod P],  j = 0 .. 2W - 1 in that order, x_b zero outside
// [0, len_b).  The table is stored tap-major with its phases in the order consecutive outputs meet them (column k holds phase
// (k Q) mod P): the 64 lanes of a wave, which hold consecutive m, read consecutive floats of row j.
__global__ __launch_bounds__(RS_TILE) void resample_kernel(const float *__restrict__ wav, const int32_t *__restrict__ lengths,
                                                           const float *__restrict__ table, float *__restrict__ out, int L_in, int L_out,
                                                           int tiles, int P, int Q, int W)
{
    extern __shared__ float xs[];               // x_b[lo .. hi] of this tile
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)tiles);
    const int64_t m0 = (int64_t)(blockIdx.x - (unsigned)b * tiles) * RS_TILE, m = m0 + tid;
    const int len = nsg_clip_len(lengths, b, L_in);
    const int64_t len_out = ((int64_t)len * P + Q - 1) / Q;             // <= L_out
    float *ob = out + (size_t)b * L_out;
    if (m0 >= len_out) {                                                // the whole tile is past the clip's end
        if (m < L_out) ob[m] = 0.f;
        return;
    }
    const int64_t m_last = m0 + RS_TILE - 1 < L_out - 1 ? m0 + RS_TILE - 1 : L_out - 1;
    const int64_t lo = m0 * Q / P - W + 1, hi = m_last * Q / P + W;     // inclusive; hi - lo + 1 <= (RS_TILE - 1) Q / P + 2 W + 1
    const float *x = wav + (size_t)b * L_in;
    for (int i = tid; i <= (int)(hi - lo); i += RS_TILE) xs[i] = nsg_clip_at(x, lo + i, len);
    __syncthreads();
    if (m >= L_out) return;
    float acc = 0.f;
    if (m < len_out) {
        const float *xp = xs + (m * Q / P - W + 1 - lo);
        const float *c = table + (int)(m % P);
#pragma unroll 8
        for (int j = 0; j < 2 * W; ++j) acc = fmaf(xp[j], c[(size_t)j * P], acc);
    }
    ob[m] = acc;
}

// mse[b][t] = mean over the frame of p^2, p = reflect_pad(x_b[0:len_b], N/2)[t hop : t hop + N]; one wave per frame: lane l adds
// samples l, l + 64, ... in that order, then the 64 lane sums meet in nsg_wave_sum_butterfly.  Frames past the clip's own count
// are left unwritten (trim_bounds_kernel never reads them).
__global__ __launch_bounds__(256) void frame_energy_kernel(const float *__restrict__ wav, const int32_t *__restrict__ lengths,
                                                           float *__restrict__ mse, int L, int T, int groups, int N, int hop)
{
    const int b = (int)(blockIdx.x / (unsigned)groups);
    const int t = (int)(blockIdx.x - (unsigned)b * groups) * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int len = nsg_clip_len_reflect(lengths, b, L);                // (the caller checked N/2 < len <= L on its host copy)
    if (t >= 1 + len / hop) return;                                     // wave-uniform
    const float *x = wav + (size_t)b * L;
    const int64_t start = (int64_t)t * hop - N / 2;
    float s = 0.f;
    for (int i = lane; i < N; i += 64) {
        const float v = x[nsg_reflect_once(start + i, len)];            // the padding N/2 < len: one fold is the exact map
        s = fmaf(v, v, s);
    }
    s = nsg_wave_sum_butterfly(s);
    if (lane == 0) mse[(size_t)b * T + t] = s / (float)N;
}

// One workgroup per clip: ref = max_t mse[t]; frame t is non-silent iff 10 log10(max(1e-10, mse[t])) - 10 log10(max(1e-10, ref))
// > -top_db; bounds = (first hop, min(len, (last + 1) hop)), or (0, 0) when no frame qualifies.  max / min / max reductions, exact
// in any order: nsg_reduce.h's wave stage, then the four wave results through LDS (as stoi_select_kernel's maximum).  A thread
// -- or a whole wave -- that owns no frame offers the identity: 0.f, INT_MAX, -1.
__global__ __launch_bounds__(256) void trim_bounds_kernel(const float *__restrict__ mse, const int32_t *__restrict__ lengths,
                                                          int32_t *__restrict__ bounds, int L, int T, int hop, float top_db)
{
    __shared__ float wmax[4];
    __shared__ int wlo[4], whi[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = nsg_clip_len_reflect(lengths, b, L);
    const int Tb = 1 + len / hop;
    const float *e = mse + (size_t)b * T;
    float mx = 0.f;                                                     // energies are >= 0
    for (int t = tid; t < Tb; t += 256) mx = fmaxf(mx, e[t]);
    mx = nsg_wave_max(mx);
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    const float ref_db = 10.f * log10f(fmaxf(1e-10f, fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
    int first = 0x7fffffff, last = -1;
    for (int t = tid; t < Tb; t += 256)
        if (10.f * log10f(fmaxf(1e-10f, e[t])) - ref_db > -top_db) {
            first = t < first ? t : first;
            last = t;
        }
    first = nsg_wave_min(first);
    last = nsg_wave_max(last);
    if (lane == 0) { wlo[wave] = first; whi[wave] = last; }
    __syncthreads();
    if (tid == 0) {
        const int lo = min(min(wlo[0], wlo[1]), min(wlo[2], wlo[3])), hi = max(max(whi[0], whi[1]), max(whi[2], whi[3]));
        const int64_t end = ((int64_t)hi + 1) * hop;
        bounds[2 * b] = hi < 0 ? 0 : (int32_t)((int64_t)lo * hop);
        bounds[2 * b + 1] = hi < 0 ? 0 : (int32_t)(end < len ? end : len);
    }
}

inline int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

}  // namespace

extern "C" {

int nsg_audio_resample(const float *wav, const int32_t *lengths, const float *table, float *out, int32_t B, int32_t L_in, int32_t up,
                       int32_t down, int32_t half_width, void *stream)
{
    NSG_REQUIRE(wav && table && out && B > 0 && L_in > 0 && up > 0 && down > 0 && half_width > 0, NSG_E_INVALID, "nsg_audio_resample: bad argument");
    NSG_REQUIRE(gcd64(up, down) == 1, NSG_E_INVALID, "nsg_audio_resample: up / down = %d / %d is not in lowest terms", up, down);
    NSG_REQUIRE((int64_t)up * 2 * half_width <= RS_MAX_TABLE, NSG_E_UNSUPPORTED,
                "nsg_audio_resample: the table of ratio %d / %d has %lld floats, more than 2^20", up, down, (long long)up * 2 * half_width);
    const int64_t L_out = ((int64_t)L_in * up + down - 1) / down;
    NSG_REQUIRE(L_out < 0x7fffffff, NSG_E_UNSUPPORTED, "nsg_audio_resample: too many output samples (ceil(L_in up / down) >= 2^31)");
    const int64_t tiles = nsg_cdiv(L_out, RS_TILE);
    NSG_REQUIRE((int64_t)B * tiles < 0x7fffffff, NSG_E_UNSUPPORTED, "nsg_audio_resample: too many tiles (B * ceil(L_out / 256) >= 2^31)");
    const size_t lds = (size_t)((int64_t)(RS_TILE - 1) * down / up + 2 * (int64_t)half_width + 1) * sizeof(float);
    NSG_REQUIRE(lds <= RS_MAX_LDS, NSG_E_UNSUPPORTED, "nsg_audio_resample: ratio %d / %d needs %zu bytes of LDS per tile, more than 64 KiB", up, down, lds);
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(B * tiles)), dim3(RS_TILE), lds, (hipStream_t)stream, wav, lengths, table, out, L_in,
                       (int)L_out, (int)tiles, up, down, half_width);
    return nsg_check_launch("resample_kernel");
}

size_t nsg_audio_trim_workspace_bytes(int32_t B, int32_t L, int32_t hop)
{
    if (B <= 0 || L <= 0 || hop <= 0) return 0;
    return nsg_align_up((size_t)B * (size_t)(1 + L / hop) * sizeof(float), 256);
}

int nsg_audio_trim_bounds(const float *wav, const int32_t *lengths, int32_t *bounds, int32_t B, int32_t L, int32_t frame_length, int32_t hop,
                          float top_db, void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(wav && bounds && B > 0 && L > 0 && hop > 0 && top_db > 0.f, NSG_E_INVALID, "nsg_audio_trim_bounds: bad argument (top_db > 0, hop > 0)");
    NSG_REQUIRE(frame_length >= 2 && frame_length <= 8192 && frame_length % 2 == 0, NSG_E_UNSUPPORTED,
                "nsg_audio_trim_bounds: frame_length must be even and in [2, 8192]");
    NSG_REQUIRE(L > frame_length / 2, NSG_E_UNSUPPORTED, "nsg_audio_trim_bounds: reflect padding needs more than frame_length/2 samples");
    const int T = 1 + L / hop, groups = (T + 3) / 4;
    NSG_REQUIRE((int64_t)B * groups < 0x7fffffff, NSG_E_UNSUPPORTED, "nsg_audio_trim_bounds: too many frames (B * (1 + L / hop) / 4 >= 2^31)");
    NSG_REQUIRE(workspace && workspace_bytes >= nsg_audio_trim_workspace_bytes(B, L, hop), NSG_E_WORKSPACE, "nsg_audio_trim_bounds: workspace too small");
    float *mse = reinterpret_cast<float *>(workspace);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(frame_energy_kernel, dim3((unsigned)(B * groups)), dim3(256), 0, s, wav, lengths, mse, L, T, groups, frame_length, hop);
    hipLaunchKernelGGL(trim_bounds_kernel, dim3((unsigned)B), dim3(256), 0, s, mse, lengths, bounds, L, T, hop, top_db);
    return nsg_check_launch("trim_bounds");
}

}  // extern "C"
