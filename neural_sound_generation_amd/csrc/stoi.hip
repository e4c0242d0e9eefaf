// Short-time objective intelligibility of a processed clip y against the clean clip x, at 10 kHz: STOI (Taal, Hendriks, Heusdens,
// Jensen 2011) and ESTOI (Jensen, Taal 2016).  An extension: the reference has no figure in the waveform domain.  include/nsg.h states
// the definition (nsg_audio_stoi_envelopes, nsg_audio_stoi_score); tests/helpers/stoi_ref.py restates it in numpy.  Four launches:
//   * stoi_energy_kernel: the windowed energy of every candidate frame of x, fp64, one wave per frame;
//   * stoi_select_kernel: one workgroup per clip -- the exact maximum, the frames within 40 dB of it, their list src by a block scan;
//   * stoi_envelope_kernel: one workgroup per (clip, kept frame) -- the frame of the compacted signal gathered through src (it is
//     never stored), x's and y's frame as the real and the imaginary part of ONE 512-point FFT (nsg_fft.h), split by Hermitian
//     symmetry, |.|^2 in LDS, the 15 third-octave band sums and their roots;
//   * stoi_score_kernel: one workgroup per clip, fp64 throughout -- a thread per (segment, band) for STOI, per segment for ESTOI
//     (its envelopes staged in LDS), closed by nsg_reduce.h's butterfly block sum.
// No workspace and no atomics: every intermediate is a caller-owned output.  LDS- and latency-bound kernels on tiny data; nothing
// here touches the matrix pipe.
#include "nsg_common.h"
#include "nsg_reduce.h"
#include "nsg_fft.h"
#include <math.h>

namespace {

constexpr int STOI_FRAME = 256, STOI_HOP = 128, STOI_LOG2_FFT = 9, STOI_BINS = 257, STOI_BANDS = 15, STOI_SEG = 30;
constexpr double STOI_EPS = 2.220446049250313e-16;            // 2^-52
constexpr double STOI_RANGE = 1e-4;                           // 40 dB below the loudest frame, as an energy ratio

// w[n] = 0.5 - 0.5 cos(2 pi (n + 1) / 257), n < 256 (MATLAB's hanning(256)), in fp64; the spectral frames use it rounded to fp32.
__device__ __forceinline__ double stoi_window(int n) { return 0.5 - 0.5 * cospi(2.0 * (double)(n + 1) / 257.0); }

// The candidate frames of a clip of `len` samples in a row of L: (len - 256) / 128 + 1, none for a length outside [256, L].
__device__ __forceinline__ int stoi_frames(const int32_t *__restrict__ lengths, int b, int L)
{
    const int len = lengths ? lengths[b] : L;
    return len < STOI_FRAME || len > L ? 0 : (len - STOI_FRAME) / STOI_HOP + 1;
}

// energy[b][t] = sum_n ((double)w[n] (double)x[128 t + n])^2, one wave per frame (four frames per workgroup), no barrier.  Order:
// lane l adds the squares of its samples 4 l .. 4 l + 3 to 0.0 in that order; the 64 lane sums are closed by
// nsg_wave_sum_butterfly.  Frames past the clip's own count are written as 0.0.
__global__ __launch_bounds__(256) void stoi_energy_kernel(const float *__restrict__ x, const int32_t *__restrict__ lengths, double *__restrict__ energy,
                                                          int B, int L, int Tmax)
{
    const int lane = threadIdx.x & 63;
    const int64_t fr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (fr >= (int64_t)B * Tmax) return;
    const int b = (int)(fr / Tmax), t = (int)(fr - (int64_t)b * Tmax);
    if (t >= stoi_frames(lengths, b, L)) {
        if (lane == 0) energy[fr] = 0.0;
        return;
    }
    const float *xf = x + (size_t)b * L + (size_t)t * STOI_HOP + 4 * lane;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double p = stoi_window(4 * lane + i) * (double)xf[i];
        s += p * p;
    }
    s = nsg_wave_sum_butterfly(s);
    if (lane == 0) energy[fr] = s;
}

// One clip per workgroup: frame t < T_b is kept iff energy[t] > 1e-4 max_t energy[t] (fp64, strict); src[k] = the k-th kept frame,
// -1 for k >= kept[b].  The maximum is exact (order-free), the list an exclusive scan of the keep flags: per round of 256 frames a
// ballot inside each wave, the four wave counts through LDS.
__global__ __launch_bounds__(256) void stoi_select_kernel(const double *__restrict__ energy, const int32_t *__restrict__ lengths, int32_t *__restrict__ src,
                                                          int32_t *__restrict__ kept, int L, int Tmax)
{
    __shared__ double wmax[4];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int Tb = stoi_frames(lengths, b, L);
    const double *e = energy + (size_t)b * Tmax;
    int32_t *sb = src + (size_t)b * Tmax;
    double mx = 0.0;                                           // (energies are >= 0)
    for (int t = tid; t < Tb; t += 256) mx = fmax(mx, e[t]);
    mx = nsg_wave_max(mx);
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    const double thr = STOI_RANGE * fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
    int base = 0;
    for (int t0 = 0; t0 < Tb; t0 += 256) {                     // (Tb is uniform: every thread meets every barrier)
        const int t = t0 + tid;
        const bool keep = t < Tb && e[t] > thr;
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wcnt[wave] = __popcll(mask);
        __syncthreads();
        int k = base + __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) k += wcnt[w];
        if (keep) sb[k] = t;
        base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();                                       // (wcnt is rewritten in the next round)
    }
    for (int k = base + tid; k < Tmax; k += 256) sb[k] = -1;
    if (tid == 0) kept[b] = base;
}

// The 15 bands as runs of bins [lo, hi), passed by value: the launcher has checked them on the host, and no upload precedes the launch.
struct StoiBands { int16_t lo[STOI_BANDS], hi[STOI_BANDS]; };

// One (clip, spectral frame m) per workgroup.  With C = kept[b] and xs[128 k + n] += w[n] x[128 src[k] + n] (k < C, n < 256) the
// compacted clean signal, frame m is w[n] xs[128 m + n]: its first half overlaps source frame src[m - 1] (m >= 1), its second half
// src[m + 1] (m + 1 < C), so a sample is  w[n] (w[n] x[128 src[m] + n] + w[n +- 128] x[128 src[m -+ 1] + n +- 128])  in fp32, the
// earlier source frame's term first.  The same for y with the same src.  z = frame_x + i frame_y, zero-padded to 512; Z = fft(z);
// X[f] = (Z[f] + conj Z[512 - f]) / 2, Y[f] = (Z[f] - conj Z[512 - f]) / 2i (melspectrogram_kernel's split).  env[s][b][m][j] =
// sqrtf(sum over f in [lo_j, hi_j) of |.|^2, added to 0.f in index order).  m >= C: zeros, and the workgroup leaves before any barrier.
__global__ __launch_bounds__(256) void stoi_envelope_kernel(const float *__restrict__ x, const float *__restrict__ y, const int32_t *__restrict__ src,
                                                            const int32_t *__restrict__ kept, const StoiBands bands, float *__restrict__ env,
                                                            int B, int L, int Tmax)
{
    constexpr int N = 1 << STOI_LOG2_FFT;
    __shared__ FftLds<STOI_LOG2_FFT> fft;
    __shared__ float pw[2][STOI_BINS];
    __shared__ float win[STOI_FRAME];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)Tmax), m = (int)(blockIdx.x - (unsigned)b * Tmax);
    const int sig = tid / STOI_BANDS, j = tid - sig * STOI_BANDS;             // the output this thread owns, for tid < 30
    float *out = env + (((size_t)sig * B + b) * Tmax + m) * STOI_BANDS + j;
    int C = kept[b];
    C = C < 0 ? 0 : (C > Tmax ? Tmax : C);
    if (m >= C) {                                                             // uniform: kept[b] and m are the workgroup's
        if (tid < 2 * STOI_BANDS) *out = 0.f;
        return;
    }
    fft.fill_twiddles(tid);
    win[tid] = (float)stoi_window(tid);
    const int32_t *sb = src + (size_t)b * Tmax;
    const int n = tid;                                                        // one sample of the frame per thread
    const int other = n < STOI_HOP ? (m >= 1 ? sb[m - 1] : -1) : (m + 1 < C ? sb[m + 1] : -1);
    const int no = n < STOI_HOP ? n + STOI_HOP : n - STOI_HOP;                // the sample's offset inside the other source frame
    const size_t at = (size_t)b * L + (size_t)sb[m] * STOI_HOP + n;
    const size_t ao = (size_t)b * L + (size_t)(other < 0 ? 0 : other) * STOI_HOP + no;
    __syncthreads();                                                          // win
    const float wn = win[n], wo = win[no];
    float vx = wn * x[at], vy = wn * y[at];
    if (other >= 0) {
        const float ox = wo * x[ao], oy = wo * y[ao];
        vx = n < STOI_HOP ? ox + vx : vx + ox;
        vy = n < STOI_HOP ? oy + vy : vy + oy;
    }
    fft.b0[n] = v2f{wn * vx, wn * vy};
    fft.b0[n + STOI_FRAME] = v2f{0.f, 0.f};
    v2f *r = fft.transform(tid, false);
    for (int f = tid; f < STOI_BINS; f += 256) {
        const v2f Z = r[f], Cj = r[(N - f) & (N - 1)];
        const float ar = Z.x + Cj.x, ai = Z.y - Cj.y;                         // 2 X[f]
        const float br = Z.y + Cj.y, bi = Z.x - Cj.x;                         // 2 i Y[f] up to sign: the same modulus
        pw[0][f] = 0.25f * (ar * ar + ai * ai);
        pw[1][f] = 0.25f * (br * br + bi * bi);
    }
    __syncthreads();
    if (tid >= 2 * STOI_BANDS) return;
    const float *p = pw[sig];
    const int f1 = bands.hi[j];
    float acc = 0.f;
    for (int f = bands.lo[j]; f < f1; ++f) acc += p[f];
    *out = sqrtf(acc);
}

// env[sig][b][m][j] widened to fp64
struct StoiEnv {
    const float *x, *y;
    __device__ __forceinline__ double X(int m, int j) const { return (double)x[(size_t)m * STOI_BANDS + j]; }
    __device__ __forceinline__ double Y(int m, int j) const { return (double)y[(size_t)m * STOI_BANDS + j]; }
};

// STOI's intermediate correlation of band j over the segment of frames m0 .. m0 + 29 (include/nsg.h states the order).
__device__ __forceinline__ double stoi_segment_band(const StoiEnv &E, int m0, int j, double clip)
{
    double xv[STOI_SEG], yv[STOI_SEG];
    double sx2 = 0.0, sy2 = 0.0, sx = 0.0;
#pragma unroll
    for (int n = 0; n < STOI_SEG; ++n) {
        xv[n] = E.X(m0 + n, j);
        yv[n] = E.Y(m0 + n, j);
        sx2 += xv[n] * xv[n];
        sy2 += yv[n] * yv[n];
        sx += xv[n];
    }
    const double alpha = sqrt(sx2 / (sy2 + STOI_EPS));
    double sy = 0.0;
#pragma unroll
    for (int n = 0; n < STOI_SEG; ++n) {
        yv[n] = fmin(alpha * yv[n], clip * xv[n]);
        sy += yv[n];
    }
    const double mx = sx / (double)STOI_SEG, my = sy / (double)STOI_SEG;
    double num = 0.0, nx = 0.0, ny = 0.0;
#pragma unroll
    for (int n = 0; n < STOI_SEG; ++n) {
        const double a = xv[n] - mx, c = yv[n] - my;
        num += a * c;
        nx += a * a;
        ny += c * c;
    }
    return num / (sqrt(nx) * sqrt(ny) + STOI_EPS);
}

// ESTOI's intermediate figure of the segment m0 .. m0 + 29.  The 15 x 30 matrices are never held: a first pass over the rows (bands)
// forms each row's mean and 1 / (norm + eps), a second pass over the columns (frames) normalises a column of the row-normalised
// matrices and adds its inner product.
__device__ __forceinline__ double estoi_segment(const StoiEnv &E, int m0)
{
    double mean[2][STOI_BANDS], scale[2][STOI_BANDS];
#pragma unroll
    for (int j = 0; j < STOI_BANDS; ++j) {
        double sx = 0.0, sy = 0.0;
        for (int n = 0; n < STOI_SEG; ++n) { sx += E.X(m0 + n, j); sy += E.Y(m0 + n, j); }
        const double mx = sx / (double)STOI_SEG, my = sy / (double)STOI_SEG;
        double nx = 0.0, ny = 0.0;
        for (int n = 0; n < STOI_SEG; ++n) {
            const double a = E.X(m0 + n, j) - mx, c = E.Y(m0 + n, j) - my;
            nx += a * a;
            ny += c * c;
        }
        mean[0][j] = mx; scale[0][j] = 1.0 / (sqrt(nx) + STOI_EPS);
        mean[1][j] = my; scale[1][j] = 1.0 / (sqrt(ny) + STOI_EPS);
    }
    double d = 0.0;
    for (int n = 0; n < STOI_SEG; ++n) {
        double xc[STOI_BANDS], yc[STOI_BANDS];
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int j = 0; j < STOI_BANDS; ++j) {
            xc[j] = (E.X(m0 + n, j) - mean[0][j]) * scale[0][j];
            yc[j] = (E.Y(m0 + n, j) - mean[1][j]) * scale[1][j];
            sx += xc[j];
            sy += yc[j];
        }
        const double mx = sx / (double)STOI_BANDS, my = sy / (double)STOI_BANDS;
        double num = 0.0, nx = 0.0, ny = 0.0;
#pragma unroll
        for (int j = 0; j < STOI_BANDS; ++j) {
            const double a = xc[j] - mx, c = yc[j] - my;
            num += a * c;
            nx += a * a;
            ny += c * c;
        }
        d += num / ((sqrt(nx) + STOI_EPS) * (sqrt(ny) + STOI_EPS));
    }
    return d / (double)STOI_SEG;
}

// One clip per workgroup: d[b] = the mean of the intermediate figures over the clip's items -- (segment, band) pairs for STOI,
// segments for ESTOI -- or NaN with fewer than 30 kept frames.  Order: thread tid adds its items tid, tid + 256, ... to 0.0 in that
// order (item i of STOI is segment i / 15, band i % 15); the 256 thread sums are closed by nsg_block_sum_butterfly.
// STOI's loads coalesce as they are (adjacent threads own adjacent (segment, band) pairs: adjacent floats).  ESTOI's threads own
// adjacent segments, 15 floats apart, and each reads its 900 values three times: the 285 frames behind a round of 256 segments are
// staged in LDS first (34 KB; a stride of 15 words meets every bank once), which is what the threads then read.
constexpr int STOI_TILE_FRAMES = 256 + STOI_SEG - 1;
template <bool EXTENDED>
__global__ __launch_bounds__(256) void stoi_score_kernel(const float *__restrict__ env, const int32_t *__restrict__ kept, double *__restrict__ d,
                                                         int B, int Tmax, double clip)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    int C = kept[b];
    C = C > Tmax ? Tmax : C;
    if (C < STOI_SEG) {                                                       // uniform
        if (tid == 0) d[b] = __builtin_nan("");
        return;
    }
    const StoiEnv E = {env + (size_t)b * Tmax * STOI_BANDS, env + ((size_t)B + b) * Tmax * STOI_BANDS};
    const int segs = C - STOI_SEG + 1;
    const int items = EXTENDED ? segs : segs * STOI_BANDS;
    double acc = 0.0;
    if constexpr (EXTENDED) {
        __shared__ float tile[2][STOI_TILE_FRAMES * STOI_BANDS];
        const StoiEnv T = {tile[0], tile[1]};
        for (int s0 = 0; s0 < segs; s0 += 256) {                              // (segs is uniform: every thread meets every barrier)
            const int nf = min(STOI_TILE_FRAMES, C - s0);                     // frames s0 .. s0 + nf - 1 serve the segments s0 .. s0 + 255
            for (int i = tid; i < nf * STOI_BANDS; i += 256) {
                tile[0][i] = E.x[(size_t)s0 * STOI_BANDS + i];
                tile[1][i] = E.y[(size_t)s0 * STOI_BANDS + i];
            }
            __syncthreads();
            if (s0 + tid < segs) acc += estoi_segment(T, tid);
            __syncthreads();                                                  // (the tile is rewritten in the next round)
        }
    } else {
        for (int i = tid; i < items; i += 256) acc += stoi_segment_band(E, i / STOI_BANDS, i % STOI_BANDS, clip);
    }
    acc = nsg_block_sum_butterfly(acc, red, tid);
    if (tid == 0) d[b] = acc / (double)items;
}

// the candidate frames of a row of L samples, and the refusal if B rows of them do not fit a grid
int stoi_grid(const char *name, int B, int Tmax)
{
    NSG_REQUIRE((int64_t)B * Tmax < 0x7fffffff, NSG_E_UNSUPPORTED, "%s: too many frames (B * Tmax >= 2^31)", name);
    return 0;
}

}  // namespace

extern "C" {

int nsg_audio_stoi_envelopes(const float *x, const float *y, const int32_t *lengths, const int32_t *band_lo, const int32_t *band_hi, double *energy,
                             int32_t *src, int32_t *kept, float *env, int32_t B, int32_t L, void *stream)
{
    NSG_REQUIRE(x && y && band_lo && band_hi && energy && src && kept && env && B > 0, NSG_E_INVALID, "nsg_audio_stoi_envelopes: bad argument");
    NSG_REQUIRE(L >= STOI_FRAME, NSG_E_UNSUPPORTED, "nsg_audio_stoi_envelopes: a row holds no frame (L < 256)");
    const int Tmax = (L - STOI_FRAME) / STOI_HOP + 1;
    if (const int rc = stoi_grid("nsg_audio_stoi_envelopes", B, Tmax)) return rc;
    StoiBands sb;
    for (int j = 0; j < STOI_BANDS; ++j) {
        const int32_t lo = band_lo[j], hi = band_hi[j];
        NSG_REQUIRE(lo >= (j ? band_hi[j - 1] : 0) && lo < hi && hi <= STOI_BINS, NSG_E_INVALID,
                    "nsg_audio_stoi_envelopes: the bands must be 15 ascending non-empty runs [lo, hi) of the bins 0 .. 256");
        sb.lo[j] = (int16_t)lo;
        sb.hi[j] = (int16_t)hi;
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t nfr = (int64_t)B * Tmax;
    hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)nsg_cdiv(nfr, 4)), dim3(256), 0, s, x, lengths, energy, B, L, Tmax);
    hipLaunchKernelGGL(stoi_select_kernel, dim3((unsigned)B), dim3(256), 0, s, energy, lengths, src, kept, L, Tmax);
    hipLaunchKernelGGL(stoi_envelope_kernel, dim3((unsigned)nfr), dim3(256), 0, s, x, y, src, kept, sb, env, B, L, Tmax);
    return nsg_check_launch("stoi_envelopes");
}

int nsg_audio_stoi_score(const float *env, const int32_t *kept, double *d, int32_t B, int32_t Tmax, int32_t extended, void *stream)
{
    NSG_REQUIRE(env && kept && d && B > 0 && Tmax > 0 && (extended == 0 || extended == 1), NSG_E_INVALID, "nsg_audio_stoi_score: bad argument");
    if (const int rc = stoi_grid("nsg_audio_stoi_score", B, Tmax)) return rc;
    const double clip = 1.0 + pow(10.0, 15.0 / 20.0);           // the lower signal-to-distortion bound, -15 dB
    hipStream_t s = (hipStream_t)stream;
    if (extended) hipLaunchKernelGGL(stoi_score_kernel<true>, dim3((unsigned)B), dim3(256), 0, s, env, kept, d, B, Tmax, clip);
    else          hipLaunchKernelGGL(stoi_score_kernel<false>, dim3((unsigned)B), dim3(256), 0, s, env, kept, d, B, Tmax, clip);
    return nsg_check_launch("stoi_score");
}

}  // extern "C"
