// Mel -> waveform inversion of the reference's epoch loop (src/main.py:164-197 -> src/audio_tacotron.py:99-116,142-153
// with use_lws=False): denormalise, dB -> amplitude, pseudo-inverse mel basis, power, Griffin-Lim, inverse pre-emphasis.
// SURVEY.md section 8f row 4.  The reference delegates the transforms to librosa (stft / istft) and scipy (lfilter);
// their published algorithms are restated here as HIP kernels (and in numpy in oracle/audio_oracle.py):
//   * radix-2 Stockham FFT of one frame per 256-thread workgroup, entirely in LDS (nsg_fft.h's FftLds: ping-pong buffers, twiddle table);
//   * stft: centred frames with reflect padding x periodic Hann window -> FFT (stft_frame_lds, the one place that forms such a
//     frame) -> keep 1 + N/2 bins; stft_kernel<LOG2N, OUT> stores them raw or fused with the Griffin-Lim phase update
//     spec = |S| * X / |X|  (with momentum: the phase of X + momentum (X - X_prev), X_prev updated in place);
//   * spectral convergence: the same frame with || |X| - S ||^2 and || S ||^2 summed in fp64 out of LDS (the spectrum is not stored);
//   * istft: Hermitian extension -> inverse FFT -> x window -> frame buffer; overlap-add as a gather (deterministic)
//     divided by the window's sum of squares, centre-trimmed;
//   * inverse pre-emphasis y[n] = x[n] + k y[n-1]: chunked, each chunk re-running a discarded warm-up (k^W < 1e-9).
// The opposite direction (audio_tacotron.py:23-26,70-78), wav -> normalised mel, is one kernel on the same FFT: pre-emphasis at the
// reflect-mapped index, Hann, two frames per complex FFT, |X| in LDS, the filterbank as a band matrix, dB, normalise, clip.
// fp32 throughout (complex as float2).  These are LDS- / HBM-bound kernels; nothing here touches the matrix pipe.
#include "nsg_common.h"
#include "nsg_reduce.h"
#include "nsg_fft.h"
#include "nsg_wave.h"
#include <math.h>
#include <type_traits>

namespace {

// Periodic Hann window 0.5 - 0.5 cos(2 pi n / N) as sin^2(pi n / N): no cancellation at the window's ends, where the cosine form
// is wrong by eps / w (8e-4 of w at n = 1, N = 512).  Griffin-Lim needs the accurate form: overlap-add divides by the sum of
// w^2, and with hop == N that sum is one term, so the quotient w / w^2 carries the window's relative error into y, and the
// next STFT multiplies those same samples (y = frame / w there) by w again.  (melspectrogram_kernel keeps the cosine form:
// it only multiplies by w, where the error is 3e-8 of the window's peak, and its outputs are pinned bit for bit.)
__device__ __forceinline__ float hann_sin2(int n, int N) { const float s = sinpif((float)n / (float)N); return s * s; }

// S[b][t][f] = max(1e-10, sum_m inv[f][m] * amp(mel[b][m][t]))^power,  amp = 10^((clip(mel,0,max_abs)*(-min_db)/max_abs + min_db + ref_db)/20)
__global__ __launch_bounds__(256) void mel_to_linear_kernel(const float *__restrict__ mel, const float *__restrict__ inv, float *__restrict__ S,
                                                            int B, int n_mels, int T, int F, float min_db, float ref_db, float max_abs, float power)
{
    extern __shared__ float amp[];     // [n_mels] of this (b, t)
    const int bt = blockIdx.x;
    const int b = bt / T, t = bt - b * T;
    for (int m = threadIdx.x; m < n_mels; m += 256) {
        const float v = fminf(fmaxf(mel[((size_t)b * n_mels + m) * T + t], 0.f), max_abs);
        const float db = v * (-min_db) / max_abs + min_db + ref_db;
        amp[m] = exp10f(db * 0.05f);
    }
    __syncthreads();
    for (int f = threadIdx.x; f < F; f += 256) {
        float acc = 0.f;
        for (int m = 0; m < n_mels; ++m) acc = fmaf(inv[(size_t)f * n_mels + m], amp[m], acc);
        S[((size_t)b * T + t) * F + f] = powf(fmaxf(acc, 1e-10f), power);
    }
}

// spec[b][t][f] = S[b][t][f] * exp(2 pi i u[b][t][f])   (the random initial phases, u uniform in [0, 1))
__global__ void init_phase_kernel(const float *__restrict__ S, const float *__restrict__ u, v2f *__restrict__ spec, int64_t n)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float sn, cs;
        sincospif(2.0f * u[i], &sn, &cs);
        spec[i] = v2f{S[i] * cs, S[i] * sn};
    }
}

// one frame per workgroup: frames[b][t][n] = hann[n] * irfft(spec[b][t])[n]
template <int LOG2N>
__global__ __launch_bounds__(256) void istft_frames_kernel(const v2f *__restrict__ spec, float *__restrict__ frames, int F)
{
    constexpr int N = 1 << LOG2N;
    __shared__ FftLds<LOG2N> fft;
    const int tid = threadIdx.x;
    const size_t fr = blockIdx.x;
    fft.fill_twiddles(tid);
    const v2f *sp = spec + fr * F;
    for (int k = tid; k < N; k += 256) {
        v2f v;
        if (k <= N / 2) { v = sp[k]; if (k == 0 || k == N / 2) v.y = 0.f; }     // irfft ignores the imaginary part of DC / Nyquist
        else { v = sp[N - k]; v.y = -v.y; }
        fft.b0[k] = v;
    }
    v2f *r = fft.transform(tid, true);
    float *dst = frames + fr * N;
    for (int n = tid; n < N; n += 256) dst[n] = r[n].x * (1.0f / (float)N) * hann_sin2(n, N);
}

// y[b][i] = (sum over frames covering sample i + N/2 of frames[b][t][i + N/2 - t hop]) / (sum of hann^2 over the same frames)
__global__ __launch_bounds__(256) void overlap_add_kernel(const float *__restrict__ frames, float *__restrict__ y, int B, int T, int N, int hop, int L)
{
    const int64_t total = (int64_t)B * L;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / L);
        const int n = (int)(i - (int64_t)b * L) + N / 2;
        int t1 = n / hop;
        if (t1 > T - 1) t1 = T - 1;
        int t0 = (n - N + hop) / hop;          // ceil((n - N + 1) / hop) for n - N + 1 > 0
        if (n - N + 1 <= 0) t0 = 0;
        float acc = 0.f, wss = 0.f;
        for (int t = t0; t <= t1; ++t) {
            const int k = n - t * hop;
            const float w = hann_sin2(k, N);
            acc += frames[((size_t)b * T + t) * N + k];
            wss += w * w;
        }
        y[i] = wss > 1.17549435e-38f ? acc / wss : acc;
    }
}

// X = rfft(hann * reflect-padded frame t of clip yb (L samples)): the frame into fft.b0, then its FFT.  The only place that forms
// such a frame, so every kernel that calls it forms the X that nsg_audio_stft returns.  The padded index is numpy's reflect map
// for every L >= 2, however short the signal is against N/2 (Griffin-Lim's grid is hop (T - 1) samples, a quarter of N/2 at
// T = 2 and hop = N/8).  L = 1 has no reflection (period 0): every launcher refuses it.
template <int LOG2N>
__device__ __forceinline__ v2f *stft_frame_lds(const float *__restrict__ yb, int t, int hop, int L, FftLds<LOG2N> &fft, int tid)
{
    constexpr int N = 1 << LOG2N;
    const int period = 2 * (L - 1);
    for (int n = tid; n < N; n += 256) {
        int idx = (t * hop + n - N / 2) % period;             // np.pad(mode="reflect"): the reflection has period 2 (L - 1) and
        if (idx < 0) idx += period;                           // folds as often as the padding needs (a grid shorter than N/2
        if (idx >= L) idx = period - idx;                     // folds more than once); the launchers guarantee L >= 2
        fft.b0[n] = v2f{yb[idx] * hann_sin2(n, N), 0.f};
    }
    return fft.transform(tid, false);
}

// What stft_kernel stores of X, one frame per workgroup:
//   STFT_RAW             spec = X                                           (nsg_audio_stft; S and prev are not read)
//   STFT_PHASE           spec = S X / |X|                                   (Griffin-Lim's phase update; X = 0 -> (S, 0))
//   STFT_MOMENTUM        t = X + momentum (X - prev);  prev <- X;  spec = S t / |t|   (fast Griffin-Lim: Perraudin, Balazs,
//                        Sondergaard 2013).  prev [B][T][F] is the caller's state buffer; each (frame, bin) is read and rewritten by
//                        the one thread that owns it, so the update is in place.
//   STFT_MOMENTUM_FIRST  the same with prev taken as 0 and not loaded (it may hold anything, NaN included), only stored.
enum StftOut { STFT_RAW, STFT_PHASE, STFT_MOMENTUM_FIRST, STFT_MOMENTUM };

template <int LOG2N, StftOut OUT>
__global__ __launch_bounds__(256) void stft_kernel(const float *__restrict__ y, const float *__restrict__ S, v2f *__restrict__ spec,
                                                   v2f *__restrict__ prev, int T, int hop, int L, int F, float momentum)
{
    __shared__ FftLds<LOG2N> fft;
    const int tid = threadIdx.x;
    const size_t fr = blockIdx.x;
    const int b = (int)(fr / T), t = (int)(fr - (size_t)b * T);
    fft.fill_twiddles(tid);
    v2f *r = stft_frame_lds<LOG2N>(y + (size_t)b * L, t, hop, L, fft, tid);
    for (int f = tid; f < F; f += 256) {
        const size_t i = fr * F + f;
        const v2f X = r[f];
        if constexpr (OUT == STFT_RAW) {
            spec[i] = X;
        } else {
            float tx = X.x, ty = X.y;
            if constexpr (OUT != STFT_PHASE) {
                const v2f P = OUT == STFT_MOMENTUM_FIRST ? v2f{0.f, 0.f} : prev[i];
                prev[i] = X;
                tx = X.x + momentum * (X.x - P.x), ty = X.y + momentum * (X.y - P.y);
            }
            const float mag = sqrtf(tx * tx + ty * ty);
            const float s = S[i];
            spec[i] = mag > 0.f ? v2f{s * tx / mag, s * ty / mag} : v2f{s, 0.f};   // np.angle(0) = 0
        }
    }
}

// The two sums of frame t of clip b behind the spectral convergence, in every thread: { sum_f (|X[f]| - S[f])^2, sum_f S[f]^2 } with
// |X| and the difference in fp32 (|X| as the phase kernels form it) and the squares and sums in fp64.  Order: thread tid adds its
// bins tid, tid + 256, ... to 0.0 in that order; the 256 thread sums are closed by nsg_block_sum_butterfly.  Barriers inside:
// called by all 256 threads from uniform control flow.  The spectrum never leaves LDS.
template <int LOG2N>
__device__ __forceinline__ void frame_convergence_sums(const float *__restrict__ yb, const float *__restrict__ Sf, int t, int hop, int L, int F,
                                                       FftLds<LOG2N> &fft, double *red, int tid, double &num, double &den)
{
    v2f *r = stft_frame_lds<LOG2N>(yb, t, hop, L, fft, tid);
    double a = 0.0, d = 0.0;
    for (int f = tid; f < F; f += 256) {
        const v2f X = r[f];
        const float s = Sf[f];
        const float e = sqrtf(X.x * X.x + X.y * X.y) - s;
        a += (double)e * (double)e;
        d += (double)s * (double)s;
    }
    num = nsg_block_sum_butterfly(a, red, tid);
    den = nsg_block_sum_butterfly(d, red, tid);
}

// one frame per workgroup: frame_sums[b][t] = frame_convergence_sums
template <int LOG2N>
__global__ __launch_bounds__(256) void convergence_frames_kernel(const float *__restrict__ y, const float *__restrict__ S, double *__restrict__ frame_sums,
                                                                 int T, int hop, int L, int F)
{
    __shared__ FftLds<LOG2N> fft;
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const size_t fr = blockIdx.x;
    const int b = (int)(fr / T), t = (int)(fr - (size_t)b * T);
    fft.fill_twiddles(tid);
    double num, den;
    frame_convergence_sums<LOG2N>(y + (size_t)b * L, S + fr * F, t, hop, L, F, fft, red, tid, num, den);
    if (tid == 0) { frame_sums[2 * fr] = num; frame_sums[2 * fr + 1] = den; }
}

// one clip per workgroup: clip_sums[b] = the frames' pairs summed over t.  Order: thread tid adds the frames tid, tid + 256, ... to
// 0.0 in that order; the 256 thread sums are closed by nsg_block_sum_butterfly.
__global__ __launch_bounds__(256) void convergence_clips_kernel(const double *__restrict__ frame_sums, double *__restrict__ clip_sums, int T)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const double *fs = frame_sums + (size_t)blockIdx.x * T * 2;
    double a = 0.0, d = 0.0;
    for (int t = tid; t < T; t += 256) { a += fs[2 * t]; d += fs[2 * t + 1]; }
    a = nsg_block_sum_butterfly(a, red, tid);
    d = nsg_block_sum_butterfly(d, red, tid);
    if (tid == 0) { clip_sums[2 * blockIdx.x] = a; clip_sums[2 * blockIdx.x + 1] = d; }
}

// The same clip sums without a frame_sums buffer: one clip per workgroup, its frames one after another, frame t's pair added by
// thread t % 256 -- the adds and their order are convergence_clips_kernel's, only the parallelism over the frames is lost.
template <int LOG2N>
__global__ __launch_bounds__(256) void convergence_serial_kernel(const float *__restrict__ y, const float *__restrict__ S, double *__restrict__ clip_sums,
                                                                 int T, int hop, int L, int F)
{
    __shared__ FftLds<LOG2N> fft;
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    fft.fill_twiddles(tid);
    double a = 0.0, d = 0.0;
    for (int t = 0; t < T; ++t) {
        double num, den;                                      // (the sums' barriers stand between a frame's last read of the FFT's buffers and the next load)
        frame_convergence_sums<LOG2N>(y + (size_t)b * L, S + ((size_t)b * T + t) * F, t, hop, L, F, fft, red, tid, num, den);
        if ((t & 255) == tid) { a += num; d += den; }
    }
    a = nsg_block_sum_butterfly(a, red, tid);
    d = nsg_block_sum_butterfly(d, red, tid);
    if (tid == 0) { clip_sums[2 * b] = a; clip_sums[2 * b + 1] = d; }
}

// y[n] = x[n] + k y[n-1] is a decaying recurrence: the influence of y[n-W] on y[n] is k^W.  Each thread owns a chunk of
// CH samples and starts the recurrence W samples earlier from zero, W chosen so that k^W < 1e-9 (605 samples for
// k = 0.97): the discarded warm-up makes the chunks independent to far below fp32 rounding.  out-of-place.
constexpr int PRE_CHUNK = 2048;
__global__ void inv_preemphasis_kernel(const float *__restrict__ x, float *__restrict__ y, int B, int L, float k, int warm)
{
    const int chunks = (L + PRE_CHUNK - 1) / PRE_CHUNK;
    const int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (id >= (int64_t)B * chunks) return;
    const int b = (int)(id / chunks), c = (int)(id - (int64_t)b * chunks);
    const float *px = x + (size_t)b * L;
    float *py = y + (size_t)b * L;
    const int n0 = c * PRE_CHUNK, n1 = min(L, n0 + PRE_CHUNK);
    float acc = 0.f;
    for (int n = max(0, n0 - warm); n < n0; ++n) acc = fmaf(k, acc, px[n]);
    for (int n = n0; n < n1; ++n) {
        acc = fmaf(k, acc, px[n]);
        py[n] = acc;
    }
}

// Per-row non-zero run [first, last] of the mel filterbank (a band matrix: each Slaney triangle covers one contiguous run of
// bins), passed by value: the launcher has checked the indices on the host, and no upload precedes the launch.
constexpr int MEL_MAX_ROWS = 128;
struct MelBands { int16_t first[MEL_MAX_ROWS], last[MEL_MAX_ROWS]; };
static_assert(2 * MEL_MAX_ROWS == 256, "melspectrogram_kernel: one thread per (frame of the pair, mel row)");

// wav -> normalised mel in one pass (audio_tacotron.py:70-78 with hparams_tacotron.py's settings): pre-emphasis evaluated at the
// reflect-mapped index, x periodic Hann, FFT, |X| kept in LDS, band product, dB, normalise, clip.  Only n_mels floats per frame
// reach HBM.  A workgroup owns frames 2q and 2q+1 of one clip and transforms them as the real and the imaginary part of ONE
// complex FFT (z = x0 + i x1; X0[f] = (Z[f] + conj Z[N-f]) / 2, X1[f] = (Z[f] - conj Z[N-f]) / 2i): half the FFTs, twiddle tables and
// barriers per frame.  Frame 2q+1 is zeros when the clip ends at 2q.  A frame's arithmetic depends on the clip's samples, its
// length and t alone (the partner is the clip's own neighbour), never on B, L or b.
template <int LOG2N>
__global__ __launch_bounds__(256) void melspectrogram_kernel(const float *__restrict__ wav, const int32_t *__restrict__ lengths,
                                                             const float *__restrict__ basis, const MelBands bands, float *__restrict__ out,
                                                             int T, int pairs, int hop, int L, int n_mels, float k, float min_amp, float min_db,
                                                             float ref_db, float max_abs, int frame_major)
{
    constexpr int N = 1 << LOG2N, F = N / 2 + 1;
    __shared__ FftLds<LOG2N> fft;
    __shared__ float mag[2][F];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)pairs), t0 = 2 * (int)(blockIdx.x - (unsigned)b * pairs);
    const int len = nsg_clip_len_reflect(lengths, b, L);      // (the caller checked N/2 < len <= L on its host copy)
    const int Tb = 1 + len / hop;                             // the clip's own frame count
    float *ob = out + (size_t)b * n_mels * T;
    const size_t m_stride = frame_major ? 1 : (size_t)T, t_stride = frame_major ? (size_t)n_mels : 1;
    const int j = tid >> 7, m = tid & (MEL_MAX_ROWS - 1);     // the output this thread owns: frame t0 + j, mel row m
    const bool owns = m < n_mels && t0 + j < T;
    if (t0 >= Tb) {                                           // past the clip's end: the collate's padding value
        if (owns) ob[(t0 + j) * t_stride + m * m_stride] = 0.f;
        return;
    }
    fft.fill_twiddles(tid);
    const float *x = wav + (size_t)b * L;
    const bool two = t0 + 1 < Tb;
    for (int n = tid; n < N; n += 256) {
        const float w = 0.5f - 0.5f * cospif(2.0f * (float)n / (float)N);
        float p[2] = {0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (q == 1 && !two) break;
            // np.pad(mode="reflect") of the pre-emphasised clip.  len > N/2 (checked by the launcher for L and by the caller for
            // lengths[]) and the padding is N/2 on each side: nsg_reflect_once's precondition.
            const int idx = nsg_reflect_once((t0 + q) * hop + n - N / 2, len);
            p[q] = idx > 0 ? x[idx] - k * x[idx - 1] : x[0];
        }
        fft.b0[n] = v2f{p[0] * w, p[1] * w};
    }
    v2f *r = fft.transform(tid, false);
    for (int f = tid; f < F; f += 256) {
        const v2f Z = r[f], C = r[(N - f) & (N - 1)];
        const float ar = Z.x + C.x, ai = Z.y - C.y;           // 2 X0[f]
        const float br = Z.y + C.y, bi = Z.x - C.x;           // 2 i X1[f] up to sign: the same modulus
        mag[0][f] = 0.5f * sqrtf(ar * ar + ai * ai);
        mag[1][f] = 0.5f * sqrtf(br * br + bi * bi);
    }
    __syncthreads();
    if (!owns) return;
    float v = 0.f;
    if (j == 0 || two) {
        const float *row = basis + (size_t)m * F;
        const float *mg = mag[j];
        const int f1 = bands.last[m];
        float acc = 0.f;
        for (int f = bands.first[m]; f <= f1; ++f) acc = fmaf(row[f], mg[f], acc);
        const float S = 20.f * log10f(fmaxf(min_amp, acc)) - ref_db;
        v = fminf(fmaxf(max_abs * ((S - min_db) / (-min_db)), 0.f), max_abs);
    }
    ob[(t0 + j) * t_stride + m * m_stride] = v;
}

// p[n] = x[n] - k x[n-1], p[0] = x[0] per clip (scipy.signal.lfilter([1, -k], [1], x)); out of place.
__global__ void preemphasis_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t total, int L, float k)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = i % L ? x[i] - k * x[i - 1] : x[i];
}

// nsg_audio_griffin_lim's workspace: the spectrum [B][T][F] | the frames [B][T][n_fft]
struct GriffinLimLayout { v2f *spec; float *frames; size_t bytes; };
inline GriffinLimLayout griffin_lim_layout(void *ws, int B, int T, int n_fft)
{
    const size_t F = (size_t)n_fft / 2 + 1;
    NsgCarver c(ws);
    return {c.take<v2f>(nsg_align_up((size_t)B * T * F * 2 * sizeof(float), 256)),
            c.take<float>(nsg_align_up((size_t)B * T * n_fft * sizeof(float), 256)), c.off};
}
inline int log2_of(int n) { int l = 0; while ((1 << l) < n) ++l; return (1 << l) == n ? l : -1; }

// The FFT sizes, n_fft in {512, 1024, 2048}, are enumerated here and nowhere else.  fft_size_log2 checks an entry point's n_fft and
// returns lg = log2(n_fft), or the refusal's (negative) code; with_fft_size(lg, fn) calls fn(std::integral_constant<int, lg>{}), whose
// type carries lg to a kernel's template argument.
int fft_size_log2(const char *name, int n_fft)
{
    const int lg = log2_of(n_fft);
    NSG_REQUIRE(lg >= 9 && lg <= 11, NSG_E_UNSUPPORTED, "%s: n_fft must be 512, 1024 or 2048", name);
    return lg;
}
template <class Fn>
void with_fft_size(int lg, Fn &&fn)
{
    if (lg == 9)       fn(std::integral_constant<int, 9>{});
    else if (lg == 10) fn(std::integral_constant<int, 10>{});
    else               fn(std::integral_constant<int, 11>{});
}

// one workgroup per frame (or pair of frames): B * T is a grid dimension
int frames_fit(const char *name, int B, int T)
{
    NSG_REQUIRE((int64_t)B * T < 0x7fffffff, NSG_E_UNSUPPORTED, "%s: too many frames (B * T >= 2^31)", name);
    return 0;
}

// The grid of nsg_audio_stft and nsg_audio_melspectrogram, T = 1 + L / hop frames of clips longer than the padding: lg, or the
// refusal's code.
int stft_grid(const char *name, int B, int L, int n_fft, int hop)
{
    const int lg = fft_size_log2(name, n_fft);
    if (lg < 0) return lg;
    NSG_REQUIRE(L > n_fft / 2, NSG_E_UNSUPPORTED, "%s: reflect padding needs more than n_fft/2 samples", name);
    const int rc = frames_fit(name, B, 1 + L / hop);
    return rc ? rc : lg;
}

// Griffin-Lim's grid, T frames over hop (T - 1) samples, as the four entry points on it take it (their pointer and sign checks
// have passed): lg, or the refusal's code.  reflects: the caller forms reflect-padded frames of the samples, so there must be two
// of them (SPSI forms none, and takes a single frame).  has_workspace: the caller takes nsg_audio_griffin_lim's workspace.
int griffin_lim_grid(const char *name, int B, int T, int n_fft, int hop, bool reflects, bool has_workspace, const void *workspace, size_t workspace_bytes)
{
    const int lg = fft_size_log2(name, n_fft);
    if (lg < 0) return lg;
    const int64_t L = (int64_t)hop * (T - 1);
    NSG_REQUIRE(n_fft % hop == 0, NSG_E_UNSUPPORTED, "%s: hop must divide n_fft", name);
    NSG_REQUIRE(L < 0x7fffffff, NSG_E_UNSUPPORTED, "%s: too many samples (hop * (T - 1) >= 2^31)", name);
    NSG_REQUIRE(!reflects || L >= 2, NSG_E_UNSUPPORTED, "%s: hop * (T - 1) must be at least 2 samples (a one-sample grid has no reflect padding)", name);
    if (const int rc = frames_fit(name, B, T)) return rc;
    NSG_REQUIRE(!has_workspace || (workspace && workspace_bytes >= griffin_lim_layout(nullptr, B, T, n_fft).bytes), NSG_E_WORKSPACE,
                "%s: workspace too small", name);
    return lg;
}

// Both Griffin-Lim entry points, under the caller's name: y_0 = istft(S exp(2 pi i u)), then per iteration the phase kernel and the
// istft.  momentum == 0 is the plain phase update, and c is not touched; otherwise c [B][T][F] complex is the state X_{i-1}, taken as
// 0 (and not loaded) in the first iteration.
int griffin_lim_run(const char *name, const float *S, const float *u, float *y, float *c, float momentum, int B, int T, int n_fft, int hop, int iters,
                    void *workspace, size_t workspace_bytes, hipStream_t s)
{
    NSG_REQUIRE(S && u && y && B > 0 && T > 1 && hop > 0 && iters >= 0, NSG_E_INVALID, "%s: bad argument", name);
    NSG_REQUIRE(momentum >= 0.f && momentum <= 1.f, NSG_E_INVALID, "%s: momentum must be in [0, 1]", name);      // (NaN fails both)
    NSG_REQUIRE(c || momentum == 0.f, NSG_E_INVALID, "%s: momentum > 0 needs the state buffer c", name);
    const int lg = griffin_lim_grid(name, B, T, n_fft, hop, true, true, workspace, workspace_bytes);
    if (lg < 0) return lg;
    const GriffinLimLayout G = griffin_lim_layout(workspace, B, T, n_fft);
    const int F = n_fft / 2 + 1;
    const int L = hop * (T - 1);
    v2f *prev = reinterpret_cast<v2f *>(c);
    const int64_t nspec = (int64_t)B * T * F;
    const unsigned nfr = (unsigned)(B * T);
    hipLaunchKernelGGL(init_phase_kernel, dim3(ew_blocks(nspec)), dim3(256), 0, s, S, u, G.spec, nspec);
    with_fft_size(lg, [&](auto lgc) {
        constexpr int LG = decltype(lgc)::value;
        auto istft = [&]() {
            hipLaunchKernelGGL((istft_frames_kernel<LG>), dim3(nfr), dim3(256), 0, s, G.spec, G.frames, F);
            hipLaunchKernelGGL(overlap_add_kernel, dim3(ew_blocks((int64_t)B * L)), dim3(256), 0, s, G.frames, y, B, T, n_fft, hop, L);
        };
        istft();
        for (int it = 0; it < iters; ++it) {
            if (momentum == 0.f) hipLaunchKernelGGL((stft_kernel<LG, STFT_PHASE>), dim3(nfr), dim3(256), 0, s, y, S, G.spec, prev, T, hop, L, F, momentum);
            else if (it == 0)    hipLaunchKernelGGL((stft_kernel<LG, STFT_MOMENTUM_FIRST>), dim3(nfr), dim3(256), 0, s, y, S, G.spec, prev, T, hop, L, F, momentum);
            else                 hipLaunchKernelGGL((stft_kernel<LG, STFT_MOMENTUM>), dim3(nfr), dim3(256), 0, s, y, S, G.spec, prev, T, hop, L, F, momentum);
            istft();
        }
    });
    return nsg_check_launch(name);
}

// ---- single-pass spectrogram inversion phases (include/nsg.h: nsg_audio_spsi_phases) ----
// Two launches.  spsi_frames_kernel, one workgroup per (clip, frame), does everything that does not depend on the frame before:
// peaks, their parabolic offsets, and for every bin the peak that owns it and that peak's advance (own + p) r.  spsi_walk_kernel,
// one workgroup per clip, is the sequential rest: phi_t[k] = frac(phi_{t-1}[own_t[k]] + adv_t[k]), one LDS gather and one add per
// bin and one barrier per frame, its operands loaded SPSI_AHEAD frames ahead.
//
// Ownership by two segmented scans over the bins, run together (Hillis-Steele in LDS, ceil(log2 F) steps whatever the frame holds,
// so the frame whose only peaks are bins 1 and F-2 costs what every other costs): forward, each bin learns the nearest peak at or
// below it and the least magnitude from that peak up to itself; backward, the nearest peak at or above and the least magnitude
// from itself up to that peak.  A bin k strictly between the peaks j < j' lies at or below the FIRST minimum of m[j .. j'] iff
// every magnitude in [j, k-1] is greater than the least of [k, j']:  min m[j .. k-1] > min m[k .. j'].
struct SpsiEl { int idx; float v; };      // the nearest peak seen so far (-1: none yet) and the least magnitude up to it

// nsg_audio_spsi_phases' workspace: the advances [B][T][F] fp64 | the owners [B][T][F] uint16.  It is carved from a workspace of
// nsg_audio_griffin_lim_workspace_bytes(B, T, n_fft) bytes, whose two sections are each at least as long as these two
// (8 F = 8 F and 4 n_fft = 8 F - 8 >= 2 F bytes per frame); the entry point checks it.
struct SpsiLayout { double *adv; uint16_t *own; size_t bytes; };
inline SpsiLayout spsi_layout(void *ws, int B, int T, int n_fft)
{
    const size_t F = (size_t)n_fft / 2 + 1;
    NsgCarver c(ws);
    return {c.take<double>(nsg_align_up((size_t)B * T * F * sizeof(double), 256)),
            c.take<uint16_t>(nsg_align_up((size_t)B * T * F * sizeof(uint16_t), 256)), c.off};
}

template <int LOG2N>
__global__ __launch_bounds__(256) void spsi_frames_kernel(const float *__restrict__ S, double *__restrict__ adv, uint16_t *__restrict__ own, double r)
{
    constexpr int F = (1 << LOG2N) / 2 + 1;
    __shared__ float m[F];
    __shared__ SpsiEl fw[2][F], bw[2][F];
    const int tid = threadIdx.x;
    const size_t row = (size_t)blockIdx.x * F;
    for (int k = tid; k < F; k += 256) m[k] = S[row + k];
    __syncthreads();
    for (int k = tid; k < F; k += 256) {
        const bool peak = k >= 1 && k <= F - 2 && m[k] > m[k - 1] && m[k] > m[k + 1];      // strict: a plateau, a NaN is no peak
        const SpsiEl e = {peak ? k : -1, m[k]};
        fw[0][k] = e;
        bw[0][k] = e;
    }
    __syncthreads();
    int cur = 0;
#pragma unroll 1
    for (int d = 1; d < F; d <<= 1) {
        for (int k = tid; k < F; k += 256) {
            SpsiEl a = fw[cur][k];
            if (a.idx < 0 && k >= d) { const SpsiEl l = fw[cur][k - d]; a.idx = l.idx; a.v = fminf(l.v, a.v); }
            fw[cur ^ 1][k] = a;
            SpsiEl b = bw[cur][k];
            if (b.idx < 0 && k + d < F) { const SpsiEl h = bw[cur][k + d]; b.idx = h.idx; b.v = fminf(b.v, h.v); }
            bw[cur ^ 1][k] = b;
        }
        __syncthreads();
        cur ^= 1;
    }
    const SpsiEl *L = fw[cur], *R = bw[cur];
    double *p = reinterpret_cast<double *>(fw[cur ^ 1]);      // the scans are done: their other buffer holds the peaks' offsets
    const bool any = L[F - 1].idx >= 0;
    for (int k = tid; k < F; k += 256)
        if (L[k].idx == k) {
            const double a = (double)m[k - 1], b = (double)m[k], c = (double)m[k + 1];
            p[k] = 0.5 * (a - c) / ((a - 2.0 * b) + c);
        }
    __syncthreads();
    for (int k = tid; k < F; k += 256) {
        int o = k;
        double a = (double)k * r;                               // a frame with no peak: every bin advances at its centre
        if (any) {
            const int lo = L[k].idx, hi = R[k].idx;
            if (lo == k || hi < 0) o = lo;
            else if (lo < 0) o = hi;
            else o = L[k - 1].v > R[k].v ? lo : hi;            // k - 1 >= lo: L[k - 1].v = min m[lo .. k - 1]
            a = ((double)o + p[o]) * r;
        }
        adv[row + k] = a;
        own[row + k] = (uint16_t)o;
    }
}

// Frames whose operands are in flight while one is applied.  The walk's loop body holds no branch: a bin index past F - 1 is
// clamped to F - 1 and a frame index past T - 1 to T - 1 (such lanes and loads repeat the last one's work, value for value), so the
// compiler can wait for exactly the oldest frame's loads (a counted vmcnt) and leave the younger ones in flight.  With a branch round
// a load it waits for all of them, and every frame then costs a trip to memory (1.42 us measured, against 0.35 us).
constexpr int SPSI_AHEAD = 8;

template <int LOG2N>
__global__ __launch_bounds__(256) void spsi_walk_kernel(const double *__restrict__ adv, const uint16_t *__restrict__ own, float *__restrict__ angles, int T)
{
    constexpr int F = (1 << LOG2N) / 2 + 1;
    constexpr int NB = (F + 255) / 256;                        // bins per thread: k = min(tid + 256 i, F - 1)
    __shared__ double phi[2][F];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * T * F;
    double a[SPSI_AHEAD][NB];
    int o[SPSI_AHEAD][NB];
    auto fetch = [&](int slot, int t) {
        const size_t at = base + (size_t)(t < T ? t : T - 1) * F;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int k = tid + 256 * i < F ? tid + 256 * i : F - 1;
            a[slot][i] = adv[at + k];
            o[slot][i] = own[at + k];
        }
    };
    auto apply = [&](int slot, int t) {                        // frame t, whose operands are in `slot`; t and slot have one parity
        const double *in = phi[slot & 1];
        double *out = phi[(slot & 1) ^ 1];
        float *dst = angles + base + (size_t)t * F;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int k = tid + 256 * i < F ? tid + 256 * i : F - 1;
            double v = in[o[slot][i]] + a[slot][i];
            v -= floor(v);
            out[k] = v;
            double w = v + 0.5 * (double)k;                     // (-1)^k of a centred symmetric window's transform
            w -= floor(w);
            const float f = (float)w;
            dst[k] = f == 1.0f ? 0.0f : f;
        }
    };
#pragma unroll
    for (int d = 0; d < SPSI_AHEAD; ++d) fetch(d, d);
    for (int k = tid; k < F; k += 256) phi[0][k] = 0.0;
    __syncthreads();
    int t0 = 0;
    for (; t0 + SPSI_AHEAD <= T; t0 += SPSI_AHEAD) {
#pragma unroll
        for (int d = 0; d < SPSI_AHEAD; ++d) {
            apply(d, t0 + d);
            fetch(d, t0 + d + SPSI_AHEAD);
            __syncthreads();
        }
    }
#pragma unroll
    for (int d = 0; d < SPSI_AHEAD; ++d) {                      // the last T mod SPSI_AHEAD frames: their operands are already here
        if (t0 + d >= T) break;
        apply(d, t0 + d);
        __syncthreads();
    }
}
static_assert(SPSI_AHEAD % 2 == 0, "spsi_walk_kernel: the ping-pong parity of frame t0 + d is d's");

}  // namespace

extern "C" {

int nsg_audio_mel_to_linear(const float *mel, const float *inv_basis, float *S, int32_t B, int32_t n_mels, int32_t T, int32_t F,
                            float min_level_db, float ref_level_db, float max_abs_value, float power, void *stream)
{
    NSG_REQUIRE(mel && inv_basis && S && B > 0 && n_mels > 0 && T > 0 && F > 0 && max_abs_value > 0.f, NSG_E_INVALID, "nsg_audio_mel_to_linear: bad argument");
    NSG_REQUIRE((int64_t)B * T < 0x7fffffff, NSG_E_UNSUPPORTED, "nsg_audio_mel_to_linear: too many frames");
    hipLaunchKernelGGL(mel_to_linear_kernel, dim3((unsigned)(B * T)), dim3(256), (size_t)n_mels * sizeof(float), (hipStream_t)stream, mel, inv_basis, S,
                       B, n_mels, T, F, min_level_db, ref_level_db, max_abs_value, power);
    return nsg_check_launch("mel_to_linear_kernel");
}

size_t nsg_audio_griffin_lim_workspace_bytes(int32_t B, int32_t T, int32_t n_fft)
{
    if (B <= 0 || T <= 0 || n_fft <= 0) return 0;
    return griffin_lim_layout(nullptr, B, T, n_fft).bytes;
}

// S [B][T][F] magnitudes, u [B][T][F] uniform numbers for the initial phases -> y [B][hop*(T-1)]
int nsg_audio_griffin_lim(const float *S, const float *u, float *y, int32_t B, int32_t T, int32_t n_fft, int32_t hop, int32_t iters,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    return griffin_lim_run("nsg_audio_griffin_lim", S, u, y, nullptr, 0.f, B, T, n_fft, hop, iters, workspace, workspace_bytes, (hipStream_t)stream);
}

// Griffin-Lim with momentum; the state X_{i-1} lives in the caller's c, the workspace is nsg_audio_griffin_lim's
int nsg_audio_griffin_lim_fast(const float *S, const float *u, float *y, float *c, int32_t B, int32_t T, int32_t n_fft, int32_t hop, int32_t iters,
                               float momentum, void *workspace, size_t workspace_bytes, void *stream)
{
    return griffin_lim_run("nsg_audio_griffin_lim_fast", S, u, y, c, momentum, B, T, n_fft, hop, iters, workspace, workspace_bytes, (hipStream_t)stream);
}

// S [B][T][F] magnitudes -> angles [B][T][F] in turns, what both Griffin-Lim entry points take as u
int nsg_audio_spsi_phases(const float *S, float *angles, int32_t B, int32_t T, int32_t n_fft, int32_t hop, void *workspace, size_t workspace_bytes,
                          void *stream)
{
    NSG_REQUIRE(S && angles && B > 0 && T > 0 && hop > 0, NSG_E_INVALID, "nsg_audio_spsi_phases: bad argument");
    const int lg = griffin_lim_grid("nsg_audio_spsi_phases", B, T, n_fft, hop, false, true, workspace, workspace_bytes);
    if (lg < 0) return lg;
    const SpsiLayout P = spsi_layout(workspace, B, T, n_fft);
    NSG_REQUIRE(P.bytes <= griffin_lim_layout(nullptr, B, T, n_fft).bytes, NSG_E_UNSUPPORTED,
                "nsg_audio_spsi_phases: the layout does not fit nsg_audio_griffin_lim's workspace");
    hipStream_t s = (hipStream_t)stream;
    const double r = (double)hop / (double)n_fft;      // a power of two: exact
    with_fft_size(lg, [&](auto lgc) {
        constexpr int LG = decltype(lgc)::value;
        hipLaunchKernelGGL((spsi_frames_kernel<LG>), dim3((unsigned)(B * T)), dim3(256), 0, s, S, P.adv, P.own, r);
        hipLaunchKernelGGL((spsi_walk_kernel<LG>), dim3((unsigned)B), dim3(256), 0, s, P.adv, P.own, angles, T);
    });
    return nsg_check_launch("spsi_phases");
}

// frame_sums [B][T][2] (may be NULL), clip_sums [B][2] fp64: the sums behind ||  |stft(y)| - S || / || S ||
int nsg_audio_spectral_convergence(const float *y, const float *S, double *frame_sums, double *clip_sums, int32_t B, int32_t T, int32_t n_fft,
                                   int32_t hop, void *stream)
{
    NSG_REQUIRE(y && S && clip_sums && B > 0 && T > 1 && hop > 0, NSG_E_INVALID, "nsg_audio_spectral_convergence: bad argument");
    const int lg = griffin_lim_grid("nsg_audio_spectral_convergence", B, T, n_fft, hop, true, false, nullptr, 0);
    if (lg < 0) return lg;
    hipStream_t s = (hipStream_t)stream;
    const int F = n_fft / 2 + 1;
    const int L = hop * (T - 1);
    with_fft_size(lg, [&](auto lgc) {
        constexpr int LG = decltype(lgc)::value;
        if (frame_sums) {
            hipLaunchKernelGGL((convergence_frames_kernel<LG>), dim3((unsigned)(B * T)), dim3(256), 0, s, y, S, frame_sums, T, hop, L, F);
            hipLaunchKernelGGL(convergence_clips_kernel, dim3((unsigned)B), dim3(256), 0, s, frame_sums, clip_sums, T);
        } else {
            hipLaunchKernelGGL((convergence_serial_kernel<LG>), dim3((unsigned)B), dim3(256), 0, s, y, S, clip_sums, T, hop, L, F);
        }
    });
    return nsg_check_launch("spectral_convergence");
}

// X [B][T][F] complex (interleaved re, im) = stft(y [B][L]) with T = 1 + L / hop frames (librosa.stft, centred, reflect, Hann)
int nsg_audio_stft(const float *y, float *X, int32_t B, int32_t L, int32_t n_fft, int32_t hop, void *stream)
{
    NSG_REQUIRE(y && X && B > 0 && L > 0 && hop > 0, NSG_E_INVALID, "nsg_audio_stft: bad argument");
    const int lg = stft_grid("nsg_audio_stft", B, L, n_fft, hop);
    if (lg < 0) return lg;
    const int T = 1 + L / hop, F = n_fft / 2 + 1;
    with_fft_size(lg, [&](auto lgc) {
        hipLaunchKernelGGL((stft_kernel<decltype(lgc)::value, STFT_RAW>), dim3((unsigned)(B * T)), dim3(256), 0, (hipStream_t)stream, y, (const float *)nullptr,
                           reinterpret_cast<v2f *>(X), (v2f *)nullptr, T, hop, L, F, 0.f);
    });
    return nsg_check_launch("stft");
}

int nsg_audio_inv_preemphasis(const float *x, float *y, int32_t B, int32_t L, float k, void *stream)
{
    NSG_REQUIRE(x && y && x != y && B > 0 && L > 0, NSG_E_INVALID, "nsg_audio_inv_preemphasis: bad argument (out of place)");
    NSG_REQUIRE(fabsf(k) < 1.f, NSG_E_UNSUPPORTED, "nsg_audio_inv_preemphasis: |k| must be below 1 (a decaying filter)");
    int warm = 0;
    if (k != 0.f) {
        const double w = ceil(log(1e-9) / log(fabs((double)k)));
        warm = w > (double)L ? L : (int)w;
    }
    const int64_t threads = (int64_t)B * nsg_cdiv(L, PRE_CHUNK);
    hipLaunchKernelGGL(inv_preemphasis_kernel, dim3((unsigned)nsg_cdiv(threads, 64)), dim3(64), 0, (hipStream_t)stream, x, y, B, L, k, warm);
    return nsg_check_launch("inv_preemphasis_kernel");
}

int nsg_audio_preemphasis(const float *x, float *y, int32_t B, int32_t L, float k, void *stream)
{
    NSG_REQUIRE(x && y && x != y && B > 0 && L > 0, NSG_E_INVALID, "nsg_audio_preemphasis: bad argument (out of place)");
    const int64_t total = (int64_t)B * L;
    hipLaunchKernelGGL(preemphasis_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, x, y, total, L, k);
    return nsg_check_launch("preemphasis_kernel");
}

int nsg_audio_melspectrogram(const float *wav, const int32_t *lengths, const float *basis, const int32_t *bands, float *out, int32_t B, int32_t L,
                             int32_t n_fft, int32_t hop, int32_t n_mels, float preemphasis, float min_level_db, float ref_level_db,
                             float max_abs_value, int32_t frame_major, void *stream)
{
    NSG_REQUIRE(wav && basis && bands && out && B > 0 && L > 0 && hop > 0 && n_mels > 0, NSG_E_INVALID, "nsg_audio_melspectrogram: bad argument");
    NSG_REQUIRE(max_abs_value > 0.f && min_level_db < 0.f && (frame_major == 0 || frame_major == 1), NSG_E_INVALID,
                "nsg_audio_melspectrogram: bad argument (max_abs_value > 0, min_level_db < 0, frame_major 0 or 1)");
    const int lg = stft_grid("nsg_audio_melspectrogram", B, L, n_fft, hop);
    if (lg < 0) return lg;
    NSG_REQUIRE(n_mels <= MEL_MAX_ROWS, NSG_E_UNSUPPORTED, "nsg_audio_melspectrogram: at most 128 mel bins");
    const int T = 1 + L / hop, F = n_fft / 2 + 1;
    MelBands mb;
    for (int m = 0; m < n_mels; ++m) {
        const int32_t f0 = bands[2 * m], f1 = bands[2 * m + 1];
        NSG_REQUIRE(f0 >= 0 && f0 < F && f1 >= 0 && f1 < F, NSG_E_INVALID, "nsg_audio_melspectrogram: band index outside [0, n_fft/2]");
        mb.first[m] = (int16_t)f0;
        mb.last[m] = (int16_t)f1;
    }
    for (int m = n_mels; m < MEL_MAX_ROWS; ++m) { mb.first[m] = 1; mb.last[m] = 0; }
    const float min_amp = (float)pow(10.0, (double)min_level_db / 20.0);
    hipStream_t s = (hipStream_t)stream;
    const int pairs = (T + 1) / 2;                 // a workgroup owns two frames of a clip
    const unsigned nwg = (unsigned)(B * pairs);
    with_fft_size(lg, [&](auto lgc) {
        hipLaunchKernelGGL((melspectrogram_kernel<decltype(lgc)::value>), dim3(nwg), dim3(256), 0, s, wav, lengths, basis, mb, out, T, pairs, hop, L, n_mels,
                           preemphasis, min_amp, min_level_db, ref_level_db, max_abs_value, frame_major);
    });
    return nsg_check_launch("melspectrogram_kernel");
}

}  // extern "C"
