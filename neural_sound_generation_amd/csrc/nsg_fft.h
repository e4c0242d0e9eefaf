// The in-LDS FFT of libnsg.so's audio kernels, stated once: audio.hip (STFT, Griffin-Lim, the mel front end) and stoi.hip (the
// intelligibility figures' spectral frames) include it, so a frame transformed in either is transformed by the same code.
// fp32, complex as float2.
#pragma once
#include "nsg_common.h"

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2f cmul(v2f a, v2f b) { return v2f{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// The LDS of a radix-2 Stockham FFT of N = 2^LOG2N points by 256 threads: declared __shared__ once per kernel, then
// fill_twiddles(tid) by all threads before the first transform (whose first barrier orders the fill).
template <int LOG2N>
struct FftLds {
    static constexpr int N = 1 << LOG2N;
    v2f b0[N], b1[N], tw[N / 2];      // the input, then ping-pong | tw[t] = exp(-2 pi i t / N), t < N/2

    __device__ __forceinline__ void fill_twiddles(int tid)
    {
        for (int t = tid; t < N / 2; t += 256) {
            float sn, cs;
            sincospif(-2.0f * (float)t / (float)N, &sn, &cs);
            tw[t] = v2f{cs, sn};
        }
    }

    // Transforms b0; returns the buffer holding the result.  inverse: conjugated twiddles (no 1/N scaling).
    __device__ v2f *transform(int tid, bool inverse)
    {
        v2f *in = b0, *out = b1;
#pragma unroll 1
        for (int s = 0; s < LOG2N; ++s) {
            const int Ns = 1 << s;
            __syncthreads();
            for (int j = tid; j < N / 2; j += 256) {
                const int k = j & (Ns - 1);
                v2f w = tw[k << (LOG2N - 1 - s)];
                if (inverse) w.y = -w.y;
                const v2f a = in[j];
                const v2f b = cmul(w, in[j + N / 2]);
                const int j0 = ((j >> s) << (s + 1)) + k;
                out[j0] = a + b;
                out[j0 + Ns] = a - b;
            }
            v2f *t = in; in = out; out = t;
        }
        __syncthreads();
        return in;
    }
};

}  // namespace
