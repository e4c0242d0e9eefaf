// The fixed-order reductions of libnsg.so, each shape stated once.  Results are bitwise reproducible, and a fused path returns
// the bits of the separate operators it replaces, because kernels that must agree call the SAME function here: the order of
// the adds is the function's, not a copy of it.  DESIGN.md ("Reduction shapes") lists the shapes and their users.
//
// Every helper that contains a barrier says so.  Such a helper is called by ALL threads of the block, from uniform control
// flow: threads with nothing to add pass a zero or `live = false`, they do not skip the call.  Blocks are 256 threads unless
// stated.  A helper that hands a result to one thread stores it through `dst` or calls `done(...)` in that thread (a lambda
// at the call site).
#pragma once
#include "nsg_common.h"

// Serial sum of n floats p[0], p[stride], p[2*stride], ... in index order.  The loads are issued 16 at a time (the finalize
// kernels are otherwise a chain of dependent global-load latencies); the adds stay in index order.
template <typename ACC>
__device__ __forceinline__ ACC nsg_strided_sum(const float *__restrict__ p, size_t stride, int n)
{
    ACC s = (ACC)0;
    int i = 0;
    for (; i + 16 <= n; i += 16) {
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = p[(size_t)(i + k) * stride];
#pragma unroll
        for (int k = 0; k < 16; ++k) s += (ACC)v[k];
    }
    if (i + 8 <= n) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(size_t)(i + k) * stride];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += (ACC)v[k];
        i += 8;
    }
    for (; i < n; ++i) s += (ACC)p[(size_t)i * stride];
    return s;
}

// ---- block sums of one double per thread --------------------------------------------------------------------------------------

// Four-then-walk.  Order: thread t < 64 forms ((p[t] + p[t+64]) + p[t+128]) + p[t+192]; thread 0 adds those 64 values to 0.0 in
// index order and stores the total to dst[blockIdx.x].  Two barriers, none on entry and none after the walk: a kernel that calls this twice
// puts a __syncthreads() between the calls (both calls use the one LDS array, and thread 0 may still be walking it).
__device__ __forceinline__ void nsg_block_sum_four_walk(double part, double *dst)
{
    __shared__ double red[256];
    red[threadIdx.x] = part;
    __syncthreads();
    if (threadIdx.x < 64) {
        double t = red[threadIdx.x] + red[threadIdx.x + 64] + red[threadIdx.x + 128] + red[threadIdx.x + 192];
        red[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 64; ++i) t += red[i];
        dst[blockIdx.x] = t;
    }
}

// Walk-256.  Order: thread 0 adds the 256 thread partials to 0.0 in thread order and calls done(total).  One barrier.
template <typename Done>
__device__ __forceinline__ void nsg_block_sum_walk256(double part, Done done)
{
    __shared__ double red[256];
    red[threadIdx.x] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 256; ++i) t += red[i];
        done(t);
    }
}

// The xor-butterfly over the 64 lanes of a wave: for off = 32, 16, ..., 1, v = op(v, the v of lane ^ off).  The result is in every
// lane.  No barrier, no LDS.
template <typename T, typename Op>
__device__ __forceinline__ T nsg_wave_butterfly(T v, Op op)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    return v;
}

// The butterfly's wave stage.  Order: nsg_wave_butterfly's, v + the other lane's (offsets 32, 16, ..., 1), in v's own precision.
__device__ __forceinline__ double nsg_wave_sum_butterfly(double v) { return nsg_wave_butterfly(v, [](double a, double b) { return a + b; }); }
__device__ __forceinline__ float nsg_wave_sum_butterfly(float v) { return nsg_wave_butterfly(v, [](float a, float b) { return a + b; }); }

// Butterfly.  Order: nsg_wave_sum_butterfly inside each wave, then the 4 wave totals through
// red[0..3] as ((w0 + w1) + w2) + w3.  The result is in every thread.  Two barriers (the second frees red for the next call).
__device__ __forceinline__ double nsg_block_sum_butterfly(double v, double *red, int tid)
{
    v = nsg_wave_sum_butterfly(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    const double r = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return r;
}

// ---- exact, order-free wave reductions ----------------------------------------------------------------------------------------

// The maximum / the minimum of the 64 lanes' values, in every lane (nsg_wave_butterfly: no barrier, no LDS).  A maximum or a
// minimum is the same number in any order, so these have no order to state; lanes with nothing to offer pass the identity.  The
// floating-point maxima are fmaxf / fmax: a NaN loses to any number.
__device__ __forceinline__ float nsg_wave_max(float v) { return nsg_wave_butterfly(v, [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ double nsg_wave_max(double v) { return nsg_wave_butterfly(v, [](double a, double b) { return fmax(a, b); }); }
__device__ __forceinline__ int nsg_wave_max(int v) { return nsg_wave_butterfly(v, [](int a, int b) { return b > a ? b : a; }); }
__device__ __forceinline__ int nsg_wave_min(int v) { return nsg_wave_butterfly(v, [](int a, int b) { return b < a ? b : a; }); }
__device__ __forceinline__ unsigned long long nsg_wave_min(unsigned long long v)
{
    return nsg_wave_butterfly(v, [](unsigned long long a, unsigned long long b) { return b < a ? b : a; });
}

// ---- closing sums over block or slab partials ---------------------------------------------------------------------------------

// One-wave closer (a block of 64 threads).  Order: lane l adds partial[l], partial[l + 64], ... to 0.0 in that order; lane 0
// adds the 64 lane sums to 0.0 in lane order and calls done(total).  One barrier.
template <typename Done>
__device__ __forceinline__ void nsg_wave_close_sum(const double *partial, int n, Done done)
{
    __shared__ double red[64];
    const int lane = threadIdx.x;
    double t = 0.0;
#pragma unroll 8
    for (int i = lane; i < n; i += 64) t += partial[i];
    red[lane] = t;
    __syncthreads();
    if (lane == 0) {
        double s = 0.0;
        for (int i = 0; i < 64; ++i) s += red[i];
        done(s);
    }
}

// L lanes per output over slabs, in double.  Thread tid works for the output tid / L as its lane j = tid % L.  col points at the
// output's element of slab 0, consecutive slabs are `stride` floats apart.  Order: lane j adds the contiguous run of slabs
// [j * per, min(nslab, (j + 1) * per)), per = ceil(nslab / L), through nsg_strided_sum<double>; lane 0 adds the L lane sums
// to 0.0 in lane order and calls done(total).  live = false for outputs past the end: their lanes add nothing, dereference
// nothing, and done is not called.  One barrier.
template <int L, typename Done>
__device__ __forceinline__ void nsg_lane_split_slab_sum(const float *__restrict__ col, size_t stride, int nslab, bool live, Done done)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int j = tid & (L - 1);
    double s = 0.0;
    if (live) {
        const int per = (nslab + L - 1) / L;
        const int b0 = j * per, b1 = min(nslab, b0 + per);
        if (b1 > b0) s = nsg_strided_sum<double>(col + (size_t)b0 * stride, stride, b1 - b0);
    }
    red[tid] = s;
    __syncthreads();
    if (j != 0 || !live) return;
    s = 0.0;
    for (int k = 0; k < L; ++k) s += red[tid + k];
    done(s);
}

// Split slab sum, in float: the closing sum of a weight gradient's block partials.  The block serves per_block = 256 / split
// outputs; thread tid works for output loc = tid % per_block as share sub = tid / per_block.  col and stride as above.
// Order: share `sub` adds the slabs [sub * chunk, min(nslab, (sub + 1) * chunk)), chunk = ceil(nslab / split), through
// nsg_strided_sum<float>; for split > 1 the threads of share 0 then add the shares to 0.f in share order.  Returns the
// total to the threads of share 0.  split is uniform over the block; for split > 1 there is one barrier, and with LOOPED a
// second one that frees the LDS array for a caller that comes round again.
template <bool LOOPED>
__device__ __forceinline__ float nsg_split_slab_sum(const float *__restrict__ col, size_t stride, int nslab, int split, bool live)
{
    __shared__ float red[256];
    const int per_block = 256 / split;
    const int tid = threadIdx.x;
    const int sub = tid / per_block, loc = tid - sub * per_block;
    float sacc = 0.f;
    if (live) {
        const int chunk = (nslab + split - 1) / split;
        const int s0 = sub * chunk, s1 = min(nslab, s0 + chunk);
        if (s1 > s0) sacc = nsg_strided_sum<float>(col + (size_t)s0 * stride, stride, s1 - s0);
    }
    if (split > 1) {
        red[tid] = sacc;
        __syncthreads();
        if (sub == 0) {
            sacc = 0.f;
            for (int k = 0; k < split; ++k) sacc += red[k * per_block + loc];
        }
        if (LOOPED) __syncthreads();
    }
    return sacc;
}

// ---- slab column fold, in float -----------------------------------------------------------------------------------------------

// The thread map of one [rows][C] slab of an [M][C] array, W channels per thread: thread (cg = tid % CW, rg = tid / CW) owns
// channels W * cg .. W * cg + W - 1 of the rows r0 + rg, r0 + rg + rgroups, ... < r1.  Threads past the last whole row group
// (active == false) own nothing.
template <int W>
struct NsgSlabMap {
    int CW, rgroups, cg, rg;
    bool active;
    int64_t r0, r1;
    __device__ __forceinline__ NsgSlabMap(int C, int64_t slab, int slab_rows, int64_t M)
    {
        const int tid = threadIdx.x;
        CW = C / W;
        rgroups = 256 / CW;
        cg = tid % CW;
        rg = tid / CW;
        active = rg < rgroups;
        r0 = slab * slab_rows;
        r1 = min(M, r0 + slab_rows);
    }
};

// Column totals of K quantities over the slab, in two steps that share red (K * 256 * W floats, free on entry).
// nsg_slab_park: an ACTIVE thread parks s[k], its W partial sums of quantity k, at red[k * 256 * W + (rg * CW + cg) * W + e].
// No barrier: a kernel calls it from the branch in which its active threads formed the sums.
template <int K, int W>
__device__ __forceinline__ void nsg_slab_park(const NsgSlabMap<W> &m, const float (&s)[K][W], float *red)
{
#pragma unroll
    for (int e = 0; e < W; ++e)
#pragma unroll
        for (int k = 0; k < K; ++k) red[k * 256 * W + (m.rg * m.CW + m.cg) * W + e] = s[k][e];
}
// nsg_slab_fold: one barrier (all threads call it), then thread tid < CW adds, for each of its channels tid * W + e, the row
// groups' parked sums to 0.f in group order and calls done(e, t) with t[k] the K totals.
template <int K, int W, typename Done>
__device__ __forceinline__ void nsg_slab_fold(const NsgSlabMap<W> &m, const float *red, Done done)
{
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < m.CW) {
#pragma unroll
        for (int e = 0; e < W; ++e) {
            float t[K];
#pragma unroll
            for (int k = 0; k < K; ++k) t[k] = 0.f;
            for (int g = 0; g < m.rgroups; ++g)
#pragma unroll
                for (int k = 0; k < K; ++k) t[k] += red[k * 256 * W + (g * m.CW + tid) * W + e];
            done(e, t);
        }
    }
}
