// What the waveform kernels (audio.hip, resample.hip, f0.hip, tsm.hip) share, each piece stated once: a clip's length as a kernel
// may use it, the zero-padded and the reflect-padded read, and the sliding-window sum of squared differences behind YIN's d(tau)
// and WSOLA's search.  As in nsg_reduce.h, kernels that must agree call the SAME function here: the order of the adds is the
// function's, not a copy of it.  DESIGN.md 3.3.1 lists the helpers and their users.
//
// A file that calls nsg_ssd_run is compiled with -fno-slp-vectorize (build.py: SOURCE_FLAGS): the loop is scalar subtract /
// multiply / add triples on adjacent registers, and packed into v_pk_add_f32 / v_pk_mul_f32 by the SLP vectoriser it pays for the
// register shuffles -- f0_kernel 1.3 x slower, tsm_chain_kernel 7 - 9 % slower at the default sizes.  The bits
// do not depend on the flag; the speed does.
#pragma once
#include "nsg_common.h"

// ---- a clip's length ------------------------------------------------------------------------------------------------------------
// Clip b of a batch of rows of L samples has lengths[b] of them (lengths == nullptr: L).  lengths is the caller's to get right
// (nsg.h); a kernel uses it clamped, so that no read leaves the row whatever it holds.

// Clamped to [0, L]: for kernels that read zeros outside the clip.
__device__ __forceinline__ int nsg_clip_len(const int32_t *__restrict__ lengths, int b, int L)
{
    const int len = lengths ? lengths[b] : L;
    return len < 0 ? 0 : (len > L ? L : len);
}

// Clamped to [1, L]: for kernels that reflect-pad (nsg_reflect_once), which need a sample to reflect onto.  Precondition L >= 1.
__device__ __forceinline__ int nsg_clip_len_reflect(const int32_t *__restrict__ lengths, int b, int L)
{
    const int len = lengths ? lengths[b] : L;
    return len < 1 ? 1 : (len > L ? L : len);
}

// ---- padded reads ---------------------------------------------------------------------------------------------------------------
// x[at] for 0 <= at < len, +0.f elsewhere; x is the clip's row, len <= the row's length.  The load is unconditional, at x[0] for a
// position outside the clip -- a select, no branch around the load -- so len = 0 still needs a readable x[0] (every caller's row
// has L >= 1 samples).  live: a caller's own condition on top (a frame past the clip, an index past the range): false reads +0.f.
__device__ __forceinline__ float nsg_clip_at(const float *__restrict__ x, int64_t at, int len, bool live = true)
{
    const bool in = live && at >= 0 && at < len;
    return in ? x[in ? at : 0] : 0.f;
}

// np.pad(mode="reflect")'s index map for a clip of len samples, folded ONCE at each end: idx < 0 -> -idx, then idx >= len ->
// 2 (len - 1) - idx.  Precondition: the padding is shorter than len, i.e. -len < idx < 2 len - 1; then one fold is the exact map
// and the final clamp to [0, len - 1] is never taken (it only keeps a read inside the row when the precondition is broken; shorter
// clips need the periodic map of audio.hip's stft_frame_lds).  len >= 1.  I is the caller's index width, int or int64_t: 2 len must
// fit it.
template <typename I>
__device__ __forceinline__ I nsg_reflect_once(I idx, int len)
{
    if (idx < 0) idx = -idx;
    if (idx >= len) idx = 2 * ((I)len - 1) - idx;
    return idx < 0 ? 0 : (idx >= len ? (I)len - 1 : idx);
}

// ---- the sliding-window sum of squared differences ------------------------------------------------------------------------------
// acc[r] = sum over j = 0 .. n - 1, in that order, of (ref[j] - win[j + r])^2,  r = 0 .. RUN - 1
// for the RUN adjacent offsets a lane owns: one fp32 chain per offset, each term t = ref[j] - win[j + r], sq = t * t, acc = acc + sq
// (three roundings, nothing contracted), starting from +0.f.  So an offset's sum does not know which lane formed it, nor RUN.
//
// On the machine: the lane keeps the RUN + 3 window samples that four consecutive j need in registers; a step of four j costs one
// 16-byte read of ref (every lane at one address: a broadcast), one read of the next four window samples, and 4 RUN triples -- the
// one-read-per-pair loop would pay 4 RUN reads.  Window reads are 16-byte where RUN % 4 == 0 and 8-byte pairs for RUN = 2.
//
// TAILS: bit k set = n mod 4 may be k (bit 0 always).  The n mod 4 last j are one more such step cut short; only the remainders
// TAILS names are instantiated, so a caller whose n is even ({0, 2}: 0b0101) carries no code for 1 and 3.  n mod 4 outside TAILS
// breaks the precondition: the sum is then over some other remainder of TAILS.
// Preconditions: ref 16-byte aligned; win 4 RUN-byte aligned (16 for RUN % 4 == 0); with n4 = n rounded DOWN to 4, ref[0 .. n4 + 4)
// and win[0 .. RUN + n4 + 4) are readable when n mod 4 != 0 (ref[0 .. n), win[0 .. RUN + n) otherwise): what is read past the sum's
// own samples is not used.
template <int RUN>
__device__ __forceinline__ void nsg_ssd_load4(const float *p, float *o)
{
    if (RUN % 4 == 0) {
        const v4f v = *reinterpret_cast<const v4f *>(p);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else {                                           // RUN = 2: the lane's window is 8-byte aligned
        const nsg_v2f a = *reinterpret_cast<const nsg_v2f *>(p), b = *reinterpret_cast<const nsg_v2f *>(p + 2);
        o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
    }
}

// NJ consecutive j from j0 for a lane's RUN offsets: w[0 .. RUN + NJ - 1) holds win[j0 ...], u the NJ samples ref[j0 ...]
template <int RUN, int NJ>
__device__ __forceinline__ void nsg_ssd_step(float (&acc)[RUN], const float (&w)[RUN + 4], const float (&u)[4])
{
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
        for (int r = 0; r < RUN; ++r) {
            const float t = u[jj] - w[jj + r];
            const float sq = t * t;
            acc[r] = acc[r] + sq;
        }
}

template <int RUN, unsigned TAILS>
__device__ __forceinline__ void nsg_ssd_run(float (&acc)[RUN], const float *win, const float *ref, int n)
{
    static_assert(RUN == 2 || RUN % 4 == 0, "window reads are 8-byte pairs (RUN = 2) or 16-byte");
    static_assert((TAILS & 1) && TAILS < 16, "TAILS: a set of remainders mod 4 that holds 0");
    constexpr bool T1 = TAILS >> 1 & 1, T2 = TAILS >> 2 & 1, T3 = TAILS >> 3 & 1;
    // The sums stay in the function's own s[] and are copied out at the end.  Accumulated through the reference, the same
    // instructions are scheduled with the wait for a step's last read at its 23rd instead of its 58th: 0.8 % slower at
    // f0_kernel's largest shape.
    float s[RUN], w[RUN + 4], u[4];
#pragma unroll
    for (int r = 0; r < RUN; ++r) s[r] = 0.f;
    if (RUN == 2) {
        const nsg_v2f v = *reinterpret_cast<const nsg_v2f *>(win);
        w[0] = v.x; w[1] = v.y;
    } else {
#pragma unroll
        for (int r = 0; r < RUN; r += 4) nsg_ssd_load4<RUN>(win + r, &w[r]);
    }
    int j0 = 0;
    for (; j0 + 4 <= n; j0 += 4) {
        nsg_ssd_load4<4>(ref + j0, u);
        nsg_ssd_load4<RUN>(win + j0 + RUN, &w[RUN]);
        nsg_ssd_step<RUN, 4>(s, w, u);
#pragma unroll
        for (int r = 0; r < RUN; ++r) w[r] = w[r + 4];
    }
    if ((T1 || T2 || T3) && j0 < n) {
        nsg_ssd_load4<4>(ref + j0, u);
        nsg_ssd_load4<RUN>(win + j0 + RUN, &w[RUN]);
        constexpr int LAST = T3 ? 3 : (T2 ? 2 : 1);    // the largest remainder TAILS names needs no test: with one, none is made
        const int rem = n - j0;
        if (T1 && LAST != 1 && rem == 1) nsg_ssd_step<RUN, 1>(s, w, u);
        else if (T2 && LAST != 2 && rem == 2) nsg_ssd_step<RUN, 2>(s, w, u);
        else nsg_ssd_step<RUN, LAST>(s, w, u);
    }
#pragma unroll
    for (int r = 0; r < RUN; ++r) acc[r] = s[r];
}
