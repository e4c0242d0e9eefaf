// F0 tracking (YIN), the F0 candidates of a path finder, and F0 statistics along a warping path: the kernels behind audio.f0,
// audio.f0_candidates (audio.f0_track; the path finder itself is csrc/f0_track.hip) and audio.f0_distortion
// (evaluate.test_conversion_f0).  include/nsg.h states the arithmetic and its order; this file is how it is laid on the machine.
// f0_kernel and f0_candidates_kernel share their front half as code -- f0_tile, f0_difference, f0_normalise: the spans, d, the
// running sum, d' -- and the parabola (f0_refine); they differ in what they look for in d'.  f0_candidates_kernel's selection of
// the 8 strongest minima is a rank count (the comment at the kernel says why).
//
// f0_kernel: the work is W * tau_max subtract-square-add triples a frame out of a span of W + tau_max samples, VALU work fed from
// LDS.  A lane owns F0_RUN adjacent lags tau = F0_RUN g .. F0_RUN g + F0_RUN - 1 (lag 0 rides along: its d is 0 and is never
// read) and forms their sums with nsg_ssd_run (nsg_wave.h), the sliding register window tsm.hip's search calls too: a step of
// four j costs one 16-byte read of the next four samples (consecutive lanes 16 bytes apart, conflict-free) and one 16-byte read of
// x[s0 + j .. j + 3] at an address the frame's lanes share (a broadcast), for 4 * F0_RUN triples.  One fp32 chain per lag over j in
// order, so a lag's sum does not know which lane or workgroup formed it.  W is even, so of the loop's tails only {0, 2} are
// instantiated (F0_TAILS).  The loop is bound by the VALU issue rate (three uncontracted instructions a pair); build.py compiles
// this file with -fno-slp-vectorize, as nsg_wave.h asks.
// G = ceil((tau_max + 1) / F0_RUN) lanes serve a frame; a workgroup takes F = 256 / G adjacent frames of one clip (as many as
// F0_LDS_BUDGET holds), lane = (frame, run), so that few lanes idle (3 frames of 85 runs at tau_max = 339).  Each frame has its
// own span in LDS: frames with gaps between them (hop > W + tau_max) cost no more than adjacent ones.
//   LDS (floats, per frame):  sx [stride]  the span x[s0 .. s0 + W + F0_RUN G), zero outside the clip; stride = that rounded up
//                                          to 4, + 4: 16-byte rows, a frame's broadcast reads 4 banks from its neighbour's
//                             dl [F0_RUN G] d(tau), then d'(tau) in place
//                             gt [NG4]     the totals of the groups of 8 lags (nsg.h: NSG_F0_LAG_GROUP)
//                             ctl [2]      the first lag below the threshold; the bits of min d' (d' >= 0: its bits order as integers)
//                                          (f0_candidates_kernel: ctl [18]: the 8 kept keys by rank, the count of minima, a pad;
//                                          and the keys of all the frame's minima over sx, which is dead once d is formed)
// The tail (running sum, d', the search) is a thread per group of 8 lags: its own chain over the group, then its own chain over
// the earlier groups' totals (at most 127 adds); integer minima through LDS atomics (exact, order-free); the frame's first
// thread advances to the local minimum, refines and stores.
//
// f0_path_stats_kernel: one wave per pair, lane l the cells l, l + 64, ..., then nsg_wave_sum_butterfly (nsg_reduce.h).
#include "nsg_common.h"
#include "nsg_reduce.h"
#include "nsg_wave.h"

namespace {

constexpr int F0_RUN = 4;                          // adjacent lags a lane owns
constexpr unsigned F0_TAILS = 0b0101;              // W mod 4 is 0 or 2: f0_check refuses an odd frame_length
constexpr int F0_THREADS = 256;                    // lanes a workgroup shares among its frames (one frame may need more: F0_MAX_THREADS)
constexpr int F0_MAX_THREADS = 320;                // ceil((1024 + 1) / 4) = 257 runs, rounded up to whole waves
constexpr int F0_MIN_W = 64, F0_MAX_W = 2048, F0_MAX_TAU = 1024;
constexpr int F0_GROUP = NSG_F0_LAG_GROUP;
constexpr size_t F0_LDS_BUDGET = 60 * 1024;        // below the 64 KiB a kernel has without opting in
static_assert(F0_RUN % 4 == 0 && F0_RUN <= F0_GROUP, "16-byte window reads; a frame's runs are at least as many as its groups");
static_assert((F0_MAX_TAU + 1 + F0_RUN - 1) / F0_RUN <= F0_MAX_THREADS, "one frame's runs fit a workgroup");

struct F0Geom {
    int W, hop, tau_min, tau_max;
    int G;          // runs (lanes) of a frame
    int RG;         // F0_RUN * G >= tau_max + 1: lags a frame forms
    int stride;     // floats between the frames' spans
    int NG, NG4;    // groups of 8 lags; rounded up to 4
    int F;          // frames of a workgroup
    int tiles_t;    // workgroups of a clip
    int threads;
    int ctl;        // control words of a frame (F0_CTL of f0_kernel, F0C_CTL of f0_candidates_kernel)
};
constexpr int F0_CTL = 2;                          // the first lag below the threshold; the bits of min d'
constexpr int F0C_CTL = 2 * NSG_F0_MAX_CANDIDATES + 2;   // the kept keys (64 bits each, by rank); the count of minima; a pad to 8 bytes
inline size_t f0_frame_floats(const F0Geom &q) { return (size_t)q.stride + q.RG + q.NG4 + q.ctl; }

inline F0Geom f0_geom(int W, int hop, int tau_min, int tau_max, int T, int ctl)
{
    F0Geom q;
    q.W = W; q.hop = hop; q.tau_min = tau_min; q.tau_max = tau_max; q.ctl = ctl;
    q.G = (tau_max + 1 + F0_RUN - 1) / F0_RUN;
    q.RG = F0_RUN * q.G;
    q.stride = (W + q.RG + 3) / 4 * 4 + 4;
    q.NG = (tau_max + F0_GROUP - 1) / F0_GROUP;
    q.NG4 = (q.NG + 3) / 4 * 4;
    const int by_lanes = F0_THREADS / q.G, by_lds = (int)(F0_LDS_BUDGET / (f0_frame_floats(q) * sizeof(float)));
    q.F = by_lanes < by_lds ? by_lanes : by_lds;
    q.F = q.F > T ? T : q.F;
    q.F = q.F < 1 ? 1 : q.F;
    q.tiles_t = (T + q.F - 1) / q.F;
    q.threads = (q.F * q.G + 63) / 64 * 64;
    return q;
}

// ---- the front half both kernels run: a tile's place, its spans, d(tau), the running sum and d'(tau) -- stated here once ------
// A workgroup's tile and its sections of LDS; thread (f, g) is run g of frame f (act: f < F), then group g of frame f
struct F0Tile {
    float *sx, *dl, *gt;        // [F][stride], [F][RG], [F][NG4]
    int *ctl;                   // [F][q.ctl], 16-byte aligned (every section before it is a multiple of 4 floats a frame)
    int tid, nthr, b, t0, len, Tb, nf, f, g;
    bool act;
};
__device__ __forceinline__ F0Tile f0_tile(float *lds, const F0Geom &q, const int32_t *__restrict__ lengths, int L, int T)
{
    F0Tile m;
    m.sx = lds;
    m.dl = m.sx + q.F * q.stride;
    m.gt = m.dl + q.F * q.RG;
    m.ctl = reinterpret_cast<int *>(m.gt + q.F * q.NG4);
    m.tid = threadIdx.x; m.nthr = blockDim.x;
    m.b = blockIdx.x / q.tiles_t; m.t0 = (blockIdx.x - m.b * q.tiles_t) * q.F;
    m.len = nsg_clip_len(lengths, m.b, L);
    m.Tb = 1 + m.len / q.hop;
    m.nf = T - m.t0 < q.F ? T - m.t0 : q.F;            // frames of this tile inside the tensor
    m.f = m.tid / q.G; m.g = m.tid - m.f * q.G;
    m.act = m.f < q.F;
    return m;
}

// The spans, then d(tau) into dl; ends with the workgroup's barrier (which also publishes what the caller wrote to ctl before).
// DIRECT (the diagnostics library's switch, for scripts/f0_timing.py): the loop the sliding window replaces -- a lane's lags are
// g, g + G, ..., each pair reads its own x[s0 + j + tau] (consecutive lanes consecutive words) -- with the same chains, so the same bits.
template <bool DIRECT>
__device__ __forceinline__ void f0_difference(const F0Geom &q, const F0Tile &m, const float *__restrict__ wav, int L)
{
    float *sx = m.sx, *dl = m.dl;
    const int tid = m.tid, nthr = m.nthr;
    const float *xb = wav + (int64_t)m.b * L;
    const int S = q.W + q.RG;
    for (int f = 0; f < q.F; ++f) {                    // a frame's span, zero outside the clip and for frames past it
        const bool livef = f < m.nf && m.t0 + f < m.Tb;
        const int64_t s0 = (int64_t)(m.t0 + f) * q.hop - q.W / 2;
        for (int i = tid; i < q.stride; i += nthr) sx[f * q.stride + i] = nsg_clip_at(xb, s0 + i, m.len, livef && i < S);
    }
    __syncthreads();

    const int f = m.f, g = m.g;
    const bool act = m.act;
    if (act && DIRECT) {
        const float *base = sx + f * q.stride, *win = base + g;
        float acc[F0_RUN];
#pragma unroll
        for (int r = 0; r < F0_RUN; ++r) acc[r] = 0.f;
#pragma unroll 4
        for (int j = 0; j < q.W; ++j) {
            const float u = base[j];
#pragma unroll
            for (int r = 0; r < F0_RUN; ++r) {
                const float t = u - win[j + q.G * r];
                const float sq = t * t;
                acc[r] = acc[r] + sq;
            }
        }
#pragma unroll
        for (int r = 0; r < F0_RUN; ++r) dl[f * q.RG + g + q.G * r] = acc[r];
    } else if (act) {
        const float *base = sx + f * q.stride;         // x[s0 + j] at base[j]: the frame's lanes read it at one address
        const float *win = base + F0_RUN * g;          // x[s0 + j + tau0] at win[j], tau0 = F0_RUN g
        float acc[F0_RUN];                             // (W = 2 mod 4: the rows are long enough for the tail's reads)
        nsg_ssd_run<F0_RUN, F0_TAILS>(acc, win, base, q.W);
        float *dst = dl + f * q.RG + F0_RUN * g;
#pragma unroll
        for (int r = 0; r < F0_RUN; r += 4) {
            const v4f v = {acc[r], acc[r + 1], acc[r + 2], acc[r + 3]};
            *reinterpret_cast<v4f *>(dst + r) = v;
        }
    }
    __syncthreads();
}

// The running sum in nsg.h's order and d' over d in dl: thread (f, g), g < NG (grp), is group g of frame f, lags 8 g + 1 .. 8 g + 8,
// and keeps its own d' in dpv (lags past tau_max: not set).  The caller puts a barrier before anybody reads another thread's d'.
__device__ __forceinline__ void f0_normalise(const F0Geom &q, const F0Tile &m, bool grp, float (&dpv)[F0_GROUP])
{
    const int f = m.f, g = m.g;
    float dv[F0_GROUP], p[F0_GROUP];
    if (grp) {
        const float *d = m.dl + f * q.RG + F0_GROUP * g + 1;
        float run = 0.f;
#pragma unroll
        for (int r = 0; r < F0_GROUP; ++r) {
            const bool in = F0_GROUP * g + 1 + r <= q.tau_max;
            dv[r] = in ? d[in ? r : 0] : 0.f;
            run = r == 0 ? dv[0] : run + dv[r];
            p[r] = run;
        }
        m.gt[f * q.NG4 + g] = run;
    }
    __syncthreads();
    if (grp) {
        float G = 0.f;
        for (int k = 0; k < g; ++k) G = G + m.gt[f * q.NG4 + k];
        float *d = m.dl + f * q.RG + F0_GROUP * g + 1;
#pragma unroll
        for (int r = 0; r < F0_GROUP; ++r) {
            const int tau = F0_GROUP * g + 1 + r;
            if (tau <= q.tau_max) {
                const float c = G + p[r];
                const float num = dv[r] * (float)tau;
                const float dp = c > 0.f ? num / c : 1.f;
                d[r] = dp;
                dpv[r] = dp;
            }
        }
    }
}

// The parabola through d' at ts and its neighbours, under nsg.h's conditions and in its order: dp = the frame's d'(0 ..)
__device__ __forceinline__ void f0_refine(const float *dp, int ts, int tau_max, float sample_rate, float &r_f0, float &r_ap)
{
    const float bb = dp[ts];
    float delta = 0.f;
    if (ts - 1 >= 1 && ts + 1 <= tau_max) {
        const float a = dp[ts - 1], c = dp[ts + 1];
        const float two_b = 2.f * bb;
        const float den = (a - two_b) + c;
        if (a >= bb && c >= bb && den > 0.f) {
            const float diff = a - c;
            const float half = 0.5f * diff;
            delta = half / den;
        }
    }
    const float period = (float)ts + delta;
    r_f0 = sample_rate / period;
    r_ap = bb;
}

template <bool DIRECT>
__global__ __launch_bounds__(F0_MAX_THREADS) void f0_kernel(const float *__restrict__ wav, const int32_t *__restrict__ lengths,
                                                            float *__restrict__ f0, float *__restrict__ ap, int L, int T, F0Geom q,
                                                            float threshold, float sample_rate)
{
    extern __shared__ __attribute__((aligned(16))) float f0_lds[];
    const F0Tile m = f0_tile(f0_lds, q, lengths, L, T);
    int *ctl = m.ctl;                                  // [F][2]
    const int tid = m.tid, f = m.f, g = m.g;
    float *of = f0 + (int64_t)m.b * T + m.t0, *oa = ap + (int64_t)m.b * T + m.t0;
    if (m.t0 >= m.Tb) {                                // the whole tile is past the clip (uniform over the workgroup)
        for (int i = tid; i < m.nf; i += m.nthr) { of[i] = 0.f; oa[i] = 1.f; }
        return;
    }
    if (tid < q.F) { ctl[2 * tid] = 0x7fffffff; ctl[2 * tid + 1] = 0x7f800000; }
    f0_difference<DIRECT>(q, m, wav, L);

    const bool grp = m.act && g < q.NG;
    float dpv[F0_GROUP];
    f0_normalise(q, m, grp, dpv);
    if (grp) {
        int first = 0x7fffffff;
        float mn = __builtin_inff();
        bool any = false;
#pragma unroll
        for (int r = 0; r < F0_GROUP; ++r) {
            const int tau = F0_GROUP * g + 1 + r;
            if (tau <= q.tau_max && tau >= q.tau_min) {
                const float dp = dpv[r];
                any = true;
                mn = dp < mn ? dp : mn;
                if (dp < threshold && first == 0x7fffffff) first = tau;
            }
        }
        if (first != 0x7fffffff) atomicMin(&ctl[2 * f], first);
        if (any) atomicMin(reinterpret_cast<unsigned *>(&ctl[2 * f + 1]), nsg_fbits(mn));
    }
    __syncthreads();

    if (m.act && g == 0 && f < m.nf) {
        float r_f0 = 0.f, r_ap = 1.f;
        if (m.t0 + f < m.Tb) {
            const float *dp = m.dl + f * q.RG;
            int ts = ctl[2 * f];
            if (ts == 0x7fffffff) {
                r_ap = nsg_bitsf((unsigned)ctl[2 * f + 1]);
            } else {
                while (ts + 1 <= q.tau_max && dp[ts + 1] < dp[ts]) ++ts;
                f0_refine(dp, ts, q.tau_max, sample_rate, r_f0, r_ap);
            }
        }
        of[f] = r_f0;
        oa[f] = r_ap;
    }
}

// f0_candidates_kernel: the same front half, then the local minima of d' (nsg.h: nsg_audio_f0_candidates).  The top-8 selection is
// a RANK COUNT, not eight rounds of a 64-bit atomicMin: a group's thread appends its minima's keys bits(d') << 32 | tau (d' >= 0: they
// order as integers; a group of 8 lags holds at most 4) to the frame's list -- laid over the frame's span of samples, which is dead
// once d is formed -- at slots one LDS atomic add hands out; after a barrier each minimum counts the keys below its own (one 8-byte
// read a key, at an address the frame's threads share; a v_cmp_lt_u64 and an add), and the keys of rank < 8 go to slot rank.  A rank
// is a property of the set, so the order in which the slots were handed out does not show.  In the ISA this is two barriers and one
// returning atomic a thread; the eight rounds are sixteen barriers and eight ds_min_rtn_u64 that every holder of a minimum waits for.
// Then thread k of the frame refines the key of rank k and stores it at the count of kept lags below its own: ascending lag.
__global__ __launch_bounds__(F0_MAX_THREADS) void f0_candidates_kernel(const float *__restrict__ wav, const int32_t *__restrict__ lengths,
                                                                       float *__restrict__ cand_f0, float *__restrict__ cand_ap,
                                                                       float *__restrict__ cand_logf, int32_t *__restrict__ count, int L,
                                                                       int T, F0Geom q, float sample_rate)
{
    constexpr int NC = NSG_F0_MAX_CANDIDATES;
    extern __shared__ __attribute__((aligned(16))) float f0_lds[];
    const F0Tile m = f0_tile(f0_lds, q, lengths, L, T);
    const int tid = m.tid, f = m.f, g = m.g;
    const int64_t row0 = (int64_t)m.b * T + m.t0;
    if (m.t0 >= m.Tb) {                                // the whole tile is past the clip (uniform over the workgroup)
        for (int i = tid; i < m.nf * NC; i += m.nthr) { cand_f0[row0 * NC + i] = 0.f; cand_ap[row0 * NC + i] = 1.f; cand_logf[row0 * NC + i] = 0.f; }
        for (int i = tid; i < m.nf; i += m.nthr) count[row0 + i] = 0;
        return;
    }
    if (tid < q.F) m.ctl[F0C_CTL * tid + 2 * NC] = 0;
    f0_difference<false>(q, m, wav, L);

    const bool grp = m.act && g < q.NG;
    float dpv[F0_GROUP];
    f0_normalise(q, m, grp, dpv);
    __syncthreads();

    const bool live = m.act && f < m.nf && m.t0 + f < m.Tb;
    const float *dp = m.dl + (m.act ? f : 0) * q.RG;
    unsigned long long *list = reinterpret_cast<unsigned long long *>(m.sx + (m.act ? f : 0) * q.stride);   // at most tau_max / 2 + 1 keys <= stride / 2
    int *fctl = m.ctl + F0C_CTL * (m.act ? f : 0);
    unsigned long long *sel = reinterpret_cast<unsigned long long *>(fctl);
    unsigned mask = 0;                                 // bit r: lag 8 g + 1 + r is a candidate
    if (grp && live) {
        const int lo = q.tau_min > 2 ? q.tau_min : 2;
#pragma unroll
        for (int r = 0; r < F0_GROUP; ++r) {
            const int tau = F0_GROUP * g + 1 + r;
            if (tau >= lo && tau <= q.tau_max) {
                const float v = dpv[r];
                const bool right = tau == q.tau_max || v <= dp[tau < q.tau_max ? tau + 1 : tau];
                if (v < dp[tau - 1] && right && v < 1.f) mask |= 1u << r;
            }
        }
        if (mask) {
            int slot = atomicAdd(&fctl[2 * NC], __popc(mask));
#pragma unroll
            for (int r = 0; r < F0_GROUP; ++r)
                if (mask >> r & 1) list[slot++] = (unsigned long long)nsg_fbits(dpv[r]) << 32 | (unsigned)(F0_GROUP * g + 1 + r);
        }
    }
    __syncthreads();
    if (mask) {
        const int n = fctl[2 * NC];
#pragma unroll
        for (int r = 0; r < F0_GROUP; ++r)
            if (mask >> r & 1) {
                const unsigned long long key = (unsigned long long)nsg_fbits(dpv[r]) << 32 | (unsigned)(F0_GROUP * g + 1 + r);
                int rank = 0;
                for (int i = 0; i < n; ++i) rank += list[i] < key ? 1 : 0;
                if (rank < NC) sel[rank] = key;
            }
    }
    __syncthreads();

    if (m.act && f < m.nf) {
        int n = live ? fctl[2 * NC] : 0;
        n = n > NC ? NC : n;
        const int64_t row = (row0 + f) * NC;
        for (int k = g; k < NC; k += q.G) {
            if (k < n) {
                const int tau = (int)(unsigned)sel[k];
                int pos = 0;
                for (int j = 0; j < n; ++j) pos += (int)(unsigned)sel[j] < tau ? 1 : 0;
                float r_f0, r_ap;
                f0_refine(dp, tau, q.tau_max, sample_rate, r_f0, r_ap);
                cand_f0[row + pos] = r_f0;
                cand_ap[row + pos] = r_ap;
                cand_logf[row + pos] = (float)log2((double)r_f0);
            } else {
                cand_f0[row + k] = 0.f;
                cand_ap[row + k] = 1.f;
                cand_logf[row + k] = 0.f;
            }
        }
        if (g == 0) count[row0 + f] = n;
    }
}

__global__ __launch_bounds__(64) void f0_path_stats_kernel(const float *__restrict__ fa, const float *__restrict__ fb,
                                                           const int32_t *__restrict__ path, const int32_t *__restrict__ steps,
                                                           double *__restrict__ stats, int Ta, int Tb)
{
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int P = Ta + Tb - 1;
    int n = steps[pair];
    n = n < 0 ? 0 : (n > P ? P : n);                   // the caller's to get right; clamped so that no access leaves a buffer
    const int32_t *pp = path + (int64_t)pair * P * 2;
    const float *A = fa + (int64_t)pair * Ta, *Bv = fb + (int64_t)pair * Tb;
    double s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = 0.0;            // n_vv, n_a_only, n_b_only, then the six sums
    for (int c = lane; c < n; c += 64) {
        int i = pp[2 * c], j = pp[2 * c + 1];
        i = i < 0 ? 0 : (i > Ta - 1 ? Ta - 1 : i);
        j = j < 0 ? 0 : (j > Tb - 1 ? Tb - 1 : j);
        const float va = A[i], vb = Bv[j];
        const bool a_on = va > 0.f, b_on = vb > 0.f;
        if (a_on && b_on) {
            const double x = log2((double)va), y = log2((double)vb), d = x - y;
            s[0] += 1.0;
            s[3] += x;
            s[4] += y;
            s[5] += x * x;
            s[6] += y * y;
            s[7] += x * y;
            s[8] += d * d;
        } else if (a_on) {
            s[1] += 1.0;
        } else if (b_on) {
            s[2] += 1.0;
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = nsg_wave_sum_butterfly(s[k]);
    if (lane == 0) {
        double *o = stats + (int64_t)pair * 10;
        o[0] = (double)n;
#pragma unroll
        for (int k = 0; k < 9; ++k) o[1 + k] = s[k];
    }
}

}  // namespace

NSG_DIAG_SWITCH(int, g_f0_direct, 0)       // nsg_debug_set_f0_direct (diagnostics library only): 1 = the one-read-per-pair loop
#ifdef NSG_DIAG
extern "C" NSG_API void nsg_debug_set_f0_direct(int on) { g_f0_direct = on; }
#endif

// The refusals nsg_audio_f0 and nsg_audio_f0_candidates share, in nsg_audio_f0's order; threshold: null where there is none
static int f0_check(const char *fn, bool pointers, int B, int L, int frame_length, int hop, int tau_min, int tau_max, const float *threshold,
                    float sample_rate)
{
    NSG_REQUIRE(pointers, NSG_E_INVALID, "%s: null pointer", fn);
    NSG_REQUIRE(B >= 1 && L >= 1 && frame_length >= 1 && hop >= 1 && tau_min >= 1 && tau_max >= 1, NSG_E_INVALID,
                "%s: non-positive size (B = %d, L = %d, frame_length = %d, hop = %d, tau_min = %d, tau_max = %d)", fn, B, L, frame_length,
                hop, tau_min, tau_max);
    NSG_REQUIRE(!threshold || (*threshold > 0.f && *threshold <= 1.f), NSG_E_INVALID, "%s: threshold = %g not in (0, 1]", fn,
                threshold ? (double)*threshold : 0.0);
    NSG_REQUIRE(sample_rate > 0.f && sample_rate <= 3.0e38f, NSG_E_INVALID, "%s: sample_rate = %g not positive and finite", fn, (double)sample_rate);
    NSG_REQUIRE(frame_length % 2 == 0 && frame_length >= F0_MIN_W && frame_length <= F0_MAX_W, NSG_E_UNSUPPORTED,
                "%s: frame_length = %d is odd or outside [%d, %d]", fn, frame_length, F0_MIN_W, F0_MAX_W);
    NSG_REQUIRE(tau_min <= tau_max && tau_max <= F0_MAX_TAU, NSG_E_UNSUPPORTED, "%s: lags [%d, %d] outside 1 <= tau_min <= tau_max <= %d", fn,
                tau_min, tau_max, F0_MAX_TAU);
    NSG_REQUIRE((int64_t)B * (1 + L / hop) < 0x7fffffffLL, NSG_E_UNSUPPORTED, "%s: too many frames (B * T = %lld >= 2^31, outside the envelope)", fn,
                (long long)B * (1 + L / hop));
    return NSG_OK;
}

extern "C" {

int nsg_audio_f0(const float *wav, const int32_t *lengths, float *f0, float *ap, int32_t B, int32_t L, int32_t frame_length, int32_t hop,
                 int32_t tau_min, int32_t tau_max, float threshold, float sample_rate, void *stream)
{
    if (const int rc = f0_check("nsg_audio_f0", wav && f0 && ap, B, L, frame_length, hop, tau_min, tau_max, &threshold, sample_rate)) return rc;
    const int T = 1 + L / hop;
    const F0Geom q = f0_geom(frame_length, hop, tau_min, tau_max, T, F0_CTL);
    const size_t lds = (size_t)q.F * f0_frame_floats(q) * sizeof(float);
    hipLaunchKernelGGL(g_f0_direct ? f0_kernel<true> : f0_kernel<false>, dim3((unsigned)(B * q.tiles_t)), dim3(q.threads), lds,
                       (hipStream_t)stream, wav, lengths, f0, ap, L, T, q, threshold, sample_rate);
    return nsg_check_launch("f0_kernel");
}

int nsg_audio_f0_candidates(const float *wav, const int32_t *lengths, float *cand_f0, float *cand_ap, float *cand_logf, int32_t *count,
                            int32_t B, int32_t L, int32_t frame_length, int32_t hop, int32_t tau_min, int32_t tau_max, float sample_rate,
                            void *stream)
{
    if (const int rc = f0_check("nsg_audio_f0_candidates", wav && cand_f0 && cand_ap && cand_logf && count, B, L, frame_length, hop, tau_min,
                                tau_max, nullptr, sample_rate))
        return rc;
    const int T = 1 + L / hop;
    const F0Geom q = f0_geom(frame_length, hop, tau_min, tau_max, T, F0C_CTL);
    const size_t lds = (size_t)q.F * f0_frame_floats(q) * sizeof(float);
    hipLaunchKernelGGL(f0_candidates_kernel, dim3((unsigned)(B * q.tiles_t)), dim3(q.threads), lds, (hipStream_t)stream, wav, lengths, cand_f0,
                       cand_ap, cand_logf, count, L, T, q, sample_rate);
    return nsg_check_launch("f0_candidates_kernel");
}

int nsg_f0_path_stats(const float *f0_a, const float *f0_b, const int32_t *path, const int32_t *steps, double *stats, int32_t B, int32_t Ta,
                      int32_t Tb, void *stream)
{
    NSG_REQUIRE(f0_a && f0_b && path && steps && stats, NSG_E_INVALID, "nsg_f0_path_stats: null pointer");
    NSG_REQUIRE(B >= 1 && Ta >= 1 && Tb >= 1, NSG_E_INVALID, "nsg_f0_path_stats: non-positive size (B = %d, Ta = %d, Tb = %d)", B, Ta, Tb);
    NSG_REQUIRE((int64_t)Ta + Tb - 1 < (1LL << 30), NSG_E_UNSUPPORTED, "nsg_f0_path_stats: Ta + Tb - 1 = %lld outside [1, 2^30)",
                (long long)Ta + Tb - 1);
    hipLaunchKernelGGL(f0_path_stats_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, f0_a, f0_b, path, steps, stats, Ta, Tb);
    return nsg_check_launch("f0_path_stats_kernel");
}

}  // extern "C"
