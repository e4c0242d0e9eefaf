// Pitch-synchronous overlap-add: the kernels behind audio.pitch_marks and audio.pitch_shift_psola.  include/nsg.h states the
// arithmetic and its order; this file is how it is laid on the machine.
//
// psola_marks_kernel (nsg_audio_pitch_marks): one wave per clip walks the chain of marks.  A step is one dependent search: the
// position of mark k + 1's range comes from mark k, so what a step costs is latency, not work -- a range is at most 1025 samples,
// 17 a lane.  Everything a step touches is therefore in LDS:
//   ring [2][PS_H]    the clip's samples of two adjacent halves of PS_H = 4096, half h in slot h & 1, zero outside the clip
//   per  [PS_FR]      the signed period of frame t in slot t & (PS_FR - 1): + P(n) of a voiced frame, - clamp(P_u) of an
//                     unvoiced one, so the fp64 division is done once per frame, off the chain
// and a step is: one LDS read (the period at m_k), integer arithmetic, the range's LDS reads (lane l reads lo + l, lo + l + 64,
// ...: consecutive banks; the maximum of the integer keys has no order to keep), six cross-lane steps, one fire-and-forget store.
// The live halves are base, base + 1.  Ranges start at most 2048 samples after one another (P <= 1024, alpha <= 1/2) and span at
// most 1025, so with "a step whose range starts in half base + 1 loads half base + 2" every range lies inside the live halves:
// by induction lo < (base + 1) PS_H + 2048 at every search.  That load is issued BEFORE the step's search into registers and
// stored to LDS after it (tsm.hip's scheme): no step waits on global memory.  A single wave needs no hardware barrier; the
// __syncthreads() are the fences that order its LDS writes and reads.
//
// psola_syn_kernel (nsg_audio_psola, first launch): the chain over the synthesis marks, a thread per clip, every clip of a wave
// side by side; the marks around a(j) and the ratios of the current and the next frame are kept in registers.
// psola_ola_kernel (second launch): a thread per output sample.
#include "nsg_common.h"
#include "nsg_reduce.h"
#include "nsg_wave.h"

namespace {

constexpr int PS_H = 4096, PS_RING = 2 * PS_H;         // samples of a half, of the ring
constexpr int PS_FR = 1024;                            // period slots: two live halves cover at most 2 PS_H / 16 + 2 frames
constexpr int PS_NPF = PS_H / 64;                      // samples of a half a lane carries
constexpr int PS_FPF = (PS_H / 16 + 2 + 63) / 64;      // periods of a half a lane carries
constexpr int PS_MIN_HOP = 16, PS_MAX_HOP = 1 << 20, PS_MAX_P = 1024, PS_MAX_ALPHA_DEN = 1 << 20;
constexpr int PS_TILE = 1024;                          // output samples of an overlap-add block

struct PsGeom {
    int L, T, hop, Pu, Pmin, Pmax, an;                 // Pu: clamp(P_u)
    float sr;
    FastDiv div_hop, div_ad;
};

__host__ __device__ __forceinline__ int ps_clamp(int p, int lo, int hi) { return !(p >= lo) ? lo : (p > hi ? hi : p); }
// G, H_max, G_s of nsg.h
inline int ps_min_gap(int Pmin, int an, int ad) { return Pmin - (int)((int64_t)an * Pmin / ad); }
inline int ps_max_gap(int Pmax, int an, int ad) { return Pmax + (int)((int64_t)an * Pmax / ad); }
inline int ps_min_syn_gap(int G)
{
    const int g = (int)__builtin_floor((double)G / 4.0 + 0.5);
    return g < 1 ? 1 : g;
}

__device__ __forceinline__ int ps_frame(int n, const PsGeom &g)
{
    const int t = nsg_div(n + g.hop / 2, g.div_hop);
    return t < g.T - 1 ? t : g.T - 1;
}
// + P of a voiced frame, - clamp(P_u) of an unvoiced one
__device__ __forceinline__ int ps_period(float f, const PsGeom &g)
{
    if (!(f > 0.f)) return -g.Pu;
    const double q = (double)g.sr / (double)f;
    const double v = floor(q + 0.5);
    if (!(v >= (double)g.Pmin)) return g.Pmin;
    if (v > (double)g.Pmax) return g.Pmax;
    return (int)v;
}

// half h of the clip, global -> registers: its samples and the periods of the frames its samples belong to ...
__device__ __forceinline__ void ps_fetch(float (&rx)[PS_NPF], int (&rp)[PS_FPF], int (&rt)[PS_FPF], const float *__restrict__ xb,
                                         const float *__restrict__ fb, int h, int len, const PsGeom &g, int lane)
{
    const int64_t s0 = (int64_t)h * PS_H;
#pragma unroll
    for (int k = 0; k < PS_NPF; ++k) rx[k] = nsg_clip_at(xb, s0 + k * 64 + lane, len);
    const int64_t tl = (s0 + g.hop / 2) / g.hop, th = (s0 + PS_H - 1 + g.hop / 2) / g.hop;
#pragma unroll
    for (int k = 0; k < PS_FPF; ++k) {
        const int64_t t = tl + k * 64 + lane;
        const int tc = (int)(t < g.T - 1 ? t : g.T - 1);          // the frames past the track are its last one
        rt[k] = t <= th ? tc : -1;
        rp[k] = ps_period(fb[tc], g);
    }
}
// ... registers -> LDS
__device__ __forceinline__ void ps_commit(float *ring, int *per, const float (&rx)[PS_NPF], const int (&rp)[PS_FPF], const int (&rt)[PS_FPF],
                                          int h, int lane)
{
    float *dst = ring + (h & 1) * PS_H;
#pragma unroll
    for (int k = 0; k < PS_NPF; ++k) dst[k * 64 + lane] = rx[k];
#pragma unroll
    for (int k = 0; k < PS_FPF; ++k)
        if (rt[k] >= 0) per[rt[k] & (PS_FR - 1)] = rp[k];
}

// the index of the greatest key over [lo, hi], 1 <= hi - lo + 1 <= 64 * 17, both inside the live halves
__device__ __forceinline__ int ps_search(const float *ring, int lo, int hi, int lane)
{
    unsigned long long best = 0;                       // below every key: a key's low word is >= 0xffffffff - 1087
    for (int i = lo + lane; i <= hi; i += 64) {
        const unsigned u = nsg_fbits(ring[i & (PS_RING - 1)]);
        const unsigned o = u & 0x80000000u ? ~u : u ^ 0x80000000u;
        const unsigned long long key = (unsigned long long)o << 32 | (0xffffffffu - (unsigned)(i - lo));
        best = key > best ? key : best;
    }
    best = nsg_wave_butterfly(best, [](unsigned long long a, unsigned long long b) { return b > a ? b : a; });
    return lo + (int)(0xffffffffu - (unsigned)best);
}

__global__ __launch_bounds__(64) void psola_marks_kernel(const float *__restrict__ wav, const int32_t *__restrict__ lengths,
                                                         const float *__restrict__ f0_in, int32_t *__restrict__ marks,
                                                         int32_t *__restrict__ n_marks, PsGeom g, int K_max)
{
    __shared__ float ring[PS_RING];
    __shared__ int per[PS_FR];
    const int lane = threadIdx.x, b = blockIdx.x;
    const int len = nsg_clip_len(lengths, b, g.L);
    const float *xb = wav + (int64_t)b * g.L;
    const float *fb = f0_in + (int64_t)b * g.T;
    int32_t *mb = marks + (int64_t)b * K_max;
    int k = 0;
    if (len > 0) {
        float rx[PS_NPF];
        int rp[PS_FPF], rt[PS_FPF];
        for (int h = 0; h < 2; ++h) {
            ps_fetch(rx, rp, rt, xb, fb, h, len, g, lane);
            ps_commit(ring, per, rx, rp, rt, h, lane);
        }
        __syncthreads();
        int base = 0;                                  // the live halves are base, base + 1
        {
            const int p0 = per[ps_frame(0, g) & (PS_FR - 1)];
            const int P0 = p0 < 0 ? -p0 : p0;
            const int m0 = ps_search(ring, 0, (P0 < len ? P0 : len) - 1, lane);
            if (lane == 0) mb[0] = m0;
            k = 1;
            int m = m0;
            while (k < K_max) {
                const int pp = per[ps_frame(m, g) & (PS_FR - 1)];
                int lo, hi;
                if (pp > 0) {
                    const int d = nsg_div(g.an * pp, g.div_ad);
                    lo = m + pp - d;
                    hi = m + pp + d;
                    hi = hi < len - 1 ? hi : len - 1;
                } else {
                    lo = hi = m - pp;
                }
                if (lo > len - 1) break;
                const bool adv = lo >= (base + 1) * PS_H;            // uniform over the wave
                if (adv) ps_fetch(rx, rp, rt, xb, fb, base + 2, len, g, lane);       // in flight while this range is searched
                m = pp > 0 ? ps_search(ring, lo, hi, lane) : lo;
                if (lane == 0) mb[k] = m;
                ++k;
                if (adv) {
                    __syncthreads();
                    ps_commit(ring, per, rx, rp, rt, base + 2, lane);
                    ++base;
                    __syncthreads();
                }
            }
        }
    }
    if (lane == 0) n_marks[b] = k;
    for (int i = k + lane; i < K_max; i += 64) mb[i] = -1;
}

// a clip's marks as the two kernels below read them: the count and every mark clamped, so that no access leaves a buffer
struct PsMarks {
    const int32_t *m;
    int K, len;
    __device__ __forceinline__ int at(int a) const { return ps_clamp(m[a], 0, len - 1); }
};
__device__ __forceinline__ PsMarks ps_marks(const int32_t *__restrict__ marks, const int32_t *__restrict__ n_marks, int b, int K_max, int len)
{
    PsMarks r;
    r.m = marks + (int64_t)b * K_max;
    r.len = len;
    r.K = len > 0 ? ps_clamp(n_marks[b], 0, K_max) : 0;
    return r;
}

__global__ __launch_bounds__(64) void psola_syn_kernel(const int32_t *__restrict__ lengths, const float *__restrict__ f0_in,
                                                       const float *__restrict__ f0_out, const int32_t *__restrict__ marks,
                                                       const int32_t *__restrict__ n_marks, int32_t *__restrict__ syn,
                                                       int32_t *__restrict__ map, int32_t *__restrict__ n_syn, PsGeom g, int B, int K_max,
                                                       int J_max)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int len = nsg_clip_len(lengths, b, g.L);
    const PsMarks mk = ps_marks(marks, n_marks, b, K_max, len);
    const float *fi = f0_in + (int64_t)b * g.T, *fo = f0_out + (int64_t)b * g.T;
    int32_t *sb = syn + (int64_t)b * J_max, *ab = map + (int64_t)b * J_max;
    int j = 0;
    if (mk.K > 0) {
        const int last = mk.at(mk.K - 1);
        // the marks a - 1 .. a + 2 and the ratios of frames tc, tc + 1 ride in registers: a step waits for a load only when s
        // jumps more than a frame (the mark two ahead and the next frame's ratio are asked for a step before they are used)
        int s = mk.at(0), a = 0;
        int m_prev = 0, m_a = s, m_n = mk.K > 1 ? mk.at(1) : 0, m_nn = mk.K > 2 ? mk.at(2) : 0;
        auto ratio = [&](int t) {
            const float vi = fi[t], vo = fo[t];
            double r = 1.0;
            if (vi > 0.f && vo > 0.f) {
                r = (double)vo / (double)vi;
                r = r < 0.25 ? 0.25 : (r > 4.0 ? 4.0 : (r == r ? r : 1.0));
            }
            return r;
        };
        int tc = -2;
        double r0 = 1.0, r1 = 1.0;
        while (j < J_max) {
            sb[j] = s;
            ab[j] = a;
            ++j;
            const int D = mk.K == 1 ? g.Pu : (a < mk.K - 1 ? m_n - m_a : m_a - m_prev);
            const int t = ps_frame(s, g);
            if (t == tc + 1) {
                r0 = r1;
                r1 = ratio(t + 1 < g.T ? t + 1 : g.T - 1);
            } else if (t != tc) {
                r0 = ratio(t);
                r1 = ratio(t + 1 < g.T ? t + 1 : g.T - 1);
            }
            tc = t;
            const double q = floor((double)D / r0 + 0.5);
            const int64_t s2 = (int64_t)s + (q >= 1.0 ? (int64_t)q : 1);
            if (s2 > last) break;
            s = (int)s2;
            while (a + 1 < mk.K) {                     // nearest mark, the smaller on a tie
                const int64_t d0 = (int64_t)m_a - s, d1 = (int64_t)m_n - s;
                if (!((d1 < 0 ? -d1 : d1) < (d0 < 0 ? -d0 : d0))) break;
                ++a;
                m_prev = m_a;
                m_a = m_n;
                m_n = m_nn;
                m_nn = a + 2 < mk.K ? mk.at(a + 2) : 0;
            }
        }
    }
    n_syn[b] = j;
    for (int i = j; i < J_max; ++i) sb[i] = ab[i] = -1;
}

__device__ __forceinline__ float ps_window(int dist, int half)
{
    const float u = (float)dist / (float)half;
    const float t2 = 2.f * u;
    const float t3 = 3.f - t2;
    const float uu = u * u;
    const float p = uu * t3;
    return 1.f - p;
}

__global__ __launch_bounds__(256) void psola_ola_kernel(const float *__restrict__ wav, const int32_t *__restrict__ lengths,
                                                        const int32_t *__restrict__ marks, const int32_t *__restrict__ n_marks,
                                                        const int32_t *__restrict__ syn, const int32_t *__restrict__ map,
                                                        const int32_t *__restrict__ n_syn, float *__restrict__ out, int L, int K_max,
                                                        int J_max, int H_max, int tiles)
{
    const int b = blockIdx.x / tiles, n0 = (blockIdx.x - b * tiles) * PS_TILE;
    const int len = nsg_clip_len(lengths, b, L);
    const PsMarks mk = ps_marks(marks, n_marks, b, K_max, len);
    const int J = mk.K > 0 ? ps_clamp(n_syn[b], 0, J_max) : 0;
    const float *xb = wav + (int64_t)b * L;
    const int32_t *sb = syn + (int64_t)b * J_max, *ab = map + (int64_t)b * J_max;
    float *ob = out + (int64_t)b * L;
    const float floor_w = 1.f / (float)(1 << NSG_PSOLA_MIN_WEIGHT_LOG2);
    for (int n = n0 + threadIdx.x; n < n0 + PS_TILE && n < L; n += 256) {
        float v = 0.f;
        if (n < len) {
            int lo = 0, hi = J;                        // the first j with s_j > n - H_max
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)sb[mid] > (int64_t)n - H_max) hi = mid; else lo = mid + 1;
            }
            float num = 0.f, den = 0.f;
            for (int j = lo; j < J; ++j) {
                const int s = sb[j];
                if ((int64_t)s >= (int64_t)n + H_max) break;
                const int a = ps_clamp(ab[j], 0, mk.K - 1), ma = mk.at(a);
                const int dist = n - s;
                float w = 1.f;
                bool hit = dist == 0;
                if (dist < 0) {
                    const int hl = a > 0 ? ma - mk.at(a - 1) : 0;
                    hit = -dist < hl;
                    if (hit) w = ps_window(-dist, hl);
                } else if (dist > 0) {
                    const int hr = a < mk.K - 1 ? mk.at(a + 1) - ma : 0;
                    hit = dist < hr;
                    if (hit) w = ps_window(dist, hr);
                }
                if (hit) {
                    const float wx = w * nsg_clip_at(xb, (int64_t)ma + dist, len);
                    num = num + wx;
                    den = den + w;
                }
            }
            v = den >= floor_w ? num / den : xb[n];
        }
        ob[n] = v;
    }
}

// the refusals the two entry points share, in nsg.h's order; *g receives the launch constants
int psola_check(const char *name, bool pointers, int B, int L, int T, int hop, float sr, int Pu, int Pmin, int Pmax, int an, int ad, int K_max,
                const int *J_max, PsGeom *g)
{
    NSG_REQUIRE(pointers, NSG_E_INVALID, "%s: null pointer", name);
    NSG_REQUIRE(B >= 1 && L >= 1 && T >= 1 && hop >= 1, NSG_E_INVALID, "%s: non-positive size (B = %d, L = %d, T = %d, hop = %d)", name, B, L, T, hop);
    NSG_REQUIRE(sr > 0.f && sr <= 3.4e38f, NSG_E_INVALID, "%s: sample_rate = %g is not a positive finite number", name, (double)sr);
    NSG_REQUIRE(Pu >= 1, NSG_E_INVALID, "%s: unvoiced period P_u = %d < 1", name, Pu);
    NSG_REQUIRE(an >= 0 && ad >= 1, NSG_E_INVALID, "%s: alpha = %d / %d is not a ratio >= 0", name, an, ad);
    NSG_REQUIRE(hop >= PS_MIN_HOP && hop <= PS_MAX_HOP, NSG_E_UNSUPPORTED, "%s: hop = %d outside [%d, %d]", name, hop, PS_MIN_HOP, PS_MAX_HOP);
    NSG_REQUIRE(Pmin >= 2 && Pmin <= Pmax && Pmax <= PS_MAX_P, NSG_E_UNSUPPORTED, "%s: periods [%d, %d] are not inside [2, %d]", name, Pmin, Pmax,
                PS_MAX_P);
    NSG_REQUIRE(2 * (int64_t)an <= ad && ad <= PS_MAX_ALPHA_DEN, NSG_E_UNSUPPORTED, "%s: alpha = %d / %d above 1 / 2, or its denominator above %d", name,
                an, ad, PS_MAX_ALPHA_DEN);
    NSG_REQUIRE((int64_t)B * L < 0x7fffffffLL && L < 0x7fffffff - (1 << 21), NSG_E_UNSUPPORTED,
                "%s: B * L = %lld >= 2^31 or L > 2^31 - 2^21, outside the envelope", name, (long long)B * L);
    const int G = ps_min_gap(Pmin, an, ad);
    NSG_REQUIRE(K_max >= nsg_cdiv(L, G), NSG_E_INVALID, "%s: K_max = %d below ceil(L / G) = %lld (G = %d)", name, K_max, (long long)nsg_cdiv(L, G), G);
    if (J_max) {
        const int Gs = ps_min_syn_gap(G);
        NSG_REQUIRE(*J_max >= nsg_cdiv(L, Gs), NSG_E_INVALID, "%s: J_max = %d below ceil(L / G_s) = %lld (G_s = %d)", name, *J_max,
                    (long long)nsg_cdiv(L, Gs), Gs);
        NSG_REQUIRE((int64_t)B * *J_max < 0x7fffffffLL, NSG_E_UNSUPPORTED, "%s: B * J_max >= 2^31", name);
    }
    NSG_REQUIRE((int64_t)B * K_max < 0x7fffffffLL, NSG_E_UNSUPPORTED, "%s: B * K_max >= 2^31", name);
    g->L = L; g->T = T; g->hop = hop; g->Pu = ps_clamp(Pu, Pmin, Pmax); g->Pmin = Pmin; g->Pmax = Pmax; g->an = an; g->sr = sr;
    g->div_hop = nsg_fastdiv((uint32_t)hop);
    g->div_ad = nsg_fastdiv((uint32_t)ad);
    return NSG_OK;
}

}  // namespace

extern "C" {

int nsg_audio_pitch_marks(const float *wav, const int32_t *lengths, const float *f0_in, int32_t *marks, int32_t *n_marks, int32_t B, int32_t L,
                          int32_t T, int32_t hop, float sample_rate, int32_t P_u, int32_t P_min, int32_t P_max, int32_t alpha_num,
                          int32_t alpha_den, int32_t K_max, void *stream)
{
    PsGeom g;
    if (const int rc = psola_check("nsg_audio_pitch_marks", wav && f0_in && marks && n_marks, B, L, T, hop, sample_rate, P_u, P_min, P_max, alpha_num,
                                   alpha_den, K_max, nullptr, &g))
        return rc;
    hipLaunchKernelGGL(psola_marks_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, wav, lengths, f0_in, marks, n_marks, g, K_max);
    return nsg_check_launch("psola_marks_kernel");
}

int nsg_audio_psola(const float *wav, const int32_t *lengths, const float *f0_in, const float *f0_out, const int32_t *marks, const int32_t *n_marks,
                    int32_t *syn, int32_t *map, int32_t *n_syn, float *out, int32_t B, int32_t L, int32_t T, int32_t hop, float sample_rate,
                    int32_t P_u, int32_t P_min, int32_t P_max, int32_t alpha_num, int32_t alpha_den, int32_t K_max, int32_t J_max, void *stream)
{
    PsGeom g;
    if (const int rc = psola_check("nsg_audio_psola", wav && f0_in && f0_out && marks && n_marks && syn && map && n_syn && out, B, L, T, hop,
                                   sample_rate, P_u, P_min, P_max, alpha_num, alpha_den, K_max, &J_max, &g))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(psola_syn_kernel, dim3((unsigned)nsg_cdiv(B, 64)), dim3(64), 0, s, lengths, f0_in, f0_out, marks, n_marks, syn, map, n_syn, g,
                       B, K_max, J_max);
    const int tiles = (int)nsg_cdiv(L, PS_TILE);
    hipLaunchKernelGGL(psola_ola_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, s, wav, lengths, marks, n_marks, syn, map, n_syn, out, L, K_max,
                       J_max, ps_max_gap(P_max, alpha_num, alpha_den), tiles);
    return nsg_check_launch("psola_kernels");
}

}  // extern "C"
