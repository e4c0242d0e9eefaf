// A min-sum path over per-frame candidates: the kernel behind ops.f0_viterbi and audio.f0_track.  include/nsg.h states the
// arithmetic and its order (nsg_f0_viterbi); this file is how it is laid on the machine.  Nothing here knows of audio.
//
// f0_viterbi_kernel: a clip is a serial chain of T_b steps of at most 9 x 9 add-compares, bound by latency, so a clip gets one
// wave and the batch is the parallelism.  Lane k = 0 .. 8 owns state k: its D(t - 1, k) and logf'_k stay in its registers, and a
// step reads the nine D and eight logf' of frame t - 1 out of the other lanes with v_readlane_b32 (a constant lane each: no LDS
// round trip on the chain), j ascending with a strict <.  A state the frame does not have holds D = +inf and logf' = 0: fl(inf +
// trans) is never < the running minimum, which is the same as leaving it out.  The candidate rows come through LDS VT_CHUNK = 64
// frames at a time: all 64 lanes load the counts (one frame a lane, the next chunk's prefetched under the chain), then the
// slots below the counts, 8 a lane, coalesced, and store logf and local(t, k); a load per step on the chain would be its whole
// cost.  Slots past a count are not read.  A step's own three LDS reads (count, logf, local) are issued a step ahead.  Measured
// (DESIGN.md 5g): 372 ns a frame step, 0.32 ms for 64 clips of 862 frames.
//   back-pointers: lane k packs its own, 4 bits a frame, into a register and stores one 32-bit word per 8 frames at
//                  [t / 8][k] (9 words per 8 frames): no cross-lane packing.  LDS when T <= NSG_F0_VITERBI_LDS_FRAMES, else the
//                  workspace (a store per 8 frames, off the chain).
//   back-trace:    blocks of NSG_F0_VITERBI_LDS_FRAMES frames from the end: the block's words are in LDS (copied back from the
//                  workspace by all lanes where they went there), lane 0 walks them and records the states as bytes, then all
//                  lanes gather f0 and ap of the block's frames and store them coalesced.
#include "nsg_common.h"

namespace {

constexpr int VT_NC = NSG_F0_MAX_CANDIDATES;       // candidate slots of a frame
constexpr int VT_NS = VT_NC + 1;                   // states: unvoiced, then the slots
constexpr int VT_CHUNK = 64;                       // frames staged at a time: one count a lane
constexpr int VT_BLOCK = NSG_F0_VITERBI_LDS_FRAMES;    // frames whose back-pointers LDS holds
constexpr int VT_BLOCK_WORDS = VT_BLOCK / 8 * VT_NS;
static_assert(VT_NC == 8 && VT_NS <= 16, "a slot index is 3 bits of a staging index; a back-pointer is 4 bits");
static_assert(VT_BLOCK % 8 == 0, "a back-trace block starts on a word");

// nsg_f0_viterbi's workspace: the back-pointers [B][ceil(T / 8)][9] 32-bit words, word [w][k] holding state k's back-pointers of
// frames 8 w .. 8 w + 7, 4 bits each, frame 8 w in the low bits; nothing when T <= NSG_F0_VITERBI_LDS_FRAMES
struct ViterbiLayout { uint32_t *bp; size_t bytes; };
inline ViterbiLayout viterbi_layout(void *ws, int B, int T)
{
    NsgCarver c(ws);
    return {c.take<uint32_t>(T > VT_BLOCK ? nsg_align_up((size_t)B * ((T + 7) / 8) * VT_NS * sizeof(uint32_t), 256) : 0), c.off};
}

__device__ __forceinline__ float vt_lane(float v, int lane) { return nsg_bitsf((unsigned)__builtin_amdgcn_readlane((int)nsg_fbits(v), lane)); }
__device__ __forceinline__ int vt_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(64) void f0_viterbi_kernel(const float *__restrict__ cand_logf, const float *__restrict__ cand_ap,
                                                        const float *__restrict__ cand_f0, const int32_t *__restrict__ count,
                                                        const int32_t *__restrict__ frames, int32_t *__restrict__ state,
                                                        float *__restrict__ cost, float *__restrict__ f0, float *__restrict__ ap,
                                                        uint32_t *ws_bp, int T, float logf_top, float octave_cost, float jump_cost,
                                                        float vuv_cost, float unvoiced_cost)
{
    __shared__ float s_logf[VT_CHUNK * VT_NC], s_loc[VT_CHUNK * VT_NC];
    __shared__ int s_cnt[VT_CHUNK];
    __shared__ uint32_t s_bp[VT_BLOCK_WORDS];
    __shared__ uint8_t s_st[VT_BLOCK];
    const int b = blockIdx.x, k = threadIdx.x;
    const int Tb = vt_clamp(frames ? frames[b] : T, T);
    const int64_t row = (int64_t)b * T;
    uint32_t *gbp = ws_bp ? ws_bp + (int64_t)b * ((T + 7) / 8) * VT_NS : nullptr;
    const float inf = __builtin_inff();

    float D = inf, lprev = 0.f;                        // lane k: D(t - 1, k) and logf'_k
    uint32_t hist = 0;
    int cnext = k < Tb ? vt_clamp(count[row + k], VT_NC) : 0;
    for (int c0 = 0; c0 < Tb; c0 += VT_CHUNK) {
        const int nfr = Tb - c0 < VT_CHUNK ? Tb - c0 : VT_CHUNK;
        __syncthreads();                               // the chain is done with the chunk before
        s_cnt[k] = cnext;                              // (0 for a frame past the clip)
        __syncthreads();
        cnext = c0 + VT_CHUNK + k < Tb ? vt_clamp(count[row + c0 + VT_CHUNK + k], VT_NC) : 0;
#pragma unroll
        for (int m = 0; m < VT_NC; ++m) {
            const int i = k + 64 * m, tt = i >> 3;
            float l = 0.f, loc = 0.f;
            if (tt < nfr && (i & 7) < s_cnt[tt]) {
                const int64_t at = (row + c0) * VT_NC + i;
                l = cand_logf[at];
                const float up = logf_top - l;
                const float oc = octave_cost * up;
                loc = cand_ap[at] + oc;
            }
            s_logf[i] = l;
            s_loc[i] = loc;
        }
        __syncthreads();
        // a step's three LDS reads are issued a step ahead, unconditionally (a slot the frame does not have was staged as 0), so
        // that their latency lies under the step before and not on the chain
        const int ks = k >= 1 && k <= VT_NC ? k - 1 : 0;
        int cnt_n = s_cnt[0];
        float l_n = s_logf[ks], loc_n = s_loc[ks];
        for (int tt = 0; tt < nfr; ++tt) {
            const int t = c0 + tt;
            const int cnt = cnt_n;
            const bool voiced = k >= 1 && k <= cnt;
            const float myl = voiced ? l_n : 0.f;
            const float loc = k == 0 ? unvoiced_cost : loc_n;
            const int nt = tt + 1 < VT_CHUNK ? tt + 1 : tt;
            cnt_n = s_cnt[nt];
            l_n = s_logf[nt * VT_NC + ks];
            loc_n = s_loc[nt * VT_NC + ks];
            float Dn = loc;
            uint32_t arg = 0;
            if (t > 0) {
                float best = 0.f;
#pragma unroll
                for (int j = 0; j < VT_NS; ++j) {
                    const float Dj = vt_lane(D, j);
                    float tr;
                    if (j == 0) {
                        tr = k == 0 ? 0.f : vuv_cost;
                    } else {
                        const float d = myl - vt_lane(lprev, j);
                        const float jump = jump_cost * __builtin_fabsf(d);
                        tr = k == 0 ? vuv_cost : jump;
                    }
                    const float c = Dj + tr;
                    if (j == 0) {
                        best = c;
                    } else if (c < best) {
                        best = c;
                        arg = j;
                    }
                }
                Dn = loc + best;
            }
            D = (k == 0 || voiced) ? Dn : inf;
            lprev = myl;
            hist |= arg << (4 * (t & 7));
            if ((t & 7) == 7 || t == Tb - 1) {
                if (k < VT_NS) {
                    if (gbp) gbp[(t >> 3) * VT_NS + k] = hist;
                    else s_bp[(t >> 3) * VT_NS + k] = hist;
                }
                hist = 0;
            }
        }
    }

    // the end state: the smallest k that minimises D(T_b - 1, k) (a state the last frame does not have holds +inf)
    int s = 0;
    float best = 0.f;
    if (Tb > 0) {
        best = vt_lane(D, 0);
#pragma unroll
        for (int j = 1; j < VT_NS; ++j) {
            const float Dj = vt_lane(D, j);
            if (Dj < best) { best = Dj; s = j; }
        }
    }
    if (k == 0) cost[b] = best;

    for (int hi = Tb; hi > 0;) {                        // back-trace blocks, from the end
        const int lo = (hi - 1) / VT_BLOCK * VT_BLOCK;
        __syncthreads();                               // the forward pass's words are written; the block before is stored
        if (gbp) {
            const int w0 = lo / 8 * VT_NS, w1 = (hi + 7) / 8 * VT_NS;
            for (int i = k; i < w1 - w0; i += 64) s_bp[i] = gbp[w0 + i];
            __syncthreads();
        }
        if (k == 0) {
            for (int t = hi - 1; t >= lo; --t) {
                s_st[t - lo] = (uint8_t)s;
                if (t > 0) s = vt_clamp((int)(s_bp[((t - lo) >> 3) * VT_NS + s] >> (4 * (t & 7)) & 15u), VT_NC);
            }
        }
        s = __builtin_amdgcn_readfirstlane(s);
        __syncthreads();
        for (int t = lo + k; t < hi; t += 64) {
            const int st = s_st[t - lo];
            const int64_t at = (row + t) * VT_NC;
            float r_f0 = 0.f, r_ap = 1.f;
            if (st > 0) {
                r_f0 = cand_f0[at + st - 1];
                r_ap = cand_ap[at + st - 1];
            } else {
                const int cnt = vt_clamp(count[row + t], VT_NC);
                for (int j = 0; j < cnt; ++j) {
                    const float v = cand_ap[at + j];
                    if (j == 0 || v < r_ap) r_ap = v;
                }
            }
            state[row + t] = st;
            f0[row + t] = r_f0;
            ap[row + t] = r_ap;
        }
        hi = lo;
    }
    for (int t = Tb + k; t < T; t += 64) {
        state[row + t] = -1;
        f0[row + t] = 0.f;
        ap[row + t] = 1.f;
    }
}

inline bool vt_cost_ok(float v) { return v >= 0.f && v <= 3.4028234e38f; }     // finite and >= 0 (a NaN fails both)

}  // namespace

extern "C" {

size_t nsg_f0_viterbi_workspace_bytes(int32_t B, int32_t T)
{
    if (B < 1 || T < 1) return 0;
    return viterbi_layout(nullptr, B, T).bytes;
}

int nsg_f0_viterbi(const float *cand_logf, const float *cand_ap, const float *cand_f0, const int32_t *count, const int32_t *frames,
                   int32_t *state, float *cost, float *f0, float *ap, int32_t B, int32_t T, float logf_top, float octave_cost, float jump_cost,
                   float vuv_cost, float unvoiced_cost, void *workspace, size_t workspace_bytes, void *stream)
{
    NSG_REQUIRE(cand_logf && cand_ap && cand_f0 && count && state && cost && f0 && ap, NSG_E_INVALID, "nsg_f0_viterbi: null pointer");
    NSG_REQUIRE(B >= 1 && T >= 1, NSG_E_INVALID, "nsg_f0_viterbi: non-positive size (B = %d, T = %d)", B, T);
    NSG_REQUIRE(vt_cost_ok(octave_cost) && vt_cost_ok(jump_cost) && vt_cost_ok(vuv_cost) && vt_cost_ok(unvoiced_cost), NSG_E_INVALID,
                "nsg_f0_viterbi: a cost is negative or not finite (octave %g, jump %g, vuv %g, unvoiced %g)", (double)octave_cost,
                (double)jump_cost, (double)vuv_cost, (double)unvoiced_cost);
    NSG_REQUIRE(logf_top >= -3.4028234e38f && logf_top <= 3.4028234e38f, NSG_E_INVALID, "nsg_f0_viterbi: logf_top = %g is not finite",
                (double)logf_top);
    NSG_REQUIRE((int64_t)B * T < 0x7fffffffLL, NSG_E_UNSUPPORTED, "nsg_f0_viterbi: too many frames (B * T = %lld >= 2^31, outside the envelope)",
                (long long)B * T);
    const ViterbiLayout lay = viterbi_layout(workspace, B, T);
    NSG_REQUIRE(lay.bytes == 0 || (workspace && workspace_bytes >= lay.bytes), NSG_E_WORKSPACE, "nsg_f0_viterbi: workspace too small");
    hipLaunchKernelGGL(f0_viterbi_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, cand_logf, cand_ap, cand_f0, count, frames, state,
                       cost, f0, ap, lay.bytes ? lay.bp : nullptr, T, logf_top, octave_cost, jump_cost, vuv_cost, unvoiced_cost);
    return nsg_check_launch("f0_viterbi_kernel");
}

}  // extern "C"
