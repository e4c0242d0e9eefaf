// Incremental sampling of the latent prior (GatedPixelCNN, src/models.py:285-341): the per-row COLUMN WALK.
//
// Row i of the code grid is sampled in two phases (prior.py, GatedPixelCNN.sample).  The row pass -- the vertical stacks, their
// gates and the vertical-to-horizontal 1x1s of every layer for all W columns of row i -- depends only on rows < i and runs
// on the conv kernels of the main path.  What is left depends on the columns before j of the same row: per layer the
// horizontal stack (1 x k//2+1 taps, the last one masked for layer 0), the gate with the vertical contribution and the class
// row, the residual 1x1; then the output head (1x1 -> ReLU -> 1x1) and the choice of the code.  That chain is this kernel.
//
// One workgroup (1024 threads) owns a slice of up to NC clips and walks the whole row, j = 0 .. W-1, with no inter-workgroup communication.
// Every matrix-vector product is y[c][n] = bias[n] + sum_k Wt[k][n] x[c][k] with Wt the transposed (k-major) weights read
// from the packed blob (L2-resident across positions) and x in LDS.  The partition of (n, k) over the threads depends
// only on the layer's (N, K), never on how many clips share the workgroup, and the reduction over k-slices is in a fixed
// order: a clip's arithmetic is the same in any batch, and the result is deterministic.  fp32 throughout.
#include "nsg_common.h"
#include <math.h>
#include <type_traits>

namespace {

constexpr int NC = 4;          // clips per workgroup (one wave per clip for the choice of the code)
constexpr int THREADS = 1024;
constexpr int SMAX = 8;        // k-slices per output at most (the slices' partials are summed serially)
constexpr int HEAD = 512;      // output_conv's hidden width (fixed by the module)
constexpr int RED = 4096;      // per-clip partial-sum slots: S * N <= THREADS * 4 for every product (see matvec_partial)
constexpr int CKMAX = 16;      // codes per lane of the pick at most: ceil(1024 / 64)

struct WalkArgs {
    const float *w;          // packed weights (layout: nsg_prior_walk_weight_floats in include/nsg.h)
    const float *emb;        // [K][dim]
    const float *cond;       // [L][B][2 dim]
    const float *vh;         // [L][B][W][2 dim]  v2h(h_vert) of row `row`, bias included
    const float *u;          // [B][H][W] or null (teacher-forced)
    const int64_t *x_in;     // [B][H][W] or null (sampling)
    int64_t *codes;          // [B][H][W] or null
    float *e_row;            // embedding of row `row`'s codes, clip b at e_row + b * e_clip_stride, [W][dim]
    int64_t e_clip_stride;
    float *logits;           // [B][H][W][K] or null
    int B, H, W, dim, L, K, Kp, row;
};

struct WalkCtlArgs : WalkArgs {   // nsg_prior_walk_ctl: u and codes are set; x_in and keep come together
    const uint8_t *keep;     // [B][H][W] or null: where non-zero the code is x_in's
    float inv_t;             // 1 / temperature
    int top_k;               // 0 = off
    float top_p;             // 1 = off
};

struct WalkCfgArgs : WalkCtlArgs {   // nsg_prior_walk_cfg: B even, clips 2p (conditional) and 2p + 1 (unconditional) are pair p;
    float guidance;                  // u, x_in, keep and codes are [B / 2][H][W], one entry per pair
};

// Partial sums of y[c][n] for n < N (N % 4 == 0), k < Kd, into red[(s * NC + c) * N + n], s = the thread's k-slice
// (S <= SMAX slices of consecutive k, each summed in k order).
// x[c][k] is read from up to three LDS segments of `seglen` floats each (segment k / seglen), clip c at +c * cs.
__device__ __forceinline__ int matvec_partial(const float *__restrict__ Wt, int ldw, int N, int Kd, const float *const *seg,
                                              int seglen, int cs, float *red)
{
    const int G = N >> 2;                       // groups of 4 outputs
    int S = THREADS / G;
    if (S > SMAX) S = SMAX;
    if (S < 1) S = 1;
    if (S > Kd) S = Kd;
    const int chunk = (Kd + S - 1) / S;
    for (int t = threadIdx.x; t < G * S; t += THREADS) {
        const int g = t % G, s = t / G;
        const int k0 = s * chunk, k1 = min(Kd, k0 + chunk);
        v4f acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = v4f{0.f, 0.f, 0.f, 0.f};
        int k = k0;
        while (k < k1) {
            const int si = k / seglen, q0 = k - si * seglen;
            const int n_ = min(k1 - k, seglen - q0);
            const float *xs = seg[si] + q0;
            const float *wp = Wt + (size_t)k * ldw + 4 * g;
            int q = 0;
            for (; q + 8 <= n_; q += 8) {            // 8 weight loads in flight before their FMAs (L2 latency)
                v4f w8[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) w8[r] = *reinterpret_cast<const v4f *>(wp + (size_t)(q + r) * ldw);
#pragma unroll
                for (int r = 0; r < 8; ++r) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) acc[c] += w8[r] * xs[c * cs + q + r];
                }
            }
            for (; q < n_; ++q) {
                const v4f w4 = *reinterpret_cast<const v4f *>(wp + (size_t)q * ldw);
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[c] += w4 * xs[c * cs + q];
            }
            k += n_;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) *reinterpret_cast<v4f *>(red + (s * NC + c) * N + 4 * g) = acc[c];
    }
    return S;
}

// bias[n] + the k-slices' partials in slice order
__device__ __forceinline__ float reduce_out(const float *red, int S, int N, int c, int n, float bias)
{
    float v = 0.f;
    for (int s = 0; s < S; ++s) v += red[(s * NC + c) * N + n];
    return v + bias;
}

// fp32 as an unsigned key of the same order (finite values and infinities)
__device__ __forceinline__ uint32_t order_key(float f)
{
    uint32_t b = __float_as_uint(f);
    if (b == 0x80000000u) b = 0;                 // -0 orders as +0, as the comparison of the values has it
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The sum over the wave of per-lane counts n <= CKMAX < 32: one ballot per bit of n, no cross-lane data movement
__device__ __forceinline__ int wave_count(int n)
{
    int s = 0;
#pragma unroll
    for (int b = 0; b < 5; ++b) s += __popcll(__ballot((n >> b) & 1)) << b;
    return s;
}

// The sum of the 64 lanes' values (every lane active) in a fixed order, the same bits in every lane: within rows of 16 lanes by
// DPP (pairs, quads, row_shr:4, row_shr:8 leave the row's sum in its lane 15), then row_bcast:15 and row_bcast:31 carry the
// rows' sums into lane 63, which is read back.  No LDS traffic: a few cycles per step where a __shfl costs an LDS round trip.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v)
{
    // lanes the pattern gives no source add 0 (old = 0, bound_ctrl off): they do not lie on lane 63's path
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

__device__ __forceinline__ float wave_sum(float v)
{
    v = dpp_add<0xb1>(v);     // quad_perm:[1,0,3,2]
    v = dpp_add<0x4e>(v);     // quad_perm:[2,3,0,1]
    v = dpp_add<0x114>(v);    // row_shr:4
    v = dpp_add<0x118>(v);    // row_shr:8
    v = dpp_add<0x142>(v);    // row_bcast:15
    v = dpp_add<0x143>(v);    // row_bcast:31
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// The pick of nsg_prior_walk_ctl (include/nsg.h) by one wave: the lane holds its chunk of ceil(K / 64) consecutive codes in
// registers as q[r] = p_k inside the kept set and 0 outside it, then runs the plain walk's scan over q.  Both thresholds are
// the largest key whose monotone statistic (a count of logits >= t, a mass of p >= v) reaches its goal, built bit by bit
// from the top with one wave reduction per bit.  With temperature 1 and both filters off q is the plain walk's p, bit for bit.
// CK: the register chunk, >= ceil(K / 64) (8 serves K <= 512 at half the per-lane work of 16; the arithmetic is the same).
// Not inlined: the walk's products already take 124 of the 128 VGPRs a 1024-thread workgroup allows, and with the pick's
// register arrays inlined the allocator spilled some 800 VGPRs to scratch; as a call it gets registers of its own (98).
template <int CK>
__device__ __noinline__ int pick_ctl(const float *l, int K, int lane, float u, float inv_t, int top_k, float top_p)
{
    const int ck = (K + 63) / 64;
    const int k0 = lane * ck, k1 = min(K, k0 + ck);
    float mx = -INFINITY;
    for (int k = k0; k < k1; ++k) mx = fmaxf(mx, l[k]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    float q[CK];
    int nlive = 0;
#pragma unroll
    for (int r = 0; r < CK; ++r) {
        q[r] = 0.f;
        if (k0 + r < k1) q[r] = expf((l[k0 + r] - mx) * inv_t);
        nlive += q[r] > 0.f;
    }
    if (top_k >= 1 && top_k < wave_count(nlive)) {   // t = the top_k-th largest logit of the live codes; ties at t are kept
        uint32_t key[CK];
#pragma unroll
        for (int r = 0; r < CK; ++r) {
            key[r] = 0u;                     // no logit has key 0
            if (q[r] > 0.f) key[r] = order_key(l[k0 + r]);
        }
        uint32_t t = 0;
#pragma unroll 1
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = t | (1u << bit);
            int n = 0;
#pragma unroll
            for (int r = 0; r < CK; ++r) n += key[r] >= cand;
            if (wave_count(n) >= top_k) t = cand;
        }
#pragma unroll
        for (int r = 0; r < CK; ++r)
            if (key[r] < t) q[r] = 0.f;
    }
    if (top_p < 1.f) {                           // v = the largest kept p whose mass of p >= v reaches top_p * S_A
        float m = 0.f;
#pragma unroll
        for (int r = 0; r < CK; ++r) m += q[r];
        const float goal = top_p * wave_sum(m);
        uint32_t t = 0;                          // q >= 0: its bits order as the values do
#pragma unroll 1
        for (int bit = 30; bit >= 0; --bit) {
            const uint32_t cand = t | (1u << bit);
            m = 0.f;
#pragma unroll
            for (int r = 0; r < CK; ++r) m += __float_as_uint(q[r]) >= cand ? q[r] : 0.f;
            if (wave_sum(m) >= goal) t = cand;
        }
#pragma unroll
        for (int r = 0; r < CK; ++r)
            if (__float_as_uint(q[r]) < t) q[r] = 0.f;
    }
    // the plain walk's scan and pick (prior_walk_kernel, step 5) over q
    float tot = 0.f;
#pragma unroll
    for (int r = 0; r < CK; ++r) tot += q[r];
    float incl = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(incl, off, 64);
        if (lane >= off) incl = o + incl;
    }
    const float target = u * __shfl(incl, 63, 64);
    const float before = __shfl_up(incl, 1, 64);
    float run = lane == 0 ? 0.f : before;
    int first = K, lastpos = -1;
#pragma unroll
    for (int r = 0; r < CK; ++r) {
        run += q[r];
        if (q[r] > 0.f) {
            if (first == K && run > target) first = k0 + r;
            lastpos = k0 + r;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        first = min(first, __shfl_xor(first, off, 64));
        lastpos = max(lastpos, __shfl_xor(lastpos, off, 64));
    }
    return first < K ? first : lastpos;
}

// CTL: the instantiation of nsg_prior_walk_ctl (temperature, top-k, top-p, kept codes); the plain one is nsg_prior_walk's.
// CFG (with CTL): the instantiation of nsg_prior_walk_cfg.  The clips of a pair run the same chain on their own cond and vh
// rows; their logits are combined in LDS, one wave picks the pair's code, and both clips take its embedding.
template <bool CTL, bool CFG = false>
__global__ __launch_bounds__(THREADS) void prior_walk_kernel(std::conditional_t<CFG, WalkCfgArgs, std::conditional_t<CTL, WalkCtlArgs, WalkArgs>> a)
{
    static_assert(CTL || !CFG, "the guided walk picks with the controlled pick");
    static_assert(NC % 2 == 0, "a pair never straddles workgroups");
    extern __shared__ float lds[];
    const int dim = a.dim, D2 = 2 * dim, L = a.L, Kp = a.Kp;
    const int b0 = blockIdx.x * NC;
    const int nc = min(NC, a.B - b0);
    // LDS carve-up (floats); every piece a multiple of 4 floats
    float *ring = lds;                           // [3][NC][dim]  e of columns j-3 .. j-1 (column c sits in slot c % 3)
    float *hprev = ring + 3 * NC * dim;          // [L][NC][dim]  h_l of column j-1 (l >= 1)
    float *hbuf = hprev + L * NC * dim;          // [2][NC][dim]  h_l of column j (ping-pong)
    float *gout = hbuf + 2 * NC * dim;           // [NC][dim]     the gate's output
    float *y512 = gout + NC * dim;               // [NC][512]     the head's hidden layer
    float *lg = y512 + NC * HEAD;                // [NC][Kp]      logits
    float *red = lg + NC * Kp;                   // [NC * RED]    k-slice partials
    int *code_sh = reinterpret_cast<int *>(red + NC * RED);   // [NC]
    const int total = (3 + L + 2 + 1) * NC * dim + NC * HEAD + NC * Kp + NC * RED;
    for (int t = threadIdx.x; t < total; t += THREADS) lds[t] = 0.f;   // columns left of the grid are zero; idle clips stay finite
    __syncthreads();

    const size_t layer0 = (size_t)3 * dim * D2 + D2 + (size_t)dim * dim + dim;
    const size_t layerN = (size_t)2 * dim * D2 + D2 + (size_t)dim * dim + dim;
    const float *head = a.w + layer0 + (size_t)(L - 1) * layerN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = a.row;

    for (int j = 0; j < a.W; ++j) {
        int cur = 0;                             // hbuf[cur] holds h_l[j] for the layer being processed (l >= 1)
        for (int l = 0; l < L; ++l) {
            const float *wl = a.w + (l == 0 ? 0 : layer0 + (size_t)(l - 1) * layerN);
            const int Kh = (l == 0 ? 3 : 2) * dim;
            const float *hz_w = wl, *hz_b = wl + (size_t)Kh * D2;
            const float *rs_w = hz_b + D2, *rs_b = rs_w + (size_t)dim * dim;
            float *hc = hbuf + cur * NC * dim, *hn = hbuf + (cur ^ 1) * NC * dim;
            float *hp = hprev + l * NC * dim;
            // 1. horizontal stack: layer 0 reads e of columns j-3, j-2, j-1 (tap 3, column j, is masked); the others h_l[j-1], h_l[j]
            const float *seg[3];
            if (l == 0) {
                seg[0] = ring + (j % 3) * NC * dim;
                seg[1] = ring + ((j + 1) % 3) * NC * dim;
                seg[2] = ring + ((j + 2) % 3) * NC * dim;
            } else {
                seg[0] = hp; seg[1] = hc; seg[2] = hc;
            }
            int S = matvec_partial(hz_w, D2, D2, Kh, seg, dim, dim, red);
            __syncthreads();
            // 2. out = gate((v2h + h_horiz) + cond)
            for (int t = threadIdx.x; t < NC * dim; t += THREADS) {
                const int c = t / dim, d = t - c * dim;
                if (c >= nc) continue;
                const int b = b0 + c;
                const float ha = reduce_out(red, S, D2, c, d, hz_b[d]);
                const float hb = reduce_out(red, S, D2, c, d + dim, hz_b[d + dim]);
                const float *vh = a.vh + (((size_t)l * a.B + b) * a.W + j) * D2;
                const float *cd = a.cond + ((size_t)l * a.B + b) * D2;
                const float pa = (vh[d] + ha) + cd[d];
                const float pb = (vh[d + dim] + hb) + cd[d + dim];
                gout[c * dim + d] = tanhf(pa) * (1.f / (1.f + expf(-pb)));
            }
            __syncthreads();
            // 3. h_{l+1} = resid(out) (+ h_l)
            const float *gseg[3] = {gout, gout, gout};
            S = matvec_partial(rs_w, dim, dim, dim, gseg, dim, dim, red);
            __syncthreads();
            for (int t = threadIdx.x; t < NC * dim; t += THREADS) {
                const int c = t / dim, d = t - c * dim;
                float v = reduce_out(red, S, dim, c, d, rs_b[d]);
                if (l > 0) {
                    const float h = hc[t];
                    v = v + h;
                    hp[t] = h;                   // h_l[j] is column j-1 of layer l at the next position
                }
                hn[t] = v;
            }
            __syncthreads();
            cur ^= 1;
        }
        // 4. the head: 1x1 dim -> 512, ReLU, 1x1 512 -> K
        const float *hL = hbuf + cur * NC * dim;
        const float *w0 = head, *bb0 = w0 + (size_t)dim * HEAD, *w2 = bb0 + HEAD, *bb2 = w2 + (size_t)HEAD * Kp;
        const float *hseg[3] = {hL, hL, hL};
        int S = matvec_partial(w0, HEAD, HEAD, dim, hseg, dim, dim, red);
        __syncthreads();
        for (int t = threadIdx.x; t < NC * HEAD; t += THREADS) {
            const int c = t / HEAD, n = t - c * HEAD;
            y512[t] = fmaxf(reduce_out(red, S, HEAD, c, n, bb0[n]), 0.f);
        }
        __syncthreads();
        const float *yseg[3] = {y512, y512, y512};
        S = matvec_partial(w2, Kp, Kp, HEAD, yseg, HEAD, HEAD, red);
        __syncthreads();
        for (int t = threadIdx.x; t < NC * Kp; t += THREADS) {
            const int c = t / Kp, n = t - c * Kp;
            const float v = reduce_out(red, S, Kp, c, n, bb2[n]);
            lg[t] = v;
            if (a.logits && c < nc && n < a.K) a.logits[(((size_t)(b0 + c) * a.H + i) * a.W + j) * a.K + n] = v;
        }
        __syncthreads();
        if constexpr (CFG) {
            // 4b. l = l_c + guidance * (l_c - l_u), three separately rounded operations, over the conditional branch's row
            for (int t = threadIdx.x; t < (NC / 2) * Kp; t += THREADS) {
                const int p = t / Kp, n = t - p * Kp;
                const float lc = lg[2 * p * Kp + n], lu = lg[(2 * p + 1) * Kp + n];
                lg[2 * p * Kp + n] = __fadd_rn(lc, __fmul_rn(a.guidance, __fsub_rn(lc, lu)));
            }
            __syncthreads();
        }
        // 5. the code: teacher-forced, or the inverse CDF of the softmax against u (one wave per clip; per pair under CFG)
        if (wave < (CFG ? nc / 2 : nc)) {
            const int c = CFG ? 2 * wave : wave, b = b0 + c;
            const size_t pos = ((size_t)(CFG ? b / 2 : b) * a.H + i) * a.W + j;
            int code;
            if constexpr (CTL) {
                if (a.keep && a.keep[pos]) code = (int)a.x_in[pos];
                else if (a.K <= 64 * 8) code = pick_ctl<8>(lg + c * Kp, a.K, lane, a.u[pos], a.inv_t, a.top_k, a.top_p);
                else code = pick_ctl<CKMAX>(lg + c * Kp, a.K, lane, a.u[pos], a.inv_t, a.top_k, a.top_p);
            } else if (a.x_in) {
                code = (int)a.x_in[pos];
            } else {
                const float *l = lg + c * Kp;
                const int K = a.K, ck = (K + 63) / 64;
                const int k0 = lane * ck, k1 = min(K, k0 + ck);
                float mx = -INFINITY;
                for (int k = k0; k < k1; ++k) mx = fmaxf(mx, l[k]);
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
                float tot = 0.f;
                for (int k = k0; k < k1; ++k) tot += expf(l[k] - mx);
                float incl = tot;                // inclusive scan of the lanes' totals, lane order
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const float o = __shfl_up(incl, off, 64);
                    if (lane >= off) incl = o + incl;
                }
                const float S_ = __shfl(incl, 63, 64);
                const float target = a.u[pos] * S_;
                // A lane's running sum starts at the scan of the lanes before it, but its end can differ from that scan's next
                // value by a few ulps.  A target in such a gap is passed at once by the next lane: only a code with p > 0 may
                // take it, so a code the distribution excludes is never returned.
                const float before = __shfl_up(incl, 1, 64);
                float run = lane == 0 ? 0.f : before;
                int first = K, lastpos = -1;
                for (int k = k0; k < k1; ++k) {
                    const float p = expf(l[k] - mx);
                    run += p;
                    if (p > 0.f) {
                        if (first == K && run > target) first = k;
                        lastpos = k;
                    }
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    first = min(first, __shfl_xor(first, off, 64));
                    lastpos = max(lastpos, __shfl_xor(lastpos, off, 64));
                }
                code = first < K ? first : lastpos;
            }
            code = min(max(code, 0), a.K - 1);
            if (lane == 0) {
                code_sh[c] = code;
                if constexpr (CFG) code_sh[c + 1] = code;      // both branches continue from the pair's code
                if (a.codes) a.codes[pos] = code;
            }
        }
        __syncthreads();
        // 6. e of column j into the ring (slot j % 3) and the row buffer
        for (int t = threadIdx.x; t < NC * dim; t += THREADS) {
            const int c = t / dim, d = t - c * dim;
            if (c >= nc) continue;
            const float v = a.emb[(size_t)code_sh[c] * dim + d];
            ring[((j % 3) * NC + c) * dim + d] = v;
            a.e_row[(size_t)(b0 + c) * a.e_clip_stride + (size_t)j * dim + d] = v;
        }
        __syncthreads();
    }
}

size_t walk_lds_bytes(int dim, int L, int Kp)
{
    return ((size_t)(3 + L + 2 + 1) * NC * dim + (size_t)NC * HEAD + (size_t)NC * Kp + (size_t)NC * RED) * sizeof(float) + NC * sizeof(int);
}

constexpr size_t LDS_MAX = 160 * 1024;

bool walk_supported(int dim, int L, int K)
{
    if (dim <= 0 || dim % 16 != 0 || dim > 128 || L < 1 || K < 1 || K > 1024) return false;
    return walk_lds_bytes(dim, L, (K + 3) / 4 * 4) <= LDS_MAX;
}

}  // namespace

extern "C" {

size_t nsg_prior_walk_weight_floats(int32_t dim, int32_t n_layers, int32_t input_dim)
{
    if (!walk_supported(dim, n_layers, input_dim)) return 0;
    const size_t D2 = 2 * (size_t)dim, Kp = ((size_t)input_dim + 3) / 4 * 4;
    const size_t layer0 = 3 * dim * D2 + D2 + (size_t)dim * dim + dim;
    const size_t layerN = 2 * dim * D2 + D2 + (size_t)dim * dim + dim;
    return layer0 + (size_t)(n_layers - 1) * layerN + (size_t)dim * HEAD + HEAD + HEAD * Kp + Kp;
}

// The checks every walk shares (fn: the entry point's name for the error string)
static int walk_checks(const char *fn, const float *w, const float *emb, const float *cond, const float *vh, const float *e_row,
                       int64_t e_clip_stride, int32_t B, int32_t H, int32_t W, int32_t dim, int32_t n_layers, int32_t input_dim, int32_t row)
{
    NSG_REQUIRE(w && emb && cond && vh && e_row, NSG_E_INVALID, "%s: null pointer", fn);
    NSG_REQUIRE(B > 0 && H > 0 && W > 0 && row >= 0 && row < H, NSG_E_INVALID, "%s: bad extents (B, H, W > 0, 0 <= row < H)", fn);
    NSG_REQUIRE(walk_supported(dim, n_layers, input_dim), NSG_E_UNSUPPORTED,
                "%s: dim=%d n_layers=%d input_dim=%d outside the envelope (dim %% 16 == 0, dim <= 128, n_layers >= 1, "
                "input_dim <= 1024, LDS <= 160 KiB)", fn, dim, n_layers, input_dim);
    NSG_REQUIRE(e_clip_stride >= (int64_t)W * dim && e_clip_stride % 4 == 0, NSG_E_INVALID, "%s: bad e_clip_stride", fn);
    NSG_REQUIRE(nsg_aligned16(w) && nsg_aligned16(emb) && nsg_aligned16(cond) && nsg_aligned16(vh) && nsg_aligned16(e_row), NSG_E_INVALID,
                "%s: pointers must be 16-byte aligned", fn);
    return NSG_OK;
}

static void walk_fill(WalkArgs &a, const float *w, const float *emb, const float *cond, const float *vh, const float *u, const int64_t *x_in,
                      int64_t *codes, float *e_row, int64_t e_clip_stride, float *logits, int32_t B, int32_t H, int32_t W, int32_t dim,
                      int32_t n_layers, int32_t input_dim, int32_t row)
{
    a.w = w; a.emb = emb; a.cond = cond; a.vh = vh; a.u = u; a.x_in = x_in; a.codes = codes;
    a.e_row = e_row; a.e_clip_stride = e_clip_stride; a.logits = logits;
    a.B = B; a.H = H; a.W = W; a.dim = dim; a.L = n_layers; a.K = input_dim; a.Kp = (input_dim + 3) / 4 * 4; a.row = row;
}

int nsg_prior_walk(const float *w, const float *emb, const float *cond, const float *vh, const float *u, const int64_t *x_in,
                   int64_t *codes, float *e_row, int64_t e_clip_stride, float *logits, int32_t B, int32_t H, int32_t W, int32_t dim,
                   int32_t n_layers, int32_t input_dim, int32_t row, void *stream)
{
    NSG_REQUIRE((u != nullptr) != (x_in != nullptr), NSG_E_INVALID, "nsg_prior_walk: exactly one of u (sampling) and x_in (teacher-forced)");
    NSG_REQUIRE(x_in || codes, NSG_E_INVALID, "nsg_prior_walk: sampling needs a codes output");
    if (const int rc = walk_checks("nsg_prior_walk", w, emb, cond, vh, e_row, e_clip_stride, B, H, W, dim, n_layers, input_dim, row)) return rc;
    static LdsOptIn once;
    if (const int rc = nsg_lds_opt_in(once, {reinterpret_cast<const void *>(&prior_walk_kernel<false>)}, LDS_MAX, "nsg_prior_walk")) return rc;
    WalkArgs a;
    walk_fill(a, w, emb, cond, vh, u, x_in, codes, e_row, e_clip_stride, logits, B, H, W, dim, n_layers, input_dim, row);
    hipLaunchKernelGGL(prior_walk_kernel<false>, dim3((unsigned)nsg_cdiv(B, NC)), dim3(THREADS), walk_lds_bytes(dim, n_layers, a.Kp),
                       (hipStream_t)stream, a);
    return nsg_check_launch("prior_walk_kernel");
}

int nsg_prior_walk_ctl(const float *w, const float *emb, const float *cond, const float *vh, const float *u, const int64_t *x_in,
                       const uint8_t *keep, int64_t *codes, float *e_row, int64_t e_clip_stride, float *logits, int32_t B, int32_t H,
                       int32_t W, int32_t dim, int32_t n_layers, int32_t input_dim, int32_t row, float temperature, int32_t top_k,
                       float top_p, void *stream)
{
    NSG_REQUIRE(u && codes, NSG_E_INVALID, "nsg_prior_walk_ctl: u and codes are required");
    NSG_REQUIRE((x_in != nullptr) == (keep != nullptr), NSG_E_INVALID, "nsg_prior_walk_ctl: x_in and keep come together");
    NSG_REQUIRE(isfinite(temperature) && temperature > 0.f && isfinite(1.0f / temperature), NSG_E_INVALID,
                "nsg_prior_walk_ctl: temperature must be finite and > 0, and so must 1 / temperature in fp32");
    NSG_REQUIRE(top_k >= 0, NSG_E_INVALID, "nsg_prior_walk_ctl: top_k=%d must be >= 0 (0 = off)", top_k);
    NSG_REQUIRE(top_p > 0.f && top_p <= 1.f, NSG_E_INVALID, "nsg_prior_walk_ctl: top_p must be in (0, 1] (1 = off)");
    if (const int rc = walk_checks("nsg_prior_walk_ctl", w, emb, cond, vh, e_row, e_clip_stride, B, H, W, dim, n_layers, input_dim, row)) return rc;
    static LdsOptIn once;
    if (const int rc = nsg_lds_opt_in(once, {reinterpret_cast<const void *>(&prior_walk_kernel<true>)}, LDS_MAX, "nsg_prior_walk_ctl")) return rc;
    WalkCtlArgs a;
    walk_fill(a, w, emb, cond, vh, u, x_in, codes, e_row, e_clip_stride, logits, B, H, W, dim, n_layers, input_dim, row);
    a.keep = keep; a.inv_t = 1.0f / temperature; a.top_k = top_k; a.top_p = top_p;
    hipLaunchKernelGGL(prior_walk_kernel<true>, dim3((unsigned)nsg_cdiv(B, NC)), dim3(THREADS), walk_lds_bytes(dim, n_layers, a.Kp),
                       (hipStream_t)stream, a);
    return nsg_check_launch("prior_walk_ctl_kernel");
}

int nsg_prior_walk_cfg(const float *w, const float *emb, const float *cond, const float *vh, const float *u, const int64_t *x_in,
                       const uint8_t *keep, int64_t *codes, float *e_row, int64_t e_clip_stride, float *logits, int32_t B, int32_t H,
                       int32_t W, int32_t dim, int32_t n_layers, int32_t input_dim, int32_t row, float temperature, int32_t top_k,
                       float top_p, float guidance, void *stream)
{
    NSG_REQUIRE(u && codes, NSG_E_INVALID, "nsg_prior_walk_cfg: u and codes are required");
    NSG_REQUIRE((x_in != nullptr) == (keep != nullptr), NSG_E_INVALID, "nsg_prior_walk_cfg: x_in and keep come together");
    NSG_REQUIRE(isfinite(temperature) && temperature > 0.f && isfinite(1.0f / temperature), NSG_E_INVALID,
                "nsg_prior_walk_cfg: temperature must be finite and > 0, and so must 1 / temperature in fp32");
    NSG_REQUIRE(top_k >= 0, NSG_E_INVALID, "nsg_prior_walk_cfg: top_k=%d must be >= 0 (0 = off)", top_k);
    NSG_REQUIRE(top_p > 0.f && top_p <= 1.f, NSG_E_INVALID, "nsg_prior_walk_cfg: top_p must be in (0, 1] (1 = off)");
    NSG_REQUIRE(B % 2 == 0, NSG_E_INVALID, "nsg_prior_walk_cfg: B=%d must be even (clips 2p and 2p + 1 are pair p)", B);
    NSG_REQUIRE(isfinite(guidance) && guidance >= 0.f && guidance <= 1024.f, NSG_E_INVALID,
                "nsg_prior_walk_cfg: guidance must be finite and in [0, 1024]");
    if (const int rc = walk_checks("nsg_prior_walk_cfg", w, emb, cond, vh, e_row, e_clip_stride, B, H, W, dim, n_layers, input_dim, row)) return rc;
    static LdsOptIn once;
    if (const int rc = nsg_lds_opt_in(once, {reinterpret_cast<const void *>(&prior_walk_kernel<true, true>)}, LDS_MAX, "nsg_prior_walk_cfg")) return rc;
    WalkCfgArgs a;
    walk_fill(a, w, emb, cond, vh, u, x_in, codes, e_row, e_clip_stride, logits, B, H, W, dim, n_layers, input_dim, row);
    a.keep = keep; a.inv_t = 1.0f / temperature; a.top_k = top_k; a.top_p = top_p; a.guidance = guidance;
    hipLaunchKernelGGL((prior_walk_kernel<true, true>), dim3((unsigned)nsg_cdiv(B, NC)), dim3(THREADS), walk_lds_bytes(dim, n_layers, a.Kp),
                       (hipStream_t)stream, a);
    return nsg_check_launch("prior_walk_cfg_kernel");
}

}  // extern "C"
