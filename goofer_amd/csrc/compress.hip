// The dynamic range compressor on the device (gfx950): every signal of a ragged batch through a feed-forward log-domain
// compressor with a smooth decoupled peak detector.  The definition (gain computer, release and attack recurrences, gain,
// tolerance) is in include/goofer_hip.h; the host half, goofer_host_compress_plan (planner.hip), makes the coefficients, the
// tile table and the powers of the two one-pole coefficients.
//
// The release stage, y1 = max(xl, aR y1' + (1 - aR) xl), is not linear, so the matrix-power scan of loudness.hip cannot carry
// it.  A sample is the map y -> max(C, A y + B); maps of that form compose to one of that form and the composition is
// associative.  All elements of a scan level share A (a power of aR from the host), so an element is the pair (C, B): C the
// state behind the element's samples from the state in front of them as the scan knows it, B the linear path alone (B <= C).
// A run that starts from a known state y0 starts from (y0, y0); one that does not from (0, 0), the neutral element for the
// states that occur (all >= 0).  The attack stage, yl = aA yl' + (1 - aA) y1, is an ordinary linear scan over y1, so it starts
// once the release states are known.  A signal is cut into tiles of 4096 samples and a tile into 256 runs of 16; five launches
// in stream order, no workgroup waits for another one, and every combination has a fixed order:
//   1  k_cp_release_sum    a workgroup per tile: xl, runs from (0, 0), a workgroup scan, the tile's (C, B) to scratch
//   2  k_cp_release_carry  a workgroup per signal: the tiles' (C, B) into the release state in front of every tile
//   3  k_cp_attack_sum     a workgroup per tile: y1 from the true state, the attack runs from 0, a scan, the tile's end state
//   4  k_cp_attack_carry   a workgroup per signal: those into the attack state in front of every tile
//   5  k_cp_apply          a workgroup per tile: y1, yl, g from the true states; y, the curve, the tile's greatest yl
#include "launchers.h"

#define CP_THREADS 256
#define CP_SPT GOOFER_COMPRESS_SPT
#define CP_T GOOFER_COMPRESS_TILE
#define CP_LEVELS 8                                   // 2^8 runs in a tile
#define CP_RUN GOOFER_COMPRESS_RUN_TILES
#define CP_POWS GOOFER_COMPRESS_POWS
static_assert(CP_T == CP_THREADS * CP_SPT && CP_SPT == 16 && (1 << CP_LEVELS) == CP_THREADS, "one workgroup of 256 runs of 16 per tile");
static_assert(CP_POWS == CP_LEVELS + 4 + CP_LEVELS && CP_RUN == 16, "a^16 .. a^2048 inside a tile, a^4096 a tile, a^(4096 * 16 * 2^k) over the runs of 16 tiles");
static_assert(GOOFER_COMPRESS_ROUND_TILES == CP_THREADS * CP_RUN, "a round of the carry kernels");
#define CP_XPAD (CP_T + CP_T / 16)                    // the tile, one pad word per 16

// entry q of the staged samples: a thread's 16 consecutive words at a lane stride of 17
__device__ __forceinline__ int cp_idx(int q) { return q + (q >> 4); }

// what the definition's formulas need of coef, per thread
struct cp_par {
    double T, W, ns, M, aR, aA, bR, bA, hw, w2, thr;
    __device__ __forceinline__ cp_par(const double *__restrict__ c, int skip)
    {
        T = c[0], W = c[1], ns = -c[2], M = c[3], aR = c[4], aA = c[5];
        bR = 1.0 - aR, bA = 1.0 - aA, hw = W / 2.0, w2 = 2.0 * W;
        thr = skip ? exp10((T - hw) / 20.0) : -1.0;            // the knee's lower end as |x| (a >= 1e-6 > -1: nothing is skipped)
    }
    // xl of the definition for the sample x.  A sample at or under the knee's lower end asks for no reduction: one compare
    // and no logarithm (option "compress_skip"; the curve is continuous there, so this moves the result by less than rounding).
    // Per sample: the same test once per run of 16 was slower on every input tried (docs/EXPERIMENTS.md).
    __device__ __forceinline__ double xl(float x) const
    {
        const double a = fmax(fabs((double)x), GOOFER_COMPRESS_FLOOR);
        if (a <= thr) return 0.0;
        const double d = 20.0 * log10(a) - T, d2 = 2.0 * d;
        if (d2 < -W) return 0.0;
        if (W > 0.0 && fabs(d2) <= W) return ns * ((d + hw) * (d + hw)) / w2;
        return ns * d;
    }
};

// the tile's samples [t0, t0 + T) into LDS (coalesced); 0 outside the signal
__device__ __forceinline__ void cp_stage(const float *__restrict__ xs, int64_t len, int64_t t0, float *__restrict__ s_x)
{
    for (int q = threadIdx.x; q < CP_T; q += CP_THREADS) {
        const int64_t p = t0 + q;
        s_x[cp_idx(q)] = p < len ? xs[p] : 0.0f;
    }
}

// MODE 0: xl of the thread's 16 samples from the staged tile; 1: likewise, and written to xlbuf (the tile's, [T]); 2: read from it
template <int MODE>
__device__ __forceinline__ void cp_levels(const cp_par &P, const float *__restrict__ s_x, double *__restrict__ xlbuf, int64_t left,
                                          double (&xl)[CP_SPT])
{
    const int q0 = threadIdx.x * CP_SPT;
#pragma unroll
    for (int e = 0; e < CP_SPT; ++e) {
        if (MODE == 2) {
            xl[e] = q0 + e < left ? xlbuf[q0 + e] : 0.0;
        } else {
            xl[e] = q0 + e < left ? P.xl(s_x[cp_idx(q0 + e)]) : 0.0;     // (past the end: xl = 0 whatever T is)
            if (MODE == 1 && q0 + e < left) xlbuf[q0 + e] = xl[e];
        }
    }
}

// the release maps of the thread's 16 samples composed onto (C, B)
__device__ __forceinline__ void cp_release_run(const cp_par &P, const double (&xl)[CP_SPT], double &C, double &B)
{
#pragma unroll
    for (int e = 0; e < CP_SPT; ++e) {
        const double b = P.bR * xl[e];
        C = fmax(xl[e], P.aR * C + b);
        B = P.aR * B + b;
    }
}

// Inclusive scan of the workgroup's release elements: (C, B)_j <- (C, B)_(j - 2^k) then (C, B)_j, for k = 0 .. 7, pw[k] the A of
// an element of level k.  Returns the buffer (of s_sc[2]) that holds the result: C in s_sc[b][0 .. 256), B behind it.
__device__ __forceinline__ int cp_scan_release(double &C, double &B, const double *__restrict__ pw, double (*s_sc)[2 * CP_THREADS])
{
    const int tid = threadIdx.x;
    int cur = 0;
    s_sc[0][tid] = C, s_sc[0][CP_THREADS + tid] = B;
    __syncthreads();
    for (int k = 0; k < CP_LEVELS; ++k) {
        const int off = 1 << k;
        if (tid >= off) {
            const double Co = s_sc[cur][tid - off], Bo = s_sc[cur][CP_THREADS + tid - off], A = pw[k];
            C = fmax(C, A * Co + B);
            B = A * Bo + B;
        }
        cur ^= 1;
        s_sc[cur][tid] = C, s_sc[cur][CP_THREADS + tid] = B;
        __syncthreads();                                        // (the next level reads this buffer and writes the other one)
    }
    return cur;
}

// Inclusive linear scan: v_j <- pw[k] v_(j - 2^k) + v_j.  The result is in s_sc[returned][0 .. 256).
__device__ __forceinline__ int cp_scan_attack(double &v, const double *__restrict__ pw, double (*s_sc)[2 * CP_THREADS])
{
    const int tid = threadIdx.x;
    int cur = 0;
    s_sc[0][tid] = v;
    __syncthreads();
    for (int k = 0; k < CP_LEVELS; ++k) {
        const int off = 1 << k;
        if (tid >= off) v = pw[k] * s_sc[cur][tid - off] + v;
        cur ^= 1;
        s_sc[cur][tid] = v;
        __syncthreads();
    }
    return cur;
}

// a tile's signal and place from the planner's table; false for a pair that is not the planner's (nothing is read or written)
__device__ __forceinline__ bool cp_tile(const int32_t *__restrict__ tiles, const int64_t *__restrict__ in_off, int n, int &sig, int &kt,
                                        int64_t &base, int64_t &len, int64_t &t0)
{
    sig = __builtin_amdgcn_readfirstlane(tiles[2 * blockIdx.x]), kt = __builtin_amdgcn_readfirstlane(tiles[2 * blockIdx.x + 1]);
    if (sig < 0 || sig >= n || kt < 0) return false;
    base = in_off[sig], len = in_off[sig + 1] - base, t0 = (int64_t)kt * CP_T;
    return base >= 0 && t0 < len && len < ((int64_t)1 << 31);
}

template <int MODE>
__global__ __launch_bounds__(CP_THREADS)
void k_cp_release_sum(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, const double *__restrict__ coef,
                      const double *__restrict__ pows, const int32_t *__restrict__ tiles, int skip, double *__restrict__ rsum,
                      int32_t *__restrict__ first_tile, double *__restrict__ xlbuf)
{
    __shared__ float s_x[CP_XPAD];
    __shared__ double s_sc[2][2 * CP_THREADS];
    int sig, kt;
    int64_t base, len, t0;
    if (!cp_tile(tiles, in_off, n, sig, kt, base, len, t0)) return;
    if (threadIdx.x == 0 && kt == 0) first_tile[sig] = (int32_t)blockIdx.x;
    const cp_par P(coef, skip);
    cp_stage(x + base, len, t0, s_x);
    __syncthreads();
    double xl[CP_SPT], C = 0.0, B = 0.0;
    cp_levels<MODE>(P, s_x, MODE ? xlbuf + base + t0 : nullptr, len - t0, xl);
    cp_release_run(P, xl, C, B);
    cp_scan_release(C, B, pows, s_sc);
    if (threadIdx.x == CP_THREADS - 1) rsum[2 * (int64_t)blockIdx.x] = C, rsum[2 * (int64_t)blockIdx.x + 1] = B;
}

// a signal's tiles in the tile table: false where the table is not the planner's
__device__ __forceinline__ bool cp_signal(const int64_t *__restrict__ in_off, int64_t n_tiles, const int32_t *__restrict__ first_tile, int &nt,
                                          int64_t &first)
{
    const int sig = blockIdx.x;
    const int64_t len = in_off[sig + 1] - in_off[sig];
    if (len <= 0 || len >= ((int64_t)1 << 31)) return false;
    nt = (int)((len + CP_T - 1) / CP_T);
    first = first_tile[sig];
    return first >= 0 && first + nt <= n_tiles;
}

// rstart[tile] = the release state in front of the tile: 0 for a signal's first, max(C_t, aR^4096 rstart[t] + B_t) for tile
// t + 1.  One workgroup per signal, GOOFER_COMPRESS_ROUND_TILES tiles a round: a thread composes 16 consecutive tiles, thread 0
// from the state in front of the round, the workgroup scans the threads' elements, and every thread walks its tiles again from
// its true state.
__global__ __launch_bounds__(CP_THREADS)
void k_cp_release_carry(const int64_t *__restrict__ in_off, int64_t n_tiles, const double *__restrict__ pows, const double *__restrict__ rsum,
                        const int32_t *__restrict__ first_tile, double *__restrict__ rstart)
{
    __shared__ double s_sc[2][2 * CP_THREADS];
    const int tid = threadIdx.x;
    int nt;
    int64_t first;
    if (!cp_signal(in_off, n_tiles, first_tile, nt, first)) return;
    const double A = pows[CP_LEVELS];                           // aR^4096: one tile
    const double *__restrict__ PR = pows + CP_LEVELS + 4;       // aR^(4096 * 16): a thread's run; level k of the scan: PR[k]
    double carry = 0.0;
    for (int c = 0; c < nt; c += CP_THREADS * CP_RUN) {
        const int t0 = c + tid * CP_RUN;
        double zc[CP_RUN], zb[CP_RUN];
#pragma unroll
        for (int e = 0; e < CP_RUN; ++e) {
            const bool in = t0 + e < nt;                        // (past the signal's last tile: the neutral element)
            zc[e] = in ? rsum[2 * (first + t0 + e)] : 0.0, zb[e] = in ? rsum[2 * (first + t0 + e) + 1] : 0.0;
        }
        double C = tid == 0 ? carry : 0.0, B = C;
#pragma unroll
        for (int e = 0; e < CP_RUN; ++e) {
            C = fmax(zc[e], A * C + zb[e]);
            B = A * B + zb[e];
        }
        const int cur = cp_scan_release(C, B, PR, s_sc);
        double st = tid == 0 ? carry : s_sc[cur][tid - 1];
        carry = s_sc[cur][CP_THREADS - 1];
#pragma unroll
        for (int e = 0; e < CP_RUN; ++e) {
            if (t0 + e < nt) rstart[first + t0 + e] = st;
            st = fmax(zc[e], A * st + zb[e]);
        }
        __syncthreads();                                        // (the next round's scan writes the buffers read above)
    }
}

// the tile's xl and, from the release state in front of the tile, the release state in front of the thread's run
template <int MODE>
__device__ __forceinline__ double cp_release_states(const cp_par &P, const float *__restrict__ s_x, double *__restrict__ xlbuf, int64_t left,
                                                    const double *__restrict__ pows, double st, double (*s_sc)[2 * CP_THREADS],
                                                    double (&xl)[CP_SPT])
{
    cp_levels<MODE>(P, s_x, xlbuf, left, xl);
    double C = threadIdx.x == 0 ? st : 0.0, B = C;
    cp_release_run(P, xl, C, B);
    const int cur = cp_scan_release(C, B, pows, s_sc);
    const double y1 = threadIdx.x == 0 ? st : s_sc[cur][threadIdx.x - 1];
    __syncthreads();                                            // (the attack scan writes the buffers read above)
    return y1;
}

// xl[e] <- y1 of the thread's samples from the state y1 in front of them; the attack recurrence over them from yl (left in yl)
__device__ __forceinline__ void cp_detector_run(const cp_par &P, double (&xl)[CP_SPT], double y1, double &yl)
{
#pragma unroll
    for (int e = 0; e < CP_SPT; ++e) {
        y1 = fmax(xl[e], P.aR * y1 + P.bR * xl[e]);
        yl = P.aA * yl + P.bA * y1;
        xl[e] = y1;
    }
}

template <int MODE>
__global__ __launch_bounds__(CP_THREADS)
void k_cp_attack_sum(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, const double *__restrict__ coef,
                     const double *__restrict__ pows, const int32_t *__restrict__ tiles, int skip, const double *__restrict__ rstart,
                     double *__restrict__ asum, double *__restrict__ xlbuf)
{
    __shared__ float s_x[CP_XPAD];
    __shared__ double s_sc[2][2 * CP_THREADS];
    int sig, kt;
    int64_t base, len, t0;
    if (!cp_tile(tiles, in_off, n, sig, kt, base, len, t0)) return;
    const cp_par P(coef, skip);
    if (MODE != 2) {
        cp_stage(x + base, len, t0, s_x);
        __syncthreads();
    }
    double xl[CP_SPT];
    const double y1 = cp_release_states<MODE == 2 ? 2 : 0>(P, s_x, MODE == 2 ? xlbuf + base + t0 : nullptr, len - t0, pows,
                                                           rstart[blockIdx.x], s_sc, xl);
    double v = 0.0;
    cp_detector_run(P, xl, y1, v);
    cp_scan_attack(v, pows + CP_POWS, s_sc);
    if (threadIdx.x == CP_THREADS - 1) asum[blockIdx.x] = v;
}

// astart[tile] = the attack state in front of the tile: 0 for a signal's first, aA^4096 astart[t] + asum[t] for tile t + 1; the
// shape of k_cp_release_carry with a linear element.
__global__ __launch_bounds__(CP_THREADS)
void k_cp_attack_carry(const int64_t *__restrict__ in_off, int64_t n_tiles, const double *__restrict__ pows, const double *__restrict__ asum,
                       const int32_t *__restrict__ first_tile, double *__restrict__ astart)
{
    __shared__ double s_sc[2][2 * CP_THREADS];
    const int tid = threadIdx.x;
    int nt;
    int64_t first;
    if (!cp_signal(in_off, n_tiles, first_tile, nt, first)) return;
    const double A = pows[CP_POWS + CP_LEVELS];
    const double *__restrict__ PR = pows + CP_POWS + CP_LEVELS + 4;
    double carry = 0.0;
    for (int c = 0; c < nt; c += CP_THREADS * CP_RUN) {
        const int t0 = c + tid * CP_RUN;
        double z[CP_RUN];
#pragma unroll
        for (int e = 0; e < CP_RUN; ++e) z[e] = t0 + e < nt ? asum[first + t0 + e] : 0.0;
        double v = tid == 0 ? carry : 0.0;
#pragma unroll
        for (int e = 0; e < CP_RUN; ++e) v = A * v + z[e];
        const int cur = cp_scan_attack(v, PR, s_sc);
        double st = tid == 0 ? carry : s_sc[cur][tid - 1];
        carry = s_sc[cur][CP_THREADS - 1];
#pragma unroll
        for (int e = 0; e < CP_RUN; ++e) {
            if (t0 + e < nt) astart[first + t0 + e] = st;
            st = A * st + z[e];
        }
        __syncthreads();
    }
}

template <int MODE>
__global__ __launch_bounds__(CP_THREADS)
void k_cp_apply(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, const double *__restrict__ coef,
                const double *__restrict__ pows, const int32_t *__restrict__ tiles, int skip, const double *__restrict__ rstart,
                const double *__restrict__ astart, float *__restrict__ out, unsigned long long *__restrict__ max_bits,
                double *__restrict__ curve, double *__restrict__ xlbuf)
{
    __shared__ float s_x[CP_XPAD];
    __shared__ double s_sc[2][2 * CP_THREADS];
    __shared__ double s_red[CP_THREADS / 64];
    int sig, kt;
    int64_t base, len, t0;
    if (!cp_tile(tiles, in_off, n, sig, kt, base, len, t0)) return;
    const int tid = threadIdx.x;
    const cp_par P(coef, skip);
    cp_stage(x + base, len, t0, s_x);                           // (x is needed for y whatever MODE is)
    __syncthreads();
    const int64_t left = len - t0;
    double y1s[CP_SPT];
    const double y1 = cp_release_states<MODE == 2 ? 2 : 0>(P, s_x, MODE == 2 ? xlbuf + base + t0 : nullptr, left, pows, rstart[blockIdx.x],
                                                           s_sc, y1s);
    const double a0 = astart[blockIdx.x];
    double v = tid == 0 ? a0 : 0.0;
    cp_detector_run(P, y1s, y1, v);
    const int cur = cp_scan_attack(v, pows + CP_POWS, s_sc);
    double yl = tid == 0 ? a0 : s_sc[cur][tid - 1], top = 0.0;
    const int q0 = tid * CP_SPT;
    double *__restrict__ cv = curve ? curve + base + t0 : nullptr;
#pragma unroll
    for (int e = 0; e < CP_SPT; ++e) {
        yl = P.aA * yl + P.bA * y1s[e];
        if (q0 + e < left) {
            const double ex = (P.M - yl) / 20.0;
            const double g = ex == 0.0 ? 1.0 : exp10(ex);       // (the identity property: 10^0 is exactly 1 whatever exp10 makes of it)
            s_x[cp_idx(q0 + e)] = (float)((double)s_x[cp_idx(q0 + e)] * g);
            top = yl > top ? yl : top;                          // (yl >= 0; a NaN is not taken)
            if (cv) cv[q0 + e] = yl;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = fmax(top, __shfl_xor(top, o, 64));
    if ((tid & 63) == 0) s_red[tid >> 6] = top;
    __syncthreads();                                            // also: every thread's y is in s_x
    float *__restrict__ o = out + base + t0;
    for (int q = tid; q < CP_T && q < left; q += CP_THREADS) o[q] = s_x[cp_idx(q)];
    if (tid == 0) {
        top = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
        if (top > 0.0) atomicMax(max_bits + sig, (unsigned long long)__double_as_longlong(top));   // non-negative doubles order like their bits
    }
}

int launch_compress(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, const double *coef, const double *pows,
                    const int32_t *tiles, int64_t n_tiles, float *out, double *max_reduction, double *curve, double *rsum,
                    double *rstart, double *asum, double *astart, int32_t *first_tile, double *xl, hipStream_t st)
{
    if (n <= 0) return GOOFER_OK;
    HIP_TRY(ctx, hipMemsetAsync(max_reduction, 0, sizeof(double) * (size_t)n, st));       // +0.0: no reduction
    if (n_tiles <= 0) return GOOFER_OK;
    HIP_TRY(ctx, hipMemsetAsync(first_tile, 0xff, sizeof(int32_t) * (size_t)n, st));      // -1: no tile seen
    const int skip = ctx->compress_skip ? 1 : 0;
    const dim3 gt((unsigned)n_tiles), gs((unsigned)n), blk(CP_THREADS);
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(max_reduction);
    if (xl)
        hipLaunchKernelGGL(k_cp_release_sum<1>, gt, blk, 0, st, x, in_off, n, coef, pows, tiles, skip, rsum, first_tile, xl);
    else
        hipLaunchKernelGGL(k_cp_release_sum<0>, gt, blk, 0, st, x, in_off, n, coef, pows, tiles, skip, rsum, first_tile, xl);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_cp_release_carry, gs, blk, 0, st, in_off, n_tiles, pows, (const double *)rsum, (const int32_t *)first_tile, rstart);
    LAUNCH_CHECK(ctx);
    if (xl)
        hipLaunchKernelGGL(k_cp_attack_sum<2>, gt, blk, 0, st, x, in_off, n, coef, pows, tiles, skip, (const double *)rstart, asum, xl);
    else
        hipLaunchKernelGGL(k_cp_attack_sum<0>, gt, blk, 0, st, x, in_off, n, coef, pows, tiles, skip, (const double *)rstart, asum, xl);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_cp_attack_carry, gs, blk, 0, st, in_off, n_tiles, pows, (const double *)asum, (const int32_t *)first_tile, astart);
    LAUNCH_CHECK(ctx);
    if (xl)
        hipLaunchKernelGGL(k_cp_apply<2>, gt, blk, 0, st, x, in_off, n, coef, pows, tiles, skip, (const double *)rstart,
                           (const double *)astart, out, bits, curve, xl);
    else
        hipLaunchKernelGGL(k_cp_apply<0>, gt, blk, 0, st, x, in_off, n, coef, pows, tiles, skip, (const double *)rstart,
                           (const double *)astart, out, bits, curve, xl);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

extern "C" int goofer_compress(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, const double *coef,
                               const double *pows, const int32_t *tiles, int64_t n_tiles, float *out, double *max_reduction, double *curve,
                               void *scratch, int64_t *scratch_bytes, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (int rc = check_counts(ctx, "goofer_compress", n, total, n_tiles)) return rc;
    if (!signal_tiles_ok(CP_T, n, total, n_tiles))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_compress: %lld tiles for %lld samples in %d signals is not a geometry of goofer_host_compress_plan",
                           (long long)n_tiles, (long long)total, n);
    if (!scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_compress: null pointer (scratch_bytes)");
    double *rsum, *rstart, *asum, *astart, *xl = nullptr;
    int32_t *first_tile;
    const bool store = ctx->compress_store;
    auto carve = [&](arena &a) {
        rsum = a.take<double>(2 * (size_t)n_tiles);
        rstart = a.take<double>((size_t)n_tiles);
        asum = a.take<double>((size_t)n_tiles);
        astart = a.take<double>((size_t)n_tiles);
        first_tile = a.take<int32_t>((size_t)n);
        if (store) xl = a.take<double>((size_t)total);
    };
    if (scratch) {
        if (n > 0 && (!in_off || !coef || !pows || !max_reduction || (total > 0 && (!x || !tiles || !out))))
            return goofer_fail(ctx, GOOFER_EINVAL, "goofer_compress: null pointer");
        if (int rc = check_aligned(ctx, "goofer_compress", "x, tiles and out", {x, tiles, out}, "in_off, coef, pows, max_reduction, curve and scratch",
                                   {in_off, coef, pows, max_reduction, curve, scratch}))
            return rc;
        if (int rc = check_overlap(ctx, "goofer_compress", x, out, total, true)) return rc;
    }
    int rc = caller_scratch(ctx, scratch, scratch_bytes, "goofer_compress", carve);
    if (rc || !scratch) return rc;
    return launch_compress(ctx, x, in_off, n, coef, pows, tiles, n_tiles, out, max_reduction, curve, rsum, rstart, asum, astart, first_tile,
                           store ? xl : nullptr, (hipStream_t)stream);
}
