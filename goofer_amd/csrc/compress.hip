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
// once the release states are known.  Tiles, runs, scans and the tile-to-tile carries are those of tile_scan.h (a signal is cut
// into tiles of 4096 samples and a tile into 256 runs of 16); five launches in stream order, no workgroup waits for another
// one, and every combination has a fixed order:
//   1  k_cp_release_sum    a workgroup per tile: xl, runs from (0, 0), a workgroup scan, the tile's (C, B) to scratch
//   2  k_cp_release_carry  a workgroup per signal: the tiles' (C, B) into the release state in front of every tile
//   3  k_cp_attack_sum     a workgroup per tile: y1 from the true state, the attack runs from 0, a scan, the tile's end state
//   4  k_cp_attack_carry   a workgroup per signal: those into the attack state in front of every tile
//   5  k_cp_apply          a workgroup per tile: y1, yl, g from the true states; y, the curve, the tile's greatest yl
#include "tile_scan.h"

#define CP_POWS GOOFER_COMPRESS_POWS
static_assert(GOOFER_COMPRESS_TILE == TS_T && GOOFER_COMPRESS_SPT == TS_SPT && GOOFER_COMPRESS_LEVELS == TS_LEVELS && GOOFER_COMPRESS_RUN_TILES == TS_RUN,
              "the tiling of tile_scan.h");
static_assert(CP_POWS == TS_LEVELS + 4 + TS_LEVELS && TS_RUN == 16, "a^16 .. a^2048 inside a tile, a^4096 a tile, a^(4096 * 16 * 2^k) over the runs of 16 tiles");
static_assert(GOOFER_COMPRESS_ROUND_TILES == TS_THREADS * TS_RUN, "a round of the carry kernels");
#define CP_XPAD TS_XPAD(0)                            // the tile alone

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

// MODE 0: xl of the thread's 16 samples from the staged tile; 1: likewise, and written to xlbuf (the tile's, [T]); 2: read from it
template <int MODE>
__device__ __forceinline__ void cp_levels(const cp_par &P, const float *__restrict__ s_x, double *__restrict__ xlbuf, int64_t left,
                                          double (&xl)[TS_SPT])
{
    const int q0 = threadIdx.x * TS_SPT;
#pragma unroll
    for (int e = 0; e < TS_SPT; ++e) {
        if (MODE == 2) {
            xl[e] = q0 + e < left ? xlbuf[q0 + e] : 0.0;
        } else {
            xl[e] = q0 + e < left ? P.xl(s_x[ts_idx(q0 + e)]) : 0.0;     // (past the end: xl = 0 whatever T is)
            if (MODE == 1 && q0 + e < left) xlbuf[q0 + e] = xl[e];
        }
    }
}

// the release maps of the thread's 16 samples composed onto (C, B)
__device__ __forceinline__ void cp_release_run(const cp_par &P, const double (&xl)[TS_SPT], double &C, double &B)
{
#pragma unroll
    for (int e = 0; e < TS_SPT; ++e) {
        const double b = P.bR * xl[e];
        C = fmax(xl[e], P.aR * C + b);
        B = P.aR * B + b;
    }
}

// The scans' combinations at level k, pw[k] the A of an element of level k (ts_scan).  Release: (C, B) <- (Co, Bo) then (C, B)
struct cp_release_level {
    const double *__restrict__ pw;
    __device__ __forceinline__ void operator()(const double (&o)[2], int k, double (&v)[2]) const
    {
        const double A = pw[k];
        v[0] = fmax(v[0], A * o[0] + v[1]);
        v[1] = A * o[1] + v[1];
    }
};
// attack, linear: v <- pw[k] o + v
struct cp_attack_level {
    const double *__restrict__ pw;
    __device__ __forceinline__ void operator()(const double (&o)[1], int k, double (&v)[1]) const { v[0] = pw[k] * o[0] + v[0]; }
};

template <int MODE>
__global__ __launch_bounds__(TS_THREADS)
void k_cp_release_sum(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, const double *__restrict__ coef,
                      const double *__restrict__ pows, const int32_t *__restrict__ tiles, int skip, double *__restrict__ rsum,
                      int32_t *__restrict__ first_tile, double *__restrict__ xlbuf)
{
    __shared__ float s_x[CP_XPAD];
    __shared__ double s_sc[2][2 * TS_THREADS];
    int sig, kt;
    int64_t base, len, t0;
    if (!ts_tile(tiles, in_off, n, sig, kt, base, len, t0)) return;
    ts_first_tile(first_tile, sig, kt);
    const cp_par P(coef, skip);
    ts_stage<0>(x + base, len, t0, s_x);
    __syncthreads();
    double xl[TS_SPT], v[2] = {0.0, 0.0};
    cp_levels<MODE>(P, s_x, MODE ? xlbuf + base + t0 : nullptr, len - t0, xl);
    cp_release_run(P, xl, v[0], v[1]);
    ts_scan(v, cp_release_level{pows}, s_sc);
    if (threadIdx.x == TS_THREADS - 1) rsum[2 * (int64_t)blockIdx.x] = v[0], rsum[2 * (int64_t)blockIdx.x + 1] = v[1];
}

// rstart[tile] = the release state in front of the tile: 0 for a signal's first, max(C_t, aR^4096 rstart[t] + B_t) for tile
// t + 1 (ts_carry, GOOFER_COMPRESS_ROUND_TILES tiles a round).  Thread 0 composes its tiles from the state in front of the
// round: a known state y0 is the element (y0, y0).
struct cp_release_carry {
    double A;                                                   // aR^4096: one tile
    cp_release_level lv;                                        // aR^(4096 * 16): a thread's run; level k of the scan: lv.pw[k]
    __device__ __forceinline__ void seed(double (&v)[2], const double (&carry)[1]) const { v[0] = v[1] = carry[0]; }
    __device__ __forceinline__ void append(double (&v)[2], const double (&z)[2]) const
    {
        v[0] = fmax(z[0], A * v[0] + z[1]);
        v[1] = A * v[1] + z[1];
    }
    __device__ __forceinline__ void join(double (&)[2], const double (&)[1]) const {}
    __device__ __forceinline__ void level(const double (&o)[2], int k, double (&v)[2]) const { lv(o, k, v); }
    __device__ __forceinline__ void step(double (&st)[1], const double (&z)[2]) const { st[0] = fmax(z[0], A * st[0] + z[1]); }
};

__global__ __launch_bounds__(TS_THREADS)
void k_cp_release_carry(const int64_t *__restrict__ in_off, int64_t n_tiles, const double *__restrict__ pows, const double *__restrict__ rsum,
                        const int32_t *__restrict__ first_tile, double *__restrict__ rstart)
{
    ts_carry<2, 1>(in_off, n_tiles, first_tile, rsum, rstart, cp_release_carry{pows[TS_LEVELS], {pows + TS_LEVELS + 4}});
}

// the tile's xl and, from the release state in front of the tile, the release state in front of the thread's run
template <int MODE>
__device__ __forceinline__ double cp_release_states(const cp_par &P, const float *__restrict__ s_x, double *__restrict__ xlbuf, int64_t left,
                                                    const double *__restrict__ pows, double st, double (*s_sc)[2 * TS_THREADS],
                                                    double (&xl)[TS_SPT])
{
    cp_levels<MODE>(P, s_x, xlbuf, left, xl);
    double v[2];
    v[0] = v[1] = threadIdx.x == 0 ? st : 0.0;
    cp_release_run(P, xl, v[0], v[1]);
    const int cur = ts_scan(v, cp_release_level{pows}, s_sc);
    const double y1 = threadIdx.x == 0 ? st : s_sc[cur][threadIdx.x - 1];
    __syncthreads();                                            // (the attack scan writes the buffers read above)
    return y1;
}

// xl[e] <- y1 of the thread's samples from the state y1 in front of them; the attack recurrence over them from yl (left in yl)
__device__ __forceinline__ void cp_detector_run(const cp_par &P, double (&xl)[TS_SPT], double y1, double &yl)
{
#pragma unroll
    for (int e = 0; e < TS_SPT; ++e) {
        y1 = fmax(xl[e], P.aR * y1 + P.bR * xl[e]);
        yl = P.aA * yl + P.bA * y1;
        xl[e] = y1;
    }
}

template <int MODE>
__global__ __launch_bounds__(TS_THREADS)
void k_cp_attack_sum(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, const double *__restrict__ coef,
                     const double *__restrict__ pows, const int32_t *__restrict__ tiles, int skip, const double *__restrict__ rstart,
                     double *__restrict__ asum, double *__restrict__ xlbuf)
{
    __shared__ float s_x[CP_XPAD];
    __shared__ double s_sc[2][2 * TS_THREADS];
    int sig, kt;
    int64_t base, len, t0;
    if (!ts_tile(tiles, in_off, n, sig, kt, base, len, t0)) return;
    const cp_par P(coef, skip);
    if (MODE != 2) {
        ts_stage<0>(x + base, len, t0, s_x);
        __syncthreads();
    }
    double xl[TS_SPT];
    const double y1 = cp_release_states<MODE == 2 ? 2 : 0>(P, s_x, MODE == 2 ? xlbuf + base + t0 : nullptr, len - t0, pows,
                                                           rstart[blockIdx.x], s_sc, xl);
    double v[1] = {0.0};
    cp_detector_run(P, xl, y1, v[0]);
    ts_scan(v, cp_attack_level{pows + CP_POWS}, s_sc);
    if (threadIdx.x == TS_THREADS - 1) asum[blockIdx.x] = v[0];
}

// astart[tile] = the attack state in front of the tile: 0 for a signal's first, aA^4096 astart[t] + asum[t] for tile t + 1; as
// the release carry with a linear element, thread 0's walk starting from the state in front of the round.
struct cp_attack_carry {
    double A;
    cp_attack_level lv;
    __device__ __forceinline__ void seed(double (&v)[1], const double (&carry)[1]) const { v[0] = carry[0]; }
    __device__ __forceinline__ void append(double (&v)[1], const double (&z)[1]) const { v[0] = A * v[0] + z[0]; }
    __device__ __forceinline__ void join(double (&)[1], const double (&)[1]) const {}
    __device__ __forceinline__ void level(const double (&o)[1], int k, double (&v)[1]) const { lv(o, k, v); }
    __device__ __forceinline__ void step(double (&st)[1], const double (&z)[1]) const { append(st, z); }
};

__global__ __launch_bounds__(TS_THREADS)
void k_cp_attack_carry(const int64_t *__restrict__ in_off, int64_t n_tiles, const double *__restrict__ pows, const double *__restrict__ asum,
                       const int32_t *__restrict__ first_tile, double *__restrict__ astart)
{
    ts_carry<1, 1>(in_off, n_tiles, first_tile, asum, astart, cp_attack_carry{pows[CP_POWS + TS_LEVELS], {pows + CP_POWS + TS_LEVELS + 4}});
}

template <int MODE>
__global__ __launch_bounds__(TS_THREADS)
void k_cp_apply(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, const double *__restrict__ coef,
                const double *__restrict__ pows, const int32_t *__restrict__ tiles, int skip, const double *__restrict__ rstart,
                const double *__restrict__ astart, float *__restrict__ out, unsigned long long *__restrict__ max_bits,
                double *__restrict__ curve, double *__restrict__ xlbuf)
{
    __shared__ float s_x[CP_XPAD];
    __shared__ double s_sc[2][2 * TS_THREADS];
    __shared__ double s_red[TS_THREADS / 64];
    int sig, kt;
    int64_t base, len, t0;
    if (!ts_tile(tiles, in_off, n, sig, kt, base, len, t0)) return;
    const int tid = threadIdx.x;
    const cp_par P(coef, skip);
    ts_stage<0>(x + base, len, t0, s_x);                        // (x is needed for y whatever MODE is)
    __syncthreads();
    const int64_t left = len - t0;
    double y1s[TS_SPT];
    const double y1 = cp_release_states<MODE == 2 ? 2 : 0>(P, s_x, MODE == 2 ? xlbuf + base + t0 : nullptr, left, pows, rstart[blockIdx.x],
                                                           s_sc, y1s);
    const double a0 = astart[blockIdx.x];
    double v[1] = {tid == 0 ? a0 : 0.0};
    cp_detector_run(P, y1s, y1, v[0]);
    const int cur = ts_scan(v, cp_attack_level{pows + CP_POWS}, s_sc);
    double yl = tid == 0 ? a0 : s_sc[cur][tid - 1], top = 0.0;
    const int q0 = tid * TS_SPT;
    double *__restrict__ cv = curve ? curve + base + t0 : nullptr;
#pragma unroll
    for (int e = 0; e < TS_SPT; ++e) {
        yl = P.aA * yl + P.bA * y1s[e];
        if (q0 + e < left) {
            const double ex = (P.M - yl) / 20.0;
            const double g = ex == 0.0 ? 1.0 : exp10(ex);       // (the identity property: 10^0 is exactly 1 whatever exp10 makes of it)
            s_x[ts_idx(q0 + e)] = (float)((double)s_x[ts_idx(q0 + e)] * g);
            top = yl > top ? yl : top;                          // (yl >= 0; a NaN is not taken)
            if (cv) cv[q0 + e] = yl;
        }
    }
    auto top_of = [](double a, double b) { return fmax(a, b); };
    top = ts_wave_reduce(top, top_of);
    if ((tid & 63) == 0) s_red[tid >> 6] = top;
    __syncthreads();                                            // also: every thread's y is in s_x
    float *__restrict__ o = out + base + t0;
    for (int q = tid; q < TS_T && q < left; q += TS_THREADS) o[q] = s_x[ts_idx(q)];
    if (tid == 0) {
        top = ts_waves(top_of, s_red);                          // (in order, where this was pairwise: the same bits only because
                                                                //  top is never NaN or -0 and fmax of such values is associative)
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
    if (int rc = ts_first_tile_reset(ctx, first_tile, n, st)) return rc;
    const int skip = ctx->compress_skip ? 1 : 0;
    const dim3 gt((unsigned)n_tiles), gs((unsigned)n), blk(TS_THREADS);
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
    if (!signal_tiles_ok(TS_T, n, total, n_tiles))
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
