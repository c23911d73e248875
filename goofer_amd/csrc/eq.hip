// The parametric equaliser on the device (gfx950): a cascade of K <= 8 biquads in fp64 over every signal of a ragged batch, the
// filtered signal written out as fp32.  The definition (bands, coefficients, recurrence, tolerance) is in include/goofer_hip.h;
// the host half, goofer_host_eq_plan (planner.hip), makes the coefficients, the tile table and the matrix powers.
//
// The cascade is a linear recurrence of order 2K, state s = (u_1[i-1], u_1[i-2], .., u_K[i-1], u_K[i-2]): a run of m samples
// from s ends in T^m s + e, e the end state of the same run from zero.  Between runs and tiles the state travels as
// (u_k[i-1], u_k[i-1] - u_k[i-2]) per section, and the planner's powers are those of T in these coordinates.
// The scheme is that of tile_scan.h: a signal is cut into tiles of 4096 samples and a tile into 256 runs of 16, and states are
// carried by scans whose operator is "multiply by a constant matrix, add".  What is this stage's own is the order 2K, up to 16.
// A scan with the coupled 2K x 2K matrix inside every tile would cost
// 8 levels x 4 K^2 fused multiply-adds a thread against the 80 K of the 16 samples themselves, and 64 KiB of LDS.  So inside a
// tile the sections run one after another: the state of section k - 1 in front of a run is exactly the input history section k
// needs there, and once section k - 1 has run from its true state, section k is a recurrence of order 2 over a known input: a
// zero-state run, a scan with the section's own 2 x 2 powers (the diagonal blocks of T^(16 * 2^j)), the run again from its true
// state.  Only the carry from tile to tile needs the coupled matrix, T^(4096 * 2^j), once per tile instead of once per run.
// Three launches in stream order; no workgroup waits for another one, and every sum has a fixed order:
//   A  k_eq_tile<false>  a workgroup per tile: the cascade from a zero state, the tile's end state (2K numbers) to scratch
//   B  k_eq_carry<K>     a workgroup per signal: the tiles' end states into the tiles' true start states, 4096 tiles a round; the
//                        matrices sit in SGPRs (uniform loads), block lower triangular: 2 K (K + 1) products
//   C  k_eq_tile<true>   every tile again from its true start state, y through LDS to coalesced stores
#include "tile_scan.h"

static_assert(GOOFER_EQ_TILE == TS_T && GOOFER_EQ_SPT == TS_SPT && GOOFER_EQ_LEVELS == TS_LEVELS && GOOFER_EQ_RUN_TILES == TS_RUN, "the tiling of tile_scan.h");
#define EQ_XPAD TS_XPAD(16)                           // the tile and the 16 samples in front of it

// One section over the thread's 16 samples u (its input on entry, its output on return) with the input history (h1, h2) and
// the section's state (s1, s2) in front of the run; returns the state behind it in (s1, s2).  KEEP false: u is left as it was
template <bool KEEP>
__device__ __forceinline__ void eq_run(double (&u)[TS_SPT], double h1, double h2, double &s1, double &s2, double b0, double b1, double b2,
                                       double a1, double a2)
{
#pragma unroll
    for (int e = 0; e < TS_SPT; ++e) {
        const double x = u[e];
        const double y = (((b0 * x + b1 * h1) + b2 * h2) - a1 * s1) - a2 * s2;
        h2 = h1, h1 = x, s2 = s1, s1 = y;
        if (KEEP) u[e] = y;
    }
}

// WRITE false: pass A, every section from a zero state, the tile's end state to ends.  WRITE true: pass C, from starts, y to out
template <bool WRITE>
__global__ __launch_bounds__(TS_THREADS)
void k_eq_tile(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, int K, const double *__restrict__ coef,
               const double *__restrict__ mats, const int32_t *__restrict__ tiles, const double *__restrict__ starts,
               double *__restrict__ ends, int32_t *__restrict__ first_tile, float *__restrict__ out)
{
    __shared__ float s_x[EQ_XPAD];
    __shared__ double s_sc[2][2 * TS_THREADS];
    int sig, kt;
    int64_t base, len, t0;
    if (!ts_tile(tiles, in_off, n, sig, kt, base, len, t0)) return;
    const int tid = threadIdx.x;
    if (!WRITE) ts_first_tile(first_tile, sig, kt);
    ts_stage<16>(x + base, len, t0, s_x);
    __syncthreads();
    const int q0 = 16 + tid * TS_SPT;
    double u[TS_SPT], h1 = (double)s_x[ts_idx(q0 - 1)], h2 = (double)s_x[ts_idx(q0 - 2)];
#pragma unroll
    for (int e = 0; e < TS_SPT; ++e) u[e] = (double)s_x[ts_idx(q0 + e)];
    int cur = 0;
    for (int k = 0; k < K; ++k) {
        const double *__restrict__ c = coef + 5 * k;
        const double *__restrict__ P = mats + 4 * TS_LEVELS * k;   // the section's own powers: P + 4 j is its T^(16 * 2^j)
        const double b0 = c[0], b1 = c[1], b2 = c[2], a1 = c[3], a2 = c[4];
        double st1 = 0.0, st2 = 0.0;                            // the section's state in front of the tile, as (u[i-1], u[i-1] - u[i-2])
        if (WRITE) st1 = starts[2 * K * (int64_t)blockIdx.x + 2 * k], st2 = starts[2 * K * (int64_t)blockIdx.x + 2 * k + 1];
        double v[2] = {0.0, 0.0};
        eq_run<false>(u, h1, h2, v[0], v[1], b0, b1, b2, a1, a2);
        v[1] = v[0] - v[1];                                     // carried as (u[i-1], u[i-1] - u[i-2]): the powers are well scaled there
        // the section's scan combination at level l: v <- P_l o + v
        const auto level = [&](const double (&o)[2], int l, double (&w)[2]) {
            const double r1 = P[4 * l] * o[0] + P[4 * l + 1] * o[1], r2 = P[4 * l + 2] * o[0] + P[4 * l + 3] * o[1];
            w[0] = r1 + w[0], w[1] = r2 + w[1];
        };
        if (WRITE && tid == 0) level({st1, st2}, 0, v);
        cur = ts_scan(v, level, s_sc, cur);
        if (tid > 0) st1 = s_sc[cur][tid - 1], st2 = s_sc[cur][TS_THREADS + tid - 1];
        if (!WRITE && tid == TS_THREADS - 1) ends[2 * K * (int64_t)blockIdx.x + 2 * k] = v[0], ends[2 * K * (int64_t)blockIdx.x + 2 * k + 1] = v[1];
        // the run again from its true state; that state is the next section's input history
        st2 = st1 - st2;                                        // back to u[i-2]
        double s1 = st1, s2 = st2;
        eq_run<true>(u, h1, h2, s1, s2, b0, b1, b2, a1, a2);
        h1 = st1, h2 = st2;
        cur ^= 1;                                               // (the next section's first store goes to the buffer nobody reads now)
    }
    if (!WRITE) return;
    __syncthreads();                                            // (K == 0 never gets here: every read of s_x lies in front of a barrier above)
#pragma unroll
    for (int e = 0; e < TS_SPT; ++e) s_x[ts_idx(q0 + e)] = (float)u[e];
    __syncthreads();
    float *__restrict__ ys = out + base;
    for (int q = 16 + tid; q < TS_T + 16; q += TS_THREADS) {
        const int64_t p = t0 - 16 + q;
        if (p < len) ys[p] = s_x[ts_idx(q)];
    }
}

// r = M s for the block lower triangular M (D x D, row-major): row i reaches column (i | 1); each row summed in ascending column
template <int D>
__device__ __forceinline__ void eq_matvec(const double *__restrict__ M, const double (&s)[D], double (&r)[D])
{
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double a = M[D * i] * s[0];
#pragma unroll
        for (int j = 1; j <= (i | 1); ++j) a += M[D * i + j] * s[j];
        r[i] = a;
    }
}

// starts[tile] = the true state in front of the tile: 0 for a signal's first, T^4096 starts[t] + ends[t] for tile t + 1.  One
// workgroup per signal, 4096 tiles a round, the walk of ts_carry (tile_scan.h) written out for elements of 2K doubles: a thread
// walks TS_RUN consecutive tiles from zero, the workgroup scans the threads' end states with T^(4096 * 16 * 2^l) (the state in
// front of the round goes through thread 0's run), and every thread walks its tiles again from its true state.  What differs
// from ts_carry: the tiles' end states are read again from memory on the second walk (16 of them at order 16 do not fit the
// registers), a walk ends at the signal's last tile, and the scan works in one buffer, a barrier between a level's loads and
// its stores, which keeps K = 8 at 32 KiB of LDS.  It is written out for measured speed alone: on ts_carry with these three
// as a second form, k_eq_carry<4> was 2 us slower (docs/EXPERIMENTS.md).  The walk is the accurate part (a true state times T^4096 cancels nothing); the scan above it
// only matters where T^65536 is not yet nothing.
template <int K>
__global__ __launch_bounds__(TS_THREADS)
void k_eq_carry(const int64_t *__restrict__ in_off, int n, int64_t n_tiles, const double *__restrict__ mats, const double *__restrict__ ends,
                const int32_t *__restrict__ first_tile, double *__restrict__ starts)
{
    constexpr int D = 2 * K;
    __shared__ double s_sc[D * TS_THREADS];
    const int tid = threadIdx.x;
    int nt;
    int64_t first;
    if (!ts_signal(in_off, n_tiles, first_tile, nt, first)) return;
    const double *__restrict__ P0 = mats + 4 * TS_LEVELS * K;   // T^4096: one tile
    const double *__restrict__ PR = P0 + D * D;                 // T^(4096 * 16): a thread's run; level l of the scan: PR + D D l
    double carry[D];
#pragma unroll
    for (int i = 0; i < D; ++i) carry[i] = 0.0;
    for (int c = 0; c < nt; c += TS_THREADS * TS_RUN) {
        const int t0 = c + tid * TS_RUN;
        double v[D], o[D], r[D];
#pragma unroll
        for (int i = 0; i < D; ++i) v[i] = 0.0;
#pragma unroll 1
        for (int e = 0; e < TS_RUN; ++e) {
            if (t0 + e >= nt) break;                            // (what lies behind the signal's last tile reaches no tile)
            eq_matvec<D>(P0, v, r);
#pragma unroll
            for (int i = 0; i < D; ++i) v[i] = r[i] + ends[D * (first + t0 + e) + i];
        }
        if (tid == 0) {
            eq_matvec<D>(PR, carry, r);
#pragma unroll
            for (int i = 0; i < D; ++i) v[i] = r[i] + v[i];
        }
#pragma unroll
        for (int i = 0; i < D; ++i) s_sc[i * TS_THREADS + tid] = v[i];
        __syncthreads();
        for (int l = 0; l < TS_LEVELS; ++l) {
            const int off = 1 << l;
            if (tid >= off) {
#pragma unroll
                for (int i = 0; i < D; ++i) o[i] = s_sc[i * TS_THREADS + tid - off];
            }
            __syncthreads();                                    // (everyone has read the level below)
            if (tid >= off) {
                eq_matvec<D>(PR + D * D * l, o, r);
#pragma unroll
                for (int i = 0; i < D; ++i) v[i] = r[i] + v[i];
#pragma unroll
                for (int i = 0; i < D; ++i) s_sc[i * TS_THREADS + tid] = v[i];
            }
            __syncthreads();
        }
        double st[D];
#pragma unroll
        for (int i = 0; i < D; ++i) st[i] = tid == 0 ? carry[i] : s_sc[i * TS_THREADS + tid - 1];
#pragma unroll
        for (int i = 0; i < D; ++i) carry[i] = s_sc[i * TS_THREADS + TS_THREADS - 1];
#pragma unroll 1
        for (int e = 0; e < TS_RUN; ++e) {
            if (t0 + e >= nt) break;
#pragma unroll
            for (int i = 0; i < D; ++i) starts[D * (first + t0 + e) + i] = st[i];
            eq_matvec<D>(P0, st, r);
#pragma unroll
            for (int i = 0; i < D; ++i) st[i] = r[i] + ends[D * (first + t0 + e) + i];
        }
        __syncthreads();                                        // (the next round writes the buffer read above)
    }
}

template <int K>
static int launch_eq_carry(goofer_ctx *ctx, int want, const int64_t *in_off, int n, int64_t n_tiles, const double *mats, const double *ends,
                           const int32_t *first_tile, double *starts, hipStream_t st)
{
    if constexpr (K > 1) {
        if (want != K) return launch_eq_carry<K - 1>(ctx, want, in_off, n, n_tiles, mats, ends, first_tile, starts, st);
    }
    hipLaunchKernelGGL(k_eq_carry<K>, dim3((unsigned)n), dim3(TS_THREADS), 0, st, in_off, n, n_tiles, mats, ends, first_tile, starts);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

int launch_eq(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int K, const double *coef, const double *mats,
              const int32_t *tiles, int64_t n_tiles, float *out, double *ends, double *starts, int32_t *first_tile, hipStream_t st)
{
    if (n <= 0 || total <= 0 || n_tiles <= 0) return GOOFER_OK;
    if (K == 0) {
        HIP_TRY(ctx, hipMemcpyAsync(out, x, sizeof(float) * (size_t)total, hipMemcpyDeviceToDevice, st));
        return GOOFER_OK;
    }
    if (int rc = ts_first_tile_reset(ctx, first_tile, n, st)) return rc;
    hipLaunchKernelGGL(k_eq_tile<false>, dim3((unsigned)n_tiles), dim3(TS_THREADS), 0, st, x, in_off, n, K, coef, mats, tiles,
                       (const double *)nullptr, ends, first_tile, (float *)nullptr);
    LAUNCH_CHECK(ctx);
    if (int rc = launch_eq_carry<GOOFER_EQ_MAX_BANDS>(ctx, K, in_off, n, n_tiles, mats, ends, first_tile, starts, st)) return rc;
    hipLaunchKernelGGL(k_eq_tile<true>, dim3((unsigned)n_tiles), dim3(TS_THREADS), 0, st, x, in_off, n, K, coef, mats, tiles,
                       (const double *)starts, (double *)nullptr, (int32_t *)nullptr, out);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

extern "C" int goofer_eq(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int K, const double *coef,
                         const double *mats, const int32_t *tiles, int64_t n_tiles, float *out, void *scratch, int64_t *scratch_bytes,
                         void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (int rc = check_counts(ctx, "goofer_eq", n, total, n_tiles)) return rc;
    if (K < 0 || K > GOOFER_EQ_MAX_BANDS || !signal_tiles_ok(TS_T, n, total, n_tiles))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_eq: %d bands, %lld tiles for %lld samples in %d signals is not a geometry of goofer_host_eq_plan",
                           K, (long long)n_tiles, (long long)total, n);
    if (!scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_eq: null pointer (scratch_bytes)");
    double *ends, *starts;
    int32_t *first_tile;
    auto carve = [&](arena &a) {
        ends = a.take<double>(2 * (size_t)K * (size_t)n_tiles);
        starts = a.take<double>(2 * (size_t)K * (size_t)n_tiles);
        first_tile = a.take<int32_t>((size_t)n);
    };
    if (scratch) {
        if (n > 0 && total > 0 && (!x || !in_off || !tiles || !out || (K > 0 && (!coef || !mats))))
            return goofer_fail(ctx, GOOFER_EINVAL, "goofer_eq: null pointer");
        if (int rc = check_aligned(ctx, "goofer_eq", "x, tiles and out", {x, tiles, out}, "in_off, coef, mats and scratch", {in_off, coef, mats, scratch}))
            return rc;
        if (int rc = check_overlap(ctx, "goofer_eq", x, out, total, false)) return rc;
    }
    int rc = caller_scratch(ctx, scratch, scratch_bytes, "goofer_eq", carve);
    if (rc || !scratch) return rc;
    return launch_eq(ctx, x, in_off, n, total, K, coef, mats, tiles, n_tiles, out, ends, starts, first_tile, (hipStream_t)stream);
}
