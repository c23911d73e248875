// The parametric equaliser on the device (gfx950): a cascade of K <= 8 biquads in fp64 over every signal of a ragged batch, the
// filtered signal written out as fp32.  The definition (bands, coefficients, recurrence, tolerance) is in include/goofer_hip.h;
// the host half, goofer_host_eq_plan (planner.hip), makes the coefficients, the tile table and the matrix powers.
//
// The cascade is a linear recurrence of order 2K, state s = (u_1[i-1], u_1[i-2], .., u_K[i-1], u_K[i-2]): a run of m samples
// from s ends in T^m s + e, e the end state of the same run from zero.  Between runs and tiles the state travels as
// (u_k[i-1], u_k[i-1] - u_k[i-2]) per section, and the planner's powers are those of T in these coordinates.
// As in loudness.hip a signal is cut into tiles of 4096 samples and a tile into 256 runs of 16, and states are carried by
// scans whose operator is "multiply by a constant matrix, add".  What differs is the order 2K, up to 16.  A scan with the coupled 2K x 2K matrix inside every tile would cost
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
#include "launchers.h"

#define EQ_THREADS 256
#define EQ_SPT GOOFER_EQ_SPT
#define EQ_T GOOFER_EQ_TILE
#define EQ_LEVELS GOOFER_EQ_LEVELS
static_assert(EQ_T == EQ_THREADS * EQ_SPT && EQ_SPT == 16 && (1 << EQ_LEVELS) == EQ_THREADS, "one workgroup of 256 runs of 16 per tile");
#define EQ_RUN GOOFER_EQ_RUN_TILES                     // tiles a thread of k_eq_carry walks
#define EQ_XPAD (EQ_T + 16 + (EQ_T + 16) / 16)       // the tile and the 16 samples in front of it, one pad word per 16 (LD_XPAD)

// entry q of the staged samples (q = 16 + position in the tile): a thread's 16 consecutive words at a lane stride of 17
__device__ __forceinline__ int eq_idx(int q) { return q + (q >> 4); }

// a tile's signal and place from the planner's table; false for a pair that is not the planner's (nothing is read or written)
__device__ __forceinline__ bool eq_tile(const int32_t *__restrict__ tiles, const int64_t *__restrict__ in_off, int n, int &sig, int &kt,
                                        int64_t &base, int64_t &len, int64_t &t0)
{
    sig = __builtin_amdgcn_readfirstlane(tiles[2 * blockIdx.x]), kt = __builtin_amdgcn_readfirstlane(tiles[2 * blockIdx.x + 1]);
    if (sig < 0 || sig >= n || kt < 0) return false;
    base = in_off[sig], len = in_off[sig + 1] - base, t0 = (int64_t)kt * EQ_T;
    return t0 < len && len < ((int64_t)1 << 31);
}

// One section over the thread's 16 samples u (its input on entry, its output on return) with the input history (h1, h2) and
// the section's state (s1, s2) in front of the run; returns the state behind it in (s1, s2).  KEEP false: u is left as it was
template <bool KEEP>
__device__ __forceinline__ void eq_run(double (&u)[EQ_SPT], double h1, double h2, double &s1, double &s2, double b0, double b1, double b2,
                                       double a1, double a2)
{
#pragma unroll
    for (int e = 0; e < EQ_SPT; ++e) {
        const double x = u[e];
        const double y = (((b0 * x + b1 * h1) + b2 * h2) - a1 * s1) - a2 * s2;
        h2 = h1, h1 = x, s2 = s1, s1 = y;
        if (KEEP) u[e] = y;
    }
}

// WRITE false: pass A, every section from a zero state, the tile's end state to ends.  WRITE true: pass C, from starts, y to out
template <bool WRITE>
__global__ __launch_bounds__(EQ_THREADS)
void k_eq_tile(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, int K, const double *__restrict__ coef,
               const double *__restrict__ mats, const int32_t *__restrict__ tiles, const double *__restrict__ starts,
               double *__restrict__ ends, int32_t *__restrict__ first_tile, float *__restrict__ out)
{
    __shared__ float s_x[EQ_XPAD];
    __shared__ double s_sc[2][2 * EQ_THREADS];
    int sig, kt;
    int64_t base, len, t0;
    if (!eq_tile(tiles, in_off, n, sig, kt, base, len, t0)) return;
    const int tid = threadIdx.x;
    if (!WRITE && tid == 0 && kt == 0) first_tile[sig] = (int32_t)blockIdx.x;
    const float *__restrict__ xs = x + base;
    for (int q = 14 + tid; q < EQ_T + 16; q += EQ_THREADS) {    // (coalesced; 0 outside the signal)
        const int64_t p = t0 - 16 + q;
        s_x[eq_idx(q)] = p >= 0 && p < len ? xs[p] : 0.0f;
    }
    __syncthreads();
    const int q0 = 16 + tid * EQ_SPT;
    double u[EQ_SPT], h1 = (double)s_x[eq_idx(q0 - 1)], h2 = (double)s_x[eq_idx(q0 - 2)];
#pragma unroll
    for (int e = 0; e < EQ_SPT; ++e) u[e] = (double)s_x[eq_idx(q0 + e)];
    int cur = 0;
    for (int k = 0; k < K; ++k) {
        const double *__restrict__ c = coef + 5 * k;
        const double *__restrict__ P = mats + 4 * EQ_LEVELS * k;   // the section's own powers: P + 4 j is its T^(16 * 2^j)
        const double b0 = c[0], b1 = c[1], b2 = c[2], a1 = c[3], a2 = c[4];
        double st1 = 0.0, st2 = 0.0;                            // the section's state in front of the tile, as (u[i-1], u[i-1] - u[i-2])
        if (WRITE) st1 = starts[2 * K * (int64_t)blockIdx.x + 2 * k], st2 = starts[2 * K * (int64_t)blockIdx.x + 2 * k + 1];
        double v1 = 0.0, v2 = 0.0;
        eq_run<false>(u, h1, h2, v1, v2, b0, b1, b2, a1, a2);
        v2 = v1 - v2;                                           // carried as (u[i-1], u[i-1] - u[i-2]): the powers are well scaled there
        if (WRITE && tid == 0) {
            const double r1 = P[0] * st1 + P[1] * st2, r2 = P[2] * st1 + P[3] * st2;
            v1 = r1 + v1, v2 = r2 + v2;
        }
        // inclusive scan over the runs: v_j <- P_l v_(j - 2^l) + v_j for l = 0 .. 7 (ld_scan of loudness.hip at order 2)
        s_sc[cur][tid] = v1, s_sc[cur][EQ_THREADS + tid] = v2;
        __syncthreads();
        for (int l = 0; l < EQ_LEVELS; ++l) {
            const int off = 1 << l;
            if (tid >= off) {
                const double o1 = s_sc[cur][tid - off], o2 = s_sc[cur][EQ_THREADS + tid - off];
                const double r1 = P[4 * l] * o1 + P[4 * l + 1] * o2, r2 = P[4 * l + 2] * o1 + P[4 * l + 3] * o2;
                v1 = r1 + v1, v2 = r2 + v2;
            }
            cur ^= 1;
            s_sc[cur][tid] = v1, s_sc[cur][EQ_THREADS + tid] = v2;
            __syncthreads();                                    // (the next level reads this buffer and writes the other one)
        }
        if (tid > 0) st1 = s_sc[cur][tid - 1], st2 = s_sc[cur][EQ_THREADS + tid - 1];
        if (!WRITE && tid == EQ_THREADS - 1) ends[2 * K * (int64_t)blockIdx.x + 2 * k] = v1, ends[2 * K * (int64_t)blockIdx.x + 2 * k + 1] = v2;
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
    for (int e = 0; e < EQ_SPT; ++e) s_x[eq_idx(q0 + e)] = (float)u[e];
    __syncthreads();
    float *__restrict__ ys = out + base;
    for (int q = 16 + tid; q < EQ_T + 16; q += EQ_THREADS) {
        const int64_t p = t0 - 16 + q;
        if (p < len) ys[p] = s_x[eq_idx(q)];
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
// workgroup per signal, 4096 tiles a round, as k_loud_carry does it: a thread walks EQ_RUN consecutive tiles from zero, the
// workgroup scans the threads' end states with T^(4096 * 16 * 2^l) (the state in front of the round goes through thread 0's
// run), and every thread walks its tiles again from its true state.  The tiles' end states are read again from memory on the
// second walk: 16 of them at order 16 do not fit the registers.  The walk is the accurate part (a true state times T^4096
// cancels nothing); the scan above it only matters where T^65536 is not yet nothing.
template <int K>
__global__ __launch_bounds__(EQ_THREADS)
void k_eq_carry(const int64_t *__restrict__ in_off, int n, int64_t n_tiles, const double *__restrict__ mats, const double *__restrict__ ends,
                const int32_t *__restrict__ first_tile, double *__restrict__ starts)
{
    constexpr int D = 2 * K;
    __shared__ double s_sc[D * EQ_THREADS];
    const int sig = blockIdx.x, tid = threadIdx.x;
    const int64_t len = in_off[sig + 1] - in_off[sig];
    if (len <= 0 || len >= ((int64_t)1 << 31)) return;
    const int nt = (int)((len + EQ_T - 1) / EQ_T);
    const int64_t first = first_tile[sig];
    if (first < 0 || first + nt > n_tiles) return;              // (a tile table that is not the planner's)
    const double *__restrict__ P0 = mats + 4 * EQ_LEVELS * K;   // T^4096: one tile
    const double *__restrict__ PR = P0 + D * D;                 // T^(4096 * 16): a thread's run; level l of the scan: PR + D D l
    double carry[D];
#pragma unroll
    for (int i = 0; i < D; ++i) carry[i] = 0.0;
    for (int c = 0; c < nt; c += EQ_THREADS * EQ_RUN) {
        const int t0 = c + tid * EQ_RUN;
        double v[D], o[D], r[D];
#pragma unroll
        for (int i = 0; i < D; ++i) v[i] = 0.0;
#pragma unroll 1
        for (int e = 0; e < EQ_RUN; ++e) {
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
        for (int i = 0; i < D; ++i) s_sc[i * EQ_THREADS + tid] = v[i];
        __syncthreads();
        for (int l = 0; l < EQ_LEVELS; ++l) {
            const int off = 1 << l;
            if (tid >= off) {
#pragma unroll
                for (int i = 0; i < D; ++i) o[i] = s_sc[i * EQ_THREADS + tid - off];
            }
            __syncthreads();                                    // (everyone has read the level below)
            if (tid >= off) {
                eq_matvec<D>(PR + D * D * l, o, r);
#pragma unroll
                for (int i = 0; i < D; ++i) v[i] = r[i] + v[i];
#pragma unroll
                for (int i = 0; i < D; ++i) s_sc[i * EQ_THREADS + tid] = v[i];
            }
            __syncthreads();
        }
        double st[D];
#pragma unroll
        for (int i = 0; i < D; ++i) st[i] = tid == 0 ? carry[i] : s_sc[i * EQ_THREADS + tid - 1];
#pragma unroll
        for (int i = 0; i < D; ++i) carry[i] = s_sc[i * EQ_THREADS + EQ_THREADS - 1];
#pragma unroll 1
        for (int e = 0; e < EQ_RUN; ++e) {
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
    hipLaunchKernelGGL(k_eq_carry<K>, dim3((unsigned)n), dim3(EQ_THREADS), 0, st, in_off, n, n_tiles, mats, ends, first_tile, starts);
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
    HIP_TRY(ctx, hipMemsetAsync(first_tile, 0xff, sizeof(int32_t) * (size_t)n, st));     // -1: no tile seen
    hipLaunchKernelGGL(k_eq_tile<false>, dim3((unsigned)n_tiles), dim3(EQ_THREADS), 0, st, x, in_off, n, K, coef, mats, tiles,
                       (const double *)nullptr, ends, first_tile, (float *)nullptr);
    LAUNCH_CHECK(ctx);
    if (int rc = launch_eq_carry<GOOFER_EQ_MAX_BANDS>(ctx, K, in_off, n, n_tiles, mats, ends, first_tile, starts, st)) return rc;
    hipLaunchKernelGGL(k_eq_tile<true>, dim3((unsigned)n_tiles), dim3(EQ_THREADS), 0, st, x, in_off, n, K, coef, mats, tiles,
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
    if (K < 0 || K > GOOFER_EQ_MAX_BANDS || !signal_tiles_ok(EQ_T, n, total, n_tiles))
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
