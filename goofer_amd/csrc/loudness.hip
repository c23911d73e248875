// Loudness metering and normalisation on the device (gfx950): the integrated loudness of every signal of a ragged batch after
// ITU-R BS.1770-4 for one channel, and the signals scaled to a target.  The definition (K-weighting, segments, blocks, gates,
// gain) is in include/goofer_hip.h; the host half, goofer_host_loudness_plan (planner.hip), makes the coefficients, the segment
// CSR, the tile table and the matrix powers.
//
// The K-weighting filter is a recurrence of order 4 in fp64, state s = (u1, u2, v1, v2).  It is linear: a run of m samples from
// state s ends in A^m s + e, e the end state of the same run from zero.  So a long signal is cut into tiles of 4096 samples, a
// tile into 256 runs of 16, and the states are carried by scans whose operator is "multiply by a constant matrix, add": all
// elements of a scan level share one matrix, A^(16 * 2^k), made on the host.  The tiles, the scan and the carry from tile to
// tile are those of tile_scan.h; this file holds the filter, its element and the statistics.  Four launches in stream order; no
// workgroup waits for another one, and every sum has a fixed order:
//   A  k_loud_ends    a workgroup per tile: runs from zero, a workgroup scan, the tile's zero-state end state to scratch
//   B  k_loud_carry   a workgroup per signal: the tiles' end states into the tiles' true start states, 4096 tiles per scan
//   C  k_loud_energy  a workgroup per tile: the scan again with the start state put into run 0, every run again from its true
//                     state, v^2 summed per segment; one partial sum per (tile, segment it touches) into a slot of its own
//   D  k_loud_stats   a workgroup per signal: the slots into E[k] in ascending tile order, blocks, gates, L, momentary max, g
// and k_loud_apply, a per-sample kernel over the ragged batch.
#include "tile_scan.h"

#define LD_SLOTS GOOFER_LOUDNESS_SLOTS
static_assert(GOOFER_LOUDNESS_TILE == TS_T && GOOFER_LOUDNESS_SPT == TS_SPT && GOOFER_LOUDNESS_LEVELS == TS_LEVELS && GOOFER_LOUDNESS_RUN_TILES == TS_RUN,
              "the tiling of tile_scan.h");
static_assert(GOOFER_LOUDNESS_MATS == TS_LEVELS + 4 + TS_LEVELS && TS_RUN == 16, "A^16 .. A^2048 inside a tile, A^4096 a tile, A^(4096 * 16 * 2^k) over the runs of 16 tiles");
static_assert(TS_T / (GOOFER_LOUDNESS_MIN_SR / 10) + 2 <= LD_SLOTS, "segments a tile can touch");
#define LD_XPAD TS_XPAD(16)                           // the tile and the 16 samples in front of it

__device__ __forceinline__ void ld_matvec(const double *__restrict__ M, const double (&s)[4], double (&r)[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = ((M[4 * i] * s[0] + M[4 * i + 1] * s[1]) + M[4 * i + 2] * s[2]) + M[4 * i + 3] * s[3];
}

// the thread's 16 samples through both biquads from state s (left in s); ENERGY: v^2 of the first `bnd` samples summed into
// e0, of the others into e1, in sample order
template <bool ENERGY>
__device__ __forceinline__ void ld_run(const float *__restrict__ s_x, const double *__restrict__ c, double (&s)[4], int bnd, double &e0, double &e1)
{
    const int q0 = 16 + threadIdx.x * TS_SPT;
    double x1 = (double)s_x[ts_idx(q0 - 1)], x2 = (double)s_x[ts_idx(q0 - 2)];
    double u1 = s[0], u2 = s[1], v1 = s[2], v2 = s[3];
#pragma unroll
    for (int e = 0; e < TS_SPT; ++e) {
        const double x = (double)s_x[ts_idx(q0 + e)];
        const double u = (((c[0] * x + c[1] * x1) + c[2] * x2) - c[3] * u1) - c[4] * u2;
        const double v = (((c[5] * u + c[6] * u1) + c[7] * u2) - c[8] * v1) - c[9] * v2;
        x2 = x1, x1 = x, u2 = u1, u1 = u, v2 = v1, v1 = v;
        if (ENERGY) {
            if (e < bnd) e0 += v * v; else e1 += v * v;
        }
    }
    s[0] = u1, s[1] = u2, s[2] = v1, s[3] = v2;
}

// r = M s + v
__device__ __forceinline__ void ld_affine(const double *__restrict__ M, const double (&s)[4], const double (&v)[4], double (&r)[4])
{
    double t[4];
    ld_matvec(M, s, t);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = t[i] + v[i];
}

// the scan's combination at level k, all elements sharing mats[k]: v <- mats[k] o + v (ts_scan)
struct ld_level {
    const double *__restrict__ mats;
    __device__ __forceinline__ void operator()(const double (&o)[4], int k, double (&v)[4]) const { ld_affine(mats + 16 * k, o, v, v); }
};

__global__ __launch_bounds__(TS_THREADS)
void k_loud_ends(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, const double *__restrict__ coef,
                 const double *__restrict__ mats, const int32_t *__restrict__ tiles, double *__restrict__ ends, int32_t *__restrict__ first_tile)
{
    __shared__ float s_x[LD_XPAD];
    __shared__ double s_sc[2][4 * TS_THREADS];
    int sig, kt;
    int64_t base, len, t0;
    if (!ts_tile(tiles, in_off, n, sig, kt, base, len, t0)) return;
    ts_first_tile(first_tile, sig, kt);
    ts_stage<16>(x + base, len, t0, s_x);
    __syncthreads();
    double v[4] = {0.0, 0.0, 0.0, 0.0}, e0 = 0.0, e1 = 0.0;
    ld_run<false>(s_x, coef, v, 0, e0, e1);
    ts_scan(v, ld_level{mats}, s_sc);
    if (threadIdx.x == TS_THREADS - 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ends[4 * (int64_t)blockIdx.x + i] = v[i];
    }
}

// starts[tile] = the true state in front of the tile: 0 for a signal's first, A^4096 starts[t] + ends[t] for tile t + 1
// (ts_carry).  A thread walks its tiles from zero; the state in front of the round goes into thread 0's element through
// A^(4096 * 16), and the scan's level k is A^(4096 * 16 * 2^k).
struct ld_carry {
    const double *__restrict__ P0, *__restrict__ PR;          // A^4096: one tile; A^(4096 * 16): a thread's run, level k of the scan: PR + 16 k
    __device__ __forceinline__ void seed(double (&)[4], const double (&)[4]) const {}
    __device__ __forceinline__ void append(double (&v)[4], const double (&z)[4]) const { ld_affine(P0, v, z, v); }
    __device__ __forceinline__ void join(double (&v)[4], const double (&carry)[4]) const { ld_affine(PR, carry, v, v); }
    __device__ __forceinline__ void level(const double (&o)[4], int k, double (&v)[4]) const { ld_affine(PR + 16 * k, o, v, v); }
    __device__ __forceinline__ void step(double (&st)[4], const double (&z)[4]) const { ld_affine(P0, st, z, st); }
};

__global__ __launch_bounds__(TS_THREADS)
void k_loud_carry(const int64_t *__restrict__ in_off, int n, int64_t n_tiles, const double *__restrict__ mats,
                  const double *__restrict__ ends, const int32_t *__restrict__ first_tile, double *__restrict__ starts)
{
    ts_carry<4, 4>(in_off, n_tiles, first_tile, ends, starts, ld_carry{mats + 16 * TS_LEVELS, mats + 16 * (TS_LEVELS + 4)});
}

__global__ __launch_bounds__(TS_THREADS)
void k_loud_energy(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, int S, const double *__restrict__ coef,
                   const double *__restrict__ mats, const int32_t *__restrict__ tiles, const double *__restrict__ starts,
                   double *__restrict__ partial)
{
    __shared__ float s_x[LD_XPAD];
    __shared__ double s_sc[2][4 * TS_THREADS];
    __shared__ double s_red[LD_SLOTS][TS_THREADS / 64];
    int sig, kt;
    int64_t base, len, t0;
    if (!ts_tile(tiles, in_off, n, sig, kt, base, len, t0)) return;
    const int tid = threadIdx.x;
    ts_stage<16>(x + base, len, t0, s_x);
    __syncthreads();
    double st[4], v[4] = {0.0, 0.0, 0.0, 0.0}, e0 = 0.0, e1 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) st[i] = starts[4 * (int64_t)blockIdx.x + i];
    ld_run<false>(s_x, coef, v, 0, e0, e1);
    if (tid == 0) ld_affine(mats, st, v, v);
    const int cur = ts_scan(v, ld_level{mats}, s_sc);
    if (tid > 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) st[i] = s_sc[cur][i * TS_THREADS + tid - 1];
    }
    // segments: sample i of the signal lies in segment i / S; the tile touches kf .. and owns slot k - kf for segment k < Kn
    const uint32_t us = (uint32_t)S, i0 = (uint32_t)t0 + (uint32_t)(tid * TS_SPT);
    const int kf = (int)((uint32_t)t0 / us), kn = (int)((uint32_t)len / us);
    const int k0 = (int)(i0 / us);
    const int bnd = (int)min((uint32_t)TS_SPT, (uint32_t)(k0 + 1) * us - i0);
    ld_run<true>(s_x, coef, st, bnd, e0, e1);
    int nq = min((int)(((uint32_t)t0 + TS_T - 1) / us), kn - 1) - kf + 1;
    nq = nq > LD_SLOTS ? LD_SLOTS : nq;
    const int q0 = k0 - kf;
    auto add = [](double a, double b) { return a + b; };
    for (int q = 0; q < nq; ++q) {
        const double r = ts_wave_reduce((q0 == q ? e0 : 0.0) + (q0 + 1 == q ? e1 : 0.0), add);
        if ((tid & 63) == 0) s_red[q][tid >> 6] = r;
    }
    __syncthreads();
    if (tid < nq) partial[LD_SLOTS * (int64_t)blockIdx.x + tid] = ts_waves(add, s_red[tid]);
}

// Blocks, both gates, L, momentary_max and g of one signal's (or one channel group's) kn segment energies E(k), by the whole
// workgroup (k_loud_stats, k_loud_link); E(k) is read by every thread that needs it and gives the same value each time.  The
// results are thread 0's (true there, false elsewhere).
template <class Energy>
__device__ __forceinline__ bool loud_gate(Energy E, int64_t kn, int S, double abs_gate, double target, double max_gain, int normalise,
                                          double *__restrict__ s_red, double &L, double &mm, float &g)
{
    const int tid = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL), ninf = __longlong_as_double(0xfff0000000000000LL);
    const int64_t kb = kn > 3 ? kn - 3 : 0;
    const double inv = 1.0 / (4.0 * (double)S);
    auto add = [](double a, double b) { return a + b; };
    auto block = [&](int64_t j) { return (((E(j) + E(j + 1)) + E(j + 2)) + E(j + 3)) * inv; };
    double sum = 0.0, cnt = 0.0, top = 0.0;
    for (int64_t j = tid; j < kb; j += TS_THREADS) {
        const double z = block(j);
        if (!(z <= abs_gate)) sum += z, cnt += 1.0;             // (a NaN block is not dropped: it makes the statistics NaN)
        top = fmax(top, z);
    }
    sum = ts_block_reduce(sum, add, s_red);
    cnt = ts_block_reduce(cnt, add, s_red);
    top = ts_block_reduce(top, [](double a, double b) { return fmax(a, b); }, s_red);
    const double rel = 0.1 * (sum / cnt);                       // (cnt == 0: nothing passes below either)
    double sum2 = 0.0, cnt2 = 0.0;
    for (int64_t j = tid; j < kb; j += TS_THREADS) {
        const double z = block(j);
        if (z > abs_gate && z > rel) sum2 += z, cnt2 += 1.0;
    }
    sum2 = ts_block_reduce(sum2, add, s_red);
    cnt2 = ts_block_reduce(cnt2, add, s_red);
    if (tid != 0) return false;
    L = ninf, mm = kb > 0 ? -0.691 + 10.0 * log10(top) : ninf;
    g = 1.0f;
    if (sum != sum) {
        L = mm = nan;
        g = normalise ? __int_as_float(0x7fc00000) : 1.0f;
    } else if (cnt2 > 0.0) {
        L = -0.691 + 10.0 * log10(sum2 / cnt2);
        if (normalise) g = (float)fmin(pow(10.0, (target - L) / 20.0), max_gain);
    }
    return true;
}

__global__ __launch_bounds__(TS_THREADS)
void k_loud_stats(const int64_t *__restrict__ in_off, int n, int64_t n_tiles, int S, const int64_t *__restrict__ seg_off, const double *__restrict__ partial,
                  const int32_t *__restrict__ first_tile, double abs_gate, double target, double max_gain, int normalise,
                  double *__restrict__ seg_energy, double *__restrict__ loud, float *__restrict__ gain)
{
    __shared__ double s_red[TS_THREADS / 64];
    const int sig = blockIdx.x, tid = threadIdx.x;
    const int64_t len = in_off[sig + 1] - in_off[sig], sbase = seg_off[sig];
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    int nt = 0;
    int64_t first = 0;
    const bool tiled = ts_signal(in_off, n_tiles, first_tile, nt, first);
    const int64_t kn = tiled ? (uint32_t)len / (uint32_t)S : 0;   // (0 < len < 2^31 there)
    if (seg_off[sig + 1] - sbase != kn || (len > 0 && !tiled)) {   // (tables that are not the planner's: no segment is written)
        if (tid == 0) { loud[2 * sig] = nan; loud[2 * sig + 1] = nan; gain[sig] = 1.0f; }
        return;
    }
    double *__restrict__ E = seg_energy + sbase;
    if (kn > 0) {
        const uint32_t us = (uint32_t)S;                        // (k + 1) S <= len < 2^31: the quotients are 32-bit
        for (uint32_t k = tid; k < (uint32_t)kn; k += TS_THREADS) {
            const uint32_t ta = k * us / TS_T, tb = ((k + 1) * us - 1) / TS_T;
            double sum = 0.0;
            for (uint32_t t = ta; t <= tb; ++t) {
                const uint32_t slot = k - t * TS_T / us;        // (the tile's first segment is at most k)
                if (slot < LD_SLOTS) sum += partial[LD_SLOTS * (first + t) + slot];
            }
            E[k] = sum;
        }
    }
    __syncthreads();                                            // E is read back by other threads of this workgroup
    double L, mm;
    float g;
    if (!loud_gate([&](int64_t k) { return E[k]; }, kn, S, abs_gate, target, max_gain, normalise, s_red, L, mm, g)) return;
    loud[2 * sig] = L;
    loud[2 * sig + 1] = mm;
    gain[sig] = g;
}

// The channel-linked gate (goofer_loudness_link): a workgroup per group of CH channels, on the segment energies a measure-only
// goofer_loudness_measure wrote; E_g[k] = E_0[k] + E_1[k], made again at every read (the same bits each time).
__global__ __launch_bounds__(TS_THREADS)
void k_loud_link(const double *__restrict__ seg_energy, const int64_t *__restrict__ seg_off, int ch, int S, double abs_gate, double target,
                 double max_gain, int normalise, double *__restrict__ loud, float *__restrict__ gain)
{
    __shared__ double s_red[TS_THREADS / 64];
    const int grp = blockIdx.x, tid = threadIdx.x, s0 = grp * ch;
    const int64_t b0 = seg_off[s0], kn = seg_off[s0 + 1] - b0;
    const int64_t b1 = ch > 1 ? seg_off[s0 + 1] : b0;
    if (kn < 0 || (ch > 1 && seg_off[s0 + 2] - b1 != kn)) {      // (channels that differ in segment count: k_loud_stats' convention)
        if (tid == 0) {
            loud[2 * grp] = loud[2 * grp + 1] = __longlong_as_double(0x7ff8000000000000LL);
            for (int c = 0; c < ch; ++c) gain[s0 + c] = 1.0f;
        }
        return;
    }
    const double *__restrict__ E0 = seg_energy + b0, *__restrict__ E1 = seg_energy + b1;
    double L, mm;
    float g;
    const bool first = ch > 1 ? loud_gate([&](int64_t k) { return E0[k] + E1[k]; }, kn, S, abs_gate, target, max_gain, normalise, s_red, L, mm, g)
                              : loud_gate([&](int64_t k) { return E0[k]; }, kn, S, abs_gate, target, max_gain, normalise, s_red, L, mm, g);
    if (!first) return;
    loud[2 * grp] = L;
    loud[2 * grp + 1] = mm;
    for (int c = 0; c < ch; ++c) gain[s0 + c] = g;
}

#define LD_APPLY_SPT 4
__global__ __launch_bounds__(256)
void k_loud_apply(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, int64_t total, const float *__restrict__ gain,
                  float *__restrict__ out, int vec)
{
    const sample_tile<LD_APPLY_SPT> t(in_off, n, total);
    if (!t.live) return;
    const int64_t g = t.g;
    if (vec && t.uniform() && g + LD_APPLY_SPT <= total) {
        const float gn = gain[t.lo];                            // (the tile's signal sits in an SGPR: a scalar load)
        float4 v = *reinterpret_cast<const float4 *>(x + g);
        v.x *= gn; v.y *= gn; v.z *= gn; v.w *= gn;
        *reinterpret_cast<float4 *>(out + g) = v;
        return;
    }
    for (int k = 0; k < LD_APPLY_SPT; ++k) {
        const int64_t gi = g + k;
        if (gi >= total) break;
        out[gi] = x[gi] * gain[t.note(in_off, gi)];
    }
}

int launch_loudness_measure(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int S, const double *coef, const double *mats,
                            const int64_t *seg_off, const int32_t *tiles, int64_t n_tiles, double target, double max_gain_db,
                            double *seg_energy, double *loud, float *gain, double *ends, double *starts, double *partial,
                            int32_t *first_tile, hipStream_t st)
{
    if (n <= 0) return GOOFER_OK;
    if (int rc = ts_first_tile_reset(ctx, first_tile, n, st)) return rc;
    if (n_tiles > 0) {
        hipLaunchKernelGGL(k_loud_ends, dim3((unsigned)n_tiles), dim3(TS_THREADS), 0, st, x, in_off, n, coef, mats, tiles, ends, first_tile);
        LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_loud_carry, dim3((unsigned)n), dim3(TS_THREADS), 0, st, in_off, n, n_tiles, mats, (const double *)ends,
                           (const int32_t *)first_tile, starts);
        LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_loud_energy, dim3((unsigned)n_tiles), dim3(TS_THREADS), 0, st, x, in_off, n, S, coef, mats, tiles,
                           (const double *)starts, partial);
        LAUNCH_CHECK(ctx);
    }
    const bool normalise = !std::isnan(target);
    hipLaunchKernelGGL(k_loud_stats, dim3((unsigned)n), dim3(TS_THREADS), 0, st, in_off, n, n_tiles, S, seg_off, (const double *)partial,
                       (const int32_t *)first_tile, std::pow(10.0, (-70.0 + 0.691) / 10.0), normalise ? target : 0.0,
                       std::pow(10.0, max_gain_db / 20.0), normalise ? 1 : 0, seg_energy, loud, gain);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

int launch_loudness_apply(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, const float *gain, float *out,
                          hipStream_t st)
{
    const int vec = (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    return launch_per_sample(ctx, k_loud_apply, total, 256 * LD_APPLY_SPT, 0, st, x, in_off, n, total, gain, out, vec);
}

extern "C" int goofer_loudness_measure(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int S, const double *coef,
                                       const double *mats, const int64_t *seg_off, const int32_t *tiles, int64_t n_tiles, double target,
                                       double max_gain_db, double *seg_energy, double *loud, float *gain, void *scratch,
                                       int64_t *scratch_bytes, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (int rc = check_counts(ctx, "goofer_loudness_measure", n, total, n_tiles)) return rc;
    const int s_lo = (GOOFER_LOUDNESS_MIN_SR + 5) / 10, s_hi = (GOOFER_LOUDNESS_MAX_SR + 5) / 10;
    if (S < s_lo || S > s_hi || std::isinf(target) || !(max_gain_db >= 0.0 && max_gain_db <= GOOFER_LOUDNESS_MAX_GAIN_DB_CAP) ||
        !signal_tiles_ok(TS_T, n, total, n_tiles))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_loudness_measure: S = %d, target %g, max_gain_db %g, %lld tiles for %lld samples in %d signals is not a geometry of goofer_host_loudness_plan",
                           S, target, max_gain_db, (long long)n_tiles, (long long)total, n);
    if (!scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_loudness_measure: null pointer (scratch_bytes)");
    double *ends, *starts, *partial;
    int32_t *first_tile;
    auto carve = [&](arena &a) {
        ends = a.take<double>(4 * (size_t)n_tiles);
        starts = a.take<double>(4 * (size_t)n_tiles);
        partial = a.take<double>(LD_SLOTS * (size_t)n_tiles);
        first_tile = a.take<int32_t>((size_t)n);
    };
    if (scratch) {
        if (n > 0 && (!in_off || !coef || !mats || !seg_off || !seg_energy || !loud || !gain || (total > 0 && (!x || !tiles))))
            return goofer_fail(ctx, GOOFER_EINVAL, "goofer_loudness_measure: null pointer");
        if (int rc = check_aligned(ctx, "goofer_loudness_measure", "x, tiles and gain", {x, tiles, gain}, "in_off, coef, mats, seg_off, seg_energy, loud and scratch",
                                   {in_off, coef, mats, seg_off, seg_energy, loud, scratch}))
            return rc;
    }
    int rc = caller_scratch(ctx, scratch, scratch_bytes, "goofer_loudness_measure", carve);
    if (rc || !scratch) return rc;
    return launch_loudness_measure(ctx, x, in_off, n, S, coef, mats, seg_off, tiles, n_tiles, target, max_gain_db, seg_energy, loud, gain,
                                   ends, starts, partial, first_tile, (hipStream_t)stream);
}

extern "C" int goofer_loudness_link(goofer_ctx *ctx, const double *seg_energy, const int64_t *seg_off, int n, int ch, int S, double target,
                                    double max_gain_db, double *loud, float *gain, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (n < 0 || (ch != 1 && ch != 2) || n % ch != 0)
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_loudness_link: %d signals in groups of %d channels (1 or 2)", n, ch);
    const int s_lo = (GOOFER_LOUDNESS_MIN_SR + 5) / 10, s_hi = (GOOFER_LOUDNESS_MAX_SR + 5) / 10;
    if (S < s_lo || S > s_hi || std::isinf(target) || !(max_gain_db >= 0.0 && max_gain_db <= GOOFER_LOUDNESS_MAX_GAIN_DB_CAP))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_loudness_link: S = %d, target %g, max_gain_db %g is outside the definition's range", S, target,
                           max_gain_db);
    if (n == 0) return GOOFER_OK;
    if (!seg_energy || !seg_off || !loud || !gain) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_loudness_link: null pointer");
    if (int rc = check_aligned(ctx, "goofer_loudness_link", "gain", {gain}, "seg_energy, seg_off and loud", {seg_energy, seg_off, loud})) return rc;
    const bool normalise = !std::isnan(target);
    hipLaunchKernelGGL(k_loud_link, dim3((unsigned)(n / ch)), dim3(TS_THREADS), 0, (hipStream_t)stream, seg_energy, seg_off, ch, S,
                       std::pow(10.0, (-70.0 + 0.691) / 10.0), normalise ? target : 0.0, std::pow(10.0, max_gain_db / 20.0), normalise ? 1 : 0, loud,
                       gain);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

extern "C" int goofer_loudness_apply(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, const float *gain,
                                     float *out, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (n < 0 || total < 0) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_loudness_apply: negative count (%d signals, %lld samples)", n, (long long)total);
    if (n == 0 || total == 0) return GOOFER_OK;
    if (!x || !in_off || !gain || !out) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_loudness_apply: null pointer");
    if (int rc = check_aligned(ctx, "goofer_loudness_apply", "x, gain and out", {x, gain, out}, "in_off", {in_off})) return rc;
    if (int rc = check_overlap(ctx, "goofer_loudness_apply", x, out, total, true)) return rc;
    return launch_loudness_apply(ctx, x, in_off, n, total, gain, out, (hipStream_t)stream);
}
