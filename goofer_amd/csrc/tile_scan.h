// A recurrence carried over every signal of a ragged batch (gfx950): what loudness.hip, compress.hip and eq.hip share.
//
// A signal is cut into tiles of TS_T = 4096 samples and a tile into 256 runs of 16, one per thread of a workgroup.  A stage
// whose samples compose to elements of D doubles with an associative combination carries them in three steps:
//   - a workgroup per tile stages the tile into LDS at a lane stride of 17 (ts_stage), every thread runs its 16 samples, and
//     the 256 run elements go through an inclusive scan of 8 levels (ts_scan); all elements of a level share one constant
//     made on the host (a matrix or coefficient power), so a level is "older element, level, this element" and the stage says
//     how they combine.  The last thread's element is the tile's;
//   - a workgroup per signal turns the tiles' elements into the true state in front of every tile (ts_carry);
//   - a workgroup per tile runs again with the tile's start state put into run 0.
// No workgroup waits for another one and every combination has a fixed order.  The tile table (pairs of signal and tile of that
// signal, ascending) and the constants are the host planners'; ts_tile and ts_signal refuse what is not a planner's table.
#pragma once

#include "launchers.h"

#define TS_THREADS 256
#define TS_SPT GOOFER_SCAN_SPT
#define TS_T GOOFER_SCAN_TILE
#define TS_LEVELS GOOFER_SCAN_LEVELS
#define TS_RUN GOOFER_SCAN_RUN_TILES                  // tiles a thread of ts_carry walks
static_assert(TS_T == TS_THREADS * TS_SPT && TS_SPT == 16 && (1 << TS_LEVELS) == TS_THREADS, "one workgroup of 256 runs of 16 per tile");
#define TS_XPAD(HIST) (TS_T + (HIST) + (TS_T + (HIST)) / 16)   // floats of a staged tile with HIST samples in front, one pad word per 16

// entry q of the staged samples (q = HIST + position in the tile): a thread's 16 consecutive words at a lane stride of 17
__device__ __forceinline__ int ts_idx(int q) { return q + (q >> 4); }

// the tile's samples [t0, t0 + T) into LDS (coalesced), 0 outside the signal; HIST 16: entry 16 is the tile's first sample and
// the two samples in front of it are staged too (entries 14 and 15); HIST 0: the tile alone
template <int HIST>
__device__ __forceinline__ void ts_stage(const float *__restrict__ xs, int64_t len, int64_t t0, float *__restrict__ s_x)
{
    static_assert(HIST == 0 || HIST == 16, "whole runs in front of the tile");
    for (int q = (HIST ? HIST - 2 : 0) + threadIdx.x; q < TS_T + HIST; q += TS_THREADS) {
        const int64_t p = t0 - HIST + q;
        s_x[ts_idx(q)] = (HIST == 0 || p >= 0) && p < len ? xs[p] : 0.0f;
    }
}

// a tile's signal and place from the planner's table; false for a pair that is not the planner's (nothing is read or written)
__device__ __forceinline__ bool ts_tile(const int32_t *__restrict__ tiles, const int64_t *__restrict__ in_off, int n, int &sig, int &kt,
                                        int64_t &base, int64_t &len, int64_t &t0)
{
    sig = __builtin_amdgcn_readfirstlane(tiles[2 * blockIdx.x]), kt = __builtin_amdgcn_readfirstlane(tiles[2 * blockIdx.x + 1]);
    if (sig < 0 || sig >= n || kt < 0) return false;
    base = in_off[sig], len = in_off[sig + 1] - base, t0 = (int64_t)kt * TS_T;
    return base >= 0 && t0 < len && len < ((int64_t)1 << 31);
}

// first_tile[signal] = the signal's first entry in the tile table: -1 from the host in front of the first launch, then written
// by thread 0 of that tile's workgroup in the stage's first tile kernel
static inline int ts_first_tile_reset(goofer_ctx *ctx, int32_t *first_tile, int n, hipStream_t st)
{
    HIP_TRY(ctx, hipMemsetAsync(first_tile, 0xff, sizeof(int32_t) * (size_t)n, st));     // -1: no tile seen
    return GOOFER_OK;
}
__device__ __forceinline__ void ts_first_tile(int32_t *__restrict__ first_tile, int sig, int kt)
{
    if (threadIdx.x == 0 && kt == 0) first_tile[sig] = (int32_t)blockIdx.x;
}

// the tiles of signal blockIdx.x in the tile table, nt of them from entry `first` on: false for an empty signal and where the
// table is not the planner's
__device__ __forceinline__ bool ts_signal(const int64_t *__restrict__ in_off, int64_t n_tiles, const int32_t *__restrict__ first_tile, int &nt,
                                          int64_t &first)
{
    const int sig = blockIdx.x;
    const int64_t len = in_off[sig + 1] - in_off[sig];
    if (len <= 0 || len >= ((int64_t)1 << 31)) return false;
    nt = (int)((len + TS_T - 1) / TS_T);
    first = first_tile[sig];
    return first >= 0 && first + nt <= n_tiles;
}

// Inclusive scan over the workgroup's 256 elements v of D doubles: for k = 0 .. 7, thread j >= 2^k does op(o, k, v), o the
// element of thread j - 2^k as it stood after level k - 1, which leaves "o, then v" in v.  The elements lie component-major
// in the two buffers of s_sc, component i of thread j at [i * 256 + j]; a level reads one and writes the other.  Starts in
// buffer `cur` and returns the buffer that holds the result.  (A caller that scans again and has read the result may start
// in the other buffer, the one nobody reads, without a barrier in between.)
template <int D, int W, typename Op>
__device__ __forceinline__ int ts_scan(double (&v)[D], Op op, double (*s_sc)[W], int cur = 0)
{
    static_assert(W >= D * TS_THREADS, "room for 256 elements a buffer");
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < D; ++i) s_sc[cur][i * TS_THREADS + tid] = v[i];
    __syncthreads();
    for (int k = 0; k < TS_LEVELS; ++k) {
        const int off = 1 << k;
        if (tid >= off) {
            double o[D];
#pragma unroll
            for (int i = 0; i < D; ++i) o[i] = s_sc[cur][i * TS_THREADS + tid - off];
            op(o, k, v);
        }
        cur ^= 1;
#pragma unroll
        for (int i = 0; i < D; ++i) s_sc[cur][i * TS_THREADS + tid] = v[i];
        __syncthreads();                                        // (the next level reads this buffer and writes the other one)
    }
    return cur;
}

// A value per thread combined in a fixed order: the butterfly inside the wave (every lane gets the wave's value), and the four
// waves' values, written to s_red[wave] by a lane of each, in order
template <typename Op>
__device__ __forceinline__ double ts_wave_reduce(double v, Op op)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
template <typename Op>
__device__ __forceinline__ double ts_waves(Op op, const double *s_red) { return op(op(op(s_red[0], s_red[1]), s_red[2]), s_red[3]); }

// both over the workgroup; every thread gets the result
template <typename Op>
__device__ __forceinline__ double ts_block_reduce(double v, Op op, double *s_red)
{
    v = ts_wave_reduce(v, op);
    __syncthreads();                                            // (the previous result has been read)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ts_waves(op, s_red);
}

// The tile-to-tile carry.  sums[tile] is the tile's element (D doubles: its samples composed from the neutral element, all
// zeros), starts[tile] becomes the true state in front of the tile (the element's first DS doubles): zeros for a signal's
// first, one step over tile t from starts[t] for tile t + 1.  One workgroup per signal, 4096 tiles a round: a thread composes
// its TS_RUN consecutive tiles, the workgroup scans the threads' elements (thread 0's holds the state in front of the round,
// the carry), and every thread walks its tiles again from its true state.  The stage S says
//   S.append(v, z)     element v takes the tile element z behind it
//   S.level(o, k, v)   the scan's combination over runs of TS_RUN << k tiles (ts_scan)
//   S.step(st, z)      the true state st steps over the tile whose element is z
//   S.seed(v, carry)   thread 0, in front of its tiles: the stages whose walk starts from the carry put it into v here ...
//   S.join(v, carry)   thread 0, behind its tiles: ... and those that walk from zeros add the carry's image here
// (two places, not a flag: which one a stage fills decides the order of its roundings).
// The 16 tile elements of a thread stay in registers between the two walks, tiles behind the signal's last as neutral
// elements: up to 4 doubles each, 128 VGPRs.  Larger elements are not served: they have to be read again from memory and
// scanned in one buffer, and k_eq_carry of eq.hip does that written out.  A second form of this walk for them was built and
// measured slower at K = 4 (docs/EXPERIMENTS.md), so a further stage with such elements copies k_eq_carry's walk: accepted.
// (A single wave scanning 64 tiles a round took 250 us for the 11 882 tiles of a 48.7 M-sample track in the loudness stage,
// 1.3 us a round: a serial chain of seven matrix-vector products whose matrices do not fit the SGPRs.)
template <int D, int DS, typename Stage>
__device__ __forceinline__ void ts_carry(const int64_t *__restrict__ in_off, int64_t n_tiles, const int32_t *__restrict__ first_tile,
                                         const double *__restrict__ sums, double *__restrict__ starts, const Stage S)
{
    static_assert(DS <= D && D <= 4, "16 elements of a thread in registers");
    __shared__ double s_sc[2][D * TS_THREADS];
    const int tid = threadIdx.x;
    int nt;
    int64_t first;
    if (!ts_signal(in_off, n_tiles, first_tile, nt, first)) return;
    const auto level = [&](const double (&o)[D], int k, double (&v)[D]) { S.level(o, k, v); };
    double carry[DS];
#pragma unroll
    for (int i = 0; i < DS; ++i) carry[i] = 0.0;
    for (int c = 0; c < nt; c += TS_THREADS * TS_RUN) {
        const int t0 = c + tid * TS_RUN;
        double z[TS_RUN][D], v[D];
#pragma unroll
        for (int e = 0; e < TS_RUN; ++e)
#pragma unroll
            for (int i = 0; i < D; ++i) z[e][i] = t0 + e < nt ? sums[D * (first + t0 + e) + i] : 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) v[i] = 0.0;
        if (tid == 0) S.seed(v, carry);
#pragma unroll
        for (int e = 0; e < TS_RUN; ++e) S.append(v, z[e]);
        if (tid == 0) S.join(v, carry);
        const int cur = ts_scan(v, level, s_sc);
        double st[DS];
#pragma unroll
        for (int i = 0; i < DS; ++i) st[i] = tid == 0 ? carry[i] : s_sc[cur][i * TS_THREADS + tid - 1];
#pragma unroll
        for (int i = 0; i < DS; ++i) carry[i] = s_sc[cur][i * TS_THREADS + TS_THREADS - 1];
#pragma unroll
        for (int e = 0; e < TS_RUN; ++e) {
            if (t0 + e < nt) {
#pragma unroll
                for (int i = 0; i < DS; ++i) starts[DS * (first + t0 + e) + i] = st[i];
            }
            S.step(st, z[e]);
        }
        __syncthreads();                                        // (the next round's scan writes the buffers read above)
    }
}
