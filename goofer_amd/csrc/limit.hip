// Look-ahead peak limiter on the device (gfx950): finished audio — the notes of a batch back to back, or a phrase's track, at the
// output rate — brought under a ceiling c immediately in front of goofer_pcm16, over a ragged batch in one launch.  The
// definition (the raised-cosine table, the windowed minimum, the order of the fp32 sum) is in include/goofer_hip.h; the host
// half, goofer_host_limit_plan (planner.hip), makes the look-ahead W, the table w[2W + 1] and the tile table.
//
// All FIR and min / max, no recursion: an output sample depends on the 4W + 1 input samples around it, of its own signal only.
// One workgroup of 512 threads per tile of GOOFER_LIMIT_TILE samples of one signal (the planner's table says which: no search):
//   1  r = c / |x| (or 1) of the tile and 2W samples of halo on either side into LDS; positions outside the signal hold 1, the
//      identity of a minimum over values that are at most 1, so an edge runs the code of the inside.  The tile's |x| maximum on the
//      way.  A tile without a sample above c, halo included, copies x to out and is done (option "limit_skip"; the definition's
//      identity property: the same bits).
//   2  window minima by doubling, in place: after the pass of step s, entry k holds min r[k .. k + 2s - 1].  K passes for the
//      largest 2^K <= 2W + 1; a window of 2W + 1 is two overlapping reads of that.  Exact in any order.
//   3  d = 1 - m of the tile and W samples on either side into a second LDS array, with the definition's index clamp applied
//      here (a position outside the signal holds the d of the signal's first or last sample), so the sum below has no guard.
//   4  the 2W + 1-tap sum: a thread owns eight consecutive samples and slides a window of d over them in registers, four taps and
//      one 16-byte LDS read a step; at a given tap all lanes use the same w[j] (scalar loads).  One rounded multiply and one
//      rounded add per tap in ascending j (the library is built with -ffp-contract=off).
//   5  s = max(1 - acc, 0), g = min(s, r) with r made again from x, y = x g stored once; the tile's minimum of g.
// Statistics: a butterfly per wave (peak_in: then over the workgroup's waves through LDS), then an integer atomic on the fp32
// bits (max for peak_in, min for min_gain; exact for non-negative values, any order) where the value would move the word, into
// words a small kernel in front has set to 0 and 1.  No scratch buffer.
//
// True-peak detection (the header's "true-peak detection" section; table: goofer_host_true_peak_plan).  k_limit<true> differs
// in step 1 only: x of [t0 - 2W - Z, t0 + T + 2W + Z) goes to LDS first (where B will live later), a thread then makes the
// envelope e of eight consecutive positions from a window of 32 staged samples sliding through its registers (tp_envelope: the
// R - 1 rows of 24 taps by scalar loads, the nine interval maxima u the eight positions touch), and r = c / e.  Step 5 cannot
// make r again from x, so the r of the tile's own samples waits in a third LDS array.  A tile whose e never exceeds c, halo
// included, copies its samples (option "limit_tp_skip").  k_true_peak, the meter, is step 1 alone on a tile with Z samples of
// halo: the maximum of e, through limit_stat_max.
#include "launchers.h"

#define LM_THREADS 512
#define LM_SPT 8                       // consecutive samples per thread in the tap sum
#define LM_T GOOFER_LIMIT_TILE
static_assert(LM_T == LM_THREADS * LM_SPT, "one workgroup of 512 threads per tile");
#define LM_STAGE ((LM_T + 4 * GOOFER_LIMIT_MAX_LOOK) / LM_THREADS)   // entries of the r array per thread, at most
#define TP_Z GOOFER_TP_ZEROS
#define TP_K (2 * GOOFER_TP_ZEROS)     // taps of a row
#define TP_CH LM_SPT                   // consecutive envelope values per thread and step
#define TP_WIN (TP_CH + TP_K)          // staged samples they are made from
static_assert(TP_WIN % 4 == 0 && TP_CH % 4 == 0, "the window is read as float4");

// (min_gain may be null: the meter has a peak alone)
__global__ __launch_bounds__(256) void k_limit_init(int n, float *__restrict__ peak_in, float *__restrict__ min_gain)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        peak_in[i] = 0.0f;
        if (min_gain) min_gain[i] = 1.0f;
    }
}

__device__ __forceinline__ float limit_r(float a, float c) { return a > c ? __fdiv_rn(c, a) : 1.0f; }

// A statistic of a signal, v >= 0, into its word: the integer order of the bits is the order of the values.  The word only ever
// rises (max) or falls (min), so a value that would not move what a plain look finds there needs no atomic: the waves of
// thousands of tiles on one address are otherwise one queue (a 48.7 M-sample signal with an atomic per wave and statistic: 1.11 ms
// where its tiles only copy and 1.37 ms where they all do the arithmetic, against 0.17 and 1.02 ms with the look first).
__device__ __forceinline__ void limit_stat_max(float *p, float v)
{
    unsigned int *w = reinterpret_cast<unsigned int *>(p);
    const unsigned int b = __float_as_uint(v);
    if (b > __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(w, b);
}
__device__ __forceinline__ void limit_stat_min(float *p, float v)
{
    unsigned int *w = reinterpret_cast<unsigned int *>(p);
    const unsigned int b = __float_as_uint(v);
    if (b < __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(w, b);
}

// e[0 .. TP_CH) of the positions p0 .. p0 + TP_CH - 1 of a signal.  X (LDS, 16-byte aligned) holds the samples of positions
// p0 - Z .. p0 + TP_CH + Z - 1, zero outside the signal.  um[m] is u of position p0 - 1 + m, the interval between p0 - 1 + m and
// p0 + m: sum_c h[c] X[m + c], in ascending c from +0.0f.  Every lane uses the same coefficient at a given tap (scalar loads).
__device__ __forceinline__ void tp_envelope(const float *__restrict__ X, int R, const float *__restrict__ taps, int64_t p0, float *__restrict__ e)
{
    float win[TP_WIN], um[TP_CH + 1];
#pragma unroll
    for (int q = 0; q < TP_WIN / 4; ++q) {
        const float4 v = reinterpret_cast<const float4 *>(X)[q];
        win[4 * q] = v.x; win[4 * q + 1] = v.y; win[4 * q + 2] = v.z; win[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int m = 0; m <= TP_CH; ++m) um[m] = 0.0f;
#pragma unroll 1
    for (int ph = 0; ph < R - 1; ++ph) {
        const float *__restrict__ h = taps + ph * TP_K;
        float acc[TP_CH + 1];
#pragma unroll
        for (int m = 0; m <= TP_CH; ++m) acc[m] = 0.0f;
#pragma unroll
        for (int t = 0; t < TP_K; ++t) {
            const float ht = h[t];
#pragma unroll
            for (int m = 0; m <= TP_CH; ++m) acc[m] = acc[m] + ht * win[m + t];
        }
#pragma unroll
        for (int m = 0; m <= TP_CH; ++m) um[m] = fmaxf(um[m], fabsf(acc[m]));
    }
#pragma unroll
    for (int i = 0; i < TP_CH; ++i) {
        const float v = fmaxf(fabsf(win[i + TP_Z]), um[i + 1]);
        e[i] = p0 + i == 0 ? v : fmaxf(v, um[i]);               // u[-1] = 0
    }
}

// CH: the channels of a group (goofer_limit_linked), signals sig CH .. sig CH + CH - 1 of equal length lying back to back; a and
// so r, the gain and the statistics are the group's.  CH == 1 is goofer_limit / goofer_limit_tp: every loop over the channels
// has one round and `n` counts signals.
template <bool TP, int CH>
__global__ __launch_bounds__(LM_THREADS)
void k_limit(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, int W, int span, const float *__restrict__ taps, float c,
             const int32_t *__restrict__ tiles, float *__restrict__ out, float *__restrict__ peak_in, float *__restrict__ min_gain, int skip,
             int R, const float *__restrict__ tp_taps)
{
    extern __shared__ __align__(16) float s_lim[];
    __shared__ float s_pk[LM_THREADS / 64];
    const int tid = threadIdx.x;
    const int sig = __builtin_amdgcn_readfirstlane(tiles[2 * blockIdx.x]), kt = __builtin_amdgcn_readfirstlane(tiles[2 * blockIdx.x + 1]);
    if (sig < 0 || sig >= n / CH || kt < 0) return;             // (a table that is not the planner's: nothing is read or written)
    const int64_t base = in_off[sig * CH], len = in_off[sig * CH + 1] - base, t0 = (int64_t)kt * LM_T;
    if (t0 >= len) return;
#pragma unroll
    for (int ch = 1; ch < CH; ++ch)
        if (in_off[sig * CH + ch + 1] - in_off[sig * CH + ch] != len) return;   // (channels of unequal length: likewise)
    const int NA = LM_T + 4 * W, NB = LM_T + 2 * W;             // r on [t0 - 2W, t0 + T + 2W), d on [t0 - W, t0 + T + W)
    float *__restrict__ A = s_lim, *__restrict__ B = s_lim + NA;   // (NA is a multiple of 4: B is 16-byte aligned; B has NB + 4 entries)
    const float *__restrict__ xs = x + base;                    // channel ch: xs + ch len
    float *__restrict__ ys = out + base;
    const int live = (int)(len - t0 < LM_T ? len - t0 : LM_T);  // samples of the tile that exist

    // 1: r, the tile's peak, whether anything is above c
    float pk = 0.0f;
    bool over = false;
    if constexpr (TP) {
        // x on [t0 - 2W - Z, t0 + T + 2W + Z + TP_CH) where B will live; the r of the tile's own samples behind it
        // one channel after the other through the same X: the r of a later channel joins the one in A by a minimum (min_c c / e_c
        // = c / max_c e_c; a thread meets its own entries again, so no barrier lies between the two)
        const int NX = NA + TP_WIN;
        float *__restrict__ X = B, *__restrict__ Rt = B + NX;
#pragma unroll 1
        for (int ch = 0; ch < CH; ++ch) {
            const float *__restrict__ xc = xs + ch * len;
            if (ch > 0) __syncthreads();                        // (the channel before has read X)
            for (int k = tid; k < NX; k += LM_THREADS) {
                const int64_t p = t0 - 2 * W - TP_Z + k;
                X[k] = p >= 0 && p < len ? xc[p] : 0.0f;
            }
            __syncthreads();
            for (int k0 = tid * TP_CH; k0 < NA; k0 += LM_THREADS * TP_CH) {     // (NA is a multiple of 4: the last step may be half one)
                const int64_t p0 = t0 - 2 * W + k0;
                float e[TP_CH];
                const bool inside = p0 + TP_CH > 0 && p0 < len;
                if (inside) tp_envelope(X + k0, R, tp_taps, p0, e);
#pragma unroll
                for (int i = 0; i < TP_CH; ++i) {
                    const int k = k0 + i;
                    const int64_t p = p0 + i;
                    if (k < NA) {
                        float r = 1.0f;
                        const bool own = k >= 2 * W && k < 2 * W + LM_T;
                        if (inside && p >= 0 && p < len) {
                            r = limit_r(e[i], c);
                            over |= e[i] > c;
                            if (own) pk = fmaxf(pk, e[i]);
                        }
                        if (ch > 0) r = fminf(r, A[k]);
                        A[k] = r;
                        if (own) Rt[k - 2 * W] = r;
                    }
                }
            }
        }
    } else {
        for (int k = tid; k < NA; k += LM_THREADS) {
            const int64_t p = t0 - 2 * W + k;
            float r = 1.0f;
            if (p >= 0 && p < len) {
                float a = fabsf(xs[p]);
#pragma unroll
                for (int ch = 1; ch < CH; ++ch) a = fmaxf(a, fabsf(xs[ch * len + p]));
                r = limit_r(a, c);
                over |= a > c;
                if (k >= 2 * W && k < 2 * W + LM_T) pk = fmaxf(pk, a);
            }
            A[k] = r;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
    if ((tid & 63) == 0) s_pk[tid >> 6] = pk;
    const bool any = __syncthreads_or(over);                    // (the barrier also publishes A and s_pk)
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < LM_THREADS / 64; ++w) pk = fmaxf(pk, s_pk[w]);
        limit_stat_max(peak_in + sig, pk);
    }
    if (!any && skip) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
            for (int e = tid; e < live; e += LM_THREADS) ys[ch * len + t0 + e] = xs[ch * len + t0 + e];
        return;
    }

    // 2: in place, A[k] = min r[k .. k + span - 1]
    for (int s = 1; s < span; s <<= 1) {
        float v[LM_STAGE];
#pragma unroll
        for (int e = 0; e < LM_STAGE; ++e) {
            const int k = tid + e * LM_THREADS;
            if (k < NA) v[e] = fminf(A[k], k + s < NA ? A[k + s] : 1.0f);
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < LM_STAGE; ++e) {
            const int k = tid + e * LM_THREADS;
            if (k < NA) A[k] = v[e];
        }
        __syncthreads();
    }

    // 3: B[k] = d[clamp(t0 - W + k, 0, len - 1)]; m of position t0 - W + kc is the minimum over A[kc .. kc + 2W]
    const int second = 2 * W + 1 - span;
    for (int k = tid; k < NB + 4; k += LM_THREADS) {
        float d = 0.0f;                                         // (the four entries behind NB are loaded by step 4, never used)
        if (k < NB) {
            int64_t p = t0 - W + k;
            p = p < 0 ? 0 : (p > len - 1 ? len - 1 : p);
            const int kc = (int)(p - (t0 - W));                 // 0 <= kc < NB: W at most where p was raised to 0, at most k elsewhere
            d = 1.0f - fminf(A[kc], A[kc + second]);            // kc + second < NB + W <= NA
        }
        B[k] = d;
    }
    __syncthreads();

    // 4: acc[e] = sum_j w[j] d[i + j] of the thread's samples i = t0 + o + e
    if ((tid & ~63) * LM_SPT >= live) return;                   // a wave without a sample (no barrier from here on)
    const int o = tid * LM_SPT;
    float gmin = 1.0f;
    if (o < live) {
        float acc[LM_SPT], win[LM_SPT + 4];
#pragma unroll
        for (int e = 0; e < LM_SPT; ++e) acc[e] = 0.0f;
        {
            const float4 q0 = *reinterpret_cast<const float4 *>(B + o), q1 = *reinterpret_cast<const float4 *>(B + o + 4);
            win[0] = q0.x; win[1] = q0.y; win[2] = q0.z; win[3] = q0.w; win[4] = q1.x; win[5] = q1.y; win[6] = q1.z; win[7] = q1.w;
        }
        const int n_taps = 2 * W + 1;
        int j = 0;                                              // win[k] = B[o + j + k]
        for (; j + 4 <= n_taps; j += 4) {
            const float4 q = *reinterpret_cast<const float4 *>(B + o + j + LM_SPT);
            win[LM_SPT] = q.x; win[LM_SPT + 1] = q.y; win[LM_SPT + 2] = q.z; win[LM_SPT + 3] = q.w;
            float w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = taps[j + u];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < LM_SPT; ++e) acc[e] = acc[e] + w[u] * win[e + u];
#pragma unroll
            for (int e = 0; e < LM_SPT; ++e) win[e] = win[e + 4];
        }
        {                                                       // the last one or three taps (2W + 1 is odd)
            const float4 q = *reinterpret_cast<const float4 *>(B + o + j + LM_SPT);
            win[LM_SPT] = q.x; win[LM_SPT + 1] = q.y; win[LM_SPT + 2] = q.z; win[LM_SPT + 3] = q.w;
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                if (j + u < n_taps) {
                    const float w = taps[j + u];
#pragma unroll
                    for (int e = 0; e < LM_SPT; ++e) acc[e] = acc[e] + w * win[e + u];
                }
            }
        }
        // 5: the gain and the output
#pragma unroll
        for (int e = 0; e < LM_SPT; ++e) {
            if (o + e < live) {
                float xv[CH], a = 0.0f;
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) {
                    xv[ch] = xs[ch * len + t0 + o + e];
                    a = ch == 0 ? fabsf(xv[0]) : fmaxf(a, fabsf(xv[ch]));
                }
                float r;
                if constexpr (TP) r = s_lim[NA + NA + TP_WIN + o + e];     // (Rt of step 1)
                else r = limit_r(a, c);
                const float s = fmaxf(1.0f - acc[e], 0.0f);
                const float g = fminf(s, r);
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) ys[ch * len + t0 + o + e] = xv[ch] * g;
                gmin = fminf(gmin, g);
            }
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) gmin = fminf(gmin, __shfl_xor(gmin, s, 64));
    if ((tid & 63) == 0 && gmin < 1.0f) limit_stat_min(min_gain + sig, gmin);
}

// The meter: the maximum of e over a signal.  One workgroup per tile, a thread per TP_CH samples; always computes.
__global__ __launch_bounds__(LM_THREADS)
void k_true_peak(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, int R, const float *__restrict__ taps,
                 const int32_t *__restrict__ tiles, float *__restrict__ peak)
{
    __shared__ __align__(16) float X[LM_T + TP_K];              // positions t0 - Z .. t0 + T + Z - 1
    __shared__ float s_pk[LM_THREADS / 64];
    const int tid = threadIdx.x;
    const int sig = __builtin_amdgcn_readfirstlane(tiles[2 * blockIdx.x]), kt = __builtin_amdgcn_readfirstlane(tiles[2 * blockIdx.x + 1]);
    if (sig < 0 || sig >= n || kt < 0) return;
    const int64_t base = in_off[sig], len = in_off[sig + 1] - base, t0 = (int64_t)kt * LM_T;
    if (t0 >= len) return;
    const float *__restrict__ xs = x + base;
    const int live = (int)(len - t0 < LM_T ? len - t0 : LM_T);
    for (int k = tid; k < LM_T + TP_K; k += LM_THREADS) {
        const int64_t p = t0 - TP_Z + k;
        X[k] = p >= 0 && p < len ? xs[p] : 0.0f;
    }
    __syncthreads();
    float pk = 0.0f;
    const int o = tid * TP_CH;
    if (o < live) {
        float e[TP_CH];
        tp_envelope(X + o, R, taps, t0 + o, e);
#pragma unroll
        for (int i = 0; i < TP_CH; ++i)
            if (o + i < live) pk = fmaxf(pk, e[i]);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) pk = fmaxf(pk, __shfl_xor(pk, s, 64));
    if ((tid & 63) == 0) s_pk[tid >> 6] = pk;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < LM_THREADS / 64; ++w) pk = fmaxf(pk, s_pk[w]);
        limit_stat_max(peak + sig, pk);
    }
}

// one launch of k_limit<TP, CH>: `lds` dynamic bytes, `allow` the opt-in above 64 KB (beside s_pk's static bytes)
template <bool TP, int CH>
static int limit_launch(goofer_ctx *ctx, size_t lds, int allow, const float *x, const int64_t *in_off, int n, int W, int span, const float *taps,
                        float c, const int32_t *tiles, int64_t n_tiles, float *out, float *peak_in, float *min_gain, int skip, int R,
                        const float *tp_taps, hipStream_t st)
{
    if (lds > 64 * 1024)
        if (int rc = kernel_allow_max_lds(ctx, (const void *)k_limit<TP, CH>, allow)) return rc;
    hipLaunchKernelGGL((k_limit<TP, CH>), dim3((unsigned)n_tiles), dim3(LM_THREADS), lds, st, x, in_off, n, W, span, taps, c, tiles, out, peak_in,
                       min_gain, skip, R, tp_taps);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

// R == 0: sample peaks (goofer_limit); R == 2 or 4 with tp_taps: true-peak detection (goofer_limit_tp); ch: the channels of a
// group (goofer_limit_linked), n / ch groups and statistics
int launch_limit(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int W, const float *taps, float c, const int32_t *tiles,
                 int64_t n_tiles, float *out, float *peak_in, float *min_gain, hipStream_t st, int R, const float *tp_taps, int ch)
{
    if (n <= 0) return GOOFER_OK;
    const int groups = n / ch;
    hipLaunchKernelGGL(k_limit_init, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, groups, peak_in, min_gain);
    LAUNCH_CHECK(ctx);
    if (n_tiles <= 0) return GOOFER_OK;
    int span = 1;
    while (2 * span <= 2 * W + 1) span *= 2;
    if (R) {
        // r, x (later d) and the tile's own r: 56 960 bytes at W = 240, 82 048 at W = 1024; the channels share them
        const size_t lds = (2 * (size_t)(LM_T + 4 * W) + TP_WIN + LM_T) * sizeof(float);
        const int skip = ctx->limit_tp_skip ? 1 : 0;
        return ch == 2 ? limit_launch<true, 2>(ctx, lds, 96 * 1024, x, in_off, n, W, span, taps, c, tiles, n_tiles, out, peak_in, min_gain, skip, R, tp_taps, st)
                       : limit_launch<true, 1>(ctx, lds, 96 * 1024, x, in_off, n, W, span, taps, c, tiles, n_tiles, out, peak_in, min_gain, skip, R, tp_taps, st);
    }
    const size_t lds = ((size_t)(LM_T + 4 * W) + (size_t)(LM_T + 2 * W + 4)) * sizeof(float);   // 57 360 bytes at W = 1024
    const int skip = ctx->limit_skip ? 1 : 0;
    return ch == 2 ? limit_launch<false, 2>(ctx, lds, 160 * 1024, x, in_off, n, W, span, taps, c, tiles, n_tiles, out, peak_in, min_gain, skip, 0, nullptr, st)
                   : limit_launch<false, 1>(ctx, lds, 160 * 1024, x, in_off, n, W, span, taps, c, tiles, n_tiles, out, peak_in, min_gain, skip, 0, nullptr, st);
}

// the checks of goofer_limit, goofer_limit_tp (`tp`: R, Z and tp_taps too) and goofer_limit_linked (`ch` channels a group: the
// tile table is the planner's for the n / ch groups), then the launch
static int limit_entry(goofer_ctx *ctx, const char *who, bool tp, const float *x, const int64_t *in_off, int n, int64_t total, int W,
                       const float *taps, float c, const int32_t *tiles, int64_t n_tiles, float *out, float *peak_in, float *min_gain, int R,
                       int Z, const float *tp_taps, void *stream, int ch = 1)
{
    if (!ctx) return GOOFER_EINVAL;
    if (int rc = check_counts(ctx, who, n, total, n_tiles)) return rc;
    if ((ch != 1 && ch != 2) || n % ch != 0) return goofer_fail(ctx, GOOFER_EINVAL, "%s: %d signals in groups of %d channels (1 or 2)", who, n, ch);
    if (W < 1 || W > GOOFER_LIMIT_MAX_LOOK || !(c > 0.0f && c <= 1.0f) || !signal_tiles_ok(LM_T, n / ch, total / ch, n_tiles))
        return goofer_fail(ctx, GOOFER_EINVAL, "%s: W = %d, c = %g, %lld tiles for %lld samples in %d signals is not a geometry of goofer_host_limit_plan",
                           who, W, (double)c, (long long)n_tiles, (long long)total, n);
    if (tp && ((R != 2 && R != 4) || Z != GOOFER_TP_ZEROS))
        return goofer_fail(ctx, GOOFER_EINVAL, "%s: R = %d, Z = %d is not a geometry of goofer_host_true_peak_plan", who, R, Z);
    if (n == 0) return GOOFER_OK;
    if (!in_off || !taps || !peak_in || !min_gain || (tp && !tp_taps) || (total > 0 && (!x || !out || !tiles)))
        return goofer_fail(ctx, GOOFER_EINVAL, "%s: null pointer", who);
    if (int rc = check_aligned(ctx, who, "x, taps, tiles, out, peak_in and min_gain", {x, taps, out, tiles, peak_in, min_gain, tp_taps}, "in_off", {in_off}))
        return rc;
    if (int rc = check_overlap(ctx, who, x, out, total, false)) return rc;
    return launch_limit(ctx, x, in_off, n, W, taps, c, tiles, n_tiles, out, peak_in, min_gain, (hipStream_t)stream, tp ? R : 0, tp_taps, ch);
}

extern "C" int goofer_limit(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int W, const float *taps, float c,
                            const int32_t *tiles, int64_t n_tiles, float *out, float *peak_in, float *min_gain, void *stream)
{
    return limit_entry(ctx, "goofer_limit", false, x, in_off, n, total, W, taps, c, tiles, n_tiles, out, peak_in, min_gain, 0, 0, nullptr, stream);
}

extern "C" int goofer_limit_tp(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int W, const float *taps, float c,
                               const int32_t *tiles, int64_t n_tiles, float *out, float *peak_in, float *min_gain, int R, int Z,
                               const float *tp_taps, void *stream)
{
    return limit_entry(ctx, "goofer_limit_tp", true, x, in_off, n, total, W, taps, c, tiles, n_tiles, out, peak_in, min_gain, R, Z, tp_taps, stream);
}

extern "C" int goofer_limit_linked(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int ch, int W, const float *taps,
                                   float c, const int32_t *tiles, int64_t n_tiles, float *out, float *peak_in, float *min_gain, int R,
                                   const float *tp_taps, void *stream)
{
    return limit_entry(ctx, "goofer_limit_linked", R != 0, x, in_off, n, total, W, taps, c, tiles, n_tiles, out, peak_in, min_gain, R, GOOFER_TP_ZEROS,
                       R != 0 ? tp_taps : nullptr, stream, ch);
}

extern "C" int goofer_true_peak(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int R, int Z, const float *taps,
                                const int32_t *tiles, int64_t n_tiles, float *peak, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (int rc = check_counts(ctx, "goofer_true_peak", n, total, n_tiles)) return rc;
    if ((R != 2 && R != 4) || Z != GOOFER_TP_ZEROS || !signal_tiles_ok(LM_T, n, total, n_tiles))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_true_peak: R = %d, Z = %d, %lld tiles for %lld samples in %d signals is not a geometry of goofer_host_true_peak_plan and goofer_host_limit_plan",
                           R, Z, (long long)n_tiles, (long long)total, n);
    if (n == 0) return GOOFER_OK;
    if (!in_off || !taps || !peak || (total > 0 && (!x || !tiles)))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_true_peak: null pointer");
    if (int rc = check_aligned(ctx, "goofer_true_peak", "x, taps, tiles and peak", {x, taps, tiles, peak}, "in_off", {in_off})) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_limit_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, peak, (float *)nullptr);
    LAUNCH_CHECK(ctx);
    if (n_tiles <= 0) return GOOFER_OK;
    hipLaunchKernelGGL(k_true_peak, dim3((unsigned)n_tiles), dim3(LM_THREADS), 0, st, x, in_off, n, R, taps, tiles, peak);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}
