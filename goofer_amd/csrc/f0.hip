// gf.extract_features' f0 post-processing (GOOFER.py:957-966; trackers.per_sample_f0 on the host) for a ragged batch of
// frame-rate f0 tracks, on the device (gfx950):
//
//   k_per_sample_f0   one lane per output sample: nan_to_num -> fix_f0_gaps (GOOFER.py:415-435) of the two track frames around
//                     the sample, np.interp over np.linspace(0, dur) grids of the track and of the samples (0 outside the track),
//                     clip to [1e-5, 2000], voicing = f0 > f0_min.  fp64 throughout; every value equals numpy's bit for bit.
//
// The frame grid is never stored: point j of linspace(0, dur, L) is j * (dur / (L - 1)), the last one dur itself, so the sample's
// interval is found from the quotient t / step and at most one step either way.  A bridged gap value depends only on its run's
// two neighbours, so each lane recomputes the (at most two) frames it reads: a run is followed at most max_gap frames each way.
#include <cfloat>

#include "common.h"

#pragma clang fp contract(off)

namespace {

// Largest s < n with off[s] <= g (off ascending, off[0] <= g): the signal a flat sample index belongs to, empty signals skipped.
__device__ __forceinline__ int f0_signal(const int64_t *__restrict__ off, int n, int64_t g)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// np.nan_to_num of one value
__device__ __forceinline__ double f0_nz(double v)
{
    if (__builtin_isnan(v)) return 0.0;
    if (__builtin_isinf(v)) return v > 0.0 ? DBL_MAX : -DBL_MAX;
    return v;
}

// Frame k of fix_f0_gaps(nan_to_num(track)): a zero inside a run of at most max_gap zeros with a neighbour on both sides is
// left * (1 - r) + right * r, r = (k - a + 1) / (gap + 1) for the run [a, a + gap); any other frame keeps its value.
__device__ __forceinline__ double f0_fixed(const double *__restrict__ tr, int64_t L, int64_t k, int max_gap)
{
    const double v = f0_nz(tr[k]);
    if (v != 0.0) return v;
    int64_t gap = 1;
    if (gap > max_gap) return 0.0;
    int64_t a = k;
    while (a > 0 && f0_nz(tr[a - 1]) == 0.0) {
        --a;
        if (++gap > max_gap) return 0.0;
    }
    int64_t b = k + 1;
    while (b < L && f0_nz(tr[b]) == 0.0) {
        ++b;
        if (++gap > max_gap) return 0.0;
    }
    if (a == 0 || b == L) return 0.0;                            // the run touches an end
    const double left = f0_nz(tr[a - 1]), right = f0_nz(tr[b]);
    const double r = (double)(k - a + 1) / (double)(gap + 1);
    return __dadd_rn(__dmul_rn(left, 1.0 - r), __dmul_rn(right, r));
}

// Point i of np.linspace(0, dur, num) (num >= 1): i * step with step = dur / (num - 1), the last point dur exactly.
__device__ __forceinline__ double f0_grid(int64_t i, int64_t num, double step, double dur)
{
    if (num == 1) return 0.0;
    return i == num - 1 ? dur : __dmul_rn((double)i, step);
}

__global__ __launch_bounds__(256) void k_per_sample_f0(const double *__restrict__ tracks, const int64_t *__restrict__ track_off,
                                                       const int64_t *__restrict__ sample_off, int n_signals, int64_t total,
                                                       double sr, double f0_min, int max_gap, double *__restrict__ f0_out,
                                                       double *__restrict__ mask_out)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int s = f0_signal(sample_off, n_signals, g);
    const int64_t s0 = sample_off[s], n = sample_off[s + 1] - s0, i = g - s0;
    const int64_t t0 = track_off[s], L = track_off[s + 1] - t0;  // L >= 2 (checked on the host)
    const double *tr = tracks + t0;
    const double dur = (double)n / sr;
    const double step_s = n > 1 ? dur / (double)(n - 1) : 0.0;
    const double step_t = dur / (double)(L - 1);
    const double x = f0_grid(i, n, step_s, dur);
    const double x_last = dur;                                   // t_track[-1]
    double v = 0.0;
    if (x >= 0.0 && x <= x_last) {
        // np.interp: j = the largest index with xp[j] <= x
        int64_t j = (int64_t)(x / step_t);
        j = j < 0 ? 0 : (j > L - 1 ? L - 1 : j);
        while (j > 0 && f0_grid(j, L, step_t, dur) > x) --j;
        while (j < L - 1 && f0_grid(j + 1, L, step_t, dur) <= x) ++j;
        const double xj = f0_grid(j, L, step_t, dur);
        if (j == L - 1 || xj == x) {
            v = f0_fixed(tr, L, j, max_gap);
        } else {
            const double xj1 = f0_grid(j + 1, L, step_t, dur);
            const double yj = f0_fixed(tr, L, j, max_gap), yj1 = f0_fixed(tr, L, j + 1, max_gap);
            const double slope = (yj1 - yj) / (xj1 - xj);
            v = __dadd_rn(__dmul_rn(slope, x - xj), yj);
            if (__builtin_isnan(v)) {                            // numpy retries from the right end, then takes the flat value
                v = __dadd_rn(__dmul_rn(slope, x - xj1), yj1);
                if (__builtin_isnan(v) && yj == yj1) v = yj;
            }
        }
    }
    if (!__builtin_isnan(v)) v = v < 1e-5 ? 1e-5 : (v > 2000.0 ? 2000.0 : v);   // np.clip keeps a NaN
    f0_out[g] = v;
    mask_out[g] = v > f0_min ? 1.0 : 0.0;
}

}  // namespace

extern "C" int goofer_per_sample_f0(goofer_ctx *ctx, const double *tracks, const int64_t *track_off, const int64_t *sample_off,
                                    int n_signals, double sr, double f0_min, int max_gap, double *f0, double *mask, void *scratch,
                                    int64_t *scratch_bytes, void *stream)
{
    if (!track_off || !sample_off || !scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "per_sample_f0: null offsets / scratch_bytes");
    if (n_signals <= 0) return goofer_fail(ctx, GOOFER_EINVAL, "per_sample_f0: %d signals", n_signals);
    if (!(sr > 0.0) || !(sr < DBL_MAX)) return goofer_fail(ctx, GOOFER_EINVAL, "per_sample_f0: sample rate %g", sr);
    if (track_off[0] != 0 || sample_off[0] != 0) return goofer_fail(ctx, GOOFER_EINVAL, "per_sample_f0: offsets must start at 0");
    for (int s = 0; s < n_signals; ++s) {
        if (track_off[s + 1] - track_off[s] < 2)
            return goofer_fail(ctx, GOOFER_EINVAL, "per_sample_f0: track %d has %lld frames (two at least)", s,
                               (long long)(track_off[s + 1] - track_off[s]));
        if (sample_off[s + 1] < sample_off[s]) return goofer_fail(ctx, GOOFER_EINVAL, "per_sample_f0: sample offsets descend at %d", s);
    }
    const int64_t total = sample_off[n_signals];
    if (scratch) {
        if (!ctx) return GOOFER_EINVAL;
        if (total > 0 && (!tracks || !f0 || !mask)) return goofer_fail(ctx, GOOFER_EINVAL, "per_sample_f0: null tracks / outputs");
    }
    int64_t *d_toff, *d_soff;
    int rc = caller_scratch(ctx, scratch, scratch_bytes, "per_sample_f0", [&](arena &a) {
        d_toff = a.take<int64_t>(n_signals + 1);
        d_soff = a.take<int64_t>(n_signals + 1);
    });
    if (rc || !scratch) return rc;
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return goofer_fail(ctx, GOOFER_EINVAL, "per_sample_f0: %lld samples in one call", (long long)total);
    if (total == 0) return GOOFER_OK;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, hipMemcpyAsync(d_toff, track_off, 8 * (size_t)(n_signals + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_soff, sample_off, 8 * (size_t)(n_signals + 1), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_per_sample_f0, dim3((unsigned)blocks), dim3(256), 0, st, tracks, d_toff, d_soff, n_signals, total, sr, f0_min,
                       max_gap, f0, mask);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}
