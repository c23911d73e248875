// The overlap-add walk of the frame walkers, written once (gfx950).
//
// A wave walks a run of consecutive frames of the concatenated frame axis, inverse-transforms every frame and overlap-adds the
// windowed samples in ascending frame order — the reference's fp32 order (GOOFER.py:379-385).  After frame t hop t is complete:
// it is divided by the summed squared window, scaled by the smoothed-mask gain and stored.  A run that starts inside a note
// first replays the `halo` frames before it (accumulate only); the wave that owns a note's last frame also flushes the hops
// behind it and the zero tail (GOOFER.py:402-413).
//
//   k_irfft_ola3, k_irfft_ola1 (samples.hip)   open sums in LDS rings: every piece below
//   k_noise_stems, k_harm_stem (stems.hip)     open sums in registers (hop == n_fft / 4): the run range and the window sums, through
//                                              `walker`; the knot window and the finished-hop walk stay their own text there for
//                                              measured reasons (docs/EXPERIMENTS.md)
#pragma once
#include "fft_core.h"
#include "samples_core.h"

// --- run range -------------------------------------------------------------------------------
// First frame f0 of wave `wave` of run group `group` (wpb waves per group); a wave whose f0 is not below total_frames has no
// frame and returns.  (The test stays with the kernel: returned through a flag it left a second branch on the same condition
// in the frame loop's way — k_irfft_ola3<1024> 118 -> 124 spilled scalar registers.)
__device__ __forceinline__ int64_t ola_run_first(int64_t group, int wpb, int wave, int run) { return (group * wpb + wave) * run; }
// The run [f0, f1) and fs = its first frame to transform: the halo in front of a run that starts inside a note
__device__ __forceinline__ void ola_run_span(int64_t f0, int run, int halo, int64_t total_frames, const int *frame_note,
                                             const int64_t *frame_off, int64_t &fs, int64_t &f1)
{
    f1 = f0 + run < total_frames ? f0 + run : total_frames;
    const int64_t t0 = f0 - frame_off[frame_note[f0]];
    fs = f0 - (t0 < halo ? t0 : halo);
}

// --- window sums (GOOFER.py:385-389) ------------------------------------------------------------
// Summed squared window of hop sample j < hop when every covering frame exists, and its correctly rounded reciprocal (div_by)
__device__ __forceinline__ void ola_full_ws(const float *win, int nf, int hop, int j, float &ws, float &rws)
{
    float s = 0.f;
    for (int q = (nf - 1 - j) / hop; q >= 0; --q) {           // ascending frame order = descending offset
        const float w = win[j + q * hop];
        s += w * w;
    }
    ws = s;
    rws = 1.0f / s;
}
// every position of a hop >= ola_max_back has all its frames behind it ...
__device__ __forceinline__ constexpr int ola_max_back(int nf, int hop) { return (nf - 1) / hop; }
// ... and hop h of a note of T frames is interior (wave-uniform) when they also exist ahead
__device__ __forceinline__ bool ola_interior(int h, int max_back, int T) { return h >= max_back && h <= T - 1; }
// the sum over the frames that exist, for sample j of hop h
__device__ __forceinline__ float ola_partial_ws(const float *win, int nf, int hop, int T, int h, int j)
{
    const int back = (nf - 1 - j) / hop;
    const int flo = h - back < 0 ? 0 : h - back, fhi = h > T - 1 ? T - 1 : h;
    float ws = 0.f;
    for (int fr = flo; fr <= fhi; ++fr) {
        const float w = win[j + (h - fr) * hop];
        ws += w * w;
    }
    return ws;
}

// --- knot window -------------------------------------------------------------------------------
// The smoothed-mask knots a hop needs (hop / MASK_DS of them, plus the KNOT_MARGIN the exact index search may reach) are fetched
// lane-parallel a frame ahead and parked in the wave's LDS slice, so the output stage reads them with LDS latency instead of
// issuing dependent global loads per sample.  MAXHOP: the widest hop the slice holds.
template <int MAXHOP> struct knot_window {
    static constexpr int KPL = (MAXHOP / MASK_DS + KNOT_MARGIN + WAVE - 1) / WAVE;
    double r[KPL];
    int lo = 0;

    // knots of hop h (m = n_fft / 2: output sample of the hop's first position is h hop - m) of a note of ns knots at ss
    __device__ __forceinline__ void fetch(int h, int hop, int m, float kps, int ns, const double *ss, int kn, int lane)
    {
        int i0 = h * hop - m;
        i0 = i0 < 0 ? 0 : i0;
        int l = (int)((float)i0 * kps) - 4;
        l = l < 0 ? 0 : l;
#pragma unroll
        for (int c = 0; c < KPL; ++c) {
            const int e = lane + WAVE * c;
            const int k = l + e < ns - 1 ? l + e : ns - 1;
            r[c] = (e < kn && ns > 0) ? ss[k] : 0.0;
        }
        lo = l;
    }
    __device__ __forceinline__ void park(double *kbuf, int kn, int lane) const
    {
#pragma unroll
        for (int c = 0; c < KPL; ++c) {
            const int e = lane + WAVE * c;
            if (e < kn) kbuf[e] = r[c];
        }
        wave_lds_sync();
    }
    // knot k from the parked window
    __device__ __forceinline__ static double at(const double *kbuf, int kn, int lo, int k)
    {
        const int e = k - lo;
        return kbuf[e < kn - 1 ? e : kn - 1];
    }
};

// --- finished hops -----------------------------------------------------------------------------
// After frame t: emit(t); behind a note's last frame also the hops up to the one holding sample n - 1 (the sums still open, then
// the zero tail), with next(h) between two hops: the next knot fetch, or the register walkers' carry -> out move.
template <class Emit, class Next>
__device__ __forceinline__ void ola_finish_hops(int t, int T, int hop, int m, int n, Emit &&emit, Next &&next)
{
    for (int h = t;;) {
        emit(h);
        ++h;
        if (t != T - 1 || h * hop - m >= n) break;
        next(h);
    }
}

// --- note state of the LDS-ring kernels -----------------------------------------------------------
struct ola_note {
    int note = -1;
    int64_t base = 0, fbase = 0;
    int n = 0, T = 0, ns = 0, out_len = 0;
    float kps = 0.f;
    double step_n = 0.0, step_s = 0.0;
    const double *ss = nullptr;

    __device__ __forceinline__ void enter(int nt, int hop, const int64_t *sample_off, const int64_t *frame_off, const double *steps,
                                          const double *short_s)
    {
        note = nt;
        base = sample_off[nt];
        n = (int)(sample_off[nt + 1] - base);
        fbase = frame_off[nt];
        T = (int)(frame_off[nt + 1] - fbase);
        ns = (n + MASK_DS - 1) / MASK_DS;
        out_len = hop * (T - 1);
        step_n = steps[2 * nt];
        step_s = steps[2 * nt + 1];
        kps = n > 1 ? (float)(ns - 1) / (float)(n - 1) : 0.f;
        ss = short_s + short_base(sample_off, nt);
    }
};

// --- ring accumulate -----------------------------------------------------------------------------
// Frame t adds its windowed samples to ring positions [t hop, t hop + NF) mod NF; sample pair m is a first contribution — the
// sum starts from zero — in a note's first frame and on the frame's last hop.
__device__ __forceinline__ bool ola_first(int t, int m, int nf, int hop) { return t == 0 || 2 * m >= nf - hop; }
__device__ __forceinline__ int ola_shift(int t, int nf, int hop) { return (t * hop) & (nf - 1); }
__device__ __forceinline__ float2 *ola_slot(float *ring, int shift, int m, int nf)
{
    return reinterpret_cast<float2 *>(ring + ((2 * m + shift) & (nf - 1)));
}
// This lane's R transform points z (pair m = lane + 64 r, window win_of(r)) into the ring: all ring reads of a CHUNK, then all
// its writes — the slots of a lane are distinct, and a branch-free body lets the LDS reads overlap instead of paying one round
// trip per slot.
template <int NF, int R, int CHUNK, class Win>
__device__ __forceinline__ void ola_ring_add(float *ring, const float2 (&z)[R], int t, int hop, int lane, Win &&win_of)
{
    static_assert(R % CHUNK == 0, "whole chunks");
    const int shift = ola_shift(t, NF, hop);
#pragma unroll
    for (int r0 = 0; r0 < R; r0 += CHUNK) {
        float2 o[CHUNK];
#pragma unroll
        for (int q = 0; q < CHUNK; ++q) o[q] = *ola_slot(ring, shift, lane + WAVE * (r0 + q), NF);
#pragma unroll
        for (int q = 0; q < CHUNK; ++q) {
            const int m = lane + WAVE * (r0 + q);
            const float2 wn = win_of(r0 + q);
            const float a = z[r0 + q].x * wn.x, b = z[r0 + q].y * wn.y;
            const bool first = ola_first(t, m, NF, hop);          // first contribution: y starts from zero
            *ola_slot(ring, shift, m, NF) = make_float2(first ? a : o[q].x + a, first ? b : o[q].y + b);
        }
    }
}

// --- LDS layout of the ring kernels ----------------------------------------------------------------
// Workgroup tables (FFT twiddles, half-bin twiddles, synthesis window), then per wave: the FFT exchange buffer, STEMS rings of
// n_fft accumulators, and a slice of kn knots (0: the knots are read from global memory).  The kernel carves from this and the
// launcher sizes from it.
template <int M, int WPB, int STEMS> struct ola_lds {
    static constexpr int NF = 2 * M, BUF = fft_cfg<M>::BUF;
    static constexpr size_t o_twh = sizeof(float2) * M, o_bufs = o_twh + sizeof(float2) * (M / 2 + 1), o_win = o_bufs + sizeof(float2) * WPB * BUF,
                            o_rings = o_win + sizeof(float) * NF, o_knots = o_rings + sizeof(float) * WPB * STEMS * NF;
    static_assert(o_knots % sizeof(double) == 0, "the knot slices hold doubles");
    static size_t bytes(int kn) { return o_knots + 16 + sizeof(double) * WPB * kn; }   // (+ 16: the slack fft_lds_bytes carries)

    float2 *tw, *twh, *buf;        // buf, ring, kbuf: this wave's
    float *win, *ring;
    double *kbuf;
    __device__ __forceinline__ void carve(unsigned char *smem, int wave, int kn)
    {
        tw = reinterpret_cast<float2 *>(smem);
        twh = reinterpret_cast<float2 *>(smem + o_twh);
        buf = reinterpret_cast<float2 *>(smem + o_bufs) + wave * BUF;
        win = reinterpret_cast<float *>(smem + o_win);
        ring = reinterpret_cast<float *>(smem + o_rings) + (size_t)wave * STEMS * NF;
        kbuf = reinterpret_cast<double *>(smem + o_knots) + (size_t)wave * kn;
    }
};
