// Framewise real FFT / inverse FFT / overlap-add for gfx950.
//
//   k_rfft_*        replace gf.stft         (GOOFER.py:355-370)
//   k_irfft_*       replace np.fft.irfft in gf.istft (GOOFER.py:399-400) and the `frames*window`
//                   product of _overlap_add (GOOFER.py:383)
//   k_ola_gather    replaces _overlap_add + trim/pad of istft (GOOFER.py:372-390, 402-413)
//
// A real n_fft-point transform is a complex M = n_fft/2 point transform (fft_core.h) between two real-input stages: frame
// fetch + window and the even/odd split going forward, the conj-trick input stage and the scaled, windowed store going back.
// Each stage is written once below, against
//   * an owner (fft_core.h): the 64-lane wave for n_fft up to 2048, the 256-thread workgroup above;
//   * the form of the M-point transform: NATIVE (M = 64 or 256 times a radix, the owner's own transform: Z in the padded
//     buffer, half-bin twiddles mirrored about M/2) or Bluestein (any M at run time on a power-of-two transform of length
//     L >= 2 M - 1: Z[k] at buf[k], a table of M + 1 half-bin twiddles, threads past M idle);
//   * plain pointers for its tables (frame_tables): the wave kernels keep them in LDS, the workgroup kernels read window,
//     half-bin twiddles and chirp from global memory.
// The kernels are shells that carve LDS and name an instantiation; with_transform maps a plan to one.  Two keep a frame loop
// of their own around the same stages: k_rfft_frames, the hot one (two frames in flight), and k_irfft_frames (its input stage
// in place).  No MFMA: ~5 flop/B, HBM-bound.
#include "fft_core.h"
#include "launchers.h"

struct frame_tables {
    const float2 *tw;                     // exp(-2 pi i k / N) of the owner's N-point transform (LDS)
    const float2 *twh, *win;              // half-bin twiddles e^{-i pi k/M}; the window as (even, odd) sample pairs
    const float2 *chirp, *bhat;           // Bluestein only: c_n, n < M, and the transform of the wrapped chirp
    float2 *buf;                          // exchange buffers (LDS): the owner's is buf + O::first() * O::BUF
    // Tables in global memory do not change from frame to frame, and hoisted out of the frame loop their per-thread values
    // would take some 130 registers at 16 points per thread: an offset of 0 the compiler cannot see through, once per
    // frame, makes each frame read them again (from L2) where it uses them.
    __device__ __forceinline__ void reread()
    {
        int o = 0;
        asm volatile("" : "+s"(o));
        twh += o; win += o; chirp += o; bhat += o;
    }
};

template <bool NATIVE> __device__ __forceinline__ constexpr int z_at(int k) { return NATIVE ? lds_pad(k) : k; }

// e^{-i pi k/M}, k < M, or its conjugate (the inverse input stage's factor)
template <bool NATIVE, bool CONJ> __device__ __forceinline__ float2 half_twiddle(const float2 *twh, int M, int k)
{
    if (!NATIVE || k <= M / 2) return CONJ ? cconj(twh[k]) : twh[k];
    return make_float2(-twh[M - k].x, CONJ ? -twh[M - k].y : twh[M - k].y);   // (the native table holds M / 2 + 1 entries)
}

// ---- forward stages --------------------------------------------------------------------------
// The raw (even, odd) sample pairs m = tid + W r of frame f, reflect-padded at the note ends (numpy 'reflect'; n == 1 is
// 'edge', GOOFER.py:358-369); zero for m >= M.
template <class O, bool NATIVE>
__device__ __forceinline__ void fetch_frame(float2 (&raw)[O::P], const float *__restrict__ x, const int64_t *__restrict__ sample_off,
                                            const int64_t *__restrict__ frame_off, const int *__restrict__ frame_note, int64_t f,
                                            int hop, int M, int tid)
{
    const int note = frame_note[f];
    const int64_t base = sample_off[note];
    const int64_t n = sample_off[note + 1] - base;
    const int64_t t = f - frame_off[note];
    const int64_t start = t * hop - M;                        // first sample of the frame, un-padded coordinates
    const float *xs = x + base;
    if (start >= 0 && start + 2 * M <= n) {
#pragma unroll
        for (int r = 0; r < O::P; ++r) {
            const int m = tid + O::W * r;
            raw[r] = (NATIVE || m < M) ? make_float2(xs[start + 2 * m], xs[start + 2 * m + 1]) : make_float2(0.f, 0.f);
        }
    } else {
#pragma unroll
        for (int r = 0; r < O::P; ++r) {
            const int m = tid + O::W * r;
            const bool in = (NATIVE || m < M) && n > 0;
            const float a = in ? xs[reflect_index(start + 2 * m, n)] : 0.f;
            const float b = in ? xs[reflect_index(start + 2 * m + 1, n)] : 0.f;
            raw[r] = make_float2(a, b);
        }
    }
}

template <class O, bool NATIVE>
__device__ __forceinline__ void window_frame(float2 (&v)[O::P], const float2 *win, int M, int tid)
{
#pragma unroll
    for (int r = 0; r < O::P; ++r) {
        const int m = tid + O::W * r;
        if (NATIVE || m < M) {
            const float2 w = win[m];
            v[r] = make_float2(v[r].x * w.x, v[r].y * w.y);
        }
    }
}

// even/odd split of bin k < M: X[k] = (Z[k] + conj Z[M-k])/2 - i/2 e^{-i pi k/M} (Z[k] - conj Z[M-k])
template <bool NATIVE> __device__ __forceinline__ float2 rfft_bin(const float2 *buf, const float2 *twh, int M, int k)
{
    const float2 zk = buf[z_at<NATIVE>(k)], zm = buf[z_at<NATIVE>(k == 0 ? 0 : M - k)];
    const float2 w = half_twiddle<NATIVE, false>(twh, M, k);
    const float2 A = make_float2(zk.x + zm.x, zk.y - zm.y), B = make_float2(zk.x - zm.x, zk.y + zm.y);
    const float2 C = cmul(w, B);
    return make_float2(0.5f * (A.x + C.y), 0.5f * (A.y - C.x));
}
__device__ __forceinline__ float2 rfft_last_bin(const float2 *buf)   // X[M], from Z[0]
{
    const float2 z0 = buf[0];
    return make_float2(z0.x - z0.y, 0.f);
}

// an owner's bins of one row, 8 bytes per store
template <class O, bool NATIVE>
__device__ __forceinline__ void split_frame(const float2 *buf, const float2 *twh, int M, float2 *row, int tid)
{
#pragma unroll
    for (int r = 0; r < O::P; ++r) {
        const int k = tid + O::W * r;
        if (NATIVE || k < M) row[k] = rfft_bin<NATIVE>(buf, twh, M, k);
    }
    if (tid == 0) row[M] = rfft_last_bin(buf);
}

// ---- inverse stages --------------------------------------------------------------------------
// S row -> the points this thread feeds into the forward transform (conj trick: Z = (A + i C)/2, inverse FFT =
// conj(FFT(conj Z)); irfft_pre).  Im of DC and Nyquist is ignored like pocketfft's c2r.
template <class O, bool NATIVE>
__device__ __forceinline__ void irfft_load(float2 (&v)[O::P], const float2 *row, const float2 *twh, int M, int tid)
{
#pragma unroll
    for (int r = 0; r < O::P; ++r) {
        const int k = tid + O::W * r;
        if (NATIVE || k < M) {
            float2 xk = row[k], xm = row[M - k];
            if (k == 0) { xk.y = 0.f; xm.y = 0.f; }
            v[r] = irfft_pre(xk, xm, half_twiddle<NATIVE, true>(twh, M, k));
        } else {
            v[r] = make_float2(0.f, 0.f);
        }
    }
}

// transform result -> windowed time frame (fp32 irfft value times window[j], the `val` of _overlap_add)
template <class O, bool NATIVE>
__device__ __forceinline__ void irfft_store(const float2 *buf, const float2 *win, int M, float2 *out, int tid)
{
    const float inv_m = 0.5f / (float)M;                      // 1/M of the transform and the 1/2 that irfft_pre leaves out
#pragma unroll
    for (int r = 0; r < O::P; ++r) {
        const int m = tid + O::W * r;
        if (NATIVE || m < M) {
            const float2 z = buf[z_at<NATIVE>(m)], w = win[m];
            out[m] = make_float2((z.x * inv_m) * w.x, (-z.y * inv_m) * w.y);
        }
    }
}

// ---- the M-point transform --------------------------------------------------------------------
// Transform sizes without a radix plan (any even n_fft): Bluestein's chirp-z form of the M = n_fft / 2 point complex DFT,
// Z_k = conj(c_k) sum_n (z_n conj(c_n)) c_{k-n} with c_n = exp(i pi n^2 / M) — a circular convolution of length L >= 2 M - 1 (a
// power of two, the owner's transform) with the wrapped chirp, whose transform goofer_plan made in fp64.  Two L-point transforms
// and three complex products per point; fp32 error ~4e-7 relative.
//
// v[r] = z[tid + W r] (anything for indices >= M) on entry; Z[k], k < M, in natural order in buf[k] (un-padded) on exit.
template <class O>
__device__ __forceinline__ void bluestein_dft(float2 (&v)[O::P], int M, const frame_tables &t, int tid)
{
    float2 *buf = t.buf;
#pragma unroll
    for (int r = 0; r < O::P; ++r) {
        const int n = tid + O::W * r;
        v[r] = n < M ? cmul(v[r], cconj(t.chirp[n < M ? n : 0])) : make_float2(0.f, 0.f);   // (chirp: M entries)
    }
    O::fft(v, buf, t.tw, tid);
#pragma unroll
    for (int r = 0; r < O::P; ++r) {
        const int n = tid + O::W * r;
        v[r] = cconj(cmul(buf[lds_pad(n)], t.bhat[n]));       // inverse transform = conj(FFT(conj .)) / L
    }
    O::sync();
    O::fft(v, buf, t.tw, tid);
    const float inv_l = 1.0f / (float)O::N;
    float2 z[O::P];
#pragma unroll
    for (int r = 0; r < O::P; ++r) {
        const int k = tid + O::W * r;
        const float2 y = buf[lds_pad(k < M ? k : 0)];
        z[r] = cmul(make_float2(y.x * inv_l, -(y.y * inv_l)), cconj(t.chirp[k < M ? k : 0]));
    }
    O::sync();
#pragma unroll
    for (int r = 0; r < O::P; ++r) {
        const int k = tid + O::W * r;
        if (k < M) buf[k] = z[r];
    }
    O::sync();
}

template <class O, bool NATIVE>
__device__ __forceinline__ void frame_dft(float2 (&v)[O::P], int M, const frame_tables &t, int tid)
{
    if constexpr (NATIVE) O::fft(v, t.buf, t.tw, tid);
    else bluestein_dft<O>(v, M, t, tid);
}

// ---- one frame at a time -----------------------------------------------------------------------
// The owner's frames of the block's range, one after the other.  The loop bound is uniform over the owner, so every thread
// of a workgroup meets every barrier.  REREAD: see frame_tables::reread.
template <class O, bool NATIVE, bool REREAD>
__device__ __forceinline__ void rfft_frames_body(const float *__restrict__ x, const int64_t *__restrict__ sample_off,
                                                 const int64_t *__restrict__ frame_off, const int *__restrict__ frame_note,
                                                 int64_t total_frames, float2 *__restrict__ S, int ldc, int hop, int M,
                                                 frame_tables tables)
{
    const int tid = O::tid();
    tables.buf += O::first() * O::BUF;
    const int64_t f_begin = (int64_t)blockIdx.x * O::FRAMES;
    for (int i = O::first(); i < O::FRAMES; i += O::STEP) {
        const int64_t f = f_begin + i;
        if (f >= total_frames) break;
        frame_tables t = tables;
        if (REREAD) t.reread();
        float2 v[O::P];
        fetch_frame<O, NATIVE>(v, x, sample_off, frame_off, frame_note, f, hop, M, tid);
        window_frame<O, NATIVE>(v, t.win, M, tid);
        frame_dft<O, NATIVE>(v, M, t, tid);
        split_frame<O, NATIVE>(t.buf, t.twh, M, S + f * (int64_t)ldc, tid);
        O::sync();                                            // the next frame's first pass overwrites buf
    }
}

template <class O, bool NATIVE, bool REREAD>
__device__ __forceinline__ void irfft_frames_body(const float2 *__restrict__ S, int ldc, int64_t total_frames,
                                                  float *__restrict__ frames, int M, frame_tables tables)
{
    const int tid = O::tid();
    tables.buf += O::first() * O::BUF;
    const int64_t f_begin = (int64_t)blockIdx.x * O::FRAMES;
    for (int i = O::first(); i < O::FRAMES; i += O::STEP) {
        const int64_t f = f_begin + i;
        if (f >= total_frames) break;
        frame_tables t = tables;
        if (REREAD) t.reread();
        float2 v[O::P];
        irfft_load<O, NATIVE>(v, S + f * (int64_t)ldc, t.twh, M, tid);
        frame_dft<O, NATIVE>(v, M, t, tid);
        irfft_store<O, NATIVE>(t.buf, t.win, M, reinterpret_cast<float2 *>(frames + f * (int64_t)(2 * M)), tid);
        O::sync();
    }
}

// ---- LDS layouts -------------------------------------------------------------------------------
// wave kernels, native sizes: transform twiddles, half-bin twiddles, four exchange buffers, window (fft_lds_bytes<M>).
// (k_rfft_frames spells the same layout out: it keeps the window as single taps.)
template <int M>
__device__ __forceinline__ frame_tables wave_lds_tables(unsigned char *smem, const float2 *g_tw, const float2 *g_twh, const float *g_win)
{
    float2 *tw = reinterpret_cast<float2 *>(smem);
    float2 *twh = tw + M;
    float2 *bufs = twh + (M / 2 + 1);
    float *win = reinterpret_cast<float *>(bufs + WAVES_PER_BLOCK * fft_cfg<M>::BUF);
    load_tables<M>(tw, twh, win, g_tw, g_twh, g_win);
    return frame_tables{tw, twh, reinterpret_cast<const float2 *>(win), nullptr, nullptr, bufs};
}

// wave kernels, Bluestein: every table in LDS
template <int L> constexpr size_t bluestein_lds_bytes()
{
    return sizeof(float2) * (2 * L + L / 2 + (L / 2 + 2) + WAVES_PER_BLOCK * fft_cfg<L>::BUF) + sizeof(float) * L;
}
template <int L>
__device__ __forceinline__ frame_tables bluestein_lds_tables(unsigned char *smem, int M, const float2 *g_twl, const float2 *g_bhat,
                                                             const float2 *g_chirp, const float2 *g_twh, const float *g_win)
{
    float2 *twl = reinterpret_cast<float2 *>(smem);
    float2 *bhat = twl + L;
    float2 *chirp = bhat + L;
    float2 *twh = chirp + L / 2;
    float2 *bufs = twh + (L / 2 + 2);
    float *win = reinterpret_cast<float *>(bufs + WAVES_PER_BLOCK * fft_cfg<L>::BUF);
    for (int i = threadIdx.x; i < L; i += blockDim.x) { twl[i] = g_twl[i]; bhat[i] = g_bhat[i]; }
    for (int i = threadIdx.x; i < M; i += blockDim.x) chirp[i] = g_chirp[i];
    for (int i = threadIdx.x; i <= M; i += blockDim.x) twh[i] = g_twh[i];
    for (int i = threadIdx.x; i < 2 * M; i += blockDim.x) win[i] = g_win[i];
    __syncthreads();
    return frame_tables{twl, twh, reinterpret_cast<const float2 *>(win), chirp, bhat, bufs};
}

// workgroup kernels: LDS holds the transform's twiddle table and the workgroup's exchange buffer; the other tables are read
// from global memory (L2-resident, every element once per frame and thread, coalesced)
template <int N> constexpr size_t wg_lds_bytes() { return sizeof(float2) * (N + wg_cfg<N>::BUF); }
template <int N>
__device__ __forceinline__ frame_tables wg_lds_tables(unsigned char *smem, const float2 *g_tw, const float2 *g_twh, const float *g_win,
                                                      const float2 *g_chirp = nullptr, const float2 *g_bhat = nullptr)
{
    float2 *tw = reinterpret_cast<float2 *>(smem);
    for (int i = threadIdx.x; i < N; i += WG_THREADS) tw[i] = g_tw[i];
    __syncthreads();
    return frame_tables{tw, g_twh, reinterpret_cast<const float2 *>(g_win), g_chirp, g_bhat, tw + N};
}

// ---- kernels -----------------------------------------------------------------------------------
extern __shared__ __align__(16) unsigned char smem[];

// The hot forward kernel: the shared fetch, transform and one-bin split in a frame loop of its own, two frames in flight.  Its
// LDS carve and its window product are written here rather than taken from wave_lds_tables / window_frame: with either, the
// compiler allocates registers of the 256-, 512- and 768-point instantiations differently, and this kernel's code is
// measured work that a refactor of the others has no reason to move.
// register budget: two frames of M / 64 sample pairs in flight; the 2048-point frame takes the 256-VGPR budget
template <int M, bool NT = false>
__global__ __launch_bounds__(256, M <= 512 ? 4 : 2) void k_rfft_frames(const float *__restrict__ x, const int64_t *__restrict__ sample_off,
                                                     const int64_t *__restrict__ frame_off, const int *__restrict__ frame_note,
                                                     int64_t total_frames, float2 *__restrict__ S, int ldc, int hop,
                                                     const float2 *__restrict__ g_tw, const float2 *__restrict__ g_twh,
                                                     const float *__restrict__ g_win)
{
    using O = wave_owner<M>;
    constexpr int R = O::P;
    float2 *tw = reinterpret_cast<float2 *>(smem);
    float2 *twh = tw + M;
    float2 *bufs = twh + (M / 2 + 1);
    float *win = reinterpret_cast<float *>(bufs + WAVES_PER_BLOCK * fft_cfg<M>::BUF);
    load_tables<M>(tw, twh, win, g_tw, g_twh, g_win);
    const int wave = O::first(), lane = O::tid();
    float2 *buf = bufs + wave * O::BUF;
    const int64_t f_begin = (int64_t)blockIdx.x * FRAMES_PER_BLOCK;
    const bool wide = (ldc & 1) == 0 && ((uintptr_t)S & 15) == 0;      // rows 16-byte aligned: two bins per store

    // raw sample pairs of a frame; the next frame's are in flight during the FFT
    auto fetch = [&](int64_t f, float2 (&raw)[R]) { fetch_frame<O, true>(raw, x, sample_off, frame_off, frame_note, f, hop, M, lane); };
    // One frame: window in place, transform, split, store.  `nf` = the frame whose sample pairs go into the same registers as
    // soon as the transform has consumed them — issued BEFORE this frame's stores.  Loads and stores share one in-order
    // counter (vmcnt): a wave that waits for a load also waits for every store issued before it, and a store completes
    // microseconds after issue.  With two frames in flight and the loads ahead of the stores, the wait for frame i + 1's
    // samples covers only stores that are two frames old — the kernel then runs at the larger of its load / compute time
    // and its store time instead of their sum (0.33 -> 0.2x ms on the 1024-note batch).
    auto frame = [&](int64_t f, float2 (&v)[R], int64_t nf) {
#pragma unroll
        for (int r = 0; r < R; ++r) {                 // (window_frame, deferred to here)
            const int m = lane + WAVE * r;
            v[r] = make_float2(v[r].x * win[2 * m], v[r].y * win[2 * m + 1]);
        }
        O::fft(v, buf, tw, lane);
        if (nf >= 0) fetch(nf, v);

        float2 *row = S + f * (int64_t)ldc;
        auto split = [&](int k) { return rfft_bin<true>(buf, twh, M, k); };
        if (wide) {
            // The split reads stay conflict-free (bin k = lane + 64 r per lane); neighbouring lanes then trade one bin each
            // (a 2 x 2 transpose over two r values, one quad-permute DPP move per dword), so that an even lane holds bins
            // (k, k + 1) of row segment r and the odd lane beside it bins (k - 1, k) of segment r + 1: every lane issues
            // 16-byte stores, on 128-byte aligned rows.
            const bool odd = lane & 1;
#pragma unroll
            for (int r = 0; r < R; r += 2) {
                const float2 xa = split(lane + WAVE * r), xb = split(lane + WAVE * (r + 1));
                const float2 send = odd ? xa : xb;
                float2 recv;
                recv.x = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(send.x), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
                recv.y = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(send.y), 0xB1, 0xF, 0xF, false));
                const float4 o = odd ? make_float4(recv.x, recv.y, xb.x, xb.y) : make_float4(xa.x, xa.y, recv.x, recv.y);
                const int k0 = odd ? lane - 1 + WAVE * (r + 1) : lane + WAVE * r;
                typedef float v4f_t __attribute__((ext_vector_type(4)));
                if (NT) __builtin_nontemporal_store(v4f_t{o.x, o.y, o.z, o.w}, reinterpret_cast<v4f_t *>(row + k0));   // write-once rows: not kept in L2
                else *reinterpret_cast<float4 *>(row + k0) = o;
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int k = lane + WAVE * r;
                row[k] = split(k);
            }
        }
        if (lane == 0) row[M] = rfft_last_bin(buf);
        wave_lds_sync();
    };

    // frames f_begin + wave + 4 q of this wave, q = 0 .. FRAMES_PER_BLOCK / 4 - 1, two at a time in registers A and B
    constexpr int PER_WAVE = FRAMES_PER_BLOCK / WAVES_PER_BLOCK;
    static_assert(PER_WAVE % 2 == 0, "frames per wave are processed in pairs");
    auto frame_id = [&](int q) -> int64_t {
        const int64_t f = f_begin + wave + (int64_t)WAVES_PER_BLOCK * q;
        return (q < PER_WAVE && f < total_frames) ? f : -1;
    };
    float2 A[R], B[R];
    if (frame_id(0) >= 0) fetch(frame_id(0), A);
    if (frame_id(1) >= 0) fetch(frame_id(1), B);
    for (int q = 0; q < PER_WAVE; q += 2) {
        if (frame_id(q) < 0) break;                   // wave-uniform
        frame(frame_id(q), A, frame_id(q + 2));
        if (frame_id(q + 1) < 0) break;
        frame(frame_id(q + 1), B, frame_id(q + 3));
    }
}

// S row -> windowed time frame.  The loop of irfft_frames_body with the input stage written in place: taken through a function,
// the compiler orders the operands of the 6- and 12-point first-pass sums (n_fft 768 / 1536) differently, and a sum of two NaNs takes
// the sign of its first operand — frames that hold a NaN would come out with other NaN sign bits than they had.
template <int M>
__global__ __launch_bounds__(256) void k_irfft_frames(const float2 *__restrict__ S, int ldc, int64_t total_frames,
                                                      float *__restrict__ frames,
                                                      const float2 *__restrict__ g_tw, const float2 *__restrict__ g_twh, const float *__restrict__ g_win)
{
    using O = wave_owner<M>;
    frame_tables t = wave_lds_tables<M>(smem, g_tw, g_twh, g_win);
    const int lane = O::tid();
    t.buf += O::first() * O::BUF;
    const int64_t f_begin = (int64_t)blockIdx.x * O::FRAMES;
    for (int i = O::first(); i < O::FRAMES; i += O::STEP) {
        const int64_t f = f_begin + i;
        if (f >= total_frames) break;
        const float2 *row = S + f * (int64_t)ldc;
        float2 v[O::P];
#pragma unroll
        for (int r = 0; r < O::P; ++r) {                      // irfft_load<O, true>, in place: see above
            const int k = lane + WAVE * r;
            float2 xk = row[k], xm = row[M - k];
            if (k == 0) { xk.y = 0.f; xm.y = 0.f; }
            v[r] = irfft_pre(xk, xm, half_twiddle<true, true>(t.twh, M, k));
        }
        frame_dft<O, true>(v, M, t, lane);
        irfft_store<O, true>(t.buf, t.win, M, reinterpret_cast<float2 *>(frames + f * (int64_t)(2 * M)), lane);
        O::sync();
    }
}

// n_fft = 2 M = 4096, the workgroup's native size
template <int M>
__global__ __launch_bounds__(256) void k_rfft_frames_wg(const float *__restrict__ x, const int64_t *__restrict__ sample_off,
                                                        const int64_t *__restrict__ frame_off, const int *__restrict__ frame_note,
                                                        int64_t total_frames, float2 *__restrict__ S, int ldc, int hop,
                                                        const float2 *__restrict__ g_tw, const float2 *__restrict__ g_twh, const float *__restrict__ g_win)
{
    rfft_frames_body<wg_owner<M>, true, false>(x, sample_off, frame_off, frame_note, total_frames, S, ldc, hop, M,
        wg_lds_tables<M>(smem, g_tw, g_twh, g_win));
}

template <int M>
__global__ __launch_bounds__(256) void k_irfft_frames_wg(const float2 *__restrict__ S, int ldc, int64_t total_frames,
                                                         float *__restrict__ frames,
                                                         const float2 *__restrict__ g_tw, const float2 *__restrict__ g_twh, const float *__restrict__ g_win)
{
    irfft_frames_body<wg_owner<M>, true, false>(S, ldc, total_frames, frames, M,
        wg_lds_tables<M>(smem, g_tw, g_twh, g_win));
}

// any even n_fft up to 2048 without a radix plan: L = 256 .. 2048
template <int L>
__global__ __launch_bounds__(256) void k_rfft_bluestein(const float *__restrict__ x, const int64_t *__restrict__ sample_off,
                                                        const int64_t *__restrict__ frame_off, const int *__restrict__ frame_note,
                                                        int64_t total_frames, float2 *__restrict__ S, int ldc, int hop,
                                                        int M, const float2 *__restrict__ g_twl, const float2 *__restrict__ g_bhat,
                                                        const float2 *__restrict__ g_chirp, const float2 *__restrict__ g_twh, const float *__restrict__ g_win)
{
    rfft_frames_body<wave_owner<L>, false, false>(x, sample_off, frame_off, frame_note, total_frames, S, ldc, hop, M,
        bluestein_lds_tables<L>(smem, M, g_twl, g_bhat, g_chirp, g_twh, g_win));
}

template <int L>
__global__ __launch_bounds__(256) void k_irfft_bluestein(const float2 *__restrict__ S, int ldc, int64_t total_frames,
                                                         float *__restrict__ frames,
                                                         int M, const float2 *__restrict__ g_twl, const float2 *__restrict__ g_bhat,
                                                         const float2 *__restrict__ g_chirp, const float2 *__restrict__ g_twh, const float *__restrict__ g_win)
{
    irfft_frames_body<wave_owner<L>, false, false>(S, ldc, total_frames, frames, M,
        bluestein_lds_tables<L>(smem, M, g_twl, g_bhat, g_chirp, g_twh, g_win));
}

// every even n_fft in [2052, 4094]: L = 4096
template <int L>
__global__ __launch_bounds__(256) void k_rfft_bluestein_wg(const float *__restrict__ x, const int64_t *__restrict__ sample_off,
                                                           const int64_t *__restrict__ frame_off, const int *__restrict__ frame_note,
                                                           int64_t total_frames, float2 *__restrict__ S, int ldc, int hop,
                                                           int M, const float2 *__restrict__ g_twl, const float2 *__restrict__ g_bhat,
                                                           const float2 *__restrict__ g_chirp, const float2 *__restrict__ g_twh, const float *__restrict__ g_win)
{
    rfft_frames_body<wg_owner<L>, false, true>(x, sample_off, frame_off, frame_note, total_frames, S, ldc, hop, M,
        wg_lds_tables<L>(smem, g_twl, g_twh, g_win, g_chirp, g_bhat));
}

template <int L>
__global__ __launch_bounds__(256) void k_irfft_bluestein_wg(const float2 *__restrict__ S, int ldc, int64_t total_frames,
                                                            float *__restrict__ frames,
                                                            int M, const float2 *__restrict__ g_twl, const float2 *__restrict__ g_bhat,
                                                            const float2 *__restrict__ g_chirp, const float2 *__restrict__ g_twh, const float *__restrict__ g_win)
{
    irfft_frames_body<wg_owner<L>, false, true>(S, ldc, total_frames, frames, M,
        wg_lds_tables<L>(smem, g_twl, g_twh, g_win, g_chirp, g_bhat));
}

// y[i] = (sum over covering frames, ascending, of frames[fr][p - fr*hop]) / (same sum of w^2), fp32,
// p = i + n_fft/2; samples past hop*(T-1) are the zero padding of istft.  Optional per-note scale.
__global__ __launch_bounds__(256) void k_ola_gather(const float *__restrict__ frames, const float *__restrict__ win_sq,
                                                    const int64_t *__restrict__ sample_off, const int64_t *__restrict__ frame_off,
                                                    int n_notes, int64_t total_samples, int n_fft, int hop,
                                                    float *__restrict__ y, const float *__restrict__ divisor)
{
    const sample_tile<> t(sample_off, n_notes, total_samples);
    if (!t.live) return;
    const int64_t g = t.g;

    auto body = [&](int note) {
        const int64_t i = g - sample_off[note];
        const int64_t fbase = frame_off[note];
        const int64_t T = frame_off[note + 1] - fbase;
        float out = 0.f;
        if (i < (int64_t)hop * (T - 1)) {
            const int64_t p = i + n_fft / 2;
            int64_t lo = p - n_fft + 1;
            lo = lo <= 0 ? 0 : (lo + hop - 1) / hop;
            int64_t hi = p / hop;
            if (hi > T - 1) hi = T - 1;
            float acc = 0.f, ws = 0.f;
            for (int64_t fr = lo; fr <= hi; ++fr) {
                int j = (int)(p - fr * hop);
                acc += frames[(fbase + fr) * n_fft + j];
                ws += win_sq[j];
            }
            if (ws > 1e-9f) acc /= ws;
            out = acc;
            if (divisor) out = out / divisor[note];
        }
        y[g] = out;
    };
    if (t.uniform()) body(t.lo);
    else body(t.note(sample_off));
}

// ---------------------------------------------------------------------------------------------
__global__ void k_frame_note(const int64_t *__restrict__ frame_off, int n_notes, int64_t total_frames, int *__restrict__ frame_note)
{
    int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < total_frames) frame_note[f] = csr_find(frame_off, n_notes, f);
}

int launch_frame_note(goofer_ctx *ctx, const int64_t *frame_off, int n_notes, int64_t total_frames, int *frame_note, hipStream_t st)
{
    if (total_frames <= 0) return GOOFER_OK;
    hipLaunchKernelGGL(k_frame_note, dim3((unsigned)((total_frames + 255) / 256)), dim3(256), 0, st, frame_off, n_notes,
                       total_frames, frame_note);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

// ---- dispatch ----------------------------------------------------------------------------------
// The kernels and the LDS of one (owner, form).  (k_rfft_frames: the spectrum rows — 80 % of the kernel's bytes, written
// once — leave as non-temporal stores: 0.40 -> 0.51 of the HBM peak.)
template <class O, bool NATIVE> struct transform {
    static constexpr bool wave = O::W == WAVE;
    static constexpr auto rfft()
    {
        if constexpr (wave && NATIVE) return k_rfft_frames<O::N, true>;
        else if constexpr (wave) return k_rfft_bluestein<O::N>;
        else if constexpr (NATIVE) return k_rfft_frames_wg<O::N>;
        else return k_rfft_bluestein_wg<O::N>;
    }
    static constexpr auto irfft()
    {
        if constexpr (wave && NATIVE) return k_irfft_frames<O::N>;
        else if constexpr (wave) return k_irfft_bluestein<O::N>;
        else if constexpr (NATIVE) return k_irfft_frames_wg<O::N>;
        else return k_irfft_bluestein_wg<O::N>;
    }
    static constexpr size_t lds = !wave ? wg_lds_bytes<O::N>() : NATIVE ? fft_lds_bytes<O::N>() : bluestein_lds_bytes<O::N>();

    // `head...`: the kernel's arguments in front of its tables
    template <typename K, typename... A> static int launch(goofer_ctx *ctx, K kernel, int64_t total_frames, hipStream_t st, A... head)
    {
        const goofer_plan_t &p = ctx->plan;
        const unsigned blocks = (unsigned)((total_frames + O::FRAMES - 1) / O::FRAMES);
        if (lds > 64 * 1024)
            if (int rc = kernel_allow_max_lds(ctx, (const void *)kernel)) return rc;
        if constexpr (NATIVE) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, st, head..., p.tw_full, p.tw_half, p.window);
        else hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, st, head..., p.n_fft / 2, p.bl_tw, p.bl_bhat, p.bl_chirp, p.bl_twh, p.window);
        LAUNCH_CHECK(ctx);
        return GOOFER_OK;
    }
};

// plan -> instantiation, for both directions.  Above n_fft 2048 the workgroup owns the frame: 4096 is its native size, every
// other even n_fft in [2052, 4094] Bluestein at L = 4096.  Up to 2048 the wave does: Bluestein where the plan has a length,
// else one of the native sizes.
template <typename F> static int with_transform(goofer_ctx *ctx, F &&f)
{
    const goofer_plan_t &p = ctx->plan;
    if (p.n_fft > 2048) {
        if (p.bl_L == 4096) return f(transform<wg_owner<4096>, false>{});
        if (p.n_fft == 4096 && p.bl_L == 0) return f(transform<wg_owner<2048>, true>{});
        return goofer_fail(ctx, GOOFER_EINVAL, "unsupported n_fft %d (Bluestein length %d)", p.n_fft, p.bl_L);
    }
    switch (p.bl_L) {
    case 0: break;
    case 256: return f(transform<wave_owner<256>, false>{});
    case 512: return f(transform<wave_owner<512>, false>{});
    case 1024: return f(transform<wave_owner<1024>, false>{});
    case 2048: return f(transform<wave_owner<2048>, false>{});
    default: return goofer_fail(ctx, GOOFER_EINVAL, "bad Bluestein length %d", p.bl_L);
    }
    switch (p.n_fft) {
    case 512: return f(transform<wave_owner<256>, true>{});
    case 1024: return f(transform<wave_owner<512>, true>{});
    case 2048: return f(transform<wave_owner<1024>, true>{});
    case 768: return f(transform<wave_owner<384>, true>{});
    case 1536: return f(transform<wave_owner<768>, true>{});
    }
    return goofer_fail(ctx, GOOFER_EINVAL, "unsupported n_fft %d", p.n_fft);
}

int launch_rfft_frames_mapped(goofer_ctx *ctx, const float *x, const int64_t *sample_off, const int64_t *frame_off,
                              const int *frame_note, int64_t total_frames, float2 *S, int ldc, hipStream_t st)
{
    if (total_frames <= 0) return GOOFER_OK;
    return with_transform(ctx, [&](auto t) {
        return t.launch(ctx, t.rfft(), total_frames, st, x, sample_off, frame_off, frame_note, total_frames, S, ldc, ctx->plan.hop);
    });
}

int launch_irfft_frames(goofer_ctx *ctx, const float2 *S, int ldc, int64_t total_frames, float *frames, hipStream_t st)
{
    if (total_frames <= 0) return GOOFER_OK;
    return with_transform(ctx, [&](auto t) { return t.launch(ctx, t.irfft(), total_frames, st, S, ldc, total_frames, frames); });
}

int launch_ola_gather(goofer_ctx *ctx, const float *frames, const int64_t *sample_off, const int64_t *frame_off,
                      int n_notes, int64_t total_samples, float *y, const float *inv_scale, hipStream_t st)
{
    const goofer_plan_t &p = ctx->plan;
    return launch_per_sample(ctx, k_ola_gather, total_samples, 256, 0, st, frames, p.win_sq, sample_off, frame_off, n_notes, total_samples,
                             p.n_fft, p.hop, y, inv_scale);
}
