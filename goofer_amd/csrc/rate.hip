// Output-rate conversion on the device (gfx950): finished audio — the notes of a batch back to back, or a phrase's track — from
// the voicebank's rate to another one by a polyphase Kaiser-windowed sinc, over a ragged batch in one launch.  The definition
// (geometry, table, the order of the sum) is in include/goofer_hip.h; the host half, goofer_host_rate_plan (planner.hip), makes
// the table taps[L][2H] and the output CSR.
//
// One thread per output sample, 64 consecutive samples of the concatenated output axis per wave.  Output k of a signal reads
// row p = (k M) mod L of the table and the 2H input samples around q = (k M) div L: both are contiguous for the thread, so a lane
// walks two float arrays four elements a load, one fp32 multiply and one fp32 add per tap in ascending j (the contract).  Taps
// that fall before or behind the signal are left out by clamping the lane's column range, which is the definition's own guard: no
// padding, no read outside a signal, the same arithmetic at an edge and inside.
//
// The lanes of a wave are on 64 different rows (p steps by M mod L) and on overlapping input windows (q steps by M / L).  The
// input comes through L1 (a wave's 16-byte loads span three or four cache lines).  The rows do not: 64 lanes on 64 cache lines
// per load is what the vector cache does slowest, so a workgroup of 1024 threads first copies the table into LDS — rows padded to
// an odd number of 16-byte slots, which puts the rows of a ds_read_b128 lane group on different banks — and reads its rows there
// (41 KB for 44.1 -> 48 kHz, two workgroups per CU; 114 KB for 44.1 -> 8 kHz, one).  A table that does not fit in 160 KiB is read
// from global memory by workgroups of 256 threads: the same code on another pointer (option "rate_lds" 0 takes that path for
// every table: the A/B, and the same bits).
//
// The number of output samples is on the device only (out_off[n]): the grid is fixed and walks the wave tiles with a stride, so
// the call stays asynchronous.  A wave finds the signal of its first sample cooperatively (wave_find); when its 64 samples lie in
// one signal (nearly always) everything per signal is a scalar load, and (q, p) of the tile's first sample is one division —
// 32-bit where k M fits, as it does in the first 2^32 / M outputs of a signal — from which a lane steps by lane * M.  No atomics,
// no scratch; every output sample is stored once.
#include "ragged.h"

#define RATE_PASS (512 * 1024)        // output samples per pass of the grid: 512 workgroups of 1024 threads, or 2048 of 256

struct __attribute__((packed, aligned(4))) rate_f4 { float v[4]; };   // four floats at 4-byte alignment: one 16-byte load

// four consecutive floats: of x (global, any alignment), of a table row in LDS (16-byte aligned: ds_read_b128)
__device__ __forceinline__ void rate_load4(const float *__restrict__ p, float (&o)[4])
{
    const rate_f4 q = *reinterpret_cast<const rate_f4 *>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = q.v[e];
}
__device__ __forceinline__ void rate_load4_aligned(const float *__restrict__ p, float (&o)[4])
{
    const float4 q = *reinterpret_cast<const float4 *>(p);
    o[0] = q.x, o[1] = q.y, o[2] = q.z, o[3] = q.w;
}

// WS: floats from one row of the table to the next where the kernel reads it (LDS: padded; global: 2H)
// Two workgroups of 1024 threads per CU are eight waves per SIMD, 64 VGPRs at most: asked for, it compiles to 62 without scratch
// (65 without the request).
template <bool LDS>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_rate_convert(const float *__restrict__ x, const int64_t *__restrict__ in_off, int n, int L, int M, int H, int WS,
                    const float *__restrict__ taps, const int64_t *__restrict__ out_off, float *__restrict__ out)
{
    extern __shared__ __align__(16) float s_taps[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int W = 2 * H;
    const int64_t total = out_off[n];
    if ((int64_t)blockIdx.x * blockDim.x >= total) return;              // none of the workgroup's waves has a tile (before the barrier)
    if (LDS) {
        for (int r = wave; r < L; r += waves)
            for (int c = lane; c < W; c += WAVE) s_taps[r * WS + c] = taps[r * W + c];
        __syncthreads();
    }
    const float *__restrict__ table = LDS ? s_taps : taps;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t w0 = ((int64_t)blockIdx.x * waves + wave) * WAVE; w0 < total; w0 += stride) {
        const int lo = __builtin_amdgcn_readfirstlane(wave_find(n, w0, lane, [&](int k) { return out_off[k]; }));
        const int64_t g = w0 + lane;
        // signal i owns output g
        auto body = [&](int i) {
            const int64_t o0 = out_off[i], b0 = in_off[i];
            const int64_t len = in_off[i + 1] - b0;                    // < 2^31
            const int64_t kb = w0 > o0 ? w0 - o0 : 0;                   // the signal's first output in this tile
            const uint32_t dk = (uint32_t)(g - o0 - kb);                // < 64
            const uint64_t km = (uint64_t)kb * (uint64_t)M;
            uint64_t qb;
            uint32_t pb;
            if ((km >> 32) == 0) {
                qb = (uint32_t)km / (uint32_t)L;
                pb = (uint32_t)km % (uint32_t)L;
            } else {
                qb = km / (uint64_t)L;
                pb = (uint32_t)(km % (uint64_t)L);
            }
            const uint32_t s = pb + dk * (uint32_t)M;                   // < L + 63 M
            const int64_t q = (int64_t)(qb + s / (uint32_t)L);          // < len: k < m = ceil(len L / M)
            const int p = (int)(s % (uint32_t)L);
            // columns c = j + H - 1 of row p with 0 <= q + j < len
            const int64_t first = (int64_t)(H - 1) - q, last = len - q + (H - 1);
            const int c0 = first > 0 ? (int)first : 0, c1 = last < W ? (int)last : W;
            const float *__restrict__ h = table + p * WS;               // (at most 1024 rows of 2 * 32 768 floats: an int)
            const float *__restrict__ xs = x + (b0 + q - (H - 1));      // xs[c] = x_i[q + j]; read for c0 <= c < c1 only
            float acc = 0.0f;
            int c = c0;
            for (; c < c1 && (c & 3); ++c) acc = acc + h[c] * xs[c];    // (an edge: up to the row's next 16-byte slot)
            for (; c + 16 <= c1; c += 16) {                             // eight loads in flight, then the sixteen taps in order
                float hv[4][4], xv[4][4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    if (LDS) rate_load4_aligned(h + c + 4 * b, hv[b]); else rate_load4(h + c + 4 * b, hv[b]);
                    rate_load4(xs + c + 4 * b, xv[b]);
                }
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = acc + hv[b][e] * xv[b][e];
            }
            for (; c + 4 <= c1; c += 4) {
                float hv[4], xv[4];
                if (LDS) rate_load4_aligned(h + c, hv); else rate_load4(h + c, hv);
                rate_load4(xs + c, xv);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = acc + hv[e] * xv[e];
            }
            for (; c < c1; ++c) acc = acc + h[c] * xs[c];
            out[g] = acc;
        };
        const int64_t gl = w0 + (WAVE - 1) < total ? w0 + (WAVE - 1) : total - 1;
        if (out_off[lo + 1] > gl) {                                     // one signal for the wave: its numbers are scalars
            if (g < total) body(lo);
        } else if (g < total) {
            int i = lo;
            while (out_off[i + 1] <= g) ++i;
            body(i);
        }
    }
}

extern "C" int goofer_rate_convert(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int L, int M, int H, const float *taps,
                                   const int64_t *out_off, float *out, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (n < 0) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_rate_convert: negative count (%d signals)", n);
    if (L < 1 || M < 1 || L > GOOFER_RATE_MAX_PHASES || M > GOOFER_RATE_MAX_PHASES || L == M ||
        H != (GOOFER_RATE_ZEROS * (L > M ? L : M) + L - 1) / L)
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_rate_convert: L = %d, M = %d, H = %d is not a geometry of goofer_host_rate_plan", L, M, H);
    if (n == 0) return GOOFER_OK;
    if (!x || !in_off || !taps || !out_off || !out) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_rate_convert: null pointer");
    if (((uintptr_t)x | (uintptr_t)taps | (uintptr_t)out) & 3 || ((uintptr_t)in_off | (uintptr_t)out_off) & 7)
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_rate_convert: x, taps and out must be 4-byte aligned, in_off and out_off 8-byte aligned");
    // the table in LDS: rows of an odd number of 16-byte slots
    const int W = 2 * H, WS = 4 * (((W + 3) / 4) | 1);
    const int64_t lds = (int64_t)L * WS * 4;
    if (ctx->rate_lds && lds <= 160 * 1024) {
        if (lds > 64 * 1024)
            if (int rc = kernel_allow_max_lds(ctx, (const void *)k_rate_convert<true>)) return rc;
        hipLaunchKernelGGL(k_rate_convert<true>, dim3(RATE_PASS / 1024), dim3(1024), (size_t)lds, (hipStream_t)stream, x, in_off, n, L, M, H, WS,
                           taps, out_off, out);
    } else {
        hipLaunchKernelGGL(k_rate_convert<false>, dim3(RATE_PASS / 256), dim3(256), 0, (hipStream_t)stream, x, in_off, n, L, M, H, W, taps,
                           out_off, out);
    }
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}
