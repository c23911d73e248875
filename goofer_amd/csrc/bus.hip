// The stereo bus on the device (gfx950): finished tracks — each wherever its own render left it in HBM — given their pan gains
// and summed onto one planar L | R time line, the mixer that follows a `wavtool`.  The definition is in include/goofer_hip.h
// ("stereo bus"); the host half, goofer_host_bus_plan (planner.hip), checks the records and lists per tile of the bus the tracks
// that reach it.
//
// k_phrase_mix's shape with two accumulators: the bus is cut into tiles of GOOFER_BUS_TILE samples, one 256-thread workgroup
// per tile, eight consecutive samples per thread held in registers for both channels; the workgroup walks the tile's tracks in
// ascending index (the order of the sum is part of the contract), loads each source sample once and stores each bus sample
// once.  The track index of the walk is wave-uniform, so a track's record is scalar loads.  Per wave and track one of two bodies
// runs, both with the same arithmetic per sample (the same bits whichever runs):
//   inside   the wave's 512 samples lie inside the track: 16-byte loads where a wave-uniform test finds the source aligned (a lane
//            is 32 bytes on: the same answer in every lane), eight floats as they lie elsewhere
//   edge     the track starts or ends in the wave: each sample guarded
// No atomics, no LDS, no scratch, no barrier: 4 sum len + 8 N bytes move, and nothing else does.
#include "common.h"

#define BUS_SPT 8                     // consecutive bus samples per thread
static_assert(GOOFER_BUS_TILE == 256 * BUS_SPT, "one workgroup of 256 threads per tile");
static_assert(sizeof(goofer_bus_track) == 32, "the record the Python side mirrors");

// acc[0 .. 8) of one channel to out[t0 ..): 16-byte stores where `vec` (the channel's base is 16-byte aligned and the eight lie
// inside the bus)
__device__ __forceinline__ void bus_store(float *__restrict__ out, int64_t t0, int64_t total_out, bool vec, const float (&acc)[BUS_SPT])
{
    if (vec) {
        *reinterpret_cast<float4 *>(out + t0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4 *>(out + t0 + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
#pragma unroll
        for (int e = 0; e < BUS_SPT; ++e)
            if (t0 + e < total_out) out[t0 + e] = acc[e];
    }
}

__global__ __launch_bounds__(256) void k_bus_mix(const goofer_bus_track *__restrict__ tracks, const int64_t *__restrict__ tile_off,
                                                 const int32_t *__restrict__ tile_tracks, int64_t total_out, float *__restrict__ out)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * GOOFER_BUS_TILE + wave * (WAVE * BUS_SPT);     // the wave's first bus sample
    if (w0 >= total_out) return;                               // (no barrier in this kernel)
    const int64_t t0 = w0 + lane * BUS_SPT;
    float accl[BUS_SPT], accr[BUS_SPT];
#pragma unroll
    for (int e = 0; e < BUS_SPT; ++e) accl[e] = accr[e] = 0.0f;

    const int64_t j1 = tile_off[blockIdx.x + 1];
    for (int64_t j = tile_off[blockIdx.x]; j < j1; ++j) {
        const int i = __builtin_amdgcn_readfirstlane(tile_tracks[j]);
        const goofer_bus_track *__restrict__ r = tracks + i;
        const float *__restrict__ xs = r->x;
        const int64_t len = r->len, uw = w0 - r->start;        // u of the wave's first sample: x_i[u] sounds at w0
        const float gl = r->gl, gr = r->gr;
        if (uw >= len || uw + WAVE * BUS_SPT <= 0) continue;   // the track does not reach this wave
        const int64_t u0 = uw + lane * BUS_SPT;
        if (uw >= 0 && uw + WAVE * BUS_SPT <= len) {           // the wave lies inside the track
            float v[BUS_SPT];
            if ((((uintptr_t)(xs + uw)) & 15) == 0) {
                const float4 q0 = *reinterpret_cast<const float4 *>(xs + u0), q1 = *reinterpret_cast<const float4 *>(xs + u0 + 4);
                v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
            } else {
#pragma unroll
                for (int e = 0; e < BUS_SPT; ++e) v[e] = xs[u0 + e];
            }
#pragma unroll
            for (int e = 0; e < BUS_SPT; ++e) {
                accl[e] = accl[e] + gl * v[e];
                accr[e] = accr[e] + gr * v[e];
            }
        } else {                                               // the track starts or ends in this wave
#pragma unroll
            for (int e = 0; e < BUS_SPT; ++e) {
                const int64_t u = u0 + e;
                const bool on = u >= 0 && u < len;
                const float xv = on ? xs[u] : 0.0f;
                accl[e] = on ? accl[e] + gl * xv : accl[e];
                accr[e] = on ? accr[e] + gr * xv : accr[e];
            }
        }
    }

    const bool whole = t0 + BUS_SPT <= total_out;
    float *__restrict__ outr = out + total_out;
    bus_store(out, t0, total_out, whole && (((uintptr_t)out) & 15) == 0, accl);
    bus_store(outr, t0, total_out, whole && (((uintptr_t)outr) & 15) == 0, accr);
}

extern "C" int goofer_bus_mix(goofer_ctx *ctx, const goofer_bus_track *tracks, int n, const int64_t *tile_off, const int32_t *tile_tracks,
                              int64_t total_out, float *out, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (n < 0 || total_out < 0)
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_bus_mix: negative count (%d tracks, %lld samples)", n, (long long)total_out);
    if (total_out == 0) return GOOFER_OK;
    if (!tile_off || !out || (n > 0 && (!tracks || !tile_tracks))) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_bus_mix: null pointer");
    if (((uintptr_t)out | (uintptr_t)tile_tracks) & 3 || ((uintptr_t)tracks | (uintptr_t)tile_off) & 7)
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_bus_mix: out and tile_tracks must be 4-byte aligned, tracks and tile_off 8-byte aligned");
    const int64_t tiles = (total_out + GOOFER_BUS_TILE - 1) / GOOFER_BUS_TILE;
    if (tiles >= ((int64_t)1 << 31)) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_bus_mix: a bus of %lld samples", (long long)total_out);
    hipLaunchKernelGGL(k_bus_mix, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, tracks, tile_off, tile_tracks, total_out, out);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}
