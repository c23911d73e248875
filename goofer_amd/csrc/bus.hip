// The stereo bus on the device (gfx950): finished tracks — each wherever its own render left it in HBM — given their pan gains
// and summed onto one planar L | R time line, the mixer that follows a `wavtool`.  The definition is in include/goofer_hip.h
// ("stereo bus"); the host half, goofer_host_bus_plan (planner.hip), checks the records and lists per tile of the bus the tracks
// that reach it.
//
// A gather-sum over the tiles of the bus, on the walk of tile_mix.h, with an accumulator per channel: each source sample is loaded
// once and each bus sample stored once.  The track index of the walk is wave-uniform, so a track's record is scalar loads.  Per
// wave and track one of two bodies runs, both with the same arithmetic per sample (the same bits whichever runs):
//   inside   the wave's 512 samples lie inside the track: 16-byte loads where a wave-uniform test finds the source aligned (a lane
//            is 32 bytes on: the same answer in every lane), eight floats as they lie elsewhere
//   edge     the track starts or ends in the wave: each sample guarded
// No atomics, no LDS, no scratch, no barrier: 4 sum len + 8 N bytes move, and nothing else does.
#include "tile_mix.h"

static_assert(sizeof(goofer_bus_track) == 32, "the record the Python side mirrors");

__global__ __launch_bounds__(256) void k_bus_mix(const goofer_bus_track *__restrict__ tracks, const int64_t *__restrict__ tile_off,
                                                 const int32_t *__restrict__ tile_tracks, int64_t total_out, float *__restrict__ out)
{
    int lane;
    const int64_t w0 = mix_wave_first(lane);                   // the wave's first bus sample
    if (w0 >= total_out) return;
    const int64_t t0 = w0 + lane * MIX_SPT;
    float accl[MIX_SPT], accr[MIX_SPT];
#pragma unroll
    for (int e = 0; e < MIX_SPT; ++e) accl[e] = accr[e] = 0.0f;

    const int64_t j1 = tile_off[blockIdx.x + 1];
    for (int64_t j = tile_off[blockIdx.x]; j < j1; ++j) {
        const int i = mix_entry(tile_tracks, j);
        const goofer_bus_track *__restrict__ r = tracks + i;
        const float *__restrict__ xs = r->x;
        const int64_t len = r->len, uw = w0 - r->start;        // u of the wave's first sample: x_i[u] sounds at w0
        const float gl = r->gl, gr = r->gr;
        if (mix_off(uw, len)) continue;
        const int64_t u0 = uw + lane * MIX_SPT;
        if (MIX_INSIDE(uw, len)) {
            float v[MIX_SPT];
            if ((((uintptr_t)(xs + uw)) & 15) == 0) mix_load8_vec(xs, u0, v);
            else mix_load8_any(xs, u0, v);
#pragma unroll
            for (int e = 0; e < MIX_SPT; ++e) {
                accl[e] = accl[e] + gl * v[e];
                accr[e] = accr[e] + gr * v[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < MIX_SPT; ++e) {
                const int64_t u = u0 + e;
                const bool on = u >= 0 && u < len;
                const float xv = on ? xs[u] : 0.0f;
                accl[e] = on ? accl[e] + gl * xv : accl[e];
                accr[e] = on ? accr[e] + gr * xv : accr[e];
            }
        }
    }

    const bool whole = t0 + MIX_SPT <= total_out;
    float *__restrict__ outr = out + total_out;
    mix_store8(out, t0, total_out, whole && (((uintptr_t)out) & 15) == 0, accl);
    mix_store8(outr, t0, total_out, whole && (((uintptr_t)outr) & 15) == 0, accr);
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
    const unsigned tiles = mix_grid(total_out);
    if (!tiles) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_bus_mix: a bus of %lld samples", (long long)total_out);
    hipLaunchKernelGGL(k_bus_mix, dim3(tiles), dim3(256), 0, (hipStream_t)stream, tracks, tile_off, tile_tracks, total_out, out);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}
