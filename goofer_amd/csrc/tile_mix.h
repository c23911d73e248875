// The tile walk of the gather-sum mixers, written once (gfx950).
//
// A mix sums ragged sources — each placed anywhere on a time line — onto that line without atomics: the line is cut into tiles
// of GOOFER_MIX_TILE samples, one 256-thread workgroup per tile, MIX_SPT consecutive samples per thread held in registers.  The
// host planner (mix_cover, planner.hip) lists per tile the sources that reach it, in ascending index; the workgroup walks that
// list (the order of the sum is part of the contract) and stores each sample once.  The source index of the walk is
// wave-uniform, so a source's record is scalar loads.  No atomics, no LDS, no scratch, no barrier.
//
//   k_phrase_mix (phrase.hip)   one channel; per source seven knots and a gain per sample
//   k_bus_mix (bus.hip)         two channels; per source two constant gains
//
// What is here: the position of a thread, an entry of the tile's list, the reach of a source in a wave, the load and the store
// of a thread's eight samples, and the launchers' tile count.  What a source contributes per sample stays with its kernel.
//
// u, the index into a source of a wave's first sample, has two types, and the reach tests take either.  The phrase clamps it into
// an int: a note is at most 2^24 samples, a clamped u is out of every note's reach, and its gain converts u to float per sample
// (one v_cvt_f32_i32; from an int64 it is a sequence).  A bus track's length is any int64, so there u stays one.
#pragma once
#include "common.h"

#define MIX_SPT 8                     // consecutive samples per thread
#define MIX_WAVE (WAVE * MIX_SPT)     // samples of a wave
static_assert(GOOFER_MIX_TILE == 256 * MIX_SPT, "one workgroup of 256 threads per tile");

// The wave's first sample on the time line, and the thread's lane; the thread's own first sample is w0 + lane * MIX_SPT.  A wave
// whose w0 is not below the line's length has nothing to do and returns (no barrier in these kernels).  That test stays with
// the kernel, like the frame walkers' (ola_walk.h, "run range").
__device__ __forceinline__ int64_t mix_wave_first(int &lane)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    lane = threadIdx.x & 63;
    return (int64_t)blockIdx.x * GOOFER_MIX_TILE + wave * MIX_WAVE;
}

// Entry j of the tile list, made wave-uniform.  A workgroup walks tile_list[tile_off[b] .. tile_off[b + 1]) of its tile b in the
// list's order; the two-line loop stays with the kernel: as a function that takes a body per entry k_phrase_mix measured slower
// than it is as text (docs/EXPERIMENTS.md).
__device__ __forceinline__ int mix_entry(const int32_t *__restrict__ tile_list, int64_t j) { return __builtin_amdgcn_readfirstlane(tile_list[j]); }

// How a source of `len` samples, whose sample uw sounds at the wave's first, meets the wave (wave-uniform): it does not reach
// the wave (mix_off); the wave's samples all lie inside it (MIX_INSIDE); or it starts or ends in the wave, and each sample is
// guarded.  MIX_INSIDE is a macro: as a function both compares were evaluated in front of one branch, the edge body was no
// longer compiled apart for a wave in front of its source, and k_phrase_mix took 60 vector and 70 scalar registers for 54 and 64.
template <typename U> __device__ __forceinline__ bool mix_off(U uw, U len) { return uw >= len || uw + MIX_WAVE <= 0; }
#define MIX_INSIDE(uw, len) ((uw) >= 0 && (uw) + MIX_WAVE <= (len))

// xs[u0 .. u0 + 8) of a wave inside its source, by 16-byte loads: for a wave whose source the caller's wave-uniform test finds
// 16-byte aligned (the same answer in every lane: a lane is 32 bytes on) ...
template <typename U> __device__ __forceinline__ void mix_load8_vec(const float *__restrict__ xs, U u0, float (&v)[MIX_SPT])
{
    const float4 q0 = *reinterpret_cast<const float4 *>(xs + u0), q1 = *reinterpret_cast<const float4 *>(xs + u0 + 4);
    v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
}
// ... and elsewhere eight floats per lane as they lie, which the compiler merges into wide loads at 4-byte alignment: measured at
// 1.04 of the rate of three aligned loads from the address below and a wave-uniform shift (scripts/phrase_rate.py,
// docs/EXPERIMENTS.md).  Two functions and the branch with the kernel: as one function with the test for an argument the two
// forms' eighth load was sunk behind the join, and every lane made three loads (16, 12 and 4 bytes) where it makes two.
template <typename U> __device__ __forceinline__ void mix_load8_any(const float *__restrict__ xs, U u0, float (&v)[MIX_SPT])
{
#pragma unroll
    for (int e = 0; e < MIX_SPT; ++e) v[e] = xs[u0 + e];
}

// acc[0 .. 8) of one channel to out[t0 ..): 16-byte stores where `vec` (the channel's base is 16-byte aligned and the eight lie
// inside the line), else what lies below total_out
__device__ __forceinline__ void mix_store8(float *__restrict__ out, int64_t t0, int64_t total_out, bool vec, const float (&acc)[MIX_SPT])
{
    if (vec) {
        *reinterpret_cast<float4 *>(out + t0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4 *>(out + t0 + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
#pragma unroll
        for (int e = 0; e < MIX_SPT; ++e)
            if (t0 + e < total_out) out[t0 + e] = acc[e];
    }
}

// The grid of a mix of total_out > 0 samples: its tiles, or 0 for a line of 2^31 tiles or more, which the launcher refuses in
// its own words
static inline unsigned mix_grid(int64_t total_out)
{
    const int64_t tiles = total_out / GOOFER_MIX_TILE + (total_out % GOOFER_MIX_TILE != 0);
    return tiles < ((int64_t)1 << 31) ? (unsigned)tiles : 0u;
}
