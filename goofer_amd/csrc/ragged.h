// Ragged batches on the device (gfx950): the notes of a batch lie back to back on one sample (or frame) axis, off[0..n] their
// CSR offsets.  Here: the searches that map an index of that axis to its note, the tile of a per-sample kernel (a workgroup's
// samples and the notes they touch), the per-note reduction of such a kernel, and the launch of one.
#pragma once

#include "common.h"

// note owning global frame/sample index g given CSR offsets off[0..n]: largest k with off[k] <= g.
__device__ __forceinline__ int csr_find(const int64_t *__restrict__ off, int n, int64_t g)
{
    int lo = 0, hi = n;  // invariant off[lo] <= g < off[hi]
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// Wave-cooperative version of csr_find for any non-decreasing key(k), k in [0, n]: all 64 lanes probe 64 evenly
// spaced positions per round (one round of dependent loads narrows the range 64x: 2 rounds for 4096 notes instead
// of 12 serial steps).  Every lane of the calling wave must be active; every lane gets the result.
template <typename Key>
__device__ __forceinline__ int wave_find(int n, int64_t g, int lane, Key key)
{
    int lo = 0, hi = n;                                      // invariant key(lo) <= g < key(hi)
    while (hi - lo > 1) {
        const int step = (hi - lo + 63) >> 6;
        const int p = lo + (lane + 1) * step;
        const bool le = p < hi && key(p) <= g;
        const int c = __popcll(__ballot(le));                // probes <= g form a prefix (keys are sorted)
        const int nhi = lo + (c + 1) * step;
        lo += c * step;
        if (nhi < hi) hi = nhi;
    }
    return lo;
}

// Notes of samples g0 and gl (RANGE; else of g0 only, hi = -1), found by the first wave of the workgroup cooperatively (a serial
// binary search costs ~20 dependent loads per workgroup, which bounded the short elementwise kernels) and handed to the others
// through LDS words: wave-uniform.  Workgroups must be at least one full wave; every thread calls it (a __syncthreads inside).
// RANGE is the caller's to say, not the optimiser's to find: the words are one variable for all kernels of a file, so the
// second search of a kernel that ignores `hi` stays alive as long as any other kernel of the file reads it.
template <bool RANGE>
static __device__ __forceinline__ void block_note_range(const int64_t *__restrict__ off, int n_notes, int64_t g0, int64_t gl, int &lo, int &hi)
{
    __shared__ int s_pair[2];
    if (threadIdx.x < WAVE) {
        const int lane = threadIdx.x;
        auto key = [&](int k) { return off[k]; };
        const int a = wave_find(n_notes, g0, lane, key);
        const int b = RANGE ? wave_find(n_notes, gl, lane, key) : -1;
        if (lane == 0) { s_pair[0] = a; s_pair[1] = b; }
    }
    __syncthreads();
    lo = __builtin_amdgcn_readfirstlane(s_pair[0]);
    hi = RANGE ? __builtin_amdgcn_readfirstlane(s_pair[1]) : -1;
}

// A workgroup's samples of a ragged batch: thread t of workgroup b owns the SPT consecutive samples from
// g = (b * blockDim.x + t) * SPT on; lo and hi are the notes of the workgroup's first and last sample.  When they coincide
// (almost always: a note is ~190 workgroups long) the kernel runs its body with that index held in an SGPR, so every per-note
// load behind it (offsets, params, constants) is a scalar load instead of a chain of dependent per-lane vector loads.
// RANGE false: for kernels that only scan from lo (no hi, no uniform()).  One tile per kernel, constructed by every thread of
// the workgroup.
template <int SPT = 1, bool RANGE = true>
struct sample_tile {
    int64_t g0, g;   // first sample of the workgroup, of this thread
    int lo, hi;      // notes of the workgroup's first and last sample (wave-uniform)
    bool live;       // g lies inside the batch

    __device__ __forceinline__ sample_tile(const int64_t *__restrict__ sample_off, int n_notes, int64_t total)
    {
        g0 = (int64_t)blockIdx.x * (blockDim.x * SPT);
        int64_t gl = g0 + (int64_t)blockDim.x * SPT - 1;
        if (gl > total - 1) gl = total - 1;
        block_note_range<RANGE>(sample_off, n_notes, g0, gl, lo, hi);
        g = g0 + (int64_t)threadIdx.x * SPT;
        live = g < total;
    }
    __device__ __forceinline__ bool uniform() const
    {
        static_assert(RANGE, "a tile without the range search does not know");
        return lo == hi;
    }
    // note of sample `at` of this tile, at < total: the forward scan from lo
    __device__ __forceinline__ int note(const int64_t *__restrict__ sample_off, int64_t at) const
    {
        int n = lo;
        while (sample_off[n + 1] <= at) ++n;
        return n;
    }
    __device__ __forceinline__ int note(const int64_t *__restrict__ sample_off) const { return note(sample_off, g); }
};

// Per-note reduction of a per-sample kernel (256 threads): thread value v (op's identity where the thread is not live) of note
// `note` (read for live threads of a tile that is not uniform only).  A uniform tile combines its values — the butterfly
// o = 32 .. 1 inside each wave, then op(op(w0, w1), op(w2, w3)) over the four waves — and thread 0 commits once,
// commit(lo, combined); otherwise every live thread commits its own, commit(note, v).  The combining order is part of the
// contract: a sum's bits depend on it (k_note_sumsq).  Every thread of the workgroup calls it.
template <int SPT, typename T, typename Op, typename Commit>
static __device__ __forceinline__ void note_reduce(const sample_tile<SPT, true> &t, int note, bool live, T v, Op op, Commit commit)
{
    if (t.uniform()) {
        __shared__ T s_red[4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) commit(t.lo, op(op(s_red[0], s_red[1]), op(s_red[2], s_red[3])));
    } else if (live) {
        commit(note, v);
    }
}

// launch of a per-sample kernel: ceil(total / samples_per_block) workgroups of 256 threads; nothing for an empty batch
template <typename K, typename... A>
int launch_per_sample(goofer_ctx *ctx, K kernel, int64_t total, int samples_per_block, size_t lds_bytes, hipStream_t st, A... args)
{
    if (total <= 0) return GOOFER_OK;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + samples_per_block - 1) / samples_per_block)), dim3(256), lds_bytes, st, args...);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}
