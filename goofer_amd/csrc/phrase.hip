// Phrase assembly on the device (gfx950): the rendered notes of a batch, which lie back to back in HBM (goofer_batch.mix with its
// CSR sample_off), trimmed, enveloped, cross-faded and summed onto one time line — UTAU's `wavtool` step — so that one track
// crosses PCIe instead of every note with its overlapped parts.  The definition is in include/goofer_hip.h (goofer_phrase_note);
// the host half, goofer_host_phrase_plan (planner.hip), checks the records and lists per tile of the track the notes that reach it.
//
// A gather-sum over the tiles of the track, on the walk of tile_mix.h; here is what a note contributes.  The note index of the
// walk is wave-uniform, so a note's record, its offsets and its seven knots are scalar loads.  Per wave and note one of three
// bodies runs, all with the same arithmetic per sample (the same bits whichever runs):
//   inside, one segment   the wave's 512 samples lie inside the note and between two knots (a note is tens of thousands of samples
//                         and six segments long: nearly always) — the segment's four numbers are scalars, no compare per sample
//   inside, some knot     the segment of each sample by five compares (pos[0] <= u < pos[6] needs none)
//   edge                  the note starts or ends in the wave: as above, each sample guarded
// The source of a thread starts wherever skip - start puts it: 16-byte loads where a wave-uniform test finds it aligned.
#include "tile_mix.h"

// g(u) of the definition for any u in [0, take): k = the largest index with pos[k] <= uf, by compares against pos[1..5]
__device__ __forceinline__ float phrase_gain(float uf, const float (&pos)[7], const float (&val)[7])
{
    float a = val[0], b = val[1], p = pos[0], q = pos[1];
#pragma unroll
    for (int k = 1; k < 6; ++k) {
        const bool ge = uf >= pos[k];
        a = ge ? val[k] : a;
        b = ge ? val[k + 1] : b;
        p = ge ? pos[k] : p;
        q = ge ? pos[k + 1] : q;
    }
    return a + (b - a) * ((uf - p) / (q - p));
}

__device__ __forceinline__ int phrase_segment(float uf, const float (&pos)[7])
{
    int k = 0;
#pragma unroll
    for (int j = 1; j < 6; ++j) k += uf >= pos[j] ? 1 : 0;
    return k;
}

__global__ __launch_bounds__(256) void k_phrase_mix(const float *__restrict__ x, const int64_t *__restrict__ sample_off,
                                                    const goofer_phrase_note *__restrict__ notes,
                                                    const int64_t *__restrict__ tile_off, const int32_t *__restrict__ tile_notes,
                                                    int64_t total_out, float *__restrict__ out)
{
    int lane;
    const int64_t w0 = mix_wave_first(lane);                   // the wave's first track sample
    if (w0 >= total_out) return;
    const int64_t t0 = w0 + lane * MIX_SPT;
    const bool x16 = (((uintptr_t)x) & 15) == 0;
    float acc[MIX_SPT];
#pragma unroll
    for (int e = 0; e < MIX_SPT; ++e) acc[e] = 0.0f;

    const int64_t j1 = tile_off[blockIdx.x + 1];
    for (int64_t j = tile_off[blockIdx.x]; j < j1; ++j) {
        const int i = mix_entry(tile_notes, j);
        const goofer_phrase_note *__restrict__ r = notes + i;
        const int64_t base = sample_off[i], len = sample_off[i + 1] - base, start = r->start;
        const int skip = r->skip, take = r->take;
        const int64_t rest = len - skip;
        const int eff = (int)(rest < take ? rest : take);     // samples of the note that exist and are used
        if (eff <= 0) continue;
        // u of the wave's first sample; clamped into an int, out of reach of [0, 2^24) where it does not fit
        int64_t uw = w0 - start;
        uw = uw < -(1 << 30) ? -(1 << 30) : (uw > (1 << 30) ? (1 << 30) : uw);
        const int uw0 = (int)uw, u0 = uw0 + lane * MIX_SPT;
        if (mix_off(uw0, eff)) continue;
        float pos[7], val[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) { pos[k] = r->pos[k]; val[k] = r->val[k]; }
        const float *__restrict__ xs = x + (base + skip);      // x_i[skip + u] = xs[u]

        if (MIX_INSIDE(uw0, eff)) {
            float v[MIX_SPT];
            if (x16 && ((base + skip + uw0) & 3) == 0) mix_load8_vec(xs, u0, v);
            else mix_load8_any(xs, u0, v);
            const int ka = phrase_segment((float)uw0, pos), kb = phrase_segment((float)(uw0 + MIX_WAVE - 1), pos);
            if (ka == kb) {                                    // one segment for the wave: its numbers are scalars
                const int k = __builtin_amdgcn_readfirstlane(ka);
                const float a = r->val[k], d = r->val[k + 1] - a, p = r->pos[k], w = r->pos[k + 1] - p;
#pragma unroll
                for (int e = 0; e < MIX_SPT; ++e) acc[e] = acc[e] + (a + d * (((float)(u0 + e) - p) / w)) * v[e];
            } else {
#pragma unroll
                for (int e = 0; e < MIX_SPT; ++e) acc[e] = acc[e] + phrase_gain((float)(u0 + e), pos, val) * v[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < MIX_SPT; ++e) {
                const int u = u0 + e;
                const bool on = u >= 0 && u < eff;
                const float xv = on ? xs[u] : 0.0f;
                const float g = phrase_gain((float)u, pos, val);   // (any value off the note: not used)
                acc[e] = on ? acc[e] + g * xv : acc[e];
            }
        }
    }

    mix_store8(out, t0, total_out, t0 + MIX_SPT <= total_out && (((uintptr_t)out) & 15) == 0, acc);
}

extern "C" int goofer_phrase_mix(goofer_ctx *ctx, const float *x, const int64_t *sample_off, int n, const goofer_phrase_note *notes,
                                 const int64_t *tile_off, const int32_t *tile_notes, int64_t total_out, float *out, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (n < 0 || total_out < 0)
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_phrase_mix: negative count (%d notes, %lld samples)", n, (long long)total_out);
    if (total_out == 0) return GOOFER_OK;
    if (!tile_off || !out || (n > 0 && (!x || !sample_off || !notes || !tile_notes)))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_phrase_mix: null pointer");
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)tile_notes) & 3 || ((uintptr_t)sample_off | (uintptr_t)notes | (uintptr_t)tile_off) & 7)
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_phrase_mix: x, out and tile_notes must be 4-byte aligned, sample_off, notes and tile_off 8-byte aligned");
    const unsigned tiles = mix_grid(total_out);
    if (!tiles) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_phrase_mix: a track of %lld samples", (long long)total_out);
    hipLaunchKernelGGL(k_phrase_mix, dim3(tiles), dim3(256), 0, (hipStream_t)stream, x, sample_off, notes, tile_off, tile_notes, total_out, out);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}
