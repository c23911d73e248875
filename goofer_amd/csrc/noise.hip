// Standard normal draws of the jitter (sh / sr) and growl (sj) flags, made on the device (gfx950).
//
//   k_normal_fill     float64 N(0, 1) for every sample of the notes that are switched on (note_on), nothing for the others;
//                     with a per-note scale the growl factor 0.5 * 2^(scale * z) instead      SillySampler.py:1063-1065
//
// The stream is a definition (tests/noise_ref.py restates it in numpy, word for word):
//   block    Philox-4x32, 10 rounds (philox_rounds<10>, the round function the phases use with 7)
//   key      batch seed ^ (params[note].seed[0] | params[note].seed[1] << 32)   — the phases' key: a note's draws are its own
//   counter  c0 = index of the sample pair inside the note (i >> 1; 32 bits: notes up to 2^33 samples), c1 = stream tag, c2 = 0, c3 = NORMAL_C3 (the phases'
//            blocks carry PHILOX_PHASE_C3 there: no (key, counter) block is shared with the phase draws of the note)
//   tags     0 f0 jitter, 1 harmonic volume jitter, 2 breath volume jitter, 3 sub-harmonic f0 jitter (reserved), 4 growl
//   normals  Box-Muller in float64 on the block's words w0..w3:
//            u1 = ((w0 | (w1 & 0x1FFFFF) << 32) + 1) * 2^-53 in (0, 1],  u2 = (w2 | (w3 & 0x1FFFFF) << 32) * 2^-53 in [0, 1),
//            r = sqrt(-2 ln u1);  even sample r cos(2 pi u2), odd sample r sin(2 pi u2)
// A lane owns one block and stores its two samples as one 16-byte vector where the pair is 16-byte aligned in the
// concatenated array (note offsets are arbitrary: a note that starts on an odd index has its pairs straddle the
// alignment and takes two 8-byte stores, and its first / last odd sample are single stores).
#include "binops_core.h"
#include "launchers.h"

#define NORMAL_C3 0x6A09E667u
#define NF_THREADS 256
#define NF_TILE (2 * NF_THREADS)     // samples per workgroup: one pair per lane

// Both normals of pair q of a note; the samples of it that lie in [g_lo, g_hi) are stored (base = the note's offset).
__device__ __forceinline__ void normal_pair(uint64_t key, uint32_t tag, int64_t q, int64_t base, int64_t g_lo, int64_t g_hi,
                                            bool growl, double scale, double *__restrict__ out)
{
    const int64_t ga = base + 2 * q, gb = ga + 1;
    const bool wa = ga >= g_lo && ga < g_hi, wb = gb >= g_lo && gb < g_hi;
    if (!wa && !wb) return;
    const uint4 w = philox_rounds<10>((uint32_t)q, tag, 0u, NORMAL_C3, (uint32_t)key, (uint32_t)(key >> 32));
    const uint64_t m1 = ((uint64_t)w.x | ((uint64_t)(w.y & 0x1FFFFFu) << 32)) + 1u;   // 1 .. 2^53: exact as a double
    const uint64_t m2 = (uint64_t)w.z | ((uint64_t)(w.w & 0x1FFFFFu) << 32);
    const double u1 = (double)m1 * 0x1p-53, u2 = (double)m2 * 0x1p-53;
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);                                // 2 u2 is exact; no reduction of 2 pi u2 by a rounded pi
    double za = r * c, zb = r * s;
    if (growl) {
        za = 0.5 * exp2(scale * za);
        zb = 0.5 * exp2(scale * zb);
    }
    if (wa && wb && !(ga & 1)) {
        *reinterpret_cast<double2 *>(out + ga) = make_double2(za, zb);
    } else {
        if (wa) out[ga] = za;
        if (wb) out[gb] = zb;
    }
}

__global__ __launch_bounds__(NF_THREADS) void k_normal_fill(uint64_t seed, const goofer_note_params *__restrict__ params,
                                                            const int64_t *__restrict__ sample_off, int n_notes, int64_t total,
                                                            uint32_t tag, const unsigned char *__restrict__ note_on,
                                                            const double *__restrict__ growl_scale, double *__restrict__ out)
{
    const sample_tile<2> t(sample_off, n_notes, total);       // a lane's two samples: one pair where the note starts on an even index
    const int64_t g0 = t.g0;
    const int64_t g1 = g0 + NF_TILE < total ? g0 + NF_TILE : total;   // the tile is [g0, g1)
    const int lo = t.lo;
    const bool growl = growl_scale != nullptr;
    auto key_of = [&](int note) { return seed ^ ((uint64_t)params[note].seed[0] | ((uint64_t)params[note].seed[1] << 32)); };
    if (t.uniform()) {                                         // the tile lies inside one note: everything per note is scalar
        if (note_on && !note_on[lo]) return;
        const int64_t base = sample_off[lo];
        const uint64_t key = key_of(lo);
        const double scale = growl ? growl_scale[lo] : 0.0;
        const int64_t i0 = g0 - base;                          // g0 is even: the tile's pairs are aligned iff i0 is
        const int64_t q0 = i0 >> 1;
        normal_pair(key, tag, q0 + threadIdx.x, base, g0, g1, growl, scale, out);
        // an odd i0: the tile starts with the second sample of pair q0 and ends with the first of pair q0 + NF_THREADS
        if ((i0 & 1) && threadIdx.x == 0) normal_pair(key, tag, q0 + NF_THREADS, base, g0, g1, growl, scale, out);
        return;
    }
    // a tile over a note boundary (or short notes): each lane takes the two samples at g, g + 1 on their own where they
    // belong to different pairs
    const int64_t g = t.g;
    if (!t.live) return;
    int note = lo;
    while (note + 1 < n_notes && sample_off[note + 1] <= g) ++note;
    int64_t base = sample_off[note];
    const bool both = g + 1 < g1 && g + 1 < sample_off[note + 1] && !((g - base) & 1);
    if (!note_on || note_on[note])
        normal_pair(key_of(note), tag, (g - base) >> 1, base, g, both ? g + 2 : g + 1, growl, growl ? growl_scale[note] : 0.0, out);
    if (both || g + 1 >= g1) return;
    while (note + 1 < n_notes && sample_off[note + 1] <= g + 1) ++note;
    base = sample_off[note];
    if (!note_on || note_on[note])
        normal_pair(key_of(note), tag, (g + 1 - base) >> 1, base, g + 1, g + 2, growl, growl ? growl_scale[note] : 0.0, out);
}

int launch_normal_fill(goofer_ctx *ctx, uint64_t seed, const goofer_note_params *params, const int64_t *sample_off, int n_notes,
                       int64_t total, int tag, const unsigned char *note_on, const double *growl_scale, double *out, hipStream_t st)
{
    if (total <= 0 || n_notes <= 0) return GOOFER_OK;
    return launch_per_sample(ctx, k_normal_fill, total, NF_TILE, 0, st, seed, params, sample_off, n_notes, total, (uint32_t)tag, note_on,
                             growl_scale, out);
}
