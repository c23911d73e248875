// Standard normal draws of the jitter (sh / sr) and growl (sj) flags, made on the device (gfx950).
//
//   k_normal_fill     float64 N(0, 1) for every sample of the notes that are switched on (note_on), nothing for the others;
//                     with a per-note scale the growl factor 0.5 * 2^(scale * z) instead      SillySampler.py:1063-1065
//   k_phase_fill      the aperiodic branch's phases as a seeded reference run draws them: numpy's PCG64 stream of every note's
//                     seed, written frame-major into the batch's phase matrix (second part of this file)      GOOFER.py:1151-1152
//   k_legacy_normal_fill   the sh / sr normals as a seeded reference process draws them: numpy's legacy MT19937 + polar Box-Muller
//                     stream of every note's seed, one workgroup per note (last part of this file)      GOOFER.py:653, 666
//   k_legacy_normal_jobs   the same stream by job table: a seed, a sample count, up to four destinations and a float32 switch
//                     per job — every legacy draw of gf.synthesize (f0, sub-harmonic, volume jitter; the roughness noises)
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

// ---------------------------------------------------------------------------------------------
// Seeded phases: np.random.default_rng(seed).uniform(0.0, 2 pi, (n_bins, T)).astype(np.float32) of every note, transposed into
// the frame-major [total_frames x ld] matrix goofer_batch.phi takes.  The stream (tests/pcg_ref.py restates it):
//   state    128 bits, state <- state * PCG_MULT + inc (mod 2^128); (state, inc) of a seed come from the host (numpy's
//            PCG64(seed).state: the SeedSequence hashing is not redone here), four 64-bit words per note: state lo, hi, inc lo, hi
//   output   of the NEW state: x = hi ^ lo, v = rotr64(x, hi >> 58), d = (v >> 11) * 2^-53 (float64)
//   value    float32(0.0 + 2 pi * d): the float64 product rounded to nearest even
//   order    element (b, t) is draw k = b * T + t of its note (C order over (bins, T)), k a 64-bit value
// The matrix is frame-major and the draws bin-major, so a lane (one bin) jumps to its first draw and then steps from frame to
// frame: k steps of the generator are state <- A_k state + G_k inc with A_k = MULT^k, G_k = 1 + MULT + .. + MULT^(k-1), and
// (A, G) of 2^j steps, j < 64, is a table made at compile time (PCG_JUMP) that composes any k from its set bits.
// A wave owns PF_FRAMES consecutive frames of the concatenated frame axis x 64 consecutive bins: every store instruction covers
// 256 contiguous bytes of a row; a tile that crosses a note boundary jumps again in the next note.
struct u128 {
    uint64_t lo, hi;
};
#define PCG_MULT_HI 0x2360ED051FC65DA4ull
#define PCG_MULT_LO 0x4385DF649FCCF645ull
#define PF_FRAMES 64

// high 64 bits of a 64 x 64 product from 32-bit pieces (the table below is made by the compiler, for host and device alike)
constexpr uint64_t mulhi64_c(uint64_t a, uint64_t b)
{
    const uint64_t a0 = a & 0xFFFFFFFFull, a1 = a >> 32, b0 = b & 0xFFFFFFFFull, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFull) + (p10 & 0xFFFFFFFFull);
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}
constexpr u128 mul128_c(u128 a, u128 b)   // a * b mod 2^128
{
    return u128{a.lo * b.lo, mulhi64_c(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo};
}
constexpr u128 add128_c(u128 a, u128 b)
{
    const uint64_t lo = a.lo + b.lo;
    return u128{lo, a.hi + b.hi + (lo < a.lo ? 1u : 0u)};
}

struct pcg_jump_table {
    uint64_t w[64][4];   // A lo, A hi, G lo, G hi of 2^j steps
};
constexpr pcg_jump_table make_pcg_jump()
{
    pcg_jump_table t{};
    u128 A{PCG_MULT_LO, PCG_MULT_HI}, G{1, 0};
    for (int j = 0; j < 64; ++j) {
        t.w[j][0] = A.lo; t.w[j][1] = A.hi; t.w[j][2] = G.lo; t.w[j][3] = G.hi;
        G = add128_c(mul128_c(G, A), G);                      // (A, G) o (A, G) = (A A, G A + G)
        A = mul128_c(A, A);
    }
    return t;
}
__constant__ const pcg_jump_table PCG_JUMP = make_pcg_jump();

__device__ __forceinline__ u128 mul128(u128 a, u128 b)
{
    return u128{a.lo * b.lo, __umul64hi(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo};
}
__device__ __forceinline__ u128 add128(u128 a, u128 b)
{
    const uint64_t lo = a.lo + b.lo;
    return u128{lo, a.hi + b.hi + (lo < a.lo ? 1u : 0u)};
}

__global__ __launch_bounds__(256) void k_phase_fill(const uint64_t *__restrict__ words, const int64_t *__restrict__ frame_off,
                                                    int n_notes, int64_t total_frames, int n_bins, int chunks, int ld,
                                                    float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform
    const int64_t ft = unit / chunks;
    const int b = (int)(unit - ft * chunks) * 64 + lane;       // this lane's bin
    const int64_t g0 = ft * PF_FRAMES;
    if (g0 >= total_frames) return;
    const int64_t g1 = g0 + PF_FRAMES < total_frames ? g0 + PF_FRAMES : total_frames;   // the tile's frames are [g0, g1)
    const bool live = b < n_bins;
    int note = __builtin_amdgcn_readfirstlane(csr_find(frame_off, n_notes, g0));
    int64_t g = g0;
    while (g < g1) {
        while (note + 1 < n_notes && frame_off[note + 1] <= g) ++note;      // (notes without a frame)
        const int64_t t0 = frame_off[note], t1 = frame_off[note + 1];
        const int64_t end = t1 < g1 ? t1 : g1;
        if (end <= g) break;                                   // offsets that do not reach total_frames: nothing beyond them
        const uint64_t *w = words + 4 * (int64_t)note;
        const u128 inc{w[2], w[3]};
        if (!(inc.lo & 1)) {                                   // an increment is odd: a zero record is a note that is not seeded
            g = end;
            continue;
        }
        u128 s{w[0], w[1]};
        const uint64_t k = (uint64_t)b * (uint64_t)(t1 - t0) + (uint64_t)(g - t0);   // the lane's first draw of this note
        for (int j = 0; j < 64 && (k >> j) != 0; ++j) {
            if ((k >> j) & 1) {
                const u128 A{PCG_JUMP.w[j][0], PCG_JUMP.w[j][1]}, G{PCG_JUMP.w[j][2], PCG_JUMP.w[j][3]};
                s = add128(mul128(A, s), mul128(G, inc));
            }
        }
        float *row = out + g * (int64_t)ld + b;
        for (; g < end; ++g, row += ld) {
            s = add128(mul128(s, u128{PCG_MULT_LO, PCG_MULT_HI}), inc);
            const uint64_t x = s.hi ^ s.lo;
            const unsigned r = (unsigned)(s.hi >> 58);
            const uint64_t v = (x >> r) | (x << ((64u - r) & 63u));
            const double d = (double)(v >> 11) * 0x1p-53;
            if (live) *row = (float)(0.0 + 0x1.921fb54442d18p+2 * d);   // low + (high - low) * d, 2 pi as numpy holds it
        }
    }
}

int launch_phase_fill(goofer_ctx *ctx, const uint64_t *words, const int64_t *frame_off, int n_notes, int64_t total_frames, int n_bins,
                      float *out, int ld, hipStream_t st)
{
    if (total_frames <= 0 || n_notes <= 0) return GOOFER_OK;
    const int chunks = (n_bins + 63) / 64;
    const int64_t units = ((total_frames + PF_FRAMES - 1) / PF_FRAMES) * chunks;
    const int64_t blocks = (units + 3) / 4;
    if (blocks > 0x7fffffffLL) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_phase_fill: %lld tiles in one call", (long long)blocks);
    hipLaunchKernelGGL(k_phase_fill, dim3((unsigned)blocks), dim3(256), 0, st, words, frame_off, n_notes, total_frames, n_bins, chunks, ld,
                       out);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

// ---------------------------------------------------------------------------------------------
// Legacy normals: what a reference process draws for the sh / sr jitter (GOOFER.py:653, 666) after np.random.seed(s) —
// numpy's global MT19937 + polar Box-Muller (`np.random.randn`).  The stream (tests/mt_ref.py restates it; the full text is
// goofer_legacy_normal_fill's in include/goofer_hip.h):
//   seed     mt[0] = s, mt[i] = 1812433253 * (mt[i-1] ^ (mt[i-1] >> 30)) + i; the first draw regenerates the block
//   block    624 words twisted in place in index order, then tempered
//   double   two words a, b: ((a >> 5) * 2^26 + (b >> 6)) * 2^-53
//   attempt  two doubles: x1 = 2 d0 - 1, x2 = 2 d1 - 1, r2 = x1 x1 + x2 x2 (two rounded products, one rounded sum); rejected
//            when r2 >= 1 or r2 == 0, else f = sqrt(-2 log(r2) / r2) and the normals f x2, f x1 in that order
// A block is 156 whole attempts.  One workgroup owns one job (LN_WG threads; option "legacy_wave": one wave) — a note's enabled
// streams (k_legacy_normal_fill), or an entry of a job table (k_legacy_normal_jobs; both run legacy_fill_job) — and walks its
// blocks in order.  The in-place twist has a fixed dependency order: k in [0, 227) reads old words only, [227, 454) the new
// words of [0, 227), [454, 624) the new words of [227, 397) and, for k = 623, of mt[0] — three steps, each of which loads every
// operand (mt[k + 1] must still be old) before any lane stores.  The attempts of a block are independent: a lane tempers its
// four words, and the accepted ones are compacted behind the note's running count by wave ballots (and the wave totals in
// LDS).  Normal p of the job goes to destination p / n at sample p % n (n the job's samples; a note's destinations are its
// enabled streams in the reference's order: f0 jitter, harmonic volume, breath volume).  The block loop is bounded:
// 2 ceil(m / 245) + 4 blocks for m normals (a block accepts 156 pi / 4 = 122.5 attempts on average, 245 normals, sd 10); a
// job that needs more raises the handle's check word LEGACY_FLAG (goofer_check) and stops.
#define LN_WORDS 624
#define LN_SHIFT 397
#define LN_ATTEMPTS 156
#define LN_WG 256

template <int NT, int LO, int HI>
__device__ __forceinline__ void mt_twist_step(uint32_t *mt, int tid)
{
    constexpr int R = (HI - LO + NT - 1) / NT;
    uint32_t nv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = LO + r * NT + tid;
        nv[r] = 0u;
        if (k < HI) {
            const int k1 = k + 1 == LN_WORDS ? 0 : k + 1;
            const int km = k + LN_SHIFT >= LN_WORDS ? k + LN_SHIFT - LN_WORDS : k + LN_SHIFT;
            const uint32_t y = (mt[k] & 0x80000000u) | (mt[k1] & 0x7fffffffu);
            nv[r] = mt[km] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
    }
    __syncthreads();                                           // every operand of the step is in a register
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = LO + r * NT + tid;
        if (k < HI) mt[k] = nv[r];
    }
    __syncthreads();
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y)
{
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// One job of one workgroup: the first m = n * nd normals after np.random.seed(seed), normal p to destination p / n at sample
// p % n (d0..d3: the first nd of them are the job's destinations in order, already at the job's first sample; a null one drops
// its draws), each rounded to float32 and widened again first when f32 is set.  att: where the attempts go (or null); id: what
// the check word takes when the block bound is hit.  Every argument is uniform over the workgroup.
// (the destinations as four pointers and branches: a select chain or an indexed array over them becomes a table in scratch)
template <int NT>
__device__ __forceinline__ void legacy_fill_job(uint32_t *mt, int *wave_cnt, uint32_t seed, int64_t n, int nd, double *d0, double *d1,
                                                double *d2, double *d3, bool f32, int64_t *att, int32_t *flag, int id)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t m = n > 0 ? n * nd : 0;                      // normals of the job
    if (m <= 0) {                                              // (uniform: nobody waits at a barrier)
        if (att && tid == 0) *att = 0;
        return;
    }
    auto put = [=](int64_t p, double v) {
        const int s = (p >= n) + (p >= 2 * n) + (p >= 3 * n);
        const int64_t i = p - s * n;
        if (f32) v = (double)(float)v;
        if (s == 0) {
            if (d0) d0[i] = v;
        } else if (s == 1) {
            if (d1) d1[i] = v;
        } else if (s == 2) {
            if (d2) d2[i] = v;
        } else if (d3) {
            d3[i] = v;
        }
    };
    uint32_t v = seed;                                         // every lane runs the recurrence and keeps the words it owns
    for (int i = 0; i < LN_WORDS; ++i) {
        if ((i & (NT - 1)) == tid) mt[i] = v;
        v = 1812433253u * (v ^ (v >> 30)) + (uint32_t)(i + 1);
    }
    __syncthreads();
    const int64_t need = (m + 1) >> 1;                         // accepted attempts that cover m normals
    const int64_t max_blocks = 2 * ((m + 244) / 245) + 4;
    int64_t done = 0;                                          // accepted so far (uniform)
    for (int64_t blk = 0; done < need; ++blk) {
        if (blk >= max_blocks) {
            if (tid == 0) atomicMax(flag, id);
            break;
        }
        mt_twist_step<NT, 0, LN_WORDS - LN_SHIFT>(mt, tid);
        mt_twist_step<NT, LN_WORDS - LN_SHIFT, 2 * (LN_WORDS - LN_SHIFT)>(mt, tid);
        mt_twist_step<NT, 2 * (LN_WORDS - LN_SHIFT), LN_WORDS>(mt, tid);
#pragma unroll
        for (int r = 0; r < (LN_ATTEMPTS + NT - 1) / NT; ++r) {
            const int a = r * NT + tid;
            bool acc = false;
            double x1 = 0.0, x2 = 0.0, r2 = 1.0;
            if (a < LN_ATTEMPTS) {
                const uint4 w = *reinterpret_cast<const uint4 *>(mt + 4 * a);
                const double u0 = ((double)(mt_temper(w.x) >> 5) * 67108864.0 + (double)(mt_temper(w.y) >> 6)) * 0x1p-53;
                const double u1 = ((double)(mt_temper(w.z) >> 5) * 67108864.0 + (double)(mt_temper(w.w) >> 6)) * 0x1p-53;
                x1 = 2.0 * u0 - 1.0;                           // (exact: multiples of 2^-52 in [-1, 1))
                x2 = 2.0 * u1 - 1.0;
                r2 = __dadd_rn(__dmul_rn(x1, x1), __dmul_rn(x2, x2));
                acc = !(r2 >= 1.0 || r2 == 0.0);
            }
            const unsigned long long bal = __ballot(acc);
            int before = __popcll(bal & ((1ull << lane) - 1ull));
            int round_total = __popcll(bal);
            if constexpr (NT > 64) {                           // (one round per block: wave_cnt is rewritten two barriers later)
                if (lane == 0) wave_cnt[tid >> 6] = round_total;
                __syncthreads();
                round_total = 0;
#pragma unroll
                for (int w2 = 0; w2 < NT / 64; ++w2) {
                    const int c = wave_cnt[w2];
                    before += w2 < (tid >> 6) ? c : 0;
                    round_total += c;
                }
            }
            const int64_t j = done + before;
            const int64_t p = 2 * j;
            if (acc && p < m) {
                const double f = sqrt(-2.0 * log(r2) / r2);
                put(p, f * x2);
                if (p + 1 < m) put(p + 1, f * x1);
                if (att && j == need - 1) *att = blk * LN_ATTEMPTS + a + 1;
            }
            done += round_total;
        }
    }
}

// goofer_legacy_normal_fill: a note's job is its enabled streams of (f0, harmonic volume, breath volume), in that order
template <int NT>
__global__ __launch_bounds__(NT) void k_legacy_normal_fill(const uint32_t *__restrict__ seeds, const unsigned char *__restrict__ stream_on,
                                                           const int64_t *__restrict__ sample_off, double *__restrict__ out_f0,
                                                           double *__restrict__ out_vol_h, double *__restrict__ out_vol_b,
                                                           int64_t *__restrict__ attempts, int32_t *__restrict__ flag)
{
    __shared__ __attribute__((aligned(16))) uint32_t mt[LN_WORDS];
    __shared__ int wave_cnt[NT / 64];
    const int note = blockIdx.x;
    const int64_t base = sample_off[note];
    const int64_t n = sample_off[note + 1] - base;
    const unsigned char *on = stream_on + 3 * (int64_t)note;
    const bool e0 = on[0] != 0, e1 = on[1] != 0, e2 = on[2] != 0;
    double *const s0 = out_f0 ? out_f0 + base : nullptr, *const s1 = out_vol_h ? out_vol_h + base : nullptr,
                 *const s2 = out_vol_b ? out_vol_b + base : nullptr;
    // the enabled streams moved to the front (a null output: its draws are consumed and dropped)
    double *const d0 = e0 ? s0 : (e1 ? s1 : s2);
    double *const d1 = (e0 && e1) ? s1 : s2;
    legacy_fill_job<NT>(mt, wave_cnt, seeds[note], n, (int)e0 + (int)e1 + (int)e2, d0, d1, s2, nullptr, false,
                        attempts ? attempts + note : nullptr, flag, note + 1);
}

// goofer_legacy_normal_jobs: the job table
template <int NT>
__global__ __launch_bounds__(NT) void k_legacy_normal_jobs(const goofer_legacy_job *__restrict__ jobs, int64_t *__restrict__ attempts,
                                                           int32_t *__restrict__ flag)
{
    __shared__ __attribute__((aligned(16))) uint32_t mt[LN_WORDS];
    __shared__ int wave_cnt[NT / 64];
    const goofer_legacy_job *jb = jobs + blockIdx.x;
    int nd = jb->n_dst;
    nd = nd < 0 ? 0 : (nd > 4 ? 4 : nd);
    double *const d0 = jb->dst[0] ? jb->dst[0] + jb->off[0] : nullptr, *const d1 = jb->dst[1] ? jb->dst[1] + jb->off[1] : nullptr,
                 *const d2 = jb->dst[2] ? jb->dst[2] + jb->off[2] : nullptr, *const d3 = jb->dst[3] ? jb->dst[3] + jb->off[3] : nullptr;
    legacy_fill_job<NT>(mt, wave_cnt, jb->seed, jb->n, nd, d0, d1, d2, d3, (jb->flags & GOOFER_LEGACY_F32) != 0,
                        attempts ? attempts + blockIdx.x : nullptr, flag, (int)blockIdx.x + 1);
}

int launch_legacy_normal_fill(goofer_ctx *ctx, const uint32_t *seeds, const unsigned char *stream_on, const int64_t *sample_off, int n_notes,
                              double *out_f0, double *out_vol_h, double *out_vol_b, int64_t *attempts, hipStream_t st)
{
    if (n_notes <= 0) return GOOFER_OK;
    int32_t *flag = ctx->ovf_flag + LEGACY_FLAG;
    if (ctx->legacy_wave)
        hipLaunchKernelGGL(k_legacy_normal_fill<64>, dim3((unsigned)n_notes), dim3(64), 0, st, seeds, stream_on, sample_off, out_f0, out_vol_h,
                           out_vol_b, attempts, flag);
    else
        hipLaunchKernelGGL(k_legacy_normal_fill<LN_WG>, dim3((unsigned)n_notes), dim3(LN_WG), 0, st, seeds, stream_on, sample_off, out_f0,
                           out_vol_h, out_vol_b, attempts, flag);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

int launch_legacy_normal_jobs(goofer_ctx *ctx, const goofer_legacy_job *jobs, int n_jobs, int64_t *attempts, hipStream_t st)
{
    if (n_jobs <= 0) return GOOFER_OK;
    int32_t *flag = ctx->ovf_flag + LEGACY_FLAG;
    if (ctx->legacy_wave)
        hipLaunchKernelGGL(k_legacy_normal_jobs<64>, dim3((unsigned)n_jobs), dim3(64), 0, st, jobs, attempts, flag);
    else
        hipLaunchKernelGGL(k_legacy_normal_jobs<LN_WG>, dim3((unsigned)n_jobs), dim3(LN_WG), 0, st, jobs, attempts, flag);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}
