// Per-sample kernels for gfx950: voicing-mask smoothing, stem gains, peak normalisation, V/B/U mix.
//
//   k_mask_short   mask[::4] -> Gaussian sigma/4 (fp64)              GOOFER.py:556-562 (smooth_mask_ds)
//   k_ola3_gains   overlap-add, lerp-upsample the smoothed mask, scale the three stems, per-note peak
//                                                                    GOOFER.py:563-567, 1179-1193, 1210
//   k_apply_gain   gain = (1/peak)^normalize, reconstruct, V/B/U mix GOOFER.py:1208-1218, SillySampler.py:1142-1151
#include <type_traits>
#include "fft_core.h"

#include "samples_core.h"
#include "ola_walk.h"
#include "launchers.h"

// A workgroup owns MS_TILE consecutive short samples of the concatenated axis.  For every note that tile touches (one,
// almost always) it parks the decimated mask values of the segment plus 2*radius in LDS — each fetched once instead of
// 2*radius+1 times, and the note lookup / tap staging paid once per 1024 outputs: the kernel is a chain of dependent
// loads in front of very little arithmetic, so fewer, longer workgroups are what makes it fast — then the waves take
// the segment's 64-sample chunks in turn.  A chunk whose 64 + 2*radius window is all zeros (ones) answers 0 (the running
// sum of the taps: the same additions in the same order) without the 2*radius+1-tap loop — voicing masks are 0/1
// almost everywhere.  fp64 accumulate in tap order.
#define MS_MAXWIN 1152     // LDS floats per workgroup = 4 * MS_MAXWIN >= MS_TILE + 2*radius
#define MS_TILE 1024
#define MS_QUART (MS_TILE / 4)   // the flags decide per quarter of a segment: 256 knots, the four chunks the waves take side by side

// tile_flags (goofer_render_batch: a word per SA_TILE samples from the kernel that wrote the mask — four bytes, bit 0 of each: some
// value of that wave is not == 0.0f, bit 1: some value is not == 1.0f; null otherwise) settle most of this without a load of
// the mask.  The windows of a quarter's knots [q, q + l) touch the decimated indices [q - radius, q + l - 1 + radius] clipped to
// the note (the reflect map never leaves that range), i.e. the samples MASK_DS times those: when the words of every SA_TILE
// tile over them say all zeros (all ones), each chunk of the quarter would find its window all zeros (ones) below and its
// knots are 0.0 (tap_sum).  A segment whose quarters are all settled that way is written at once: no mask load, no LDS
// window, no barrier.  Otherwise the window is staged for the unsettled quarters only.  Every wave reads the same flag words
// (one load, two votes), so the decisions are workgroup-uniform.
// sparse (render_link::mask_sparse): a wave of the kernel that wrote the mask left its values unwritten where its flag byte carries
// MASK_UNSTORED.  A settled quarter never asked for them; the staged window of an unsettled one can reach into such a wave (its own
// tile's other waves, the tiles under its halo), and takes those values from the bytes (mask_value).
// counters (or null): segments answered from the flags / segments that staged a window, one atomic per segment, each counter
// spread over MASK_COUNTER_SLOTS words by workgroup (common.h).
__global__ __launch_bounds__(256) void k_mask_short(const float *__restrict__ mask, const int64_t *__restrict__ sample_off,
                                                    int n_notes, int64_t total_short, const double *__restrict__ taps, int radius,
                                                    double *__restrict__ short_s, double tap_sum,
                                                    const unsigned char *__restrict__ tile_flags, int32_t *__restrict__ counters, int sparse)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const unsigned char *const sparse_flags = sparse ? tile_flags : nullptr;
    double *s_taps = reinterpret_cast<double *>(smem);
    float *s_all = reinterpret_cast<float *>(s_taps + (2 * radius + 1));          // 4 * MS_MAXWIN floats
    __shared__ int s_lo[2];
    for (int i = threadIdx.x; i < 2 * radius + 1; i += blockDim.x) s_taps[i] = taps[i];
    const int64_t g0 = (int64_t)blockIdx.x * MS_TILE;
    int64_t g1 = g0 + MS_TILE;                               // one past the tile
    if (g1 > total_short) g1 = total_short;
    if (threadIdx.x < WAVE) {                               // largest note with short_base(note) <= g, first wave cooperatively
        auto key = [&](int k) { return short_base(sample_off, k); };
        const int a = wave_find(n_notes, g0, (int)threadIdx.x, key);
        const int b = wave_find(n_notes, g1 - 1, (int)threadIdx.x, key);
        if (threadIdx.x == 0) { s_lo[0] = a; s_lo[1] = b; }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n_lo = __builtin_amdgcn_readfirstlane(s_lo[0]), n_hi = __builtin_amdgcn_readfirstlane(s_lo[1]);

    if (2 * radius + MS_TILE <= 4 * MS_MAXWIN) {
        bool staged = false;                                 // some segment of this workgroup has used the LDS window
        for (int note = n_lo; note <= n_hi; ++note) {
            const int64_t sb = short_base(sample_off, note);
            const int64_t base = sample_off[note], n = sample_off[note + 1] - base;
            const int64_t ns = (n + MASK_DS - 1) / MASK_DS;
            const int64_t s0 = g0 > sb ? g0 : sb, s1 = g1 < sb + ns ? g1 : sb + ns;    // the tile's part of this note's live range
            if (s1 <= s0) continue;                          // workgroup-uniform
            const int64_t q0 = s0 - sb;
            const int len = (int)(s1 - s0);
            // bit k of flat0 (flat1): the flags say every window of quarter k is all zeros (ones)
            unsigned flat0 = 0u, flat1 = 0u;
            const int nq = (len + MS_QUART - 1) / MS_QUART;
            if (tile_flags) {
                auto tile_of = [&](int64_t q) {              // flag tile of decimated index q (clipped to the note) of this note
                    q = q < 0 ? 0 : (q > ns - 1 ? ns - 1 : q);
                    return (base + MASK_DS * q) / SA_TILE;
                };
                const int64_t t0 = tile_of(q0 - radius), t1 = tile_of(q0 + len - 1 + radius);
                if (t1 - t0 < WAVE) {                        // (19 tiles at the largest radius of this path)
                    const uint32_t f = lane <= (int)(t1 - t0) ? reinterpret_cast<const uint32_t *>(tile_flags)[t0 + lane] : 0x03030303u;
                    const uint64_t z = __ballot((f & 0x01010101u) == 0u), o = __ballot((f & 0x02020202u) == 0u);
                    // lane k settles quarter k: the tiles a .. b (relative to t0) of its windows against the two votes
                    const int ql = (lane < nq ? lane : 0) * MS_QUART, qh = ql + MS_QUART < len ? ql + MS_QUART : len;
                    const int a = (int)(tile_of(q0 + ql - radius) - t0), b = (int)(tile_of(q0 + qh - 1 + radius) - t0);
                    const uint64_t need = (b - a >= 63 ? ~0ull : (1ull << (b - a + 1)) - 1ull) << a;
                    const bool is0 = lane < nq && (z & need) == need, is1 = lane < nq && !is0 && (o & need) == need;
                    flat0 = (unsigned)__ballot(is0);
                    flat1 = (unsigned)__ballot(is1);
                }
            }
            const unsigned flat = flat0 | flat1;
            if (flat == (1u << nq) - 1u) {                   // answered from the flags: the values the all0 / all1 chunks get below
                for (int w = threadIdx.x; w < len; w += blockDim.x) short_s[s0 + w] = ((flat1 >> (w / MS_QUART)) & 1u) ? tap_sum : 0.0;
                if (counters && threadIdx.x == 0) atomicAdd(counters + (2 * (blockIdx.x % MASK_COUNTER_SLOTS)) * MASK_COUNTER_STRIDE, 1);
                continue;
            }
            if (counters && threadIdx.x == 0) atomicAdd(counters + (2 * (blockIdx.x % MASK_COUNTER_SLOTS) + 1) * MASK_COUNTER_STRIDE, 1);
            if (staged) __syncthreads();                     // the previous segment's window is no longer read
            staged = true;
            for (int w = threadIdx.x; w < len + 2 * radius; w += blockDim.x) {
                bool want = flat == 0u;                      // a settled quarter's part of the window is not read
                for (int k = 0; k < nq && !want; ++k) want = !((flat >> k) & 1u) && w >= k * MS_QUART && w < (k + 1) * MS_QUART + 2 * radius;
                if (want) s_all[w] = mask_value(mask, sparse_flags, base + MASK_DS * reflect_index(q0 - radius + w, ns));
            }
            __syncthreads();
            for (int c0 = wv * WAVE; c0 < len; c0 += 4 * WAVE) {
                const float *x0 = s_all + c0;                // this chunk's window: cl + 2r values
                const int cl = len - c0 < WAVE ? len - c0 : WAVE;
                const bool live = lane < cl;
                double acc;
                if ((flat >> (c0 / MS_QUART)) & 1u) {        // (a chunk lies inside one quarter)
                    acc = ((flat1 >> (c0 / MS_QUART)) & 1u) ? tap_sum : 0.0;
                } else {
                    bool all0 = true, all1 = true;
                    for (int w = lane; w < cl + 2 * radius; w += WAVE) {
                        const float v = x0[w];
                        all0 &= v == 0.0f;
                        all1 &= v == 1.0f;
                    }
                    if (__all(all0)) {
                        acc = 0.0;
                    } else if (__all(all1)) {
                        acc = tap_sum;
                    } else {
                        acc = 0.0;
                        const float *x = x0 + lane;
                        if (live)
                            for (int j = 0; j <= 2 * radius; ++j) acc += s_taps[j] * (double)x[j];
                    }
                }
                if (live) short_s[s0 + c0 + lane] = acc;
            }
        }
        return;
    }
    for (int64_t g = g0 + threadIdx.x; g < g1; g += blockDim.x) {
        int note = n_lo;
        while (note + 1 < n_notes && short_base(sample_off, note + 1) <= g) ++note;
        const int64_t q = g - short_base(sample_off, note);
        const int64_t base = sample_off[note], n = sample_off[note + 1] - base;
        const int64_t ns = (n + MASK_DS - 1) / MASK_DS;
        if (q >= ns) continue;
        double acc = 0.0;
        for (int j = 0; j <= 2 * radius; ++j) acc += s_taps[j] * (double)mask_value(mask, sparse_flags, base + MASK_DS * reflect_index(q + j - radius, ns));
        short_s[g] = acc;
    }
}

// per-note constants of the mask upsampler: 1/(n-1) and 1/(ns-1) as true divisions (numpy's linspace step)
__global__ void k_note_steps(const int64_t *__restrict__ sample_off, int n_notes, double *__restrict__ steps)
{
    int note = blockIdx.x * blockDim.x + threadIdx.x;
    if (note >= n_notes) return;
    const int64_t n = sample_off[note + 1] - sample_off[note];
    const int64_t ns = (n + MASK_DS - 1) / MASK_DS;
    steps[2 * note] = n > 1 ? 1.0 / (double)(n - 1) : 0.0;
    steps[2 * note + 1] = ns > 1 ? 1.0 / (double)(ns - 1) : 0.0;
}

// The per-sample kernels below: each thread owns SPT consecutive samples (16-byte loads / stores); a block of 256 threads
// covers 1024 samples.
#define SPT 4

// Overlap-add of the three stems + mask upsample + stem gains + per-note peak in ONE pass over the samples
// (k_ola_gather x3 + a gain pass): each output sample gathers its covering windowed frames of the three
// stems in ascending frame order (the reference's fp32 accumulation order), normalises by the summed
// squared window, then applies the gains.  Saves one full write + read of the three stems.
__global__ __launch_bounds__(256) void k_ola3_gains(const float *__restrict__ fr_h, const float *__restrict__ fr_u,
                                                    const float *__restrict__ fr_b, const float *__restrict__ win_sq,
                                                    const float *__restrict__ note_mag, const double *__restrict__ short_s,
                                                    const int64_t *__restrict__ sample_off, const int64_t *__restrict__ frame_off,
                                                    int n_notes, int64_t total_samples, int n_fft, int hop,
                                                    const goofer_note_params *__restrict__ params, const double *__restrict__ steps,
                                                    float *__restrict__ harm, float *__restrict__ uv, float *__restrict__ bre,
                                                    float *__restrict__ note_peak)
{
    const sample_tile<> t(sample_off, n_notes, total_samples);
    const int64_t g = t.g;

    auto body = [&](int note) -> float {
        const int64_t base = sample_off[note], n = sample_off[note + 1] - base;
        const int64_t i = g - base;
        const int64_t fbase = frame_off[note];
        const int64_t T = frame_off[note + 1] - fbase;
        float h = 0.f, u = 0.f, b = 0.f;
        if (i < (int64_t)hop * (T - 1)) {
            const int64_t p = i + n_fft / 2;
            int64_t lo = p - n_fft + 1;
            lo = lo <= 0 ? 0 : (lo + hop - 1) / hop;
            int64_t hi = p / hop;
            if (hi > T - 1) hi = T - 1;
            float ws = 0.f;
            for (int64_t fr = lo; fr <= hi; ++fr) {
                const int j = (int)(p - fr * hop);
                const int64_t at = (fbase + fr) * n_fft + j;
                h += fr_h[at];
                u += fr_u[at];
                b += fr_b[at];
                ws += win_sq[j];
            }
            if (ws > 1e-9f) { h /= ws; u /= ws; b /= ws; }
            h = h / note_mag[note];
        }
        const int64_t ns = (n + MASK_DS - 1) / MASK_DS;
        const float ms = smooth_mask_at(short_s + short_base(sample_off, note), ns, i, n, steps[2 * note], steps[2 * note + 1]);
        b = (b * ms) * params[note].breath_strength;
        u = (u * (1.0f - ms)) * params[note].uv_strength;
        harm[g] = h;
        uv[g] = u;
        bre[g] = b;
        return fabsf((h + u) + b);
    };
    // (the body twice, so that the uniform tile's runs on a scalar note index)
    const int note = t.live && !t.uniform() ? t.note(sample_off) : t.lo;
    const float pk = !t.live ? 0.f : (t.uniform() ? body(t.lo) : body(note));
    note_reduce(t, note, t.live, pk, [](float a, float b) { return fmaxf(a, b); }, [&](int k, float m) { atomic_max_pos(note_peak + k, m); });
}

// ---------------------------------------------------------------------------------------------
// irFFT of the three stems + overlap-add + gains + per-note peak in one pass over the spectra (replaces three
// k_irfft_frames launches and k_ola3_gains: the windowed frames never go to HBM).
//
// A wave walks `run` consecutive frames of the concatenated frame axis in order.  Per stem it keeps a ring of
// n_fft accumulators in LDS indexed by (padded sample position mod n_fft): frame t adds its windowed samples to
// positions [t hop, t hop + n_fft); the last `hop` of them are first contributions and are stored, the rest are
// added — so every output sample receives its covering frames in ascending frame order, the reference's fp32
// order (GOOFER.py:379-385).  After frame t, hop t is complete: it is normalised by the summed squared window,
// scaled by the stem gains and written.  A run that starts inside a note first replays the `halo` preceding
// frames (accumulate only); the wave that owns a note's last frame also flushes the hops behind it and the
// zero-filled tail (GOOFER.py:402-413).  The walk itself is csrc/ola_walk.h.

// 64-sample register slots of the output stage: hop <= 64 SLOTS; larger hops go sample by sample.  Eight slots in the 1024-point
// kernel would cost it its second wave per SIMD
template <int M> constexpr int ola3_slots = M >= 1024 ? 8 : 4;
template <int M>
__global__ __launch_bounds__(256, M <= 512 ? 2 : 1) void k_irfft_ola3(const float2 *__restrict__ S_h, const float2 *__restrict__ S_u,
                                                    const float2 *__restrict__ S_b, int ldc, int64_t total_frames,
                                                    const int *__restrict__ frame_note, const int64_t *__restrict__ frame_off,
                                                    const int64_t *__restrict__ sample_off, int hop, int run, int halo,
                                                    const float *__restrict__ note_mag, const double *__restrict__ short_s,
                                                    const double *__restrict__ steps, const goofer_note_params *__restrict__ params,
                                                    float *__restrict__ harm, float *__restrict__ uv, float *__restrict__ bre,
                                                    float *__restrict__ note_peak, const float2 *__restrict__ g_tw,
                                                    const float2 *__restrict__ g_twh, const float *__restrict__ g_win)
{
    constexpr int R = fft_cfg<M>::R, NF = 2 * M;
    constexpr int SLOTS = ola3_slots<M>;
    extern __shared__ __align__(16) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int KN = hop / MASK_DS + KNOT_MARGIN;
    ola_lds<M, WAVES_PER_BLOCK, 3> L;
    L.carve(smem, wave, KN);
    float2 *const tw = L.tw, *const twh = L.twh, *const buf = L.buf;
    float *const win = L.win, *const ring = L.ring;
    double *const kbuf = L.kbuf;
    load_tables<M>(tw, twh, win, g_tw, g_twh, g_win);

    const int64_t f0 = ola_run_first(blockIdx.x, WAVES_PER_BLOCK, wave, run);
    if (f0 >= total_frames) return;                          // no block barrier below
    int64_t fs, f1;
    ola_run_span(f0, run, halo, total_frames, frame_note, frame_off, fs, f1);
    const float inv_m = 0.5f / (float)M;                     // 1/M of the transform and the 1/2 of the input stage (irfft_pre)

    // spectrum rows of the next (frame, stem) job are fetched while the current one is transformed
    float2 nk[R], nm[R];
    auto fetch = [&](int64_t f, int stem) {
        const float2 *row = (stem == 0 ? S_h : (stem == 1 ? S_u : S_b)) + f * (int64_t)ldc;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int k = lane + WAVE * r;
            nk[r] = row[k];
            nm[r] = row[M - k];
        }
    };
    fetch(fs, 0);

    ola_note N;
    float mag = 1.f, rmag = 1.f, g_b = 0.f, g_u = 0.f, pk = 0.f;

    // per-lane constants of the output stage for its samples j = lane + 64 u of a hop: the summed squared window
    // when all covering frames exist (interior hops), and its reciprocal
    float ws_u[SLOTS], rws_u[SLOTS];
    const int max_back = ola_max_back(NF, hop);
#pragma unroll
    for (int u = 0; u < SLOTS; ++u) {
        ws_u[u] = 0.f;
        rws_u[u] = 0.f;
        if (lane + WAVE * u < hop) ola_full_ws(win, NF, hop, lane + WAVE * u, ws_u[u], rws_u[u]);
    }
    // per-lane constants of the transform's two ends: the conj-trick twiddle of bin k and the synthesis window of
    // sample pair m, k = m = lane + 64 r
    // (kept in registers up to M = 512; the 2048-point frame has no registers to spare and re-reads them from LDS)
    constexpr bool HOIST = M <= 512;
    auto wc_of = [&](int k) { return (k <= M / 2) ? cconj(twh[k]) : make_float2(-twh[M - k].x, -twh[M - k].y); };
    // (z / M) * w == z * (w / M) exactly (M is a power of two), and the conjugate's sign rides along
    auto win_of = [&](int k) { return make_float2(win[2 * k] * inv_m, -(win[2 * k + 1] * inv_m)); };
    float2 tw1_r[7], tw2_r[7];                                // radix-8 pass twiddles of this lane (M == 512 only)
    if constexpr (M == 512) fft_lane_twiddles<M>(tw, lane, tw1_r, tw2_r);
    float2 wc_r[HOIST ? R : 1], win_r[HOIST ? R : 1];
    if constexpr (HOIST) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            wc_r[r] = wc_of(lane + WAVE * r);
            win_r[r] = win_of(lane + WAVE * r);
        }
    }

    // hop <= 64 SLOTS: the hop's knots are parked in LDS (knot_window) and its samples' window sums are the constants above
    knot_window<WAVE * SLOTS> kw;
    const bool slots_ok = hop <= WAVE * SLOTS;

    // finished hop h of the current note -> window-sum quotient -> gains -> stems; also the flush hops and the zero tail.
    // NS slots of 64 samples cover the hop: loads first, then the arithmetic, then the stores, with the knots parked in LDS and
    // the interior window sums the constants above.  NS == 0: a hop wider than the slots goes 64 samples a pass, with the
    // knots from global memory and every window sum taken over the frames that exist.
    auto emit = [&](auto ns_tag, int h) {
        constexpr int NS = decltype(ns_tag)::value, U = NS > 0 ? NS : 1;
        const int p0 = h * hop - M;                           // output index of the hop's first sample
        const int lo = kw.lo;
        auto knot = [&](int k) {
            if constexpr (NS > 0) return kw.at(kbuf, KN, lo, k);
            else return N.ss[k];
        };
        for (int j0 = lane; j0 < (NS > 0 ? WAVE : hop); j0 += WAVE) {
            float vh[U], vu[U], vb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (h * hop + j0 + WAVE * u) & (NF - 1);
                vh[u] = ring[q];
                vu[u] = ring[NF + q];
                vb[u] = ring[2 * NF + q];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + WAVE * u;
                const int i = p0 + j;
                if (j >= hop || i < 0 || i >= N.n) continue;
                float xh = 0.f, xu = 0.f, xb = 0.f;
                if (i < N.out_len) {
                    xh = vh[u]; xu = vu[u]; xb = vb[u];
                    if (NS > 0 && ola_interior(h, max_back, N.T)) {
                        // interior hop: the divisor is a per-lane constant; with r = RN(1 / ws) the quotient correction
                        // q + fma(-q, ws, x) * r is the correctly rounded x / ws (Markstein) in three instructions
                        const float ws = ws_u[NS > 0 ? u : 0], rw = rws_u[NS > 0 ? u : 0];
                        if (ws > 1e-9f) { xh = div_by(xh, ws, rw); xu = div_by(xu, ws, rw); xb = div_by(xb, ws, rw); }
                    } else {
                        const float ws = ola_partial_ws(win, NF, hop, N.T, h, j);
                        if (ws > 1e-9f) { xh /= ws; xu /= ws; xb /= ws; }
                    }
                    // (a wide hop takes the quotient itself, as it always has: under this build's fp32 division the two are not
                    // the same float on every sample, and the wide form's bits stay what they were)
                    xh = NS > 0 ? div_by(xh, mag, rmag) : xh / mag;
                }
                const float ms = smooth_mask_at32(knot, N.ns, i, N.n, N.step_n, N.step_s, N.kps);
                xb = (xb * ms) * g_b;
                xu = (xu * (1.0f - ms)) * g_u;
                harm[N.base + i] = xh;
                uv[N.base + i] = xu;
                bre[N.base + i] = xb;
                pk = fmaxf(pk, fabsf((xh + xu) + xb));
            }
        }
    };
    const int nslot = (hop + WAVE - 1) / WAVE;
    auto peak_out = [&]() {
        const float m = wave_max(pk);
        if (lane == 0) atomic_max_pos(note_peak + N.note, m);
    };

    for (int64_t f = fs; f < f1; ++f) {
        const int nt = frame_note[f];
        if (nt != N.note) {
            if (N.note >= 0) peak_out();
            N.enter(nt, hop, sample_off, frame_off, steps, short_s);
            pk = 0.f;
            mag = note_mag[nt];
            rmag = 1.0f / mag;
            g_b = params[nt].breath_strength;
            g_u = params[nt].uv_strength;
        }
        const int t = (int)(f - N.fbase);
        if (f >= f0 && slots_ok) kw.fetch(t, hop, M, N.kps, N.ns, N.ss, KN, lane);   // lands during the three transforms below
#pragma unroll
        for (int stem = 0; stem < 3; ++stem) {
            float2 v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int k = lane + WAVE * r;
                float2 xk = nk[r], xm = nm[r];
                if (k == 0) { xk.y = 0.f; xm.y = 0.f; }       // irfft ignores Im of DC and Nyquist
                v[r] = irfft_pre(xk, xm, HOIST ? wc_r[HOIST ? r : 0] : wc_of(k));
            }
            // next job's rows: same frame next stem, or the next frame's first stem
            if (stem < 2) fetch(f, stem + 1);
            else if (f + 1 < f1) fetch(f + 1, 0);
            float2 z[R];
            if constexpr (M == 512) {
                wave_fft_keep_tw<M>(v, buf, tw1_r, tw2_r, lane, z);   // twiddles and the lane's output points in registers
            } else if constexpr (M >= 512) {
                wave_fft_keep<M>(v, buf, tw, lane, z);        // the lane's output points stay in registers
            } else {
                wave_fft<M>(v, buf, tw, lane);
#pragma unroll
                for (int r = 0; r < R; ++r) z[r] = buf[lds_pad(lane + WAVE * r)];
            }
            // (all R ring reads ahead of the writes)
            ola_ring_add<NF, R, R>(ring + stem * NF, z, t, hop, lane, [&](int r) { return HOIST ? win_r[HOIST ? r : 0] : win_of(lane + WAVE * r); });
            wave_lds_sync();
        }
        if (f >= f0)
            ola_finish_hops(
                t, N.T, hop, M, N.n,
                [&](int h) {
                    if (slots_ok) {
                        kw.park(kbuf, KN, lane);
                        if (nslot <= 2) emit(std::integral_constant<int, 2>{}, h);
                        else if (nslot <= 4) emit(std::integral_constant<int, 4>{}, h);
                        else if constexpr (SLOTS >= 8) emit(std::integral_constant<int, 8>{}, h);
                    } else {
                        emit(std::integral_constant<int, 0>{}, h);
                    }
                },
                [&](int h) {
                    if (slots_ok) kw.fetch(h, hop, M, N.kps, N.ns, N.ss, KN, lane);
                });
        wave_lds_sync();
    }
    if (N.note >= 0) peak_out();
}

// ---------------------------------------------------------------------------------------------
// The same pass with ONE stem per wave, for geometries whose three rings do not leave room for a second wave per SIMD
// (n_fft 2048: 24 KB of rings + 8 KB of exchange buffer per wave, 1 wave per SIMD, 0.17-0.22 of the HBM roofline).  A wave
// walks a run of frames of one stem — job = 3 * run + stem — with a single n_fft-float ring (16.6 KB per wave at 2048:
// eight waves per CU), and leaves its stem the way the stem walkers of stems.hip do: the harmonic stem divided by the
// window sum only (1 / max|S| is applied by k_note_finish, which also takes the peak), the noise stems with their
// mask gains.  Same transforms, same ascending-frame accumulation: bit-identical to k_irfft_ola3 + k_apply_gain (tested).
// Arguments needed once per note, once per 64 frames or at set-up are read from the kernarg segment where they are used
// (cold_arg, as in the stem walkers): the frame loop holds ~60 scalars of wave state, and with 22 arguments live beside them
// the compiler spilled 142 SGPRs (a v_writelane / v_readlane pair each) and a vector register to scratch.
constexpr int OLA1_MAXHOP = 512;                                  // widest hop whose knots are parked in LDS; wider hops read them from global memory
constexpr int OLA1_KNOTS = OLA1_MAXHOP / MASK_DS + KNOT_MARGIN;   // the knot slice of a wave
struct ola1_args {
    // every frame
    const float2 *S_h, *S_u, *S_b;
    const int *frame_note;
    int ldc, hop, run, halo;
    // cold
    int64_t total_frames;
    const int64_t *frame_off, *sample_off;
    const double *short_s, *steps;
    const goofer_note_params *params;
    float *harm, *uv, *bre;
    const float2 *g_tw, *g_twh;
    const float *g_win;
    const unsigned char *frame_skip;
};
template <int M, int WPB>
__global__ __launch_bounds__(64 * WPB, 2) void k_irfft_ola1(const ola1_args A)
{
    const int ldc = A.ldc, hop = A.hop, run = A.run, halo = A.halo;
    const int *__restrict__ frame_note = A.frame_note;
    constexpr int R = fft_cfg<M>::R, NF = 2 * M;
    extern __shared__ __align__(16) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    ola_lds<M, WPB, 1> L;
    L.carve(smem, wave, OLA1_KNOTS);
    float2 *const tw = L.tw, *const twh = L.twh, *const buf = L.buf;
    float *const win = L.win, *const ring = L.ring;
    double *const kbuf = L.kbuf;
    load_tables<M>(tw, twh, win, COLD(ola1_args, g_tw), COLD(ola1_args, g_twh), COLD(ola1_args, g_win));

    // A workgroup holds runs of ONE stem (stems interleaved workgroup by workgroup): where a stem's transforms are skipped
    // (frame_skip: its gain is exactly zero over everything the frame reaches) whole workgroups retire early and the
    // dispatcher hands their CU to the next one — with the three stems of a run side by side in one workgroup the skipped
    // waves only idled beside the others.
    const int stem = (int)(blockIdx.x % 3);                   // workgroup-uniform
    const int64_t f0 = ola_run_first(blockIdx.x / 3, WPB, wave, run);
    if (f0 >= COLD(ola1_args, total_frames)) return;          // no block barrier below
    int64_t fs, f1;
    ola_run_span(f0, run, halo, COLD(ola1_args, total_frames), frame_note, COLD(ola1_args, frame_off), fs, f1);
    const unsigned skip_bit = COLD(ola1_args, frame_skip) ? (unsigned)stem : 0u;   // bit 0 (1): unvoiced stem, bit 1 (2): breath stem; harmonic: never
    // the skip bits of 64 consecutive frames as one ballot (a byte load per frame would sit on the loop's critical path)
    uint64_t skip_mask = 0;
    int64_t skip_base = -(int64_t)WAVE;
    auto skipped = [&](int64_t f) {
        if (skip_bit == 0u) return false;
        if (f >= skip_base + WAVE || f < skip_base) {
            skip_base = f;
            const int64_t g = f + lane;
            skip_mask = __ballot(g < COLD(ola1_args, total_frames) && (COLD(ola1_args, frame_skip)[g] & skip_bit) != 0);
        }
        return ((skip_mask >> (int)(f - skip_base)) & 1ull) != 0;
    };
    const float inv_m = 0.5f / (float)M;                     // 1/M of the transform and the 1/2 of the input stage (irfft_pre)
    const float2 *S = stem == 0 ? A.S_h : (stem == 1 ? A.S_u : A.S_b);
    float *out = stem == 0 ? COLD(ola1_args, harm) : (stem == 1 ? COLD(ola1_args, uv) : COLD(ola1_args, bre));

    // spectrum row of the next frame, fetched during the transform: bins lane + 64 r and the Nyquist bin; the mirrored bins
    // X[M - k] of the inverse transform's input stage come from the row itself through the (idle) exchange buffer — a second
    // set of loads would hold 32 more registers across the whole frame
    float2 nk[R], ny;
    auto fetch = [&](int64_t f) {
        const float2 *row = S + f * (int64_t)ldc;
#pragma unroll
        for (int r = 0; r < R; ++r) nk[r] = row[lane + WAVE * r];
        ny = row[M];
    };
    bool skip_cur = skipped(fs);
    if (!skip_cur) fetch(fs);

    ola_note N;
    float gain = 0.f;
    const int max_back = ola_max_back(NF, hop);
    auto wc_of = [&](int k) { return (k <= M / 2) ? cconj(twh[k]) : make_float2(-twh[M - k].x, -twh[M - k].y); };
    auto win_of = [&](int k) { return make_float2(win[2 * k] * inv_m, -(win[2 * k + 1] * inv_m)); };

    // summed squared window of this lane's hop samples j = lane + 64 u for interior hops (every covering frame exists): a
    // constant per lane, with its correctly rounded reciprocal (div_by); the first two slots only — wider hops take the loop
    float ws_c[2] = {0.f, 0.f}, rws_c[2] = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u)
        if (lane + WAVE * u < hop) ola_full_ws(win, NF, hop, lane + WAVE * u, ws_c[u], rws_c[u]);
    const int KN = hop / MASK_DS + KNOT_MARGIN;
    knot_window<OLA1_MAXHOP> kw;
    const bool slots_ok = hop <= OLA1_MAXHOP && stem != 0;    // the harmonic stem has no mask gain
    // finished hop h of the current note -> window-sum quotient -> (noise stems) mask gain -> out; also the flush hops and the zero tail
    auto emit = [&](int h) {
        const int lo = kw.lo;
        auto knot_l = [&](int k) { return kw.at(kbuf, KN, lo, k); };
        auto knot_g = [&](int k) { return N.ss[k]; };
        const bool inner = ola_interior(h, max_back, N.T);    // every covering frame exists
        for (int j = lane, u = 0; j < hop; j += WAVE, ++u) {
            const int i = h * hop + j - M;
            if (i < 0 || i >= N.n) continue;
            float x = 0.f;
            if (i < N.out_len) {
                x = ring[(h * hop + j) & (NF - 1)];
                if (inner && u < 2) {
                    const float ws = u == 0 ? ws_c[0] : ws_c[1], rw = u == 0 ? rws_c[0] : rws_c[1];
                    if (ws > 1e-9f) x = div_by(x, ws, rw);
                } else {
                    const float ws = ola_partial_ws(win, NF, hop, N.T, h, j);
                    if (ws > 1e-9f) x /= ws;
                }
            }
            if (stem != 0) {
                const float ms = slots_ok ? smooth_mask_at32(knot_l, N.ns, i, N.n, N.step_n, N.step_s, N.kps)
                                          : smooth_mask_at32(knot_g, N.ns, i, N.n, N.step_n, N.step_s, N.kps);
                x = (x * (stem == 1 ? 1.0f - ms : ms)) * gain;
            }
            out[N.base + i] = x;
        }
    };

    for (int64_t f = fs; f < f1; ++f) {
        const int nt = frame_note[f];
        if (nt != N.note) {
            N.enter(nt, hop, COLD(ola1_args, sample_off), COLD(ola1_args, frame_off), COLD(ola1_args, steps), COLD(ola1_args, short_s));
            const goofer_note_params *params = COLD(ola1_args, params);
            gain = stem == 1 ? params[nt].uv_strength : params[nt].breath_strength;
        }
        const int t = (int)(f - N.fbase);
        const bool skip_this = skip_cur;
        if (f >= f0 && slots_ok && !skip_this) kw.fetch(t, hop, M, N.kps, N.ns, N.ss, KN, lane);
        skip_cur = f + 1 < f1 && skipped(f + 1);
        if (skip_this) {
            // no transform: the slots this frame would have started from zero are zeroed, the others keep their sums
            if (f + 1 < f1 && !skip_cur) fetch(f + 1);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int m = lane + WAVE * r;
                if (ola_first(t, m, NF, hop)) *ola_slot(ring, ola_shift(t, NF, hop), m, NF) = make_float2(0.f, 0.f);
            }
        } else {
        float2 v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) buf[lane + WAVE * r] = nk[r];
        if (lane == 0) buf[M] = ny;
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int k = lane + WAVE * r;
            float2 xk = nk[r], xm = buf[M - k];
            if (k == 0) { xk.y = 0.f; xm.y = 0.f; }           // irfft ignores Im of DC and Nyquist
            v[r] = irfft_pre(xk, xm, wc_of(k));
        }
        wave_lds_sync();                                      // the row is read before the transform reuses buf
        if (f + 1 < f1 && !skip_cur) fetch(f + 1);
        float2 z[R];
        wave_fft_keep<M>(v, buf, tw, lane, z);                // the lane's output points stay in registers
        // (ring reads ahead of ring writes eight slots at a time)
        ola_ring_add<NF, R, 8>(ring, z, t, hop, lane, [&](int r) { return win_of(lane + WAVE * r); });
        }
        wave_lds_sync();
        if (f >= f0)
            ola_finish_hops(
                t, N.T, hop, M, N.n,
                [&](int h) {
                    if (skip_this) {
                        // every hop this frame reaches has a gain of exactly zero: the hop (and the flush hops behind a last frame) is zeros
                        for (int j = lane; j < hop; j += WAVE) {
                            const int i = h * hop + j - M;
                            if (i >= 0 && i < N.n) out[N.base + i] = 0.f;
                        }
                    } else {
                        if (slots_ok) kw.park(kbuf, KN, lane);
                        emit(h);
                    }
                },
                [&](int h) {
                    if (slots_ok && !skip_this) kw.fetch(h, hop, M, N.kps, N.ns, N.ss, KN, lane);
                });
        wave_lds_sync();
    }
}

template <int M>
static int irfft_ola1_impl(goofer_ctx *ctx, const float2 *S_h, const float2 *S_u, const float2 *S_b, int ldc, int64_t total_frames,
                           const int *frame_note, const int64_t *frame_off, const int64_t *sample_off, const double *short_s,
                           const double *steps, const goofer_note_params *params, float *harm, float *uv, float *bre,
                           const unsigned char *frame_skip, hipStream_t st)
{
    constexpr int WPB = 8;
    const goofer_plan_t &p = ctx->plan;
    const int halo = (p.n_fft + p.hop - 1) / p.hop - 1;
    const size_t lds = ola_lds<M, WPB, 1>::bytes(OLA1_KNOTS);
    if (lds > 160 * 1024) return goofer_fail(ctx, GOOFER_EINVAL, "one-stem overlap-add: %zu bytes of LDS", lds);
    const void *fn = (const void *)k_irfft_ola1<M, WPB>;
    int rc = kernel_allow_max_lds(ctx, fn);
    if (rc) return rc;
    int cus = 0;
    HIP_TRY(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const int64_t slots = (int64_t)(cus > 0 ? cus : 256) * WPB;          // one workgroup per CU
    // jobs = 3 stems x runs: a wave walks one stem of a run, a run >= 8 halos
    const int run = walk_run_choice(ctx, WALK_OLA1, 3 * total_frames, slots, walk_floor(halo), 256);
    const int64_t runs = (total_frames + run - 1) / run;
    ola1_args A;
    A.S_h = S_h; A.S_u = S_u; A.S_b = S_b; A.frame_note = frame_note; A.ldc = ldc; A.hop = p.hop; A.run = run; A.halo = halo;
    A.total_frames = total_frames; A.frame_off = frame_off; A.sample_off = sample_off; A.short_s = short_s; A.steps = steps;
    A.params = params; A.harm = harm; A.uv = uv; A.bre = bre; A.g_tw = p.tw_full; A.g_twh = p.tw_half; A.g_win = p.window;
    A.frame_skip = frame_skip;
    hipLaunchKernelGGL((k_irfft_ola1<M, WPB>), dim3((unsigned)(3 * ((runs + WPB - 1) / WPB))), dim3(64 * WPB), lds, st, A);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

// one stem per wave (n_fft 2048); needs k_note_finish behind it (1 / max|S|, peak, gain)
bool ola_split_supported(const goofer_plan_t &p) { return p.n_fft == 2048 && (p.hop & 1) == 0; }

int launch_irfft_ola1(goofer_ctx *ctx, const float2 *S_h, const float2 *S_u, const float2 *S_b, int ldc, int64_t total_frames,
                      const int *frame_note, const int64_t *frame_off, const int64_t *sample_off, int n_notes, const double *short_s,
                      double *steps, const goofer_note_params *params, float *harm, float *uv, float *bre,
                      const unsigned char *frame_skip, hipStream_t st)
{
    if (total_frames <= 0) return GOOFER_OK;
    if (!ola_split_supported(ctx->plan)) return goofer_fail(ctx, GOOFER_EINVAL, "one-stem overlap-add is built for n_fft 2048");
    hipLaunchKernelGGL(k_note_steps, dim3((n_notes + 255) / 256), dim3(256), 0, st, sample_off, n_notes, steps);
    LAUNCH_CHECK(ctx);
    return irfft_ola1_impl<1024>(ctx, S_h, S_u, S_b, ldc, total_frames, frame_note, frame_off, sample_off, short_s, steps, params,
                                 harm, uv, bre, frame_skip, st);
}

// ---------------------------------------------------------------------------------------------
// Exact sparsity of the noise stems for the LDS-ring pipeline (the walkers of stems.hip decide the same thing per hop inside
// their frame loop): where the smoothed mask is flat at (float) 1 over every knot a hop's samples can read, the unvoiced stem
// of that hop is multiplied by exactly 0 (GOOFER.py:1181), where it is flat at 0 the breath stem is (:1180).  A frame whose
// every hop is such a hop cannot reach a non-zero sample of that stem: its spectrum is neither written nor transformed.
// hop_flat[frame_off[note] + reach * note + h], h < T + reach: bit 0 flat at one, bit 1 flat at zero (hops without an
// output sample count as both); the knot window is the one k_irfft_ola1 stages for the hop (knots_fetch).
// eq[k] = (short_s[k] == short_s[k + 1]) over the whole smoothed-mask array: a hop's knots are one constant iff the eq bytes of
// its window are all set, and a hop then reads 35 bytes instead of 36 doubles (its neighbours' windows overlap it by a third:
// read as doubles, thread by thread, they cost eight times the unique bytes)
__global__ void k_knot_eq(const double *__restrict__ short_s, int64_t count, unsigned char *__restrict__ eq)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < count) eq[k] = k + 1 < count && short_s[k] == short_s[k + 1] ? 1 : 0;
}

__global__ void k_hop_flat(const double *__restrict__ short_s, const unsigned char *__restrict__ eq, const int64_t *__restrict__ sample_off,
                           const int64_t *__restrict__ frame_off, int n_notes, int hop, int M, int reach, unsigned char *__restrict__ hop_flat)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= frame_off[n_notes] + (int64_t)reach * n_notes) return;
    int lo = 0, hi = n_notes;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (frame_off[mid] + (int64_t)reach * mid <= g) lo = mid; else hi = mid;
    }
    const int note = lo;
    const int h = (int)(g - (frame_off[note] + (int64_t)reach * note));
    const int n = (int)(sample_off[note + 1] - sample_off[note]);
    const int ns = (n + MASK_DS - 1) / MASK_DS;
    const int i_lo = h * hop - M, i_hi = i_lo + hop - 1;
    unsigned flags = 3u;
    if (!(i_hi < 0 || i_lo >= n || ns <= 0)) {
        const int64_t sb = short_base(sample_off, note);
        const double *ss = short_s + sb;
        const unsigned char *eqn = eq + sb;
        const float kps = n > 1 ? (float)(ns - 1) / (float)(n - 1) : 0.f;
        int k0 = (int)((float)(i_lo < 0 ? 0 : i_lo) * kps) - 4;
        k0 = k0 < 0 ? 0 : (k0 > ns - 1 ? ns - 1 : k0);
        int k1 = k0 + hop / MASK_DS + KNOT_MARGIN - 1;
        k1 = k1 > ns - 1 ? ns - 1 : k1;
        const double c = ss[k0];
        bool same = true;
        for (int k = k0; k < k1; ++k) same = same && eqn[k] != 0;      // ss[k0] == ss[k0 + 1] == ... == ss[k1]
        const float cf = (float)c;
        flags = same ? ((1.0f - cf == 0.0f ? 1u : 0u) | (cf == 0.0f ? 2u : 0u)) : 0u;
    }
    hop_flat[g] = (unsigned char)flags;
}

__global__ void k_frame_skip(const unsigned char *__restrict__ hop_flat, const int *__restrict__ frame_note, const int64_t *__restrict__ frame_off,
                             int64_t total_frames, int reach, unsigned char *__restrict__ frame_skip)
{
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= total_frames) return;
    const int note = frame_note[f];
    const unsigned char *hf = hop_flat + f + (int64_t)reach * note;      // (= frame_off[note] + reach * note + t)
    unsigned acc = 3u;
    for (int q = 0; q < reach; ++q) acc &= hf[q];
    frame_skip[f] = (unsigned char)acc;
}

int launch_frame_skip(goofer_ctx *ctx, const double *short_s, int64_t short_count, const int64_t *sample_off, const int64_t *frame_off,
                      const int *frame_note, int n_notes, int64_t total_frames, unsigned char *knot_eq, unsigned char *hop_flat,
                      unsigned char *frame_skip, hipStream_t st)
{
    if (total_frames <= 0) return GOOFER_OK;
    const goofer_plan_t &p = ctx->plan;
    const int reach = (p.n_fft + p.hop - 1) / p.hop;
    const int64_t hops = total_frames + (int64_t)reach * n_notes;
    hipLaunchKernelGGL(k_knot_eq, dim3((unsigned)((short_count + 255) / 256)), dim3(256), 0, st, short_s, short_count, knot_eq);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_hop_flat, dim3((unsigned)((hops + 255) / 256)), dim3(256), 0, st, short_s, knot_eq, sample_off, frame_off, n_notes, p.hop,
                       p.n_fft / 2, reach, hop_flat);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_frame_skip, dim3((unsigned)((total_frames + 255) / 256)), dim3(256), 0, st, hop_flat, frame_note, frame_off,
                       total_frames, reach, frame_skip);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

template <int M>
static int irfft_ola3_impl(goofer_ctx *ctx, const float2 *S_h, const float2 *S_u, const float2 *S_b, int ldc, int64_t total_frames,
                           const int *frame_note, const int64_t *frame_off, const int64_t *sample_off, const float *note_mag,
                           const double *short_s, const double *steps, const goofer_note_params *params, float *harm, float *uv,
                           float *bre, float *note_peak, hipStream_t st)
{
    const goofer_plan_t &p = ctx->plan;
    const int halo = (p.n_fft + p.hop - 1) / p.hop - 1;
    // (hops wider than the slots park no knots)
    const size_t lds = ola_lds<M, WAVES_PER_BLOCK, 3>::bytes(p.hop <= WAVE * ola3_slots<M> ? p.hop / MASK_DS + KNOT_MARGIN : 0);
    int rc = kernel_allow_max_lds(ctx, (const void *)k_irfft_ola3<M>);
    if (rc) return rc;
    int slots = 0;                                            // waves of this kernel the device holds at once
    if ((rc = kernel_resident_waves(ctx, (const void *)k_irfft_ola3<M>, lds, &slots))) return rc;
    const int run = walk_run_choice(ctx, WALK_OLA3, total_frames, slots, walk_floor(halo), 128);
    const int64_t runs = (total_frames + run - 1) / run;
    hipLaunchKernelGGL(k_irfft_ola3<M>, dim3((unsigned)((runs + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK)), dim3(256), lds, st, S_h, S_u,
                       S_b, ldc, total_frames, frame_note, frame_off, sample_off, p.hop, run, halo, note_mag, short_s, steps, params,
                       harm, uv, bre, note_peak, p.tw_full, p.tw_half, p.window);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

// smooth_mask_ds's last step on its own (GOOFER.py:563-567): np.interp of the smoothed decimated mask back to the sample
// grid.  `fast` selects the walkers' 32-bit interpolant (smooth_mask_at32: flat-knot shortcut, one-step index fix-up)
// instead of the search-loop form the separate stem-gain kernels use; the two must agree bit for bit.
__global__ __launch_bounds__(256) void k_mask_upsample(const double *__restrict__ short_s, const int64_t *__restrict__ sample_off,
                                                       int n_notes, int64_t total_samples, const double *__restrict__ steps, int fast,
                                                       float *__restrict__ out)
{
    const sample_tile<1, false> t(sample_off, n_notes, total_samples);
    if (!t.live) return;
    const int64_t g = t.g;
    const int note = t.note(sample_off);
    const int64_t base = sample_off[note], n = sample_off[note + 1] - base;
    const int64_t ns = (n + MASK_DS - 1) / MASK_DS;
    const double *ss = short_s + short_base(sample_off, note);
    if (fast) {
        const float kps = n > 1 ? (float)(ns - 1) / (float)(n - 1) : 0.f;
        auto knot = [&](int k) { return ss[k]; };
        out[g] = smooth_mask_at32(knot, (int)ns, (int)(g - base), (int)n, steps[2 * note], steps[2 * note + 1], kps);
    } else {
        out[g] = smooth_mask_at(ss, ns, g - base, n, steps[2 * note], steps[2 * note + 1]);
    }
}

int launch_mask_upsample(goofer_ctx *ctx, const double *short_s, const int64_t *sample_off, int n_notes, int64_t total_samples,
                         double *steps, bool fast, float *out, hipStream_t st)
{
    if (total_samples <= 0) return GOOFER_OK;
    hipLaunchKernelGGL(k_note_steps, dim3((n_notes + 255) / 256), dim3(256), 0, st, sample_off, n_notes, steps);
    LAUNCH_CHECK(ctx);
    return launch_per_sample(ctx, k_mask_upsample, total_samples, 256, 0, st, short_s, sample_off, n_notes, total_samples, steps,
                             fast ? 1 : 0, out);
}

int launch_irfft_ola3(goofer_ctx *ctx, const float2 *S_h, const float2 *S_u, const float2 *S_b, int ldc, int64_t total_frames,
                      const int *frame_note, const int64_t *frame_off, const int64_t *sample_off, int n_notes, const float *note_mag,
                      const double *short_s, double *steps, const goofer_note_params *params, float *harm, float *uv, float *bre,
                      float *note_peak, hipStream_t st)
{
    if (total_frames <= 0) return GOOFER_OK;
    const goofer_plan_t &p = ctx->plan;
    if (p.hop & 1) return goofer_fail(ctx, GOOFER_EINVAL, "the fused overlap-add needs an even hop");
    hipLaunchKernelGGL(k_note_steps, dim3((n_notes + 255) / 256), dim3(256), 0, st, sample_off, n_notes, steps);
    LAUNCH_CHECK(ctx);
    switch (p.n_fft) {
    case 512: return irfft_ola3_impl<256>(ctx, S_h, S_u, S_b, ldc, total_frames, frame_note, frame_off, sample_off, note_mag, short_s, steps, params, harm, uv, bre, note_peak, st);
    case 1024: return irfft_ola3_impl<512>(ctx, S_h, S_u, S_b, ldc, total_frames, frame_note, frame_off, sample_off, note_mag, short_s, steps, params, harm, uv, bre, note_peak, st);
    case 2048: return irfft_ola3_impl<1024>(ctx, S_h, S_u, S_b, ldc, total_frames, frame_note, frame_off, sample_off, note_mag, short_s, steps, params, harm, uv, bre, note_peak, st);
    }
    return goofer_fail(ctx, GOOFER_EINVAL, "unsupported n_fft %d", p.n_fft);
}

__global__ __launch_bounds__(256) void k_apply_gain(float *__restrict__ harm, float *__restrict__ uv, float *__restrict__ bre,
                                                    float *__restrict__ rec, float *__restrict__ mix,
                                                    const int64_t *__restrict__ sample_off, int n_notes, int64_t total_samples,
                                                    const goofer_note_params *__restrict__ params, const float *__restrict__ note_peak,
                                                    int write_stems)
{
    const sample_tile<SPT> t(sample_off, n_notes, total_samples);
    if (!t.live) return;
    const int64_t g = t.g;
    const int lo = t.lo;

    auto gain_of = [&](int note) -> float {
        const float peak = note_peak[note] + 1e-12f;                 // fp32 add, like np.float32 + 1e-12
        return peak_gain(peak, params[note].normalize);
    };
    auto mixdown = [&](int note, float h, float u, float b) -> float {
        return ((h * params[note].mix_harm + b * params[note].mix_breath) + u * params[note].mix_unvoiced) * params[note].volume;
    };
    if (t.uniform() && g + SPT <= total_samples) {
        const float gain = gain_of(lo);
        float4 h = *reinterpret_cast<const float4 *>(harm + g);
        float4 u = *reinterpret_cast<const float4 *>(uv + g);
        float4 b = *reinterpret_cast<const float4 *>(bre + g);
        const float4 comb = make_float4((h.x + u.x) + b.x, (h.y + u.y) + b.y, (h.z + u.z) + b.z, (h.w + u.w) + b.w);
        h.x *= gain; h.y *= gain; h.z *= gain; h.w *= gain;
        u.x *= gain; u.y *= gain; u.z *= gain; u.w *= gain;
        b.x *= gain; b.y *= gain; b.z *= gain; b.w *= gain;
        if (write_stems) {
            *reinterpret_cast<float4 *>(harm + g) = h;
            *reinterpret_cast<float4 *>(uv + g) = u;
            *reinterpret_cast<float4 *>(bre + g) = b;
        }
        if (rec) *reinterpret_cast<float4 *>(rec + g) = make_float4(comb.x * gain, comb.y * gain, comb.z * gain, comb.w * gain);
        if (mix)
            *reinterpret_cast<float4 *>(mix + g) = make_float4(mixdown(lo, h.x, u.x, b.x), mixdown(lo, h.y, u.y, b.y),
                                                               mixdown(lo, h.z, u.z, b.z), mixdown(lo, h.w, u.w, b.w));
        return;
    }
    for (int k = 0; k < SPT; ++k) {
        const int64_t gi = g + k;
        if (gi >= total_samples) break;
        const int note = t.note(sample_off, gi);
        const float gain = gain_of(note);
        float h = harm[gi], u = uv[gi], b = bre[gi];
        const float comb = (h + u) + b;
        h *= gain; u *= gain; b *= gain;
        if (write_stems) { harm[gi] = h; uv[gi] = u; bre[gi] = b; }
        if (rec) rec[gi] = comb * gain;
        if (mix) mix[gi] = mixdown(note, h, u, b);
    }
}

// per-note max |harm + uv + bre| (used when the volume jitter changes stems after the fused OLA/gain pass)
__global__ __launch_bounds__(256) void k_stem_peak(const float *__restrict__ harm, const float *__restrict__ uv, const float *__restrict__ bre,
                                                   const int64_t *__restrict__ sample_off, int n_notes, int64_t total,
                                                   float *__restrict__ note_peak)
{
    const sample_tile<> t(sample_off, n_notes, total);
    const int64_t g = t.g;
    const float pk = t.live ? fabsf((harm[g] + uv[g]) + bre[g]) : 0.f;
    const int note = t.live && !t.uniform() ? t.note(sample_off) : t.lo;
    note_reduce(t, note, t.live, pk, [](float a, float b) { return fmaxf(a, b); }, [&](int k, float m) { atomic_max_pos(note_peak + k, m); });
}

int launch_stem_peak(goofer_ctx *ctx, const float *harm, const float *uv, const float *bre, const int64_t *sample_off, int n_notes,
                     int64_t total, float *note_peak, hipStream_t st)
{
    return launch_per_sample(ctx, k_stem_peak, total, 256, 0, st, harm, uv, bre, sample_off, n_notes, total, note_peak);
}

int launch_mask_short(goofer_ctx *ctx, const float *mask, const int64_t *sample_off, int n_notes, int64_t total_samples,
                      const double *d_taps, int radius, double tap_sum, double *short_s, const unsigned char *tile_flags,
                      int32_t *counters, bool sparse, hipStream_t st)
{
    int64_t total_short = total_samples / MASK_DS + n_notes;
    if (total_short <= 0) return GOOFER_OK;
    hipLaunchKernelGGL(k_mask_short, dim3((unsigned)((total_short + MS_TILE - 1) / MS_TILE)), dim3(256),
                       sizeof(double) * (2 * radius + 1) + sizeof(float) * 4 * MS_MAXWIN, st, mask, sample_off, n_notes, total_short,
                       d_taps, radius, short_s, tap_sum, tile_flags, counters, sparse && tile_flags ? 1 : 0);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

int launch_apply_gain(goofer_ctx *ctx, float *harm, float *uv, float *bre, float *rec, float *mix, const int64_t *sample_off,
                      int n_notes, int64_t total_samples, const goofer_note_params *params, const float *note_peak, bool write_stems,
                      hipStream_t st)
{
    return launch_per_sample(ctx, k_apply_gain, total_samples, 256 * SPT, 0, st, harm, uv, bre, rec, mix, sample_off, n_notes, total_samples,
                             params, note_peak, write_stems ? 1 : 0);
}

int launch_ola3_gains(goofer_ctx *ctx, const float *fr_h, const float *fr_u, const float *fr_b, const float *note_mag,
                      const double *short_s, const int64_t *sample_off, const int64_t *frame_off, int n_notes, int64_t total_samples,
                      const goofer_note_params *params, double *steps, float *harm, float *uv, float *bre, float *note_peak,
                      hipStream_t st)
{
    if (total_samples <= 0) return GOOFER_OK;
    const goofer_plan_t &p = ctx->plan;
    hipLaunchKernelGGL(k_note_steps, dim3((n_notes + 255) / 256), dim3(256), 0, st, sample_off, n_notes, steps);
    LAUNCH_CHECK(ctx);
    return launch_per_sample(ctx, k_ola3_gains, total_samples, 256, 0, st, fr_h, fr_u, fr_b, p.win_sq, note_mag, short_s, sample_off,
                             frame_off, n_notes, total_samples, p.n_fft, p.hop, params, steps, harm, uv, bre, note_peak);
}
