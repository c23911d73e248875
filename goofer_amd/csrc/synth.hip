// The batch driver of libgoofer_hip.so: goofer_synth_batch strings the kernels into gf.synthesize (GOOFER.py:971-1220),
// goofer_assemble_batch runs the resampler's assembly, goofer_render_batch both as one call.  Here: which pipeline a batch takes
// (synth_route), its scratch (synth_scratch), the per-stage clock of the profiler and the small kernels the driver launches itself.
#include <algorithm>
#include <vector>

#include "common.h"
#include "launchers.h"
#include "samples_core.h"

// ---------------------------------------------------------------------------------------------
// small helper kernels of the batch driver
// Frame f of `note` -> its envelope row and, with picks != nullptr, the frame's picks of the per-sample arrays, x[::hop]
// edge-padded to the frame count (GOOFER.py:1104-1106), as one (f0, mask) record per frame.  The shaping kernels then find
// them one dependent load earlier (frame -> record) instead of three (frame -> note -> offsets -> sample).
__device__ __forceinline__ void frame_pick_and_row(int64_t f, int note, const int64_t *__restrict__ frame_off,
                                                   const int64_t *__restrict__ env_off, int64_t *__restrict__ row_src,
                                                   const int64_t *__restrict__ sample_off, const float *__restrict__ f0,
                                                   const float *__restrict__ mask, int hop, float2 *__restrict__ picks,
                                                   const unsigned char *__restrict__ sparse_flags = nullptr)
{
    int64_t t = f - frame_off[note];
    if (picks) {
        const int64_t base = sample_off[note], n = sample_off[note + 1] - base;
        float2 pv = make_float2(0.f, 0.f);
        if (n > 0) {
            int64_t at = t * hop;
            if (at >= n) at = ((n - 1) / hop) * hop;          // edge-padded: the last pick
            pv = make_float2(f0[base + at], mask_value(mask, sparse_flags, base + at));
        }
        picks[f] = pv;
    }
    const int64_t rows = env_off[note + 1] - env_off[note];
    if (t > rows - 1) t = rows - 1;     // edge-repeat (np.pad mode='edge'); truncation is implicit
    if (t < 0) t = 0;
    row_src[f] = env_off[note] + t;
}

__global__ void k_row_src(const int64_t *__restrict__ frame_off, const int64_t *__restrict__ env_off,
                          const int *__restrict__ frame_note, int64_t total_frames, int64_t *__restrict__ row_src,
                          const int64_t *__restrict__ sample_off, const float *__restrict__ f0, const float *__restrict__ mask,
                          int hop, float2 *__restrict__ picks)
{
    int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= total_frames) return;
    frame_pick_and_row(f, frame_note[f], frame_off, env_off, row_src, sample_off, f0, mask, hop, picks);
}

// The frame maps of the stem path in one launch (they were a memset and three small kernels in a row on the critical path,
// ~10 us of dispatch each): frame -> note, frame -> envelope row, the frame's (f0, mask) picks; per note the two reciprocal
// steps of the mask upsampler and the zeroed maxima the walkers reduce into.
__global__ void k_frame_maps(const int64_t *__restrict__ frame_off, const int64_t *__restrict__ env_off, int n_notes, int64_t total_frames,
                             int *__restrict__ frame_note, int64_t *__restrict__ row_src, const int64_t *__restrict__ sample_off,
                             const float *__restrict__ f0, const float *__restrict__ mask, int hop, float2 *__restrict__ picks,
                             double *__restrict__ steps, float *__restrict__ note_mag, const unsigned char *__restrict__ sparse_flags)
{
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < 2 * (int64_t)n_notes) note_mag[f] = 0.f;
    if (f < n_notes) {
        const int64_t n = sample_off[f + 1] - sample_off[f];
        const int64_t ns = (n + MASK_DS - 1) / MASK_DS;
        steps[2 * f] = n > 1 ? 1.0 / (double)(n - 1) : 0.0;
        steps[2 * f + 1] = ns > 1 ? 1.0 / (double)(ns - 1) : 0.0;
    }
    if (f >= total_frames) return;
    const int note = csr_find(frame_off, n_notes, f);
    frame_note[f] = note;
    frame_pick_and_row(f, note, frame_off, env_off, row_src, sample_off, f0, mask, hop, picks, sparse_flags);
}

// f0 *= pitch_shift (GOOFER.py:995), fp32.  1024 samples per workgroup, 16-byte accesses when the tile sits in one note.
__global__ __launch_bounds__(256) void k_scale_f0(const float *__restrict__ f0, const int64_t *__restrict__ sample_off, int n_notes,
                                                  int64_t total, const goofer_note_params *__restrict__ params, float *__restrict__ out)
{
    const sample_tile<4> t(sample_off, n_notes, total);
    if (!t.live) return;
    const int64_t g = t.g;
    const bool vec = (((uintptr_t)f0 | (uintptr_t)out) & 15) == 0;
    if (t.uniform() && g + 4 <= total && vec) {
        const float ps = params[t.lo].pitch_shift;
        float4 v = *reinterpret_cast<const float4 *>(f0 + g);
        v.x *= ps; v.y *= ps; v.z *= ps; v.w *= ps;
        *reinterpret_cast<float4 *>(out + g) = v;
        return;
    }
    for (int k = 0; k < 4 && g + k < total; ++k) out[g + k] = f0[g + k] * params[t.note(sample_off, g + k)].pitch_shift;
}

__global__ void k_note_sub_flags(const goofer_note_params *__restrict__ params, int n_notes, unsigned char *__restrict__ on_sub,
                                 unsigned char *__restrict__ on_subj)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_notes) {
        on_sub[i] = params[i].subharm_weight > 0.f;
        on_subj[i] = params[i].subharm_weight > 0.f && params[i].subharm_f0_jitter > 0.0;
    }
}

__global__ void k_note_flags(const goofer_note_params *__restrict__ params, int n_notes, unsigned char *__restrict__ on_f0,
                             unsigned char *__restrict__ on_vol)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_notes) return;
    on_f0[i] = params[i].f0_jitter > 0.0;
    on_vol[i] = params[i].vol_jitter_harm > 0.f || params[i].vol_jitter_breath > 0.f;
}

// Which pipeline synth_batch runs for a batch, decided here only (synth_batch, goofer_render_batch's warped rows,
// goofer_reserve).  goofer_amd/render.py's Renderer.run splits mixed batches by the same walkers rule.
struct synth_route {
    bool jit_f0, jit_vol, vol_vib;   // 'sh' f0 jitter; 'sr' volume jitter on harm / breath (vol_vib: its vibrato form)
    bool sub_on, sub_jit;            // 'sg' sub-harmonic pulse layer (sub_jit: with its own f0 jitter)
    bool f64_on;                     // a private fp64 copy of f0 for the jitters / the sub-harmonic trackers
    bool walkers;                    // the stem walkers (stems.hip), no spectra in HBM; else the spectra kernels, with
    bool ola_split, ola_one;         // n_fft 2048: one stem per wave (k_irfft_ola1) + per-note finish; fused overlap-add rings
    bool skip_frames;                // ola_split with the noise stems' exact sparsity decided per frame up front (k_frame_skip)
    bool side_on, early;             // the pulse chain on the side stream (early: forked from goofer_render_batch's ev_f0)
    bool f0_alias, picks_on;         // the input f0 is the scaled f0; the map kernel takes the per-frame (f0, mask) picks
    bool sparse_ok;                  // nothing of the route reads b->mask but the picks and k_mask_short, and the caller is not handed it
};

static synth_route synth_route_of(const goofer_ctx *ctx, const goofer_batch *b, const render_link &link)
{
    const goofer_plan_t &p = ctx->plan;
    synth_route r;
    r.jit_f0 = b->noise_f0 != nullptr;
    r.vol_vib = b->volume_vibrato != 0;
    r.jit_vol = r.vol_vib || (b->noise_vol_h != nullptr && b->noise_vol_b != nullptr);
    r.sub_on = b->subharm_ratio > 0.0;
    r.sub_jit = r.sub_on && b->noise_subharm != nullptr;
    // gf.synthesize behind its time stretch: f0_interp is a float64 array from there on (GOOFER.py:1053) — the f0 jitter multiplies
    // it (the pulse train sees the float32 cast of the product, :1071-1074) and the sub-harmonic trackers accumulate it (:1077-1097);
    // a private copy, since the jitters work in place
    r.f64_on = b->f0_64 != nullptr && (r.jit_f0 || r.sub_on);
    // the fused overlap-add rings index by position mod n_fft with a mask: power-of-two transforms only (768 / 1536 take the
    // separate irFFT + gather kernels; 64 .. 256: Bluestein plans), and one wave per frame (above 2048 the transform is a
    // workgroup's: the spectra-in-HBM kernels)
    const bool fused = ctx->ola_fused && p.hop % 2 == 0;
    r.ola_one = fused && (p.n_fft & (p.n_fft - 1)) == 0 && p.bl_L == 0 && p.n_fft <= 2048;
    // The spectra-in-HBM kernels stay for the other geometries, for the volume-jitter / sub-harmonic layers (which edit the
    // stems or the pulse train between the steps) and as the A/B path.
    r.walkers = fused && ctx->stems && stems_supported(p) && !r.sub_on && !r.jit_vol;
    r.ola_split = !r.walkers && fused && ctx->stems && ola_split_supported(p) && !r.jit_vol;
    r.skip_frames = r.ola_split && ctx->skip_zero && ctx->overlap && !r.sub_on && p.hop <= 512;
    r.side_on = ctx->overlap && r.ola_one && !r.sub_on;
    r.early = r.side_on && !r.jit_f0 && link.fork_early && link.f0_ready == b->f0 && ctx->side != nullptr;
    // f0 * pitch_shift (GOOFER.py:995).  When the caller vouches that every pitch_shift is 1 (the resampler path: the pitch
    // lives in the curve) and nothing jitters f0 in place, the input array IS the scaled f0 and the pass is skipped.
    r.f0_alias = b->unit_pitch_shift && !r.jit_f0 && !r.sub_jit;
    // the picks ride on the map kernel when the scaled f0 is final at that point of the caller's stream: nothing jitters it in
    // place later, and it is not being produced on the side stream
    r.picks_on = !r.jit_f0 && !r.sub_jit && !(r.early && !r.f0_alias);
    // The voicing mask may stay sparse (render_link::mask_sparse) on the walker route — no sub-harmonic layer, no volume jitter, and the
    // spectra routes' k_harm_shape / k_noise_spectra are not run — without the f0 jitter, which reads it sample by sample, in a
    // mix_only batch: there the per-sample arrays of the call are scratch to the caller (goofer_batch::mix_only), the mask with them.
    r.sparse_ok = ctx->mask_sparse && r.walkers && !r.jit_f0 && !r.jit_vol && !r.sub_on && !r.sub_jit && b->mix_only && (b->mix || b->rec);
    return r;
}

// The scratch of one goofer_synth_batch, in arena order.  Pieces a route does not use are null or empty.
struct synth_scratch {
    size_t slots, spec, tframes, env_noise;   // element counts: onset slots, spectrum / time-frame / noise-envelope floats
    int *frame_note;
    int64_t *row_src;
    float2 *picks, *S_h, *S_uv, *S_br;
    float *f0s, *pulse, *frames, *frames_u, *frames_b, *env_h, *env_n, *note_mag, *note_peak;
    onset_t *onsets;
    int32_t *onset_idx, *onset_cnt, *pulse_tiles;
    double *short_s, *note_steps, *inc = nullptr, *jit_a = nullptr, *jit_b = nullptr, *jit_c = nullptr, *sub_buf = nullptr,
           *sub_fm = nullptr, *f0d = nullptr;
    unsigned long long *jit_max = nullptr, *sub_max = nullptr;
    unsigned char *hopz, *hop_flat = nullptr, *frame_skip = nullptr, *knot_eq = nullptr, *on_f0 = nullptr, *on_vol = nullptr,
                  *on_sub = nullptr, *on_subj = nullptr;
};

static void carve_synth(arena &a, const goofer_plan_t &p, const synth_route &r, int64_t F, int64_t N, int n, int ld, synth_scratch &s)
{
    s.slots = onset_slots(N, n, r.sub_on);
    s.spec = r.walkers ? 0 : (size_t)F * spec_stride(p.n_bins);
    s.tframes = r.walkers ? 0 : (size_t)F * p.n_fft;
    s.env_noise = r.walkers ? 0 : (size_t)F * ld;
    s.frame_note = a.take<int>(F);
    s.row_src = a.take<int64_t>(F);
    s.picks = a.take<float2>(F);                              // per-frame (f0, mask) picks
    s.f0s = a.take<float>(N);                                 // f0 scaled
    if (r.sub_on) s.inc = a.take<double>(N);                  // increments of the sub-harmonic trackers
    s.onsets = (onset_t *)a.take<char>(s.slots * ONSET_BYTES);
    s.onset_idx = a.take<int32_t>(s.slots);                   // raw onset sample indices
    s.onset_cnt = a.take<int32_t>(n + 16);
    s.pulse = a.take<float>(N);
    s.pulse_tiles = a.take<int32_t>((size_t)PULSE_TILE_INTS(N));   // pulse placement: 4 ints per tile
    s.S_h = a.take<float2>(s.spec); s.S_uv = a.take<float2>(s.spec); s.S_br = a.take<float2>(s.spec);
    s.frames = a.take<float>(s.tframes); s.frames_u = a.take<float>(s.tframes); s.frames_b = a.take<float>(s.tframes);
    s.env_h = a.take<float>((size_t)F * ld);
    s.env_n = a.take<float>(s.env_noise);
    s.short_s = a.take<double>(N / 4 + n + 16);               // smoothed decimated mask
    s.note_mag = a.take<float>(2 * (size_t)n + 16);           // note_mag, note_peak
    s.note_steps = a.take<double>(2 * (size_t)n + 16);        // per-note linspace steps
    // stem walkers: a byte per output hop of a note (T + 3 of them) — which stems the noise walker left unstored because they are
    // exactly zero there (k_noise_stems -> k_note_finish)
    s.hopz = a.take<unsigned char>(r.walkers ? (size_t)F + 3 * (size_t)n + 64 : 0);
    if (r.skip_frames) {                                      // per-hop flatness, per-frame skip bits, knot equalities
        s.hop_flat = a.take<unsigned char>((size_t)F + (size_t)((p.n_fft + p.hop - 1) / p.hop) * n + 16);
        s.frame_skip = a.take<unsigned char>((size_t)F + 16);
        s.knot_eq = a.take<unsigned char>((size_t)(N / 4 + n + 16));
    }
    if (r.jit_f0 || r.jit_vol || r.sub_jit) {
        s.jit_a = a.take<double>(N); s.jit_b = a.take<double>(N); s.jit_c = a.take<double>(N);
        s.jit_max = a.take<unsigned long long>(3 * (size_t)n + 16); s.on_f0 = a.take<unsigned char>(n + 16); s.on_vol = a.take<unsigned char>(n + 16);
    }
    if (r.sub_on) {
        s.sub_buf = a.take<double>(N); s.sub_fm = a.take<double>(N); s.sub_max = a.take<unsigned long long>(n + 16);
        s.on_sub = a.take<unsigned char>(n + 16); s.on_subj = a.take<unsigned char>(n + 16);
    }
    if (r.f64_on) s.f0d = a.take<double>(N);
}

static int ensure_side_stream(goofer_ctx *ctx)
{
    if (ctx->side) return GOOFER_OK;
    {
        // the pulse chain (f0 kernel -> onsets -> placement) is the longest dependency chain of a step and shares the chip with
        // the envelope kernels and the noise walker of the caller's stream: its workgroups go first (highest stream priority)
        int least = 0, greatest = 0;
        HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->side, hipStreamNonBlocking, greatest));
    }
    hipEvent_t *evs[] = {&ctx->ev_fork, &ctx->ev_join, &ctx->ev_maps, &ctx->ev_entry, &ctx->ev_f0, &ctx->ev_f0s};
    for (hipEvent_t *e : evs)
        if (!*e) HIP_TRY(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming));
    return GOOFER_OK;
}

// Per-stage timing of one goofer_synth_batch: stage s runs from event s to event s + 1 on the caller's stream.  Option
// "prof_only" = s records only the events stage s needs (bench.py's timed steps carry the dominant kernel's two events; the
// twenty records of the full breakdown cost 0.06 ms of a 2.3 ms step).  When the pulse chain runs on the side stream it is
// bracketed there (prof_side), and the two kernels launched beside it on the caller's stream (stages 6 / 7 of the stem path,
// 9 / 12 of the other) by the prof_main2 pair.
struct stage_clock {
    goofer_ctx *ctx;
    hipStream_t st;
    bool side;
    bool timed;                 // this step is profiled: it records into step prof_steps of the pools
    int next = 0;               // the stage whose opening event comes next

    stage_clock(goofer_ctx *c, hipStream_t s, const synth_route &r)
        : ctx(c), st(s), side(r.side_on), timed(c->prof_on && c->prof_steps < c->prof_cap)
    {
        if (timed) ctx->prof_stems = r.walkers;
        if (side || timed) ctx->prof_side_used = side;
    }
    int record(bool want, const event_pool &pool, int i, hipStream_t on)
    {
        if (timed && want) HIP_TRY(ctx, hipEventRecord(pool.step(ctx->prof_steps)[i], on));
        return GOOFER_OK;
    }
    // open stage s, after the (empty) stages skipped on the way; close(): end the last one
    int at(int s)
    {
        const int o = ctx->prof_only;
        for (int rc; next <= s; ++next)
            if ((rc = record(o < 0 || next == o || next == o + 1 || (next == 5 && (o == 6 || o == 9)), ctx->prof_ev, next, st))) return rc;
        return GOOFER_OK;
    }
    int close()
    {
        const int rc = at(PROF_STAGES);
        if (!rc && timed) ctx->prof_steps++;
        return rc;
    }
    // boundary k of the pulse chain on the side stream; the end of the q-th kernel launched beside it on the caller's stream
    int pulse(int k, hipStream_t pst) { return record(side && in(3, 5), ctx->prof_side, k, pst); }
    int beside(int q) { return record(in(6, 7) || in(9, 9) || in(12, 12), ctx->prof_main2, q, st); }
    bool in(int lo, int hi) const { return ctx->prof_only < 0 || (ctx->prof_only >= lo && ctx->prof_only <= hi); }
};

// One goofer_synth_batch in flight: what the driver hands to its route's tail, and the launches written once for both
struct synth_call {
    goofer_ctx *ctx;
    const goofer_batch *b;
    const render_link &link;
    const synth_route &r;
    synth_scratch &s;
    stage_clock &clk;
    hipStream_t st;
    int64_t F, N;
    int n;

    // the flag bytes the mask is to be read through (mask_value), or null: the mask is whole
    const unsigned char *sparse_flags() const { return link.mask_sparse ? link.tile_flags : nullptr; }
    int mask_short() const
    {
        // (link.tile_flags: goofer_render_batch, the flags of b->mask as the f0 kernel wrote it — no kernel of any route writes the mask)
        return launch_mask_short(ctx, b->mask, b->sample_off, n, N, ctx->mask_taps, ctx->mask_taps_radius, ctx->mask_taps_sum, s.short_s,
                                 link.tile_flags, ctx->ovf_flag ? ctx->ovf_flag + MASK_COUNTERS : nullptr, link.mask_sparse, st);
    }
    int late_picks() const
    {
        return r.picks_on ? GOOFER_OK : launch_frame_picks(ctx, b->frame_off, s.frame_note, F, b->sample_off, s.f0s, b->mask, sparse_flags(), s.picks, st);
    }
    // aperiodic half of the stem-split path: the two noise stems straight to samples (needs the smoothed mask knots and the final
    // scaled f0, nothing of the pulse chain)
    int noise_walker() const
    {
        return launch_noise_stems(ctx, b->env_noise ? b->env_noise : b->env, b->ld, s.row_src, b->phi, F, s.frame_note, b->frame_off,
                                  b->sample_off, s.picks, b->params, b->seed, b->env_noise != nullptr, s.short_s, s.note_steps, b->uv,
                                  b->bre, s.hopz, st);
    }
    // (frame_skip is null unless skip_frames, which runs on the side-stream route)
    int noise_spectra() const
    {
        return launch_noise_spectra(ctx, s.S_uv, s.S_br, spec_stride(ctx->plan.n_bins), F, s.frame_note, b->frame_off, b->sample_off, s.f0s,
                                    b->mask, b->env_noise ? b->env_noise : b->env, b->phi, b->ld, b->params, b->seed, s.row_src,
                                    b->env_noise != nullptr, s.frame_skip, r.picks_on ? s.picks : nullptr, st);
    }
    // Harmonic envelope rows for the harmonic walker: formant-anchored + uniform warp, one wave per row (GOOFER.py:1004-1017).
    // Not inside the walker: the crossing-anchor path is several times slower than the sorted one, and a walker wave holds
    // ~95 frames of ONE note, so the slow notes would set the kernel's time.
    int warp(hipStream_t on) const
    {
        return launch_warp_bins(ctx, b->env, s.env_h, F, ctx->plan.n_bins, b->ld, b->formants, nullptr, b->params, s.frame_note, s.row_src,
                                1.0, on);
    }
    bool keep_stems() const { return !(b->mix_only && (b->mix || b->rec)); }

    // The stem walkers after the pulse chain: mask smoothing, noise walker and warp (unless they ran beside the pulse chain), the
    // harmonic walker, the per-note finish
    int walker_tail()
    {
        int rc;
        if ((rc = clk.at(6))) return rc;                        // 6: mask_short
        if (!r.side_on && (rc = mask_short())) return rc;
        if ((rc = clk.at(7))) return rc;                        // 7: noise_stems
        if (!r.side_on) {
            if ((rc = late_picks())) return rc;
            if ((rc = noise_walker())) return rc;
            if (!link.warped && (rc = warp(st))) return rc;
        }
        if ((rc = clk.at(9))) return rc;                        // 9: harm_stem = rFFT + shaping + irFFT + overlap-add of the harmonic stem
        // (goofer_render_batch: the assembly already wrote the warped rows)
        if ((rc = launch_harm_stem(ctx, s.pulse, link.warped ? ctx->warp_rows : s.env_h, link.warped ? b->env : nullptr, b->formants != nullptr,
                                   b->ld, link.warped ? s.row_src : nullptr, F, s.frame_note, b->frame_off, b->sample_off, s.picks, b->params,
                                   b->harm, s.note_mag, st)))
            return rc;
        if ((rc = clk.at(13))) return rc;                       // 13: harm / max|S|, peak, gain, reconstruct, mix
        if ((rc = launch_note_finish(ctx, b->harm, b->uv, b->bre, b->rec, b->mix, b->sample_off, n, b->params, s.note_mag, s.note_peak,
                                     keep_stems(), s.hopz, b->frame_off, st)))
            return rc;
        return clk.close();
    }

    // The spectra in HBM after the pulse chain: rFFT, shaping, irFFTs, then the overlap-add (one stem per wave, three, or separate
    // kernels) with the gains, the volume jitter, the gain
    int spectra_tail()
    {
        const int ldc = spec_stride(ctx->plan.n_bins);
        int rc;
        if ((rc = clk.at(6))) return rc;                        // 6: framewise rFFT of the pulse train
        if ((rc = launch_rfft_frames_mapped(ctx, s.pulse, b->sample_off, b->frame_off, s.frame_note, F, s.S_h, ldc, st))) return rc;
        if ((rc = clk.at(7))) return rc;
        if ((rc = launch_harm_shape(ctx, s.S_h, ldc, F, s.frame_note, b->frame_off, b->sample_off, s.f0s, b->mask, b->env, b->ld, b->params,
                                    s.note_mag, s.row_src, b->formants, b->no_warp != 0, r.picks_on ? s.picks : nullptr, st)))
            return rc;
        if ((rc = clk.at(8))) return rc;
        if (!r.ola_one && (rc = launch_irfft_frames(ctx, s.S_h, ldc, F, s.frames, st))) return rc;
        if ((rc = clk.at(9))) return rc;                        // 9: aperiodic spectra
        if (!r.side_on && (rc = noise_spectra())) return rc;
        if ((rc = clk.at(10))) return rc;
        if (!r.ola_one && (rc = launch_irfft_frames(ctx, s.S_br, ldc, F, s.frames_b, st))) return rc;
        if ((rc = clk.at(11))) return rc;
        if (!r.ola_one && (rc = launch_irfft_frames(ctx, s.S_uv, ldc, F, s.frames_u, st))) return rc;
        if ((rc = clk.at(12))) return rc;                       // 12: decimated + smoothed voicing mask
        if (!r.side_on && (rc = mask_short())) return rc;
        if ((rc = clk.at(13))) return rc;                       // 13: (irFFT of the three stems +) overlap-add + gains + per-note peak
        if (r.ola_split) {
            if ((rc = launch_irfft_ola1(ctx, s.S_h, s.S_uv, s.S_br, ldc, F, s.frame_note, b->frame_off, b->sample_off, n, s.short_s, s.note_steps,
                                        b->params, b->harm, b->uv, b->bre, s.frame_skip, st)))
                return rc;
            if ((rc = clk.at(14))) return rc;
            if ((rc = launch_note_finish(ctx, b->harm, b->uv, b->bre, b->rec, b->mix, b->sample_off, n, b->params, s.note_mag, s.note_peak,
                                         keep_stems(), nullptr, nullptr, st)))
                return rc;
            return clk.close();
        }
        if (r.ola_one) {
            if ((rc = launch_irfft_ola3(ctx, s.S_h, s.S_uv, s.S_br, ldc, F, s.frame_note, b->frame_off, b->sample_off, n, s.note_mag, s.short_s,
                                        s.note_steps, b->params, b->harm, b->uv, b->bre, s.note_peak, st)))
                return rc;
        } else if ((rc = launch_ola3_gains(ctx, s.frames, s.frames_u, s.frames_b, s.note_mag, s.short_s, b->sample_off, b->frame_off, n, N,
                                           b->params, s.note_steps, b->harm, b->uv, b->bre, s.note_peak, st)))
            return rc;
        if (r.jit_vol) {  // 'sr': volume jitter on harm / breath, then the peak is taken again (GOOFER.py:1185-1193)
            const double *d_t = nullptr, *d_t20; int rt = 0, r20;
            if (!r.vol_vib && (rc = upload_jitter_taps(ctx, (double)b->vol_jitter_sigma, 1, &d_t, &rt, st))) return rc;
            if ((rc = upload_jitter_taps(ctx, 20.0, 2, &d_t20, &r20, st))) return rc;
            if (!r.vol_vib) {
                if ((rc = launch_gauss_samples<double>(ctx, b->noise_vol_h, b->sample_off, n, N, d_t, rt, s.on_vol, s.jit_a, st))) return rc;
                if ((rc = launch_gauss_samples<double>(ctx, b->noise_vol_b, b->sample_off, n, N, d_t, rt, s.on_vol, s.jit_b, st))) return rc;
                if ((rc = launch_note_absmax(ctx, s.jit_a, b->sample_off, n, N, s.on_vol, s.jit_max + n, st))) return rc;
                if ((rc = launch_note_absmax(ctx, s.jit_b, b->sample_off, n, N, s.on_vol, s.jit_max + 2 * (size_t)n, st))) return rc;
            }
            if ((rc = launch_gauss_samples<float>(ctx, b->mask, b->sample_off, n, N, d_t20, r20, s.on_vol, s.jit_c, st))) return rc;
            if ((rc = launch_volume_jitter(ctx, b->harm, b->bre, s.jit_a, s.jit_b, s.jit_c, s.jit_max + n, s.jit_max + 2 * (size_t)n, b->sample_off,
                                           n, N, b->params, r.vol_vib ? 1 : 0, (double)b->vol_jitter_speed, st)))
                return rc;
            HIP_TRY(ctx, hipMemsetAsync(s.note_peak, 0, (size_t)n * sizeof(float), st));
            if ((rc = launch_stem_peak(ctx, b->harm, b->uv, b->bre, b->sample_off, n, N, s.note_peak, st))) return rc;
        }
        if ((rc = clk.at(14))) return rc;                       // 14: gain, reconstruct, mix
        if ((rc = launch_apply_gain(ctx, b->harm, b->uv, b->bre, b->rec, b->mix, b->sample_off, n, N, b->params, s.note_peak, keep_stems(), st)))
            return rc;
        return clk.close();
    }
};

// goofer_assemble_batch; under goofer_render_batch `link` carries what the synthesis wants of it and takes what it did
static int assemble_batch(goofer_ctx *ctx, const goofer_assembly *asmb, render_link &link, hipStream_t st)
{
    if (asmb->n_notes <= 0) return GOOFER_OK;
    if (asmb->ld < asmb->n_bins || asmb->max_K < 2 || asmb->max_K > 4096) return goofer_fail(ctx, GOOFER_EINVAL, "bad assembly geometry");
    if (asmb->n_bins > 1025) return goofer_fail(ctx, GOOFER_EINVAL, "the resampler's assembly takes n_fft <= 2048 (%d bins)", asmb->n_bins);
    if (asmb->any_fry && ctx->plan.hop <= 0) return goofer_fail(ctx, GOOFER_EINVAL, "the fry envelope warp needs goofer_plan first");
    goofer_assembly a = *asmb;
    // the row -> note maps (map_out right behind map_edit, 64 ints of padding behind both), the edited rows unless the caller
    // gives them, the per-row records of k_row_recs / k_env_rows; 4 KiB behind the last piece
    int *map_edit;
    float *edit_rows;
    char *recs;
    unsigned char *flags;
    const bool want_flags = link.want_tile_flags && a.mask_out && a.total_samples > 0;
    int2 *tile_notes;
    const bool want_table = ctx->sa_table && a.total_samples > 0;
    int rc = carve_block(ctx, &ctx->asm_scratch, &ctx->asm_bytes, "assembly scratch", [&](arena &m) {
        map_edit = m.take<int>((size_t)(a.total_edit_rows + a.total_out_rows) + 64);
        edit_rows = m.take<float>(a.edit_rows ? 0 : (size_t)a.total_edit_rows * a.ld);
        // (whatever "value_f64" says: launch_assemble runs k_row_recs / k_env_rows under either arithmetic)
        recs = m.take<char>((size_t)a.total_out_rows * env_row_rec_bytes());
        // goofer_render_batch: a word per SA_TILE samples of the mask, written by the f0 / mask kernel for k_mask_short
        flags = m.take<unsigned char>(want_flags ? 4 * (size_t)((a.total_samples + SA_TILE - 1) / SA_TILE) + 64 : 0);
        // the notes of each SA_TILE tile's first and last sample, written by k_sample_tile_notes for the f0 / mask kernel
        tile_notes = m.take<int2>(want_table ? (size_t)((a.total_samples + SA_TILE - 1) / SA_TILE) : 0);
    });
    if (rc) return rc;
    link.tile_flags_dst = want_flags ? flags : nullptr;
    if (!want_flags) link.mask_sparse = false;                // no bytes to say what was left out: the mask is written in full
    if (!a.edit_rows) a.edit_rows = edit_rows;
    return launch_assemble(ctx, &a, map_edit, map_edit + a.total_edit_rows, recs, want_table ? tile_notes : nullptr, link, st);
}

// goofer_synth_batch; under goofer_render_batch `link` says what the assembly in front of it left: an f0 event to fork the pulse
// chain from, f0 / mask still in flight on the side stream, the harmonic walker's warped rows
static int synth_batch(goofer_ctx *ctx, const goofer_batch *b, render_link &link, hipStream_t st)
{
    const goofer_plan_t &p = ctx->plan;
    if (b->n_bins != p.n_bins || b->ld < p.n_bins) return goofer_fail(ctx, GOOFER_EINVAL, "batch geometry does not match the plan");
    if (b->n_notes <= 0 || b->total_samples <= 0) return GOOFER_OK;
    const int64_t F = b->total_frames, N = b->total_samples;
    const int n = b->n_notes;
    const synth_route r = synth_route_of(ctx, b, link);
    if (link.mask_sparse && !(r.sparse_ok && link.tile_flags))
        return goofer_fail(ctx, GOOFER_EINVAL, "the mask was left sparse for a route that reads it in full");
    synth_scratch s;
    int rc = carve_scratch(ctx, [&](arena &a) { carve_synth(a, p, r, F, N, n, b->ld, s); });
    if (rc) return rc;
    s.note_peak = s.note_mag + n;
    if (r.f64_on) HIP_TRY(ctx, hipMemcpyAsync(s.f0d, b->f0_64, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (r.f0_alias) s.f0s = const_cast<float *>(b->f0);
    // the debug views (goofer_debug_fetch); frame_skip per frame: bit 0 unvoiced, bit 1 breath transform skipped
    const void *views[16] = {s.frame_note, s.row_src, s.f0s, s.pulse, s.S_h, s.S_uv, s.S_br, s.frames, s.env_h, s.env_n, s.short_s,
                             s.note_mag, s.note_peak, s.onset_cnt, s.onset_idx, s.frame_skip};
    const size_t view_bytes[16] = {F * sizeof(int), F * sizeof(int64_t), N * sizeof(float), N * sizeof(float), s.spec * sizeof(float2),
                                   s.spec * sizeof(float2), s.spec * sizeof(float2), s.tframes * sizeof(float), (size_t)F * b->ld * sizeof(float),
                                   s.env_noise * sizeof(float), (N / 4 + n) * sizeof(double), n * sizeof(float), n * sizeof(float),
                                   n * sizeof(int32_t), s.slots * sizeof(int32_t), s.frame_skip ? (size_t)F : 0};
    for (int i = 0; i < 16; ++i) { ctx->dbg_ptr[i] = views[i]; ctx->dbg_bytes[i] = view_bytes[i]; }
    ctx->dbg_ptr[16] = s.picks;                               // view 16: the per-frame (f0, mask) picks
    ctx->dbg_bytes[16] = F * sizeof(float2);

    // mask-smoothing taps for this call's sigma; device copy cached on the handle (steady state:
    // no host work, no synchronisation)
    if (ctx->mask_taps_sigma != b->transition_sigma || !ctx->mask_taps) {
        std::vector<double> mtaps;
        int mrad;
        gauss_taps_host(std::max(1.0, (double)b->transition_sigma / 4.0), mtaps, mrad);   // GOOFER.py:561
        if (mrad > 2048) return goofer_fail(ctx, GOOFER_EINVAL, "transition sigma too large");
        HIP_TRY(ctx, hipDeviceSynchronize());
        if ((rc = grow_block(ctx, (void **)&ctx->mask_taps, &ctx->mask_taps_bytes, 4097 * sizeof(double), "mask taps"))) return rc;
        HIP_TRY(ctx, hipMemcpy(ctx->mask_taps, mtaps.data(), mtaps.size() * sizeof(double), hipMemcpyHostToDevice));
        ctx->mask_taps_sigma = b->transition_sigma;
        ctx->mask_taps_radius = mrad;
        double acc = 0.0;
        for (double tv : mtaps) acc += tv * 1.0;
        ctx->mask_taps_sum = acc;
    }

    stage_clock clk(ctx, st, r);
    synth_call c{ctx, b, link, r, s, clk, st, F, N, n};
    // goofer_render_batch ran the f0 / mask kernel on the side stream: the caller's stream reads them from here on
    if (link.f0_side) {
        HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_f0, 0));
        link.f0_side = false;
    }
    if (!r.walkers) HIP_TRY(ctx, hipMemsetAsync(s.note_mag, 0, 2 * (size_t)n * sizeof(float), st));
    if ((rc = clk.at(0))) return rc;                          // 0: setup
    // goofer_render_batch: the assembly recorded ev_f0 right after the f0 / mask kernel.  The pulse chain (f0 scaling,
    // sequential walk, placement) then runs on the side stream from that point on, beside the envelope assembly and the
    // map kernels, instead of starting when this call's first kernel is reached in stream order.
    if (r.early) {
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_entry, 0));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_f0, 0));
        if (!r.f0_alias && (rc = launch_per_sample(ctx, k_scale_f0, N, 1024, 0, ctx->side, b->f0, b->sample_off, n, N, b->params, s.f0s))) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_f0s, ctx->side));
    }
    if (!r.walkers && (rc = launch_frame_note(ctx, b->frame_off, n, F, s.frame_note, st))) return rc;
    // (the pulse walk divides by sr itself)
    if (!r.early && !r.f0_alias && (rc = launch_per_sample(ctx, k_scale_f0, N, 1024, 0, st, b->f0, b->sample_off, n, N, b->params, s.f0s))) return rc;
    if (r.walkers) {   // the stem walkers' frame maps in one launch
        const int64_t threads = std::max<int64_t>(F, 2 * (int64_t)n);
        hipLaunchKernelGGL(k_frame_maps, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, b->frame_off, b->env_off, n, F, s.frame_note,
                           s.row_src, b->sample_off, (const float *)s.f0s, b->mask, p.hop, r.picks_on ? s.picks : (float2 *)nullptr, s.note_steps,
                           s.note_mag, c.sparse_flags());
    } else {
        hipLaunchKernelGGL(k_row_src, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, b->frame_off, b->env_off, s.frame_note, F, s.row_src,
                           b->sample_off, (const float *)s.f0s, b->mask, p.hop, r.picks_on ? s.picks : (float2 *)nullptr);
    }
    LAUNCH_CHECK(ctx);
    if (r.jit_f0 || r.jit_vol) {
        hipLaunchKernelGGL(k_note_flags, dim3((n + 255) / 256), dim3(256), 0, st, b->params, n, s.on_f0, s.on_vol);
        LAUNCH_CHECK(ctx);
        HIP_TRY(ctx, hipMemsetAsync(s.jit_max, 0, 3 * (size_t)n * sizeof(unsigned long long), st));
    }
    if (r.jit_f0) {   // 'sh': f0 *= 1 + (jitter - 1) * mask, after pitch_shift and before the pulse train (GOOFER.py:1069-1071)
        const double *d_t; int rt;
        if ((rc = upload_jitter_taps(ctx, (double)b->f0_jitter_sigma, 0, &d_t, &rt, st))) return rc;
        if ((rc = launch_gauss_samples<double>(ctx, b->noise_f0, b->sample_off, n, N, d_t, rt, s.on_f0, s.jit_a, st))) return rc;
        if ((rc = launch_note_absmax(ctx, s.jit_a, b->sample_off, n, N, s.on_f0, s.jit_max, st))) return rc;
        if ((rc = launch_f0_jitter(ctx, s.f0s, s.f0d, b->mask, s.jit_a, s.jit_max, b->sample_off, n, N, b->params, 0, st))) return rc;
    }
    // The pulse walk is one latency-bound wave per SIMD: it goes to a side stream FIRST (so its workgroups are resident
    // from the start), and the aperiodic branch — noise, mask smoothing, which depend only on the maps and the scaled f0 —
    // fills the rest of the machine from the caller's stream meanwhile.
    hipStream_t pst = st;                                     // stream of the pulse chain
    if (r.side_on) {
        if ((rc = ensure_side_stream(ctx))) return rc;
        if (r.walkers && !link.warped) HIP_TRY(ctx, hipEventRecord(ctx->ev_maps, st));   // the frame maps and everything before them on this stream (for k_warp_bins)
        if (!r.early) {
            HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, st));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
        }
        pst = ctx->side;
    }
    // 1: noise envelope = sigma-1.75 blur of the un-warped rows (GOOFER.py:993), 2: harmonic envelope = formant-anchored +
    // uniform warp (folded into the shaping kernels / walkers: the standalone envelope kernels remain as C-ABI entry points)
    if ((rc = clk.at(3))) return rc;                          // 3..5: pulse train
    if ((rc = clk.pulse(0, pst))) return rc;
    if ((rc = clk.at(4))) return rc;
    if ((rc = clk.pulse(1, pst))) return rc;
    // stage 4 holds the fused kernel (scan, periods and placement per note) and stage 5 is empty, or the four kernels share them
    const bool pulse_fused = ctx->pulse_scan != 0 && ctx->pulse_fused;
    if (pulse_fused) {
        if ((rc = launch_pulse_note(ctx, s.f0s, 1.0f, b->sample_off, n, s.onsets, s.onset_idx, s.onset_cnt, ctx->ovf_flag, s.pulse, pst))) return rc;
    } else if ((rc = launch_pulse_onsets(ctx, s.f0s, 1.0f, b->sample_off, n, s.onsets, s.onset_idx, s.onset_cnt, ctx->ovf_flag, N, s.pulse_tiles, pst))) {
        return rc;
    }
    if ((rc = clk.at(5))) return rc;
    if ((rc = clk.pulse(2, pst))) return rc;
    if (!pulse_fused && (rc = launch_pulse_place(ctx, s.onsets, s.onset_cnt, b->sample_off, n, N, s.pulse, s.pulse_tiles, pst))) return rc;
    if (r.side_on) {
        // the warp behind the pulse placement on its stream (the caller's stream carries the mask smoothing and the noise walker)
        if (r.walkers && !link.warped) {
            HIP_TRY(ctx, hipStreamWaitEvent(pst, ctx->ev_maps, 0));   // frame_note / row_src come from the caller's stream
            if ((rc = c.warp(pst))) return rc;
        }
        if ((rc = clk.pulse(3, pst))) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_join, pst));
        // meanwhile, on the caller's stream
        if (r.early && !r.f0_alias) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_f0s, 0));   // the scaled f0 comes from the side stream
        if (r.walkers) {
            if ((rc = c.late_picks()) || (rc = c.mask_short()) || (rc = clk.beside(0)) || (rc = c.noise_walker()) || (rc = clk.beside(1)))
                return rc;
        } else {
            // (the skip bits need the smoothed mask: it goes first then)
            if (r.skip_frames) {
                if ((rc = c.mask_short())) return rc;
                if ((rc = launch_frame_skip(ctx, s.short_s, N / 4 + n, b->sample_off, b->frame_off, s.frame_note, n, F, s.knot_eq, s.hop_flat,
                                            s.frame_skip, st)))
                    return rc;
            }
            if ((rc = c.noise_spectra()) || (rc = clk.beside(0))) return rc;
            if (!r.skip_frames && (rc = c.mask_short())) return rc;
            if ((rc = clk.beside(1))) return rc;
        }
        HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_join, 0));
    }
    if (r.sub_on) {   // 'sg': extra LF pulse layer at f0 * ratio with vibrato, added to the pulse train (GOOFER.py:1076-1097)
        hipLaunchKernelGGL(k_note_sub_flags, dim3((n + 255) / 256), dim3(256), 0, st, b->params, n, s.on_sub, s.on_subj);
        LAUNCH_CHECK(ctx);
        HIP_TRY(ctx, hipMemsetAsync(s.sub_max, 0, (size_t)n * sizeof(unsigned long long), st));
        if (r.sub_jit) {   // subharm_f0_jitter: f0 (the array itself, as in the reference) *= 1 + (jitter - 1) * mask   :1078-1080
            const double *d_t; int rt;
            if ((rc = upload_jitter_taps(ctx, (double)b->f0_jitter_sigma, 0, &d_t, &rt, st))) return rc;
            HIP_TRY(ctx, hipMemsetAsync(s.jit_max, 0, (size_t)n * sizeof(unsigned long long), st));
            if ((rc = launch_gauss_samples<double>(ctx, b->noise_subharm, b->sample_off, n, N, d_t, rt, s.on_subj, s.jit_a, st))) return rc;
            if ((rc = launch_note_absmax(ctx, s.jit_a, b->sample_off, n, N, s.on_subj, s.jit_max, st))) return rc;
            if ((rc = launch_f0_jitter(ctx, s.f0s, s.f0d, b->mask, s.jit_a, s.jit_max, b->sample_off, n, N, b->params, 1, st))) return rc;
        }
        double ratios[16];
        ratios[0] = b->subharm_ratio;
        for (int q = 0; q < 15; ++q) ratios[q + 1] = b->subharm_more[q];
        int n_ratios = 1;
        while (n_ratios < 16 && ratios[n_ratios] > 0.0) ++n_ratios;
        if ((rc = launch_subharm(ctx, s.f0s, s.f0d, b->mask, b->sample_off, n, N, b->params, ratios, n_ratios, b->subharm_vibrato,
                                 b->subharm_vib_rate, b->subharm_vib_depth, b->subharm_vib_delay, s.sub_fm, s.inc, s.onsets,
                                 s.onset_idx, s.onset_cnt, ctx->ovf_flag, s.on_sub, s.sub_buf, s.sub_max, s.pulse, st)))
            return rc;
    }
    return r.walkers ? c.walker_tail() : c.spectra_tail();
}

extern "C" {

int goofer_reserve(goofer_ctx *ctx, int64_t max_frames, int64_t max_samples, int64_t max_notes)
{
    if (!ctx) return GOOFER_EINVAL;
    const goofer_plan_t &p = ctx->plan;
    if (!p.n_fft) return goofer_fail(ctx, GOOFER_ENOPLAN, "goofer_plan first");
    goofer_batch plain = {};
    plain.total_frames = max_frames;
    plain.total_samples = max_samples;
    plain.n_notes = (int)max_notes;
    synth_route r = synth_route_of(ctx, &plain, render_link());
    // the spectra routes keep room for the 'sg' layer (one onset slot per sample, the trackers) and the skip bits as well
    if (!r.walkers) r.sub_on = r.skip_frames = true;
    synth_scratch s;
    arena count{nullptr, 0};
    carve_synth(count, p, r, max_frames, max_samples, (int)max_notes, (p.n_bins + 3) & ~3, s);
    return grow_block(ctx, &ctx->scratch, &ctx->scratch_bytes, count.used + 8192, "scratch");   // (never less than the hand-summed size it replaces)
}

int goofer_assemble_batch(goofer_ctx *ctx, const goofer_assembly *asmb, void *stream)
{
    if (!ctx || !asmb) return GOOFER_EINVAL;
    render_link none;
    return assemble_batch(ctx, asmb, none, (hipStream_t)stream);
}

int goofer_synth_batch(goofer_ctx *ctx, const goofer_batch *b, void *stream)
{
    NEED_PLAN(ctx);
    if (!b) return goofer_fail(ctx, GOOFER_EINVAL, "null batch");
    render_link none;
    return synth_batch(ctx, b, none, (hipStream_t)stream);
}

// SillySampler.resample end to end for one batch (SillySampler.py:698-1151 up to the post chain): assembly and synthesis as
// one call.  Same kernels and results as goofer_assemble_batch followed by goofer_synth_batch; the difference is scheduling.
// Because both descriptors are in hand at once, everything they point to is known to be enqueued before this call, so
// the synthesis' pulse chain may start on the side stream as soon as the assembled f0 exists.
int goofer_render_batch(goofer_ctx *ctx, const goofer_assembly *asmb, const goofer_batch *b, void *stream)
{
    NEED_PLAN(ctx);
    if (!asmb || !b) return goofer_fail(ctx, GOOFER_EINVAL, "null descriptor");
    if (ctx->plan.n_fft > 2048) return goofer_fail(ctx, GOOFER_EINVAL, "the resampler's render takes n_fft <= 2048 (the plan has %d)", ctx->plan.n_fft);
    hipStream_t st = (hipStream_t)stream;
    render_link link;
    int rc;
    if (ctx->overlap && asmb->f0_out == b->f0 && asmb->n_notes > 0) {
        if ((rc = ensure_side_stream(ctx))) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_entry, st));      // every input of either descriptor precedes this point
        link.fork_early = true;
    }
    // Stem-split path: the harmonic walker wants warped envelope rows.  The assembly's frame-gather kernel has every row in
    // hand, so it writes the warped copy too (k_env_rows<true>) — one pass instead of a separate read + write of the matrix.
    // (the other routes warp in k_harm_shape: a warped copy written here would never be read)
    if (synth_route_of(ctx, b, link).walkers && ctx->overlap && asmb->env_out == b->env && asmb->n_notes == b->n_notes &&
        asmb->total_out_rows == b->total_env_rows && asmb->ld == b->ld && !asmb->any_fry) {
        const size_t need = (size_t)b->total_env_rows * b->ld * sizeof(float);
        if (need > ctx->warp_rows_bytes &&                                            // grown with 25 % to spare
            (rc = grow_block(ctx, (void **)&ctx->warp_rows, &ctx->warp_rows_bytes, need + need / 4, "warped rows")))
            return rc;
        link.formants = b->formants;
        link.params = b->params;
        link.warp_dst = ctx->warp_rows;
    }
    // The smoothing of the voicing mask answers flat windows from a word per tile that the kernel which writes the mask leaves
    // behind.  Only when the synthesis reads the very array the assembly writes, over the same concatenated sample axis.
    link.want_tile_flags = ctx->mask_flags && asmb->mask_out && asmb->mask_out == b->mask && asmb->total_samples == b->total_samples &&
                           asmb->n_notes == b->n_notes;
    // ... and where the route has no other reader of the mask than those of the flag bytes, the flat waves' values are not stored at all
    link.mask_sparse = link.want_tile_flags && synth_route_of(ctx, b, link).sparse_ok;
    rc = assemble_batch(ctx, asmb, link, st);
    if (!rc) rc = synth_batch(ctx, b, link, st);
    // the synthesis did not come to place the wait (it refused its batch, or was not reached): f0 / mask are in flight on the side
    // stream, and whatever the caller enqueues next may read them
    if (link.f0_side) (void)hipStreamWaitEvent(st, ctx->ev_f0, 0);
    return rc;
}

}  // extern "C"
