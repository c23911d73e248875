// Every kernel launcher (and geometry predicate) one translation unit of libgoofer_hip.so offers the others, by the file that
// defines it.  Included by the files that define them and by the files that call them (api.hip, synth.hip, post.hip).
#pragma once

#include <initializer_list>

#include "common.h"
#include "ragged.h"

struct onset_t;   // pulse.hip

// Frames per wave of the four kernels in which a wave walks a run of consecutive frames (k_noise_stems, k_harm_stem, k_irfft_ola3,
// k_irfft_ola1).  A run replays the `halo` frames in front of it without emitting them, so longer runs waste less; and every wave
// does the same work, so the grid should fill the device a whole number of times: with k rounds of `slots` waves,
// run = ceil(work / (k slots)), k the smallest that keeps a run at or below `cap` frames, and never below `floor_run`
// (0.92 -> 0.85 ms for k_irfft_ola3 on the 1024-note batch: 95 frames per wave in one round instead of 32 in three).
// `work`: the frames the waves share — k_irfft_ola1 gives a stem of a run to a wave: three times the batch's frames.
// Option "walk_run" N > 0 replaces the choice by N clamped to what the choice itself can return for this kernel,
// [floor_run, max(cap, floor_run)]: a test reaches long runs on a small batch and never a run no batch could get.
// `which`: 0 k_noise_stems, 1 k_harm_stem, 2 k_irfft_ola3, 3 k_irfft_ola1 — the run is kept for goofer_counter "walk_run_*".
enum { WALK_NOISE = 0, WALK_HARM = 1, WALK_OLA3 = 2, WALK_OLA1 = 3 };
static inline int walk_floor(int halo) { return halo <= 4 ? 32 : 8 * halo; }
static inline int walk_run_choice(goofer_ctx *ctx, int which, int64_t work, int64_t slots, int floor_run, int cap)
{
    int64_t run;
    if (ctx->walk_run > 0) {
        const int hi = cap > floor_run ? cap : floor_run;
        run = ctx->walk_run < floor_run ? floor_run : (ctx->walk_run > hi ? hi : ctx->walk_run);
    } else {
        const int64_t rounds = (work + slots * cap - 1) / (slots * cap);
        const int64_t fit = (work + rounds * slots - 1) / (rounds * slots);
        run = fit > floor_run ? fit : floor_run;
    }
    ctx->walk_run_used[which] = (int)run;
    return (int)run;
}

// ---- entry checks of the stages over a ragged batch of signals (limit.hip, loudness.hip, compress.hip, eq.hip) ----
// Host code.  A check fails in the name of the entry point `who` (goofer_fail) and returns its code, or GOOFER_OK.

static inline int check_counts(goofer_ctx *ctx, const char *who, int n, int64_t total, int64_t n_tiles)
{
    if (n >= 0 && total >= 0 && n_tiles >= 0) return GOOFER_OK;
    return goofer_fail(ctx, GOOFER_EINVAL, "%s: negative count (%d signals, %lld samples, %lld tiles)", who, n, (long long)total,
                       (long long)n_tiles);
}

// the tile table of a host planner: every signal with samples has ceil(len / tile) tiles, between ceil(total / tile) and that plus
// one per signal
static inline bool signal_tiles_ok(int64_t tile, int n, int64_t total, int64_t n_tiles)
{
    const int64_t least = (total + tile - 1) / tile;
    return n_tiles >= least && n_tiles <= least + n && n_tiles < ((int64_t)1 << 31);
}

// `p4` (null allowed) on 4 bytes, `p8` on 8; `names4` / `names8`: how the message lists them
static inline int check_aligned(goofer_ctx *ctx, const char *who, const char *names4, std::initializer_list<const void *> p4,
                                const char *names8, std::initializer_list<const void *> p8)
{
    uintptr_t a4 = 0, a8 = 0;
    for (const void *p : p4) a4 |= (uintptr_t)p;
    for (const void *p : p8) a8 |= (uintptr_t)p;
    if (!(a4 & 3) && !(a8 & 7)) return GOOFER_OK;
    return goofer_fail(ctx, GOOFER_EINVAL, "%s: %s must be 4-byte aligned, %s 8-byte aligned", who, names4, names8);
}

// `out` [total] may not overlap `x` [total]; with `in_place` it may be x itself
static inline int check_overlap(goofer_ctx *ctx, const char *who, const float *x, const float *out, int64_t total, bool in_place)
{
    if ((in_place && out == x) || total <= 0 || (uintptr_t)out >= (uintptr_t)(x + total) || (uintptr_t)x >= (uintptr_t)(out + total))
        return GOOFER_OK;
    return goofer_fail(ctx, GOOFER_EINVAL, in_place ? "%s: out overlaps x without being x" : "%s: out overlaps x (halos are read from x again: not in place)", who);
}

// analysis.hip
int launch_gauss_rows64(goofer_ctx *ctx, const float *in, int ld, double *out, int ld64, int64_t rows, int n_bins, const double *d_taps,
                        int radius, hipStream_t st);
int launch_knot_error(goofer_ctx *ctx, const double *env2, int ld64, const int64_t *probe, int n_probe, int n_bins, const int *knot_bin,
                      int K, const int *lerp_idx, const float *w0, const float *w1, unsigned long long *err_bits, hipStream_t st);
int launch_knot_gather(goofer_ctx *ctx, const double *env2, int ld64, int64_t rows, const int *knot_bin, int K, uint16_t *knots,
                       hipStream_t st);
int launch_env_rows_fused(goofer_ctx *ctx, const float2 *S, int ldc, int64_t rows, int n_bins, const double *taps_env, int r_env,
                          const double *taps_fit, int r_fit, double *env_rows, int ld64, double *env2, int ld2, hipStream_t st);
int launch_knot_search(goofer_ctx *ctx, const double *env2, int ld2, const int64_t *probe_row, const int *probe_sig, int n_probe,
                       int n_bins, const int *knot_bin, const int *lerp_idx, const float *w0, const float *w1, unsigned long long *err_bits,
                       hipStream_t st);
int launch_knot_pick(goofer_ctx *ctx, const double *env2, int ld2, int64_t rows, const int *frame_sig, const int64_t *frame_off,
                     const int *knot_bin, const unsigned long long *err_bits, uint16_t *knots, int32_t *K_out, hipStream_t st);

// assemble.hip
size_t env_row_rec_bytes();
// tile_notes: scratch for one int2 per SA_TILE samples (k_sample_tile_notes), or null: k_sample_assemble searches the plans
int launch_assemble(goofer_ctx *ctx, const goofer_assembly *a, int *row_note_edit, int *row_note_out, void *row_recs, int2 *tile_notes,
                    render_link &link, hipStream_t st);

// binops.hip
int launch_gauss_bins(goofer_ctx *ctx, const float *in, float *out, int64_t rows, int n_bins, int ld, const double *d_taps, int radius,
                      const int64_t *row_src, hipStream_t st);
int launch_warp_bins(goofer_ctx *ctx, const float *in, float *out, int64_t rows, int n_bins, int ld, const double *formants,
                     const double *d_f_shift, const goofer_note_params *params, const int *row_note, const int64_t *row_src, double ratio,
                     hipStream_t st);
int launch_warp_bins_ragged(goofer_ctx *ctx, const float *in, float *out, int64_t rows, int n_bins, int ld, const double *formants,
                            const int64_t *row_off, int n_notes, const double *note_args, hipStream_t st);
int launch_knot_decode(goofer_ctx *ctx, const uint16_t *knots, int K, int64_t rows, const int *idx, const float *w0, const float *w1,
                       float *env, int n_bins, int ld, hipStream_t st);
int launch_harm_shape(goofer_ctx *ctx, float2 *S, int ldc, int64_t total_frames, const int *frame_note, const int64_t *frame_off,
                      const int64_t *sample_off, const float *f0, const float *mask, const float *env, int ld,
                      const goofer_note_params *params, float *note_mag, const int64_t *row_src, const double *formants, bool no_warp,
                      const float2 *picks, hipStream_t st);
int launch_noise_spectra(goofer_ctx *ctx, float2 *S_uv, float2 *S_br, int ldc, int64_t total_frames, const int *frame_note,
                         const int64_t *frame_off, const int64_t *sample_off, const float *f0, const float *mask, const float *env_noise,
                         const float *phi, int ld, const goofer_note_params *params, uint64_t seed, const int64_t *row_src, bool preblurred,
                         const unsigned char *frame_skip, const float2 *picks, hipStream_t st);

// fft.hip
int launch_frame_note(goofer_ctx *ctx, const int64_t *frame_off, int n_notes, int64_t total_frames, int *frame_note, hipStream_t st);
int launch_rfft_frames_mapped(goofer_ctx *ctx, const float *x, const int64_t *sample_off, const int64_t *frame_off, const int *frame_note,
                              int64_t total_frames, float2 *S, int ldc, hipStream_t st);
int launch_irfft_frames(goofer_ctx *ctx, const float2 *S, int ldc, int64_t total_frames, float *frames, hipStream_t st);
int launch_ola_gather(goofer_ctx *ctx, const float *frames, const int64_t *sample_off, const int64_t *frame_off, int n_notes,
                      int64_t total_samples, float *y, const float *inv_scale, hipStream_t st);

// jitter.hip
template <typename Tin>
int launch_gauss_samples(goofer_ctx *ctx, const Tin *in, const int64_t *sample_off, int n_notes, int64_t total, const double *d_taps,
                         int radius, const unsigned char *note_on, double *out, hipStream_t st);
int launch_note_absmax(goofer_ctx *ctx, const double *x, const int64_t *sample_off, int n_notes, int64_t total,
                       const unsigned char *note_on, unsigned long long *max_bits, hipStream_t st);
int launch_f0_jitter(goofer_ctx *ctx, float *f0, double *f0_64, const float *mask, const double *noise_s,
                     const unsigned long long *max_bits, const int64_t *sample_off, int n_notes, int64_t total,
                     const goofer_note_params *params, int which, hipStream_t st);
int launch_volume_jitter(goofer_ctx *ctx, float *harm, float *bre, const double *nh, const double *nb, const double *vjm,
                         const unsigned long long *max_h, const unsigned long long *max_b, const int64_t *sample_off, int n_notes,
                         int64_t total, const goofer_note_params *params, int vibrato, double speed, hipStream_t st);

// limit.hip
int launch_limit(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int W, const float *taps, float c, const int32_t *tiles,
                 int64_t n_tiles, float *out, float *peak_in, float *min_gain, hipStream_t st, int R = 0, const float *tp_taps = nullptr,
                 int ch = 1);

// loudness.hip
int launch_loudness_measure(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int S, const double *coef, const double *mats,
                            const int64_t *seg_off, const int32_t *tiles, int64_t n_tiles, double target, double max_gain_db,
                            double *seg_energy, double *loud, float *gain, double *ends, double *starts, double *partial,
                            int32_t *first_tile, hipStream_t st);
int launch_loudness_apply(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, const float *gain, float *out,
                          hipStream_t st);

// compress.hip
int launch_compress(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, const double *coef, const double *pows,
                    const int32_t *tiles, int64_t n_tiles, float *out, double *max_reduction, double *curve, double *rsum,
                    double *rstart, double *asum, double *astart, int32_t *first_tile, double *xl, hipStream_t st);

// eq.hip
int launch_eq(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int K, const double *coef, const double *mats,
              const int32_t *tiles, int64_t n_tiles, float *out, double *ends, double *starts, int32_t *first_tile, hipStream_t st);

// reverb.hip
int launch_reverb(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, const void *ir, int L, int pre, float dry,
                  float wet, const int64_t *out_off, const int64_t *blk_off, int64_t total_blocks, const int32_t *runs, int64_t n_runs,
                  int64_t total_out, float *out, float2 *X, float2 *Y, hipStream_t st);

// noise.hip
int launch_normal_fill(goofer_ctx *ctx, uint64_t seed, const goofer_note_params *params, const int64_t *sample_off, int n_notes,
                       int64_t total, int tag, const unsigned char *note_on, const double *growl_scale, double *out, hipStream_t st);
int launch_phase_fill(goofer_ctx *ctx, const uint64_t *words, const int64_t *frame_off, int n_notes, int64_t total_frames, int n_bins,
                      float *out, int ld, hipStream_t st);
int launch_legacy_normal_fill(goofer_ctx *ctx, const uint32_t *seeds, const unsigned char *stream_on, const int64_t *sample_off, int n_notes,
                              double *out_f0, double *out_vol_h, double *out_vol_b, int64_t *attempts, hipStream_t st);
int launch_legacy_normal_jobs(goofer_ctx *ctx, const goofer_legacy_job *jobs, int n_jobs, int64_t *attempts, hipStream_t st);

// post.hip
int launch_onepole(goofer_ctx *ctx, const float *src, float *dst, const float *f0, const goofer_onepole_job *jobs, int n_jobs,
                   hipStream_t st);
int launch_post_layers(goofer_ctx *ctx, float *harm, const float *su, const float *sj, const goofer_post_note *notes,
                       const int64_t *sample_off, int n_notes, int64_t total, hipStream_t st);
int launch_post_fry(goofer_ctx *ctx, float *harm, float *bre, const float *harm_hp, const float *bre_hp, const goofer_post_note *notes,
                    const int64_t *sample_off, int n_notes, int64_t total, hipStream_t st);
int launch_post_sd(goofer_ctx *ctx, float *bre, const double *vmask_s, const goofer_post_note *notes, const int64_t *sample_off,
                   int n_notes, int64_t total, hipStream_t st);
int launch_note_sumsq(goofer_ctx *ctx, const float *harm, const float *bre, const goofer_post_note *notes, const int64_t *sample_off,
                      int n_notes, int64_t total, double *sums, hipStream_t st);
int launch_post_tension(goofer_ctx *ctx, float *harm, float *bre, const float *harm_hp, const goofer_post_note *notes,
                        const int64_t *sample_off, int n_notes, int64_t total, hipStream_t st);
int launch_post_scale(goofer_ctx *ctx, float *harm, float *bre, const double *before, const double *after, const goofer_post_note *notes,
                      const int64_t *sample_off, int n_notes, int64_t total, hipStream_t st);
int launch_post_mix(goofer_ctx *ctx, const float *harm, const float *uv, const float *bre, const float *sa_uv, const float *sa_bre,
                    const double *dyn, const goofer_post_note *notes, const unsigned char *note_on, const goofer_note_params *params,
                    const int64_t *sample_off, int n_notes, int64_t total, float *mix, hipStream_t st);
int launch_dyn_gain(goofer_ctx *ctx, const double *bend_s, const double *vmask_s, const unsigned char *note_on, double *ref,
                    const goofer_post_note *notes, const int64_t *sample_off, int n_notes, int64_t total, double *dyn, hipStream_t st);
int launch_vocal_roughness(goofer_ctx *ctx, const float *y, const float *f0, const float *mask, const double *nz, int n_k,
                           const double *k_list, const double *h_list, double noise_amp, double hp_fc, const float *aslew,
                           const int64_t *sample_off, int n_notes, int64_t total, float *out, hipStream_t st);

// pulse.hip
int launch_pulse_peak(goofer_ctx *ctx, float *peak, double sr, hipStream_t st);
size_t pulse_shape_table_floats();
int launch_pulse_shape_table(goofer_ctx *ctx, float *tab, const float *peak, double sr, hipStream_t st);
int launch_pulse_onsets(goofer_ctx *ctx, const float *f0, float f0_scale, const int64_t *sample_off, int n_notes, onset_t *onsets,
                        int32_t *onset_idx, int32_t *onset_cnt, int32_t *overflow, int64_t total_samples, int32_t *tiles, hipStream_t st);
int launch_pulse_place(goofer_ctx *ctx, const onset_t *onsets, const int32_t *onset_cnt, const int64_t *sample_off, int n_notes,
                       int64_t total_samples, float *pulse, const int32_t *tiles, hipStream_t st);
int launch_pulse_note(goofer_ctx *ctx, const float *f0, float f0_scale, const int64_t *sample_off, int n_notes, onset_t *onsets,
                      int32_t *onset_idx, int32_t *onset_cnt, int32_t *overflow, float *pulse, hipStream_t st);
int launch_pulse_train(goofer_ctx *ctx, const float *f0, float f0_scale, const int64_t *sample_off, int n_notes, int64_t total_samples,
                       float *pulse, double *inc, onset_t *onsets, int32_t *onset_idx, int32_t *onset_cnt, int32_t *overflow,
                       hipStream_t st);
int launch_subharm(goofer_ctx *ctx, const float *f0s, const double *f0_64, const float *mask, const int64_t *sample_off, int n_notes,
                   int64_t total, const goofer_note_params *params, const double *ratios, int n_ratios, int vib_on, double vib_rate,
                   double vib_depth, double vib_delay, double *fm, double *inc, onset_t *onsets, int32_t *onset_idx, int32_t *onset_cnt,
                   int32_t *overflow, const unsigned char *note_on, double *sub, unsigned long long *max_bits, float *pulse,
                   hipStream_t st);

// resample.hip
int launch_lerp_axis0(goofer_ctx *ctx, const float *in, int64_t ld_in, int64_t R_in, float *out, int64_t ld_out, int64_t R_out, int n_cols,
                      hipStream_t st);
int launch_lerp_1d(goofer_ctx *ctx, const float *in, int64_t R_in, float *out, int64_t R_out, hipStream_t st);
int launch_ingest_rows(goofer_ctx *ctx, const void *in, int in_f64, const int64_t *row_off, const int64_t *tile_off, int n_notes,
                       int64_t total_tiles, int n_cols, float *out, int ld, hipStream_t st);
int launch_stretch_ragged(goofer_ctx *ctx, const int64_t *row_off_in, const int64_t *row_off_out, const int64_t *row_cut,
                          const int64_t *sample_off_in, const int64_t *sample_off_out, const int64_t *sample_cut, int n_notes,
                          int64_t rows_out, int64_t samples_out, int n_cols, int ld, const float *env_h, const float *env_n,
                          float *env_h_out, float *env_n_out, const float *f0, const float *mask, float *f0_out, float *mask_out,
                          hipStream_t st);

// samples.hip
bool ola_split_supported(const goofer_plan_t &p);
int launch_irfft_ola1(goofer_ctx *ctx, const float2 *S_h, const float2 *S_u, const float2 *S_b, int ldc, int64_t total_frames,
                      const int *frame_note, const int64_t *frame_off, const int64_t *sample_off, int n_notes, const double *short_s,
                      double *steps, const goofer_note_params *params, float *harm, float *uv, float *bre, const unsigned char *frame_skip,
                      hipStream_t st);
int launch_frame_skip(goofer_ctx *ctx, const double *short_s, int64_t short_count, const int64_t *sample_off, const int64_t *frame_off,
                      const int *frame_note, int n_notes, int64_t total_frames, unsigned char *knot_eq, unsigned char *hop_flat,
                      unsigned char *frame_skip, hipStream_t st);
int launch_mask_upsample(goofer_ctx *ctx, const double *short_s, const int64_t *sample_off, int n_notes, int64_t total_samples,
                         double *steps, bool fast, float *out, hipStream_t st);
int launch_irfft_ola3(goofer_ctx *ctx, const float2 *S_h, const float2 *S_u, const float2 *S_b, int ldc, int64_t total_frames,
                      const int *frame_note, const int64_t *frame_off, const int64_t *sample_off, int n_notes, const float *note_mag,
                      const double *short_s, double *steps, const goofer_note_params *params, float *harm, float *uv, float *bre,
                      float *note_peak, hipStream_t st);
int launch_stem_peak(goofer_ctx *ctx, const float *harm, const float *uv, const float *bre, const int64_t *sample_off, int n_notes,
                     int64_t total, float *note_peak, hipStream_t st);
// tile_flags: render_link::tile_flags of this very mask, or null (sparse: render_link::mask_sparse — the mask is read through mask_value); counters: goofer_ctx::ovf_flag + MASK_COUNTERS (the slotted words of the two segment counters), or null
int launch_mask_short(goofer_ctx *ctx, const float *mask, const int64_t *sample_off, int n_notes, int64_t total_samples,
                      const double *d_taps, int radius, double tap_sum, double *short_s, const unsigned char *tile_flags,
                      int32_t *counters, bool sparse, hipStream_t st);
int launch_apply_gain(goofer_ctx *ctx, float *harm, float *uv, float *bre, float *rec, float *mix, const int64_t *sample_off, int n_notes,
                      int64_t total_samples, const goofer_note_params *params, const float *note_peak, bool write_stems, hipStream_t st);
int launch_ola3_gains(goofer_ctx *ctx, const float *fr_h, const float *fr_u, const float *fr_b, const float *note_mag,
                      const double *short_s, const int64_t *sample_off, const int64_t *frame_off, int n_notes, int64_t total_samples,
                      const goofer_note_params *params, double *steps, float *harm, float *uv, float *bre, float *note_peak,
                      hipStream_t st);

// stems.hip
bool stems_supported(const goofer_plan_t &p);
int launch_frame_picks(goofer_ctx *ctx, const int64_t *frame_off, const int *frame_note, int64_t F, const int64_t *sample_off,
                       const float *f0, const float *mask, const unsigned char *sparse_flags, float2 *picks, hipStream_t st);
int launch_noise_stems(goofer_ctx *ctx, const float *env, int ld, const int64_t *row_src, const float *phi, int64_t F,
                       const int *frame_note, const int64_t *frame_off, const int64_t *sample_off, const float2 *picks,
                       const goofer_note_params *params, uint64_t seed, bool preblurred, const double *short_s, const double *steps,
                       float *uv, float *bre, unsigned char *hopz, hipStream_t st);
int launch_harm_stem(goofer_ctx *ctx, const float *pulse, const float *env, const float *env_plain, bool have_formants, int ld,
                     const int64_t *row_src, int64_t F, const int *frame_note, const int64_t *frame_off, const int64_t *sample_off,
                     const float2 *picks, const goofer_note_params *params, float *harm, float *note_mag, hipStream_t st);
int launch_note_finish(goofer_ctx *ctx, float *harm, float *uv, float *bre, float *rec, float *mix, const int64_t *sample_off, int n_notes,
                       const goofer_note_params *params, const float *note_mag, float *note_peak, bool write_stems,
                       const unsigned char *hopz, const int64_t *frame_off, hipStream_t st);
