/*
 * goofer_hip.h — C ABI of libgoofer_hip.so, the MI355X (gfx950) backend for GOOFER's per-frame
 * source-filter resampler loop.
 *
 * The reference is pure Python: its "FFI" for this path is the set of numpy calls made by
 * GOOFER.py / SillySampler.py.  Each entry point below names the reference function it replaces
 * (file:line under the reference repo).  Conventions:
 *   - plain C, no torch types: device pointers are raw (e.g. torch.Tensor.data_ptr()), the stream is
 *     a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); NULL = default stream
 *   - every call is asynchronous on that stream; the caller owns all buffers; the library only
 *     allocates per-plan tables and scratch owned by the handle (goofer_reserve grows it, never
 *     inside a timed region if the caller reserved up front)
 *   - return 0 on success, negative GOOFER_E* on failure; goofer_last_error() gives the text
 *   - ragged batches are CSR: sample_off[n_notes+1], frame_off[n_notes+1] (int64, device memory)
 *   - device matrices are [frames x bins] row-major (the reference is [bins, frames]) with an
 *     explicit row stride `ld` in elements (ld >= n_bins; 516 keeps fp32 rows 16-byte aligned)
 *   - one handle per device per host thread; no global state
 */
#ifndef GOOFER_HIP_H
#define GOOFER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOOFER_OK 0
#define GOOFER_EINVAL (-1)   /* bad argument / unsupported geometry */
#define GOOFER_EHIP (-2)     /* a HIP runtime call failed */
#define GOOFER_ENOPLAN (-3)  /* goofer_plan() has not been called */
#define GOOFER_ENOMEM (-4)

typedef struct goofer_ctx goofer_ctx;

/* Per-note scalars of one synthesize() call — the keyword arguments of GOOFER.py:971-983 that the
 * sampler actually varies (SillySampler.py:1006-1035), plus the V/B/U mix of :1142-1151. */
typedef struct {
    float pitch_shift;          /* f0 *= pitch_shift (fp32)                       GOOFER.py:995  */
    float formant_shift;        /* 'g' flag: uniform warp ratio, 1 = off          GOOFER.py:1016 */
    double f_shift[4];          /* 'fa'..'fd': per-formant ratios, all 1 = off    GOOFER.py:1004 */
    float uv_strength;          /* default 0.75                                    GOOFER.py:1181 */
    float breath_strength;      /* default 0.1                                     GOOFER.py:1180 */
    float normalize;            /* 0..1 exponent of 1/peak                         GOOFER.py:1208 */
    int32_t apply_brightness;   /* default 1                                       GOOFER.py:1131 */
    int32_t cut_below_f0;       /* cut_subharm_below_f0, default 1                 GOOFER.py:1113 */
    float mix_harm, mix_breath, mix_unvoiced, volume;   /* V, (B+100)/100, (U+100)/100, volume */
    uint32_t seed[2];           /* per-note Philox key (lo, hi), XORed with the batch seed: a note's  */
                                /* noise never depends on where it sits in a batch                    */
    float vol_jitter_harm;      /* 'sr': volume_jitter_strength_harm, 0 = off     GOOFER.py:1185-1191 */
    float vol_jitter_breath;    /*       volume_jitter_strength_breath                                */
    float subharm_weight;       /* 'sg': +12 st pulse layer weight, 0 = off       GOOFER.py:1076-1097 */
    /* The two f0 jitter strengths are python floats in the reference and scale a factor that is rounded into the fp32 f0   */
    /* the pulse onsets are derived from: they stay fp64 (an fp32 strength moves a fifth of the f0 samples by an ulp).    */
    double f0_jitter;           /* 'sh': f0_jitter_strength, 0 = off              GOOFER.py:1069-1071 */
    double subharm_f0_jitter;   /* jitter of the f0 the sub-harmonic layer tracks; applied IN PLACE after the pulse   */
                                /* train, so the later per-frame f0 picks see it too (the reference's aliasing) :1078-1080 */
} goofer_note_params;

/* One ragged batch of notes for goofer_synth_batch.  All pointers are device memory. */
typedef struct {
    int32_t n_notes;
    int32_t n_bins;             /* n_fft/2 + 1 */
    int32_t ld;                 /* row stride of env / phi in floats */
    int32_t mix_only;           /* 1: only `mix` (and `rec`) are final; harm / uv / bre are scratch: the stems   */
                                /* before the peak gain, and (round 6) UNDEFINED wherever the noise walker found  */
                                /* a stem exactly zero over a whole hop and did not store it                      */
    int64_t total_frames;       /* frame_off[n_notes]: sum over notes of 1 + n_samples/hop */
    int64_t total_samples;      /* sample_off[n_notes] */
    int64_t total_env_rows;     /* env_off[n_notes] */
    const int64_t *sample_off;  /* [n_notes+1] */
    const int64_t *frame_off;   /* [n_notes+1] synthesis frames (pulse STFT frames)            */
    const int64_t *env_off;     /* [n_notes+1] envelope rows; a note's rows are truncated or   */
                                /*             edge-repeated to its frame count (GOOFER.py:1115-1119) */
    const float *env;           /* [total_env_rows x ld] spectral envelope                     */
    const double *formants;     /* [total_env_rows x 4] F1..F4 in Hz, or NULL when no f_shift  */
    const float *f0;            /* [total_samples] Hz, 0 where unvoiced                        */
    const float *mask;          /* [total_samples] voicing mask                                */
    const float *phi;           /* [total_frames x ld] random phases, or NULL: on-device Philox */
    const float *env_noise;     /* [total_env_rows x ld] noise envelope (sigma-1.75 blur of env along bins,    */
                                /* GOOFER.py:993) when the caller has it already — gf.synthesize's time stretch  */
                                /* resamples it separately from the warped env — else NULL: blurred in-kernel    */
    const goofer_note_params *params;  /* [n_notes] */
    uint64_t seed;              /* Philox key when phi == NULL */
    float transition_sigma;     /* noise_transition_smoothness of this call (default 100; the 'sa'  */
    float vol_jitter_speed;     /* layer uses 1) — one value per batch            GOOFER.py:1179 */
                                /* vol_jitter_speed: Hz of the volume_vibrato sinusoid (see volume_vibrato)       */
    /* jitter flags: standard-normal draws supplied by the caller (the reference takes them from the legacy  */
    /* global np.random stream), [total_samples] fp64 each, NULL when no note of the batch uses the flag      */
    const double *noise_f0;     /* for notes with f0_jitter > 0                   GOOFER.py:666        */
    const double *noise_vol_h;  /* harmonic volume jitter draw                    GOOFER.py:653        */
    const double *noise_vol_b;  /* breath volume jitter draw                                           */
    const double *noise_subharm;/* draw of subharm_f0_jitter (between the f0 and the volume draws), or NULL  :1079   */
    float f0_jitter_sigma;      /* sr / (6 * f0_jitter_speed)  samples            GOOFER.py:667        */
    float vol_jitter_sigma;     /* sr / (6 * volume_jitter_speed)                 GOOFER.py:654        */
    /* sub-harmonic pulse layer ('sg'): notes with params.subharm_weight > 0         GOOFER.py:1076-1097  */
    double subharm_ratio;       /* 2^(subharm_semitones / 12); 0 disables the layer for the batch         */
    double subharm_more[15];    /* further ratios when subharm_semitones is a list (0 = unused): one phase      */
                                /* tracker each, pulses summed before the joint max-normalisation  :672-736     */
    double subharm_vib_rate;    /* Hz                                              GOOFER.py:748-766       */
    double subharm_vib_depth;
    double subharm_vib_delay;   /* seconds of linear fade-in                                              */
    int32_t subharm_vibrato;    /* 0 / 1                                                                  */
    int32_t volume_vibrato;     /* 1: the volume jitter is a sinusoid, no noise draws needed  GOOFER.py:643-652  */
    int32_t unit_pitch_shift;   /* 1: the caller vouches params[i].pitch_shift == 1 for every note (the resampler  */
    int32_t no_warp;            /* path: pitch lives in the curve), so f0 needs no scaling pass          :995    */
                                /* no_warp = 1: the caller vouches that no note of the batch warps its envelope    */
                                /* (every f_shift == 1 and formant_shift == 1): kernels that could warp rows in    */
                                /* LDS need not reserve those rows (a note that warps anyway is rendered unwarped) */
    float *harm, *uv, *bre;     /* [total_samples] stems, gain-normalised like the reference   */
    float *rec;                 /* [total_samples] harm+uv+bre (reconstruct), may be NULL      */
    float *mix;                 /* [total_samples] (harm*V + bre*B + uv*U)*volume, may be NULL */
    const double *f0_64;        /* NULL, or [total_samples] the same f0 as a float64 array: what f0_interp IS in      */
                                /* gf.synthesize behind its time stretch (interp1d returns float64, GOOFER.py:1053).  */
                                /* The f0 jitters then multiply THIS array (`f0` becomes its float32 cast, which is   */
                                /* what the pulse train is handed, :1071-1074) and the sub-harmonic phase trackers    */
                                /* accumulate it (:1077-1097): on a float32 copy one event in ~10^5 lands a sample    */
                                /* off.  Final values (no pitch_shift is applied to it); read only with noise_f0 or   */
                                /* a sub-harmonic ratio set; not modified (the library works on a copy)                */
} goofer_batch;

/* One note's assembly plan (host-computed scalars, SillySampler.py:449-855).  "Logical" source rows /
 * samples are those of the feature arrays after the optional R1 reversal. */
typedef struct {
    int64_t knot_off;        /* first fp16 element of the note's source knot rows, [n_src_rows x K]      */
    int64_t edit_off;        /* first row of this note in the edited-row scratch                          */
    int64_t tap_off;         /* first row of this note in tap_idx / tap_w                                 */
    int64_t env_off;         /* first output envelope row (== fst_tracks row)                             */
    int64_t src_sample_off;  /* first element of the note's source voicing mask                           */
    int64_t out_sample_off;  /* first output sample                                                       */
    int64_t ylen;            /* source length in samples                                                  */
    int64_t bend_off;        /* first element of the note's pitch curve in goofer_assembly.bend           */
    double es_amount;        /* sharpen amount 5*|es|                                                     */
    double vel_factor;       /* 2^(1 - velocity/100)                                                      */
    double pitch_m;          /* MIDI note number                                                          */
    double pitch_t;          /* 't' flag / 100, added after bend/100 + pitch_m                            */
    double tick_dt;          /* 60 / (tempo * 96) seconds per pitch-bend tick                             */
    double fst[4];           /* formant-strength values (python floats in the reference)                  */
    int32_t K, lerp_plan, n_src_rows, reverse;
    int32_t row_lo, n_edit;  /* edited window: logical rows [row_lo, row_lo + n_edit)                     */
    int32_t tilt;            /* br tilt table index or -1                                                 */
    int32_t es_mode;         /* 0 off, 1 smooth, 2 sharpen                                                */
    int32_t es_taps_off, es_radius;
    int32_t fw_plan;         /* fw plan index or -1                                                       */
    int32_t n_out_rows, env_f64;
    int32_t n_out, n_pre, s_pre, s_tail, tail_len, want_samples, n_before_vel, pre_new;
    int32_t vel_active, force_voiced, n_bend, reserved;
    /* vocal fry ('vf' / 'vh' / 'vl', SillySampler.py:883-997); all ranges in output samples          */
    double fry_hz;           /* 'vh' base frequency (>= 1)                                                */
    int32_t fry_dir;         /* 0 off, +1 fry from the start, -1 fry towards the end                      */
    int32_t fry_const_lo, fry_const_hi;   /* f0 = fry_hz * (mask > 0)                                     */
    int32_t fry_glide_lo, fry_glide_hi;   /* f0 = (1 - w) * fry_hz * (mask > 0) + w * f0, w linspace      */
    int32_t fry_a, fry_b, fry_fade;       /* fry mask = 1 on [a, b) with linear fades of fry_fade samples */
    /* pitch dynamics ('pd', SillySampler.py:857-881)                                                     */
    int32_t pd_on;           /* write midi_curve - pd_base (fp32) to goofer_assembly.bend_out             */
    int32_t reserved4;
    double pd_base;          /* pitch_m + t/100                                                           */
} goofer_note_plan;

/* A batch of note assemblies.  All pointers are device memory. */
typedef struct {
    int32_t n_notes, n_bins, ld, sr, max_K, reserved;
    int64_t total_edit_rows, total_out_rows, total_samples;
    const goofer_note_plan *notes;   /* [n_notes] */
    const uint16_t *knots;           /* fp16 log-knot values, per note [n_src_rows x K]                   */
    const int32_t *lerp_idx;         /* [n_lerp_plans x n_bins] 2-tap lerp plans (GOOFER.py:84-90)        */
    const float *lerp_w0, *lerp_w1;
    const float *tilts;              /* [n_tilts x n_bins] br tilt curves (SillySampler.py:506-510)       */
    const double *es_taps;           /* concatenated Gaussian taps of the es flag                          */
    const int32_t *fw_lo, *fw_hi;    /* [n_fw x n_bins] fw plans (SillySampler.py:555-564)                */
    const double *fw_frac;
    const int32_t *tap_idx;          /* [total_out_rows x 4] logical source rows                           */
    const double *tap_w;             /* [total_out_rows x 4]                                               */
    const float *fst_tracks;         /* [total_out_rows x 4] sanitised + smoothed F1..F4 (Hz)              */
    const float *mask_src;           /* source voicing masks, concatenated                                 */
    const double *bend;              /* pitch curve per tick in MIDI semitones, concatenated: bend/100 + pitch_m */
                                     /* (+ t/100), fp64 like the reference builds it (SillySampler.py:838-846)    */
    float *edit_rows;                /* scratch [total_edit_rows x ld] (NULL: handle-owned)                */
    float *env_out;                  /* [total_out_rows x ld] assembled envelope                           */
    float *f0_out, *mask_out;        /* [total_samples]                                                    */
    float *bend_out;                 /* [total_samples] pitch-bend semitones of the 'pd' notes, or NULL    */
    int32_t any_fry, reserved5;      /* some note has fry_a < fry_b: run the envelope fry warp             */
    /* 'sj' growl layer (SillySampler.py:1061-1065): its f0 is f0_new * (0.5 * 2^noise) with f0_new still fp64, rounded */
    /* to fp32 ONCE inside synthesize.  f0_mul [total_samples] fp64 factors (anything on notes without the layer) and   */
    /* f0_mul_out [total_samples] = (float)(fp64 f0 * f0_mul), or both NULL.  Scaling the rounded f0_out instead moves    */
    /* two thirds of the layer's f0 samples by an ulp, enough to flip a pulse onset in ~3 % of such notes.              */
    const double *f0_mul;
    float *f0_mul_out;
} goofer_assembly;

/* One time-varying one-pole cascade (dynamic_butter_filter, SillySampler.py:95-174): `order` sections of
 * y = y' + a (x - y') (low-pass) or y = a (y' + x - x') (high-pass), each restarted from zero, the per-sample
 * coefficient following cutoff_factor * (5-tap box-smoothed f0 reference), clamped to [60|20 Hz, 0.45 sr]. */
typedef struct {
    int64_t src_off, dst_off;   /* element offsets into src / dst (equal offsets with src == dst: in place)  */
    int64_t f0_off;             /* element offset of the note's f0 reference                                 */
    int32_t n;                  /* samples                                                                   */
    int32_t order;              /* 1..12 (two chained order-6 calls are one order-12 cascade)                */
    int32_t highpass;           /* 0 low-pass, 1 high-pass                                                   */
    int32_t f0_mode;            /* 0: f0, 1: max(f0, 120), 2: ones (cutoff_factor is then the cutoff in Hz)  */
    float cutoff_factor;
    int32_t reserved;
} goofer_onepole_job;

/* Per-note settings of the sample-domain post chain (SillySampler.py:1037-1182). */
typedef struct {
    int64_t su_off, sj_off, sa_off;  /* first sample of the note in su_harm / sj_harm / sa_uv+sa_bre, -1: flag off */
    float su_gain;              /* 'su' / 100                                              :1037-1059        */
    float sj_mix;               /* 'sj' / 100                                              :1061-1081        */
    float sa_mix;               /* 'sa' / 100                                              :1153-1172        */
    float sd_strength;          /* 'sd' value                                              :1101-1112        */
    float tension;              /* 'st' / 100, in [-1, 1]                                  :1114-1140        */
    float pitch_dyn;            /* 'pd' / 100                                              :857-881, 1174-1182 */
    int32_t fry_a, fry_b, fry_fade;   /* fry mask range (see goofer_note_plan); a >= b: off :1083-1099       */
    int32_t reserved;
} goofer_post_note;

typedef struct {
    int32_t n_notes, reserved;
    int64_t total_samples;
    const int64_t *sample_off;          /* [n_notes+1] device                                                */
    const int64_t *sample_off_host;     /* [n_notes+1] the same offsets in HOST memory                       */
    const goofer_note_params *params;   /* [n_notes] device (mix_harm / mix_breath / mix_unvoiced / volume)  */
    const goofer_post_note *notes;      /* [n_notes] HOST memory: the library builds its job lists from it   */
    const float *f0, *mask;             /* [total_samples] assembled f0 / voicing mask                       */
    const float *bend;                  /* [total_samples] goofer_assembly.bend_out, NULL without 'pd'       */
    float *harm, *uv, *bre;             /* [total_samples] stems of the main synth call, edited in place     */
    float *su_harm, *sj_harm;           /* harmonic stems of the extra synth calls (compact, filtered in place) */
    const float *sa_uv, *sa_bre;        /* noise stems of the all-voiced 'sa' synth call (compact)           */
    float *mix;                         /* [total_samples] out; only notes with some post flag are rewritten */
} goofer_post;

/* ---- lifetime ------------------------------------------------------------------------------ */
int goofer_create(int device_id, goofer_ctx **out);
void goofer_destroy(goofer_ctx *ctx);
const char *goofer_last_error(const goofer_ctx *ctx);
const char *goofer_version(void);

/* Tables per (sr, n_fft, hop): sqrt-Hann window, bin freqs, boost, brightness curves, FFT twiddles
 * (GOOFER.py:12-46, 585-595).  n_fft: 512, 768, 1024, 1536, 2048, 4096 (radix plans; the stem walkers run at 1024 with hop 256,
 * the fused overlap-add at 512 / 1024 / 2048; at 4096 one workgroup shares a frame) or any other even size in [64, 4096] but 2050
 * (Bluestein's chirp-z transform through power-of-two transforms, one kernel per reference step; above 2048 at length 4096 on
 * the workgroup transform); re-planning replaces the tables.  The resampler's assembly and render calls take n_fft <= 2048. */
int goofer_plan(goofer_ctx *ctx, int sr, int n_fft, int hop);

/* Pre-size handle-owned scratch for batches up to these totals (else grown on demand). */
int goofer_reserve(goofer_ctx *ctx, int64_t max_frames, int64_t max_samples, int64_t max_notes);

/* ---- single-kernel entry points (unit parity + roofline runs) ------------------------------ */

/* gf.stft (GOOFER.py:355-370): per note reflect-pad n_fft/2, frame, sqrt-Hann, rFFT.
 * x [total_samples] -> S [total_frames x ldc] complex64 (interleaved re,im; ldc in complex elements). */
int goofer_rfft_frames(goofer_ctx *ctx, const float *x, const int64_t *sample_off, const int64_t *frame_off,
                       int n_notes, int64_t total_frames, float *S, int ldc, void *stream);

/* gf.istft + _overlap_add (GOOFER.py:372-413): irFFT, windowed OLA normalised by the summed squared
 * window, trim n_fft/2, zero-pad to the note length.  S [total_frames x ldc] -> y [total_samples]. */
int goofer_irfft_ola(goofer_ctx *ctx, const float *S, int ldc, const int64_t *sample_off, const int64_t *frame_off,
                     int n_notes, int64_t total_frames, int64_t total_samples, float *y, void *stream);

/* The LF glottal-pulse model of gf.pulse_train_numba — its keyword arguments Ra, Rg, Rk (GOOFER.py:474, 508-519: opening
 * phase sin^2 up to Tp = Ra T, return phase exp(-Rg tau) cos(pi tau / 2) up to Tc = Tp + Rk (T - Tp)).  A plan starts with
 * 0.02 / 1.7 / 0.8, the values gf.synthesize passes (GOOFER.py:1074); this call rebuilds the plan's pulse tables for other
 * values (it synchronises the device) and they hold until the next goofer_plan.  Every pulse the handle makes afterwards —
 * goofer_pulse_train and the synthesis — uses them. */
int goofer_pulse_model(goofer_ctx *ctx, double Ra, double Rg, double Rk);

/* gf.pulse_train_numba (GOOFER.py:473-554) with the plan's pulse model (goofer_pulse_model): f0 [total_samples] -> pulse. */
int goofer_pulse_train(goofer_ctx *ctx, const float *f0, const int64_t *sample_off, int n_notes,
                       int64_t total_samples, float *pulse, void *stream);

/* gf.gaussian_filter1d(axis=bins) (GOOFER.py:241-261): fp64 taps [2*radius+1] (host memory, the
 * caller normalises them exactly as the reference does), numpy-'reflect' padding, fp64 accumulate.
 * in/out [rows x ld] fp32. */
int goofer_gauss_bins(goofer_ctx *ctx, const float *in, float *out, int64_t rows, int n_bins, int ld,
                      const double *taps, int radius, void *stream);

/* gf.warp_env_by_formants then gf.shift_formants (GOOFER.py:840-875, 618-627) on rows of env.
 * formants [rows x 4] fp64 (may be NULL when all f_shift == 1); f_shift NULL = no anchor warp;
 * ratio 1 = no uniform warp.  Each stage rounds to fp32 like the reference. */
int goofer_warp_bins(goofer_ctx *ctx, const float *in, float *out, int64_t rows, int n_bins, int ld,
                     const double *formants, const double *f_shift, double ratio, void *stream);

/* gf.decode_env_from_knots (GOOFER.py:149-168): knots fp16 [rows x K] (frames-major) -> env fp32
 * [rows x ld]; hz_knots fp32 [K] in host memory. */
int goofer_knot_decode(goofer_ctx *ctx, const uint16_t *knots_f16, int K, const float *hz_knots,
                       int64_t rows, float *env, int n_bins, int ld, void *stream);

/* ---- analysis half that does not need Praat (GOOFER.py:942-946, 97-147) -------------------------------- */

/* Caller scratch: goofer_envelope_knots_batch, the goofer_track_* calls and goofer_per_sample_f0 take device scratch from the
 * caller.  Call once with scratch = NULL, the query form: the batch is checked as the call checks it, the HOST offset arrays
 * the call writes and *scratch_bytes are filled in, and no device code runs (ctx may be NULL, but for
 * goofer_envelope_knots_batch, which needs the plan).  Then call with device scratch of at least *scratch_bytes bytes (a
 * shorter block: GOOFER_EINVAL, before anything is launched); it is in use until the stream reaches the end of the call. */

/* The pieces of compress_env_to_knots for a caller's envelope (core.compress_env_to_knots runs the K search on the host). */

/* gaussian_filter1d(axis=bins) with the reference's fp64 result kept: in fp32 [rows x ld] -> out fp64 [rows x ld64];
 * taps fp64 [2*radius+1] in HOST memory. */
int goofer_gauss_bins_f64(goofer_ctx *ctx, const float *in, int ld, double *out, int ld64, int64_t rows, int n_bins,
                          const double *taps, int radius, void *stream);

/* One candidate of compress_env_to_knots' search: max over the probe rows and all bins of
 * abs(exp(lerp(log knots)) - env) / (env + 1e-8), with knots = log(max(env, 1e-8)) sampled at knot_bin (all device
 * arrays; hz_knots fp32 [K] in HOST memory defines the lerp).  *max_rel_err is written on the host (synchronises). */
int goofer_knot_fit_error(goofer_ctx *ctx, const double *env, int ld64, const int64_t *probe_rows, int n_probe, int n_bins,
                          const int32_t *knot_bin, int K, const float *hz_knots, double *max_rel_err, void *stream);

/* knot_vals_log = log(max(env, 1e-8))[knot_bin] as fp16, [rows x K] (frames-major). */
int goofer_knot_gather(goofer_ctx *ctx, const double *env, int ld64, int64_t rows, const int32_t *knot_bin, int K,
                       uint16_t *knots_f16, void *stream);

/* The envelope half of gf.extract_features (GOOFER.py:942-946) with compress_env_to_knots (GOOFER.py:97-147) for a ragged
 * batch of fp32 signals y (device) at the plan's (sr, n_fft, hop): per signal gf.stft's T = 1 + n / hop frames (reflect-padded
 * at its own ends), |S| + 1e-8, the sigma-2 bin blur in fp64, rounded to fp32, the sigma-0.5 blur in fp64, then the smallest
 * knot count K of 32, 48, ..., 192 whose 2-tap lerp reproduces that envelope to < 1e-2 max relative error on the probe rows
 * linspace(0, T - 1, min(256, T)) (else 192), and log(max(env, 1e-8)) at its knots' bins as fp16.  Each signal's K and knots
 * are what compress_env_to_knots' defaults (goofer_gauss_bins_f64, goofer_knot_fit_error, goofer_knot_gather) give for its
 * env_rows rounded to fp32, bit for bit, and do not depend on the other signals of the batch.
 *   sample_off [n_signals+1], frame_off [n_signals+1]: HOST arrays; frame_off is written.  Every signal has >= 1 sample.
 *   taps_env [2*radius_env+1], taps_fit [2*radius_fit+1]: fp64 taps of the two blurs in HOST memory (core.gaussian_taps).
 *   hz_knots, knot_bin: fp32 knot frequencies and int32 nearest bins of the eleven candidates back to back (32 + 48 + ... + 192
 *   = 1232 entries each) in HOST memory.
 *   knots_f16 [frame_off[n] x 192] (device): signal s writes its [T_s x K_s] knots frames-major at frame_off[s] * 192.
 *   K_out [n_signals] int32 (device).  env_rows (device, or NULL): the sigma-2 envelope in fp64, [frame_off[n] x ld64].
 * Caller scratch as above.  The call synchronises the stream once, after uploading its tables and before its kernels. */
int goofer_envelope_knots_batch(goofer_ctx *ctx, const float *y, const int64_t *sample_off, int n_signals, const double *taps_env,
                                int radius_env, const double *taps_fit, int radius_fit, const float *hz_knots, const int32_t *knot_bin,
                                int64_t *frame_off, uint16_t *knots_f16, int32_t *K_out, double *env_rows, int ld64, void *scratch,
                                int64_t *scratch_bytes, void *stream);

/* ---- f0 and formant tracks of the cold-cache analysis (goofer_amd/csrc/tracker.hip) -------------------------------
 * The tracker's settings belong to the handle, as goofer_pulse_model's do: goofer_create starts at the defaults, and
 * goofer_track_configure replaces them for every goofer_track_* call that follows on the handle, their query forms
 * included (a query form with ctx NULL reads the defaults). */
typedef struct goofer_track_settings {
    int pitch_floor;             /* Hz, integer in [20, 600]; the pitch window is 3 / pitch_floor seconds             75   */
    double pitch_ceiling;        /* Hz, above the floor and at most 20000; a call uses min(pitch_ceiling, sr / 2)     950  */
    double silence_threshold;    /* finite, >= 0                                                                      0.03 */
    double voicing_threshold;    /* in (0, 1)                                                                         0.45 */
    double octave_cost;          /* finite, >= 0                                                                      0.01 */
    double octave_jump_cost;     /* finite, >= 0                                                                      0.35 */
    double voiced_unvoiced_cost; /* finite, >= 0                                                                      0.14 */
    int max_formant;             /* Hz, integer in [2500, 8000]; the formant stage resamples to 2 max_formant         5500 */
    int n_formants;              /* 3, 4 or 5; Burg order 2 n_formants                                                5    */
} goofer_track_settings;
#define GOOFER_TRACK_SETTINGS_DEFAULT {75, 950.0, 0.03, 0.45, 0.01, 0.35, 0.14, 5500, 5}

/* The default settings (the values above). */
void goofer_track_settings_default(goofer_track_settings *settings);
/* The handle's tracker settings from now on; NULL: the defaults.  A value outside its range above: GOOFER_EINVAL, a message
 * that names the field, and the handle keeps the settings it had. */
int goofer_track_configure(goofer_ctx *ctx, const goofer_track_settings *settings);
/* The frame layout the tracker gives a batch under `settings` (NULL: the defaults), without a handle or a device:
 * pitch_off, x_off and formant_off [n_signals+1] (HOST, any may be NULL) as goofer_track_pitch, goofer_track_resample and
 * goofer_track_formants write them, and their refusals (GOOFER_EINVAL). */
int goofer_track_layout(const goofer_track_settings *settings, const int64_t *sample_off, int n_signals, int sr, int hop,
                        int64_t *pitch_off, int64_t *x_off, int64_t *formant_off);

/* A ragged batch of fp64 signals y (device) at one sample rate sr in [8000, 96000]; sample_off[n_signals+1] and
 * frame_off[n_signals+1] are HOST arrays, frame_off is written by the call; caller scratch as above.  With the handle's
 * settings (defaults in brackets), all in the integer arithmetic written here:
 *
 * goofer_track_pitch: Boersma's autocorrelation method with a Viterbi path, floor pitch_floor (75) Hz, ceiling
 * min(pitch_ceiling (950), sr/2) Hz, time step hop / sr, Hann window of W = 3 sr / floor samples, lags floor(sr / ceiling) ..
 * ceil(sr / floor), up to 15 candidates per frame.  Frames: (floor n - 3 sr) / (floor hop) + 1 per signal, centred in it.
 * f0 [frame_off[n]] in Hz, 0 where unvoiced.  Every signal needs ceil(3 sr / floor) samples at least (GOOFER_EINVAL).  A frame
 * and its lags live in LDS: a floor and rate that need more than 160 KiB are refused (GOOFER_EINVAL; none of the admitted
 * floors does at an admitted rate).
 * goofer_track_formants: Burg LPC of order 2 n_formants (10) on the signal resampled to R = 2 max_formant (11000) Hz (up as
 * well as down) and pre-emphasised from 50 Hz (factor exp(-2 pi 50 / R)), Gaussian window of R / 20 samples (50 ms; 550),
 * same time step; frames: floor((m - R / 20) sr / (R hop)) + 1 for m = n * R / sr resampled samples (0 when m < R / 20).
 * formants [frame_off[n] x 5] in Hz, ascending, 0 where fewer than five roots lie in (50, R / 2 - 50) Hz; the columns from
 * n_formants on are 0.
 * Non-finite samples: a NaN or infinite sample makes its signal's peak deviation NaN, as numpy's max does.  Every pitch frame
 * of that signal then has the unvoiced strength voicing_threshold (the silence term max(0, 2 - NaN) is 0), a frame whose
 * window holds such a sample has no voiced candidate, and a formant frame whose resampled samples are not finite has no
 * formants (0).  The other signals of the batch are not affected.
 * Each call is a composition of the single-stage calls below, and gives their bits. */
int goofer_track_pitch(goofer_ctx *ctx, const double *y, const int64_t *sample_off, int n_signals, int sr, int hop,
                       int64_t *frame_off, double *f0, void *scratch, int64_t *scratch_bytes, void *stream);
int goofer_track_formants(goofer_ctx *ctx, const double *y, const int64_t *sample_off, int n_signals, int sr, int hop,
                          int64_t *frame_off, double *formants, void *scratch, int64_t *scratch_bytes, void *stream);

/* Single-stage entry points of the tracker (unit parity), with the conventions above: HOST offset arrays, caller scratch,
 * device arrays otherwise.
 * goofer_track_candidates: goofer_track_pitch's per-frame stage.  cand_f, cand_s [frame_off[n] x 15] fp64 and cand_n
 * [frame_off[n]] int32 (device): frame f has cand_n[f] candidates; slot 0 is the unvoiced one (frequency 0, the unvoiced
 * strength), slots 1.. the voiced ones in lag order (frequency in Hz, strength); the slots from cand_n[f] on are not written.
 * goofer_track_path: goofer_track_pitch's Viterbi stage on candidates in that layout, for time step hop / sr.  frame_off
 * [n_signals+1] is read (0 first, never decreasing); a cand_n outside [1, 15] is taken as the nearest of 1 and 15.  f0
 * [frame_off[n]]: the chosen candidate's frequency; the first best predecessor, and the first best last candidate, win ties.
 * goofer_track_resample: goofer_track_formants' resampled signal (11 kHz by default).  x_off [n_signals+1] is written
 * (n * R / sr samples per signal), x11 [x_off[n]] fp64 (device).  Every signal needs one sample at least.
 * goofer_track_formant_frames: goofer_track_formants' per-frame stage on a caller's signals at R Hz, x11 [x_off[n]] (device),
 * x_off read (0 first, never decreasing); sr and hop are the original rate and hop, which place the frames; frame_off is
 * written; formants as goofer_track_formants. */
int goofer_track_candidates(goofer_ctx *ctx, const double *y, const int64_t *sample_off, int n_signals, int sr, int hop,
                            int64_t *frame_off, double *cand_f, double *cand_s, int32_t *cand_n, void *scratch,
                            int64_t *scratch_bytes, void *stream);
int goofer_track_path(goofer_ctx *ctx, const double *cand_f, const double *cand_s, const int32_t *cand_n, const int64_t *frame_off,
                      int n_signals, int sr, int hop, double *f0, void *scratch, int64_t *scratch_bytes, void *stream);
int goofer_track_resample(goofer_ctx *ctx, const double *y, const int64_t *sample_off, int n_signals, int sr, int64_t *x_off,
                          double *x11, void *scratch, int64_t *scratch_bytes, void *stream);
int goofer_track_formant_frames(goofer_ctx *ctx, const double *x11, const int64_t *x_off, int n_signals, int sr, int hop,
                                int64_t *frame_off, double *formants, void *scratch, int64_t *scratch_bytes, void *stream);

/* gf.extract_features' f0 post-processing (GOOFER.py:957-966) for a ragged batch of frame-rate f0 tracks (goofer_amd/csrc/f0.hip):
 * NaN -> 0, zero runs of at most max_gap frames with a neighbour on both sides bridged linearly (GOOFER.py:415-435), np.interp
 * over np.linspace(0, n / sr) grids of the track and of the n samples (0 outside the track), clip to [1e-5, 2000].
 * tracks [track_off[n_signals]] fp64 (device); track_off and sample_off [n_signals + 1] are HOST arrays starting at 0, every track
 * with two frames at least (one frame or none: GOOFER_EINVAL; the host handles them).  Writes f0 and mask (f0 > f0_min as 0 / 1)
 * [sample_off[n_signals]] fp64, bit for bit numpy's.  Caller scratch as above. */
int goofer_per_sample_f0(goofer_ctx *ctx, const double *tracks, const int64_t *track_off, const int64_t *sample_off, int n_signals,
                         double sr, double f0_min, int max_gap, double *f0, double *mask, void *scratch, int64_t *scratch_bytes,
                         void *stream);

/* ---- the hot path --------------------------------------------------------------------------- */

/* gf.synthesize for a ragged batch (GOOFER.py:971-1220) + the V/B/U mix (SillySampler.py:1142-1151). */
int goofer_synth_batch(goofer_ctx *ctx, const goofer_batch *batch, void *stream);

/* SillySampler.resample up to (not including) the synthesize call: knot decode, br / es / fw on the source
 * rows, slicing + loop modes + velocity stretch as a 4-tap frame gather, formant-strength gain, per-sample
 * voicing mask and pitch curve (SillySampler.py:449-855).  Outputs feed goofer_synth_batch directly. */
int goofer_assemble_batch(goofer_ctx *ctx, const goofer_assembly *assembly, void *stream);

/* SillySampler.resample for one batch as ONE call (SillySampler.py:449-1151 without the post chain): exactly
 * goofer_assemble_batch followed by goofer_synth_batch — same kernels, same results — for a batch whose
 * assembly->f0_out is batch->f0.  With both descriptors in hand everything they point to must already be enqueued on
 * `stream` (or complete) when the call is made; that lets the synthesis' pulse chain (f0 scaling, the sequential
 * phase walk, pulse placement) start on the handle's side stream as soon as the assembled f0 exists, beside the
 * envelope assembly, instead of when the synthesis' first kernel is reached in stream order. */
int goofer_render_batch(goofer_ctx *ctx, const goofer_assembly *assembly, const goofer_batch *batch, void *stream);

/* gf.stretch_feature (GOOFER.py:597-616): np.interp(linspace(0,1,rows_out), linspace(0,1,rows_in), column) along
 * axis 0 of a [rows x n_cols] fp32 matrix with row strides ld_in / ld_out (n_cols = 1, ld = 1: a 1-D array). */
/* Host-side helper of the note planner (no device involved): Gaussian FIR along the rows of an fp64 [rows x T] matrix, numpy
 * 'reflect' padding, taps applied in ascending order — the sigma-4 smoothing of the formant tracks, SillySampler.py:264-283. */
int goofer_host_gauss_rows(const double *x, int64_t rows, int T, const double *taps, int radius, double *out);

/* ---- host-side note planner (pure CPU code: no device, no handle) ----------------------------------------------------
 * What SillySampler.resample decides about a note before it touches an array (SillySampler.py:449-500 cut points, :625-696
 * loop modes, :698-788 sample counts + velocity stretch, :714-763 / 264-283 / 791-806 formant tracks, :883-955 fry ranges),
 * for a whole batch in one call; the arithmetic of goofer_amd/sampler.py's numpy planner, bit for bit. */
typedef struct {
    double offset, length, consonant, cutoff;   /* seconds: the request's offset / length / consonant / cutoff / 1000     */
    double vel_factor;                          /* 2 ** (1 - velocity / 100)                                :765           */
    double fry, fry_glide;                      /* 'vf' (clipped to +-100), 'vl'                            :883-888       */
    int64_t ylen;                               /* samples of the source                                                   */
    int32_t sr, n_src_frames;                   /* n_src_frames = rows of the source envelope = 1 + ylen / hop             */
    int32_t loop_mode, reverse;                 /* 0 concat (L0), 1 mirror mean (L1), 2 stretch (L2); 'R1'                 */
    const double *tracks[4];                    /* the source's F1..F4 tracks (Hz, fp64, HOST memory)                      */
    int32_t track_len[4];                       /* their lengths; -1: the source has no such track                         */
    int32_t fst_skip[4];                        /* != 0: this formant's 'fst' strength is off for the note (|s| < 1e-6), so */
                                                /* its fst_tracks column is never read: left 0, the sigma-4 blur not run    */
} goofer_plan_request;

typedef struct {
    int64_t start_sample, consonant_sample, end_sample;     /* cut points                                   :453-487       */
    int64_t tap_off;                            /* first row of the note in the arrays of goofer_host_plans_view           */
    double vel_factor;                          /* the stretch factor when vel_active, else 1                              */
    int32_t status;                             /* 0 planned; 1: a case the reference answers with an exception (empty     */
                                                /* tail to loop, negative length): nothing else of the record is valid     */
    int32_t start_frame, consonant_frame, end_frame;
    int32_t n_rows;                             /* envelope frames the reference would assemble                            */
    int32_t n_out_rows;                         /* rows planned: n_rows, or 1 + n_out / hop when trim_rows cut the rest     */
    int32_t row_lo, row_hi;                     /* source rows [row_lo, row_hi) the planned rows read                      */
    int32_t env_f64;                            /* the reference holds this note's envelope in float64 (lerps / fades)     */
    int32_t n_out, n_pre, s_pre, s_tail, tail_len, want_samples, n_before_vel, pre_new, vel_active;   /* goofer_note_plan */
    int32_t fry_dir, fry_const_lo, fry_const_hi, fry_glide_lo, fry_glide_hi, fry_a, fry_b, fry_fade;  /* goofer_note_plan */
    int32_t reserved;
} goofer_plan_geometry;

typedef struct goofer_host_plans goofer_host_plans;

/* Plan n_notes notes.  gauss_taps[2 * gauss_radius + 1]: the sigma-4 taps of sanitize_smooth_formant (:281), made by the
 * caller the way numpy makes them.  trim_rows != 0: plan only the envelope rows gf.synthesize can reach (GOOFER.py:1115-1119).
 * n_threads <= 0: up to eight host threads.  The result is freed with goofer_host_plans_free. */
int goofer_host_plan_notes(const goofer_plan_request *req, int n_notes, int hop, int trim_rows, const double *gauss_taps,
                           int gauss_radius, int n_threads, goofer_host_plans **out);
/* The same plans written into memory of the caller — pinned staging buffers one H2D copy ships, re-used from batch to batch.
 * geometry[n_notes]; the four row arrays hold row_capacity rows x 4 (layout as goofer_host_plans_view); *rows_out = rows of the
 * batch.  Returns 0 with the arrays filled, 1 when row_capacity is too small (*rows_out and the geometry's status / n_out_rows /
 * tap_off are written: grow, call again), or a negative error code as goofer_host_plan_notes. */
int goofer_host_plan_into(const goofer_plan_request *req, int n_notes, int hop, int trim_rows, const double *gauss_taps,
                          int gauss_radius, int n_threads, goofer_plan_geometry *geometry, int64_t row_capacity, int32_t *tap_idx,
                          double *tap_w, double *formants, float *fst_tracks, int64_t *rows_out);
/* The planned batch: geometry[n_notes]; rows = sum of n_out_rows over the notes with status 0; tap_idx / tap_w [rows x 4]
 * (goofer_assembly.tap_idx / tap_w), formants [rows x 4] fp64 (goofer_batch.formants), fst_tracks [rows x 4] fp32
 * (goofer_assembly.fst_tracks).  HOST memory owned by the handle.  Any out pointer may be NULL. */
int goofer_host_plans_view(const goofer_host_plans *plans, const goofer_plan_geometry **geometry, int64_t *rows,
                           const int32_t **tap_idx, const double **tap_w, const double **formants, const float **fst_tracks);
void goofer_host_plans_free(goofer_host_plans *plans);

/* UTAU pitch-bend strings of a batch (SillySampler.py:56-84): text = the strings back to back, text_off[n + 1] their bounds.
 * Writes out_off[n + 1] and, when out != NULL, the decoded cents (at most `capacity` values); returns the number of values,
 * or -(i + 1) when string i is not well formed (the caller's character loop then raises what the reference raises). */
int64_t goofer_host_decode_bends(const char *text, const int64_t *text_off, int n, float *out, int64_t capacity, int64_t *out_off);

/* float() of n plain decimal strings back to back (the numeric resampler arguments of a batch, SillySampler.py:289-298):
 * out[i] / ok[i] = 1 for [+-]digits[.digits][e[+-]digits]; ok[i] = 0 for anything else (the caller asks Python's float()).
 * strip_bang: skip leading '!' (the tempo argument).  Returns how many strings were not taken, or -1 on a null argument. */
int goofer_host_parse_floats(const char *text, const int64_t *text_off, int n, int strip_bang, double *out, unsigned char *ok);

/* Host arrays back to back into one block (pinned staging memory) on `threads` threads: piece i, nbytes[i] bytes at src[i], lands
 * behind the pieces in front of it.  The upload path of fresh voicebank samples (goofer_amd/render.py SourceArena: the reference
 * re-reads a sample's features from disk per note, GOOFER.py:1227-1262; here they go to HBM once).  Pure CPU code.  Returns the
 * bytes written, or a negative error (GOOFER_EINVAL: more than `capacity` bytes, null pieces). */
int64_t goofer_host_pack(const void *const *src, const int64_t *nbytes, int64_t count, void *dst, int64_t capacity, int threads);

/* Synchronise the device and report errors the asynchronous batch calls detect on the device (today: a note with more
 * pulse onsets than its n / 2 + 16 onset slots, GOOFER.py:493 with f0 above sr / 2; a batch with the 'sg' layer leaves its
 * sub-harmonic onsets in n + 16 slots per note, one per sample at most).  0, or GOOFER_EINVAL + goofer_last_error. */
int goofer_check(goofer_ctx *ctx);

/* Cumulative per-handle counters kept on the device (the call synchronises): "pulse_scanned_notes" = notes whose pulse onsets
 * (GOOFER.py:487-493) were taken from the parallel phase scan, "pulse_fallback_notes" = those of them that had to be walked
 * sequentially afterwards because a sample's phase lay within the scan's rounding band of an integer, "pulse_list_notes" =
 * notes the fused pulse kernel (option "pulse_fused") placed from the onset list in global memory and not from its LDS ring: the
 * walked ones, and those with more than 2048 onsets alive at once.
 * "mask_flag_segments" / "mask_staged_segments": note segments of the mask smoother's 1024-knot tiles (goofer_synth_batch /
 * goofer_render_batch) that were answered from the f0 kernel's tile flags alone / that staged their window of the mask (option
 * "mask_flags"; without flags every segment stages; the per-sample loop of a radius above 1792 knots counts nothing).
 * "walk_run_noise" / "walk_run_harm" / "walk_run_ola3" / "walk_run_ola1": not cumulative and not on the device — the frames per
 * wave that the last launch of k_noise_stems / k_harm_stem / k_irfft_ola3 / k_irfft_ola1 on this handle was given (0: none
 * yet; option "walk_run"). */
int goofer_counter(goofer_ctx *ctx, const char *name, int64_t *value);

/* gf.smooth_mask_ds (GOOFER.py:556-569) on its own, for a ragged batch of voicing masks (sample_off[n_notes + 1]): decimate by
 * 4, Gaussian max(1, sigma / 4) in fp64, np.interp back on float32 linspace grids -> out[total_samples] fp32.
 * fast_interp != 0 selects the interpolant form the stem walkers use (must give the same bits). */
int goofer_smooth_mask_ds(goofer_ctx *ctx, const float *mask, const int64_t *sample_off, int n_notes, int64_t total_samples,
                          float sigma, int fast_interp, float *out, void *stream);

int goofer_stretch_rows(goofer_ctx *ctx, const float *in, int64_t ld_in, int64_t rows_in, float *out, int64_t ld_out,
                        int64_t rows_out, int n_cols, void *stream);

/* ---- ragged feature preparation for core.synthesize_batch (many gf.synthesize calls per device pass) ------------------------
 * All CSR arrays are device memory; every launch covers the whole batch. */

/* to_compute(env_spec).T per note (GOOFER.py:72, 984) in one launch: note i's [n_cols x T_i] array (row-major, the reference's
 * [bins, frames] layout) starts at element row_off[i] * n_cols of `in` (fp64 when in_f64, else fp32), T_i = row_off[i+1] -
 * row_off[i]; it becomes rows row_off[i] .. row_off[i+1] of out [row_off[n] x ld] fp32.  fp64 is rounded to nearest even, as
 * numpy's astype(np.float32).  tile_off [n_notes+1]: prefix sums of ceil(T_i / 64), total_tiles = tile_off[n_notes].  Also
 * lays out injected phases (gf.synthesize's phi). */
int goofer_ingest_rows(goofer_ctx *ctx, const void *in, int in_f64, const int64_t *row_off, const int64_t *tile_off, int n_notes,
                       int64_t total_tiles, int n_cols, float *out, int ld, void *stream);

/* goofer_warp_bins with settings per note: row r of in / out [rows x ld] belongs to the note i with row_off[i] <= r <
 * row_off[i+1]; formants [rows x 4] fp64 or NULL; note_args [n_notes x 6] fp64 = f_shift[4], ratio, anchor (0: no anchor
 * warp, goofer_warp_bins' f_shift == NULL; else warp by f_shift even when all four are 1).  Note by note the bits of
 * goofer_warp_bins(f_shift or NULL, ratio). */
int goofer_warp_bins_ragged(goofer_ctx *ctx, const float *in, float *out, int64_t rows, int n_bins, int ld, const double *formants,
                            const int64_t *row_off, int n_notes, const double *note_args, void *stream);

/* gf.synthesize's time stretch (GOOFER.py:1019-1057) for a ragged batch in one launch: per note concat(x[:a],
 * stretch_feature(x[a:b], factor), x[b:]) of env_h and env_n ([rows x ld] fp32, the frame axis: row_off_in -> row_off_out,
 * (a, b) = row_cut[2i], row_cut[2i+1] note-relative) and of f0 and mask (fp32, the sample axis: sample_off_in -> sample_off_out,
 * sample_cut).  The stretched length is implied: out_len - a - (in_len - b); the region b - a must be >= 1 wherever it is
 * stretched to >= 1 element.  The arithmetic of goofer_stretch_rows, without its 65535-row limit. */
int goofer_stretch_ragged(goofer_ctx *ctx, const int64_t *row_off_in, const int64_t *row_off_out, const int64_t *row_cut,
                          const int64_t *sample_off_in, const int64_t *sample_off_out, const int64_t *sample_cut, int n_notes,
                          int64_t rows_out, int64_t samples_out, int n_cols, int ld, const float *env_h, const float *env_n,
                          float *env_h_out, float *env_n_out, const float *f0, const float *mask, float *f0_out, float *mask_out,
                          void *stream);

/* gf.gaussian_filter1d along the last axis of ragged fp64 rows (GOOFER.py:241-261: numpy 'reflect' padding, fp64
 * accumulate in tap order): row r is in[row_off[r] .. row_off[r+1]) (device CSR); taps are HOST memory, 2*radius+1. */
int goofer_gauss_rows_f64(goofer_ctx *ctx, const double *in, const int64_t *row_off, int n_rows, int64_t total, const double *taps,
                          int radius, double *out, void *stream);

/* apply_vocal_roughness (GOOFER.py:901-940; gf.synthesize's roughness_on layer) for a ragged batch: out = y + alpha_slewed *
 * highpass(y * (1 + sum_k h_k cos(2 pi cumsum(f_mod_k) / sr)) - y), f_mod_k = max(f0 / k * (1 + noise_amp * noise_k), 0) * mask.
 * noise_s [n_k x total_samples] fp64 = the smoothed noises (make_smooth_noise), alpha_slewed [total_samples] fp32 = the slewed
 * alpha * mask — both Gaussian filters of host draws / the mask (goofer_gauss_rows_f64); k_list / h_list are HOST arrays. */
int goofer_vocal_roughness(goofer_ctx *ctx, const float *y, const float *f0, const float *mask, const double *noise_s, int n_k,
                           const double *k_list, const double *h_list, double noise_amp, double hp_fc, const float *alpha_slewed,
                           const int64_t *sample_off, int n_notes, int64_t total_samples, float *out, void *stream);

/* dynamic_butter_filter (SillySampler.py:95-174) for a list of jobs (device array): src -> dst, fp32. */
int goofer_onepole_cascade(goofer_ctx *ctx, const float *src, float *dst, const float *f0, const goofer_onepole_job *jobs,
                           int n_jobs, void *stream);

/* The sample-domain post chain after the synth calls (SillySampler.py:1037-1182): su / sj layers, fry blend,
 * sd dryness, st tension, V/B/U mix, sa whisper blend, pd gain.  Notes without any of these keep their mix. */
int goofer_post_batch(goofer_ctx *ctx, const goofer_post *post, void *stream);

/* Finished audio as the reference's wav holds it (soundfile's default PCM_16, SillySampler.py:1184-1185): out[i] =
 * int16(round_half_even(clip(x[i], -1, 1 - 2^-15) * 32768)), the arithmetic of goofer_amd.render.write_wav.  Two bytes per
 * sample across PCIe instead of four. */
int goofer_pcm16(goofer_ctx *ctx, const float *x, int64_t n, int16_t *out, void *stream);

/* Standard normal draws of the jitter / growl flags on the device (noise.hip): out[sample_off[k] + i], float64, for every note
 * k with note_on[k] != 0 (NULL: every note); the samples of the other notes are not written.  The stream is defined:
 * Philox-4x32 with 10 rounds, key = seed ^ (params[k].seed[0] | params[k].seed[1] << 32) (the noise phases' key), counter
 * (i >> 1, stream_tag, 0, 0x6A09E667); the block's words w0..w3 give u1 = ((w0 | (w1 & 0x1FFFFF) << 32) + 1) * 2^-53,
 * u2 = (w2 | (w3 & 0x1FFFFF) << 32) * 2^-53, r = sqrt(-2 ln u1), sample 2q = r cos(2 pi u2), sample 2q + 1 = r sin(2 pi u2) — a
 * note's draws depend on its key and the tag only, not on the batch.  stream_tag: 0 f0 jitter, 1 harmonic volume jitter,
 * 2 breath volume jitter, 3 sub-harmonic f0 jitter, 4 growl.  growl_scale ([n_notes], or NULL for the plain normals z): writes
 * 0.5 * 2^(growl_scale[k] * z) instead (SillySampler.py:1063-1065 with scale = mix^2).  params, sample_off ([n_notes + 1], from
 * 0 to total_samples), note_on, growl_scale and out (16-byte aligned, the caller's) are device arrays; asynchronous on
 * `stream`; needs no plan.  GOOFER_EINVAL for a null pointer, a negative count, a tag outside 0..4 or an `out` that is not
 * 16-byte aligned (an odd element of a float64 array).  The counter word is 32 bits wide: a note of more than 2^33 samples
 * would repeat its stream. */
int goofer_normal_fill(goofer_ctx *ctx, uint64_t seed, const goofer_note_params *params, const int64_t *sample_off, int n_notes,
                       int64_t total_samples, int stream_tag, const unsigned char *note_on, const double *growl_scale, double *out,
                       void *stream);

/* The aperiodic branch's phases as a seeded reference run draws them (GOOFER.py:1151-1152), on the device (noise.hip): for note
 * k with T_k = frame_off[k + 1] - frame_off[k] frames, out[(frame_off[k] + t) * ld + b], b < n_bins, is element [b, t] of
 * np.random.default_rng(seed_k).uniform(0.0, 2 pi, (n_bins, T_k)).astype(np.float32), bit for bit: the layout goofer_batch.phi
 * takes.  The stream is numpy's PCG64: state <- state * 0x2360ED051FC65DA44385DF649FCCF645 + inc (mod 2^128), and from the NEW
 * state x = hi ^ lo, v = rotr64(x, hi >> 58), d = (v >> 11) * 2^-53 in float64, value = float32(0.0 + 2 pi * d) rounded to
 * nearest even; element [b, t] is draw b * T_k + t of its note (a 64-bit index), reached by the generator's jump-ahead.
 * Seeding stays with the caller: pcg_words holds four 64-bit words per note, (state lo, state hi, inc lo, inc hi) of
 * np.random.PCG64(seed_k).state; a note whose increment is even (a zero record: a real increment is odd) is not seeded, and
 * its rows are not written.  The columns n_bins .. ld - 1 are not written either.  pcg_words, frame_off ([n_notes + 1], from 0
 * to total_frames) and out are device arrays; asynchronous on `stream`; needs no plan and no scratch.  GOOFER_EINVAL for a null
 * pointer, a negative count, n_bins < 1 or ld < n_bins, pcg_words or frame_off not 8-byte aligned, out not 4-byte aligned. */
int goofer_phase_fill(goofer_ctx *ctx, const uint64_t *pcg_words, const int64_t *frame_off, int n_notes, int64_t total_frames,
                      int n_bins, float *out, int ld, void *stream);

/* The normals a reference process draws for the sh / sr jitter (GOOFER.py:653, 666) after np.random.seed(seed_k): numpy's legacy
 * global stream, `np.random.randn`, made on the device (noise.hip) for every note k of a ragged batch.  The stream:
 *   seeding  (np.random.seed(s), 0 <= s < 2^32) mt[0] = s, mt[i] = (1812433253 * (mt[i-1] ^ (mt[i-1] >> 30)) + i) mod 2^32 for
 *            i = 1..623; position 624 (the first draw regenerates the block); no cached normal
 *   block    of 624 words, for k = 0..623 in order and in place: y = (mt[k] & 0x80000000) | (mt[(k+1) % 624] & 0x7fffffff),
 *            mt[k] = mt[(k+397) % 624] ^ (y >> 1) ^ (y & 1 ? 0x9908b0df : 0); a word is tempered as it is drawn: y ^= y >> 11,
 *            y ^= (y << 7) & 0x9d2c5680, y ^= (y << 15) & 0xefc60000, y ^= y >> 18
 *   double   two consecutive words a, b: ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0 (exact)
 *   attempt  two doubles d0, d1 — always four words: x1 = 2 d0 - 1, x2 = 2 d1 - 1, r2 = x1 x1 + x2 x2 (two rounded products and
 *            one rounded sum, no fused multiply-add); rejected when r2 >= 1.0 or r2 == 0.0; otherwise f = sqrt(-2.0 * log(r2) / r2)
 *            (IEEE division and square root) and two normals in this order: f x2, then f x1
 *   randn(n) the next n normals; the second normal of a pair waits for the next call, so a note's consecutive randn calls are
 *            consecutive slices of one stream of normals.  A block is 156 whole attempts.
 * Everything but `log` is exact, so a value differs from the host's by what the two `log` differ in their last place, and the
 * acceptances (every later position of the stream) not at all.
 * stream_on holds three bytes per note: whether it draws the f0 jitter, the harmonic volume jitter, the breath volume jitter
 * (the reference's order).  With n = sample_off[k + 1] - sample_off[k], normal p of note k goes to its enabled stream p / n at
 * sample p % n: out_f0 / out_vol_h / out_vol_b [sample_off[k] + p % n], the concatenated float64 arrays goofer_batch.noise_f0 /
 * noise_vol_h / noise_vol_b take.  The samples of a stream that is off, and everything of a note with nothing on or without
 * samples, are not written; a NULL output drops the draws of its stream (they are still consumed).  attempts (int64 [n_notes],
 * or NULL): the attempts the note's normals took — the reference's generator has drawn 4 * attempts words — 0 for a note that
 * draws nothing.  A note walks at most 2 * ceil(m / 245) + 4 blocks for its m normals (a block yields 245 on average, with a
 * standard deviation of 10); one that would need more stops there and is reported by the next goofer_check.
 * seeds (uint32 [n_notes]), stream_on, sample_off ([n_notes + 1], from 0 to total_samples), the outputs and attempts are device
 * arrays; asynchronous on `stream`; needs no plan and no scratch.  GOOFER_EINVAL for a null seeds / stream_on / sample_off, no
 * output at all, a negative count, seeds not 4-byte aligned, sample_off, an output or attempts not 8-byte aligned. */
int goofer_legacy_normal_fill(goofer_ctx *ctx, const uint32_t *seeds, const unsigned char *stream_on, const int64_t *sample_off,
                              int n_notes, int64_t total_samples, double *out_f0, double *out_vol_h, double *out_vol_b,
                              int64_t *attempts, void *stream);

/* The same stream by job table: every legacy draw of gf.synthesize.  Job j draws the first n * n_dst normals after
 * np.random.seed(seed), and normal p goes to its destination p / n at sample p % n: dst[p / n][off[p / n] + p % n].  That is one
 * np.random.randn(n) per destination, in order, with the polar method's second value carried from one to the next (an odd n) —
 * the f0, sub-harmonic f0, harmonic volume and breath volume jitter of a note are one job of up to four destinations
 * (GOOFER.py:1069-1080, 1185-1191).  A NULL destination among the n_dst consumes its n draws and stores nothing; a job with
 * n <= 0 or n_dst == 0 draws nothing.  With GOOFER_LEGACY_F32 in flags every normal is rounded to float32 and widened again
 * before the store — np.random.randn(n).astype(np.float32) held in float64, make_smooth_noise's draw (GOOFER.py:894-899: one job
 * per roughness partial, seed 1337 + idx, one destination).  One workgroup per job, the arithmetic, the block bound and the
 * goofer_check report of goofer_legacy_normal_fill (which is the job table of a note's enabled streams: the same bits);
 * attempts (int64 [n_jobs], or NULL) as there.  Destinations of one call must not overlap.
 * jobs, everything a job points to and attempts are device arrays; asynchronous on `stream`; needs no plan and no scratch.  The
 * table is read on the device: the caller answers for n_dst <= 4 (larger counts as 4) and for off[k] + n staying inside dst[k].
 * GOOFER_EINVAL for a null jobs, a negative count, jobs or attempts not 8-byte aligned. */
#define GOOFER_LEGACY_F32 1u
typedef struct {
    uint32_t seed;              /* np.random.seed's one 32-bit word                                                   */
    uint32_t flags;             /* GOOFER_LEGACY_F32                                                                   */
    int64_t n;                  /* samples per destination                                                            */
    int32_t n_dst;              /* destinations in use, 0..4                                                          */
    int32_t reserved;
    double *dst[4];             /* device float64 arrays (NULL: that destination's draws are dropped)                 */
    int64_t off[4];             /* first element of the job in dst[k]                                                 */
} goofer_legacy_job;
int goofer_legacy_normal_jobs(goofer_ctx *ctx, const goofer_legacy_job *jobs, int n_jobs, int64_t *attempts, void *stream);

/* ---- phrase assembly: envelope and mix the notes of a batch into one track ------------------------------------------------
 * What UTAU leaves to a separate `wavtool`: every rendered note trimmed, enveloped, cross-faded with its neighbours and summed
 * onto one time line.  The reference has no counterpart; this is the definition (restated in float64 numpy by
 * tests/phrase_ref.py).
 *
 * A batch of n notes holds samples x[sample_off[i] .. sample_off[i+1]), len_i that difference (goofer_batch.mix with its CSR).
 * Note i has a record:
 *   start   track position of the note's first used sample, any sign
 *   skip    >= 0: samples dropped from the note's head (wavtool's stp)
 *   take    in [0, 2^24]: samples used
 *   pos[7]  knot positions in samples, non-decreasing, pos[0] == 0 and pos[6] == (float)take
 *   val[7]  linear gains, finite
 * For t in [0, total_out):  track[t] = sum_i g_i(u) * x_i[skip_i + u],  u = t - start_i,  over the notes with 0 <= u < take_i and
 * skip_i + u < len_i (beyond a note's end is silence; what falls before 0 or past total_out is dropped).  The sum runs in
 * ascending note index from +0.0f, each term one fp32 multiply, then one fp32 add (the library is built with
 * -ffp-contract=off).  The gain: k = the largest index with pos[k] <= (float)u — pos[6] = take > u, so k <= 5 and
 * pos[k+1] > pos[k] — and, in fp32 and in this order,
 *   g = val[k] + (val[k+1] - val[k]) * (((float)u - pos[k]) / (pos[k+1] - pos[k]))
 * Coincident knots are a step (the later value holds from that position on); nothing divides by zero. */
/* The tiling of the gather-sum mixers (this one and the stereo bus below; csrc/tile_mix.h): their planners' cover tables are laid
 * out for this number, and each mixer's own name is defined from it. */
#define GOOFER_MIX_TILE 2048         /* samples of a tile: one 256-thread workgroup, eight samples per thread */
#define GOOFER_PHRASE_TILE GOOFER_MIX_TILE
typedef struct {
    int64_t start;
    int32_t skip;
    int32_t take;
    float pos[7];
    float val[7];
} goofer_phrase_note;

/* Host side (no device, no handle): check the n records against note_len[n] (len_i, >= 0) and write the cover table of the
 * track's tiles of GOOFER_PHRASE_TILE samples, tiles = ceil(total_out / GOOFER_PHRASE_TILE): tile_off[tiles + 1] (CSR) and
 * tile_notes, the notes whose effective range [max(start, 0), min(start + min(take, len - skip), total_out)) meets the tile, in
 * ascending note index (a note with an empty effective range is in no tile).  *need = entries of tile_notes.  Returns 0 with
 * both arrays written; 1 when cap < *need (only *need is valid: grow, call again); GOOFER_EINVAL for a null argument, a negative
 * count or length, decreasing knots, a position or value that is not finite, pos[0] != 0, pos[6] != take, take outside
 * [0, 2^24], skip < 0, or a track of 2^31 tiles or more. */
int goofer_host_phrase_plan(const goofer_phrase_note *notes, const int64_t *note_len, int n, int64_t total_out, int64_t *tile_off,
                            int32_t *tile_notes, int64_t cap, int64_t *need);

/* The track (phrase.hip): out[0 .. total_out), every sample stored exactly once — zeros where no note sounds — so `out` needs
 * no clearing.  x, sample_off ([n + 1]), notes ([n], as validated by goofer_host_phrase_plan), tile_off and tile_notes (that
 * call's table for the same records, lengths and total_out) and out are device arrays of the caller; `out` must not overlap x.
 * One workgroup per tile, no atomics, no scratch; 16-byte stores when `out` is 16-byte aligned.  Asynchronous on `stream`;
 * needs no plan.  total_out == 0: nothing is launched; n == 0: zeros.  GOOFER_EINVAL for a null pointer (x and notes may be null
 * when n == 0), a negative count, x or out not 4-byte aligned, sample_off / notes / tile_off not 8-byte aligned. */
int goofer_phrase_mix(goofer_ctx *ctx, const float *x, const int64_t *sample_off, int n, const goofer_phrase_note *notes,
                      const int64_t *tile_off, const int32_t *tile_notes, int64_t total_out, float *out, void *stream);

/* ---- output-rate conversion: a ragged polyphase resampler ----------------------------------------------------------------
 * Every note and every track is rendered at the voicebank's rate; this converts finished audio to another one (44.1 -> 48 kHz
 * for a session, 96 kHz, ...) on the device, in front of goofer_pcm16 and the one download.  The reference has no counterpart;
 * this is the definition (restated in numpy by tests/rate_ref.py).
 *
 * Geometry.  g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, r = min(1, L / M).  Half width in input samples
 *   H = ceil(GOOFER_RATE_ZEROS / r) = (GOOFER_RATE_ZEROS * max(L, M) + L - 1) div L,
 * cutoff fc = GOOFER_RATE_ROLLOFF * r as a fraction of the input Nyquist rate.
 *
 * Taps (host, float64, stored as fp32).  The table is taps[L][2H], phase-major: row p holds h_p[j] for j = -H+1 .. H at column
 * j + H - 1.  With t = j - p / L:
 *   w(t) = I0(GOOFER_RATE_BETA * sqrt(1 - (t/H)^2)) / I0(GOOFER_RATE_BETA)  for |t| < H, else 0     (a Kaiser window)
 *   h    = fc * sinc(fc * t) * w(t),  sinc(z) = sin(pi z) / (pi z), sinc(0) = 1
 * Each row is divided by its float64 sum, then rounded to fp32 to nearest even.
 *
 * Output of a signal x of n samples: m = (n * L + M - 1) div M samples.  For 0 <= k < m, in int64,
 *   q = (k * M) div L,  p = (k * M) mod L,
 *   y[k] = sum over j = -H+1 .. H with 0 <= q + j < n of h_p[j] * x[q + j].
 * The sum runs in ascending j from +0.0f, each term one fp32 multiply, then one fp32 add (the library is built with
 * -ffp-contract=off).  For finite input, adding the out-of-range taps as products with zero gives the same bits (the
 * accumulator is never -0.0); non-finite input propagates exactly as the sum says.
 *
 * Refused (GOOFER_EINVAL): a rate below 1, sr_in == sr_out, max(L, M) > GOOFER_RATE_MAX_PHASES (the table stays under 67 000
 * floats: every pair among 8, 11.025, 16, 22.05, 24, 32, 44.1, 48, 88.2, 96 and 192 kHz but a few with L > 1024), a signal of
 * 2^31 samples or more.
 *
 * Of the definition (float64 sums on the fp32 table): a unit sine up to 0.8 of the lower Nyquist rate comes out within 2.6e-7 of
 * the analytic sine, a tone at 1.12 of the new Nyquist rate stays below 1.1e-7 after down-conversion, row sums are 1 within
 * 6.1e-8 and max_p sum_j |h_p[j]| <= 2.30; the fp32 sum defined above is within 7.1e-7. */
#define GOOFER_RATE_ZEROS 32
#define GOOFER_RATE_ROLLOFF 0.945
#define GOOFER_RATE_BETA 14.0
#define GOOFER_RATE_MAX_PHASES 1024

/* Host side (no device, no handle): the geometry of sr_in -> sr_out, the tap table and, for n signals whose samples lie back to
 * back with the CSR in_off[n + 1] (non-decreasing), out_off[n + 1], the CSR of the m_i.  *need = L * 2H, the floats of `taps`.
 * Returns 0 with L, M, H, taps, need and out_off written; 1 when cap < *need (only *need, *L, *M and *H are valid: grow, call
 * again); GOOFER_EINVAL for what the definition refuses, a null argument (in_off may be null when n == 0, taps when cap == 0), a
 * negative count or capacity, or offsets that decrease. */
int goofer_host_rate_plan(int sr_in, int sr_out, const int64_t *in_off, int n, int *L, int *M, int *H, float *taps, int64_t cap,
                          int64_t *need, int64_t *out_off);

/* The conversion (rate.hip): out[out_off[i] .. out_off[i+1]) = y of signal x[in_off[i] .. in_off[i+1]), every output sample stored
 * exactly once.  x, in_off ([n + 1]), taps ([L][2H]), out_off ([n + 1]) and out are device arrays of the caller, the geometry,
 * table and offsets those of goofer_host_rate_plan for the same in_off; `out` must not overlap x.  One thread per output sample,
 * no atomics, no scratch; the table is staged in LDS where it fits in 160 KiB (option "rate_lds").  Asynchronous on `stream` (the
 * output count is read on the device: a fixed grid walks the batch); needs no plan.  n == 0: nothing is launched.  GOOFER_EINVAL for a null pointer (all arrays may be null when n == 0), a negative count, L, M or H outside the
 * definition's range (1 <= L, M <= GOOFER_RATE_MAX_PHASES, H as defined), x, taps or out not 4-byte aligned, in_off or out_off
 * not 8-byte aligned. */
int goofer_rate_convert(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int L, int M, int H, const float *taps,
                        const int64_t *out_off, float *out, void *stream);

/* ---- look-ahead peak limiter ----------------------------------------------------------------------------------------------
 * goofer_pcm16 clamps to [-1, 1 - 2^-15]: whatever arrives above full scale is hard-clipped.  Notes are peak-normalised to 1
 * before `volume`, goofer_phrase_mix sums cross-faded neighbours, and goofer_rate_convert's rows have sum_j |h_p[j]| up to 2.30,
 * so a finished track can exceed 1.  This stage brings it under a ceiling on the device, at the output rate, immediately in
 * front of goofer_pcm16.  The reference has no counterpart; this is the definition (restated in numpy by tests/limit_ref.py).
 * All FIR and min / max, no recursion: an output sample depends on at most 4W + 1 input samples of its own signal, and a signal
 * gets the same bits alone as at any position in any batch.
 *
 * Parameters.  Ceiling c: fp32, 0 < c <= 1 (default 32767/32768).  Look-ahead W = floor(look_ms * sr / 1000 + 0.5) samples, in
 * float64 (default look_ms 5).  Refused (GOOFER_EINVAL): W < 1, W > GOOFER_LIMIT_MAX_LOOK, a non-finite or out-of-range c,
 * sr < 1, a signal of 2^31 samples or more.
 *
 * Table (host, float64, stored as fp32).  w[j] for j = -W .. W (at index j + W) is 1 + cos(pi j / (W + 1)), divided by the
 * float64 sum of the 2W + 1 values (taken in ascending j; 2W + 2 in the reals) and rounded to fp32 to nearest even.
 *
 * Per signal x[0 .. n), all arithmetic fp32, no contraction:
 *   1  a[i] = |x[i]|
 *   2  r[i] = a[i] > c ? c / a[i] : 1                 (the division correctly rounded)
 *   3  m[i] = min r[k] over k in [i - W, i + W] intersected with [0, n)
 *   4  d[i] = 1 - m[i]
 *   5  acc[i] = sum_j w[j] * d[clamp(i + j, 0, n - 1)], in ascending j from +0.0f, one rounded multiply and one rounded add
 *      per tap
 *   6  s[i] = max(1 - acc[i], 0)
 *   7  g[i] = min(s[i], r[i])
 *   8  y[i] = x[i] * g[i]
 * A signal with n = 0 produces nothing.  Statistics per signal, both exact: peak_in = max_i a[i] (0 for an empty signal),
 * min_gain = min_i g[i] (1 for an empty signal).
 *
 * Properties (tried in numpy, fp32, at W = 1, 7, 220 and c = 32767/32768, 0.891, 0.5).  Ceiling: every term of acc uses an m
 * whose window contains i, so in the reals s[i] <= r[i]; the final min takes care of the table's rounding; g <= r = fl(c / a)
 * and y = fl(a g), so |y[i]| <= c (1 + 2^-24)^2 (the tests use c (1 + 2^-22); worst seen c (1 + 2^-23)); at the default c
 * goofer_pcm16 of a limited track gives what an unclamped round would give.  Identity: where a <= c on all of [i - 2W, i + 2W]
 * every d is +0, acc is +0 and g is exactly 1, so a signal that never exceeds c comes back bit for bit — which is why the sum
 * is over the deficiency d and not over m.  Non-finite samples follow the arithmetic as written (a NaN asks for gain 1 and
 * stays NaN).  Loudness metering and normalisation live in goofer_loudness_* below, in front of this stage; true-peak
 * (oversampled) detection is the next section: goofer_limit_tp is this limiter with a[i] the oversampled envelope. */
#define GOOFER_LIMIT_MAX_LOOK 1024
#define GOOFER_LIMIT_TILE 4096
#define GOOFER_LIMIT_CEILING (32767.0f / 32768.0f)
#define GOOFER_LIMIT_LOOK_MS 5.0

/* Host side (no device, no handle): W, the table and the tile table for n signals whose samples lie back to back with the CSR
 * in_off[n + 1] (non-decreasing; the limited signals lie at the same offsets).  need[0] = 2W + 1, the floats of `taps`;
 * need[1] = sum_i ceil(len_i / GOOFER_LIMIT_TILE), the tiles: `tiles` holds one pair of int32 per tile, (signal, tile of that
 * signal), in ascending order — the workgroups of goofer_limit.  Returns 0 with W, taps, tiles and need written; 1 when
 * taps_cap < need[0] or tiles_cap (in pairs) < need[1] (only *W and need are valid: grow, call again); GOOFER_EINVAL for what the
 * definition refuses, a null argument (in_off may be null when n == 0, taps / tiles when their capacity is 0), a negative count
 * or capacity, or offsets that decrease. */
int goofer_host_limit_plan(int sr, double look_ms, float c, const int64_t *in_off, int n, int *W, float *taps, int64_t taps_cap,
                           int32_t *tiles, int64_t tiles_cap, int64_t *need);

/* The limiter (limit.hip): out[in_off[i] .. in_off[i+1]) = y of signal x[in_off[i] .. in_off[i+1]), every sample stored exactly
 * once; peak_in[i] and min_gain[i] (fp32 [n]) the statistics, set by the call (they need not be cleared).  x, in_off ([n + 1]),
 * taps ([2W + 1]), tiles ([n_tiles] pairs), out, peak_in and min_gain are device arrays of the caller; W, taps, tiles and n_tiles
 * those of goofer_host_limit_plan for the same in_off, total = in_off[n].  One workgroup per tile: the tile's r with 2W samples of
 * halo on either side in LDS (halos are read from x again, so `out` must not overlap x: in place is a race), window minima by
 * doubling, the tap sum from LDS, statistics by integer atomics on the fp32 bits.  A tile with nothing above c, halo included,
 * copies its samples (option "limit_skip").  No scratch buffer, no plan; asynchronous on `stream`.  n == 0: nothing is launched;
 * total == 0: only the statistics are set.  GOOFER_EINVAL, with nothing launched, for a null pointer (all arrays may be null when
 * n == 0; x, out and tiles when total == 0), a negative count, W or c outside the definition's range, an n_tiles that is not
 * between ceil(total / GOOFER_LIMIT_TILE) and that plus n, x, taps, tiles, out, peak_in or min_gain not 4-byte aligned, in_off not
 * 8-byte aligned, or an out that overlaps x. */
int goofer_limit(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int W, const float *taps, float c,
                 const int32_t *tiles, int64_t n_tiles, float *out, float *peak_in, float *min_gain, void *stream);

/* ---- true-peak detection ---------------------------------------------------------------------------------------------------
 * The limiter above looks at sample values.  The signal a converter reconstructs from them passes between them, and can pass
 * higher: a full-scale sine at a quarter of the sample rate, sampled at 45 degrees, has a sample peak of -3.01 dBFS and a true
 * peak of 0 dBTP, and the limiter returns it bit for bit at any ceiling down to -3 dBFS.  A delivery specification of "-16 LUFS,
 * -1 dBTP" means the true peak.  This is the other half of ITU-R BS.1770-4 (Annex 2) beside goofer_loudness_*: the signal
 * reconstructed at R times its rate by a short windowed sinc, as a meter (goofer_true_peak) and as what the limiter watches
 * (goofer_limit_tp).  The definition is this project's own (restated in numpy by tests/true_peak_ref.py).
 *
 * Geometry.  sr: an integer, GOOFER_TP_MIN_SR <= sr <= GOOFER_TP_MAX_SR; anything else is refused (GOOFER_EINVAL).
 * Oversampling factor R = 4 for sr < 96000, else 2: the oversampled rate is at least 32 kHz and reaches 192 kHz from 48 kHz
 * on.  Z = GOOFER_TP_ZEROS: a row has 2Z = 24 taps.
 *
 * Table (host, float64, stored as fp32).  taps[R - 1][2Z], one row per phase p = 1 .. R - 1 (phase 0 is the sample itself and
 * is never filtered): row p - 1 holds h_p[j] for j = -Z+1 .. Z at column j + Z - 1.  With t = j - p / R:
 *   h = sinc(t) * w(t),  sinc(z) = sin(pi z) / (pi z),
 *   w(t) = I0(GOOFER_TP_BETA * sqrt(1 - (t/Z)^2)) / I0(GOOFER_TP_BETA)      (goofer_rate_convert's Kaiser window, half width Z)
 * Each row is divided by its float64 sum (taken in ascending j), then rounded to fp32 to nearest even.
 *
 * Per signal x[0 .. n), with x outside [0, n) taken as 0; all arithmetic fp32, no contraction:
 *   u[i] = max over p of | sum_j h_p[j] * x[i + j] |   for 0 <= i < n: the reconstructed signal at the R - 1 grid points strictly
 *          between samples i and i + 1.  Each sum runs in ascending j from +0.0f, one rounded multiply and one rounded add per
 *          tap, the products with the zeros outside the signal included.
 *   e[i] = max(|x[i]|, u[i], u[i - 1]), u[-1] = 0.  A sample's gain shapes the reconstruction on both sides of it, so a sample
 *          answers for both neighbouring intervals.
 * Meter: true_peak = max_i e[i], 0 for an empty signal; exact, a maximum of fp32 values.
 * Limiter with true-peak detection: step 1 of goofer_limit's definition becomes a[i] = e[i]; steps 2 to 8 stay word for word.
 * peak_in becomes max_i e[i]; min_gain is unchanged.  An output sample depends on 4W + 1 + 2Z input samples of its own signal,
 * and a signal gets the same bits alone as at any position in any batch.  The identity property carries over: where e <= c on
 * all of [i - 2W, i + 2W], g[i] is exactly 1, so a signal whose true peak stays at or under c comes back bit for bit.
 * Every max above is fmaxf, started from 0 for u: a NaN operand is ignored.  A NaN sample makes the sums it enters NaN, so those
 * u are 0 unless another phase is finite, and its own e is 0: it asks for gain 1 and stays NaN, as in goofer_limit.  An infinite
 * sample has e = inf, r = 0 and becomes NaN, as there; its neighbours' sums are infinite or NaN as the arithmetic says.
 *
 * Properties (measured on the float64 flavour of tests/true_peak_ref.py, on the fp32 table; tests/test_true_peak_plan.py holds
 * them).  (a) On unit sines at 0.25, 0.3, 0.4 and 0.45 of the sample rate, over 13 start phases, away from the signal's ends,
 * the meter reads between -0.40 dB (at 0.4; R = 2: -0.58 dB at 0.25) and +0.0004 dB: the under-read is the grid of R points per
 * sample itself (cos(pi f / R) of a peak that falls midway between two grid points), not the table; the quarter-rate sine at
 * 45 degrees reads 0.000 dBTP.  (b) S = max_p sum_j |h_p[j]| = 2.2064, row sums are 1 within 3.1e-8: u <= S max |x|.
 * (c) Gain smoothing does not commute with interpolation, so the true peak of the limiter's output is held to c closely, not
 * exactly: on five inputs of 12 000 samples (noise low-passed at 0.9, 0.5 and 1.0 of the Nyquist rate with peaks 3, 1.5 and 8,
 * a 0.95 square wave, a chirp of amplitude 1.4) at c = 0.891, 0.5 and 32767/32768, the 4-phase true peak of the output exceeds
 * c by at most 4.96e-3 relative (0.043 dB) at W = 7, 9.85e-6 at W = 48 and 7.9e-8 at W = 240 — the shorter the look-ahead, the
 * faster the gain moves between two samples and the weaker the guarantee; at the default 5 ms it is below an fp32 rounding of
 * the samples.  goofer_limit on the same inputs leaves true peaks up to 3.8 dB above c (noise, W = 7; 1.9 dB at W = 240). */
#define GOOFER_TP_ZEROS 12
#define GOOFER_TP_BETA 8.0
#define GOOFER_TP_MIN_SR 8000
#define GOOFER_TP_MAX_SR 192000

/* Host side (no device, no handle): R, Z and the table at `sr`.  *need = (R - 1) * 2Z, the floats of `taps`.  Returns 0 with R,
 * Z, taps and need written; 1 when cap < *need (only *need, *R and *Z are valid: grow, call again); GOOFER_EINVAL for a rate out
 * of range, a null argument (taps may be null when cap == 0) or a negative capacity.  The tile table of a call below is
 * goofer_host_limit_plan's own, for the same in_off. */
int goofer_host_true_peak_plan(int sr, int *R, int *Z, float *taps, int64_t cap, int64_t *need);

/* The meter (limit.hip): peak[i] (fp32 [n], set by the call) = true_peak of signal x[in_off[i] .. in_off[i+1]).  x, in_off
 * ([n + 1]), taps ([R - 1][2Z]), tiles ([n_tiles] pairs) and peak are device arrays of the caller; R, Z and taps those of
 * goofer_host_true_peak_plan, tiles and n_tiles those of goofer_host_limit_plan for the same in_off (any ceiling and look-ahead),
 * total = in_off[n].  One workgroup per tile: the tile's x with Z samples of halo on either side in LDS, a thread makes e of
 * eight consecutive samples from a window sliding through its registers, the maximum goes to the signal's word by an integer
 * atomic on the fp32 bits.  Every tile computes: a meter has no ceiling under which it could stop.  No scratch buffer, no plan;
 * asynchronous on `stream`; the same bits alone as in any batch.  n == 0: nothing is launched; total == 0: zeros.
 * GOOFER_EINVAL, with nothing launched, for a null pointer (all arrays may be null when n == 0; x and tiles when total == 0), a
 * negative count, R not 2 or 4, Z not GOOFER_TP_ZEROS, an n_tiles that is not between ceil(total / GOOFER_LIMIT_TILE) and that
 * plus n, x, taps, tiles or peak not 4-byte aligned, in_off not 8-byte aligned. */
int goofer_true_peak(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int R, int Z, const float *taps,
                     const int32_t *tiles, int64_t n_tiles, float *peak, void *stream);

/* The limiter with true-peak detection (limit.hip): goofer_limit's arguments and contract, with R, Z and tp_taps of
 * goofer_host_true_peak_plan.  The kernel is goofer_limit's with another first step: x of [t0 - 2W - Z, t0 + T + 2W + Z) staged
 * in LDS, e and r = c / e made from it.  A tile whose e never exceeds c, halo included, copies its samples (option
 * "limit_tp_skip"; the identity property: the same bits).  There is no exit in front of the interpolation: peak_in is the
 * maximum of e, which a tile that did not interpolate could not report.  GOOFER_EINVAL as goofer_limit, and for R not 2 or 4, Z
 * not GOOFER_TP_ZEROS, a null or misaligned tp_taps. */
int goofer_limit_tp(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int W, const float *taps, float c,
                    const int32_t *tiles, int64_t n_tiles, float *out, float *peak_in, float *min_gain, int R, int Z, const float *tp_taps,
                    void *stream);

/* The tiling of the three stages that carry a recurrence over a signal (loudness, compressor, equaliser; csrc/tile_scan.h): their
 * planners' tile tables and powers are laid out for these numbers, and each stage's own names below are defined from them. */
#define GOOFER_SCAN_SPT 16           /* samples of a run: one thread's */
#define GOOFER_SCAN_LEVELS 8         /* 2^8 runs in a tile; 2^8 threads in a round of the tile-to-tile carry */
#define GOOFER_SCAN_TILE 4096        /* samples of a tile: SPT << LEVELS */
#define GOOFER_SCAN_RUN_TILES 16     /* tiles a thread of a tile-to-tile carry walks: RUN_TILES << LEVELS = 4096 tiles a round */

/* ---- loudness metering and normalisation ------------------------------------------------------------------------------------
 * The limiter watches peaks; this stage watches level: a signal's integrated loudness measured on the device and the signal
 * scaled to a target, in front of the limiter (mix, rate conversion, loudness, limiter, int16).  The definition is this
 * project's own, after ITU-R BS.1770-4 for one channel (restated in numpy by tests/loudness_ref.py).  A signal gets the same
 * bits alone as at any position in any batch, on every run: no floating-point atomics.
 *
 * Parameters.  sr: an integer, GOOFER_LOUDNESS_MIN_SR <= sr <= GOOFER_LOUDNESS_MAX_SR.  target: LUFS, finite, or NaN for
 * "measure only"; max_gain_db in [0, GOOFER_LOUDNESS_MAX_GAIN_DB_CAP] (default GOOFER_LOUDNESS_MAX_GAIN_DB).  Anything else is
 * refused (GOOFER_EINVAL).
 *
 * K-weighting (host, float64): two biquads from the analogue prototypes by the bilinear transform.
 *   Shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / sr), Vh = 10^(G/20),
 *     Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2;
 *     b = [(Vh + Vb K/Q + K^2), 2 (K^2 - Vh), (Vh - Vb K/Q + K^2)] / a0,  a = [2 (K^2 - 1), (1 - K/Q + K^2)] / a0
 *   High-pass: f0 = 38.13547087602444, Q = 0.5003270373238773; K = tan(pi f0 / sr), a0 = 1 + K/Q + K^2;
 *     b = [1, -2, 1],  a = [2 (K^2 - 1), (1 - K/Q + K^2)] / a0
 * At 48 kHz these are the standard's table within 9e-16.  coef[10] = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2.
 *
 * Per signal x[0 .. n), zero history in front of every signal, all recurrences and sums in float64 (an fp32 state misses the
 * tolerance below by a factor of 200: the high-pass has poles of radius 0.9950 at 48 kHz):
 *   u[i] = b0 x[i] + b1 x[i-1] + b2 x[i-2] - a1 u[i-1] - a2 u[i-2]       (shelf), then v from u likewise (high-pass)
 *   S = floor(sr / 10 + 0.5);  E[k] = sum v[i]^2 over kS <= i < (k+1)S  for k < Kn = floor(n / S)   (a trailing partial
 *     segment is not counted)
 *   z[j] = (E[j] + E[j+1] + E[j+2] + E[j+3]) / (4S)  for j < max(0, Kn - 3)          (400 ms blocks, 75 % overlap)
 *   absolute gate: z[j] > 10^((-70 + 0.691) / 10);  relative gate: z[j] > 0.1 * mean of z over the absolutely gated blocks
 *     (both in the linear domain: no logarithm decides a gate)
 *   L = -0.691 + 10 log10(mean of z over the blocks passing both gates), -inf when none passes
 *   momentary_max = -0.691 + 10 log10(max_j z[j]), -inf without a block
 *   g = fp32(min(10^((target - L) / 20), 10^(max_gain_db / 20))); exactly 1.0f when L is -inf or when measuring only
 *   y[i] = x[i] * g, one rounded fp32 multiply
 * The sums may be taken in any order.  A NaN sample makes E NaN from its segment on; where any z[j] is NaN, L, momentary_max and
 * g are NaN (a NaN is not dropped by a gate).  An infinite sample leaves E, L, momentary_max and g of its signal unspecified from
 * its segment on (non-finite or not: carrying the state by matrix powers multiplies their structural zeros by it, which the
 * recurrence as written does not).  Either way the other signals of the batch are untouched.
 *
 * The recurrence is of order 4 with state s = (u[i-1], u[i-2], v[i-1], v[i-2]); with A its 4x4 transition matrix for x = 0, a
 * run of m samples from state s ends in A^m s + (the end state of the same run from s = 0).  The kernels cut a signal into
 * tiles of GOOFER_LOUDNESS_TILE samples and a tile into runs of GOOFER_LOUDNESS_SPT, and carry the state across them with
 * mats[k] = A^(GOOFER_LOUDNESS_SPT * 2^k), k < GOOFER_LOUDNESS_MATS (row-major, float64; by repeated squaring on the host in long
 * double, rounded once: squaring in float64 costs the tolerance at 192 kHz).
 * Tolerance: |E[k] - E_longdouble[k]| <= 2^-26 max_k E_longdouble[k] per signal, which keeps g within one fp32 ulp. */
#define GOOFER_LOUDNESS_MIN_SR 8000
#define GOOFER_LOUDNESS_MAX_SR 192000
#define GOOFER_LOUDNESS_MAX_GAIN_DB 20.0
#define GOOFER_LOUDNESS_MAX_GAIN_DB_CAP 60.0
#define GOOFER_LOUDNESS_TILE GOOFER_SCAN_TILE
#define GOOFER_LOUDNESS_SPT GOOFER_SCAN_SPT
#define GOOFER_LOUDNESS_LEVELS GOOFER_SCAN_LEVELS
#define GOOFER_LOUDNESS_RUN_TILES GOOFER_SCAN_RUN_TILES
#define GOOFER_LOUDNESS_MATS 20      /* A^16 .. A^(16 * 2^19): 8 for the 256 runs of a tile, A^4096 for a tile, 8 from A^(4096 * 16) on for 256 runs of 16 tiles */
#define GOOFER_LOUDNESS_SLOTS 8      /* segments a tile can touch: S >= 800 */

/* Host side (no device, no handle): for n signals whose samples lie back to back with the CSR in_off[n + 1] (non-decreasing),
 * S, coef[10], mats[GOOFER_LOUDNESS_MATS][16], the segment CSR seg_off[n + 1] (signal i has floor(len_i / S) segments) and the
 * tile table: need[0] = sum_i ceil(len_i / GOOFER_LOUDNESS_TILE) pairs of int32 (signal, tile of that signal), ascending.
 * Returns 0 with everything written; 1 when tiles_cap (in pairs) < need[0] (only *S and need are valid: grow, call again);
 * GOOFER_EINVAL for an sr out of range, a null argument (in_off may be null when n == 0, tiles when tiles_cap == 0), a negative
 * count or capacity, offsets that decrease, a signal of 2^31 samples or more. */
int goofer_host_loudness_plan(int sr, const int64_t *in_off, int n, int *S, double *coef, double *mats, int64_t *seg_off,
                              int32_t *tiles, int64_t tiles_cap, int64_t *need);

/* The measurement (loudness.hip).  x, in_off ([n + 1]), coef, mats, seg_off ([n + 1]) and tiles are device arrays of the
 * caller, S and the tables those of goofer_host_loudness_plan for the same in_off, total = in_off[n].  Outputs, device arrays:
 * seg_energy, float64 [seg_off[n]], the E[k] (the momentary-loudness curve follows from them); loud, float64 [n][2]: L and
 * momentary_max; gain, fp32 [n]: g.  Four launches in stream order, and no workgroup ever waits for another: (A) a workgroup
 * per tile runs its samples from a zero state and scans the runs' end states into the tile's; (B) a workgroup per signal scans the
 * tiles' end states, 4096 at a time, into the tiles' start states; (C) every tile again, from its start state, with v^2 summed
 * per segment into a slot of its own per (tile, segment); (D) a workgroup per signal sums the slots in a fixed order, forms the
 * blocks, gates them and writes L, momentary_max and g.  x is read twice and nothing of the signal's size is written.
 * Scratch by the caller-scratch protocol: with scratch NULL the size goes to *scratch_bytes and nothing runs.  Asynchronous on
 * `stream`.  n == 0: nothing is launched.  GOOFER_EINVAL, with nothing launched, for a null pointer (all arrays may be null when
 * n == 0; x and tiles when total == 0), a negative count, S, target or max_gain_db outside the definition's range, an n_tiles
 * that is not between ceil(total / GOOFER_LOUDNESS_TILE) and that plus n, x or gain not 4-byte aligned, the others not 8-byte
 * aligned, or a scratch block that is too short. */
int goofer_loudness_measure(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int S, const double *coef,
                            const double *mats, const int64_t *seg_off, const int32_t *tiles, int64_t n_tiles, double target,
                            double max_gain_db, double *seg_energy, double *loud, float *gain, void *scratch, int64_t *scratch_bytes,
                            void *stream);

/* out[i] = x[i] * gain[signal of i] over the ragged batch: one rounded fp32 multiply, every sample stored once.  gain is the
 * device array goofer_loudness_measure wrote: it never visits the host.  out == x is allowed (there is no halo); any other
 * overlap is refused.  Asynchronous on `stream`; n == 0 or total == 0: nothing is launched. */
int goofer_loudness_apply(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, const float *gain, float *out,
                          void *stream);

/* ---- dynamic range compressor ----------------------------------------------------------------------------------------------
 * Phrase mix, loudness and the limiter are linear or protect peaks; this stage evens out level: a feed-forward log-domain
 * compressor with a smooth decoupled peak detector behind the gain computer (after Giannoulis, Massberg and Reiss, 2012), in
 * front of the loudness stage (mix, rate conversion, compressor, loudness, limiter, int16).  The definition is this project's
 * own (restated in numpy by tests/compress_ref.py).  A signal gets the same bits alone as at any position in any batch, on
 * every run: no floating-point atomics.
 *
 * Parameters.  sr: an integer, GOOFER_COMPRESS_MIN_SR <= sr <= GOOFER_COMPRESS_MAX_SR.  threshold_db T in [-80, 0]; ratio R in
 * [1, +inf]; knee_db W in [0, 40] (default 6); attack_ms in [0, 1000] (default 5); release_ms in [0, 5000] (default 100);
 * makeup_db M in [-24, 24] (default 0).  Anything else, a NaN included, is refused (GOOFER_EINVAL).
 *
 * Coefficients (host, float64): aA = attack_ms == 0 ? 0 : exp(-1 / (attack_ms * 1e-3 * sr)), aR likewise from release_ms,
 * s = 1/R - 1, in [-1, 0].  coef[GOOFER_COMPRESS_COEF] = T, W, s, M, aR, aA.
 *
 * Per signal x[0 .. n), zero state in front of every signal, everything in float64 until the last step:
 *   a[i]  = max(|x[i]|, 1e-6);  xg[i] = 20 log10 a[i];  d = xg[i] - T
 *   xl[i] = 0                        if 2d < -W
 *         = -s (d + W/2)^2 / (2W)    if |2d| <= W   (W > 0)
 *         = -s d                     otherwise                  (xl >= 0: the reduction asked for, in dB)
 *   y1[i] = max(xl[i], aR y1[i-1] + (1 - aR) xl[i])             (release; y1[-1] = 0)
 *   yl[i] = aA yl[i-1] + (1 - aA) y1[i]                         (attack;  yl[-1] = 0)
 *   g[i]  = 10^((M - yl[i]) / 20), exactly 1 where M - yl[i] == 0
 *   y[i]  = fp32(double(x[i]) * g[i])                           (one rounding to fp32)
 * Statistic per signal: max_reduction = max_k yl[k], float64 dB, 0 for a signal without a sample.  Optional output: the curve
 * yl, float64 [total].
 *
 * Identity: where every sample has 20 log10 a <= T - W/2 and M == 0, xl, y1 and yl are exactly 0 and g exactly 1: the signal
 * comes back bit for bit.  Non-finite samples: a non-finite sample leaves its own signal unspecified from that sample on
 * (max_reduction included); the other signals of the batch are untouched.
 *
 * The release stage is a recurrence with a max in it.  One sample is the map f(y) = max(C, A y + B) with C = xl, A = aR,
 * B = (1 - aR) xl; two such maps compose to one of the same form, C' = max(C2, A2 C1 + B2), A' = A2 A1, B' = A2 B1 + B2, and
 * the composition is associative: a scan.  Samples past a signal's end count as xl = 0 (no later tile reads that state), so
 * all elements of a scan level share A, a power of aR from the host, and only (C, B) are carried; xl >= 0 and the state starts
 * at 0, so C = 0 is the neutral element (never -inf: A underflows to 0 over many tiles, and 0 * -inf is NaN).  C of a prefix
 * is the state behind it from the true start, B the linear path alone (B <= C).  The attack stage is a linear scan over y1 with
 * powers of aA.  pows[2][GOOFER_COMPRESS_POWS]: aR^(GOOFER_COMPRESS_SPT * 2^k), then aA^(...) likewise, each by one
 * long-double pow on the host, rounded once.
 * Tolerance: |yl - yl_ref| <= 2^-22 dB, which keeps g within 2^-25 (an error of e dB moves g by a relative 0.1151 e); with the
 * one fp32 rounding, |y - y_ref| <= 2^-23 |y_ref| + 2^-149 per sample.  An fp32 detector state does not hold it (eps / (1 - a),
 * a up to 0.99999). */
#define GOOFER_COMPRESS_MIN_SR 8000
#define GOOFER_COMPRESS_MAX_SR 192000
#define GOOFER_COMPRESS_KNEE_DB 6.0
#define GOOFER_COMPRESS_ATTACK_MS 5.0
#define GOOFER_COMPRESS_RELEASE_MS 100.0
#define GOOFER_COMPRESS_FLOOR 1e-6   /* the least |x| the level detector sees: -120 dB */
#define GOOFER_COMPRESS_TILE GOOFER_SCAN_TILE
#define GOOFER_COMPRESS_SPT GOOFER_SCAN_SPT
#define GOOFER_COMPRESS_LEVELS GOOFER_SCAN_LEVELS
#define GOOFER_COMPRESS_COEF 6
#define GOOFER_COMPRESS_POWS 20      /* a^16 .. a^(16 * 2^19): 8 for the 256 runs of a tile, a^4096 for a tile, 8 from a^(4096 * 16) on for 256 runs of 16 tiles */
#define GOOFER_COMPRESS_RUN_TILES GOOFER_SCAN_RUN_TILES   /* tiles a thread of the carry kernels walks */
#define GOOFER_COMPRESS_ROUND_TILES (GOOFER_SCAN_RUN_TILES << GOOFER_SCAN_LEVELS)   /* 4096 tiles the carry kernels take per round: 256 threads of GOOFER_COMPRESS_RUN_TILES; the state in front of a round goes through its first thread */

/* Host side (no device, no handle): for n signals whose samples lie back to back with the CSR in_off[n + 1] (non-decreasing),
 * coef[GOOFER_COMPRESS_COEF], pows[2 * GOOFER_COMPRESS_POWS] and the tile table: need[0] = sum_i ceil(len_i /
 * GOOFER_COMPRESS_TILE) pairs of int32 (signal, tile of that signal), ascending.  Returns 0 with everything written; 1 when
 * tiles_cap (in pairs) < need[0] (only need is valid: grow, call again); GOOFER_EINVAL for a parameter outside the
 * definition's range, a null argument (in_off may be null when n == 0, tiles when tiles_cap == 0), a negative count or
 * capacity, offsets that decrease, a signal of 2^31 samples or more. */
int goofer_host_compress_plan(int sr, double threshold_db, double ratio, double knee_db, double attack_ms, double release_ms,
                              double makeup_db, const int64_t *in_off, int n, double *coef, double *pows, int32_t *tiles,
                              int64_t tiles_cap, int64_t *need);

/* The compressor (compress.hip).  x, in_off ([n + 1]), coef, pows and tiles are device arrays of the caller, the tables those
 * of goofer_host_compress_plan for the same in_off, total = in_off[n].  Outputs, device arrays: out, fp32 [total], y;
 * max_reduction, float64 [n]; curve, float64 [total], yl, or NULL: not written.  Five launches in stream order, and no
 * workgroup ever waits for another: (1) a workgroup per tile composes its samples' release maps from the neutral element;
 * (2) a workgroup per signal scans the tiles' maps, GOOFER_COMPRESS_ROUND_TILES at a time, into the release state in front of
 * every tile; (3) every tile again: y1 from its true start, the attack recurrence from zero, the tile's end state; (4) a
 * workgroup per signal scans those into the attack state in front of every tile; (5) every tile a third time: y1, yl and g from
 * the true states, y stored once, the curve stored, and the tile's greatest yl folded into max_reduction by an integer atomic
 * maximum over the bits of the non-negative values.  x is read three times and written once.  out == x is allowed (there is no
 * halo); any other overlap of out with x is refused.  Scratch by the caller-scratch protocol: with scratch NULL the size goes
 * to *scratch_bytes and nothing runs.  Asynchronous on `stream`.  n == 0: nothing is launched.  GOOFER_EINVAL, with nothing
 * launched, for a null pointer (all arrays may be null when n == 0; x, tiles and out when total == 0), a negative count, an
 * n_tiles that is not between ceil(total / GOOFER_COMPRESS_TILE) and that plus n, x, tiles or out not 4-byte aligned, the
 * others not 8-byte aligned, or a scratch block that is too short. */
int goofer_compress(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, const double *coef, const double *pows,
                    const int32_t *tiles, int64_t n_tiles, float *out, double *max_reduction, double *curve, void *scratch,
                    int64_t *scratch_bytes, void *stream);

/* ---- parametric equaliser -------------------------------------------------------------------------------------------------
 * Every other stage of the finishing chain acts on level or peaks; this one shapes the spectrum: a cascade of up to
 * GOOFER_EQ_MAX_BANDS biquads over every signal of a ragged batch, behind the rate conversion and in front of the compressor
 * (mix, rate conversion, equaliser, compressor, loudness, limiter, int16).  The definition is this project's own (restated in
 * numpy by tests/eq_ref.py).  A signal gets the same bits alone as at any position in any batch, on every run: no floating-point
 * atomics.
 *
 * Bands.  A plan has K bands, 0 <= K <= GOOFER_EQ_MAX_BANDS, shared by the whole batch; a band is (kind, f0_hz, gain_db, q),
 * kind one of GOOFER_EQ_HIGHPASS, _LOWPASS, _LOWSHELF, _HIGHSHELF, _PEAK, _NOTCH.  sr: an integer, GOOFER_EQ_MIN_SR <= sr <=
 * GOOFER_EQ_MAX_SR.  sr / GOOFER_EQ_F_MIN_DIV <= f0_hz <= GOOFER_EQ_F_MAX_REL sr; GOOFER_EQ_Q_MIN <= q <= GOOFER_EQ_Q_MAX
 * (GOOFER_EQ_SHELF_Q_MAX for the two shelves);
 * |gain_db| <= GOOFER_EQ_MAX_GAIN_DB for the shelves and the peak, gain_db == 0 for the others, which ignore it.  Anything else,
 * a NaN included, is refused (GOOFER_EINVAL).  The lowest f0, the highest q and the greatest gain are measured, not chosen: see
 * the tolerance.
 *
 * Coefficients (host, float64): the Audio-EQ-Cookbook biquads.  w0 = 2 pi f0 / sr, c = cos w0, s = sin w0, alpha = s / (2 q),
 * A = 10^(gain_db / 40), r = 2 sqrt(A) alpha:
 *   highpass   b = [(1 + c) / 2, -(1 + c), (1 + c) / 2]                        a = [1 + alpha, -2 c, 1 - alpha]
 *   lowpass    b = [(1 - c) / 2, 1 - c, (1 - c) / 2]                           a = [1 + alpha, -2 c, 1 - alpha]
 *   notch      b = [1, -2 c, 1]                                                a = [1 + alpha, -2 c, 1 - alpha]
 *   peak       b = [1 + alpha A, -2 c, 1 - alpha A]                            a = [1 + alpha / A, -2 c, 1 - alpha / A]
 *   lowshelf   b = [A ((A+1) - (A-1) c + r), 2 A ((A-1) - (A+1) c), A ((A+1) - (A-1) c - r)]
 *              a = [(A+1) + (A-1) c + r, -2 ((A-1) + (A+1) c), (A+1) + (A-1) c - r]
 *   highshelf  b = [A ((A+1) + (A-1) c + r), -2 A ((A-1) + (A+1) c), A ((A+1) + (A-1) c - r)]
 *              a = [(A+1) - (A-1) c + r, 2 ((A-1) - (A+1) c), (A+1) - (A-1) c - r]
 * each divided by its a0.  coef[5 K] = b0 b1 b2 a1 a2 per band, in band order.
 *
 * Identity.  A peak, lowshelf or highshelf band with gain_db == 0 is the identity in exact arithmetic (b = a) and is dropped by
 * the planner: K counts the bands that are left.  With K == 0 the output is a copy of the input, the same bits.
 *
 * Per signal x[0 .. n), zero history in front of every signal, all recurrences in float64, no contraction:
 *   u_0 = x
 *   u_k[i] = b0 u_(k-1)[i] + b1 u_(k-1)[i-1] + b2 u_(k-1)[i-2] - a1 u_k[i-1] - a2 u_k[i-2]    for k = 1 .. K, with band k's coef
 *   y[i] = fp32(u_K[i]), rounded once
 * A NaN sample makes its own signal NaN from that sample on.  An infinite sample leaves the rest of its signal unspecified, for
 * the reason the loudness section gives (matrix powers multiply their structural zeros by it).  Either way the other signals of
 * the batch are untouched.
 *
 * The cascade is linear with the state s = (u_1[i-1], u_1[i-2], .., u_K[i-1], u_K[i-2]): a run of m samples from s ends in
 * T^m s + (the end state of the same run from s = 0), T the 2K x 2K transition matrix for x = 0 — block lower triangular in
 * 2 x 2 blocks, and the diagonal block of section k in T^m is that section's own 2 x 2 matrix to the m.  The kernels cut a
 * signal into tiles of GOOFER_EQ_TILE samples and a tile into runs of GOOFER_EQ_SPT.  Only the carry from tile to tile uses the
 * coupled matrix: inside a tile, once its start state is known, the sections run one after another, each with a scan over its
 * own 2 x 2 powers (the state of section k - 1 in front of a run is the input history section k needs there).
 * Between runs and tiles the state travels as (u_k[i-1], u_k[i-1] - u_k[i-2]) per section, and every stored power is C T^m C, C
 * block diagonal with the blocks [[1, 0], [1, -1]] (its own inverse): T^m of a section with poles near z = 1 has entries of
 * about 1 / w0 that cancel against each other on a smooth state, and their float64 rounding alone costs eight bits of the
 * output; in these coordinates the entries are well scaled.
 * mats (float64): first [K][GOOFER_EQ_LEVELS][4], section k's 2 x 2 block of C T^(SPT 2^j) C, row-major; then
 * [1 + GOOFER_EQ_LEVELS][2K][2K], row-major: C T^TILE C, which carries the state over one tile, and C T^(TILE RUN_TILES 2^j) C
 * for the scan over runs of GOOFER_EQ_RUN_TILES tiles: GOOFER_EQ_MATS(K) numbers.  The powers are made by repeated squaring
 * in double-double on the host, transformed there and rounded once: squared in long double, T^4096 of a 20 Hz high-pass at
 * 192 kHz is off by 2^-35 of its largest entry.
 *
 * Tolerance: |y[i] - u_K_longdouble[i]| <= 2^-24 |u_K_longdouble[i]| + GOOFER_EQ_TOL max_i |u_K_longdouble[i]| per signal; the
 * first term is the one fp32 rounding, the second covers the carry.  Carrying a recurrence as "zero-state run plus matrix
 * times start state" is exact in exact arithmetic only: for poles near z = 1 the free response of a state is about
 * |u[i-1] - u[i-2]| / w0, hundreds of times the output, and a zero-state run is the true output minus that free response, so
 * its rounding noise is larger by the same factor; and a later band that boosts amplifies the carry noise of the bands in
 * front of it, most where those have cut the signal itself away.  The ranges above are the widest of those tried for which a
 * float64 model of the kernels' scheme (tests/eq_ref.py, `tiled`) stays within GOOFER_EQ_TOL / 4 on every corner of the range
 * (tests/eq_ref.py, `corners`, 63 chains; tests/test_eq_ref.py runs them), every band at the lowest f0, the highest q of its
 * kind and the greatest gain: one band and eight equal bands of every kind, boost and cut; chains of eight that cut and then
 * boost (notches, cutting peaks and shelves, high- and low-passes, then peaks or either shelf); chains that boost and then cut;
 * inverse pairs, the identity in exact arithmetic (four shelves or peaks one way, four the other); unequal splits (1 + 7, 2 + 6,
 * 3 + 5, 6 + 2); six seeded random chains — at 8, 44.1, 48, 96 and 192 kHz, on noise of 0.3 rms with a 40 Hz sine and a DC step
 * over 16 tiles.  Measured worst 2^-29.44 of the output's peak (one notch, then seven peaks of +9 dB, q 8, at 96 kHz; 2^-29.51
 * at 192 kHz, 2^-29.95 at 48 kHz), times 4 under GOOFER_EQ_TOL = 2^-26, a quarter of an fp32 ulp at the signal's peak; the
 * kernels themselves are at 2^-29.52 on that corner.  This is a statement about these corners and inputs, not a proof for every
 * chain of the range.  What the same rule refused, at 96 kHz: shelves of q up to 4 (four low shelves of +12 dB and four of -12
 * dB, the
 * identity: 2^-22.6; a shelf above q 2 is a resonance, and a cascade of them and their inverses is badly conditioned in
 * sequential float64 already); with the shelves at q <= 2, gains to 12 dB (two notches and six peaks: 2^-27.6; 2^-27.9 with
 * every q <= 4); gains
 * to 24 dB in every range tried from sr / 600 (2^-26.3 at q 4); and, with the state carried as (u[i-1], u[i-2]), every range
 * down to sr / 150.  Not built: a double-double carry, which would widen the range. */
#define GOOFER_EQ_MAX_BANDS 8
#define GOOFER_EQ_MIN_SR 8000
#define GOOFER_EQ_MAX_SR 192000
#define GOOFER_EQ_F_MIN_DIV 600.0    /* f0_hz * 600 >= sr: 13.3 Hz at 8 kHz, 73.5 Hz at 44.1 kHz, 80 Hz at 48 kHz, 320 Hz at 192 kHz */
#define GOOFER_EQ_F_MAX_REL 0.45
#define GOOFER_EQ_Q_MIN 0.1
#define GOOFER_EQ_Q_MAX 8.0
#define GOOFER_EQ_SHELF_Q_MAX 2.0    /* lowshelf, highshelf: above it a shelf is a resonance; cascades of those cost the tolerance */
#define GOOFER_EQ_MAX_GAIN_DB 9.0
#define GOOFER_EQ_TOL 0x1p-26
#define GOOFER_EQ_TILE GOOFER_SCAN_TILE
#define GOOFER_EQ_SPT GOOFER_SCAN_SPT
#define GOOFER_EQ_LEVELS GOOFER_SCAN_LEVELS   /* 2^8 runs in a tile; 2^8 threads in a round of the tile-to-tile carry */
#define GOOFER_EQ_RUN_TILES GOOFER_SCAN_RUN_TILES   /* tiles a thread of the tile-to-tile carry walks: 4096 tiles a round */
#define GOOFER_EQ_MATS(K) (4 * GOOFER_EQ_LEVELS * (K) + 4 * (1 + GOOFER_EQ_LEVELS) * (K) * (K))
enum { GOOFER_EQ_HIGHPASS = 0, GOOFER_EQ_LOWPASS = 1, GOOFER_EQ_LOWSHELF = 2, GOOFER_EQ_HIGHSHELF = 3, GOOFER_EQ_PEAK = 4,
       GOOFER_EQ_NOTCH = 5, GOOFER_EQ_KINDS = 6 };

/* Host side (no device, no handle): for n_bands bands (kind, f0_hz, gain_db, q: one array each) and n signals whose samples lie
 * back to back with the CSR in_off[n + 1] (non-decreasing): *K, the bands left; coef[5 K] (room for 5 GOOFER_EQ_MAX_BANDS);
 * mats[GOOFER_EQ_MATS(K)] (room for GOOFER_EQ_MATS(GOOFER_EQ_MAX_BANDS)); and the tile table: need[0] = sum_i ceil(len_i /
 * GOOFER_EQ_TILE) pairs of int32 (signal, tile of that signal), ascending.  Returns 0 with everything written; 1 when tiles_cap
 * (in pairs) < need[0] (only *K and need are valid: grow, call again); GOOFER_EINVAL for what the definition refuses, more than
 * GOOFER_EQ_MAX_BANDS bands, a null argument (in_off may be null when n == 0, tiles when tiles_cap == 0, the band arrays when
 * n_bands == 0), a negative count or capacity, offsets that decrease, a signal of 2^31 samples or more. */
int goofer_host_eq_plan(int sr, const int32_t *kind, const double *f0_hz, const double *gain_db, const double *q, int n_bands,
                        const int64_t *in_off, int n, int *K, double *coef, double *mats, int32_t *tiles, int64_t tiles_cap, int64_t *need);

/* The equaliser (eq.hip): out[in_off[i] .. in_off[i+1]) = y of signal x[in_off[i] .. in_off[i+1]), every sample stored exactly
 * once.  x, in_off ([n + 1]), coef, mats, tiles and out are device arrays of the caller, K and the tables those of
 * goofer_host_eq_plan for the same in_off, total = in_off[n].  Three launches in stream order, and no workgroup ever waits for
 * another: (A) a workgroup per tile runs the cascade over its samples from a zero state, section by section, and leaves the
 * tile's end state; (B) a workgroup per signal turns the tiles' end states, 4096 at a time, with the coupled matrices into the
 * tiles' true start states (a thread walks 16 tiles, the workgroup scans the threads); (C) every tile again from its true start
 * state, y stored once.  x is read twice and written once.
 * A tile reads the two samples in front of it from x, so `out` must not overlap x: in place is a race, and is refused.  K == 0:
 * one device-to-device copy.  Scratch by the caller-scratch protocol: with scratch NULL the size goes to *scratch_bytes and
 * nothing runs.  Asynchronous on `stream`.  n == 0 or total == 0: nothing is launched.  GOOFER_EINVAL, with nothing launched,
 * for a null pointer (all arrays may be null when n == 0 or total == 0; coef and mats when K == 0), a negative count, K outside
 * [0, GOOFER_EQ_MAX_BANDS], an n_tiles that is not between ceil(total / GOOFER_EQ_TILE) and that plus n, x, tiles or out not
 * 4-byte aligned, the others not 8-byte aligned, an out that overlaps x, or a scratch block that is too short. */
int goofer_eq(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int K, const double *coef, const double *mats,
              const int32_t *tiles, int64_t n_tiles, float *out, void *scratch, int64_t *scratch_bytes, void *stream);

/* ---- convolution reverb ---------------------------------------------------------------------------------------------------
 * Every other stage of the finishing chain acts on level, spectrum or peaks; this one gives the voice a room: every signal of a
 * ragged batch convolved with one impulse response (the IR; a tap is one of its coefficients), behind the compressor, so that the
 * tail is not pumped, and in front of the loudness stage and the limiter, so that their targets hold for what is written (mix,
 * rate conversion, equaliser, compressor, reverb, loudness, limiter, int16).  The definition is this project's own (restated in
 * numpy by tests/reverb_ref.py).  For a signal x of n samples and the IR h of L taps, shared by the batch:
 *   c[i] = sum_{k < L} h[k] x[i - pre - k]          (x is 0 outside [0, n))
 *   y[i] = dry x[i] + wet c[i]                      for 0 <= i < n_out
 *   n_out = n + (pre + L - 1 if tail else 0)        (and 0 for n == 0)
 * dry and wet are linear gains, pre is the pre-delay in whole samples, tail keeps the decay past the signal's end.  x, h and y
 * are fp32.  Signals never bleed into each other, and a signal gets the same bits alone as at any position in any batch, on every
 * run: no atomics, and every sum has one order.  Ranges, anything else refused (GOOFER_EINVAL): 1 <= L <= GOOFER_REVERB_MAX_TAPS
 * (2^18: 5.4 s at 48 kHz); 0 <= pre <= GOOFER_REVERB_MAX_PREDELAY (2^16); a sample rate that is a whole number of Hz in
 * [GOOFER_REVERB_MIN_SR, GOOFER_REVERB_MAX_SR] (the host planner's; it only converts nothing, the rate is what the settings were
 * given at); dry, wet and every tap finite; n_out < 2^31.
 *
 * Scheme: uniformly partitioned overlap-save.  The block is B = GOOFER_REVERB_BLOCK samples, the transform 2 B real points (the
 * complex B-point transform a 64-lane wave owns in csrc/fft_core.h, rectangular window, zeros outside the signal), and the IR is
 * cut into P = ceil(L / B) partitions, at most 256.  Blocks are counted from each signal's own start: block j of a signal is the
 * transform X[j] of x[(j - 1) B - pre .. (j + 1) B - pre), the pre-delay an index shift; Y[b] = sum_p X[b - p] H[p], summed over
 * p descending (b - P + 1 .. b ascending) for every block wherever it lies; the last B samples of the inverse transform of Y[b]
 * are c[b B .. (b + 1) B).  A signal has ceil(n_out / B) blocks.  A spectrum row is B complex numbers: bins 1 .. B - 1, and in
 * slot 0 the two real bins (0 and B) as one pair, multiplied element by element.  wet == 0 runs no transform: y = dry x, the
 * input's bits for dry == 1, and the tail exact zeros.
 *
 * Tolerance: |y[i] - y_float64[i]| <= GOOFER_REVERB_TOL max_i |y_float64[i]| per signal.  The constant is measured, not chosen:
 * a numpy model of the scheme in float32 / complex64 (tests/reverb_ref.py, `tiled`: the same blocks, partitions and order over
 * p) is run against the float64 restatement on the cases of tests/test_gpu_reverb.py, and the constant is four times the worst
 * max|err| / max|ref| per signal, rounded up to a power of two (tests/test_reverb_ref.py does it again on every run); the factor
 * covers the kernels' other FFT factorisation and their fused multiply-adds. */
#define GOOFER_REVERB_BLOCK 1024
#define GOOFER_REVERB_RUN 32                /* blocks of one signal per entry of the run table: one workgroup */
#define GOOFER_REVERB_MAX_TAPS 262144
#define GOOFER_REVERB_MAX_PREDELAY 65536
#define GOOFER_REVERB_MIN_SR 8000
#define GOOFER_REVERB_MAX_SR 192000
#define GOOFER_REVERB_TOL 0x1p-19
#define GOOFER_REVERB_IR_HEAD 12800         /* bytes in front of the partitions' spectra: the transform's tables and the live bytes */
#define GOOFER_REVERB_IR_BYTES(L) (GOOFER_REVERB_IR_HEAD + 8 * GOOFER_REVERB_BLOCK * (((L) + GOOFER_REVERB_BLOCK - 1) / GOOFER_REVERB_BLOCK))

/* Host side (no device, no handle): for n signals whose samples lie back to back with the CSR in_off[n + 1] (non-decreasing), an
 * IR of L taps, a pre-delay of pre samples and tail (0 / 1): out_off[n + 1], the CSR of the outputs (n_out per signal);
 * blk_off[n + 1], the CSR of the signals' blocks (ceil(n_out / GOOFER_REVERB_BLOCK) each: a signal's spectrum rows); and the run
 * table: need[0] triples of int32 (signal, first block of the run, blocks: up to GOOFER_REVERB_RUN), ascending, every block of
 * every signal in exactly one run.  Returns 0 with everything written; 1 when runs_cap (in triples) < need[0] (only need is
 * valid: grow, call again); GOOFER_EINVAL for what the definition refuses (sr, L, pre, an output of 2^31 samples or more), a null
 * argument (in_off may be null when n == 0, runs when runs_cap == 0), a negative count or capacity, offsets that decrease. */
int goofer_host_reverb_plan(int sr, const int64_t *in_off, int n, int L, int pre, int tail, int64_t *out_off, int64_t *blk_off,
                            int32_t *runs, int64_t runs_cap, int64_t *need);

/* The IR's spectra (reverb.hip), once per IR: h is a HOST array of L taps, ir a device buffer of at least
 * GOOFER_REVERB_IR_BYTES(L) bytes, 16-byte aligned, that the caller keeps and passes to every goofer_reverb with this L.  It
 * receives the transform's tables, one "live" byte per partition (0: every tap of the partition is zero; its row is exact zeros
 * and the multiply-accumulate skips it) and H[p], the transform of h[p B .. (p + 1) B) and B zeros, p < ceil(L / B).  The taps
 * are copied on `stream`, which is synchronised once (h is the caller's again on return); the transforms run asynchronously
 * behind it.  GOOFER_EINVAL for L outside [1, GOOFER_REVERB_MAX_TAPS], a tap that is not finite, a null or misaligned pointer,
 * a buffer that is too short. */
int goofer_reverb_ir(goofer_ctx *ctx, const float *h, int L, void *ir, int64_t ir_bytes, void *stream);

/* The reverb (reverb.hip): out[out_off[i] .. out_off[i+1]) = y of signal x[in_off[i] .. in_off[i+1]), every sample stored exactly
 * once, the tail included.  x, in_off, out_off, blk_off ([n + 1] each), runs and out are device arrays of the caller, the
 * tables those of goofer_host_reverb_plan for the same in_off, L, pre and tail; total = in_off[n], total_out = out_off[n],
 * total_blocks = blk_off[n]; ir: goofer_reverb_ir's buffer for the same L (not read when wet == 0).  Three launches in stream
 * order, and no workgroup ever waits for another: (A) a wave per block transforms its 2 B samples of x; (B) a workgroup per slice
 * of 64 bins stages that slice of every H[p] in LDS once and walks runs with it (256 threads and a run at a time up to 64
 * partitions, 1024 threads and four runs at a time above), a wave keeping eight output blocks' sums in registers and streaming
 * the input spectra past them once; (C) a wave per block transforms back and stores dry x + wet c.  Both spectra (8 bytes a block
 * sample each) lie in the caller's scratch, by the caller-scratch protocol: with scratch NULL the size goes to *scratch_bytes
 * and nothing runs.  Blocks read x again, so `out` must not overlap x.  Asynchronous on `stream`.  n == 0 or total_out == 0:
 * nothing is launched.  GOOFER_EINVAL, with nothing launched, for a setting outside the definition's ranges, a null pointer (all
 * arrays may be null when n == 0 or total_out == 0; ir when wet == 0), a negative count, counts that are not a geometry of the
 * planner, x, runs or out not 4-byte aligned, the others not 8-byte aligned, an out that overlaps x, or a scratch block that is
 * too short. */
int goofer_reverb(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, const void *ir, int L, int pre, int tail,
                  float dry, float wet, const int64_t *out_off, const int64_t *blk_off, int64_t total_blocks, const int32_t *runs,
                  int64_t n_runs, int64_t total_out, float *out, void *scratch, int64_t *scratch_bytes, void *stream);

/* ---- stereo bus: pan and mix tracks, channel-linked loudness and limiter ------------------------------------------------------
 * What follows a `wavtool` in every host: the mixer.  A song is several tracks (goofer_phrase_mix makes one), each with a volume
 * and a pan fader, summed onto a stereo bus which is then brought to a loudness and under a peak ceiling.  The bus is planar:
 * out[0 .. N) is L and out[N .. 2N) is R, a ragged batch of two signals of equal length with the CSR [0, N, 2N], so the stages
 * that treat every signal by itself (rate conversion, equaliser, reverb) run on it unchanged.  Two stages cannot: a limiter
 * that makes a gain per channel moves the stereo image whenever one side peaks, and BS.1770 gates a programme on the sum of its
 * channels' energies.  Those have channel-linked forms here.  The reference has no counterpart; this is the definition (restated
 * in numpy by tests/bus_ref.py).  All fp32 arithmetic is uncontracted.
 *
 * Pan law (host, float64, stored as fp32): constant power.  g = 10^(gain_db / 20), gain_db finite in [-144, 24]; pan in [-1, 1]
 * (-1 left, 1 right), theta = (pan + 1) pi / 4; gl = fp32(g cos theta), gr = fp32(g sin theta).  Three positions are exact:
 * pan == -1 has gr = +0.0f, pan == 1 has gl = +0.0f, and pan == 0 has gl = gr = fp32(g sqrt(0.5)) (in float64 cos(pi/4) and
 * sin(pi/4) differ in the last place).  A muted track is not in the table at all.
 *
 * Mix.  Track i has a record: x, a device pointer to its len samples (tracks need not lie back to back), len >= 0, start >= 0 its
 * position on the bus, and the finite gains gl, gr.  For t in [0, total_out):
 *   L[t] = sum_i gl_i * x_i[t - start_i]  over the tracks with 0 <= t - start_i < len_i,   R[t] likewise with gr_i
 * in ascending i from +0.0f, each term one rounded multiply, then one rounded add.  out[t] = L[t], out[total_out + t] = R[t];
 * every sample of both channels is stored exactly once, zeros where no track sounds; what lies past total_out is dropped. */
#define GOOFER_BUS_TILE GOOFER_MIX_TILE
typedef struct {
    const float *x;             /* device pointer */
    int64_t len;                /* >= 0 */
    int64_t start;              /* >= 0 */
    float gl, gr;               /* finite */
} goofer_bus_track;

/* Host side (no device, no handle; x is not read): check the n records and write the cover table of the bus's tiles of
 * GOOFER_BUS_TILE samples, tiles = ceil(total_out / GOOFER_BUS_TILE): tile_off[tiles + 1] (CSR) and tile_tracks, the tracks whose
 * range [start, min(start + len, total_out)) meets the tile, in ascending track index (a track with an empty range is in no
 * tile).  *need = entries of tile_tracks.  Returns 0 with both arrays written; 1 when cap < *need (only *need is valid: grow,
 * call again); GOOFER_EINVAL for a null argument (tracks may be null when n == 0, tile_tracks when cap == 0), a negative count,
 * length or start, a gain that is not finite, an x that is null where len > 0 or not 4-byte aligned (the pointer's value alone),
 * or a bus of 2^31 tiles or more. */
int goofer_host_bus_plan(const goofer_bus_track *tracks, int n, int64_t total_out, int64_t *tile_off, int32_t *tile_tracks, int64_t cap,
                         int64_t *need);

/* The bus (bus.hip): out[0 .. 2 total_out), planar, every sample stored exactly once, so `out` needs no clearing.  tracks ([n],
 * as validated by goofer_host_bus_plan), tile_off and tile_tracks (that call's table for the same records and total_out) and out
 * are device arrays of the caller; `out` must not overlap any track.  One workgroup per tile, eight consecutive samples of both
 * channels per thread in registers, every source sample loaded once; no atomics, no LDS, no scratch; 16-byte loads where a
 * wave's source is 16-byte aligned and 16-byte stores for a channel whose base is (R is not when total_out % 4 != 0).  It moves
 * 4 sum_i len_i + 8 total_out bytes.  Asynchronous on `stream`; needs no plan.  total_out == 0: nothing is launched; n == 0:
 * zeros.  GOOFER_EINVAL, with nothing written, for a null pointer (tracks and tile_tracks may be null when n == 0), a negative
 * count, out or tile_tracks not 4-byte aligned, tracks or tile_off not 8-byte aligned, a bus of 2^31 tiles or more. */
int goofer_bus_mix(goofer_ctx *ctx, const goofer_bus_track *tracks, int n, const int64_t *tile_off, const int32_t *tile_tracks,
                   int64_t total_out, float *out, void *stream);

/* The channel-linked limiter (limit.hip).  ch is 1 or 2 and n % ch == 0: signals g ch .. g ch + ch - 1 of the ragged batch are the
 * channels of group g and have equal lengths.  The definition is goofer_limit's with step 1 replaced by
 *   1  a[i] = max_c |x_c[i]|        (fmaxf: a NaN operand is ignored)
 * and with R = 2 or 4 and tp_taps (goofer_host_true_peak_plan's; Z = GOOFER_TP_ZEROS) by a[i] = max_c e_c[i], e_c the envelope of
 * the true-peak section; R == 0 is sample-peak detection and tp_taps is not read.  Steps 2 to 7 run once per group, word for
 * word, and step 8 is y_c[i] = x_c[i] * g[i] for every channel: both channels get the same gain, so the image does not move.
 * peak_in and min_gain are fp32 [n / ch], one pair per group.  `tiles` / n_tiles are goofer_host_limit_plan's for the groups' CSR
 * (the group lengths; the planner is the same): one workgroup per (group, tile), and the LDS need does not grow with ch.
 * Properties: ch == 1 gives the bits of goofer_limit (R == 0) or goofer_limit_tp; a pair (x, x) returns goofer_limit's output in
 * both channels; a group that never exceeds c comes back bit for bit; |y_c| <= c (1 + 2^-24)^2, because g <= fl(c / a) and
 * a >= |x_c|.  Whether a tile copies its samples (options "limit_skip", "limit_tp_skip") is decided over all channels of the
 * group: the quiet channel beside a peak in the other one is reduced like it.  A group whose signals differ in length is neither
 * read nor written (a table that is not the planner's).  GOOFER_EINVAL for ch outside {1, 2}, n % ch != 0, R not 0, 2 or 4, an
 * n_tiles that is not a tile count of n / ch signals with total / ch samples, and everything goofer_limit and goofer_limit_tp
 * refuse. */
int goofer_limit_linked(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, int ch, int W, const float *taps,
                        float c, const int32_t *tiles, int64_t n_tiles, float *out, float *peak_in, float *min_gain, int R,
                        const float *tp_taps, void *stream);

/* The channel-linked loudness gate (loudness.hip), behind a measure-only goofer_loudness_measure (target NaN) of the n channel
 * signals on the same stream: seg_energy and seg_off ([n + 1]) are that call's.  ch is 1 or 2 and n % ch == 0.  For group g,
 * E_g[k] = sum_c E_c[k] in ascending channel from channel 0 (BS.1770's channel weight 1.0 for L and R); blocks, both gates, L,
 * momentary_max and the gain follow the loudness section as written for one channel, on E_g.  loud: float64 [n / ch][2]; gain:
 * fp32 [n], the group's value in each of its channels, so goofer_loudness_apply runs unchanged.  One workgroup per group, the
 * gating code goofer_loudness_measure's own.  A group whose channels differ in segment count gets NaN, NaN and a gain of 1.0f;
 * a NaN energy makes its group NaN as in the definition and leaves the others alone.  target NaN: measure only.  Asynchronous
 * on `stream`; no scratch, no plan; n == 0: nothing is launched.  GOOFER_EINVAL for ch outside {1, 2}, n % ch != 0, a null
 * pointer, a negative count, S, target or max_gain_db outside the definition's range, gain not 4-byte aligned, the others not
 * 8-byte aligned. */
int goofer_loudness_link(goofer_ctx *ctx, const double *seg_energy, const int64_t *seg_off, int n, int ch, int S, double target,
                         double max_gain_db, double *loud, float *gain, void *stream);

/* goofer_pcm16 of a planar signal of ch channels of n samples, interleaved for a wav: out[i ch + c] = pcm16(x[c n + i]), the same
 * arithmetic.  ch is 1 or 2; ch == 1 gives goofer_pcm16's bits.  Asynchronous on `stream`; n <= 0: nothing is launched. */
int goofer_pcm16_planar(goofer_ctx *ctx, const float *x, int64_t n, int ch, int16_t *out, void *stream);

/* ---- measurement / test hooks --------------------------------------------------------------- */

/* HIP-event timing of every stage of goofer_synth_batch on the caller's stream: begin() arms up to
 * max_steps batches, end() synchronises and writes the summed milliseconds of each stage
 * (goofer_profile_stage_name(i), i < 18); returns the number of batches recorded.  Stages 15..17 are the assembly's three
 * large kernels ("env_edit", "env_rows", "sample_assemble"), each bracketed on the stream it runs on. */
int goofer_profile_begin(goofer_ctx *ctx, int max_steps);
int goofer_profile_end(goofer_ctx *ctx, double *ms_per_stage, int n_stages);
const char *goofer_profile_stage_name(int stage);
const char *goofer_profile_stage_name_ex(const goofer_ctx *ctx, int stage);   /* names of the path the last profiled batch took */

/* Options (each is an A/B reference a parity test needs; every setting but td_blur and value_f64 produces the same stems):
 *   "fused_ola" 1 (default): irFFT of the three stems + overlap-add + gains in one kernel; 0: separate kernels
 *   "overlap"   1 (default): pulse chain on the handle's side stream beside the aperiodic branch; 0: one stream
 *   "stems"     1 (default): stem-split walker kernels where the geometry allows (hop == n_fft / 4); 0: one kernel per
 *               reference step up to the spectra, then the fused overlap-add
 *   "skip_zero" 1 (default): a noise-stem transform whose stem gain is exactly zero over every sample it reaches is skipped
 *               (the walkers decide per hop; the n_fft 2048 pipeline per frame up front); 0: every frame runs every transform
 *   "td_blur"   1 (default): the stem walkers fold the voiced frames' 5-tap bin blur into the synthesis window (agrees with
 *               0, the blur over the bins, to fp32 rounding — the only option that is not bit-identical)
 *   "pulse_scan" 1 (default): pulse onsets from a parallel fp64 phase scan wherever its rounding band provably cannot move
 *               floor(phase), the sequential walk only for the remaining notes; 0: the sequential walk for every note;
 *               2: the scan kernel walks every note (tests the hand-over)
 *   "pulse_fused" 1 (default): with "pulse_scan" != 0 the pulse train is one kernel, a workgroup per note: scan, periods and
 *               placement per round of 2048 samples, the onsets in an LDS ring (k_pulse_note); 0: the chain of four kernels
 *               (scan, onset records, tile table, placement).  A/B, the same bits
 *   "value_f64" 0 (default): k_env_edit's VALUE arithmetic (fw interpolation, es blur, knot exp) in fp32 — everything that
 *               decides an index, a threshold or the pitch curve stays fp64; 1: round 4's fp64
 *               arithmetic there (agrees to 2e-8 sample-RMS on the 1024-note batch; not bit-identical)
 *   "sa_fast"   1 (default): k_sample_assemble's branch-free path with all of a thread's loads in flight together; 0: per sample
 *   "sa_table"  1 (default): k_sample_assemble reads the notes of its 1024-sample tile from a table a small kernel ahead of it
 *               writes without a search; 0: every workgroup searches the note plans.  Same bits.
 *   "mask_flags" 1 (default): goofer_render_batch has k_sample_assemble leave a word per 1024 samples of the voicing mask (all == 0,
 *               all == 1, neither) and k_mask_short answer the windows those words settle without loading the mask; 0: no flags
 *               (goofer_assemble_batch / goofer_synth_batch on their own and goofer_smooth_mask_ds never have them).  Same bits.
 *   "mask_sparse" 1 (default): where goofer_render_batch writes those words, takes the stem walkers, renders mix_only and runs no
 *               layer that reads the mask sample by sample (f0 / volume jitter, sub-harmonics), k_sample_assemble does not store
 *               the 256 mask values of a wave that are all 0.0f or all 1.0f: the frame picks and k_mask_short take them from the
 *               wave's byte.  `mask` is scratch in such a call, like the stems.  0: the mask is always written in full.  Same bits.
 *   "legacy_wave" 0 (default): goofer_legacy_normal_fill / _jobs give a job a workgroup of 256 threads; 1: one wave.  Same bits.
 *   "rate_lds"  1 (default): goofer_rate_convert stages the tap table in LDS where it fits in 160 KiB; 0: every lane reads its
 *               row from global memory, as it does for a table that does not fit.  Same bits.
 *   "limit_skip" 1 (default): a tile of goofer_limit with no sample above the ceiling, its halo of 2W samples on either side
 *               included, copies x to out; 0: every tile does the full arithmetic.  Same bits (the identity property).
 *   "limit_tp_skip" 1 (default): a tile of goofer_limit_tp whose true-peak envelope never exceeds the ceiling, its halo of 2W
 *               samples on either side included, copies x to out behind the interpolation; 0: every tile does the full
 *               arithmetic.  Same bits (the identity property).
 *   "compress_skip" 1 (default): goofer_compress finds a sample under the lower end of the knee (|x| <= 10^((T - W/2) / 20)) by
 *               one compare and takes xl = 0 without the logarithm; 0: the logarithm for every sample.  The curve is continuous
 *               there, so the two agree within rounding (and bit for bit wherever the identity property holds).
 *   "compress_store" 0 (default): every pass of goofer_compress computes xl again from x; 1: the first pass writes xl (float64
 *               [total], more scratch: ask for the size with the option set) and the other two read it.  Same bits.
 *   "reverb_skip" 1 (default): goofer_reverb's multiply-accumulate leaves out a partition of the impulse response whose taps are
 *               all zero (its "live" byte); 0: every partition is multiplied.  Same bits on finite input.
 *   "walk_run"  0 (default): the four frame walkers (k_noise_stems, k_harm_stem, k_irfft_ola3, k_irfft_ola1) get the frames per
 *               wave that fill the device a whole number of times: from a floor of 32 frames (8 halos where the halo
 *               (n_fft - 1) / hop is above 4) to 128, k_irfft_ola1 256; a batch leaves the floor only with tens of thousands of
 *               frames.  N > 0: N frames per wave, clamped per kernel to that same range [floor, max(cap, floor)] — the runs of
 *               a full-size batch on a small one, never a run no batch could get.  Same bits (the overlap-add runs in ascending
 *               frame order however the frames are cut into runs).  Read back with goofer_counter "walk_run_*".
 *   "prof_only" s >= 0: goofer_profile_begin .. end record the events of stage s only; -1 (default): every stage     */
int goofer_set_option(goofer_ctx *ctx, const char *name, int value);

/* Copy a plan table (0 window, 1 freqs, 2 boost, 3 bright_harm, 4 bright_breath, 5 pulse peak) or an
 * intermediate of the last synth batch to HOST memory; return element count / byte size. Tests only. */
int goofer_debug_table(goofer_ctx *ctx, int which, float *host_out, int capacity);
/* sizeof of the ABI structs (0 note_params, 1 batch, 2 note_plan, 3 assembly, 4 onepole_job, 5 post_note, 6 post,
 * 7 plan_request, 8 plan_geometry, 9 legacy_job, 10 track_settings, 11 phrase_note) so bindings can verify layout */
int goofer_sizeof(int which);
int64_t goofer_debug_fetch(goofer_ctx *ctx, int which, void *host_out, int64_t capacity_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOOFER_HIP_H */
