// Internal declarations shared by the HIP translation units of libgoofer_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/goofer_hip.h"

#define WAVE 64
#define PROF_STAGES 18
#define PROF_ASM0 15           // profile stages 15..17: the assembly's k_env_edit, k_env_rows, k_sample_assemble
#define SA_TILE 1024            // k_sample_assemble<4>: samples per workgroup (256 threads x 4), and per tile-flag word (render_link::tile_flags)
#define MASK_COUNTERS 32        // goofer_ctx::ovf_flag + MASK_COUNTERS: k_mask_short's two counters (segments answered from tile flags, segments staged),
#define MASK_COUNTER_SLOTS 64   // each spread over this many words a cache line apart (slot = workgroup & 63): thirteen thousand atomics on
#define MASK_COUNTER_STRIDE 32  // ONE word took longer than the kernel; counter c, slot s: word MASK_COUNTERS + (2 * s + c) * MASK_COUNTER_STRIDE
#define LEGACY_FLAG 3           // goofer_ctx::ovf_flag[LEGACY_FLAG]: sticky like [0]: 1 + index of a note whose legacy normal fill ran into its block bound
#define PULSE_LIST_COUNTER 4    // goofer_ctx::ovf_flag[PULSE_LIST_COUNTER]: cumulative like [1], [2]: notes k_pulse_note placed from the onset list (goofer_counter "pulse_list_notes")
#define OVF_WORDS (MASK_COUNTERS + 2 * MASK_COUNTER_SLOTS * MASK_COUNTER_STRIDE)
#define PP_SPT 8                // k_pulse_place: consecutive samples per thread; a tile = one workgroup = 256 * PP_SPT samples
#define PULSE_TILE_INTS(samples) (4 * (((samples) + 256 * PP_SPT - 1) / (256 * PP_SPT)) + 64)   // k_pulse_tiles' table: 4 ints per tile
// compress_env_to_knots' candidate knot counts (GOOFER.py:97-147): K = KN_K0, KN_K0 + KN_DK, ..., KN_KMAX
#define KN_K0 32
#define KN_DK 16
#define KN_KMAX 192
#define KN_CAND ((KN_KMAX - KN_K0) / KN_DK + 1)
#define KN_BINS_TOTAL (KN_CAND * KN_K0 + KN_DK * KN_CAND * (KN_CAND - 1) / 2)   // knots of all candidates back to back (1232)
#define PULSE_TAB_MAX 8192     // pulse lengths served from the shape table: all of them (the reference caps T0 at 8192, GOOFER.py:497-498) — 134 MB of
                               // a 288 GB device; until late in round 5 the table ended at 2048 and k_pulse_place evaluated longer pulses on the fly, whose
                               // fp64 sin / exp / cos set the kernel's registers (115, four waves per SIMD) though no note of the workloads reached them

// the LF glottal-pulse model of gf.pulse_train_numba (GOOFER.py:474, 508): its keyword arguments, defaults = what gf.synthesize passes
struct lf_model {
    double ra = 0.02, rg = 1.7, rk = 0.8;
};
#define PULSE_PEAK_FLOATS (8193 + 1 + 6)   // k_pulse_peak's table + the model's three doubles behind it (8-byte aligned; goofer_debug_table, tests)

struct goofer_plan_t {
    int sr = 0, n_fft = 0, hop = 0, n_bins = 0;
    float *window = nullptr;      // [n_fft] sqrt-Hann, fp32                      GOOFER.py:12-18
    float *window_blur = nullptr; // [n_fft] window x the time-domain image of the sigma-0.5 bin blur (see stems.hip)
    float *blur_edge = nullptr;   // [4][64] per-lane coefficients of the blur's edge correction (bins 1..6 and M-6..M-1)
    float *win_sq = nullptr;      // [n_fft] window*window in fp32 (OLA weights)  GOOFER.py:385
    float *freqs = nullptr;       // [n_bins] rfftfreq fp32                       GOOFER.py:20-26
    float *lin_freqs = nullptr;   // [n_bins] np.linspace(0, sr/2, n_bins) rounded to fp32 (the bells' bin frequencies, SillySampler.py:812)
    float *boost = nullptr;       // [n_bins] linspace(1,100)                     GOOFER.py:28-35
    float *bright_h = nullptr;    // [n_bins] harmonic brightness                 GOOFER.py:42
    float *bright_b = nullptr;    // [n_bins] breath brightness                   GOOFER.py:43
    float2 *tw_full = nullptr;    // [n_fft/2]   exp(-2 pi i k / (n_fft/2))
    float2 *tw_half = nullptr;    // [n_fft/4+1] exp(-2 pi i k / n_fft)
    // transform sizes without a native radix plan (any other even n_fft in [64, 4096] but 2050): Bluestein's chirp-z
    // transform of the n_fft/2-point complex DFT through power-of-two transforms of length bl_L >= n_fft - 1 (fft.hip)
    int bl_L = 0;                 // 0: native
    float2 *bl_chirp = nullptr;   // [M]     exp(+i pi n^2 / M)
    float2 *bl_bhat = nullptr;    // [bl_L]  FFT of the wrapped chirp
    float2 *bl_tw = nullptr;      // [bl_L]  exp(-2 pi i k / bl_L)
    float2 *bl_twh = nullptr;     // [M + 1] exp(-i pi k / M)
    lf_model lf;                  // goofer_pulse_model
    float *pulse_peak = nullptr;  // [PULSE_PEAK_FLOATS] peak of the un-normalised LF shape per T0 (fp64 math), then the model's Ra, Rg, Rk
    float *pulse_shape = nullptr; // normalised LF pulses for T0 = 3..PULSE_TAB_MAX back to back (row T0 at T0(T0-1)/2 - 3)
    double *blur5 = nullptr;      // [5] sigma=0.5 taps (brightness blur)         GOOFER.py:1143
    double *blur175 = nullptr;    // [15] sigma=1.75 taps                         GOOFER.py:993
    float taps5_f[5] = {0}, taps175_f[15] = {0};   // the same taps rounded to fp32, host side (passed to kernels by value)
};

// HIP events of a profiled run (goofer_profile_begin): `per_step` for each step the pool was grown to
struct event_pool {
    int per_step;
    hipEvent_t *ev = nullptr;     // null until the first goofer_profile_begin
    int steps = 0;
    hipEvent_t *step(int k) const { return ev + (size_t)k * per_step; }
};

// What one goofer_render_batch hands from its assembly half to its synthesis half (synth.hip).  It lives on that call's stack;
// goofer_assemble_batch and goofer_synth_batch pass an empty one.
struct render_link {
    // asked of the assembly
    bool fork_early = false;              // ev_entry is recorded: record ev_f0 behind the f0 / mask kernel, so that the pulse chain may fork there
    float *warp_dst = nullptr;            // the frame-gather kernel also writes the rows the harmonic walker needs (formant-anchored +
    const double *formants = nullptr;     // uniform warp) here, from these formants and note parameters
    const goofer_note_params *params = nullptr;
    bool want_tile_flags = false;         // carve tile_flags_dst (assemble_batch), where the f0 / mask kernel also leaves a word per SA_TILE samples
    unsigned char *tile_flags_dst = nullptr;   // of the mask it writes: four bytes, one per wave, bit 0: some value is not == 0.0f, bit 1: some value
                                          // is not == 1.0f (word & 0x01010101 == 0: the tile is all zeros, & 0x02020202 == 0: all ones)
    bool mask_sparse = false;             // the f0 / mask kernel may leave the mask values of a wave unwritten where one byte says them all (MASK_UNSTORED):
                                          // decided by goofer_render_batch from synth_route::sparse_ok, cleared by the assembly when it writes no flags; the
                                          // synthesis then reads the mask through mask_value() only
    // answered by the assembly
    const float *f0_ready = nullptr;      // the f0 array ev_f0 stands for (null: no event recorded)
    bool f0_side = false;                 // the f0 / mask kernel ran on the side stream, in front of the pulse chain it feeds: the caller's
                                          // stream waits for ev_f0 before it reads f0 / mask (cleared by whoever places that wait)
    bool warped = false;                  // warp_dst holds the warped rows of the batch
    const unsigned char *tile_flags = nullptr;   // the tile flags of the mask as the f0 / mask kernel wrote it (ready where f0 / mask are), for
                                          // k_mask_short; null: none were written
};

// The tile-flag byte of sample g of the concatenated axis: k_sample_assemble<4> gives wave w of the workgroup of tile g / SA_TILE the
// four 64-sample strips at 64 w + 256 u of the tile, and its byte is the w-th of the tile's word.  The kernel's own store of the
// byte is this map for the samples of thread threadIdx.x of workgroup blockIdx.x, written out there as 4 * blockIdx.x +
// (threadIdx.x >> 6): through this function the same instructions came out in another order, and the instantiations from before
// the sparse mask are kept instruction for instruction.
__host__ __device__ __forceinline__ int64_t mask_flag_index(int64_t g) { return 4 * (g / SA_TILE) + (((g % SA_TILE) & 255) >> 6); }
// bit 2 of a flag byte (render_link::mask_sparse only): the wave's 256 values are all 0.0f or all 1.0f to the bit and were NOT stored;
// bit 0 then says which.  (The two words k_mask_short masks the bytes with do not see the bit.)
#define MASK_UNSTORED 4u
// mask[g] where the mask may be sparse (`sparse_flags`: render_link::tile_flags under mask_sparse, else null).  Both loads go out
// together — the array is allocated whether or not the wave stored, and what an unstored place holds is discarded.
__device__ __forceinline__ float mask_value(const float *__restrict__ mask, const unsigned char *__restrict__ sparse_flags, int64_t g)
{
    const float v = mask[g];
    if (!sparse_flags) return v;
    const unsigned f = sparse_flags[mask_flag_index(g)];
    return (f & MASK_UNSTORED) ? ((f & 1u) ? 1.0f : 0.0f) : v;
}

struct goofer_ctx {
    int device = 0;
    char err[512] = {0};
    goofer_plan_t plan;
    goofer_track_settings track = GOOFER_TRACK_SETTINGS_DEFAULT;   // goofer_track_configure
    // handle-owned device blocks, each grown by grow_block
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    void *asm_scratch = nullptr;  // assembly scratch: edited rows + row->note maps
    size_t asm_bytes = 0;
    void *small = nullptr;        // small staging buffer for taps etc. (its regions: SMALL_* below)
    size_t small_bytes = 0;
    // device pointers of the last synth batch's intermediates (goofer_debug_fetch; tests only)
    const void *dbg_ptr[17] = {nullptr};
    size_t dbg_bytes[17] = {0};
    bool overlap = true;          // noise spectra + mask smoothing on a side stream, beside the latency-bound pulse walk
    hipStream_t side = nullptr;   // created on first use
                                  // ... with the highest stream priority (measured: 2.41 ms per step against 2.50 at the default, 2.54 at the lowest)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_maps = nullptr;
    // goofer_render_batch: the pulse chain forks as soon as the assembled f0 exists, not when the synthesis call starts
    hipEvent_t ev_entry = nullptr, ev_f0 = nullptr, ev_f0s = nullptr;
    int32_t *ovf_flag = nullptr;           // handle-owned device words (OVF_WORDS of them; [1], [2] and from MASK_COUNTERS on: cumulative counters, goofer_counter); [0] sticky between goofer_check calls: 1 + index (inside its batch) of a
                                           // note whose pulse onsets overflowed their slots, written with atomicMax by every pulse-chain launch
    // goofer_render_batch, stem-split path: the buffer the assembly's frame-gather kernel writes the harmonic walker's warped rows
    // to (render_link::warp_dst)
    float *warp_rows = nullptr;
    size_t warp_rows_bytes = 0;
    event_pool prof_side{4};            // boundaries of the pulse chain on the side stream
    event_pool prof_main2{2};           // ends of noise_spectra / mask_short when they run beside it
    event_pool prof_asm{6};             // [3][2]: the assembly's three large kernels, each on its own stream
    unsigned char prof_asm_mask[4096] = {0};   // which of the three pairs assembly k of the profiled run recorded
    int prof_asm_steps = 0;
    bool prof_side_used = false;
    bool ola_fused = true;        // irFFT x3 + overlap-add + gains in one kernel (k_irfft_ola3); false: separate irFFT launches + k_ola3_gains
    bool stems = true;            // stem-split frame walkers (stems.hip) where the geometry allows (hop == n_fft / 4); false: the
                                  // one-kernel-per-reference-step pipeline with the spectra in HBM (A/B parity path)
    bool skip_zero = true;        // noise walker: skip transforms whose stem gain is exactly zero over everything they reach (option "skip_zero")
    bool td_blur = true;          // stem walkers: the 5-tap bin blur of voiced frames as a window on the frame's samples (option "td_blur")
    bool prof_stems = false;      // the last profiled batch ran the stem-split path (stage order differs)
    bool mask_flags = true;       // goofer_render_batch: k_sample_assemble leaves tile flags of the mask and k_mask_short answers flat windows from
                                  // them without loading the mask (option "mask_flags"; 0: A/B, the same bits)
    bool mask_sparse = true;      // goofer_render_batch, walker route, mix_only: k_sample_assemble does not store the mask values of a wave that are all 0.0f or
                                  // all 1.0f, and the picks / k_mask_short take them from the wave's flag byte (option "mask_sparse"; 0: A/B, the same bits)
    bool sa_fast = true;          // k_sample_assemble: the branch-free path with all of a thread's loads in flight together (option "sa_fast"; 0: A/B)
    bool sa_table = true;         // k_sample_assemble reads the notes of its tile from k_sample_tile_notes' table instead of searching the plans
                                  // (option "sa_table"; 0: A/B, the same bits)
    bool value_f64 = false;       // k_env_edit: round 4's fp64 value arithmetic (fw interpolation, es blur) instead of fp32 — A/B and the
                                  // error-budget tests (option "value_f64")
    bool legacy_wave = false;     // k_legacy_normal_fill: one wave per note instead of one 256-thread workgroup (option "legacy_wave"; A/B, the same bits)
    bool rate_lds = true;         // goofer_rate_convert: the tap table staged in LDS where it fits (option "rate_lds"; 0: read from global memory, A/B, the same bits)
    bool limit_skip = true;       // goofer_limit: a tile with nothing above the ceiling, halo included, copies its samples (option "limit_skip"; 0: the full arithmetic for every tile, A/B, the same bits)
    bool limit_tp_skip = true;    // goofer_limit_tp: a tile whose true-peak envelope never exceeds the ceiling, halo included, copies its samples (option "limit_tp_skip"; 0: the full arithmetic for every tile, A/B, the same bits)
    bool compress_skip = true;    // goofer_compress: a sample under the knee's lower end is found by one compare and its logarithm is not taken (option "compress_skip"; 0: A/B, equal within rounding)
    bool compress_store = false;  // goofer_compress: xl is written to scratch by the first pass and read back by the other two instead of being computed again (option "compress_store"; A/B, the same bits)
    bool reverb_skip = true;      // goofer_reverb: the multiply-accumulate leaves out a partition of the impulse response whose taps are all zero (option "reverb_skip"; 0: A/B, the same bits)
    int walk_run = 0;             // frames per wave of the four frame walkers (option "walk_run"; 0: chosen from the device, N > 0: N clamped to the
                                  // range that choice can produce for the kernel: walk_run_choice, launchers.h; tests, the same bits)
    int walk_run_used[4] = {0, 0, 0, 0};   // the run the last launch of k_noise_stems / k_harm_stem / k_irfft_ola3 / k_irfft_ola1 got (goofer_counter "walk_run_*")
    int pulse_scan = 1;           // 1: onsets from the parallel phase scan, the sequential walk only for the notes it cannot settle;
                                  // 0: the sequential walk kernel for every note; 2: the scan kernel walks every note (tests)
    bool pulse_fused = true;      // with pulse_scan != 0: scan, periods and placement in one kernel, a workgroup per note (k_pulse_note; option
                                  // "pulse_fused"); 0: k_pulse_onsets_par, k_onset_finish, k_pulse_tiles, k_pulse_place (A/B, the same bits)
    // per-context kernel state: hipFuncSetAttribute is per device, and a handle belongs to one device, so what was set /
    // queried is remembered here and never in process-wide statics
    struct kernel_state {
        const void *fn;
        size_t lds;               // dynamic LDS the occupancy below was queried for
        int waves;                // waves of this kernel the device holds at once (0: not queried)
        bool max_lds_set;
    } kstate[32] = {};
    int n_kstate = 0;
    // per-stage HIP-event timing of goofer_synth_batch (goofer_profile_begin/end)
    bool prof_on = false;
    int prof_only = -1;           // >= 0: goofer_profile_begin .. end bracket this stage only (option "prof_only")
    int prof_steps = 0, prof_cap = 0;
    event_pool prof_ev{PROF_STAGES + 1};   // stage s of a step runs from event s to event s + 1
    double *mask_taps = nullptr;  // device taps of the voicing-mask smoother, cached per sigma
    size_t mask_taps_bytes = 0;
    float mask_taps_sigma = -1.f;
    int mask_taps_radius = 0;
    double mask_taps_sum = 0.0;   // running fp64 sum of the taps in tap order (the FIR's answer on a window of ones)
};

int goofer_fail(goofer_ctx *ctx, int code, const char *fmt, ...);
#define NEED_PLAN(ctx)                                                                    \
    if (!(ctx)) return GOOFER_EINVAL;                                                     \
    if (!(ctx)->plan.n_fft) return goofer_fail((ctx), GOOFER_ENOPLAN, "goofer_plan first")
// float2 slots per row of a [frames x bins] complex spectrum matrix: n_bins rounded up to 16 (128-byte aligned rows, so that
// the framewise rFFT's 16-byte stores and every row-wise reader start on a cache-line boundary)
static inline int spec_stride(int n_bins) { return (n_bins + 15) & ~15; }
// opt a kernel in to the full 160 KiB of dynamic LDS on this handle's device (once per handle)
int kernel_allow_max_lds(goofer_ctx *ctx, const void *fn, int bytes = 160 * 1024);
// waves of `fn` (256-thread workgroups, `lds` bytes of dynamic LDS) resident on this handle's device at once
int kernel_resident_waves(goofer_ctx *ctx, const void *fn, size_t lds, int *waves);

#define HIP_TRY(ctx, call)                                                                       \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return goofer_fail((ctx), GOOFER_EHIP, "%s failed: %s (%s:%d)", #call,               \
                               hipGetErrorString(e_), __FILE__, __LINE__);                       \
    } while (0)

#define LAUNCH_CHECK(ctx)                                                                        \
    do {                                                                                         \
        hipError_t e_ = hipGetLastError();                                                       \
        if (e_ != hipSuccess)                                                                    \
            return goofer_fail((ctx), GOOFER_EHIP, "kernel launch failed: %s (%s:%d)",           \
                               hipGetErrorString(e_), __FILE__, __LINE__);                       \
    } while (0)

// ---- scratch layouts -----------------------------------------------------------------------

// scratch arena: 256-byte aligned pieces taken in order.  Without a base it only counts, so the code that carves a call's
// buffers also sizes them.
struct arena {
    char *base;
    size_t used;
    template <typename T> T *take(size_t count)
    {
        T *p = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

// The caller-scratch protocol of include/goofer_hip.h: carve(arena &) runs once counting.  With scratch NULL the count goes to
// *scratch_bytes and nothing else happens (GOOFER_OK: the caller returns, as `scratch` tells it); otherwise a block shorter
// than the count is refused and carve runs again over the caller's block.
template <typename Carve>
int caller_scratch(goofer_ctx *ctx, void *scratch, int64_t *scratch_bytes, const char *what, Carve &&carve)
{
    arena a{nullptr, 0};
    carve(a);
    if (!scratch) {
        *scratch_bytes = (int64_t)a.used;
        return GOOFER_OK;
    }
    if (*scratch_bytes < (int64_t)a.used)
        return goofer_fail(ctx, GOOFER_EINVAL, "%s: scratch of %lld bytes, %zu needed", what, (long long)*scratch_bytes, a.used);
    a = arena{(char *)scratch, 0};
    carve(a);
    return GOOFER_OK;
}

// grow a handle-owned device block (*p, *bytes) to `need` bytes (api.hip)
int grow_block(goofer_ctx *ctx, void **p, size_t *bytes, size_t need, const char *what);

// carve(arena &) once counting, grow a handle block to what it took (+ 4 KiB behind the last piece), then carve once over it
template <typename Carve> int carve_block(goofer_ctx *ctx, void **block, size_t *bytes, const char *what, Carve &&carve)
{
    arena count{nullptr, 0};
    carve(count);
    if (int rc = grow_block(ctx, block, bytes, count.used + 4096, what)) return rc;
    arena a{(char *)*block, 0};
    carve(a);
    return GOOFER_OK;
}
template <typename Carve> int carve_scratch(goofer_ctx *ctx, Carve &&carve)
{
    return carve_block(ctx, &ctx->scratch, &ctx->scratch_bytes, "scratch", carve);
}

// The handle's small block (ctx->small): host tables a call uploads for its own kernels.  Its regions, by byte offset:
constexpr size_t SMALL_TABLES = 0;       // [0, 32 KiB): taps of goofer_gauss_bins / _gauss_bins_f64; the lerp tables of
                                         // goofer_knot_decode / _knot_fit_error (12 bytes per bin)
constexpr size_t SMALL_WORDS = 32768;    // [32 KiB, 64 KiB): goofer_warp_bins' f_shift (4 doubles), goofer_knot_fit_error's error word
constexpr size_t SMALL_FIXED = 65536;    // tables and words: what their users grow the block to at least
constexpr size_t SMALL_JIT = 65536;      // three jitter tap slots of JIT_SLOT_BYTES (upload_jitter_taps)
constexpr size_t JIT_SLOT_BYTES = 131072;
constexpr size_t SMALL_RAGGED = SMALL_JIT + 3 * JIT_SLOT_BYTES;   // goofer_gauss_rows_f64's taps, any radius
// Overlaps: goofer_gauss_bins / _gauss_bins_f64 accept radius 4096, 65 544 bytes of taps from byte 0: through the words and
// 8 bytes into jitter slot 0.  goofer_smooth_mask_ds uses [0, its size) as one piece (taps, decimated mask, per-note steps),
// across every region.  Each use is in stream order, which is what keeps the overlaps harmless.

// host helpers of api.hip that synth.hip and post.hip use as well: normalised taps of a Gaussian of radius int(4 sigma + 0.5), fp64
void gauss_taps_host(double sigma, std::vector<double> &taps, int &radius);
// taps of a sample-axis Gaussian, uploaded into jitter slot `slot` of the small block (api.hip)
int upload_jitter_taps(goofer_ctx *ctx, double sigma, int slot, const double **d_taps, int *radius, hipStream_t st);

static const size_t ONSET_BYTES = 24;    // bytes per onset slot (onset_t, pulse.hip)
// Onset slots (the onset index list and the onset_t list share the layout): n / 2 + 16 per note for the pulse train (an f0 above
// sr / 2 is refused) — n + 16 with the sub-harmonic layer, whose tracker fires at most once per sample and does so on every sample
// once its increment passes 1 (the resampler's vibrato depth of 3 takes the layer to 8 x f0: above sr / 2 from F7 on).
// base = sample_off[note]; a pulse-train note's slots end where the next note's begin.
__host__ __device__ __forceinline__ int64_t pulse_slot_base(int64_t base, int note) { return base / 2 + 16 * (int64_t)note; }
__host__ __device__ __forceinline__ int64_t sub_slot_base(int64_t base, int note) { return base + 16 * (int64_t)note; }
__host__ __device__ __forceinline__ int32_t pulse_slot_cap(const int64_t *sample_off, int note)
{
    return (int32_t)(pulse_slot_base(sample_off[note + 1], note + 1) - pulse_slot_base(sample_off[note], note));
}
// slots of a batch of n notes, N samples in all (+ 16 behind the last note)
static inline size_t onset_slots(int64_t N, int n, bool sub_on) { return (size_t)(sub_on ? N : N / 2) + 16 * (size_t)n + 16; }

// ---- device helpers ------------------------------------------------------------------------

// numpy 'reflect' (no edge repeat) as a periodic map; n == 1 degenerates to 'edge'.
__device__ __forceinline__ int64_t reflect_index(int64_t i, int64_t n)
{
    if (n <= 1) return 0;
    if (i >= 0 && i < n) return i;                           // in range: the usual case
    const int64_t period = 2 * (n - 1);
    if (i > -n && i < period) return i < 0 ? -i : period - i;   // one reflection, no 64-bit modulo (it costs ~100 instructions)
    int64_t m = i % period;
    if (m < 0) m += period;
    return m < n ? m : period - m;
}

__device__ __forceinline__ void wave_lds_sync()
{
    // LDS ops of one wave complete in issue order; this only stops the compiler reordering
    // across the exchange and waits for outstanding LDS traffic.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// butterfly reductions over the 64 lanes (o = 32 .. 1): every lane gets the result
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// write-once data: a store with the non-temporal hint (global_store ... nt) when `nt`
typedef float v4f_nt __attribute__((ext_vector_type(4)));
typedef float v2f_nt __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_f4(float *p, float4 v, bool nt)
{
    if (nt) __builtin_nontemporal_store(v4f_nt{v.x, v.y, v.z, v.w}, reinterpret_cast<v4f_nt *>(p));
    else *reinterpret_cast<float4 *>(p) = v;
}
__device__ __forceinline__ void store_f2(float2 *p, float2 v, bool nt)
{
    if (nt) __builtin_nontemporal_store(v2f_nt{v.x, v.y}, reinterpret_cast<v2f_nt *>(p));
    else *p = v;
}
__device__ __forceinline__ void store_f1(float *p, float v, bool nt)
{
    if (nt) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// ~1e-16-accurate reciprocal (v_rcp_f64 + two Newton steps), used where the reference divides but
// the quotient only positions or scales a continuous interpolant (the fp32 result is unaffected
// except in knife-edge roundings)
__device__ __forceinline__ double fast_rcp(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    return r;
}

// atomic max on a non-negative float through its bit pattern
__device__ __forceinline__ void atomic_max_pos(float *addr, float v)
{
    atomicMax(reinterpret_cast<unsigned int *>(addr), __float_as_uint(v));
}

// x / d for a divisor whose correctly rounded reciprocal r = RN(1 / d) is at hand: q = RN(x r) is within an ulp,
// the FMA residual x - q d is exact, and RN(q + residual r) is the correctly rounded quotient (Markstein 1990) —
// for finite operands and a quotient in the normal range, which is where audio samples over a window sum live
// (a zero stays a zero; a subnormal quotient may differ from the division in its last subnormal bit).  Three FMAs
// instead of the dozen instructions of the IEEE division sequence.
__device__ __forceinline__ float div_by(float x, float d, float r)
{
    const float q = x * r;
    return fmaf(fmaf(-q, d, x), r, q);
}
__device__ __forceinline__ double div_by(double x, double d, double r)
{
    const double q = x * r;
    return fma(fma(-q, d, x), r, q);
}

// np.linspace(0, 1, m)[k] and np.linspace(1, 0, m)[k] in fp64, 0 <= k < m: numpy's step form with the last point pinned
__device__ __forceinline__ double ramp_up(int k, int m) { return m > 1 ? (k == m - 1 ? 1.0 : (double)k * (1.0 / (double)(m - 1))) : 0.0; }
__device__ __forceinline__ double ramp_down(int k, int m) { return m > 1 ? (k == m - 1 ? 0.0 : (double)k * (-1.0 / (double)(m - 1)) + 1.0) : 1.0; }

// 1 inside [a, b), 0 outside, with linear fades of up to `fade` samples at both ends (fp32 products of fp64 weights): the
// vocal-fry mask of the resampler, per sample in the post chain and per frame centre in the assembly   SillySampler.py:883-934
__device__ __forceinline__ float fade_mask(int64_t i, int a, int b, int fade)
{
    if (i < a || i >= b) return 0.f;
    float v = 1.0f;
    if (fade > 0) {
        const int a1 = b < a + fade ? b : a + fade;
        if (i < a1) v = (float)((double)v * ramp_up((int)(i - a), a1 - a));
        const int b0 = a > b - fade ? a : b - fade;
        if (i >= b0) v = (float)((double)v * ramp_down((int)(i - b0), b - b0));
    }
    return v;
}

// gf.create_volume_jitter(vibrato=True) before its strength and clip: a zero-phase sinusoid at `speed` Hz with a 0.1 s linear
// fade-in (none for a note no longer than the fade), sample i of n   GOOFER.py:638-660
__device__ __forceinline__ double vibrato_env(int64_t i, int64_t n, double sr, double speed)
{
    double z = sin(((2.0 * 3.141592653589793) * speed) * ((double)i / sr) + 0.0);
    const int fade = (int)(0.1 * sr);
    if (fade < n && i < fade) z *= ramp_up((int)i, fade);
    return z;
}

// Read a kernel argument from the kernarg segment at the point of use.  The frame walkers keep ~40 scalars of wave state across
// their frame loop; arguments that are only needed every 64 frames (the frame-record arrays) or once per note kept live
// beside them pushed the compiler past the 102 SGPRs of a wave, and every overflow costs a v_writelane / v_readlane pair in
// the loop (the noise walker carried 105 such spills).  The empty asm hides the segment pointer from the optimiser, so the
// load cannot be hoisted back to the kernel entry; it is a scalar load from the constant cache.
template <typename T>
__device__ __forceinline__ T cold_arg(size_t offset)
{
    const char __attribute__((address_space(4))) *ka = (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *reinterpret_cast<const T __attribute__((address_space(4))) *>(ka + offset);
}
#define COLD(type, field) cold_arg<decltype(type::field)>(offsetof(type, field))
