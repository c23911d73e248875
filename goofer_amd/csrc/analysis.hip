// Analysis half that does not need Praat (gfx950): spectral envelope of a wav and its mel-knot encoding.
//
//   k_gauss_rows64 Gaussian FIR along bins with fp64 output (sigma = 0.5 pre-blur)       GOOFER.py:100
//   k_knot_error   for one knot count K: max over probe frames and bins of
//                  |exp(lerp(log knots)) - env| / (env + 1e-8)                            GOOFER.py:112-121
//   k_knot_gather  log-envelope sampled at the knots' nearest bins -> fp16 [rows x K]     GOOFER.py:114-115, 126
// These serve compress_env_to_knots on a caller's envelope; its K search loop (9 candidates) is host logic.
//
// The analysis of signals (goofer_envelope_knots_batch) runs the same arithmetic for a ragged batch in three launches:
//   k_env_rows_fused  |S| + 1e-8 (fp32) -> k_gauss_rows64 (sigma 2) -> fp32 cast -> k_gauss_rows64 (sigma 0.5) for one frame
//                     row, in LDS
//   k_knot_search     every probe row of every signal against all KN_CAND knot counts; per (signal, candidate) the max of
//                     k_knot_error's relative error
//   k_knot_pick       per signal the first candidate under 1e-2 (else the last), then k_knot_gather's fp16 knots at its bins
#include <hip/hip_fp16.h>

#include "common.h"
#include "launchers.h"

constexpr int AN_ROWS = 4;

// numpy's max / maximum: a NaN operand wins (fmax returns the other one).  On non-NaN operands this is fmax, so every
// finite result keeps its bits; a NaN error's bit pattern orders above every finite one for the atomicMax below.
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

__global__ __launch_bounds__(256) void k_gauss_rows64(const float *__restrict__ in, int ld, double *__restrict__ out, int ld64,
                                                      int64_t rows, int n_bins, const double *__restrict__ taps, int radius)
{
    extern __shared__ __align__(16) unsigned char smem[];
    float *s_rows = reinterpret_cast<float *>(smem);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * AN_ROWS + wave;
    if (r >= rows) return;
    float *row = s_rows + wave * n_bins;
    for (int b = lane; b < n_bins; b += WAVE) row[b] = in[r * ld + b];
    wave_lds_sync();
    for (int b = lane; b < n_bins; b += WAVE) {
        double acc = 0.0;
        for (int j = 0; j <= 2 * radius; ++j) acc += taps[j] * (double)row[reflect_index(b + j - radius, n_bins)];
        out[r * ld64 + b] = acc;
    }
}

// err_bits: max relative error as the bit pattern of a non-negative double or NaN (order-preserving for atomicMax, NaN on top)
__global__ __launch_bounds__(256) void k_knot_error(const double *__restrict__ env2, int ld64, const int64_t *__restrict__ probe,
                                                    int n_probe, int n_bins, const int *__restrict__ knot_bin, int K,
                                                    const int *__restrict__ lerp_idx, const float *__restrict__ w0,
                                                    const float *__restrict__ w1, unsigned long long *__restrict__ err_bits)
{
    extern __shared__ __align__(16) unsigned char smem[];
    float *s_kv = reinterpret_cast<float *>(smem);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pi = blockIdx.x * AN_ROWS + wave;
    if (pi >= n_probe) return;
    const double *row = env2 + probe[pi] * (int64_t)ld64;
    float *kv = s_kv + wave * K;
    for (int k = lane; k < K; k += WAVE) kv[k] = (float)log(nan_max(row[knot_bin[k]], 1e-8));
    wave_lds_sync();
    double worst = 0.0;
    for (int b = lane; b < n_bins; b += WAVE) {
        int i = lerp_idx[b];
        float rec = w0[b] * kv[i] + w1[b] * kv[i + 1];
        double e = row[b];
        double err = fabs((double)expf(rec) - e) / (e + 1e-8);
        worst = nan_max(worst, err);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = nan_max(worst, __shfl_xor(worst, o, 64));
    if (lane == 0) atomicMax(err_bits, (unsigned long long)__double_as_longlong(worst));
}

__global__ __launch_bounds__(256) void k_knot_gather(const double *__restrict__ env2, int ld64, int64_t rows,
                                                     const int *__restrict__ knot_bin, int K, __half *__restrict__ knots)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= rows * K) return;
    int64_t r = g / K;
    int k = (int)(g - r * K);
    float v = (float)log(nan_max(env2[r * ld64 + knot_bin[k]], 1e-8));     // log in fp64, cast to fp32 (DCOMPUTE)
    knots[g] = __float2half(v);                                         // then to fp16 (DSTORAGE)
}

int launch_gauss_rows64(goofer_ctx *ctx, const float *in, int ld, double *out, int ld64, int64_t rows, int n_bins,
                        const double *d_taps, int radius, hipStream_t st)
{
    if (rows <= 0) return GOOFER_OK;
    hipLaunchKernelGGL(k_gauss_rows64, dim3((unsigned)((rows + AN_ROWS - 1) / AN_ROWS)), dim3(256), sizeof(float) * AN_ROWS * n_bins,
                       st, in, ld, out, ld64, rows, n_bins, d_taps, radius);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

int launch_knot_error(goofer_ctx *ctx, const double *env2, int ld64, const int64_t *probe, int n_probe, int n_bins,
                      const int *knot_bin, int K, const int *lerp_idx, const float *w0, const float *w1,
                      unsigned long long *err_bits, hipStream_t st)
{
    if (n_probe <= 0) return GOOFER_OK;
    hipLaunchKernelGGL(k_knot_error, dim3((n_probe + AN_ROWS - 1) / AN_ROWS), dim3(256), sizeof(float) * AN_ROWS * K, st, env2, ld64,
                       probe, n_probe, n_bins, knot_bin, K, lerp_idx, w0, w1, err_bits);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

int launch_knot_gather(goofer_ctx *ctx, const double *env2, int ld64, int64_t rows, const int *knot_bin, int K, uint16_t *knots,
                       hipStream_t st)
{
    if (rows <= 0) return GOOFER_OK;
    hipLaunchKernelGGL(k_knot_gather, dim3((unsigned)((rows * K + 255) / 256)), dim3(256), 0, st, env2, ld64, rows, knot_bin, K,
                       reinterpret_cast<__half *>(knots));
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

// ---- the batched analysis ------------------------------------------------------------------------------------------------

// One wave per frame row: |S| + 1e-8 (fp32), sigma-2 blur (fp64, optionally written out), rounded to fp32, sigma-0.5 blur (fp64)
// into env2.  Same taps, tap order, reflect_index and casts as hypotf + 1e-8 -> k_gauss_rows64 -> .to(float32) -> k_gauss_rows64.
__global__ __launch_bounds__(256) void k_env_rows_fused(const float2 *__restrict__ S, int ldc, int64_t rows, int n_bins,
                                                        const double *__restrict__ taps_env, int r_env, const double *__restrict__ taps_fit,
                                                        int r_fit, double *__restrict__ env_rows, int ld64, double *__restrict__ env2, int ld2)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * AN_ROWS + wave;
    if (r >= rows) return;
    float *mag = reinterpret_cast<float *>(smem) + (size_t)wave * 2 * n_bins;
    float *env32 = mag + n_bins;
    for (int b = lane; b < n_bins; b += WAVE) {
        float2 s = S[r * ldc + b];
        mag[b] = hypotf(s.x, s.y) + 1e-8f;
    }
    wave_lds_sync();
    for (int b = lane; b < n_bins; b += WAVE) {
        double acc = 0.0;
        for (int j = 0; j <= 2 * r_env; ++j) acc += taps_env[j] * (double)mag[reflect_index(b + j - r_env, n_bins)];
        if (env_rows) env_rows[r * ld64 + b] = acc;
        env32[b] = (float)acc;
    }
    wave_lds_sync();
    for (int b = lane; b < n_bins; b += WAVE) {
        double acc = 0.0;
        for (int j = 0; j <= 2 * r_fit; ++j) acc += taps_fit[j] * (double)env32[reflect_index(b + j - r_fit, n_bins)];
        env2[r * ld2 + b] = acc;
    }
}

// One wave per probe row: the row is read into LDS once, then every candidate K = KN_K0 + KN_DK c is scored against it with
// k_knot_error's arithmetic.  Per wave and candidate one atomicMax on the bit pattern of a non-negative double (max is
// order-independent).  knot_bin: the candidates' bins back to back; lerp_idx / w0 / w1: [KN_CAND][n_bins].
__global__ __launch_bounds__(256) void k_knot_search(const double *__restrict__ env2, int ld2, const int64_t *__restrict__ probe_row,
                                                     const int *__restrict__ probe_sig, int n_probe, int n_bins,
                                                     const int *__restrict__ knot_bin, const int *__restrict__ lerp_idx,
                                                     const float *__restrict__ w0, const float *__restrict__ w1,
                                                     unsigned long long *__restrict__ err_bits)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pi = blockIdx.x * AN_ROWS + wave;
    if (pi >= n_probe) return;
    double *row = reinterpret_cast<double *>(smem) + (size_t)wave * n_bins;
    float *kv = reinterpret_cast<float *>(reinterpret_cast<double *>(smem) + (size_t)AN_ROWS * n_bins) + wave * KN_KMAX;
    const double *src = env2 + probe_row[pi] * (int64_t)ld2;
    for (int b = lane; b < n_bins; b += WAVE) row[b] = src[b];
    const int sig = probe_sig[pi];
    wave_lds_sync();
    int kb = 0;
    for (int c = 0; c < KN_CAND; ++c) {
        const int K = KN_K0 + KN_DK * c;
        for (int k = lane; k < K; k += WAVE) kv[k] = (float)log(nan_max(row[knot_bin[kb + k]], 1e-8));
        wave_lds_sync();
        const int *idx = lerp_idx + (size_t)c * n_bins;
        const float *a0 = w0 + (size_t)c * n_bins, *a1 = w1 + (size_t)c * n_bins;
        double worst = 0.0;
        for (int b = lane; b < n_bins; b += WAVE) {
            int i = idx[b];
            float rec = a0[b] * kv[i] + a1[b] * kv[i + 1];
            double e = row[b];
            double err = fabs((double)expf(rec) - e) / (e + 1e-8);
            worst = nan_max(worst, err);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) worst = nan_max(worst, __shfl_xor(worst, o, 64));
        if (lane == 0) atomicMax(err_bits + (size_t)sig * KN_CAND + c, (unsigned long long)__double_as_longlong(worst));
        wave_lds_sync();                                                   // every lane is done with kv before the next K fills it
        kb += K;
    }
}

// One thread per (frame row, knot slot < KN_KMAX): the signal's K is the first candidate with error < 1e-2, else the last;
// knots of signal s go frames-major [T_s x K_s] to the start of its slot of T_s x KN_KMAX halves at frame_off[s] * KN_KMAX.
__global__ __launch_bounds__(256) void k_knot_pick(const double *__restrict__ env2, int ld2, int64_t rows, const int *__restrict__ frame_sig,
                                                   const int64_t *__restrict__ frame_off, const int *__restrict__ knot_bin,
                                                   const unsigned long long *__restrict__ err_bits, __half *__restrict__ knots,
                                                   int32_t *__restrict__ K_out)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= rows * KN_KMAX) return;
    const int64_t r = g / KN_KMAX;
    const int k = (int)(g - r * KN_KMAX);
    const int s = frame_sig[r];
    int c = 0, kb = 0;
    while (c < KN_CAND - 1 && !(__longlong_as_double((long long)err_bits[(size_t)s * KN_CAND + c]) < 1e-2)) {
        kb += KN_K0 + KN_DK * c;
        ++c;
    }
    const int K = KN_K0 + KN_DK * c;
    const int64_t f0 = frame_off[s];
    if (r == f0 && k == 0) K_out[s] = K;
    if (k >= K) return;
    float v = (float)log(nan_max(env2[r * ld2 + knot_bin[kb + k]], 1e-8));
    knots[f0 * KN_KMAX + (r - f0) * K + k] = __float2half(v);
}

int launch_env_rows_fused(goofer_ctx *ctx, const float2 *S, int ldc, int64_t rows, int n_bins, const double *taps_env, int r_env,
                          const double *taps_fit, int r_fit, double *env_rows, int ld64, double *env2, int ld2, hipStream_t st)
{
    if (rows <= 0) return GOOFER_OK;
    const size_t lds = sizeof(float) * 2 * AN_ROWS * n_bins;
    if (lds > 64 * 1024)                                       // n_fft above 2048: 65.6 KB at 2049 bins
        if (int arc = kernel_allow_max_lds(ctx, (const void *)k_env_rows_fused)) return arc;
    hipLaunchKernelGGL(k_env_rows_fused, dim3((unsigned)((rows + AN_ROWS - 1) / AN_ROWS)), dim3(256), lds,
                       st, S, ldc, rows, n_bins, taps_env, r_env, taps_fit, r_fit, env_rows, ld64, env2, ld2);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

int launch_knot_search(goofer_ctx *ctx, const double *env2, int ld2, const int64_t *probe_row, const int *probe_sig, int n_probe, int n_bins,
                       const int *knot_bin, const int *lerp_idx, const float *w0, const float *w1, unsigned long long *err_bits,
                       hipStream_t st)
{
    if (n_probe <= 0) return GOOFER_OK;
    const size_t lds = AN_ROWS * (sizeof(double) * n_bins + sizeof(float) * KN_KMAX);
    if (lds > 64 * 1024)                                       // n_fft above 2048: 68.6 KB at 2049 bins
        if (int arc = kernel_allow_max_lds(ctx, (const void *)k_knot_search)) return arc;
    hipLaunchKernelGGL(k_knot_search, dim3((n_probe + AN_ROWS - 1) / AN_ROWS), dim3(256), lds, st, env2, ld2, probe_row, probe_sig, n_probe,
                       n_bins, knot_bin, lerp_idx, w0, w1, err_bits);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

int launch_knot_pick(goofer_ctx *ctx, const double *env2, int ld2, int64_t rows, const int *frame_sig, const int64_t *frame_off,
                     const int *knot_bin, const unsigned long long *err_bits, uint16_t *knots, int32_t *K_out, hipStream_t st)
{
    if (rows <= 0) return GOOFER_OK;
    hipLaunchKernelGGL(k_knot_pick, dim3((unsigned)((rows * KN_KMAX + 255) / 256)), dim3(256), 0, st, env2, ld2, rows, frame_sig, frame_off,
                       knot_bin, err_bits, reinterpret_cast<__half *>(knots), K_out);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}
