// The f0 and formant half of the cold-cache analysis (gfx950), for a ragged batch of fp64 signals at one sample rate.
//
// The settings are the handle's goofer_track_settings (goofer_track_configure); their defaults, in brackets below, are what
// the reference hands to Praat.
//
// Pitch, Boersma (1993) autocorrelation method (floor [75] Hz, ceiling [950] Hz, time step hop / sr, 15 candidates, silence
// [0.03], voicing [0.45], octave [0.01], octave jump [0.35], voiced/unvoiced [0.14]):
//   k_pitch_stats    per signal: mean and peak of |y - mean| (the unvoiced candidate needs the whole signal's peak)
//   k_pitch_frames   per frame: mean removed, Hann window of 3 / floor, autocorrelation over the lag range divided by the
//                    window's own, parabolic peaks, octave cost, unvoiced strength; up to 15 candidates
//   k_pitch_viterbi  per signal, one wave: the best candidate path under octave-jump and voicing costs; unvoiced frames 0
// Formants, Burg's method as Praat's to_formant_burg describes it ([5] formants, ceiling [5500] Hz, 50 ms Gaussian):
//   k_resample       windowed-sinc interpolation to R = 2 x ceiling [11 kHz], up or down, one output sample per thread
//   k_formant_frames per frame, one wave: pre-emphasis from 50 Hz, Gaussian window of R / 20 samples [550], Burg of order
//                    2 x formants [10] in fp64, roots of the predictor by Aberth's method plus Newton polishing, roots at
//                    50 < f < R / 2 - 50 Hz sorted into F1..; a template on (window slots per lane, order), the default
//                    settings' instantiation with its window and rate as compile-time constants
// Every frame and signal is computed from its own samples in a fixed order, so a signal's tracks do not depend on the batch.
// tests/tracker_ref.py restates the same algorithm in numpy.
#include <math.h>

#include <vector>

#include "common.h"
#include "ragged.h"

namespace {

constexpr int TR_PERIODS = 3, TR_MAX_CAND = 15;
constexpr double TR_SILENT_PEAK = 1e-10;               // a signal whose peak deviation from its mean is below this is silence
constexpr int TR_SR_MIN = 8000, TR_SR_MAX = 96000;
constexpr int TR_FLOOR_MIN = 20, TR_FLOOR_MAX = 600;   // W = 3 sr / floor: 14400 doubles at most, 40 at least
constexpr double TR_CEILING_MAX = 20000.0;
constexpr size_t TR_LDS_OPT_IN = 64 * 1024, TR_LDS_MAX = 160 * 1024;   // a pitch frame and its lags in LDS (k_pitch_frames)

constexpr goofer_track_settings TR_DEFAULT = GOOFER_TRACK_SETTINGS_DEFAULT;
// the default settings' formant geometry: k_formant_frames' instantiation with compile-time sizes
constexpr int FM_SR = 2 * TR_DEFAULT.max_formant, FM_WIN = FM_SR / 20, FM_ORDER = 2 * TR_DEFAULT.n_formants;
constexpr int FM_N = 5;                                // output columns
constexpr int FM_MAX_FORMANT_MIN = 2500, FM_MAX_FORMANT_MAX = 8000, FM_WIN_MAX = 2 * FM_MAX_FORMANT_MAX / 20;
constexpr int FM_SLOTS_MIN = (2 * FM_MAX_FORMANT_MIN / 20 + WAVE - 1) / WAVE, FM_SLOTS_MAX = (FM_WIN_MAX + WAVE - 1) / WAVE;
constexpr double FM_PRE_HZ = 50.0, FM_SINC_ZEROS = 20.0;
constexpr int FM_ABERTH_ITERS = 100;

constexpr int TR_THREADS = 256;

// the settings a call runs with: the handle's, or the defaults where a query form has no handle
const goofer_track_settings &settings_of(const goofer_ctx *ctx) { return ctx ? ctx->track : TR_DEFAULT; }

struct pitch_geom {
    int floor, W, min_lag, max_lag, lo, hi;               // r[] is kept for lags lo..hi
    double ceiling;
};

pitch_geom pitch_geometry(const goofer_track_settings &ts, int sr)
{
    pitch_geom g;
    g.floor = ts.pitch_floor;
    g.W = TR_PERIODS * sr / g.floor;
    g.ceiling = std::min(ts.pitch_ceiling, 0.5 * sr);
    g.min_lag = (int)floor(sr / g.ceiling);
    g.max_lag = (sr + g.floor - 1) / g.floor;
    g.lo = std::max(1, g.min_lag - 1);
    g.hi = std::min(g.max_lag + 1, g.W - 1);
    return g;
}

int64_t pitch_min_length(const goofer_track_settings &ts, int sr) { return ((int64_t)TR_PERIODS * sr + ts.pitch_floor - 1) / ts.pitch_floor; }

int64_t pitch_frames(const goofer_track_settings &ts, int64_t n, int sr, int hop)
{
    const int64_t d = (int64_t)ts.pitch_floor * n - (int64_t)TR_PERIODS * sr;
    return d < 0 ? 0 : d / ((int64_t)ts.pitch_floor * hop) + 1;
}

// the formant stage's rate R, its window and its Burg order
struct formant_geom {
    int fsr, win, order;
};
formant_geom formant_geometry(const goofer_track_settings &ts) { return {2 * ts.max_formant, 2 * ts.max_formant / 20, 2 * ts.n_formants}; }

int64_t resampled_length(const formant_geom &fg, int64_t n, int sr) { return n * fg.fsr / sr; }

// formant frames of a signal of m samples at R Hz placed as a signal at sr with hop would place them
int64_t formant_frames(const formant_geom &fg, int64_t m, int sr, int hop)
{
    return m < fg.win ? 0 : (m - fg.win) * sr / ((int64_t)fg.fsr * hop) + 1;
}

// ---- device helpers ----------------------------------------------------------------------------------------------
// numpy's max: a NaN operand wins (fmax returns the other one).  On non-NaN operands this is fmax, so every finite result
// keeps its bits.
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ double wave_max_d(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o, 64));
    return v;
}

// fixed-order block reductions over TR_THREADS threads (every thread gets the result); red: 4 doubles of LDS
__device__ double block_sum_d(double v, double *red)
{
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ double block_max_d(double v, double *red)
{
    v = wave_max_d(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    return nan_max(nan_max(red[0], red[1]), nan_max(red[2], red[3]));
}

// ---- pitch -------------------------------------------------------------------------------------------------------
// stats[2 s] = mean of signal s, stats[2 s + 1] = max |y - mean|, NaN when a sample is NaN or infinite (as numpy's max)
__global__ __launch_bounds__(TR_THREADS) void k_pitch_stats(const double *__restrict__ y, const int64_t *__restrict__ soff,
                                                            double *__restrict__ stats)
{
    __shared__ double red[4];
    const int s = blockIdx.x;
    const int64_t a = soff[s], n = soff[s + 1] - a;
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += TR_THREADS) acc += y[a + j];
    const double mean = block_sum_d(acc, red) / (double)n;
    double pk = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += TR_THREADS) pk = nan_max(pk, fabs(y[a + j] - mean));
    pk = block_max_d(pk, red);
    if (threadIdx.x == 0) {
        stats[2 * s] = mean;
        stats[2 * s + 1] = pk;
    }
}

// One frame per workgroup.  LDS: the windowed frame [W], the normalised autocorrelation for lags lo..hi, reductions.
__global__ __launch_bounds__(TR_THREADS) void k_pitch_frames(const double *__restrict__ y, const int64_t *__restrict__ soff,
                                                             const int64_t *__restrict__ foff, int n_sig, int sr, int hop,
                                                             pitch_geom g, double silence, double voicing, double octave,
                                                             const double *__restrict__ win, const double *__restrict__ rw,
                                                             const double *__restrict__ stats,
                                                             double *__restrict__ cand_f, double *__restrict__ cand_s,
                                                             int *__restrict__ cand_n)
{
    extern __shared__ __align__(16) unsigned char smem[];
    double *xw = reinterpret_cast<double *>(smem);
    double *r = xw + g.W;                                 // r[t - lo]
    __shared__ double red[4];
    __shared__ double kf[TR_MAX_CAND - 1], ks[TR_MAX_CAND - 1];
    const int64_t f = blockIdx.x;
    const int s = csr_find(foff, n_sig, f);
    const int64_t n = soff[s + 1] - soff[s], nf = foff[s + 1] - foff[s], i = f - foff[s];
    const int W = g.W;
    const double *x = y + soff[s] + (n - (nf - 1) * hop - W) / 2 + i * hop;

    double acc = 0.0;
    for (int j = threadIdx.x; j < W; j += TR_THREADS) {
        const double v = x[j];
        xw[j] = v;
        acc += v;
    }
    const double mean = block_sum_d(acc, red) / (double)W;
    double pk = 0.0, e = 0.0;
    for (int j = threadIdx.x; j < W; j += TR_THREADS) {
        const double v = xw[j] - mean;
        pk = nan_max(pk, fabs(v));
        const double u = v * win[j];
        xw[j] = u;
        e += u * u;
    }
    pk = block_max_d(pk, red);
    const double r0 = block_sum_d(e, red);               // also orders the xw writes before the lag products
    const double gp = stats[2 * s + 1];
    // a NaN peak (a non-finite sample) gives a NaN ratio, and fmax(0, NaN) = 0 as Python's max(0.0, nan): uv = voicing
    const double ratio = !(gp <= TR_SILENT_PEAK) ? pk / gp : 0.0;
    const double uv = voicing + fmax(0.0, 2.0 - ratio / (silence / (1.0 + voicing)));
    double *cf = cand_f + f * TR_MAX_CAND, *cs = cand_s + f * TR_MAX_CAND;
    if (!(r0 > 0.0)) {
        if (threadIdx.x == 0) {
            cf[0] = 0.0;
            cs[0] = uv;
            cand_n[f] = 1;
        }
        return;
    }
    for (int t = g.lo + threadIdx.x; t <= g.hi; t += TR_THREADS) {
        double a = 0.0;
        for (int j = 0; j < W - t; ++j) a += xw[j] * xw[j + t];
        r[t - g.lo] = a / (r0 * rw[t]);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    // serial peak scan in lag order; keep the 14 strongest (the earlier lag among equals), in lag order
    int cnt = 0;
    const int t0 = max(g.lo + 1, g.min_lag), t1 = min(g.max_lag, g.hi - 1);
    for (int t = t0; t <= t1; ++t) {
        const double rm1 = r[t - 1 - g.lo], rc = r[t - g.lo], rp1 = r[t + 1 - g.lo];
        if (!(rc > 0.5 * voicing && rc > rm1 && rc >= rp1)) continue;
        const double dr = 0.5 * (rp1 - rm1), d2r = 2.0 * rc - rm1 - rp1;
        const double delta = d2r > 0.0 ? dr / d2r : 0.0;
        double rmax = rc + 0.5 * dr * delta;
        if (rmax > 1.0) rmax = 1.0 / rmax;
        const double fr = (double)sr / ((double)t + delta);
        if (fr < (double)g.floor || fr > g.ceiling) continue;
        const double st = rmax - octave * log2((double)g.floor / fr);
        if (cnt < TR_MAX_CAND - 1) {
            kf[cnt] = fr;
            ks[cnt] = st;
            ++cnt;
            continue;
        }
        int w = 0;                                        // the weakest kept, the latest among equals
        for (int k = 1; k < cnt; ++k)
            if (ks[k] <= ks[w]) w = k;
        if (!(st > ks[w])) continue;
        for (int k = w; k < cnt - 1; ++k) {
            kf[k] = kf[k + 1];
            ks[k] = ks[k + 1];
        }
        kf[cnt - 1] = fr;
        ks[cnt - 1] = st;
    }
    cf[0] = 0.0;
    cs[0] = uv;
    for (int k = 0; k < cnt; ++k) {
        cf[k + 1] = kf[k];
        cs[k + 1] = ks[k];
    }
    cand_n[f] = cnt + 1;
}

__device__ __forceinline__ double pitch_transition(double fp, double fc, double tsc, double octave_jump, double vuv)
{
    if (fp == 0.0 && fc == 0.0) return 0.0;
    if (fp == 0.0 || fc == 0.0) return vuv * tsc;
    return octave_jump * tsc * fabs(log2(fp / fc));
}

// One wave per signal: lane c holds candidate c of the current frame; back pointers go to global memory.  The first best
// predecessor wins a tie, and the first best candidate of the last frame.
__global__ __launch_bounds__(WAVE) void k_pitch_viterbi(const int64_t *__restrict__ foff, const double *__restrict__ cand_f,
                                                        const double *__restrict__ cand_s, const int *__restrict__ cand_n,
                                                        double tsc, double octave_jump, double vuv,
                                                        unsigned char *__restrict__ back, double *__restrict__ f0)
{
    __shared__ double pf[TR_MAX_CAND], pd[TR_MAX_CAND];
    __shared__ int pn;
    const int s = blockIdx.x, c = threadIdx.x;
    const int64_t a = foff[s], nf = foff[s + 1] - a;
    if (nf <= 0) return;
    const int n0 = min(max(cand_n[a], 1), TR_MAX_CAND);   // a caller's count outside [1, 15] is clamped into it
    if (c < TR_MAX_CAND) {
        const bool on = c < n0;
        pf[c] = on ? cand_f[a * TR_MAX_CAND + c] : 0.0;
        pd[c] = on ? cand_s[a * TR_MAX_CAND + c] : -INFINITY;
    }
    if (c == 0) pn = n0;
    wave_lds_sync();
    for (int64_t i = 1; i < nf; ++i) {
        const int64_t fr = a + i;
        const int cn = min(max(cand_n[fr], 1), TR_MAX_CAND);
        double fc = 0.0, best = -INFINITY;
        int arg = 0;
        if (c < cn) {
            fc = cand_f[fr * TR_MAX_CAND + c];
            for (int p = 0; p < pn; ++p) {
                const double v = pd[p] - pitch_transition(pf[p], fc, tsc, octave_jump, vuv);
                if (v > best) {
                    best = v;
                    arg = p;
                }
            }
            best += cand_s[fr * TR_MAX_CAND + c];
            back[fr * TR_MAX_CAND + c] = (unsigned char)arg;
        }
        wave_lds_sync();                                  // every lane has read the previous frame
        if (c < TR_MAX_CAND) {
            pf[c] = fc;
            pd[c] = c < cn ? best : -INFINITY;
        }
        if (c == 0) pn = cn;
        wave_lds_sync();
    }
    if (c != 0) return;
    int k = 0;
    for (int p = 1; p < pn; ++p)
        if (pd[p] > pd[k]) k = p;
    for (int64_t i = nf - 1; i >= 0; --i) {
        const int64_t fr = a + i;
        f0[fr] = cand_f[fr * TR_MAX_CAND + k];
        if (i > 0) k = back[fr * TR_MAX_CAND + k];
    }
}

// ---- formants ----------------------------------------------------------------------------------------------------
// out[m] = sum_k y[k] h(k - p), p = m sr / fsr: a Hann-windowed sinc with its cut-off at the lower Nyquist, its half-width
// 20 zero crossings of the lower rate (fsr > sr interpolates between the samples).  FSR > 0: the output rate as a compile-time
// constant (the default settings; fsr_rt is not read), FSR = 0: fsr_rt.
template <int FSR>
__global__ __launch_bounds__(TR_THREADS) void k_resample(const double *__restrict__ y, const int64_t *__restrict__ soff,
                                                         const int64_t *__restrict__ moff, int n_sig, int64_t m_total, int sr,
                                                         int fsr_rt, double *__restrict__ out)
{
    const int fsr = FSR > 0 ? FSR : fsr_rt;
    const int64_t g = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x;
    if (g >= m_total) return;
    const int s = csr_find(moff, n_sig, g);
    const int64_t m = g - moff[s], n = soff[s + 1] - soff[s];
    const double *x = y + soff[s];
    const double fc = 0.5 * (double)min(sr, fsr) / (double)sr;
    const double half = FM_SINC_ZEROS * fmax(1.0, (double)sr / (double)fsr);
    const double p = (double)m * (double)sr / (double)fsr;
    const int64_t k0 = max((int64_t)0, (int64_t)ceil(p - half)), k1 = min(n - 1, (int64_t)floor(p + half));
    double acc = 0.0;
    for (int64_t k = k0; k <= k1; ++k) {
        const double d = (double)k - p;
        const double u = M_PI * (2.0 * fc * d);
        const double sinc = u == 0.0 ? 1.0 : sin(u) / u;
        acc += 2.0 * fc * sinc * (0.5 + 0.5 * cos(M_PI * d / half)) * x[k];
    }
    out[g] = acc;
}

struct cplx {
    double re, im;
};
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cplx cdiv(cplx a, cplx b)
{
    const double d = b.re * b.re + b.im * b.im;
    return {(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}

// p(z) and p'(z) of z^m + a[1] z^(m-1) + ... + a[m]
__device__ __forceinline__ void poly_eval(const double *a, int m, cplx z, cplx &p, cplx &d)
{
    p = {1.0, 0.0};
    d = {0.0, 0.0};
    for (int k = 1; k <= m; ++k) {
        d = cmul(d, z);
        d.re += p.re;
        d.im += p.im;
        p = cmul(p, z);
        p.re += a[k];
    }
}

// One wave per frame.  LDS per frame: the forward / backward prediction errors, the predictor, the roots.
// PER_LANE: window samples per lane, ORDER: the Burg order (twice the formants looked for).  FSR > 0: the rate and, with it,
// the window FSR / 20 and the pre-emphasis factor are compile-time constants and fsr_rt / win_rt / alpha_rt are not read (the
// default settings); FSR = 0: any rate whose window fits PER_LANE slots, with alpha_rt = exp(-2 pi 50 / fsr_rt) from the host.
template <int PER_LANE, int ORDER, int FSR>
__global__ __launch_bounds__(WAVE) void k_formant_frames(const double *__restrict__ x11, const int64_t *__restrict__ moff,
                                                         const int64_t *__restrict__ foff, int n_sig, int sr, int hop,
                                                         int fsr_rt, int win_rt, double alpha_rt,
                                                         const double *__restrict__ gwin, double *__restrict__ formants)
{
    constexpr int WIN_CAP = FSR > 0 ? FSR / 20 : PER_LANE * WAVE, NF = ORDER / 2;
    static_assert(WIN_CAP <= PER_LANE * WAVE && NF <= FM_N, "the window fits the lanes' slots, the formants the output row");
    __shared__ double fe[WIN_CAP], be[WIN_CAP];
    __shared__ double a[ORDER + 1];
    __shared__ cplx z[ORDER], w[ORDER];
    const int fsr = FSR > 0 ? FSR : fsr_rt, win = FSR > 0 ? FSR / 20 : win_rt;
    const int lane = threadIdx.x;
    const int64_t f = blockIdx.x;
    const int s = csr_find(foff, n_sig, f);
    const int64_t m = moff[s + 1] - moff[s], nf = foff[s + 1] - foff[s], i = f - foff[s];
    const int64_t num = (m - win) * sr + (2 * i - nf + 1) * (int64_t)hop * fsr;
    int64_t st = (num + sr) / (2 * (int64_t)sr);          // num + sr >= 0 for every frame of the layout
    st = min(max(st, (int64_t)0), m - win);
    const double *x = x11 + moff[s];
    const double alpha = FSR > 0 ? exp(-2.0 * M_PI * FM_PRE_HZ / FSR) : alpha_rt;

    double pk = 0.0;
    for (int j = lane; j < win; j += WAVE) {
        const int64_t q = st + j;
        const double v = (q > 0 ? x[q] - alpha * x[q - 1] : x[q]) * gwin[j];
        fe[j] = be[j] = v;
        pk = nan_max(pk, fabs(v));
    }
    double *out = formants + f * FM_N;
    if (wave_max_d(pk) == 0.0) {
        if (lane < FM_N) out[lane] = 0.0;
        return;
    }
    if (lane == 0) a[0] = 1.0;
    wave_lds_sync();
    int order = 0;
    for (int mo = 1; mo <= ORDER; ++mo) {
        double nu = 0.0, de = 0.0;
        double fn[PER_LANE], bn[PER_LANE];
#pragma unroll
        for (int q = 0; q < PER_LANE; ++q) {
            const int j = mo + lane + q * WAVE;
            if (j < win) {
                const double ff = fe[j], bb = be[j - 1];
                nu += ff * bb;
                de += ff * ff + bb * bb;
            }
        }
        nu = wave_sum(nu);
        de = wave_sum(de);
        if (!(de > 0.0)) break;
        const double k = -2.0 * nu / de;
#pragma unroll
        for (int q = 0; q < PER_LANE; ++q) {
            const int j = mo + lane + q * WAVE;
            if (j < win) {
                const double ff = fe[j], bb = be[j - 1];
                fn[q] = ff + k * bb;
                bn[q] = bb + k * ff;
            }
        }
        wave_lds_sync();                                  // all old values read before any is replaced
#pragma unroll
        for (int q = 0; q < PER_LANE; ++q) {
            const int j = mo + lane + q * WAVE;
            if (j < win) {
                fe[j] = fn[q];
                be[j] = bn[q];
            }
        }
        if (lane == 0) {
            a[mo] = 0.0;
            for (int l = 0; 2 * l <= mo; ++l) {           // a[l], a[mo - l] <- a[l] + k a[mo - l], a[mo - l] + k a[l]
                const double lo = a[l], hi = a[mo - l];
                a[l] = lo + k * hi;
                if (mo - l != l) a[mo - l] = hi + k * lo;
            }
        }
        wave_lds_sync();
        order = mo;
    }
    if (lane != 0) return;

    // Aberth-Ehrlich: all corrections from the current roots, then all roots move
    for (int k = 0; k < order; ++k) {
        const double ang = 2.0 * M_PI * k / order + 0.25;
        z[k] = {0.9 * cos(ang), 0.9 * sin(ang)};
    }
    for (int it = 0; it < FM_ABERTH_ITERS && order > 0; ++it) {
        for (int k = 0; k < order; ++k) {
            cplx p, d;
            poly_eval(a, order, z[k], p, d);
            const cplx ratio = (d.re != 0.0 || d.im != 0.0) ? cdiv(p, d) : cplx{0.0, 0.0};
            cplx sum = {0.0, 0.0};
            for (int j = 0; j < order; ++j) {
                if (j == k) continue;
                const cplx q = cdiv({1.0, 0.0}, {z[k].re - z[j].re, z[k].im - z[j].im});
                sum.re += q.re;
                sum.im += q.im;
            }
            const cplx rs = cmul(ratio, sum);
            w[k] = cdiv(ratio, {1.0 - rs.re, -rs.im});
        }
        bool done = true;
        for (int k = 0; k < order; ++k) {
            z[k].re -= w[k].re;
            z[k].im -= w[k].im;
            const double wa = hypot(w[k].re, w[k].im), za = fmax(hypot(z[k].re, z[k].im), 1e-300);
            done &= wa <= 1e-14 * za;
        }
        if (done) break;
    }
    for (int pass = 0; pass < 2; ++pass)
        for (int k = 0; k < order; ++k) {
            cplx p, d;
            poly_eval(a, order, z[k], p, d);
            if (d.re != 0.0 || d.im != 0.0) {
                const cplx c = cdiv(p, d);
                z[k].re -= c.re;
                z[k].im -= c.im;
            }
        }
    double fk[NF];
    int nk = 0;
    for (int k = 0; k < order; ++k) {
        if (!(z[k].im > 0.0)) continue;
        const double fr = atan2(z[k].im, z[k].re) * fsr / (2.0 * M_PI);
        if (!(fr > 50.0 && fr < 0.5 * fsr - 50.0)) continue;
        int pos = nk < NF ? nk++ : NF;                    // insertion into the NF lowest
        while (pos > 0 && fk[pos - 1] > fr) {
            if (pos < NF) fk[pos] = fk[pos - 1];
            --pos;
        }
        if (pos < NF) fk[pos] = fr;
    }
    for (int k = 0; k < FM_N; ++k) out[k] = k < nk ? fk[k] : 0.0;
}

// ---- host side ---------------------------------------------------------------------------------------------------
int check_batch(goofer_ctx *ctx, const int64_t *sample_off, int n_sig, int sr, int hop, int64_t min_len)
{
    if (!sample_off || n_sig <= 0) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: empty batch");
    if (sr < TR_SR_MIN || sr > TR_SR_MAX) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: sample rate %d outside [%d, %d]", sr, TR_SR_MIN, TR_SR_MAX);
    if (hop <= 0) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: hop %d", hop);
    if (sample_off[0] != 0) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: sample_off[0] must be 0");
    for (int s = 0; s < n_sig; ++s) {
        const int64_t n = sample_off[s + 1] - sample_off[s];
        if (n < min_len || n < 1)
            return goofer_fail(ctx, GOOFER_EINVAL, "tracker: signal %d has %lld samples, the pitch window needs at least %lld", s,
                               (long long)n, (long long)std::max<int64_t>(min_len, 1));
    }
    return GOOFER_OK;
}

// sr and hop as check_batch takes them, and offsets off[0..n_sig] that start at 0 and never decrease
int check_offsets(goofer_ctx *ctx, const int64_t *off, int n_sig, int sr, int hop, const char *what)
{
    if (!off || n_sig <= 0) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: empty batch");
    if (sr < TR_SR_MIN || sr > TR_SR_MAX) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: sample rate %d outside [%d, %d]", sr, TR_SR_MIN, TR_SR_MAX);
    if (hop <= 0) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: hop %d", hop);
    if (off[0] != 0) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: %s[0] must be 0", what);
    for (int s = 0; s < n_sig; ++s)
        if (off[s + 1] < off[s]) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: %s decreases at signal %d", what, s);
    return GOOFER_OK;
}

// the offsets each stage writes: out[s + 1] - out[s] = count(in[s + 1] - in[s])
template <typename Count> void fill_offsets(const int64_t *in, int n_sig, int64_t *out, Count count)
{
    out[0] = 0;
    for (int s = 0; s < n_sig; ++s) out[s + 1] = out[s] + count(in[s + 1] - in[s]);
}

// Each stage's scratch, in arena order (a braced list takes its pieces left to right).  A composite call carves its stages'
// blocks behind its own pieces and hands each stage its block.
struct cand_scratch { int64_t *soff, *foff; double *stats, *win, *rw; };
cand_scratch carve_candidates(arena &a, int n, const pitch_geom &g)
{
    return {a.take<int64_t>(n + 1), a.take<int64_t>(n + 1), a.take<double>(2 * (size_t)n), a.take<double>(g.W), a.take<double>(g.hi + 1)};
}
struct path_scratch { int64_t *foff; unsigned char *back; };
path_scratch carve_path(arena &a, int n, int64_t F) { return {a.take<int64_t>(n + 1), a.take<unsigned char>(TR_MAX_CAND * (size_t)F)}; }
struct resample_scratch { int64_t *soff, *moff; };
resample_scratch carve_resample(arena &a, int n) { return {a.take<int64_t>(n + 1), a.take<int64_t>(n + 1)}; }
struct formant_scratch { int64_t *moff, *foff; double *gwin; };
formant_scratch carve_formant_frames(arena &a, int n, const formant_geom &fg)
{
    return {a.take<int64_t>(n + 1), a.take<int64_t>(n + 1), a.take<double>(fg.win)};
}

// dynamic LDS of k_pitch_frames: the windowed frame and the lags lo..hi
size_t pitch_lds(const pitch_geom &g) { return 8 * (size_t)(g.W + g.hi - g.lo + 1); }
constexpr size_t PITCH_STATIC_LDS = 8 * (4 + 2 * (TR_MAX_CAND - 1));   // red, kf, ks

// a floor and rate whose frame does not fit a workgroup's LDS: refused by every form of the pitch calls
int check_pitch_lds(goofer_ctx *ctx, const pitch_geom &g, int sr)
{
    const size_t need = pitch_lds(g) + PITCH_STATIC_LDS;
    if (need > TR_LDS_MAX)
        return goofer_fail(ctx, GOOFER_EINVAL, "tracker: pitch floor %d Hz at %d Hz needs %zu bytes of LDS per frame (window %d, lags %d..%d), "
                           "more than %zu", g.floor, sr, need, g.W, g.lo, g.hi, TR_LDS_MAX);
    return GOOFER_OK;
}

const char *settings_error(const goofer_track_settings &t, char *buf, size_t cap)
{
    auto cost_ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
    if (t.pitch_floor < TR_FLOOR_MIN || t.pitch_floor > TR_FLOOR_MAX)
        snprintf(buf, cap, "pitch_floor %d outside [%d, %d]", t.pitch_floor, TR_FLOOR_MIN, TR_FLOOR_MAX);
    else if (!(t.pitch_ceiling > (double)t.pitch_floor && t.pitch_ceiling <= TR_CEILING_MAX))
        snprintf(buf, cap, "pitch_ceiling %g must be above the floor (%d) and at most %g", t.pitch_ceiling, t.pitch_floor, TR_CEILING_MAX);
    else if (!cost_ok(t.silence_threshold))
        snprintf(buf, cap, "silence_threshold %g must be finite and >= 0", t.silence_threshold);
    else if (!(t.voicing_threshold > 0.0 && t.voicing_threshold < 1.0))
        snprintf(buf, cap, "voicing_threshold %g outside (0, 1)", t.voicing_threshold);
    else if (!cost_ok(t.octave_cost))
        snprintf(buf, cap, "octave_cost %g must be finite and >= 0", t.octave_cost);
    else if (!cost_ok(t.octave_jump_cost))
        snprintf(buf, cap, "octave_jump_cost %g must be finite and >= 0", t.octave_jump_cost);
    else if (!cost_ok(t.voiced_unvoiced_cost))
        snprintf(buf, cap, "voiced_unvoiced_cost %g must be finite and >= 0", t.voiced_unvoiced_cost);
    else if (t.max_formant < FM_MAX_FORMANT_MIN || t.max_formant > FM_MAX_FORMANT_MAX)
        snprintf(buf, cap, "max_formant %d outside [%d, %d]", t.max_formant, FM_MAX_FORMANT_MIN, FM_MAX_FORMANT_MAX);
    else if (t.n_formants < 3 || t.n_formants > FM_N)
        snprintf(buf, cap, "n_formants %d is not 3, 4 or 5", t.n_formants);
    else
        return nullptr;
    return buf;
}

// k_formant_frames by (slots per lane, order): the default geometry runs its compile-time instantiation
using formant_kernel = void (*)(const double *, const int64_t *, const int64_t *, int, int, int, int, int, double, const double *, double *);
template <int ORDER> formant_kernel formant_kernel_of_slots(int slots)
{
    switch (slots) {
    case 4: return k_formant_frames<4, ORDER, 0>;
    case 5: return k_formant_frames<5, ORDER, 0>;
    case 6: return k_formant_frames<6, ORDER, 0>;
    case 7: return k_formant_frames<7, ORDER, 0>;
    case 8: return k_formant_frames<8, ORDER, 0>;
    case 9: return k_formant_frames<9, ORDER, 0>;
    case 10: return k_formant_frames<10, ORDER, 0>;
    case 11: return k_formant_frames<11, ORDER, 0>;
    case 12: return k_formant_frames<12, ORDER, 0>;
    case 13: return k_formant_frames<13, ORDER, 0>;
    }
    return nullptr;
}
static_assert(FM_SLOTS_MIN == 4 && FM_SLOTS_MAX == 13, "formant_kernel_of_slots covers the admitted windows");

formant_kernel formant_kernel_of(const formant_geom &fg)
{
    if (fg.fsr == FM_SR && fg.order == FM_ORDER) return k_formant_frames<(FM_WIN + WAVE - 1) / WAVE, FM_ORDER, FM_SR>;
    const int slots = (fg.win + WAVE - 1) / WAVE;
    switch (fg.order) {
    case 6: return formant_kernel_of_slots<6>(slots);
    case 8: return formant_kernel_of_slots<8>(slots);
    case 10: return formant_kernel_of_slots<10>(slots);
    }
    return nullptr;
}

}  // namespace

/* Exported: see include/goofer_hip.h */
extern "C" void goofer_track_settings_default(goofer_track_settings *settings)
{
    if (settings) *settings = TR_DEFAULT;
}

extern "C" int goofer_track_configure(goofer_ctx *ctx, const goofer_track_settings *settings)
{
    if (!ctx) return GOOFER_EINVAL;
    char why[160];
    if (settings && settings_error(*settings, why, sizeof why)) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_track_configure: %s", why);
    ctx->track = settings ? *settings : TR_DEFAULT;
    return GOOFER_OK;
}

extern "C" int goofer_track_layout(const goofer_track_settings *settings, const int64_t *sample_off, int n_signals, int sr, int hop,
                                   int64_t *pitch_off, int64_t *x_off, int64_t *formant_off)
{
    const goofer_track_settings &ts = settings ? *settings : TR_DEFAULT;
    char why[160];
    if (settings_error(ts, why, sizeof why)) return GOOFER_EINVAL;
    const formant_geom fg = formant_geometry(ts);
    int rc;
    if (pitch_off) {
        if ((rc = check_batch(nullptr, sample_off, n_signals, sr, hop, pitch_min_length(ts, sr)))) return rc;
        if ((rc = check_pitch_lds(nullptr, pitch_geometry(ts, sr), sr))) return rc;
        fill_offsets(sample_off, n_signals, pitch_off, [&](int64_t n) { return pitch_frames(ts, n, sr, hop); });
    }
    if ((rc = check_batch(nullptr, sample_off, n_signals, sr, hop, 1))) return rc;
    std::vector<int64_t> xo(n_signals + 1);
    fill_offsets(sample_off, n_signals, xo.data(), [&](int64_t n) { return resampled_length(fg, n, sr); });
    if (x_off) std::copy(xo.begin(), xo.end(), x_off);
    if (formant_off) fill_offsets(xo.data(), n_signals, formant_off, [&](int64_t m) { return formant_frames(fg, m, sr, hop); });
    return GOOFER_OK;
}

extern "C" int goofer_track_candidates(goofer_ctx *ctx, const double *y, const int64_t *sample_off, int n_signals, int sr, int hop,
                                       int64_t *frame_off, double *cand_f, double *cand_s, int32_t *cand_n, void *scratch,
                                       int64_t *scratch_bytes, void *stream)
{
    const goofer_track_settings ts = settings_of(ctx);
    int rc = check_batch(ctx, sample_off, n_signals, sr, hop, pitch_min_length(ts, sr));
    if (rc) return rc;
    if (!frame_off || !scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null frame_off / scratch_bytes");
    const pitch_geom g = pitch_geometry(ts, sr);
    if ((rc = check_pitch_lds(ctx, g, sr))) return rc;
    fill_offsets(sample_off, n_signals, frame_off, [&](int64_t n) { return pitch_frames(ts, n, sr, hop); });
    const int64_t F = frame_off[n_signals];
    if (scratch) {
        if (!ctx) return GOOFER_EINVAL;
        if (!y || !cand_f || !cand_s || !cand_n) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null signal / candidates");
    }
    cand_scratch s;
    if ((rc = caller_scratch(ctx, scratch, scratch_bytes, "tracker", [&](arena &a) { s = carve_candidates(a, n_signals, g); })) || !scratch)
        return rc;
    hipStream_t st = (hipStream_t)stream;

    // Hann window of W samples and its own autocorrelation, normalised at lag 0
    std::vector<double> win(g.W), rw(g.hi + 1);
    for (int j = 0; j < g.W; ++j) win[j] = 0.5 - 0.5 * cos(2.0 * M_PI * (j + 1.0) / (g.W + 1.0));
    for (int t = 0; t <= g.hi; ++t) {
        double acc = 0.0;
        for (int j = 0; j < g.W - t; ++j) acc += win[j] * win[j + t];
        rw[t] = acc;
    }
    for (int t = g.hi; t >= 0; --t) rw[t] /= rw[0];
    HIP_TRY(ctx, hipMemcpyAsync(s.soff, sample_off, 8 * (size_t)(n_signals + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(s.foff, frame_off, 8 * (size_t)(n_signals + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(s.win, win.data(), 8 * (size_t)g.W, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(s.rw, rw.data(), 8 * (size_t)(g.hi + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                            // the host vectors go out of scope

    hipLaunchKernelGGL(k_pitch_stats, dim3(n_signals), dim3(TR_THREADS), 0, st, y, s.soff, s.stats);
    LAUNCH_CHECK(ctx);
    if (F > 0) {
        const size_t lds = pitch_lds(g);
        // the opt-in is for dynamic LDS: what the kernel's static arrays leave of a workgroup's 160 KiB
        if (lds > TR_LDS_OPT_IN && (rc = kernel_allow_max_lds(ctx, (const void *)k_pitch_frames, (int)(TR_LDS_MAX - PITCH_STATIC_LDS)))) return rc;
        hipLaunchKernelGGL(k_pitch_frames, dim3((unsigned)F), dim3(TR_THREADS), lds, st, y, s.soff, s.foff, n_signals, sr, hop, g,
                           ts.silence_threshold, ts.voicing_threshold, ts.octave_cost, s.win, s.rw, s.stats, cand_f, cand_s, cand_n);
        LAUNCH_CHECK(ctx);
    }
    return GOOFER_OK;
}

extern "C" int goofer_track_path(goofer_ctx *ctx, const double *cand_f, const double *cand_s, const int32_t *cand_n,
                                 const int64_t *frame_off, int n_signals, int sr, int hop, double *f0, void *scratch,
                                 int64_t *scratch_bytes, void *stream)
{
    int rc = check_offsets(ctx, frame_off, n_signals, sr, hop, "frame_off");
    if (rc) return rc;
    if (!scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null scratch_bytes");
    const int64_t F = frame_off[n_signals];
    if (scratch) {
        if (!ctx) return GOOFER_EINVAL;
        if (F == 0) return GOOFER_OK;
        if (!cand_f || !cand_s || !cand_n || !f0) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null candidates / f0");
    }
    path_scratch s;
    if ((rc = caller_scratch(ctx, scratch, scratch_bytes, "tracker", [&](arena &a) { s = carve_path(a, n_signals, F); })) || !scratch)
        return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, hipMemcpyAsync(s.foff, frame_off, 8 * (size_t)(n_signals + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                            // frame_off is the caller's host array
    const goofer_track_settings &ts = settings_of(ctx);
    hipLaunchKernelGGL(k_pitch_viterbi, dim3(n_signals), dim3(WAVE), 0, st, s.foff, cand_f, cand_s, cand_n, 0.01 * sr / hop,
                       ts.octave_jump_cost, ts.voiced_unvoiced_cost, s.back, f0);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

extern "C" int goofer_track_pitch(goofer_ctx *ctx, const double *y, const int64_t *sample_off, int n_signals, int sr, int hop,
                                  int64_t *frame_off, double *f0, void *scratch, int64_t *scratch_bytes, void *stream)
{
    if (!scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null frame_off / scratch_bytes");
    const goofer_track_settings ts = settings_of(ctx);
    int rc = check_batch(ctx, sample_off, n_signals, sr, hop, pitch_min_length(ts, sr));
    if (rc) return rc;
    if (!frame_off) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null frame_off / scratch_bytes");
    const pitch_geom g = pitch_geometry(ts, sr);
    if ((rc = check_pitch_lds(ctx, g, sr))) return rc;
    fill_offsets(sample_off, n_signals, frame_off, [&](int64_t n) { return pitch_frames(ts, n, sr, hop); });
    const int64_t F = frame_off[n_signals];
    if (scratch) {
        if (!ctx) return GOOFER_EINVAL;
        if (!y || !f0) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null signal / f0");
    }
    double *cand_f, *cand_s;
    int32_t *cand_n;
    size_t at_c, at_p, end;                                                            // the stages' blocks
    auto carve = [&](arena &a) {
        cand_f = a.take<double>(TR_MAX_CAND * (size_t)F);
        cand_s = a.take<double>(TR_MAX_CAND * (size_t)F);
        cand_n = a.take<int32_t>(F);
        at_c = a.used;
        carve_candidates(a, n_signals, g);
        at_p = a.used;
        carve_path(a, n_signals, F);
        end = a.used;
    };
    if ((rc = caller_scratch(ctx, scratch, scratch_bytes, "tracker", carve)) || !scratch) return rc;
    int64_t need_c = at_p - at_c, need_p = end - at_p;
    char *p = (char *)scratch;
    if ((rc = goofer_track_candidates(ctx, y, sample_off, n_signals, sr, hop, frame_off, cand_f, cand_s, cand_n, p + at_c, &need_c, stream))) return rc;
    return goofer_track_path(ctx, cand_f, cand_s, cand_n, frame_off, n_signals, sr, hop, f0, p + at_p, &need_p, stream);
}

extern "C" int goofer_track_resample(goofer_ctx *ctx, const double *y, const int64_t *sample_off, int n_signals, int sr, int64_t *x_off,
                                     double *x11, void *scratch, int64_t *scratch_bytes, void *stream)
{
    int rc = check_batch(ctx, sample_off, n_signals, sr, 1, 1);
    if (rc) return rc;
    if (!x_off || !scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null x_off / scratch_bytes");
    const formant_geom fg = formant_geometry(settings_of(ctx));
    fill_offsets(sample_off, n_signals, x_off, [&](int64_t n) { return resampled_length(fg, n, sr); });
    const int64_t M = x_off[n_signals];
    if (scratch) {
        if (!ctx) return GOOFER_EINVAL;
        if (M == 0) return GOOFER_OK;                                                  // every signal shorter than one output sample
        if (!y || !x11) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null signal / x11");
    }
    resample_scratch s;
    if ((rc = caller_scratch(ctx, scratch, scratch_bytes, "tracker", [&](arena &a) { s = carve_resample(a, n_signals); })) || !scratch)
        return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, hipMemcpyAsync(s.soff, sample_off, 8 * (size_t)(n_signals + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(s.moff, x_off, 8 * (size_t)(n_signals + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                            // the offsets are the caller's host arrays
    hipLaunchKernelGGL(fg.fsr == FM_SR ? k_resample<FM_SR> : k_resample<0>, dim3((unsigned)((M + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, st, y, s.soff, s.moff,
                       n_signals, M, sr, fg.fsr, x11);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

extern "C" int goofer_track_formant_frames(goofer_ctx *ctx, const double *x11, const int64_t *x_off, int n_signals, int sr, int hop,
                                           int64_t *frame_off, double *formants, void *scratch, int64_t *scratch_bytes, void *stream)
{
    int rc = check_offsets(ctx, x_off, n_signals, sr, hop, "x_off");
    if (rc) return rc;
    if (!frame_off || !scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null frame_off / scratch_bytes");
    const formant_geom fg = formant_geometry(settings_of(ctx));
    fill_offsets(x_off, n_signals, frame_off, [&](int64_t m) { return formant_frames(fg, m, sr, hop); });
    const int64_t F = frame_off[n_signals];
    if (scratch) {
        if (!ctx) return GOOFER_EINVAL;
        if (F == 0) return GOOFER_OK;                                                  // every signal shorter than a formant window
        if (!x11 || !formants) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null x11 / formants");
    }
    formant_scratch s;
    if ((rc = caller_scratch(ctx, scratch, scratch_bytes, "tracker", [&](arena &a) { s = carve_formant_frames(a, n_signals, fg); })) || !scratch)
        return rc;
    const formant_kernel kernel = formant_kernel_of(fg);
    if (!kernel) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: no formant kernel for a window of %d samples and order %d", fg.win, fg.order);
    hipStream_t st = (hipStream_t)stream;

    // Praat's Gaussian-like window: exp(-48 (i - mid)^2 / (W + 1)^2), i = 1..W, lifted to zero at the ends
    std::vector<double> gwin(fg.win);
    const double e12 = exp(-12.0);
    for (int j = 0; j < fg.win; ++j) {
        const double d = (j + 1.0) - 0.5 * (fg.win + 1);
        gwin[j] = (exp(-48.0 * d * d / ((fg.win + 1.0) * (fg.win + 1.0))) - e12) / (1.0 - e12);
    }
    HIP_TRY(ctx, hipMemcpyAsync(s.moff, x_off, 8 * (size_t)(n_signals + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(s.foff, frame_off, 8 * (size_t)(n_signals + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(s.gwin, gwin.data(), 8 * (size_t)fg.win, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                            // the host vectors go out of scope
    hipLaunchKernelGGL(kernel, dim3((unsigned)F), dim3(WAVE), 0, st, x11, s.moff, s.foff, n_signals, sr, hop, fg.fsr, fg.win,
                       exp(-2.0 * M_PI * FM_PRE_HZ / fg.fsr), s.gwin, formants);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

extern "C" int goofer_track_formants(goofer_ctx *ctx, const double *y, const int64_t *sample_off, int n_signals, int sr, int hop,
                                     int64_t *frame_off, double *formants, void *scratch, int64_t *scratch_bytes, void *stream)
{
    int rc = check_batch(ctx, sample_off, n_signals, sr, hop, 1);
    if (rc) return rc;
    if (!frame_off || !scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null frame_off / scratch_bytes");
    const formant_geom fg = formant_geometry(settings_of(ctx));
    std::vector<int64_t> x_off(n_signals + 1);
    fill_offsets(sample_off, n_signals, x_off.data(), [&](int64_t n) { return resampled_length(fg, n, sr); });
    fill_offsets(x_off.data(), n_signals, frame_off, [&](int64_t m) { return formant_frames(fg, m, sr, hop); });
    const int64_t F = frame_off[n_signals], M = x_off[n_signals];
    if (scratch) {
        if (!ctx) return GOOFER_EINVAL;
        if (F == 0) return GOOFER_OK;                                                  // every signal shorter than a formant window
        if (!y || !formants) return goofer_fail(ctx, GOOFER_EINVAL, "tracker: null signal / formants");
    }
    double *x11;
    size_t at_r, at_f, end;                                                            // the stages' blocks
    auto carve = [&](arena &a) {
        x11 = a.take<double>(M);
        at_r = a.used;
        carve_resample(a, n_signals);
        at_f = a.used;
        carve_formant_frames(a, n_signals, fg);
        end = a.used;
    };
    if ((rc = caller_scratch(ctx, scratch, scratch_bytes, "tracker", carve)) || !scratch) return rc;
    int64_t need_r = at_f - at_r, need_f = end - at_f;
    char *p = (char *)scratch;
    if ((rc = goofer_track_resample(ctx, y, sample_off, n_signals, sr, x_off.data(), x11, p + at_r, &need_r, stream))) return rc;
    return goofer_track_formant_frames(ctx, x11, x_off.data(), n_signals, sr, hop, frame_off, formants, p + at_f, &need_f, stream);
}
