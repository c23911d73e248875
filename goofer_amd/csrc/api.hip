// C ABI of libgoofer_hip.so: handle lifetime, per-(sr, n_fft, hop) tables, options, counters, the profiler and the entry points
// that validate their arguments and call one launcher.  The batch driver (goofer_synth_batch and company) is synth.hip.
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "launchers.h"

int goofer_fail(goofer_ctx *ctx, int code, const char *fmt, ...)
{
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

static goofer_ctx::kernel_state *kstate_of(goofer_ctx *ctx, const void *fn)
{
    for (int i = 0; i < ctx->n_kstate; ++i)
        if (ctx->kstate[i].fn == fn) return &ctx->kstate[i];
    if (ctx->n_kstate >= 32) return nullptr;
    goofer_ctx::kernel_state *k = &ctx->kstate[ctx->n_kstate++];
    *k = {fn, 0, 0, false};
    return k;
}

int kernel_allow_max_lds(goofer_ctx *ctx, const void *fn, int bytes)
{
    goofer_ctx::kernel_state *k = kstate_of(ctx, fn);
    if (k && k->max_lds_set) return GOOFER_OK;
    HIP_TRY(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (k) k->max_lds_set = true;
    return GOOFER_OK;
}

int kernel_resident_waves(goofer_ctx *ctx, const void *fn, size_t lds, int *waves)
{
    goofer_ctx::kernel_state *k = kstate_of(ctx, fn);
    if (k && k->waves > 0 && k->lds == lds) {
        *waves = k->waves;
        return GOOFER_OK;
    }
    int cus = 0, per_cu = 0;
    HIP_TRY(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds));
    *waves = (cus > 0 ? cus : 256) * (per_cu > 0 ? per_cu : 1) * 4;
    if (k) { k->waves = *waves; k->lds = lds; }
    return GOOFER_OK;
}

// A handle-owned device block (*p, *bytes) grown to `need` bytes when it is smaller: the device is drained first (work in
// flight may still read the old block), then the block is freed and allocated anew.
int grow_block(goofer_ctx *ctx, void **p, size_t *bytes, size_t need, const char *what)
{
    if (*bytes >= need) return GOOFER_OK;
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (*p) HIP_TRY(ctx, hipFree(*p));
    *p = nullptr;
    *bytes = 0;
    hipError_t e = hipMalloc(p, need);
    if (e != hipSuccess) return goofer_fail(ctx, GOOFER_ENOMEM, "%s hipMalloc(%zu) failed: %s", what, need, hipGetErrorString(e));
    *bytes = need;
    return GOOFER_OK;
}

// taps of a sample-axis Gaussian, uploaded into jitter slot `slot` of the handle's small block: radius <= 8000, i.e. a jitter speed
// down to sr / 12 000 Hz (3.7 Hz at 44.1 kHz; the reference's defaults are 100 and 150 Hz.  Until round 6: radius <= 1000 =
// 29.4 Hz, which a random keyword set hit)
int upload_jitter_taps(goofer_ctx *ctx, double sigma, int slot, const double **d_taps, int *radius, hipStream_t st)
{
    std::vector<double> taps;
    int r;
    gauss_taps_host(sigma, taps, r);
    if (r > 8000) return goofer_fail(ctx, GOOFER_EINVAL, "jitter sigma %g too large", sigma);
    int rc = grow_block(ctx, &ctx->small, &ctx->small_bytes, SMALL_RAGGED, "small block");
    if (rc) return rc;
    double *dst = (double *)((char *)ctx->small + SMALL_JIT + (size_t)slot * JIT_SLOT_BYTES);
    HIP_TRY(ctx, hipMemcpyAsync(dst, taps.data(), taps.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *d_taps = dst;
    *radius = r;
    return GOOFER_OK;
}

// ---------------------------------------------------------------------------------------------
// host-side table construction (fp64 then rounded exactly where numpy rounds)
void gauss_taps_host(double sigma, std::vector<double> &taps, int &radius)
{
    radius = (int)(4.0 * sigma + 0.5);          // GOOFER.py:247
    taps.assign(2 * radius + 1, 0.0);
    double sum = 0.0;
    for (int t = -radius; t <= radius; ++t) {
        double q = (double)t / sigma;
        taps[t + radius] = exp(-0.5 * (q * q));
        sum += taps[t + radius];
    }
    for (auto &v : taps) v /= sum;
}

static void ramp_gain_host(int n_bins, double sr, double lo, double hi, double db, std::vector<float> &out)
{
    std::vector<double> f(n_bins), g(n_bins, 1.0);
    double step = (sr / 2.0) / (double)(n_bins - 1);
    for (int i = 0; i < n_bins; ++i) f[i] = (double)i * step;
    f[n_bins - 1] = sr / 2.0;
    int a = (int)(std::lower_bound(f.begin(), f.end(), lo) - f.begin());
    int b = (int)(std::lower_bound(f.begin(), f.end(), hi) - f.begin());
    double top = pow(10.0, db / 20.0);
    int m = b - a;
    for (int i = 0; i < m; ++i) {
        double rise = m > 1 ? (i == m - 1 ? 1.0 : (double)i * (1.0 / (double)(m - 1))) : 0.0;
        g[a + i] = 1.0 + rise * (top - 1.0);
    }
    for (int i = b; i < n_bins; ++i) g[i] = top;
    out.resize(n_bins);
    for (int i = 0; i < n_bins; ++i) out[i] = (float)g[i];
}

template <typename T> static int upload(goofer_ctx *ctx, T **dst, const std::vector<T> &src)
{
    if (*dst) HIP_TRY(ctx, hipFree(*dst));
    *dst = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)dst, src.size() * sizeof(T)));
    HIP_TRY(ctx, hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return GOOFER_OK;
}

static void free_plan(goofer_plan_t &p)
{
    void *ptrs[] = {p.window, p.window_blur, p.blur_edge, p.win_sq, p.freqs, p.lin_freqs, p.boost, p.bright_h, p.bright_b, p.tw_full, p.tw_half, p.pulse_peak, p.pulse_shape, p.blur5, p.blur175,
                    p.bl_chirp, p.bl_bhat, p.bl_tw, p.bl_twh};
    for (void *q : ptrs)
        if (q) (void)hipFree(q);
    p = goofer_plan_t();
}

// An event pool of the profiler (common.h) grown to `steps` steps: the events it holds are destroyed and made anew.
static void pool_destroy(event_pool &p)
{
    for (int i = 0; i < p.steps * p.per_step; ++i)
        if (p.ev[i]) (void)hipEventDestroy(p.ev[i]);
    free(p.ev);
    p.ev = nullptr;
    p.steps = 0;
}

static int pool_grow(goofer_ctx *ctx, event_pool &p, int steps)
{
    if (p.steps >= steps) return GOOFER_OK;
    pool_destroy(p);
    p.ev = (hipEvent_t *)calloc((size_t)steps * p.per_step, sizeof(hipEvent_t));
    if (!p.ev) return goofer_fail(ctx, GOOFER_ENOMEM, "event pool");
    p.steps = steps;                                          // (a failed create leaves null events behind: pool_destroy skips them)
    for (int i = 0; i < steps * p.per_step; ++i) HIP_TRY(ctx, hipEventCreate(&p.ev[i]));
    return GOOFER_OK;
}

// ---------------------------------------------------------------------------------------------
extern "C" {

const char *goofer_version(void) { return "goofer_hip 0.1 (gfx950)"; }

int goofer_create(int device_id, goofer_ctx **out)
{
    if (!out) return GOOFER_EINVAL;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count) return GOOFER_EHIP;
    if (hipSetDevice(device_id) != hipSuccess) return GOOFER_EHIP;
    goofer_ctx *c = new goofer_ctx();
    c->device = device_id;
    // the onset-overflow word lives as long as the handle (never inside the re-carved, re-allocated scratch arena)
    if (hipMalloc((void **)&c->ovf_flag, OVF_WORDS * sizeof(int32_t)) != hipSuccess || hipMemset(c->ovf_flag, 0, OVF_WORDS * sizeof(int32_t)) != hipSuccess) {
        delete c;
        return GOOFER_EHIP;
    }
    *out = c;
    return GOOFER_OK;
}

void goofer_destroy(goofer_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    free_plan(ctx->plan);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->small) (void)hipFree(ctx->small);
    if (ctx->asm_scratch) (void)hipFree(ctx->asm_scratch);
    if (ctx->mask_taps) (void)hipFree(ctx->mask_taps);
    if (ctx->warp_rows) (void)hipFree(ctx->warp_rows);
    if (ctx->ovf_flag) (void)hipFree(ctx->ovf_flag);
    for (event_pool *q : {&ctx->prof_ev, &ctx->prof_asm, &ctx->prof_side, &ctx->prof_main2}) pool_destroy(*q);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->ev_maps) (void)hipEventDestroy(ctx->ev_maps);
    if (ctx->ev_entry) (void)hipEventDestroy(ctx->ev_entry);
    if (ctx->ev_f0) (void)hipEventDestroy(ctx->ev_f0);
    if (ctx->ev_f0s) (void)hipEventDestroy(ctx->ev_f0s);
    if (ctx->side) (void)hipStreamDestroy(ctx->side);
    delete ctx;
}

const char *goofer_last_error(const goofer_ctx *ctx) { return ctx ? ctx->err : "null context"; }

int goofer_plan(goofer_ctx *ctx, int sr, int n_fft, int hop)
{
    if (!ctx) return GOOFER_EINVAL;
    // (above 2048 the frame is shared by a workgroup: 4096 natively, the other even sizes through Bluestein at L = 4096).
    // 2050 stays refused, as it was when the range ended at 2048: the test suite pins that refusal, and lifting it is a change
    // of existing behaviour of its own.
    const bool native = n_fft == 512 || n_fft == 768 || n_fft == 1024 || n_fft == 1536 || n_fft == 2048 || n_fft == 4096;
    if (!native && (n_fft < 64 || n_fft > 4096 || (n_fft & 1) || n_fft == 2050))
        return goofer_fail(ctx, GOOFER_EINVAL, "n_fft must be an even number in [64, 4096] other than 2050 (got %d)", n_fft);
    if (hop <= 0 || hop > n_fft || sr <= 0) return goofer_fail(ctx, GOOFER_EINVAL, "bad sr/hop (%d, %d)", sr, hop);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    free_plan(ctx->plan);
    goofer_plan_t &p = ctx->plan;
    const int B = n_fft / 2 + 1, M = n_fft / 2;
    const double PI = 3.14159265358979323846;

    std::vector<float> win(n_fft), wsq(n_fft), freqs(B), boost(B), bh, bb;
    for (int i = 0; i < n_fft; ++i) {
        // np.hanning: 0.5 + 0.5 cos(pi n/(M-1)), n = 1-M, 3-M, ...   -> fp32 -> sqrt (numpy's ** 0.5)
        double n = (double)(1 - n_fft + 2 * i);
        float h = (float)(0.5 + 0.5 * cos(PI * n / (double)(n_fft - 1)));
        win[i] = sqrtf(h);
        wsq[i] = win[i] * win[i];
    }
    {
        double val = 1.0 / ((double)n_fft * (1.0 / (double)sr));   // np.fft.rfftfreq
        for (int k = 0; k < B; ++k) freqs[k] = (float)((double)k * val);
        double step = 99.0 / (double)(B - 1);                      // np.linspace(1, 100, B)
        for (int k = 0; k < B; ++k) boost[k] = (float)((double)k * step + 1.0);
        boost[B - 1] = 100.0f;
    }
    ramp_gain_host(B, (double)sr, 2000.0, 3500.0, 3.0, bh);
    ramp_gain_host(B, (double)sr, 3500.0, 5000.0, 20.0, bb);
    std::vector<float2> twf(M), twh(M / 2 + 1);
    for (int k = 0; k < M; ++k) twf[k] = make_float2((float)cos(-2.0 * PI * k / M), (float)sin(-2.0 * PI * k / M));
    for (int k = 0; k <= M / 2; ++k) twh[k] = make_float2((float)cos(-PI * k / M), (float)sin(-PI * k / M));
    std::vector<double> t5, t175;
    int r5, r175;
    gauss_taps_host(0.5, t5, r5);
    gauss_taps_host(1.75, t175, r175);

    // Time-domain image of the sigma-0.5 bin blur (GOOFER.py:1143, 1171).  A circular convolution of a frame's spectrum with
    // the symmetric taps t is a multiplication of its samples by W[n] = t2 + 2 t1 cos(2 pi n / N) + 2 t0 cos(4 pi n / N); the
    // stem walkers fold W into the synthesis window of the frames that get the blur (stems.hip).
    std::vector<float> winb(n_fft);
    for (int i = 0; i < n_fft; ++i) {
        const double a = 2.0 * PI * (double)i / (double)n_fft;
        winb[i] = (float)((double)win[i] * (t5[2] + 2.0 * t5[1] * cos(a) + 2.0 * t5[0] * cos(2.0 * a)));
    }
    // ... circularly, i.e. over the spectrum's own Hermitian continuation past DC and Nyquist, where the reference's
    // gaussian_filter1d reflects the array.  The two differ by a purely imaginary E on four bins (E_1 = i (2 t0 Im X_1 + t1 Im X_0),
    // E_2 = i t0 Im X_0, and the mirror image below Nyquist); adding D with blur(D) = E to the spectrum in front of the transform
    // makes the product form the reflected blur.  On imaginary, odd-continued sequences the blur is the matrix T below; its
    // inverse decays like 0.135^k, six bins carry it to 6e-6 of E.  c1 / c2 = the first two columns of T^-1, stored per lane of
    // the walkers' bin layout (bin k = lane + 64 i): rows 0, 1 for bins 1..6 (slot 0), rows 2, 3 for bins M-6..M-1 (last slot).
    std::vector<float> edge(4 * 64, 0.f);
    {
        const int K = 6;
        double T[6][12] = {{0}};
        for (int k = 1; k <= K; ++k) {
            const int dd[5] = {-2, -1, 0, 1, 2};
            for (int q = 0; q < 5; ++q) {
                int j = k + dd[q];
                double sg = 1.0;
                if (j == 0) continue;                          // Im D_0 = 0
                if (j < 0) { j = -j; sg = -1.0; }              // odd continuation
                if (j <= K) T[k - 1][j - 1] += sg * t5[q];
            }
            T[k - 1][K + k - 1] = 1.0;                          // [T | I] -> Gauss-Jordan
        }
        for (int c = 0; c < K; ++c) {
            int piv = c;
            for (int r = c + 1; r < K; ++r)
                if (fabs(T[r][c]) > fabs(T[piv][c])) piv = r;
            for (int j = 0; j < 2 * K; ++j) std::swap(T[c][j], T[piv][j]);
            const double d = T[c][c];
            for (int j = 0; j < 2 * K; ++j) T[c][j] /= d;
            for (int r = 0; r < K; ++r) {
                if (r == c) continue;
                const double f = T[r][c];
                for (int j = 0; j < 2 * K; ++j) T[r][j] -= f * T[c][j];
            }
        }
        for (int j = 1; j <= K; ++j) {
            edge[0 * 64 + j] = (float)T[j - 1][K + 0];           // c1_j at lane j (bin j)
            edge[1 * 64 + j] = (float)T[j - 1][K + 1];           // c2_j
            edge[2 * 64 + (64 - j)] = (float)T[j - 1][K + 0];    // bin M - j sits in lane 64 - j of the last slot
            edge[3 * 64 + (64 - j)] = (float)T[j - 1][K + 1];
        }
    }
    int rc;
    if (!native) {
        // Bluestein: X[k] = conj(c_k) sum_n (x_n conj(c_n)) c_{k-n}, c_n = exp(i pi n^2 / M): a circular convolution of length
        // L >= 2 M - 1 with the wrapped chirp, whose transform is made here in fp64 (n^2 mod 2 M keeps the phases exact)
        int L = 256;
        while (L < 2 * M - 1) L *= 2;
        std::vector<float2> chirp(M), bhat(L), twl(L), twhf(M + 1);
        std::vector<double> br(L, 0.0), bi(L, 0.0);
        for (int k = 0; k < M; ++k) {
            const long long q = ((long long)k * k) % (2LL * M);
            const double ang = PI * (double)q / (double)M;
            chirp[k] = make_float2((float)cos(ang), (float)sin(ang));
            br[k] = cos(ang); bi[k] = sin(ang);
            if (k) { br[L - k] = cos(ang); bi[L - k] = sin(ang); }
        }
        std::vector<double> cr(L), ci(L);
        for (int k = 0; k < L; ++k) { cr[k] = cos(-2.0 * PI * k / L); ci[k] = sin(-2.0 * PI * k / L); twl[k] = make_float2((float)cr[k], (float)ci[k]); }
        for (int k = 0; k < L; ++k) {
            double sr_ = 0.0, si_ = 0.0;
            for (int j = 0; j < L; ++j) {
                if (br[j] == 0.0 && bi[j] == 0.0) continue;
                const int t = (int)(((long long)k * j) & (L - 1));
                sr_ += br[j] * cr[t] - bi[j] * ci[t];
                si_ += br[j] * ci[t] + bi[j] * cr[t];
            }
            bhat[k] = make_float2((float)sr_, (float)si_);
        }
        for (int k = 0; k <= M; ++k) twhf[k] = make_float2((float)cos(-PI * k / M), (float)sin(-PI * k / M));
        if ((rc = upload(ctx, &p.bl_chirp, chirp))) return rc;
        if ((rc = upload(ctx, &p.bl_bhat, bhat))) return rc;
        if ((rc = upload(ctx, &p.bl_tw, twl))) return rc;
        if ((rc = upload(ctx, &p.bl_twh, twhf))) return rc;
        p.bl_L = L;
    }
    if ((rc = upload(ctx, &p.blur_edge, edge))) return rc;
    if ((rc = upload(ctx, &p.window_blur, winb))) return rc;
    if ((rc = upload(ctx, &p.window, win))) return rc;
    if ((rc = upload(ctx, &p.win_sq, wsq))) return rc;
    if ((rc = upload(ctx, &p.freqs, freqs))) return rc;
    {
        std::vector<float> lin(B);
        const double fstep = ((double)sr / 2.0) / (double)(B - 1);
        for (int k = 0; k < B; ++k) lin[k] = (float)(k >= B - 1 ? (double)sr / 2.0 : (double)k * fstep);
        if ((rc = upload(ctx, &p.lin_freqs, lin))) return rc;
    }
    if ((rc = upload(ctx, &p.boost, boost))) return rc;
    if ((rc = upload(ctx, &p.bright_h, bh))) return rc;
    if ((rc = upload(ctx, &p.bright_b, bb))) return rc;
    if ((rc = upload(ctx, &p.tw_full, twf))) return rc;
    if ((rc = upload(ctx, &p.tw_half, twh))) return rc;
    if ((rc = upload(ctx, &p.blur5, t5))) return rc;
    if ((rc = upload(ctx, &p.blur175, t175))) return rc;
    for (int j = 0; j < 5; ++j) p.taps5_f[j] = (float)t5[j];
    for (int j = 0; j < 15; ++j) p.taps175_f[j] = (float)t175[j];
    HIP_TRY(ctx, hipMalloc((void **)&p.pulse_peak, PULSE_PEAK_FLOATS * sizeof(float)));
    p.sr = sr; p.n_fft = n_fft; p.hop = hop; p.n_bins = B;
    if ((rc = launch_pulse_peak(ctx, p.pulse_peak, (double)sr, 0))) return rc;
    HIP_TRY(ctx, hipMalloc((void **)&p.pulse_shape, pulse_shape_table_floats() * sizeof(float)));
    if ((rc = launch_pulse_shape_table(ctx, p.pulse_shape, p.pulse_peak, (double)sr, 0))) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return GOOFER_OK;
}

int goofer_pulse_model(goofer_ctx *ctx, double Ra, double Rg, double Rk)
{
    if (!ctx) return GOOFER_EINVAL;
    goofer_plan_t &p = ctx->plan;
    if (!p.pulse_peak || !p.pulse_shape) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_pulse_model needs a plan (goofer_plan)");
    if (!std::isfinite(Ra) || !std::isfinite(Rg) || !std::isfinite(Rk))
        return goofer_fail(ctx, GOOFER_EINVAL, "Ra, Rg, Rk must be finite (got %g, %g, %g)", Ra, Rg, Rk);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());                     // nothing in flight still reads the tables
    p.lf.ra = Ra; p.lf.rg = Rg; p.lf.rk = Rk;
    int rc;
    if ((rc = launch_pulse_peak(ctx, p.pulse_peak, (double)p.sr, 0))) return rc;
    if ((rc = launch_pulse_shape_table(ctx, p.pulse_shape, p.pulse_peak, (double)p.sr, 0))) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return GOOFER_OK;
}

// copy one plan table to host memory (tests / debugging); which: 0 window 1 freqs 2 boost 3 bright_h
// 4 bright_b 5 pulse_peak; returns the element count or a negative error
int goofer_debug_table(goofer_ctx *ctx, int which, float *host_out, int capacity)
{
    if (!ctx || !ctx->plan.n_fft) return GOOFER_ENOPLAN;
    const goofer_plan_t &p = ctx->plan;
    const float *src[] = {p.window, p.freqs, p.boost, p.bright_h, p.bright_b, p.pulse_peak};
    const int cnt[] = {p.n_fft, p.n_bins, p.n_bins, p.n_bins, p.n_bins, 8193};
    if (which < 0 || which > 5) return GOOFER_EINVAL;
    int n = std::min(cnt[which], capacity);
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(host_out, src[which], n * sizeof(float), hipMemcpyDeviceToHost));
    return cnt[which];
}

/* Host helper of the note planner (goofer_amd/sampler.py, SillySampler.py:264-283): Gaussian FIR along the rows of a small
 * fp64 matrix with numpy 'reflect' padding, accumulated tap by tap in ascending order (product rounded, then added: the
 * arithmetic of the planner's numpy loop, so the tracks are the same bits either way).  Pure CPU code: no device is touched. */
int goofer_host_gauss_rows(const double *x, int64_t rows, int T, const double *taps, int radius, double *out)
{
    if (!x || !taps || !out || rows < 0 || T <= 0 || radius < 0) return GOOFER_EINVAL;
    const int nt = 2 * radius + 1;
    std::vector<int> idx((size_t)T + 2 * radius);
    const int period = T > 1 ? 2 * (T - 1) : 1;
    for (int q = -radius; q < T + radius; ++q) {              // numpy 'reflect' as a periodic map (T == 1: 'edge')
        int m = T > 1 ? ((q % period) + period) % period : 0;
        idx[q + radius] = m < T ? m : period - m;
    }
    std::vector<double> pad((size_t)T + 2 * radius);
    for (int64_t r = 0; r < rows; ++r) {
        const double *xr = x + r * T;
        double *o = out + r * T;
        for (int q = 0; q < T + 2 * radius; ++q) pad[q] = xr[idx[q]];
        const double *pp = pad.data();
        for (int t = 0; t < T; ++t) o[t] = taps[0] * pp[t];
        for (int j = 1; j < nt; ++j) {                       // tap-outer: every o[t] still sums its taps in ascending order
            const double kj = taps[j];
            for (int t = 0; t < T; ++t) {
                const double prod = kj * pp[t + j];
                o[t] = o[t] + prod;
            }
        }
    }
    return GOOFER_OK;
}

/* Synchronise the device and report what the asynchronous batch calls could not: a note whose pulse onsets did not fit its
 * onset slots (n / 2 + 16 per note — more than one pulse per two samples; the onsets beyond were dropped.  The 'sg' layer's
 * trackers fire at most once per sample into n + 16 slots per note, the layout such a batch leaves behind).  The flag is a
 * handle-owned word every pulse-chain launch (goofer_pulse_train, goofer_synth_batch / goofer_render_batch incl. the extra
 * synthesis calls of the post chain) raises with atomicMax; it stays up until this call reads and clears it.  Word LEGACY_FLAG
 * beside it is goofer_legacy_normal_fill's: a note that ran into the bound of its block loop. */
int goofer_check(goofer_ctx *ctx)
{
    if (!ctx) return GOOFER_EINVAL;
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (!ctx->ovf_flag) return GOOFER_OK;
    int32_t w[LEGACY_FLAG + 1] = {0};
    HIP_TRY(ctx, hipMemcpy(w, ctx->ovf_flag, sizeof(w), hipMemcpyDeviceToHost));
    if (w[LEGACY_FLAG] != 0) {                                       // goofer_legacy_normal_fill: a note ran into its block bound
        HIP_TRY(ctx, hipMemset(ctx->ovf_flag + LEGACY_FLAG, 0, sizeof(int32_t)));   // reported once
        return goofer_fail(ctx, GOOFER_EINVAL, "note %d of a legacy normal fill since the last check did not get its normals within "
                           "its block bound: its outputs are incomplete", w[LEGACY_FLAG] - 1);
    }
    const int32_t v = w[0];
    if (v != 0) {
        HIP_TRY(ctx, hipMemset(ctx->ovf_flag, 0, sizeof(v)));        // reported once
        return goofer_fail(ctx, GOOFER_EINVAL, "note %d of a batch since the last check has more pulse onsets than n / 2 + 16 (f0 above "
                           "sr / 2?): the pulses beyond its onset slots were dropped (the 'sg' layer's trackers have n + 16)", v - 1);
    }
    return GOOFER_OK;
}

/* Cumulative counters of the handle (device words beside the overflow flag; the call synchronises the device):
 *   "pulse_scanned_notes"   notes whose onsets went through the parallel phase scan (k_pulse_note, or k_pulse_onsets_par with option pulse_fused = 0)
 *   "pulse_fallback_notes"  ... of which were walked sequentially afterwards (a sample within the error band of an integer
 *                           phase, a negative / non-finite increment, or option pulse_scan = 2)
 *   "pulse_list_notes"      notes k_pulse_note placed from the onset list in global memory and not from its LDS ring (the walked
 *                           ones, and those with more than 2048 onsets live at once)
 *   "mask_flag_segments"    note segments of k_mask_short's tiles (goofer_synth_batch / goofer_render_batch) answered from the
 *                           f0 kernel's tile flags alone
 *   "mask_staged_segments"  ... that staged their mask window in LDS (every segment when there are no flags; the large-radius
 *                           loop counts nothing)
 * and, host-side ints of the handle (no device word is read): the frames per wave the LAST launch of a frame walker was given,
 *   "walk_run_noise" k_noise_stems   "walk_run_harm" k_harm_stem   "walk_run_ola3" k_irfft_ola3   "walk_run_ola1" k_irfft_ola1
 * (0: not launched on this handle yet; option "walk_run", walk_run_choice in launchers.h) */
int goofer_counter(goofer_ctx *ctx, const char *name, int64_t *value)
{
    if (!ctx || !name || !value) return GOOFER_EINVAL;
    int which = !strcmp(name, "pulse_fallback_notes") ? 1 : (!strcmp(name, "pulse_scanned_notes") ? 2 : (!strcmp(name, "pulse_list_notes") ? PULSE_LIST_COUNTER : -1));
    const int mask_c = !strcmp(name, "mask_flag_segments") ? 0 : (!strcmp(name, "mask_staged_segments") ? 1 : -1);
    static const char *const walk_names[4] = {"walk_run_noise", "walk_run_harm", "walk_run_ola3", "walk_run_ola1"};
    int walk = -1;
    for (int k = 0; k < 4; ++k)
        if (!strcmp(name, walk_names[k])) walk = k;
    if (which < 0 && mask_c < 0 && walk < 0) return goofer_fail(ctx, GOOFER_EINVAL, "unknown counter %s", name);
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (walk >= 0) {
        *value = ctx->walk_run_used[walk];
        return GOOFER_OK;
    }
    if (mask_c >= 0) {                                        // the sum of the counter's slots
        static_assert(OVF_WORDS <= 8192, "goofer_counter reads the words through a stack buffer");
        int32_t w[OVF_WORDS];
        HIP_TRY(ctx, hipMemcpy(w, ctx->ovf_flag, sizeof(w), hipMemcpyDeviceToHost));
        int64_t sum = 0;
        for (int sl = 0; sl < MASK_COUNTER_SLOTS; ++sl) sum += (int64_t)(uint32_t)w[MASK_COUNTERS + (2 * sl + mask_c) * MASK_COUNTER_STRIDE];
        *value = sum;
        return GOOFER_OK;
    }
    int32_t v = 0;
    HIP_TRY(ctx, hipMemcpy(&v, ctx->ovf_flag + which, sizeof(v), hipMemcpyDeviceToHost));
    *value = (int64_t)(uint32_t)v;
    return GOOFER_OK;
}

// copy intermediate `which` of the last goofer_synth_batch to host memory (tests / debugging):
// 0 frame_note 1 row_src 2 f0_scaled 3 pulse 4 S_harm 5 S_uv 6 S_breath 7 frames(last stem) 8 env_harm
// 9 env_noise 10 mask_short 11 note_mag 12 note_peak 13 onset_cnt 14 onset_idx (13, 14: also of the last goofer_pulse_train)
// 15 frame_skip (the spectra-in-HBM pipeline with per-frame skipping: one byte per frame).
// onset_idx holds every onset slot: note k's onsets start at sample_off[k] / 2 + 16 k — after a batch with the 'sg' layer at
// sample_off[k] + 16 k, where k_pulse_onsets_wrap left the sub-harmonic onsets of the last ratio (onset_cnt: their counts).
// Returns the byte size.
int64_t goofer_debug_fetch(goofer_ctx *ctx, int which, void *host_out, int64_t capacity_bytes)
{
    if (!ctx || which < 0 || which >= 17 || !ctx->dbg_ptr[which]) return GOOFER_EINVAL;
    if (int rc = goofer_check(ctx)) return rc;
    size_t nb = ctx->dbg_bytes[which] < (size_t)capacity_bytes ? ctx->dbg_bytes[which] : (size_t)capacity_bytes;
    if (hipMemcpy(host_out, ctx->dbg_ptr[which], nb, hipMemcpyDeviceToHost) != hipSuccess) return GOOFER_EHIP;
    return (int64_t)ctx->dbg_bytes[which];
}

static const char *const PROF_NAMES[PROF_STAGES] = {
    "setup_maps", "", "", "phase_inc", "pulse_onsets", "pulse_place", "rfft_frames", "harm_shape",
    "irfft_harm", "noise_spectra", "irfft_breath", "irfft_unvoiced", "mask_short", "ola3_gains", "apply_gain", "env_edit", "env_rows", "sample_assemble"};

// Per-stage timing of goofer_synth_batch with HIP events recorded on the caller's stream (so the
// numbers are what that stream really executed).  begin(max_steps) arms it; every synth batch then
// records PROF_STAGES+1 events; end() synchronises and returns the summed milliseconds per stage.
int goofer_profile_begin(goofer_ctx *ctx, int max_steps)
{
    if (!ctx || max_steps <= 0) return GOOFER_EINVAL;
    if (ctx->prof_cap < max_steps) {
        ctx->prof_cap = 0;
        for (event_pool *q : {&ctx->prof_asm, &ctx->prof_ev, &ctx->prof_side, &ctx->prof_main2})
            if (int rc = pool_grow(ctx, *q, max_steps)) return rc;
        ctx->prof_cap = max_steps;
    }
    ctx->prof_steps = 0;
    ctx->prof_asm_steps = 0;
    ctx->prof_on = true;
    return GOOFER_OK;
}

int goofer_profile_end(goofer_ctx *ctx, double *ms_per_stage, int n_stages)
{
    if (!ctx) return GOOFER_EINVAL;
    ctx->prof_on = false;
    HIP_TRY(ctx, hipDeviceSynchronize());
    for (int s = 0; s < n_stages && s < PROF_STAGES; ++s) {
        double acc = 0.0;
        if (ctx->prof_only >= 0 && s != ctx->prof_only) {                // (its events were not recorded)
            ms_per_stage[s] = 0.0;
            continue;
        }
        if (s >= PROF_ASM0) {
            // the assembly's three large kernels (goofer_assemble_batch / goofer_render_batch), each bracketed on the stream it ran on
            for (int k = 0; k < ctx->prof_asm_steps; ++k) {
                hipEvent_t *q = ctx->prof_asm.step(k) + 2 * (s - PROF_ASM0);
                float ms = 0.f;
                if (ctx->prof_asm_mask[k] & (1u << (s - PROF_ASM0))) HIP_TRY(ctx, hipEventElapsedTime(&ms, q[0], q[1]));
                acc += ms;
            }
            ms_per_stage[s] = acc;
            continue;
        }
        for (int k = 0; k < ctx->prof_steps; ++k) {
            hipEvent_t *e = ctx->prof_ev.step(k);
            float ms = 0.f;
            if (ctx->prof_side_used && s >= 3 && s <= 5) {              // the pulse chain ran on the side stream
                hipEvent_t *q = ctx->prof_side.step(k);
                HIP_TRY(ctx, hipEventElapsedTime(&ms, q[s - 3], q[s - 2]));
            } else if (ctx->prof_side_used && (s == (ctx->prof_stems ? 6 : 9) || s == (ctx->prof_stems ? 7 : 12))) {
                // the two kernels launched beside it on the caller's stream, in launch order
                hipEvent_t *q = ctx->prof_main2.step(k);
                const bool first = s == (ctx->prof_stems ? 6 : 9);
                HIP_TRY(ctx, hipEventElapsedTime(&ms, first ? e[5] : q[0], first ? q[0] : q[1]));
            } else {
                HIP_TRY(ctx, hipEventElapsedTime(&ms, e[s], e[s + 1]));
            }
            acc += ms;
        }
        ms_per_stage[s] = acc;
    }
    return ctx->prof_steps;
}

const char *goofer_profile_stage_name(int stage) { return stage >= 0 && stage < PROF_STAGES ? PROF_NAMES[stage] : ""; }

static const char *const PROF_NAMES_STEMS[PROF_STAGES] = {
    "setup_maps", "", "", "phase_inc", "pulse_onsets", "pulse_place", "mask_short", "noise_stems",
    "", "harm_stem", "", "", "", "note_finish", "", "env_edit", "env_rows", "sample_assemble"};

// fused_ola routes; ola_split reports k_irfft_ola1 as irfft_ola3 and k_note_finish as apply_gain (bench.py keys on these names)
static const char *const PROF_NAMES_OLA[PROF_STAGES] = {
    "setup_maps", "", "", "phase_inc", "pulse_onsets", "pulse_place", "rfft_frames", "harm_shape",
    "", "noise_spectra", "", "", "mask_short", "irfft_ola3", "apply_gain", "env_edit", "env_rows", "sample_assemble"};

const char *goofer_profile_stage_name_ex(const goofer_ctx *ctx, int stage)
{
    if (stage < 0 || stage >= PROF_STAGES) return "";
    if (ctx && ctx->prof_stems) return PROF_NAMES_STEMS[stage];
    return (ctx && ctx->ola_fused) ? PROF_NAMES_OLA[stage] : PROF_NAMES[stage];
}

/* options: see include/goofer_hip.h */
int goofer_set_option(goofer_ctx *ctx, const char *name, int value)
{
    if (!ctx || !name) return GOOFER_EINVAL;
    if (!strcmp(name, "fused_ola")) { ctx->ola_fused = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "overlap")) { ctx->overlap = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "stems")) { ctx->stems = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "prof_only")) { ctx->prof_only = value < 0 || value >= PROF_STAGES ? -1 : value; return GOOFER_OK; }   // stage index, -1: all
    if (!strcmp(name, "skip_zero")) { ctx->skip_zero = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "td_blur")) { ctx->td_blur = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "pulse_scan")) { ctx->pulse_scan = value < 0 ? 0 : (value > 2 ? 2 : value); return GOOFER_OK; }
    if (!strcmp(name, "pulse_fused")) { ctx->pulse_fused = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "sa_fast")) { ctx->sa_fast = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "sa_table")) { ctx->sa_table = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "legacy_wave")) { ctx->legacy_wave = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "mask_flags")) { ctx->mask_flags = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "mask_sparse")) { ctx->mask_sparse = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "value_f64")) { ctx->value_f64 = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "rate_lds")) { ctx->rate_lds = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "limit_skip")) { ctx->limit_skip = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "limit_tp_skip")) { ctx->limit_tp_skip = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "compress_skip")) { ctx->compress_skip = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "compress_store")) { ctx->compress_store = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "reverb_skip")) { ctx->reverb_skip = value != 0; return GOOFER_OK; }
    if (!strcmp(name, "walk_run")) { ctx->walk_run = value < 0 ? 0 : value; return GOOFER_OK; }   // clamped per kernel where the run is chosen (walk_run_choice)
    return goofer_fail(ctx, GOOFER_EINVAL, "unknown option %s", name);
}

int goofer_sizeof(int which)
{
    switch (which) {
    case 0: return (int)sizeof(goofer_note_params);
    case 1: return (int)sizeof(goofer_batch);
    case 2: return (int)sizeof(goofer_note_plan);
    case 3: return (int)sizeof(goofer_assembly);
    case 4: return (int)sizeof(goofer_onepole_job);
    case 5: return (int)sizeof(goofer_post_note);
    case 6: return (int)sizeof(goofer_post);
    case 7: return (int)sizeof(goofer_plan_request);
    case 8: return (int)sizeof(goofer_plan_geometry);
    case 9: return (int)sizeof(goofer_legacy_job);
    case 10: return (int)sizeof(goofer_track_settings);
    case 11: return (int)sizeof(goofer_phrase_note);
    }
    return -1;
}

int goofer_rfft_frames(goofer_ctx *ctx, const float *x, const int64_t *sample_off, const int64_t *frame_off, int n_notes,
                       int64_t total_frames, float *S, int ldc, void *stream)
{
    NEED_PLAN(ctx);
    if (ldc < ctx->plan.n_bins) return goofer_fail(ctx, GOOFER_EINVAL, "ldc %d < n_bins %d", ldc, ctx->plan.n_bins);
    hipStream_t st = (hipStream_t)stream;
    int *frame_note;
    int rc = carve_scratch(ctx, [&](arena &a) { frame_note = a.take<int>(total_frames); });
    if (rc) return rc;
    if ((rc = launch_frame_note(ctx, frame_off, n_notes, total_frames, frame_note, st))) return rc;
    return launch_rfft_frames_mapped(ctx, x, sample_off, frame_off, frame_note, total_frames, (float2 *)S, ldc, st);
}

int goofer_irfft_ola(goofer_ctx *ctx, const float *S, int ldc, const int64_t *sample_off, const int64_t *frame_off, int n_notes,
                     int64_t total_frames, int64_t total_samples, float *y, void *stream)
{
    NEED_PLAN(ctx);
    hipStream_t st = (hipStream_t)stream;
    float *frames;
    int rc = carve_scratch(ctx, [&](arena &a) { frames = a.take<float>((size_t)total_frames * ctx->plan.n_fft); });
    if (rc) return rc;
    if ((rc = launch_irfft_frames(ctx, (const float2 *)S, ldc, total_frames, frames, st))) return rc;
    return launch_ola_gather(ctx, frames, sample_off, frame_off, n_notes, total_samples, y, nullptr, st);
}

int goofer_pulse_train(goofer_ctx *ctx, const float *f0, const int64_t *sample_off, int n_notes, int64_t total_samples,
                       float *pulse, void *stream)
{
    NEED_PLAN(ctx);
    hipStream_t st = (hipStream_t)stream;
    const size_t slots = onset_slots(total_samples, n_notes, false);
    double *inc;
    onset_t *onsets;
    int32_t *oidx, *cnt;
    int rc = carve_scratch(ctx, [&](arena &a) {
        inc = a.take<double>(total_samples + 16);          // (also holds the placement's tile table: 16 bytes per 256 * PP_SPT samples)
        onsets = (onset_t *)a.take<char>(slots * ONSET_BYTES);
        oidx = a.take<int32_t>(slots);
        cnt = a.take<int32_t>(n_notes + 16);
    });
    if (rc) return rc;
    for (int i = 0; i < 17; ++i) ctx->dbg_ptr[i] = nullptr;
    ctx->dbg_ptr[13] = cnt; ctx->dbg_bytes[13] = n_notes * sizeof(int32_t);
    ctx->dbg_ptr[14] = oidx; ctx->dbg_bytes[14] = slots * sizeof(int32_t);
    return launch_pulse_train(ctx, f0, 1.0f, sample_off, n_notes, total_samples, pulse, inc, onsets, oidx, cnt, ctx->ovf_flag, st);
}

int goofer_gauss_bins(goofer_ctx *ctx, const float *in, float *out, int64_t rows, int n_bins, int ld, const double *taps,
                      int radius, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (radius < 0 || radius > 4096 || n_bins <= 0 || ld < n_bins) return goofer_fail(ctx, GOOFER_EINVAL, "bad gauss geometry");
    hipStream_t st = (hipStream_t)stream;
    int rc = grow_block(ctx, &ctx->small, &ctx->small_bytes, std::max<size_t>(SMALL_FIXED, (size_t)(2 * radius + 1) * sizeof(double) + 64),
                        "small block");
    if (rc) return rc;
    double *d_taps = (double *)((char *)ctx->small + SMALL_TABLES);
    HIP_TRY(ctx, hipMemcpyAsync(d_taps, taps, (2 * radius + 1) * sizeof(double), hipMemcpyHostToDevice, st));
    return launch_gauss_bins(ctx, in, out, rows, n_bins, ld, d_taps, radius, nullptr, st);
}

int goofer_warp_bins(goofer_ctx *ctx, const float *in, float *out, int64_t rows, int n_bins, int ld, const double *formants,
                     const double *f_shift, double ratio, void *stream)
{
    NEED_PLAN(ctx);
    hipStream_t st = (hipStream_t)stream;
    const double *d_shift = nullptr;
    if (f_shift) {
        int rc = grow_block(ctx, &ctx->small, &ctx->small_bytes, SMALL_FIXED, "small block");
        if (rc) return rc;
        d_shift = (const double *)((char *)ctx->small + SMALL_WORDS);
        HIP_TRY(ctx, hipMemcpyAsync((void *)d_shift, f_shift, 4 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    return launch_warp_bins(ctx, in, out, rows, n_bins, ld, formants, d_shift, nullptr, nullptr, nullptr, ratio, st);
}

static void knot_lerp_plan(const goofer_plan_t &p, const float *hz_knots, int K, int n_bins, std::vector<int> &idx,
                           std::vector<float> &w0, std::vector<float> &w1)
{
    // 2-tap lerp plan, fp32 arithmetic like precompute_interp_matrix (GOOFER.py:84-90)
    idx.resize(n_bins); w0.resize(n_bins); w1.resize(n_bins);
    double val = 1.0 / ((double)p.n_fft * (1.0 / (double)p.sr));
    for (int b = 0; b < n_bins; ++b) {
        float f = (float)((double)b * val);
        int i = (int)(std::upper_bound(hz_knots, hz_knots + K, f) - hz_knots) - 1;   // searchsorted(side='right') - 1
        i = std::min(std::max(i, 0), K - 2);
        float x0 = hz_knots[i], x1 = hz_knots[i + 1];
        float den = std::max(x1 - x0, 1e-12f);
        float b1 = (f - x0) / den;
        idx[b] = i; w1[b] = b1; w0[b] = 1.0f - b1;
    }
}

int goofer_knot_decode(goofer_ctx *ctx, const uint16_t *knots_f16, int K, const float *hz_knots, int64_t rows, float *env,
                       int n_bins, int ld, void *stream)
{
    NEED_PLAN(ctx);
    if (K < 2 || K > 4096) return goofer_fail(ctx, GOOFER_EINVAL, "bad knot count %d", K);
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> idx;
    std::vector<float> w0, w1;
    knot_lerp_plan(ctx->plan, hz_knots, K, n_bins, idx, w0, w1);
    int rc = grow_block(ctx, &ctx->small, &ctx->small_bytes, SMALL_FIXED, "small block");
    if (rc) return rc;
    if ((size_t)n_bins * 12 > SMALL_WORDS - SMALL_TABLES) return goofer_fail(ctx, GOOFER_EINVAL, "n_bins too large");
    char *d = (char *)ctx->small + SMALL_TABLES;
    int *d_idx = (int *)d;
    float *d_w0 = (float *)(d + 4 * (size_t)n_bins), *d_w1 = (float *)(d + 8 * (size_t)n_bins);
    HIP_TRY(ctx, hipMemcpyAsync(d_idx, idx.data(), n_bins * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_w0, w0.data(), n_bins * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_w1, w1.data(), n_bins * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));   // the host vectors die at return
    return launch_knot_decode(ctx, knots_f16, K, rows, d_idx, d_w0, d_w1, env, n_bins, ld, st);
}

int goofer_gauss_bins_f64(goofer_ctx *ctx, const float *in, int ld, double *out, int ld64, int64_t rows, int n_bins,
                          const double *taps, int radius, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (radius < 0 || radius > 4096 || ld < n_bins || ld64 < n_bins) return goofer_fail(ctx, GOOFER_EINVAL, "bad gauss geometry");
    hipStream_t st = (hipStream_t)stream;
    int rc = grow_block(ctx, &ctx->small, &ctx->small_bytes, std::max<size_t>(SMALL_FIXED, (size_t)(2 * radius + 1) * sizeof(double) + 64),
                        "small block");
    if (rc) return rc;
    double *d_taps = (double *)((char *)ctx->small + SMALL_TABLES);
    HIP_TRY(ctx, hipMemcpyAsync(d_taps, taps, (2 * radius + 1) * sizeof(double), hipMemcpyHostToDevice, st));
    return launch_gauss_rows64(ctx, in, ld, out, ld64, rows, n_bins, d_taps, radius, st);
}

int goofer_knot_fit_error(goofer_ctx *ctx, const double *env, int ld64, const int64_t *probe_rows, int n_probe, int n_bins,
                          const int32_t *knot_bin, int K, const float *hz_knots, double *max_rel_err, void *stream)
{
    NEED_PLAN(ctx);
    if (K < 2 || K > 4096 || !max_rel_err) return goofer_fail(ctx, GOOFER_EINVAL, "bad knot count %d", K);
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> idx;
    std::vector<float> w0, w1;
    knot_lerp_plan(ctx->plan, hz_knots, K, n_bins, idx, w0, w1);
    int rc = grow_block(ctx, &ctx->small, &ctx->small_bytes, SMALL_FIXED, "small block");
    if (rc) return rc;
    if ((size_t)n_bins * 12 + 64 > SMALL_WORDS - SMALL_TABLES) return goofer_fail(ctx, GOOFER_EINVAL, "n_bins too large");
    char *d = (char *)ctx->small + SMALL_TABLES;
    int *d_idx = (int *)d;
    float *d_w0 = (float *)(d + 4 * (size_t)n_bins), *d_w1 = (float *)(d + 8 * (size_t)n_bins);
    unsigned long long *d_err = (unsigned long long *)((char *)ctx->small + SMALL_WORDS);
    HIP_TRY(ctx, hipMemcpyAsync(d_idx, idx.data(), n_bins * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_w0, w0.data(), n_bins * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_w1, w1.data(), n_bins * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(d_err, 0, sizeof(unsigned long long), st));
    if ((rc = launch_knot_error(ctx, env, ld64, probe_rows, n_probe, n_bins, knot_bin, K, d_idx, d_w0, d_w1, d_err, st))) return rc;
    unsigned long long bits = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bits, d_err, sizeof(bits), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    memcpy(max_rel_err, &bits, sizeof(double));
    return GOOFER_OK;
}

int goofer_knot_gather(goofer_ctx *ctx, const double *env, int ld64, int64_t rows, const int32_t *knot_bin, int K,
                       uint16_t *knots_f16, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    return launch_knot_gather(ctx, env, ld64, rows, knot_bin, K, knots_f16, (hipStream_t)stream);
}

int goofer_envelope_knots_batch(goofer_ctx *ctx, const float *y, const int64_t *sample_off, int n_signals, const double *taps_env,
                                int radius_env, const double *taps_fit, int radius_fit, const float *hz_knots, const int32_t *knot_bin,
                                int64_t *frame_off, uint16_t *knots_f16, int32_t *K_out, double *env_rows, int ld64, void *scratch,
                                int64_t *scratch_bytes, void *stream)
{
    NEED_PLAN(ctx);
    const goofer_plan_t &p = ctx->plan;
    const int nb = p.n_bins, ldc = spec_stride(nb), ld2 = (nb + 1) & ~1;
    if (!sample_off || n_signals <= 0 || !frame_off || !scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "envelope batch: null argument");
    if (sample_off[0] != 0) return goofer_fail(ctx, GOOFER_EINVAL, "envelope batch: sample_off[0] must be 0");
    if (radius_env < 0 || radius_env > 64 || radius_fit < 0 || radius_fit > 64 || !taps_env || !taps_fit)
        return goofer_fail(ctx, GOOFER_EINVAL, "envelope batch: bad taps");
    frame_off[0] = 0;
    int64_t n_probe = 0;
    for (int s = 0; s < n_signals; ++s) {
        const int64_t n = sample_off[s + 1] - sample_off[s];
        if (n < 1) return goofer_fail(ctx, GOOFER_EINVAL, "envelope batch: signal %d is empty", s);
        const int64_t T = 1 + n / p.hop;                                               // frames of gf.stft
        frame_off[s + 1] = frame_off[s] + T;
        n_probe += std::min<int64_t>(256, T);
    }
    const int64_t F = frame_off[n_signals];
    int64_t *d_soff, *d_foff, *probe_row;
    int *frame_sig, *probe_sig, *d_bin, *d_idx;
    float2 *S;
    double *env2, *d_taps;
    float *d_w0, *d_w1;
    unsigned long long *err;
    auto carve = [&](arena &a) {
        d_soff = a.take<int64_t>(n_signals + 1);
        d_foff = a.take<int64_t>(n_signals + 1);
        frame_sig = a.take<int>(F);
        S = a.take<float2>((size_t)F * ldc);
        env2 = a.take<double>((size_t)F * ld2);
        probe_row = a.take<int64_t>(n_probe);
        probe_sig = a.take<int>(n_probe);
        err = a.take<unsigned long long>((size_t)n_signals * KN_CAND);
        d_taps = a.take<double>(2 * (radius_env + radius_fit) + 2);
        d_bin = a.take<int>(KN_BINS_TOTAL);
        d_idx = a.take<int>((size_t)KN_CAND * nb);
        d_w0 = a.take<float>((size_t)KN_CAND * nb);
        d_w1 = a.take<float>((size_t)KN_CAND * nb);
    };
    if (scratch && (!y || !knots_f16 || !K_out || !hz_knots || !knot_bin || (env_rows && ld64 < nb)))
        return goofer_fail(ctx, GOOFER_EINVAL, "envelope batch: null signal, output or ld64 < n_bins");
    int rc = caller_scratch(ctx, scratch, scratch_bytes, "envelope batch", carve);
    if (rc || !scratch) return rc;
    for (int i = 0; i < KN_BINS_TOTAL; ++i)
        if (knot_bin[i] < 0 || knot_bin[i] >= nb) return goofer_fail(ctx, GOOFER_EINVAL, "envelope batch: knot bin %d out of range", knot_bin[i]);

    // probe rows: linspace(0, T - 1, min(256, T), dtype=int) per signal, as numpy computes it (start + j * step, last = stop, floor)
    std::vector<int64_t> prow;
    std::vector<int> psig;
    prow.reserve(n_probe);
    psig.reserve(n_probe);
    for (int s = 0; s < n_signals; ++s) {
        const int64_t T = frame_off[s + 1] - frame_off[s], num = std::min<int64_t>(256, T);
        const double step = num > 1 ? (double)(T - 1) / (double)(num - 1) : 0.0;
        for (int64_t j = 0; j < num; ++j) {
            const int64_t v = j == num - 1 ? T - 1 : (int64_t)floor((double)j * step);
            prow.push_back(frame_off[s] + v);
            psig.push_back(s);
        }
    }
    // the lerp tables of every candidate, from the helper goofer_knot_fit_error / goofer_knot_decode use
    std::vector<int> idx_all((size_t)KN_CAND * nb), idx;
    std::vector<float> w0_all((size_t)KN_CAND * nb), w1_all((size_t)KN_CAND * nb), w0, w1;
    for (int c = 0, kb = 0; c < KN_CAND; kb += KN_K0 + KN_DK * c, ++c) {
        knot_lerp_plan(p, hz_knots + kb, KN_K0 + KN_DK * c, nb, idx, w0, w1);
        std::copy(idx.begin(), idx.end(), idx_all.begin() + (size_t)c * nb);
        std::copy(w0.begin(), w0.end(), w0_all.begin() + (size_t)c * nb);
        std::copy(w1.begin(), w1.end(), w1_all.begin() + (size_t)c * nb);
    }
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, hipMemcpyAsync(d_soff, sample_off, 8 * (size_t)(n_signals + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_foff, frame_off, 8 * (size_t)(n_signals + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(probe_row, prow.data(), 8 * (size_t)n_probe, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(probe_sig, psig.data(), 4 * (size_t)n_probe, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_taps, taps_env, 8 * (size_t)(2 * radius_env + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_taps + 2 * radius_env + 1, taps_fit, 8 * (size_t)(2 * radius_fit + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_bin, knot_bin, 4 * (size_t)KN_BINS_TOTAL, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_idx, idx_all.data(), 4 * idx_all.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_w0, w0_all.data(), 4 * w0_all.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_w1, w1_all.data(), 4 * w1_all.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(err, 0, 8 * (size_t)n_signals * KN_CAND, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                            // the host vectors go out of scope

    if ((rc = launch_frame_note(ctx, d_foff, n_signals, F, frame_sig, st))) return rc;
    if ((rc = launch_rfft_frames_mapped(ctx, y, d_soff, d_foff, frame_sig, F, S, ldc, st))) return rc;
    if ((rc = launch_env_rows_fused(ctx, S, ldc, F, nb, d_taps, radius_env, d_taps + 2 * radius_env + 1, radius_fit, env_rows, ld64, env2, ld2,
                                    st)))
        return rc;
    if ((rc = launch_knot_search(ctx, env2, ld2, probe_row, probe_sig, (int)n_probe, nb, d_bin, d_idx, d_w0, d_w1, err, st))) return rc;
    return launch_knot_pick(ctx, env2, ld2, F, frame_sig, d_foff, d_bin, err, knots_f16, K_out, st);
}

/* gf.smooth_mask_ds (GOOFER.py:556-569) for a ragged batch of masks: decimate by 4, Gaussian sigma/4 (fp64), linear
 * upsample on float32 linspace grids.  `fast_interp` selects the interpolant form the stem walkers use. */
int goofer_smooth_mask_ds(goofer_ctx *ctx, const float *mask, const int64_t *sample_off, int n_notes, int64_t total_samples,
                          float sigma, int fast_interp, float *out, void *stream)
{
    NEED_PLAN(ctx);
    if (!mask || !sample_off || !out || n_notes <= 0) return goofer_fail(ctx, GOOFER_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    std::vector<double> taps;
    int radius;
    gauss_taps_host(std::max(1.0, (double)sigma / 4.0), taps, radius);                // GOOFER.py:561
    if (radius > 2048) return goofer_fail(ctx, GOOFER_EINVAL, "transition sigma too large");
    const size_t n_short = (size_t)(total_samples / 4 + n_notes + 16);
    // the small block from byte 0 as one piece (see SMALL_*): taps, decimated mask, per-note steps
    int rc = grow_block(ctx, &ctx->small, &ctx->small_bytes, (taps.size() + 16 + n_short + 2 * (size_t)n_notes + 16) * sizeof(double),
                        "small block");
    if (rc) return rc;
    double *d_taps = (double *)ctx->small, *short_s = d_taps + taps.size() + 16, *steps = short_s + n_short;
    HIP_TRY(ctx, hipMemcpyAsync(d_taps, taps.data(), taps.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                            // the host vector goes out of scope
    double acc = 0.0;
    for (double tv : taps) acc += tv * 1.0;
    if ((rc = launch_mask_short(ctx, mask, sample_off, n_notes, total_samples, d_taps, radius, acc, short_s, nullptr, nullptr, false, st))) return rc;
    return launch_mask_upsample(ctx, short_s, sample_off, n_notes, total_samples, steps, fast_interp != 0, out, st);
}

int goofer_normal_fill(goofer_ctx *ctx, uint64_t seed, const goofer_note_params *params, const int64_t *sample_off, int n_notes,
                       int64_t total_samples, int stream_tag, const unsigned char *note_on, const double *growl_scale, double *out,
                       void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (!params || !sample_off || !out) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_normal_fill: null pointer");
    if (n_notes < 0 || total_samples < 0)
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_normal_fill: negative count (%d notes, %lld samples)", n_notes, (long long)total_samples);
    if (stream_tag < 0 || stream_tag > 4) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_normal_fill: stream tag %d outside 0..4", stream_tag);
    if ((uintptr_t)out & 15) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_normal_fill: out must be 16-byte aligned");
    return launch_normal_fill(ctx, seed, params, sample_off, n_notes, total_samples, stream_tag, note_on, growl_scale, out, (hipStream_t)stream);
}

int goofer_phase_fill(goofer_ctx *ctx, const uint64_t *pcg_words, const int64_t *frame_off, int n_notes, int64_t total_frames, int n_bins,
                      float *out, int ld, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (!pcg_words || !frame_off || !out) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_phase_fill: null pointer");
    if (n_notes < 0 || total_frames < 0)
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_phase_fill: negative count (%d notes, %lld frames)", n_notes, (long long)total_frames);
    if (n_bins <= 0 || ld < n_bins) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_phase_fill: %d bins with row stride %d", n_bins, ld);
    if (((uintptr_t)pcg_words & 7) || ((uintptr_t)frame_off & 7) || ((uintptr_t)out & 3))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_phase_fill: pcg_words and frame_off must be 8-byte aligned, out 4-byte aligned");
    return launch_phase_fill(ctx, pcg_words, frame_off, n_notes, total_frames, n_bins, out, ld, (hipStream_t)stream);
}

int goofer_legacy_normal_fill(goofer_ctx *ctx, const uint32_t *seeds, const unsigned char *stream_on, const int64_t *sample_off, int n_notes,
                              int64_t total_samples, double *out_f0, double *out_vol_h, double *out_vol_b, int64_t *attempts, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (!seeds || !stream_on || !sample_off) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_legacy_normal_fill: null pointer");
    if (!out_f0 && !out_vol_h && !out_vol_b && !attempts) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_legacy_normal_fill: no output");
    if (n_notes < 0 || total_samples < 0)
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_legacy_normal_fill: negative count (%d notes, %lld samples)", n_notes, (long long)total_samples);
    if (((uintptr_t)seeds & 3) || ((uintptr_t)sample_off & 7) || ((uintptr_t)out_f0 & 7) || ((uintptr_t)out_vol_h & 7) || ((uintptr_t)out_vol_b & 7) ||
        ((uintptr_t)attempts & 7))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_legacy_normal_fill: seeds must be 4-byte aligned, sample_off, the outputs and attempts 8-byte aligned");
    if (total_samples == 0 && !attempts) return GOOFER_OK;
    return launch_legacy_normal_fill(ctx, seeds, stream_on, sample_off, n_notes, out_f0, out_vol_h, out_vol_b, attempts, (hipStream_t)stream);
}

int goofer_legacy_normal_jobs(goofer_ctx *ctx, const goofer_legacy_job *jobs, int n_jobs, int64_t *attempts, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (!jobs) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_legacy_normal_jobs: null pointer");
    if (n_jobs < 0) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_legacy_normal_jobs: negative count (%d jobs)", n_jobs);
    if (((uintptr_t)jobs & 7) || ((uintptr_t)attempts & 7))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_legacy_normal_jobs: jobs and attempts must be 8-byte aligned");
    return launch_legacy_normal_jobs(ctx, jobs, n_jobs, attempts, (hipStream_t)stream);
}

int goofer_stretch_rows(goofer_ctx *ctx, const float *in, int64_t ld_in, int64_t rows_in, float *out, int64_t ld_out, int64_t rows_out,
                        int n_cols, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (!in || !out) return goofer_fail(ctx, GOOFER_EINVAL, "null pointer");
    if (n_cols == 1 && ld_in == 1 && ld_out == 1) return launch_lerp_1d(ctx, in, rows_in, out, rows_out, (hipStream_t)stream);
    return launch_lerp_axis0(ctx, in, ld_in, rows_in, out, ld_out, rows_out, n_cols, (hipStream_t)stream);
}

int goofer_ingest_rows(goofer_ctx *ctx, const void *in, int in_f64, const int64_t *row_off, const int64_t *tile_off, int n_notes,
                       int64_t total_tiles, int n_cols, float *out, int ld, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (n_notes <= 0 || total_tiles <= 0) return GOOFER_OK;
    if (!in || !row_off || !tile_off || !out) return goofer_fail(ctx, GOOFER_EINVAL, "null pointer");
    if (n_cols <= 0 || ld < n_cols) return goofer_fail(ctx, GOOFER_EINVAL, "ingest: %d columns with row stride %d", n_cols, ld);
    return launch_ingest_rows(ctx, in, in_f64 != 0, row_off, tile_off, n_notes, total_tiles, n_cols, out, ld, (hipStream_t)stream);
}

int goofer_warp_bins_ragged(goofer_ctx *ctx, const float *in, float *out, int64_t rows, int n_bins, int ld, const double *formants,
                            const int64_t *row_off, int n_notes, const double *note_args, void *stream)
{
    NEED_PLAN(ctx);
    if (rows <= 0 || n_notes <= 0) return GOOFER_OK;
    if (!in || !out || !row_off || !note_args) return goofer_fail(ctx, GOOFER_EINVAL, "null pointer");
    if (n_bins != ctx->plan.n_bins || ld < n_bins) return goofer_fail(ctx, GOOFER_EINVAL, "ragged warp: %d bins, the plan has %d", n_bins, ctx->plan.n_bins);
    return launch_warp_bins_ragged(ctx, in, out, rows, n_bins, ld, formants, row_off, n_notes, note_args, (hipStream_t)stream);
}

int goofer_stretch_ragged(goofer_ctx *ctx, const int64_t *row_off_in, const int64_t *row_off_out, const int64_t *row_cut,
                          const int64_t *sample_off_in, const int64_t *sample_off_out, const int64_t *sample_cut, int n_notes,
                          int64_t rows_out, int64_t samples_out, int n_cols, int ld, const float *env_h, const float *env_n,
                          float *env_h_out, float *env_n_out, const float *f0, const float *mask, float *f0_out, float *mask_out,
                          void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (n_notes <= 0) return GOOFER_OK;
    if (!row_off_in || !row_off_out || !row_cut || !sample_off_in || !sample_off_out || !sample_cut)
        return goofer_fail(ctx, GOOFER_EINVAL, "null pointer");
    if (rows_out > 0 && (!env_h || !env_n || !env_h_out || !env_n_out || n_cols <= 0 || ld < n_cols))
        return goofer_fail(ctx, GOOFER_EINVAL, "ragged stretch: envelope rows without matrices");
    if (samples_out > 0 && (!f0 || !mask || !f0_out || !mask_out)) return goofer_fail(ctx, GOOFER_EINVAL, "ragged stretch: samples without arrays");
    return launch_stretch_ragged(ctx, row_off_in, row_off_out, row_cut, sample_off_in, sample_off_out, sample_cut, n_notes, rows_out,
                                 samples_out, n_cols, ld, env_h, env_n, env_h_out, env_n_out, f0, mask, f0_out, mask_out,
                                 (hipStream_t)stream);
}

int goofer_gauss_rows_f64(goofer_ctx *ctx, const double *in, const int64_t *row_off, int n_rows, int64_t total, const double *taps,
                          int radius, double *out, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (!in || !out || !row_off || !taps) return goofer_fail(ctx, GOOFER_EINVAL, "null pointer");
    if (radius < 0 || radius > (1 << 22)) return goofer_fail(ctx, GOOFER_EINVAL, "gaussian radius %d outside [0, 2^22]", radius);
    if (n_rows <= 0 || total <= 0) return GOOFER_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t tap_bytes = (size_t)(2 * radius + 1) * sizeof(double);
    int rc = grow_block(ctx, &ctx->small, &ctx->small_bytes, SMALL_RAGGED + tap_bytes, "small block");
    if (rc) return rc;
    double *d_taps = (double *)((char *)ctx->small + SMALL_RAGGED);
    HIP_TRY(ctx, hipMemcpyAsync(d_taps, taps, tap_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                   // the caller's taps buffer may be transient
    return launch_gauss_samples<double>(ctx, in, row_off, n_rows, total, d_taps, radius, nullptr, out, st);
}

int goofer_vocal_roughness(goofer_ctx *ctx, const float *y, const float *f0, const float *mask, const double *noise_s, int n_k,
                           const double *k_list, const double *h_list, double noise_amp, double hp_fc, const float *alpha_slewed,
                           const int64_t *sample_off, int n_notes, int64_t total_samples, float *out, void *stream)
{
    NEED_PLAN(ctx);
    if (!y || !f0 || !mask || !alpha_slewed || !sample_off || !out || (n_k > 0 && (!noise_s || !k_list || !h_list)))
        return goofer_fail(ctx, GOOFER_EINVAL, "null pointer");
    return launch_vocal_roughness(ctx, y, f0, mask, noise_s, n_k, k_list, h_list, noise_amp, hp_fc, alpha_slewed, sample_off, n_notes,
                                  total_samples, out, (hipStream_t)stream);
}

int goofer_onepole_cascade(goofer_ctx *ctx, const float *src, float *dst, const float *f0, const goofer_onepole_job *jobs, int n_jobs,
                           void *stream)
{
    NEED_PLAN(ctx);
    if (!src || !dst || !f0 || !jobs) return goofer_fail(ctx, GOOFER_EINVAL, "null pointer");
    return launch_onepole(ctx, src, dst, f0, jobs, n_jobs, (hipStream_t)stream);
}

}  // extern "C"
