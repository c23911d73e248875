// gf.stretch_feature (GOOFER.py:597-616) for gfx950: resample axis 0 of a [rows x cols] fp32 matrix (or a 1-D array,
// cols = 1) to R_out rows on normalised coordinates — np.interp(linspace(0, 1, R_out), linspace(0, 1, R_in), column),
// evaluated in fp64 like numpy and rounded to fp32.  Used by gf.synthesize's optional time stretch (GOOFER.py:1019-1067).
#include "common.h"
#include "launchers.h"

// np.linspace(0, 1, n)[i]
__device__ __forceinline__ double lin01(int64_t i, int64_t n, double step)
{
    if (n <= 1) return 0.0;
    if (i >= n - 1) return 1.0;
    return (double)i * step;
}

// Where output row r of R_out falls on the R_in input rows: np.interp's segment (j, j + 1) and abscissae, found once per row
// and shared by every column (k_lerp_axis0, k_lerp_1d and the ragged k_stretch_ragged make the same fp64 steps).
struct lerp_pt {
    int64_t j;          // left input row; j >= R_in - 1: the last row's value (one = R_in == 1: the constant)
    double x, x0, x1;
    bool last, one;
};

__device__ __forceinline__ lerp_pt lerp_locate(int64_t r, int64_t R_in, int64_t R_out, double step_in, double step_out)
{
    lerp_pt p;
    p.one = R_in == 1;                                        // one knot: constant                GOOFER.py:183-191
    p.j = 0; p.x = p.x0 = p.x1 = 0.0; p.last = false;
    if (p.one) return p;
    const double x = lin01(r, R_out, step_out);
    int64_t j = (int64_t)(x * (double)(R_in - 1));
    if (j > R_in - 1) j = R_in - 1;
    if (j < 0) j = 0;
    while (j + 1 <= R_in - 1 && lin01(j + 1, R_in, step_in) <= x) ++j;
    while (j > 0 && lin01(j, R_in, step_in) > x) --j;
    p.j = j; p.x = x;
    p.last = j >= R_in - 1;
    if (!p.last) { p.x0 = lin01(j, R_in, step_in); p.x1 = lin01(j + 1, R_in, step_in); }
    return p;
}

// The fp32 value at a located point of one column: `col` is the column's first element, `ld` its row stride.
__device__ __forceinline__ float lerp_value(const lerp_pt &p, const float *__restrict__ col, int64_t ld, int64_t R_in)
{
    if (p.one) return col[0];
    if (p.last) return col[(R_in - 1) * ld];
    const double y0 = (double)col[p.j * ld], y1 = (double)col[(p.j + 1) * ld];
    const double v = p.x == p.x0 ? y0 : ((y1 - y0) / (p.x1 - p.x0)) * (p.x - p.x0) + y0;      // np.interp's slope form
    return (float)v;
}

__global__ __launch_bounds__(256) void k_lerp_axis0(const float *__restrict__ in, int64_t ld_in, int64_t R_in, float *__restrict__ out,
                                                    int64_t ld_out, int64_t R_out, int n_cols, double step_in, double step_out)
{
    const int64_t r = blockIdx.y;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R_out || c >= n_cols) return;
    out[r * ld_out + c] = lerp_value(lerp_locate(r, R_in, R_out, step_in, step_out), in + c, ld_in, R_in);
}

int launch_lerp_axis0(goofer_ctx *ctx, const float *in, int64_t ld_in, int64_t R_in, float *out, int64_t ld_out, int64_t R_out,
                      int n_cols, hipStream_t st)
{
    if (R_out <= 0 || n_cols <= 0) return GOOFER_OK;
    if (R_in <= 0) return goofer_fail(ctx, GOOFER_EINVAL, "cannot stretch an empty feature");
    const double step_in = R_in > 1 ? 1.0 / (double)(R_in - 1) : 0.0, step_out = R_out > 1 ? 1.0 / (double)(R_out - 1) : 0.0;
    if (R_out > 65535) return goofer_fail(ctx, GOOFER_EINVAL, "more than 65535 output rows: resample in pieces (1-D arrays have their own entry)");
    dim3 grid((unsigned)((n_cols + 255) / 256), (unsigned)R_out);
    hipLaunchKernelGGL(k_lerp_axis0, grid, dim3(256), 0, st, in, ld_in, R_in, out, ld_out, R_out, n_cols, step_in, step_out);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

// 1-D flavour: thread per output element
__global__ __launch_bounds__(256) void k_lerp_1d(const float *__restrict__ in, int64_t R_in, float *__restrict__ out, int64_t R_out,
                                                 double step_in, double step_out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R_out) return;
    out[r] = lerp_value(lerp_locate(r, R_in, R_out, step_in, step_out), in, 1, R_in);
}

int launch_lerp_1d(goofer_ctx *ctx, const float *in, int64_t R_in, float *out, int64_t R_out, hipStream_t st)
{
    if (R_out <= 0) return GOOFER_OK;
    if (R_in <= 0) return goofer_fail(ctx, GOOFER_EINVAL, "cannot stretch an empty feature");
    const double step_in = R_in > 1 ? 1.0 / (double)(R_in - 1) : 0.0, step_out = R_out > 1 ? 1.0 / (double)(R_out - 1) : 0.0;
    hipLaunchKernelGGL(k_lerp_1d, dim3((unsigned)((R_out + 255) / 256)), dim3(256), 0, st, in, R_in, out, R_out, step_in, step_out);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

// ---------------------------------------------------------------------------------------------
// Envelope ingest (gf.synthesize's to_compute(env_spec).T per note, GOOFER.py:72, 984): every note's [n_cols x T] block of the
// caller's array, fp64 or fp32, back to back in one buffer, becomes T rows of the ld-strided fp32 matrix the batch reads.
// A block of 256 threads moves one 64 x 64 tile through LDS (row stride 65: the transposed reads hit 64 different banks):
// the loads run along the note's frame axis and the stores along the bins, both coalesced.  fp64 -> fp32 is the
// round-to-nearest-even conversion of numpy's astype(np.float32).
constexpr int INGEST_TILE = 64;

// Largest i < n with off[i] <= g (off ascending, off[0] <= g): the note a flat index belongs to, empty notes skipped.
__device__ __forceinline__ int csr_note(const int64_t *__restrict__ off, int n, int64_t g)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename T>
__global__ __launch_bounds__(256) void k_ingest_rows(const T *__restrict__ in, const int64_t *__restrict__ row_off,
                                                     const int64_t *__restrict__ tile_off, int n_notes, int n_cols, int col_tiles,
                                                     float *__restrict__ out, int ld)
{
    __shared__ float s[INGEST_TILE][INGEST_TILE + 1];
    const int64_t ft = (int64_t)blockIdx.x / col_tiles;
    const int c0 = (int)((int64_t)blockIdx.x - ft * col_tiles) * INGEST_TILE;
    const int note = csr_note(tile_off, n_notes, ft);
    const int64_t r0 = row_off[note], T_n = row_off[note + 1] - r0;
    const int64_t t0 = (ft - tile_off[note]) * INGEST_TILE;
    const T *src = in + r0 * (int64_t)n_cols;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int k = ty; k < INGEST_TILE; k += 4) {                 // column c0 + k of the note's block, frames t0 .. t0 + 63
        const int c = c0 + k;
        const int64_t t = t0 + tx;
        if (c < n_cols && t < T_n) s[k][tx] = (float)src[(int64_t)c * T_n + t];
    }
    __syncthreads();
    for (int k = ty; k < INGEST_TILE; k += 4) {                 // row t0 + k, bins c0 .. c0 + 63
        const int64_t t = t0 + k;
        const int c = c0 + tx;
        if (t < T_n && c < n_cols) out[(r0 + t) * ld + c] = s[tx][k];
    }
}

int launch_ingest_rows(goofer_ctx *ctx, const void *in, int in_f64, const int64_t *row_off, const int64_t *tile_off, int n_notes,
                       int64_t total_tiles, int n_cols, float *out, int ld, hipStream_t st)
{
    if (total_tiles <= 0 || n_notes <= 0) return GOOFER_OK;
    const int col_tiles = (n_cols + INGEST_TILE - 1) / INGEST_TILE;
    const int64_t blocks = total_tiles * col_tiles;
    if (blocks > 0x7fffffffLL) return goofer_fail(ctx, GOOFER_EINVAL, "envelope ingest: %lld tiles in one call", (long long)blocks);
    if (in_f64)
        hipLaunchKernelGGL(k_ingest_rows<double>, dim3((unsigned)blocks), dim3(256), 0, st, (const double *)in, row_off, tile_off, n_notes,
                           n_cols, col_tiles, out, ld);
    else
        hipLaunchKernelGGL(k_ingest_rows<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float *)in, row_off, tile_off, n_notes,
                           n_cols, col_tiles, out, ld);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

// ---------------------------------------------------------------------------------------------
// gf.synthesize's time stretch for a ragged batch (GOOFER.py:1019-1057): per note concat(x[:a], stretch_feature(x[a:b], factor),
// x[b:]) of the two envelope matrices (frame axis) and of f0 and the mask (sample axis), in one launch.  The stretched middle is
// k_lerp_axis0's arithmetic (lerp_locate / lerp_value); head and tail are copies.  Blocks [0, row_blocks) take four output
// rows each (a wave per row, both matrices), the rest 256 output samples each (f0 and mask): a 1-D grid, so neither axis has a
// row limit.
struct stretch_axis {
    const int64_t *off_in, *off_out, *cut;   // [n + 1] input / output CSR, [2 n] (a, b) per note
};

// Output element g of note `note` on an axis: its input index, or (for the stretched middle) the located point in the region.
__device__ __forceinline__ int64_t stretch_src(const stretch_axis &ax, int note, int64_t g, lerp_pt &pt, int64_t &R_in, bool &mid)
{
    const int64_t i0 = ax.off_in[note], o0 = ax.off_out[note];
    const int64_t a = ax.cut[2 * note], b = ax.cut[2 * note + 1];
    const int64_t m = (ax.off_out[note + 1] - o0) - a - (ax.off_in[note + 1] - i0 - b);
    const int64_t l = g - o0;
    mid = false;
    if (l < a) return i0 + l;
    if (l >= a + m) return i0 + b + (l - a - m);
    R_in = b - a;
    const double step_in = R_in > 1 ? 1.0 / (double)(R_in - 1) : 0.0, step_out = m > 1 ? 1.0 / (double)(m - 1) : 0.0;
    pt = lerp_locate(l - a, R_in, m, step_in, step_out);
    mid = true;
    return i0 + a;                                            // first row of the region
}

__global__ __launch_bounds__(256) void k_stretch_ragged(stretch_axis rows, stretch_axis samples, int n_notes, int64_t row_blocks,
                                                        int64_t rows_out, int64_t samples_out, int n_cols, int ld,
                                                        const float *__restrict__ env_h, const float *__restrict__ env_n,
                                                        float *__restrict__ env_h_out, float *__restrict__ env_n_out,
                                                        const float *__restrict__ f0, const float *__restrict__ mask,
                                                        float *__restrict__ f0_out, float *__restrict__ mask_out)
{
    lerp_pt pt;
    int64_t R_in = 0;
    bool mid;
    if ((int64_t)blockIdx.x < row_blocks) {
        const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        if (r >= rows_out) return;
        const int lane = threadIdx.x & 63;
        const int note = csr_note(rows.off_out, n_notes, r);
        const int64_t src = stretch_src(rows, note, r, pt, R_in, mid);
        for (int c = lane; c < n_cols; c += WAVE) {
            env_h_out[r * ld + c] = mid ? lerp_value(pt, env_h + src * ld + c, ld, R_in) : env_h[src * ld + c];
            env_n_out[r * ld + c] = mid ? lerp_value(pt, env_n + src * ld + c, ld, R_in) : env_n[src * ld + c];
        }
        return;
    }
    const int64_t g = ((int64_t)blockIdx.x - row_blocks) * 256 + threadIdx.x;
    if (g >= samples_out) return;
    const int note = csr_note(samples.off_out, n_notes, g);
    const int64_t src = stretch_src(samples, note, g, pt, R_in, mid);
    f0_out[g] = mid ? lerp_value(pt, f0 + src, 1, R_in) : f0[src];
    mask_out[g] = mid ? lerp_value(pt, mask + src, 1, R_in) : mask[src];
}

int launch_stretch_ragged(goofer_ctx *ctx, const int64_t *row_off_in, const int64_t *row_off_out, const int64_t *row_cut,
                          const int64_t *sample_off_in, const int64_t *sample_off_out, const int64_t *sample_cut, int n_notes,
                          int64_t rows_out, int64_t samples_out, int n_cols, int ld, const float *env_h, const float *env_n,
                          float *env_h_out, float *env_n_out, const float *f0, const float *mask, float *f0_out, float *mask_out,
                          hipStream_t st)
{
    if (n_notes <= 0 || (rows_out <= 0 && samples_out <= 0)) return GOOFER_OK;
    const int64_t row_blocks = (rows_out + 3) / 4, blocks = row_blocks + (samples_out + 255) / 256;
    if (blocks > 0x7fffffffLL) return goofer_fail(ctx, GOOFER_EINVAL, "ragged stretch: %lld blocks in one call", (long long)blocks);
    stretch_axis rows{row_off_in, row_off_out, row_cut}, samples{sample_off_in, sample_off_out, sample_cut};
    hipLaunchKernelGGL(k_stretch_ragged, dim3((unsigned)blocks), dim3(256), 0, st, rows, samples, n_notes, row_blocks, rows_out,
                       samples_out, n_cols, ld, env_h, env_n, env_h_out, env_n_out, f0, mask, f0_out, mask_out);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}
