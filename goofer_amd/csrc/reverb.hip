// The convolution reverb on the device (gfx950): every signal of a ragged batch convolved with one impulse response of up to
// 2^18 taps by uniformly partitioned overlap-save, out = dry x + wet (h * x delayed by pre).  The definition (ranges, n_out,
// tolerance) is in include/goofer_hip.h; the host half, goofer_host_reverb_plan (planner.hip), makes the output CSR, the
// per-signal block CSR and the table of runs.
//
// The block is B = 1024 samples and the transform 2 B real points: the complex 1024-point transform a wave owns in fft_core.h
// (wave_fft<1024>) between the real-input stages fft.hip uses (rfft_bin / irfft_pre), here with a rectangular window and zeros
// outside the signal instead of reflect padding.  A spectrum row is B float2: bins 1 .. B - 1, and in slot 0 the two real bins
// (DC, Nyquist) side by side, which multiply element by element.  Blocks are counted from each signal's own start, so a signal
// gets the same bits alone as anywhere in a batch.
//   goofer_reverb_ir   once per impulse response: the twiddle tables, then partition p = h[p B .. (p + 1) B) and B zeros
//                      transformed to H[p], and one "live" byte per partition (0: every tap is zero, the row is exact zeros)
//   A  k_reverb_fwd    a workgroup per run of up to 32 blocks of one signal, a wave per block: X[j] = the transform of
//                      x[(j - 1) B - pre .. (j + 1) B - pre) — the pre-delay is an index shift
//   B  k_reverb_mac    Y[b] = sum_p X[b - p] H[p].  A workgroup takes one slice of 64 bins, stages that slice of every H[p] in LDS
//                      once (P x 64 x 8 bytes: 128 KiB at the most; lane = bin, so a wave reads 512 contiguous bytes per
//                      ds_read_b64, no bank conflict) and walks runs with it: four waves per run, each with 8 output blocks
//                      as accumulators in registers, the input rows b - P + 1 .. b streamed past them once, ascending, i.e.
//                      p descending: the order of the sum is the same for every output block wherever it lies.  Up to 64
//                      partitions: 256 threads, a run at a time; above: 1024 threads, four runs at a time, and a register
//                      ring for the H values of the steady rows.  fp32 complex FMAs, no atomics.
//   C  k_reverb_inv    a wave per block: Y[b] back, the last B samples kept, out = dry x + wet c stored once per sample of
//                      [0, n_out), the tail included
// wet == 0 runs no transform: one kernel writes dry x and the tail's zeros (dry == 1: the input's bits).
// No workgroup waits for another; three launches in stream order with both spectra in the caller's scratch (16 bytes a sample).
#include "fft_core.h"
#include "launchers.h"

#define RV_B GOOFER_REVERB_BLOCK
#define RV_T GOOFER_REVERB_RUN                          // blocks per run: one workgroup
#define RV_TW (RV_T / 4)                                // output blocks a wave of k_reverb_mac accumulates
#define RV_SLICE 64                                     // bins per workgroup of k_reverb_mac: one per lane
#define RV_SLICES (RV_B / RV_SLICE)
#define RV_MAC_BIG 64                                   // k_reverb_mac: above this many partitions, 16 waves and the register ring
#define RV_AHEAD 4                                      // input rows a wave of k_reverb_mac has in flight
#define RV_BUF fft_cfg<RV_B>::BUF
static_assert(RV_B == 1024 && RV_T == 32 && GOOFER_REVERB_MAX_TAPS == 256 * RV_B, "wave_fft<1024>; four waves of eight blocks; 256 partitions, one per thread");
// the impulse-response buffer: tw[B], twh[B / 2 + 1] (padded), live[256], then H[P][B]
#define RV_OFF_TWH (8 * RV_B)
#define RV_OFF_LIVE (RV_OFF_TWH + 8 * 544)
static_assert(RV_OFF_LIVE + 256 == GOOFER_REVERB_IR_HEAD, "layout of the impulse-response buffer");

struct rv_run_t {
    int sig, first, count;                              // signal, first block of the run, blocks
    int64_t xbase, n, obase, n_out, sbase;              // the signal's samples in x / out, its first spectrum row
};

// run `at` of the planner's table; false for anything that is not the planner's (nothing is read or
// written): every index the kernels form below is inside x [total], out [total_out] and the spectra [total_blocks] rows
__device__ __forceinline__ bool rv_run(const int32_t *__restrict__ runs, const int64_t *__restrict__ in_off, const int64_t *__restrict__ out_off,
                                       const int64_t *__restrict__ blk_off, int n, int64_t total, int64_t total_out, int64_t total_blocks,
                                       rv_run_t &r, int64_t at)
{
    r.sig = __builtin_amdgcn_readfirstlane(runs[3 * at]);
    r.first = __builtin_amdgcn_readfirstlane(runs[3 * at + 1]);
    r.count = __builtin_amdgcn_readfirstlane(runs[3 * at + 2]);
    if (r.sig < 0 || r.sig >= n || r.first < 0 || r.count < 1 || r.count > RV_T) return false;
    r.xbase = in_off[r.sig], r.n = in_off[r.sig + 1] - r.xbase;
    r.obase = out_off[r.sig], r.n_out = out_off[r.sig + 1] - r.obase;
    r.sbase = blk_off[r.sig];
    const int64_t nb = blk_off[r.sig + 1] - r.sbase;
    if (r.xbase < 0 || r.n < 0 || r.xbase + r.n > total || r.obase < 0 || r.n_out < 1 || r.n_out >= ((int64_t)1 << 31) ||
        r.obase + r.n_out > total_out || r.sbase < 0 || nb != (r.n_out + RV_B - 1) / RV_B || r.sbase + nb > total_blocks ||
        (int64_t)r.first + r.count > nb)
        return false;
    return true;
}

__device__ __forceinline__ void rv_tables(float2 *s_tw, float2 *s_twh, const float2 *__restrict__ g_tw, const float2 *__restrict__ g_twh)
{
    for (int i = threadIdx.x; i < RV_B; i += blockDim.x) s_tw[i] = g_tw[i];
    for (int i = threadIdx.x; i < RV_B / 2 + 1; i += blockDim.x) s_twh[i] = g_twh[i];
    __syncthreads();
}

// e^{-i pi k / B}, k < B, or its conjugate, from the table of B / 2 + 1 entries mirrored about B / 2 (half_twiddle of fft.hip)
template <bool CONJ> __device__ __forceinline__ float2 rv_half_twiddle(const float2 *twh, int k)
{
    if (k <= RV_B / 2) return CONJ ? cconj(twh[k]) : twh[k];
    return make_float2(-twh[RV_B - k].x, CONJ ? -twh[RV_B - k].y : twh[RV_B - k].y);
}

// even/odd split of bin k < B (rfft_bin of fft.hip): X[k] = (Z[k] + conj Z[B-k]) / 2 - i / 2 e^{-i pi k / B} (Z[k] - conj Z[B-k])
__device__ __forceinline__ float2 rv_bin(const float2 *buf, const float2 *twh, int k)
{
    const float2 zk = buf[lds_pad(k)], zm = buf[lds_pad(k == 0 ? 0 : RV_B - k)];
    const float2 w = rv_half_twiddle<false>(twh, k);
    const float2 A = make_float2(zk.x + zm.x, zk.y - zm.y), B = make_float2(zk.x - zm.x, zk.y + zm.y);
    const float2 C = cmul(w, B);
    return make_float2(0.5f * (A.x + C.y), 0.5f * (A.y - C.x));
}

// the transform in buf -> the packed row: slot 0 = (X[0], X[B]), both real; slot k = X[k]
__device__ __forceinline__ void rv_split_store(const float2 *buf, const float2 *s_twh, float2 *__restrict__ row, int lane)
{
#pragma unroll
    for (int r = 0; r < RV_B / WAVE; ++r) {
        const int k = lane + WAVE * r;
        float2 v = rv_bin(buf, s_twh, k);
        if (k == 0) v = make_float2(buf[0].x + buf[0].y, buf[0].x - buf[0].y);
        row[k] = v;
    }
}

// exp(-2 pi i k / B), k < B, and exp(-i pi k / B), k <= B / 2: what goofer_plan makes for an n_fft of 2 B, here on the device
__global__ __launch_bounds__(256) void k_reverb_tables(float2 *__restrict__ tw, float2 *__restrict__ twh)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    double s, c;
    if (k < RV_B) {
        sincospi(-2.0 * (double)k / (double)RV_B, &s, &c);
        tw[k] = make_float2((float)c, (float)s);
    }
    if (k <= RV_B / 2) {
        sincospi(-(double)k / (double)RV_B, &s, &c);
        twh[k] = make_float2((float)c, (float)s);
    }
}

// A wave per partition.  The partition's taps lie in the second half of its own row (goofer_reverb_ir put them there) and are
// read before the row is written; taps past L are not read.
__global__ __launch_bounds__(256) void k_reverb_ir(unsigned char *__restrict__ ir, int L, int P)
{
    __shared__ float2 s_tw[RV_B], s_twh[RV_B / 2 + 1], s_buf[4 * RV_BUF];
    rv_tables(s_tw, s_twh, reinterpret_cast<const float2 *>(ir), reinterpret_cast<const float2 *>(ir + RV_OFF_TWH));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + wave;
    if (p >= P) return;
    float2 *row = reinterpret_cast<float2 *>(ir + GOOFER_REVERB_IR_HEAD) + (size_t)p * RV_B;
    const float *taps = reinterpret_cast<const float *>(row + RV_B / 2);
    const int left = L - p * RV_B;                       // taps of this partition: min(left, B)
    float2 v[RV_B / WAVE];
    bool some = false;
#pragma unroll
    for (int r = 0; r < RV_B / WAVE; ++r) {
        const int m = lane + WAVE * r;                   // sample pair (2 m, 2 m + 1) of the 2 B-point frame: B taps, B zeros
        const float a = m < RV_B / 2 && 2 * m < left ? taps[2 * m] : 0.0f;
        const float b = m < RV_B / 2 && 2 * m + 1 < left ? taps[2 * m + 1] : 0.0f;
        some = some || a != 0.0f || b != 0.0f;
        v[r] = make_float2(a, b);
    }
    const bool live = __ballot(some) != 0;
    if (lane == 0) ir[RV_OFF_LIVE + p] = live ? 1 : 0;
    if (!live) {
#pragma unroll
        for (int r = 0; r < RV_B / WAVE; ++r) row[lane + WAVE * r] = make_float2(0.0f, 0.0f);
        return;
    }
    float2 *buf = s_buf + wave * RV_BUF;
    wave_fft<RV_B>(v, buf, s_tw, lane);
    rv_split_store(buf, s_twh, row, lane);
}

__global__ __launch_bounds__(256) void k_reverb_fwd(const float *__restrict__ x, const int64_t *__restrict__ in_off, const int64_t *__restrict__ out_off,
                                                    const int64_t *__restrict__ blk_off, int n, int64_t total, int64_t total_out,
                                                    int64_t total_blocks, const int32_t *__restrict__ runs, int pre,
                                                    const float2 *__restrict__ g_tw, const float2 *__restrict__ g_twh, float2 *__restrict__ X)
{
    __shared__ float2 s_tw[RV_B], s_twh[RV_B / 2 + 1], s_buf[4 * RV_BUF];
    rv_run_t run;
    if (!rv_run(runs, in_off, out_off, blk_off, n, total, total_out, total_blocks, run, blockIdx.x)) return;
    rv_tables(s_tw, s_twh, g_tw, g_twh);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float2 *buf = s_buf + wave * RV_BUF;
    const float *__restrict__ xs = x + run.xbase;
    for (int t = wave; t < run.count; t += 4) {
        const int64_t j = run.first + t;
        const int64_t start = (j - 1) * RV_B - pre;          // the frame's first sample, in the signal's coordinates
        float2 v[RV_B / WAVE];
        if (start >= 0 && start + 2 * RV_B <= run.n) {
#pragma unroll
            for (int r = 0; r < RV_B / WAVE; ++r) {
                const int m = lane + WAVE * r;
                v[r] = make_float2(xs[start + 2 * m], xs[start + 2 * m + 1]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < RV_B / WAVE; ++r) {
                const int64_t i = start + 2 * (lane + WAVE * r);
                v[r] = make_float2(i >= 0 && i < run.n ? xs[i] : 0.0f, i + 1 >= 0 && i + 1 < run.n ? xs[i + 1] : 0.0f);
            }
        }
        wave_fft<RV_B>(v, buf, s_tw, lane);
        rv_split_store(buf, s_twh, X + (run.sbase + j) * RV_B, lane);
        wave_lds_sync();                                      // the next block's first pass overwrites buf
    }
}

extern __shared__ __align__(16) unsigned char rv_smem[];

// acc += x h: complex, or for the lane that holds slot 0 of a row (DC) the two real bins element by element.  PACKED: two packed
// FMAs (cmul of fft_core.h with the accumulator as the addend): t = (x.x h.x + acc.x, x.x h.y + acc.y), then (-x.y h.y + t.x,
// x.y h.x + t.y) — the roundings of the four fmaf calls of the other form, which the small shape of k_reverb_mac takes.
template <bool DC, bool PACKED> __device__ __forceinline__ float2 rv_cfma(float2 x, float2 h, float2 acc, bool slot0)
{
    float2 g;
    if constexpr (PACKED) {
        const v2f_t vx = {x.x, x.y}, vh = {h.x, h.y}, va = {acc.x, acc.y};
        v2f_t t, r;
        asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(t) : "v"(vx), "v"(vh), "v"(va));
        asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(vx), "v"(vh), "v"(t));
        g = make_float2(r.x, r.y);
    } else {
        g.x = fmaf(-x.y, h.y, fmaf(x.x, h.x, acc.x));
        g.y = fmaf(x.y, h.x, fmaf(x.x, h.y, acc.y));
    }
    if (DC && slot0) g = make_float2(fmaf(x.x, h.x, acc.x), fmaf(x.y, h.y, acc.y));
    return g;
}

// Input rows qa .. qb of one wave's pass, ascending, every product tested against the range of p and the live mask (m0 .. m3: bit
// p set where partition p takes part): RV_AHEAD rows at a time, the next ones in flight under these rows' products — a wave has
// 8 bytes a lane per load.
template <bool DC, bool PACKED>
__device__ __forceinline__ void rv_rows_checked(float2 (&acc)[RV_TW], const float2 *__restrict__ xp, const float2 *sH, int b0, int P,
                                                uint64_t m0, uint64_t m1, uint64_t m2, uint64_t m3, int qa, int qb, int lane)
{
    float2 cur[RV_AHEAD], nxt[RV_AHEAD];
#pragma unroll
    for (int u = 0; u < RV_AHEAD; ++u) cur[u] = qa + u <= qb ? xp[(int64_t)(qa + u) * RV_B] : make_float2(0.0f, 0.0f);
    for (int q0 = qa; q0 <= qb; q0 += RV_AHEAD) {
#pragma unroll
        for (int u = 0; u < RV_AHEAD; ++u)
            nxt[u] = q0 + RV_AHEAD + u <= qb ? xp[(int64_t)(q0 + RV_AHEAD + u) * RV_B] : make_float2(0.0f, 0.0f);
#pragma unroll
        for (int u = 0; u < RV_AHEAD; ++u) {
            const int q = q0 + u;
            if (q > qb) break;
#pragma unroll
            for (int t = 0; t < RV_TW; ++t) {
                const int p = b0 + t - q;                     // (wave-uniform)
                if (p < 0 || p >= P) continue;
                const uint64_t w = p < 128 ? (p < 64 ? m0 : m1) : (p < 192 ? m2 : m3);
                if (!((w >> (p & 63)) & 1)) continue;
                acc[t] = rv_cfma<DC, PACKED>(cur[u], sH[p * RV_SLICE + lane], acc[t], lane == 0);
            }
        }
#pragma unroll
        for (int u = 0; u < RV_AHEAD; ++u) cur[u] = nxt[u];
    }
}

// One wave: output blocks b0 .. b0 + cnt - 1 of a signal, bin `lane` of the slice.  xp: slot (slice, lane) of the signal's row
// 0; all_live: every partition takes part.  The input rows go past the accumulators in ascending order, whatever path a row
// takes.  RING false (the small shape): every row on the checked path.  RING true: a row q in [b0 + 8 - P, b0] reaches a
// partition for every accumulator, p = (b0 - q) + t: eight consecutive rows of the staged slice, seven of them the ones the row
// before used.  Where all partitions are live these rows run in groups of eight with the eight H values in a register ring (H[j]
// in R[j & 7], the group starting where (b0 - q) & 7 == 7, so that every index is static): one LDS read per row instead of eight,
// no test per product.  The rows in front of and behind the groups, and every row when a partition is dead, take the checked path.
template <bool DC, bool RING>
__device__ __forceinline__ void rv_mac_wave(const float2 *__restrict__ xp, const float2 *sH, float2 *__restrict__ yp, int b0, int cnt, int P,
                                            uint64_t m0, uint64_t m1, uint64_t m2, uint64_t m3, bool all_live, int lane)
{
    float2 acc[RV_TW];
#pragma unroll
    for (int t = 0; t < RV_TW; ++t) acc[t] = make_float2(0.0f, 0.0f);
    const int q_lo = b0 - P + 1 > 0 ? b0 - P + 1 : 0, q_hi = b0 + cnt - 1;
    if constexpr (!RING) {
        rv_rows_checked<DC, false>(acc, xp, sH, b0, P, m0, m1, m2, m3, q_lo, q_hi, lane);
    } else {
        int qf = q_hi + 1, qe = q_hi + 1;                     // the rows that run in groups: [qf, qe)
        if (all_live && P >= RV_TW) {
            int s_lo = b0 + RV_TW - P;
            if (s_lo < q_lo) s_lo = q_lo;
            const int first = s_lo + ((b0 - s_lo + 1) & 7);   // the first row at or behind s_lo with (b0 - q) & 7 == 7
            const int groups = first <= b0 ? (b0 - first + 1) / RV_TW : 0;
            if (groups > 0) qf = first, qe = first + RV_TW * groups;
        }
        rv_rows_checked<DC, true>(acc, xp, sH, b0, P, m0, m1, m2, m3, q_lo, qf - 1, lane);
        if (qf < qe) {
            static_assert(RV_TW == 8, "a ring of eight");
            float2 R[8], cur[8], nxt[8];
            int d = b0 - qf;                                  // (d & 7) == 7; 0 <= d - 7 and d + 7 <= P - 1 for every group
#pragma unroll
            for (int t = 1; t < 8; ++t) R[t - 1] = sH[(d + t) * RV_SLICE + lane];  // H[d + t] at R[(d + t) & 7]
#pragma unroll
            for (int u = 0; u < 8; ++u) cur[u] = xp[(int64_t)(qf + u) * RV_B];
            for (int q0 = qf; q0 < qe; q0 += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) nxt[u] = q0 + 8 + u < qe ? xp[(int64_t)(q0 + 8 + u) * RV_B] : make_float2(0.0f, 0.0f);
#pragma unroll
                for (int s = 0; s < 8; ++s) {                 // row q0 + s: partitions d - s .. d - s + 7
                    R[7 - s] = sH[(d - s) * RV_SLICE + lane]; // the new one replaces H[d - s + 8], which no later row needs
#pragma unroll
                    for (int t = 0; t < 8; ++t) acc[t] = rv_cfma<DC, true>(cur[s], R[(7 - s + t) & 7], acc[t], lane == 0);
                }
                d -= 8;
#pragma unroll
                for (int u = 0; u < 8; ++u) cur[u] = nxt[u];
            }
        }
        rv_rows_checked<DC, true>(acc, xp, sH, b0, P, m0, m1, m2, m3, qe, q_hi, lane);
    }
#pragma unroll
    for (int t = 0; t < RV_TW; ++t)
        if (t < cnt) yp[(int64_t)(b0 + t) * RV_B] = acc[t];
}

// Two shapes, chosen by the launcher from P.  THREADS 256, RING false: four waves, a run at a time, every row on the checked path,
// in few enough registers for eight waves a SIMD to stream the input rows — right while the slice is small and the kernel lives
// on memory.  THREADS 1024, RING true: sixteen waves, four runs at a time on one staged slice, the steady rows through the
// register ring — a long impulse response leaves LDS for one workgroup per CU, and four waves on a CU hide no latency.  What
// each shape costs on the other's ground is in DESIGN.md.
template <int THREADS, bool RING>
__global__ __launch_bounds__(THREADS) void k_reverb_mac(const int64_t *__restrict__ in_off, const int64_t *__restrict__ out_off,
                                                               const int64_t *__restrict__ blk_off, int n, int64_t total, int64_t total_out,
                                                               int64_t total_blocks, const int32_t *__restrict__ runs, int64_t n_runs, int P,
                                                               const unsigned char *__restrict__ live, int skip, const float2 *__restrict__ H,
                                                               const float2 *__restrict__ X, float2 *__restrict__ Y)
{
    __shared__ uint64_t s_mask[4];
    float2 *sH = reinterpret_cast<float2 *>(rv_smem);         // [P][64]: the slice of every partition
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int slice = blockIdx.y;
    for (int i = tid; i < P * RV_SLICE; i += THREADS) sH[i] = H[(size_t)(i >> 6) * RV_B + slice * RV_SLICE + (i & 63)];
    if (wave < 4) {                                           // thread p < 256 speaks for partition p
        const uint64_t mine = __ballot(tid < P && (!skip || live[tid < P ? tid : 0] != 0));
        if (lane == 0) s_mask[wave] = mine;
    }
    __syncthreads();
    uint64_t m[4];
    bool all_live = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t v = s_mask[k];
        m[k] = ((uint64_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
        const int in_k = P - 64 * k < 0 ? 0 : (P - 64 * k > 64 ? 64 : P - 64 * k);       // partitions of word k
        all_live = all_live && m[k] == (in_k == 64 ? ~(uint64_t)0 : ((uint64_t)1 << in_k) - 1);
    }
    // the staged slice serves any run: the workgroup walks the runs, G = THREADS / 256 at a time, waves 4 g .. 4 g + 3 on run
    // G blockIdx.x + g and on every G gridDim.x-th behind it (no barrier from here on)
    constexpr int G = THREADS / 256;
    const int t0 = (wave & 3) * RV_TW;
    for (int64_t r = G * (int64_t)blockIdx.x + (wave >> 2); r < n_runs; r += G * (int64_t)gridDim.x) {
        rv_run_t run;
        if (!rv_run(runs, in_off, out_off, blk_off, n, total, total_out, total_blocks, run, r) || t0 >= run.count) continue;
        const int cnt = run.count - t0 < RV_TW ? run.count - t0 : RV_TW;
        const size_t at = (size_t)run.sbase * RV_B + slice * RV_SLICE + lane;
        if (slice == 0) rv_mac_wave<true, RING>(X + at, sH, Y + at, run.first + t0, cnt, P, m[0], m[1], m[2], m[3], all_live, lane);
        else rv_mac_wave<false, RING>(X + at, sH, Y + at, run.first + t0, cnt, P, m[0], m[1], m[2], m[3], all_live, lane);
    }
}

__global__ __launch_bounds__(256) void k_reverb_inv(const float *__restrict__ x, const int64_t *__restrict__ in_off, const int64_t *__restrict__ out_off,
                                                    const int64_t *__restrict__ blk_off, int n, int64_t total, int64_t total_out,
                                                    int64_t total_blocks, const int32_t *__restrict__ runs, float dry, float wet,
                                                    const float2 *__restrict__ g_tw, const float2 *__restrict__ g_twh, const float2 *__restrict__ Y,
                                                    float *__restrict__ out)
{
    __shared__ float2 s_tw[RV_B], s_twh[RV_B / 2 + 1], s_buf[4 * RV_BUF];
    rv_run_t run;
    if (!rv_run(runs, in_off, out_off, blk_off, n, total, total_out, total_blocks, run, blockIdx.x)) return;
    rv_tables(s_tw, s_twh, g_tw, g_twh);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float2 *buf = s_buf + wave * RV_BUF;
    const float *__restrict__ xs = x + run.xbase;
    float *__restrict__ ys = out + run.obase;
    const float inv_m = 0.5f / (float)RV_B;                   // 1 / B of the transform and the 1 / 2 irfft_pre leaves out
    const bool pair_x = ((uintptr_t)xs & 7) == 0, pair_y = ((uintptr_t)ys & 7) == 0;   // a pair of samples per load / store (uniform)
    for (int t = wave; t < run.count; t += 4) {
        const int64_t b = run.first + t;
        const float2 *__restrict__ row = Y + (run.sbase + b) * RV_B;
        float2 v[RV_B / WAVE];
#pragma unroll
        for (int r = 0; r < RV_B / WAVE; ++r) {
            const int k = lane + WAVE * r;
            float2 xk = row[k], xm = row[(RV_B - k) & (RV_B - 1)];
            if (k == 0) { xm = make_float2(xk.y, 0.0f); xk.y = 0.0f; }     // slot 0: (DC, Nyquist)
            v[r] = irfft_pre(xk, xm, rv_half_twiddle<true>(s_twh, k));
        }
        wave_fft<RV_B>(v, buf, s_tw, lane);
#pragma unroll
        for (int r = RV_B / WAVE / 2; r < RV_B / WAVE; ++r) {  // the last B samples of the frame: pairs B / 2 .. B - 1
            const int m = lane + WAVE * r;
            const float2 z = buf[lds_pad(m)];
            const float c0 = z.x * inv_m, c1 = -z.y * inv_m;
            const int64_t i = b * RV_B + 2 * (m - RV_B / 2);  // (even)
            float2 xv = make_float2(0.0f, 0.0f);
            if (pair_x && i + 1 < run.n) xv = *reinterpret_cast<const float2 *>(xs + i);
            else xv = make_float2(i < run.n ? xs[i] : 0.0f, i + 1 < run.n ? xs[i + 1] : 0.0f);
            const float2 yv = make_float2(dry * xv.x + wet * c0, dry * xv.y + wet * c1);
            if (pair_y && i + 1 < run.n_out) *reinterpret_cast<float2 *>(ys + i) = yv;
            else {
                if (i < run.n_out) ys[i] = yv.x;
                if (i + 1 < run.n_out) ys[i + 1] = yv.y;
            }
        }
        wave_lds_sync();
    }
}

// wet == 0: dry x over the signal (dry == 1: its bits), exact zeros over the tail
__global__ __launch_bounds__(256) void k_reverb_dry(const float *__restrict__ x, const int64_t *__restrict__ in_off, const int64_t *__restrict__ out_off,
                                                    const int64_t *__restrict__ blk_off, int n, int64_t total, int64_t total_out,
                                                    int64_t total_blocks, const int32_t *__restrict__ runs, float dry, float *__restrict__ out)
{
    rv_run_t run;
    if (!rv_run(runs, in_off, out_off, blk_off, n, total, total_out, total_blocks, run, blockIdx.x)) return;
    const int64_t i0 = (int64_t)run.first * RV_B;
    int64_t i1 = i0 + (int64_t)run.count * RV_B;
    if (i1 > run.n_out) i1 = run.n_out;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const float v = i < run.n ? x[run.xbase + i] : 0.0f;
        out[run.obase + i] = i < run.n && dry != 1.0f ? dry * v : v;
    }
}

static inline int rv_partitions(int L) { return (L + RV_B - 1) / RV_B; }

int launch_reverb(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, const void *ir, int L, int pre, float dry,
                  float wet, const int64_t *out_off, const int64_t *blk_off, int64_t total_blocks, const int32_t *runs, int64_t n_runs,
                  int64_t total_out, float *out, float2 *X, float2 *Y, hipStream_t st)
{
    if (n <= 0 || total_out <= 0 || n_runs <= 0) return GOOFER_OK;
    const dim3 grid((unsigned)n_runs), wg(256);
    if (wet == 0.0f) {
        hipLaunchKernelGGL(k_reverb_dry, grid, wg, 0, st, x, in_off, out_off, blk_off, n, total, total_out, total_blocks, runs, dry, out);
        LAUNCH_CHECK(ctx);
        return GOOFER_OK;
    }
    const unsigned char *base = (const unsigned char *)ir;
    const float2 *tw = (const float2 *)base, *twh = (const float2 *)(base + RV_OFF_TWH), *H = (const float2 *)(base + GOOFER_REVERB_IR_HEAD);
    const int P = rv_partitions(L);
    const size_t lds = (size_t)P * RV_SLICE * sizeof(float2);
    hipLaunchKernelGGL(k_reverb_fwd, grid, wg, 0, st, x, in_off, out_off, blk_off, n, total, total_out, total_blocks, runs, pre, tw, twh, X);
    LAUNCH_CHECK(ctx);
    // A workgroup stages its slice once and walks runs with it: as many workgroups as the device holds twice over, so that a long
    // impulse response is staged tens of times and not once per run.
    const bool big = P > RV_MAC_BIG;
    const void *fn = big ? (const void *)k_reverb_mac<1024, true> : (const void *)k_reverb_mac<256, false>;
    if (lds > 48 * 1024)
        if (int rc = kernel_allow_max_lds(ctx, fn, GOOFER_REVERB_MAX_TAPS / RV_B * RV_SLICE * (int)sizeof(float2))) return rc;
    int64_t per_slice;
    if (big) {                                                // one workgroup of 1024 threads a CU: its registers, and above 80 KiB its LDS
        int cus = 0;
        HIP_TRY(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        per_slice = (int64_t)(cus > 0 ? cus : 256) * 2 / RV_SLICES;
    } else {
        int waves = 0;
        if (int rc = kernel_resident_waves(ctx, fn, lds, &waves)) return rc;
        per_slice = (int64_t)waves / 4 * 2 / RV_SLICES;
    }
    const int64_t most = big ? (n_runs + 3) / 4 : n_runs;
    per_slice = per_slice < 1 ? 1 : (per_slice > most ? most : per_slice);
    const dim3 mac_grid((unsigned)per_slice, RV_SLICES);
    if (big)
        hipLaunchKernelGGL((k_reverb_mac<1024, true>), mac_grid, dim3(1024), lds, st, in_off, out_off, blk_off, n, total, total_out, total_blocks, runs,
                           n_runs, P, base + RV_OFF_LIVE, ctx->reverb_skip ? 1 : 0, H, (const float2 *)X, Y);
    else
        hipLaunchKernelGGL((k_reverb_mac<256, false>), mac_grid, wg, lds, st, in_off, out_off, blk_off, n, total, total_out, total_blocks, runs,
                           n_runs, P, base + RV_OFF_LIVE, ctx->reverb_skip ? 1 : 0, H, (const float2 *)X, Y);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_reverb_inv, grid, wg, 0, st, x, in_off, out_off, blk_off, n, total, total_out, total_blocks, runs, dry, wet, tw, twh,
                       (const float2 *)Y, out);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

extern "C" int goofer_reverb_ir(goofer_ctx *ctx, const float *h, int L, void *ir, int64_t ir_bytes, void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (L < 1 || L > GOOFER_REVERB_MAX_TAPS)
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_reverb_ir: %d taps, 1 to %d are taken", L, GOOFER_REVERB_MAX_TAPS);
    if (!h || !ir || ((uintptr_t)h & 3) || ((uintptr_t)ir & 15)) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_reverb_ir: null or misaligned pointer (h on 4 bytes, ir on 16)");
    if (ir_bytes < (int64_t)GOOFER_REVERB_IR_BYTES(L))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_reverb_ir: ir of %lld bytes, %lld needed", (long long)ir_bytes, (long long)GOOFER_REVERB_IR_BYTES(L));
    for (int k = 0; k < L; ++k)
        if (!(h[k] - h[k] == 0.0f)) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_reverb_ir: tap %d is not finite", k);
    hipStream_t st = (hipStream_t)stream;
    unsigned char *base = (unsigned char *)ir;
    const int P = rv_partitions(L), whole = L / RV_B;
    // partition p's taps into the second half of its own row, where k_reverb_ir reads them before it writes the row
    unsigned char *rows = base + GOOFER_REVERB_IR_HEAD + sizeof(float2) * RV_B / 2;
    if (whole)
        HIP_TRY(ctx, hipMemcpy2DAsync(rows, sizeof(float2) * RV_B, h, sizeof(float) * RV_B, sizeof(float) * RV_B, (size_t)whole, hipMemcpyHostToDevice, st));
    if (L > whole * RV_B)
        HIP_TRY(ctx, hipMemcpyAsync(rows + sizeof(float2) * RV_B * (size_t)whole, h + (size_t)whole * RV_B, sizeof(float) * (size_t)(L - whole * RV_B),
                                    hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                   // h is the caller's host memory: theirs again when this returns
    HIP_TRY(ctx, hipMemsetAsync(base + RV_OFF_LIVE, 0, 256, st));
    hipLaunchKernelGGL(k_reverb_tables, dim3(RV_B / 256), dim3(256), 0, st, (float2 *)base, (float2 *)(base + RV_OFF_TWH));
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_reverb_ir, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, st, base, L, P);
    LAUNCH_CHECK(ctx);
    return GOOFER_OK;
}

extern "C" int goofer_reverb(goofer_ctx *ctx, const float *x, const int64_t *in_off, int n, int64_t total, const void *ir, int L, int pre,
                             int tail, float dry, float wet, const int64_t *out_off, const int64_t *blk_off, int64_t total_blocks,
                             const int32_t *runs, int64_t n_runs, int64_t total_out, float *out, void *scratch, int64_t *scratch_bytes,
                             void *stream)
{
    if (!ctx) return GOOFER_EINVAL;
    if (int rc = check_counts(ctx, "goofer_reverb", n, total, n_runs)) return rc;
    if (L < 1 || L > GOOFER_REVERB_MAX_TAPS || pre < 0 || pre > GOOFER_REVERB_MAX_PREDELAY || !(dry - dry == 0.0f) || !(wet - wet == 0.0f))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_reverb: %d taps (1 to %d), a pre-delay of %d samples (0 to %d), dry %g and wet %g (finite)",
                           L, GOOFER_REVERB_MAX_TAPS, pre, GOOFER_REVERB_MAX_PREDELAY, (double)dry, (double)wet);
    // what goofer_host_reverb_plan makes: every signal with samples grows by the tail; ceil(n_out / B) blocks and ceil(blocks / T) runs each
    const int64_t grow = tail ? (int64_t)pre + L - 1 : 0;
    const int64_t least_b = (total_out + RV_B - 1) / RV_B, least_r = (total_blocks + RV_T - 1) / RV_T;
    if (total_out < total || total_out > total + (int64_t)n * grow || total_blocks < least_b || total_blocks > least_b + n || n_runs < least_r ||
        n_runs > least_r + n || n_runs >= ((int64_t)1 << 31))
        return goofer_fail(ctx, GOOFER_EINVAL, "goofer_reverb: %lld output samples in %lld blocks and %lld runs for %lld samples in %d signals is not a "
                           "geometry of goofer_host_reverb_plan", (long long)total_out, (long long)total_blocks, (long long)n_runs, (long long)total, n);
    if (!scratch_bytes) return goofer_fail(ctx, GOOFER_EINVAL, "goofer_reverb: null pointer (scratch_bytes)");
    float2 *X = nullptr, *Y = nullptr;
    auto carve = [&](arena &a) {
        if (wet == 0.0f) return;                               // no transform: no spectra
        X = a.take<float2>((size_t)total_blocks * RV_B);
        Y = a.take<float2>((size_t)total_blocks * RV_B);
    };
    if (scratch) {
        if (n > 0 && total_out > 0 && (!in_off || !out_off || !blk_off || !runs || !out || (total > 0 && !x) || (wet != 0.0f && !ir)))
            return goofer_fail(ctx, GOOFER_EINVAL, "goofer_reverb: null pointer");
        if (int rc = check_aligned(ctx, "goofer_reverb", "x, runs and out", {x, runs, out}, "in_off, out_off, blk_off, ir and scratch",
                                   {in_off, out_off, blk_off, ir, scratch}))
            return rc;
        if (total > 0 && total_out > 0 && (uintptr_t)out < (uintptr_t)(x + total) && (uintptr_t)x < (uintptr_t)(out + total_out))
            return goofer_fail(ctx, GOOFER_EINVAL, "goofer_reverb: out overlaps x (blocks read x again: not in place)");
    }
    int rc = caller_scratch(ctx, scratch, scratch_bytes, "goofer_reverb", carve);
    if (rc || !scratch) return rc;
    return launch_reverb(ctx, x, in_off, n, total, ir, L, pre, dry, wet, out_off, blk_off, total_blocks, runs, n_runs, total_out, out, X, Y,
                         (hipStream_t)stream);
}
