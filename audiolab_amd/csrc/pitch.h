// Pitch shifting of a stem on the GPU: a phase vocoder with identity phase locking stretches the signal by r = 2^(s/12) at constant
// pitch, a Kaiser-windowed sinc resamples the stretched signal back to its original length.  The reference's "transpose the song" path
// (wrappers/merge.py:125-127 -> util/audio_track.py:603-694) shells out to ffmpeg's rubberband filter; this is a shifter of the project's
// own, parity unpinned, specified in tests/pitch_oracle.py and DESIGN section 4c.  Included at the end of reverb.hip: it runs on that
// file's float64 Stockham passes (fft_pow2_batched).  gfx950 only.
//
// Arithmetic: double precision throughout, one rounding to float32 at the end.  The peak and owner decisions and the wrap() of the phase
// advance are discontinuous, so the operations that feed them are written one IEEE operation at a time and contraction into fused
// multiply-adds is switched off for this header: a host restatement in float64 then takes the same side of every tie that is exact in
// the arithmetic (the real DC and Nyquist bins, whose phases are 0 or pi and whose heterodyned advance lands on a multiple of pi).
//
// Stages, per batch of B frames (the workspace is a function of B, not of the track length):
//   1. analysis    gather + window -> batched FFT -> |D|, atan2 -> per frame: peaks, owners, and the per-bin constant of the recurrence
//                  c_u[k] = inc_u[own] + pa_u[k] - pa_u[own]; independent across frames, one workgroup per frame
//   2. recurrence  ps_u[k] = wrap(ps_{u-1}[own_u[k]] + c_u[k]): sequential in u; one workgroup per channel, the previous row in LDS
//                  (two rows, one barrier per frame), own / c of the next frame prefetched into registers; no workgroup waits for another
//   3. synthesis   mag (cos, sin)(ps) as a Hermitian spectrum -> batched inverse FFT -> gather-form overlap-add in ascending frame order
//                  over the window-square envelope into a z segment; the partial sums of the n - hs samples past the last complete one
//                  carry to the next batch
//   4. resampling  of every output sample whose whole reach lies in the z held so far; the segment keeps the reach (up to 2 * 271
//                  samples at r = 4, more than four hops at n_fft 256), not just one frame's overlap
#pragma clang fp contract(off)

namespace {

constexpr int kPvLockThreads = 256;
constexpr int kPvRecThreads = 1024;
constexpr int kPvRecPer = 5;                                                 // ceil(4097 / 1024): bins per thread at n_fft 8192
constexpr double kPvTwoPi = 2.0 * 3.14159265358979323846;
constexpr double kPvPi = 3.14159265358979323846;
constexpr int kPvZeros = 64;                                                 // the published "kaiser_best" design, restated
constexpr double kPvBeta = 14.769656459379492;
constexpr double kPvRolloff = 0.9475937167399596;
constexpr int64_t kPvReachPad = 640;                                         // >= 2 * 64 * 4 / rolloff + 3 complete samples kept for the resampler
constexpr int kPvI0Terms = 30;                                               // (beta^2 / 4)^30 / (30!)^2 = 2e-13 beside I0(beta) = 1.6e5

__host__ __device__ __forceinline__ double pv_wrap(double d) { return d - kPvTwoPi * rint(d / kPvTwoPi); }

// I0(2 sqrt(y)) = sum_k y^k / (k!)^2, all terms positive: Horner from the tail
__host__ __device__ __forceinline__ double pv_i0_series(double y) {
    double s = 1.0;
#pragma unroll
    for (int k = kPvI0Terms; k >= 1; --k) s = 1.0 + (y * (1.0 / ((double)k * (double)k))) * s;
    return s;
}

struct PvGeom {
    int log2n;
    int64_t n, hs, K;
    double r, ha;
    int64_t U, Lz;
    double cut, half, scale;                                                 // c, Z / c, c / I0(beta)
};

int64_t pv_frames(int64_t N, int64_t n, double r) {
    const double ha = (double)(n / 4) / r;
    return (int64_t)ceil((double)N / ha) + 1;
}

bool pv_nfft_ok(int n_fft) { return n_fft >= 256 && n_fft <= 8192 && (n_fft & (n_fft - 1)) == 0; }
bool pv_ratio_ok(double r) { return r >= 0.25 && r <= 4.0; }                 // NaN fails both

PvGeom pv_geom(int64_t N, int n_fft, double r) {
    PvGeom g;
    g.log2n = log2_ceil(n_fft);
    g.n = n_fft;
    g.hs = n_fft / 4;
    g.K = n_fft / 2 + 1;
    g.r = r;
    g.ha = (double)g.hs / r;
    g.U = pv_frames(N, n_fft, r);
    g.Lz = (g.U - 1) * g.hs + g.n / 2;
    g.cut = kPvRolloff * (r > 1.0 ? 1.0 / r : 1.0);
    g.half = (double)kPvZeros / g.cut;
    g.scale = g.cut / pv_i0_series(kPvBeta * kPvBeta / 4.0);
    return g;
}

struct PvLayout {
    int64_t w, a, b, mag, pa, cc, own, state, z0, z1, total, lseg;
};

PvLayout pv_layout(int channels, int64_t n, int64_t B) {
    const int64_t K = n / 2 + 1, hs = n / 4, fr = (int64_t)channels * B;
    auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    PvLayout L;
    L.lseg = B * hs + (n - hs) + kPvReachPad;
    int64_t o = 0;
    L.w = o;     o += up(n * 8);
    L.a = o;     o += up(fr * n * 16);
    L.b = o;     o += up(fr * n * 16);
    L.mag = o;   o += up(fr * K * 8);
    L.pa = o;    o += up((int64_t)channels * (B + 1) * K * 8);
    L.cc = o;    o += up(fr * K * 8);
    L.own = o;   o += up(fr * K * 4);
    L.state = o; o += up((int64_t)channels * K * 8);
    L.z0 = o;    o += up((int64_t)channels * L.lseg * 8);
    L.z1 = o;    o += up((int64_t)channels * L.lseg * 8);
    L.total = o;
    return L;
}

__device__ __forceinline__ int64_t pv_frame_start(int64_t u, double ha) { return (int64_t)floor((double)u * ha); }

__global__ void __launch_bounds__(kRvThreads)
pv_window_kernel(double* __restrict__ w, int64_t n) {
    for (int64_t j = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kRvThreads)
        w[j] = 0.5 - 0.5 * cos(kPvTwoPi * (double)j / (double)n);
}

// frame f = c * nb + b of the batch: z[f][j] = x[c][a_u - n/2 + j] w[j], u = u0 + b; zero outside [0, N)
__global__ void __launch_bounds__(kRvThreads)
pv_gather_kernel(const float* __restrict__ x, int64_t N, int64_t ld, const double* __restrict__ w, cplx* __restrict__ z, int log2n, double ha,
                 int64_t u0, int64_t nb, int64_t frames) {
    const int64_t n = (int64_t)1 << log2n, total = frames << log2n;
    for (int64_t i = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRvThreads) {
        const int64_t f = i >> log2n, j = i & (n - 1), c = f / nb, b = f - c * nb;
        const int64_t s = pv_frame_start(u0 + b, ha) - n / 2 + j;
        double v = 0.0;
        if (s >= 0 && s < N) v = (double)x[c * ld + s] * w[j];
        z[i] = {v, 0.0};
    }
}

// rfft's view of the transform: bins 0 .. n/2, DC and Nyquist real; mag[f][k], pa[c][1 + b][k] in `rows` rows per channel (row 0: the
// last frame of the batch before)
__global__ void __launch_bounds__(kRvThreads)
pv_polar_kernel(const cplx* __restrict__ D, double* __restrict__ mag, double* __restrict__ pa, int log2n, int64_t rows, int64_t nb, int64_t frames) {
    const int64_t n = (int64_t)1 << log2n, K = n / 2 + 1, total = frames * K;
    for (int64_t i = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRvThreads) {
        const int64_t f = i / K, k = i - f * K, c = f / nb, b = f - c * nb;
        cplx d = D[(f << log2n) + k];
        if (k == 0 || k == n / 2) d.y = 0.0;
        mag[i] = hypot(d.x, d.y);
        pa[(c * rows + 1 + b) * K + k] = (d.x == 0.0 && d.y == 0.0) ? 0.0 : atan2(d.y, d.x);
    }
}

__device__ __forceinline__ bool pv_is_peak(const double* m, int64_t k, int64_t K) {
    const double v = m[k];
    const double l1 = k >= 1 ? m[k - 1] : -1.0, l2 = k >= 2 ? m[k - 2] : -1.0;
    const double r1 = k + 1 < K ? m[k + 1] : -1.0, r2 = k + 2 < K ? m[k + 2] : -1.0;
    return v > l1 && v > l2 && v >= r1 && v >= r2;
}

// One workgroup per frame: peaks from the magnitudes, the nearest peak of every bin (the lower one on equal distance), and the constant
// of the recurrence.  Thread t owns the bins [t L, (t + 1) L): a backward pass leaves the nearest peak at or above each bin of the chunk
// in LDS, a forward pass finds the one at or below; the nearest peak outside the chunk comes from the chunks' first / last peaks.
// LDS: K doubles + K ints + 2 * 256 ints (51 KB at n_fft 8192).
__global__ void __launch_bounds__(kPvLockThreads)
pv_lock_kernel(const double* __restrict__ mag, const double* __restrict__ pa, int* __restrict__ own, double* __restrict__ cc, int log2n,
               double ha, int64_t rows, int64_t u0, int64_t nb) {
    const int64_t n = (int64_t)1 << log2n, K = n / 2 + 1, hs = n / 4;
    const int64_t f = blockIdx.x, c = f / nb, b = f - c * nb, u = u0 + b;
    double* m = (double*)alsep_smem;
    int* hi = (int*)(alsep_smem + K * 8);
    int* first = hi + K;
    int* last = first + kPvLockThreads;
    const int t = threadIdx.x;
    const double* pa_u = pa + (c * rows + 1 + b) * K;
    const double* pa_p = pa_u - K;
    int* own_u = own + f * K;
    double* cc_u = cc + f * K;
    if (u == 0) {                                                            // ps_0 = pa_0
        for (int64_t k = t; k < K; k += kPvLockThreads) { own_u[k] = (int)k; cc_u[k] = pa_u[k]; }
        return;
    }
    for (int64_t k = t; k < K; k += kPvLockThreads) m[k] = mag[f * K + k];
    __syncthreads();
    const int64_t L = (K + kPvLockThreads - 1) / kPvLockThreads;
    const int64_t k0 = t * L, k1 = k0 + L < K ? k0 + L : K;
    int nxt = -1, lst = -1;
    for (int64_t k = k1 - 1; k >= k0; --k) {
        if (pv_is_peak(m, k, K)) { nxt = (int)k; if (lst < 0) lst = (int)k; }
        hi[k] = nxt;
    }
    first[t] = nxt;
    last[t] = lst;
    __syncthreads();
    int below = -1, above = -1;
    for (int s = t - 1; s >= 0 && below < 0; --s) below = last[s];
    for (int s = t + 1; s < kPvLockThreads && above < 0; ++s) above = first[s];
    const double da = (double)(pv_frame_start(u, ha) - pv_frame_start(u - 1, ha));
    for (int64_t k = k0; k < k1; ++k) {
        const int h = hi[k] >= 0 ? hi[k] : above;
        if (h == (int)k) below = h;
        int o;
        if (below < 0 && h < 0) o = (int)k;
        else if (below < 0) o = h;
        else if (h < 0) o = below;
        else o = (k - below <= h - k) ? below : h;
        const double om = kPvTwoPi * (double)o / (double)n;
        const double pu = pa_u[o];
        const double inc = (om + pv_wrap(pu - pa_p[o] - om * da) / da) * (double)hs;
        own_u[k] = o;
        cc_u[k] = inc + pa_u[k] - pu;
    }
}

// ps_u[k] = wrap(ps_{u-1}[own_u[k]] + c_u[k]), u = u0 .. u0 + nb, written over c.  One workgroup per channel, the bins spread over its
// threads; the previous row lives in LDS (two rows, so that one barrier per frame separates the reads of row u-1 from the writes of row
// u+1), and the own / c values of frame u+1 are loaded before the barrier of frame u: they do not depend on the recurrence.
// `state` holds the row of the last frame between batches.
__global__ void __launch_bounds__(kPvRecThreads)
pv_recurrence_kernel(const int* __restrict__ own, double* __restrict__ cc, double* __restrict__ state, int64_t K, int64_t u0, int64_t nb) {
    const int64_t c = blockIdx.x;
    const int t = threadIdx.x;
    double* rows = (double*)alsep_smem;
    const int* own_c = own + c * nb * K;
    double* cc_c = cc + c * nb * K;
    double* st = state + c * K;
    int cur = 0;
    if (u0 > 0) {
#pragma unroll
        for (int p = 0; p < kPvRecPer; ++p) { const int64_t k = t + (int64_t)p * kPvRecThreads; if (k < K) rows[k] = st[k]; }
    }
    int o_n[kPvRecPer];
    double c_n[kPvRecPer];
#pragma unroll
    for (int p = 0; p < kPvRecPer; ++p) {
        const int64_t k = t + (int64_t)p * kPvRecThreads;
        o_n[p] = 0; c_n[p] = 0.0;
        if (k < K) { o_n[p] = own_c[k]; c_n[p] = cc_c[k]; }
    }
    __syncthreads();
    for (int64_t b = 0; b < nb; ++b) {
        int o[kPvRecPer];
        double cv[kPvRecPer];
#pragma unroll
        for (int p = 0; p < kPvRecPer; ++p) { o[p] = o_n[p]; cv[p] = c_n[p]; }
        if (b + 1 < nb) {
#pragma unroll
            for (int p = 0; p < kPvRecPer; ++p) {
                const int64_t k = t + (int64_t)p * kPvRecThreads;
                if (k < K) { o_n[p] = own_c[(b + 1) * K + k]; c_n[p] = cc_c[(b + 1) * K + k]; }
            }
        }
        const double* prev = rows + (int64_t)cur * K;
        double* next = rows + (int64_t)(cur ^ 1) * K;
        const bool head = u0 + b == 0;
#pragma unroll
        for (int p = 0; p < kPvRecPer; ++p) {
            const int64_t k = t + (int64_t)p * kPvRecThreads;
            if (k < K) {
                const double v = head ? cv[p] : pv_wrap(prev[o[p]] + cv[p]);
                next[k] = v;
                cc_c[b * K + k] = v;
            }
        }
        cur ^= 1;
        __syncthreads();
    }
    const double* fin = rows + (int64_t)cur * K;
#pragma unroll
    for (int p = 0; p < kPvRecPer; ++p) { const int64_t k = t + (int64_t)p * kPvRecThreads; if (k < K) st[k] = fin[k]; }
}

// the pa row of a batch's last frame -> row 0 of its channel, where the next batch's first frame looks for its predecessor
__global__ void __launch_bounds__(kRvThreads)
pv_carry_pa_kernel(double* __restrict__ pa, int64_t K, int64_t rows, int64_t nb, int channels) {
    const int64_t total = (int64_t)channels * K;
    for (int64_t i = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRvThreads) {
        const int64_t c = i / K, k = i - c * K;
        pa[c * rows * K + k] = pa[(c * rows + nb) * K + k];
    }
}

// the Hermitian spectrum irfft builds from mag exp(i ps): the real parts only of DC and Nyquist
__global__ void __launch_bounds__(kRvThreads)
pv_spectrum_kernel(const double* __restrict__ mag, const double* __restrict__ ps, cplx* __restrict__ S, int log2n, int64_t frames) {
    const int64_t n = (int64_t)1 << log2n, K = n / 2 + 1, total = frames << log2n;
    for (int64_t i = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRvThreads) {
        const int64_t f = i >> log2n, j = i & (n - 1), k = j <= n / 2 ? j : n - j;
        const double m = mag[f * K + k];
        double s, c;
        sincos(ps[f * K + k], &s, &c);
        cplx v = {m * c, m * s};
        if (k == 0 || k == n / 2) v.y = 0.0;
        else if (j > n / 2) v.y = -v.y;
        S[i] = v;
    }
}

// Gather-form overlap-add into the z segment of channel c: dst[j] is z[base_new + j].  Samples below done_old are final and are copied;
// the n - hs samples from done_old on hold the partial sums of the batches before; the frames of this batch are added in ascending order,
// and a sample below done_new is complete and is divided by the envelope of all the frames that cover it.
__global__ void __launch_bounds__(kRvThreads)
pv_overlap_add_kernel(const cplx* __restrict__ Y, const double* __restrict__ w, const double* __restrict__ src, double* __restrict__ dst,
                      int log2n, int64_t lseg, int64_t base_old, int64_t base_new, int64_t done_old, int64_t done_new, int64_t u0, int64_t nb,
                      int64_t U, int channels) {
    const int64_t n = (int64_t)1 << log2n, hs = n / 4, total = (int64_t)channels * lseg;
    const double inv_n = 1.0 / (double)n;
    for (int64_t q = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; q < total; q += (int64_t)gridDim.x * kRvThreads) {
        const int64_t c = q / lseg, j = q - c * lseg, i = base_new + j;
        double acc = 0.0;
        if (i < done_old + (n - hs) && i - base_old < lseg && done_old > 0) acc = src[c * lseg + (i - base_old)];
        if (i >= done_old) {
            const int64_t lo_all = i - n / 2 + hs >= 0 ? (i - n / 2 + hs) / hs : 0;
            int64_t hi_all = (i + n / 2) / hs;
            if (hi_all > U - 1) hi_all = U - 1;
            const int64_t lo = lo_all > u0 ? lo_all : u0, hi = hi_all < u0 + nb - 1 ? hi_all : u0 + nb - 1;
            for (int64_t u = lo; u <= hi; ++u) {
                const int64_t p = i + n / 2 - u * hs;
                acc = acc + w[p] * (Y[((c * nb + (u - u0)) << log2n) + p].x * inv_n);
            }
            if (i < done_new) {
                double env = 0.0;
                for (int64_t u = lo_all; u <= hi_all; ++u) { const double wv = w[i + n / 2 - u * hs]; env = env + wv * wv; }
                acc = acc / (env > 1e-10 ? env : 1.0);
            }
        }
        dst[q] = acc;
    }
}

// out[c][m] = sum_i z[i] g(m r - i), m0 <= m < m1; z[i] = seg[c][i - base]; i in [0, Lz) with |m r - i| <= half
__global__ void __launch_bounds__(kRvThreads)
pv_resample_kernel(const double* __restrict__ seg, int64_t lseg, int64_t base, int64_t Lz, double r, double cut, double half, double scale,
                   float* __restrict__ out, int64_t ld_out, int64_t m0, int64_t m1, int channels) {
    const int64_t span = m1 - m0, total = (int64_t)channels * span;
    for (int64_t q = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; q < total; q += (int64_t)gridDim.x * kRvThreads) {
        const int64_t c = q / span, m = m0 + (q - c * span);
        const double t0 = (double)m * r;
        int64_t lo = (int64_t)ceil(t0 - half), hi = (int64_t)floor(t0 + half);
        if (lo < 0) lo = 0;
        if (hi > Lz - 1) hi = Lz - 1;
        const double* z = seg + c * lseg;
        double acc = 0.0;
        for (int64_t i = lo; i <= hi; ++i) {
            const double t = t0 - (double)i;
            if (fabs(t) > half) continue;
            const double e = t / half, q1 = 1.0 - e * e;
            const double a = kPvPi * (cut * t);
            const double sinc = a == 0.0 ? 1.0 : sin(a) / a;
            const double y = (kPvBeta * kPvBeta / 4.0) * (q1 > 0.0 ? q1 : 0.0);
            acc = acc + z[i - base] * (scale * sinc * pv_i0_series(y));
        }
        out[c * ld_out + m] = (float)acc;
    }
}

// the index of the last z sample output m reads, as the kernel computes it
int64_t pv_reach_hi(int64_t m, const PvGeom& g) {
    int64_t hi = (int64_t)floor((double)m * g.r + g.half);
    return hi > g.Lz - 1 ? g.Lz - 1 : hi;
}

}  // namespace

extern "C" int64_t alsep_pitch_shift_frames(int64_t n, int n_fft, double ratio) {
    if (n < 1 || !pv_nfft_ok(n_fft) || !pv_ratio_ok(ratio)) return -1;
    return pv_frames(n, n_fft, ratio);
}

extern "C" int64_t alsep_pitch_shift_workspace_bytes(int channels, int n_fft, int frames_per_batch, double ratio) {
    if (channels < 1 || !pv_nfft_ok(n_fft) || frames_per_batch < 4 || !pv_ratio_ok(ratio)) return -1;
    return pv_layout(channels, n_fft, frames_per_batch).total;
}

extern "C" int alsep_pitch_shift(alsep_ctx* ctx, const float* x, int channels, int64_t n, int64_t ld, double ratio, int n_fft,
                                 int frames_per_batch, float* out, int64_t ld_out, void* ws, int64_t ws_bytes) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !out || !ws || channels < 1 || n < 1 || ld < n || ld_out < n)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_pitch_shift: bad argument");
    if (!pv_nfft_ok(n_fft) || frames_per_batch < 4 || !pv_ratio_ok(ratio))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_pitch_shift: n_fft %d (a power of two, 256 .. 8192), %d frames per batch (>= 4) or ratio %g (1/4 .. 4)",
                          n_fft, frames_per_batch, ratio);
    const float *x_end = x + ((int64_t)(channels - 1) * ld + n), *out_end = out + ((int64_t)(channels - 1) * ld_out + n);
    if (x < out_end && out < x_end) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_pitch_shift: out overlaps x");
    const PvLayout L = pv_layout(channels, n_fft, frames_per_batch);
    if (ws_bytes < L.total) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_pitch_shift: workspace too small");
    const PvGeom g = pv_geom(n, n_fft, ratio);
    char* base = (char*)ws;
    double* w = (double*)(base + L.w);
    cplx* A = (cplx*)(base + L.a);
    cplx* Bf = (cplx*)(base + L.b);
    double* mag = (double*)(base + L.mag);
    double* pa = (double*)(base + L.pa);
    double* cc = (double*)(base + L.cc);
    int* own = (int*)(base + L.own);
    double* state = (double*)(base + L.state);
    double* zseg[2] = {(double*)(base + L.z0), (double*)(base + L.z1)};
    const dim3 block(kRvThreads);
    const int64_t rows = (int64_t)frames_per_batch + 1;

    hipLaunchKernelGGL(pv_window_kernel, dim3(rv_grid(g.n)), block, 0, ctx->stream, w, g.n);
    ALSEP_LAUNCH_CHECK(ctx, "pv_window_kernel");
    const size_t lock_lds = (size_t)g.K * 12 + 2 * kPvLockThreads * sizeof(int);
    const size_t rec_lds = (size_t)g.K * 16;
    ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)pv_recurrence_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rec_lds));

    int64_t z_base = 0, z_done = 0, m_next = 0;
    int cur = 0;
    for (int64_t u0 = 0; u0 < g.U && m_next < n; u0 += frames_per_batch) {
        const int64_t nb = g.U - u0 < frames_per_batch ? g.U - u0 : frames_per_batch, frames = (int64_t)channels * nb;
        // 1. analysis
        {
        ProfScope prof(ctx, ALSEP_PROF_PITCH_ANALYSIS);
        hipLaunchKernelGGL(pv_gather_kernel, dim3(rv_grid(frames * g.n)), block, 0, ctx->stream, x, n, ld, w, Bf, g.log2n, g.ha, u0, nb, frames);
        ALSEP_LAUNCH_CHECK(ctx, "pv_gather_kernel");
        cplx* D = nullptr;
        if (int rc = fft_pow2_batched(ctx, Bf, A, g.log2n, -1.0, frames, &D)) return rc;
        hipLaunchKernelGGL(pv_polar_kernel, dim3(rv_grid(frames * g.K)), block, 0, ctx->stream, D, mag, pa, g.log2n, rows, nb, frames);
        ALSEP_LAUNCH_CHECK(ctx, "pv_polar_kernel");
        hipLaunchKernelGGL(pv_lock_kernel, dim3((unsigned)frames), dim3(kPvLockThreads), lock_lds, ctx->stream, mag, pa, own, cc, g.log2n, g.ha, rows, u0, nb);
        ALSEP_LAUNCH_CHECK(ctx, "pv_lock_kernel");
        }
        // 2. the recurrence
        {
        ProfScope prof(ctx, ALSEP_PROF_PITCH_RECURRENCE);
        hipLaunchKernelGGL(pv_recurrence_kernel, dim3(channels), dim3(kPvRecThreads), rec_lds, ctx->stream, own, cc, state, g.K, u0, nb);
        ALSEP_LAUNCH_CHECK(ctx, "pv_recurrence_kernel");
        }
        // 3. synthesis
        const int64_t ue = u0 + nb;
        {
        ProfScope prof(ctx, ALSEP_PROF_PITCH_SYNTHESIS);
        hipLaunchKernelGGL(pv_spectrum_kernel, dim3(rv_grid(frames * g.n)), block, 0, ctx->stream, mag, cc, A, g.log2n, frames);
        ALSEP_LAUNCH_CHECK(ctx, "pv_spectrum_kernel");
        cplx* Y = nullptr;
        if (int rc = fft_pow2_batched(ctx, A, Bf, g.log2n, +1.0, frames, &Y)) return rc;
        const int64_t done_new = ue < g.U ? ue * g.hs - g.n / 2 : g.Lz;
        // the segment restarts just below the reach of the next output sample
        int64_t base_new = (int64_t)floor((double)m_next * g.r - g.half) - 2;
        if (base_new < 0) base_new = 0;
        if (base_new < z_base) base_new = z_base;
        if ((ue < g.U ? done_new + (g.n - g.hs) : g.Lz) - base_new > L.lseg)
            return alsep_fail(ctx, ALSEP_ERR_STATE, "alsep_pitch_shift: the z segment does not hold the resampler's reach");
        hipLaunchKernelGGL(pv_overlap_add_kernel, dim3(rv_grid(channels * L.lseg)), block, 0, ctx->stream, Y, w, zseg[cur], zseg[cur ^ 1], g.log2n,
                           L.lseg, z_base, base_new, z_done, done_new, u0, nb, g.U, channels);
        ALSEP_LAUNCH_CHECK(ctx, "pv_overlap_add_kernel");
        cur ^= 1;
        z_base = base_new;
        z_done = done_new;
        hipLaunchKernelGGL(pv_carry_pa_kernel, dim3(rv_grid(channels * g.K)), block, 0, ctx->stream, pa, g.K, rows, nb, channels);
        ALSEP_LAUNCH_CHECK(ctx, "pv_carry_pa_kernel");
        }
        // 4. resampling: every output whose reach ends below z_done
        int64_t m1;
        if (ue >= g.U) {
            m1 = n;
        } else {
            m1 = (int64_t)floor(((double)z_done - 1.0 - g.half) / g.r);
            if (m1 < m_next) m1 = m_next;
            if (m1 > n) m1 = n;
            while (m1 > m_next && pv_reach_hi(m1 - 1, g) >= z_done) --m1;
            while (m1 < n && pv_reach_hi(m1, g) < z_done) ++m1;
        }
        if (m1 > m_next) {
            ProfScope prof(ctx, ALSEP_PROF_PITCH_RESAMPLE);
            hipLaunchKernelGGL(pv_resample_kernel, dim3(rv_grid(channels * (m1 - m_next))), block, 0, ctx->stream, zseg[cur], L.lseg, z_base, g.Lz, g.r,
                               g.cut, g.half, g.scale, out, ld_out, m_next, m1, channels);
            ALSEP_LAUNCH_CHECK(ctx, "pv_resample_kernel");
            m_next = m1;
        }
    }
    return ALSEP_OK;
}
