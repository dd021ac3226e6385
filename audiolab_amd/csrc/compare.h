// The arithmetic of the reference's Compare plugin (wrappers/compare.py:73-124) on the GPU: two tracks, RMS-normalised (:96-99), their
// absolute difference (:102), the magnitude spectrogram of track 1 and the spectrogram difference in decibels (:110-124, :145, :152) --
// scipy.signal.stft(x, nperseg=2048, noverlap=1024) with its defaults: periodic Hann, zero boundary, padded tail, scaled by
// 1 / sum(window) = 1 / 1024 -- plus the two reductions that bring the arrays to figure resolution.  Included at the end of reverb.hip:
// the float64 resampler in front of all this is that file's.  gfx950 only.
//
// Arithmetic: double precision throughout; the two decibel arrays are rounded once to float32.  The fourth panel is
// 20 log10(|S1 - S2| + 1e-9): single-precision noise (1e-7 of the peak) would stand 40 dB above that floor wherever the tracks agree.
//
// cmp_spectra_kernel, one workgroup of 256 threads per frame: the two real frames, windowed, are the real and the imaginary part of ONE
// 2048-point complex transform; the spectra come apart by conjugate symmetry (split_spectra).  The transform is the Stockham
// decomposition of fft_pass_kernel -- radix 8, 8, 8, 4, one butterfly per thread and pass (two in the last) -- with the array in LDS and
// the butterflies in registers; the first pass reads global memory directly.  Twiddles are exp(-2 pi i m / 2048) from a float64 table the
// caller computes on the host, like the window.
// LDS: a frame is 2048 complex doubles = 32 KB.  The passes run IN PLACE: every thread reads its butterfly, a barrier, every thread
// writes, a barrier -- 7 barriers per frame instead of the 4 of a ping-pong.  Ping-pong needs 64 KB, two workgroups per CU out of the
// 160 KB; in place the LDS admits five (exactly 5 x 32 KB, nothing else is kept there), 20 waves per CU, and the kernel's 60 VGPRs
// without scratch do not limit it further.  The output is bin-major [1025, F], so a workgroup writes one column in strided 4-byte
// stores; neighbouring frames run side by side and fill the same lines.  Measured, 5 minutes of stereo (25 841 frames): 0.88 ms
// (profiles/compare_bench.txt), beside 24.6 ms for a resample in front of it -- gathering frames per workgroup to widen the stores
// was not pursued.
namespace {

constexpr int kCmpThreads = 256;
constexpr int kCmpN = 2048, kCmpHop = 1024, kCmpBins = 1025;
constexpr int kCmpPartials = 1024;                                           // block partials of the sum of squares (8 KB of workspace)
constexpr int kCmpDefaultFrames = 65536;                                     // frames per launch when the caller passes 0

int64_t cmp_frames(int64_t n) { return 1 + (n + kCmpHop - 1) / kCmpHop; }

unsigned cmp_rms_blocks(int64_t n) {                                         // a function of n alone: the reduction order is fixed
    const int64_t g = (n + kCmpThreads - 1) / kCmpThreads;
    return (unsigned)(g < kCmpPartials ? g : kCmpPartials);
}

// sums of `count` values spread over the threads of a block, in a fixed tree; the result is in sv[0] after the call
__device__ __forceinline__ void cmp_tree_sum(double* sv, double v) {
    sv[threadIdx.x] = v;
    __syncthreads();
    for (int s = kCmpThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sv[threadIdx.x] = sv[threadIdx.x] + sv[threadIdx.x + s];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kCmpThreads)
cmp_sumsq_partial_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ partial) {
    double acc = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * kCmpThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kCmpThreads) acc = acc + x[j] * x[j];
    cmp_tree_sum((double*)alsep_smem, acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = ((double*)alsep_smem)[0];
}

__global__ void __launch_bounds__(kCmpThreads)
cmp_sumsq_final_kernel(const double* __restrict__ partial, int count, double* __restrict__ out) {
    double acc = 0.0;
    for (int j = threadIdx.x; j < count; j += kCmpThreads) acc = acc + partial[j];
    cmp_tree_sum((double*)alsep_smem, acc);
    if (threadIdx.x == 0) out[0] = ((double*)alsep_smem)[0];
}

// :96-99 and :102.  rms = sqrt(mean(x^2)) from the sums of squares; a track at or below 1e-9 stays as it is
__global__ void __launch_bounds__(kCmpThreads)
cmp_wave_kernel(const double* __restrict__ x0, const double* __restrict__ x1, int64_t n, const double* __restrict__ sumsq,
                double* __restrict__ w0, double* __restrict__ w1, double* __restrict__ diff) {
    const double r0 = sqrt(sumsq[0] / (double)n), r1 = sqrt(sumsq[1] / (double)n);
    const bool s0 = r0 > 1e-9, s1 = r1 > 1e-9;
    for (int64_t j = (int64_t)blockIdx.x * kCmpThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kCmpThreads) {
        double a = x0[j], b = x1[j];
        if (s0) a = a / r0;
        if (s1) b = b / r1;
        w0[j] = a;
        w1[j] = b;
        diff[j] = fabs(a - b);
    }
}

// One in-place radix-8 Stockham pass over the 2048 points in LDS; ns = the length of the sub-transforms done so far (8 or 64).
// tw[m] = exp(-2 pi i m / 2048): w^(q k) with w = exp(-2 pi i / (8 ns)) is entry q k (256 / ns), q k <= 7 (ns - 1).
__device__ __forceinline__ void cmp_pass8(cplx* z, const cplx* __restrict__ tw, int j, int ns) {
    const int k = j & (ns - 1), step = (kCmpN / 8) / ns;
    cplx v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = z[j + q * (kCmpN / 8)];
    __syncthreads();
#pragma unroll
    for (int q = 1; q < 8; ++q) v[q] = cmul(v[q], tw[q * k * step]);
    dft_small<8>(v, -1.0);
    const int j0 = (j - k) * 8 + k;
#pragma unroll
    for (int q = 0; q < 8; ++q) z[j0 + q * ns] = v[q];
    __syncthreads();
}

// Frame f = f0 + blockIdx.x: samples [1024 f - 1024, 1024 f + 1024) of both tracks, zero outside [0, n), times the window.
// spec1_db / diff_db: float32 [1025][F]; s1_lin / sd_lin: the same shape in float64, optional.
__global__ void __launch_bounds__(kCmpThreads)
cmp_spectra_kernel(const double* __restrict__ w0, const double* __restrict__ w1, int64_t n, const double* __restrict__ win,
                   const cplx* __restrict__ tw, int64_t f0, int64_t F, float* __restrict__ spec1_db, float* __restrict__ diff_db,
                   double* __restrict__ s1_lin, double* __restrict__ sd_lin) {
    cplx* z = (cplx*)alsep_smem;
    const int t = threadIdx.x;
    const int64_t f = f0 + blockIdx.x;
    const int64_t base = f * kCmpHop - kCmpHop;
    {   // pass 1, radix 8, ns = 1: no twiddles, inputs straight from global memory
        cplx v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int p = t + q * (kCmpN / 8);
            const int64_t s = base + p;
            cplx c = {0.0, 0.0};
            if (s >= 0 && s < n) { const double h = win[p]; c = {w0[s] * h, w1[s] * h}; }
            v[q] = c;
        }
        dft_small<8>(v, -1.0);
#pragma unroll
        for (int q = 0; q < 8; ++q) z[t * 8 + q] = v[q];
        __syncthreads();
    }
    cmp_pass8(z, tw, t, 8);
    cmp_pass8(z, tw, t, 64);
    {   // pass 4, radix 4, ns = 512: butterflies j = t and t + 256 (k = j), inputs j + q 512, outputs k + q 512
        cplx a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[q] = z[t + q * 512]; b[q] = z[t + 256 + q * 512]; }
        __syncthreads();
#pragma unroll
        for (int q = 1; q < 4; ++q) { a[q] = cmul(a[q], tw[q * t]); b[q] = cmul(b[q], tw[q * (t + 256)]); }
        dft_small<4>(a, -1.0);
        dft_small<4>(b, -1.0);
#pragma unroll
        for (int q = 0; q < 4; ++q) { z[t + q * 512] = a[q]; z[t + 256 + q * 512] = b[q]; }
        __syncthreads();
    }
    const double scale = 1.0 / (double)kCmpHop;                              // 1 / sum(window), a power of two
    for (int k = t; k < kCmpBins; k += kCmpThreads) {
        cplx A, B;
        split_spectra(z[k], z[(kCmpN - k) & (kCmpN - 1)], &A, &B);
        const double s1 = hypot(A.x, A.y) * scale, s2 = hypot(B.x, B.y) * scale, d = fabs(s1 - s2);
        const int64_t o = (int64_t)k * F + f;
        spec1_db[o] = (float)(20.0 * log10(s1 + 1e-9));
        diff_db[o] = (float)(20.0 * log10(d + 1e-9));
        if (s1_lin) s1_lin[o] = s1;
        if (sd_lin) sd_lin[o] = d;
    }
}

// bucket b of K over [0, n): samples [floor(b n / K), floor((b + 1) n / K)), K <= n so that none is empty.  One workgroup per bucket;
// the smallest and the largest value with the first index of each.
__global__ void __launch_bounds__(kCmpThreads)
cmp_minmax_kernel(const double* __restrict__ x, int64_t n, int64_t K, double* __restrict__ mn, int64_t* __restrict__ imn,
                  double* __restrict__ mx, int64_t* __restrict__ imx) {
    double* lo_v = (double*)alsep_smem;
    double* hi_v = lo_v + kCmpThreads;
    int64_t* lo_i = (int64_t*)(hi_v + kCmpThreads);
    int64_t* hi_i = lo_i + kCmpThreads;
    const int t = threadIdx.x;
    for (int64_t b = blockIdx.x; b < K; b += gridDim.x) {
        const int64_t j0 = b * n / K, j1 = (b + 1) * n / K;
        double lv = INFINITY, hv = -INFINITY;
        int64_t li = INT64_MAX, hi = INT64_MAX;
        for (int64_t j = j0 + t; j < j1; j += kCmpThreads) {                 // ascending j: a strict comparison keeps the first index
            const double v = x[j];
            if (v < lv || li == INT64_MAX) { lv = v; li = j; }
            if (v > hv || hi == INT64_MAX) { hv = v; hi = j; }
        }
        lo_v[t] = lv; lo_i[t] = li; hi_v[t] = hv; hi_i[t] = hi;
        __syncthreads();
        for (int s = kCmpThreads / 2; s > 0; s >>= 1) {
            if (t < s) {
                const double ov = lo_v[t + s];
                const int64_t oi = lo_i[t + s];
                if (oi != INT64_MAX && (lo_i[t] == INT64_MAX || ov < lo_v[t] || (ov == lo_v[t] && oi < lo_i[t]))) { lo_v[t] = ov; lo_i[t] = oi; }
                const double pv = hi_v[t + s];
                const int64_t pi = hi_i[t + s];
                if (pi != INT64_MAX && (hi_i[t] == INT64_MAX || pv > hi_v[t] || (pv == hi_v[t] && pi < hi_i[t]))) { hi_v[t] = pv; hi_i[t] = pi; }
            }
            __syncthreads();
        }
        if (t == 0) { mn[b] = lo_v[0]; imn[b] = lo_i[0]; mx[b] = hi_v[0]; imx[b] = hi_i[0]; }
        __syncthreads();
    }
}

// out[k][j] = max of in[k][floor(j F / Kt) .. floor((j + 1) F / Kt)), Kt <= F; one thread per output, its frames are contiguous
__global__ void __launch_bounds__(kCmpThreads)
cmp_colmax_kernel(const float* __restrict__ in, int64_t F, int64_t Kt, float* __restrict__ out) {
    const int64_t total = (int64_t)kCmpBins * Kt;
    for (int64_t i = (int64_t)blockIdx.x * kCmpThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kCmpThreads) {
        const int64_t k = i / Kt, j = i - k * Kt, c0 = j * F / Kt, c1 = (j + 1) * F / Kt;
        const float* row = in + k * F;
        float m = row[c0];
        for (int64_t c = c0 + 1; c < c1; ++c) { const float v = row[c]; if (v > m) m = v; }
        out[i] = m;
    }
}

constexpr int64_t kCmpMaxSamples = (int64_t)1 << 31;                         // b n / K stays below 2^62

}  // namespace

extern "C" int64_t alsep_compare_frames(int64_t n) { return n < kCmpN || n > kCmpMaxSamples ? -1 : cmp_frames(n); }

extern "C" int64_t alsep_compare_rms_workspace_bytes(void) { return kCmpPartials * (int64_t)sizeof(double); }

extern "C" int alsep_compare_rms(alsep_ctx* ctx, const double* x, int64_t n, double* sumsq_out, void* ws, int64_t ws_bytes) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !sumsq_out || !ws || n < 1 || n > kCmpMaxSamples) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_compare_rms: bad argument");
    if (ws_bytes < kCmpPartials * (int64_t)sizeof(double)) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_compare_rms: workspace too small");
    ProfScope prof(ctx, ALSEP_PROF_COMPARE_RMS);
    const unsigned blocks = cmp_rms_blocks(n);
    const size_t lds = kCmpThreads * sizeof(double);
    hipLaunchKernelGGL(cmp_sumsq_partial_kernel, dim3(blocks), dim3(kCmpThreads), lds, ctx->stream, x, n, (double*)ws);
    ALSEP_LAUNCH_CHECK(ctx, "cmp_sumsq_partial_kernel");
    hipLaunchKernelGGL(cmp_sumsq_final_kernel, dim3(1), dim3(kCmpThreads), lds, ctx->stream, (const double*)ws, (int)blocks, sumsq_out);
    ALSEP_LAUNCH_CHECK(ctx, "cmp_sumsq_final_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_compare_wave(alsep_ctx* ctx, const double* x0, const double* x1, int64_t n, const double* sumsq, double* w0, double* w1,
                                  double* diff) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x0 || !x1 || !sumsq || !w0 || !w1 || !diff || n < 1 || n > kCmpMaxSamples)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_compare_wave: bad argument");
    ProfScope prof(ctx, ALSEP_PROF_COMPARE_WAVE);
    hipLaunchKernelGGL(cmp_wave_kernel, dim3(rv_grid(n)), dim3(kCmpThreads), 0, ctx->stream, x0, x1, n, sumsq, w0, w1, diff);
    ALSEP_LAUNCH_CHECK(ctx, "cmp_wave_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_compare_spectra(alsep_ctx* ctx, const double* w0, const double* w1, int64_t n, const double* window, const double* twiddle,
                                     int frames_per_batch, float* spec1_db, float* diff_db, double* s1_lin, double* sd_lin) {
    ALSEP_ENTER(ctx);
    if (!ctx || !w0 || !w1 || !window || !twiddle || !spec1_db || !diff_db || frames_per_batch < 0)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_compare_spectra: bad argument");
    if (n < kCmpN || n > kCmpMaxSamples)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_compare_spectra: %lld samples (%d .. 2^31)", (long long)n, kCmpN);
    ProfScope prof(ctx, ALSEP_PROF_COMPARE_SPECTRA);
    const int64_t F = cmp_frames(n), per = frames_per_batch > 0 ? frames_per_batch : kCmpDefaultFrames;
    const size_t lds = (size_t)kCmpN * sizeof(cplx);
    for (int64_t f0 = 0; f0 < F; f0 += per) {
        const int64_t nb = F - f0 < per ? F - f0 : per;
        hipLaunchKernelGGL(cmp_spectra_kernel, dim3((unsigned)nb), dim3(kCmpThreads), lds, ctx->stream, w0, w1, n, window, (const cplx*)twiddle, f0, F,
                           spec1_db, diff_db, s1_lin, sd_lin);
        ALSEP_LAUNCH_CHECK(ctx, "cmp_spectra_kernel");
    }
    return ALSEP_OK;
}

extern "C" int alsep_compare_minmax(alsep_ctx* ctx, const double* x, int64_t n, int64_t buckets, double* mn, int64_t* imn, double* mx,
                                    int64_t* imx) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !mn || !imn || !mx || !imx || n < 1 || n > kCmpMaxSamples || buckets < 1 || buckets > n)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_compare_minmax: bad argument (1 <= buckets <= n <= 2^31)");
    ProfScope prof(ctx, ALSEP_PROF_COMPARE_REDUCE);
    const unsigned grid = (unsigned)(buckets < 65536 ? buckets : 65536);
    hipLaunchKernelGGL(cmp_minmax_kernel, dim3(grid), dim3(kCmpThreads), kCmpThreads * 32, ctx->stream, x, n, buckets, mn, imn, mx, imx);
    ALSEP_LAUNCH_CHECK(ctx, "cmp_minmax_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_compare_colmax(alsep_ctx* ctx, const float* in, int64_t frames, int64_t buckets, float* out) {
    ALSEP_ENTER(ctx);
    if (!ctx || !in || !out || frames < 1 || frames > kCmpMaxSamples || buckets < 1 || buckets > frames)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_compare_colmax: bad argument (1 <= buckets <= frames)");
    ProfScope prof(ctx, ALSEP_PROF_COMPARE_REDUCE);
    hipLaunchKernelGGL(cmp_colmax_kernel, dim3(rv_grid(kCmpBins * buckets)), dim3(kCmpThreads), 0, ctx->stream, in, frames, buckets, out);
    ALSEP_LAUNCH_CHECK(ctx, "cmp_colmax_kernel");
    return ALSEP_OK;
}
