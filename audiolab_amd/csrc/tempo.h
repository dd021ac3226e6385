// Tempo and beat tracking on the GPU: the arithmetic behind the reference's Export plugin (wrappers/export.py:18-40 hands the instrumental to
// librosa.load and librosa.beat.beat_track) restated from the published design -- a mel power spectrogram, spectral flux, an autocorrelation
// tempogram and Ellis' dynamic-programming beat tracker.  Parity unpinned: the specification is tests/tempo_oracle.py (numpy / scipy) and
// DESIGN section 4f.  Included at the end of reverb.hip: the transform is master.h's in-LDS Stockham, the reductions are compare.h's and
// master.h's fixed trees.  gfx950 only.
//
// Geometry, fixed: 22050 Hz, frames of 2048 samples every 512, centred (1024 zeros on both sides: F = 1 + n / 512 frames), 128 mel bands,
// tempogram window 344 frames.  Arithmetic: double precision throughout; no floating-point atomics, every reduction has an order that
// depends on the geometry alone.
//
// tp_mel_kernel, one workgroup of 256 threads per PAIR of frames: the two windowed frames are the real and the imaginary part of one
// 2048-point complex transform in LDS (32 KB, in place: five workgroups = ten frames per CU); the spectra come apart by conjugate
// symmetry, the 2 x 1025 powers go back into the same LDS, and thread t sums band t & 127 of frame t >> 7 over that band's bins: the
// 1025-bin spectrum never reaches memory.
// tp_flux_kernel: a wave per frame sorts the 128 rectified band differences in LDS (bitonic network) and takes the mean of the middle pair.
// tp_tempogram_kernel: a workgroup walks a fixed range of frames; thread t < 172 owns the lags t and 343 - t (345 products together) and
// keeps their running sums in registers; the ranges' sums are added in index order by tp_tempogram_final_kernel.
// tp_beat_dp_kernel: ONE wave, sequential in the frame index.  The reachable stretch of the cumulative score (at most 2 x 343 frames back)
// lives in an LDS ring of 1024; a step is up to 9 ring reads per lane, adds, a wave reduction (value, then the lowest index on ties)
// and one LDS store; the scores come in, and cum / back go out, 64 frames at a time.  The kernel only adds and compares.
namespace {

constexpr int kTpThreads = 256;
constexpr int kTpN = 2048, kTpLog2N = 11, kTpHop = 512, kTpBins = 1025, kTpMels = 128;
constexpr int kTpWin = 344, kTpHalf = kTpWin / 2;                            // int(8.0 * 22050 / 512) frames
constexpr int kTpGroups = 256;                                               // workgroups (frame ranges) of the averaged tempogram
constexpr int kTpMaxPeriod = kTpWin - 1;
constexpr int kTpRing = 1024;                                                // >= 2 * kTpMaxPeriod, a power of two
constexpr int kTpDpPer = 9;                                                  // window offsets per lane: 64 * 9 >= 2 * 343 - 172 + 1
constexpr int kTpFluxLead = 3;                                               // 1 + n_fft / (2 hop) leading zeros of the envelope
constexpr int64_t kTpMaxSamples = (int64_t)3600 * 22050;

int64_t tp_frames(int64_t n) { return 1 + n / kTpHop; }
bool tp_frames_ok(int64_t F) { return F >= 1 && F <= tp_frames(kTpMaxSamples); }

// frames fa = 2 blockIdx.x and fa + 1: samples [512 f - 1024, 512 f + 1024) of y, zero outside [0, n), times the window.
// bands: int32 [128][3] = first bin, bin count, offset of the band's weights in `weights`; a band that points outside is left at zero.
__global__ void __launch_bounds__(kTpThreads)
tp_mel_kernel(const double* __restrict__ y, int64_t n, const double* __restrict__ win, const cplx* __restrict__ tw,
              const int32_t* __restrict__ bands, const double* __restrict__ weights, int64_t n_weights, int64_t F, double* __restrict__ mel) {
    cplx* z = (cplx*)alsep_smem;
    const int t = threadIdx.x;
    const int64_t fa = 2 * (int64_t)blockIdx.x;
    const int64_t base = fa * kTpHop - kTpN / 2;
    for (int p = t; p < kTpN; p += kTpThreads) {
        const int64_t s0 = base + p, s1 = s0 + kTpHop;
        const double h = win[p];
        cplx c = {0.0, 0.0};
        if (s0 >= 0 && s0 < n) c.x = y[s0] * h;
        if (s1 >= 0 && s1 < n) c.y = y[s1] * h;
        z[p] = c;
    }
    __syncthreads();
    ms_fft_lds<kTpLog2N>(z, tw, t);
    constexpr int kPer = (kTpBins + kTpThreads - 1) / kTpThreads;            // 5
    double pa[kPer], pb[kPer];
#pragma unroll
    for (int c = 0; c < kPer; ++c) {
        const int k = t + c * kTpThreads;
        pa[c] = 0.0;
        pb[c] = 0.0;
        if (k < kTpBins) {
            cplx A, B;
            split_spectra(z[k], z[(kTpN - k) & (kTpN - 1)], &A, &B);
            pa[c] = A.x * A.x + A.y * A.y;
            pb[c] = B.x * B.x + B.y * B.y;
        }
    }
    __syncthreads();
    double* pw = (double*)alsep_smem;                                        // [2][1025] over the transform
#pragma unroll
    for (int c = 0; c < kPer; ++c) {
        const int k = t + c * kTpThreads;
        if (k < kTpBins) { pw[k] = pa[c]; pw[kTpBins + k] = pb[c]; }
    }
    __syncthreads();
    const int band = t & (kTpMels - 1), which = t >> 7;
    const int64_t f = fa + which;
    const int first = bands[3 * band], off = bands[3 * band + 2];
    int cnt = bands[3 * band + 1];
    if (first < 0 || cnt < 0 || first + cnt > kTpBins || off < 0 || (int64_t)off + cnt > n_weights) cnt = 0;
    const double* p = pw + which * kTpBins + first;
    const double* w = weights + off;
    double acc = 0.0;
    for (int j = 0; j < cnt; ++j) acc = acc + w[j] * p[j];
    if (f < F) mel[(int64_t)band * F + f] = acc;
}

// D = 10 log10(max(1e-10, M)), floored at max(D) - 80; peak[0] = max(M), so that max(D) is the same expression of it
__global__ void __launch_bounds__(kTpThreads)
tp_db_kernel(const double* __restrict__ mel, int64_t total, const double* __restrict__ peak, double* __restrict__ db) {
    const double pk = peak[0];
    const double floor_db = 10.0 * log10(pk > 1e-10 ? pk : 1e-10) - 80.0;
    for (int64_t i = (int64_t)blockIdx.x * kTpThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kTpThreads) {
        const double v = mel[i];
        const double d = 10.0 * log10(v > 1e-10 ? v : 1e-10);
        db[i] = d > floor_db ? d : floor_db;
    }
}

// env[i] = median over the bands of max(0, D[:, i - 2] - D[:, i - 3]) for 3 <= i < F, 0 before; wave w of a workgroup takes i = 4 blockIdx.x + w
__global__ void __launch_bounds__(kTpThreads)
tp_flux_kernel(const double* __restrict__ db, int64_t F, double* __restrict__ env) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* s = (double*)alsep_smem + wv * kTpMels;
    const int64_t i = (int64_t)blockIdx.x * (kTpThreads / 64) + wv;
    const bool live = i >= kTpFluxLead && i < F;
    for (int e = lane; e < kTpMels; e += 64) {
        double v = 0.0;
        if (live) {
            const double d = db[(int64_t)e * F + (i - 2)] - db[(int64_t)e * F + (i - 3)];
            v = d > 0.0 ? d : 0.0;
        }
        s[e] = v;
    }
    __syncthreads();
    // bitonic network over 128 values, 64 compare-exchanges per step: lane p takes the pair (lo, lo + j)
    for (int k = 2; k <= kTpMels; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int lo = (lane / j) * 2 * j + (lane % j), hi = lo + j;
            const bool up = (lo & k) == 0;
            const double a = s[lo], b = s[hi];
            if ((a > b) == up) { s[lo] = b; s[hi] = a; }
            __syncthreads();
        }
    }
    if (lane == 0 && i < F) env[i] = live ? 0.5 * (s[kTpMels / 2 - 1] + s[kTpMels / 2]) : 0.0;
}

// out[0] = max|env|, out[1] = mean, out[2] = the standard deviation with ddof = 1 (NaN for one frame, as numpy); one workgroup
__global__ void __launch_bounds__(kTpThreads)
tp_env_stats_kernel(const double* __restrict__ env, int64_t F, double* __restrict__ out) {
    double* sv = (double*)alsep_smem;
    const int t = threadIdx.x;
    double acc = 0.0, m = 0.0;
    for (int64_t j = t; j < F; j += kTpThreads) { acc = acc + env[j]; m = ms_max(m, fabs(env[j])); }
    cmp_tree_sum(sv, acc);
    const double mean = sv[0] / (double)F;
    __syncthreads();
    ms_tree_max(sv, m);
    const double peak = sv[0];
    __syncthreads();
    acc = 0.0;
    for (int64_t j = t; j < F; j += kTpThreads) { const double d = env[j] - mean; acc = acc + d * d; }
    cmp_tree_sum(sv, acc);
    if (t == 0) { out[0] = peak; out[1] = mean; out[2] = sqrt(sv[0] / (double)(F - 1)); }
}

// Frame f = entries [f, f + 344) of the envelope padded by 172 on both sides with a linear ramp to 0 (numpy.pad "linear_ramp": element i of
// the left ramp is (edge / 172) i, the right one mirrors it), times the window; its autocorrelation at the lags 0 .. 343, divided by the
// largest magnitude unless that is below the smallest normal double.  Workgroup g sums the frames [g F / G, (g + 1) F / G) in ascending
// order into partial[g][lag].
__global__ void __launch_bounds__(kTpThreads)
tp_tempogram_kernel(const double* __restrict__ env, int64_t F, const double* __restrict__ win, double* __restrict__ partial) {
    double* x = (double*)alsep_smem;                                         // [344]
    double* red = x + kTpWin;                                                // [256]
    const int t = threadIdx.x;
    const int64_t G = gridDim.x, g = blockIdx.x, f0 = g * F / G, f1 = (g + 1) * F / G;
    const double left = env[0] / (double)kTpHalf, right = env[F - 1] / (double)kTpHalf;
    const int la = t, lb = kTpWin - 1 - t;
    const bool owner = t < kTpHalf;
    double sa = 0.0, sb = 0.0;
    for (int64_t f = f0; f < f1; ++f) {
        for (int e = t; e < kTpWin; e += kTpThreads) {
            const int64_t p = f + e, src = p - kTpHalf;
            double v;
            if (src < 0) v = left * (double)p;
            else if (src >= F) v = right * (double)(F + 2 * kTpHalf - 1 - p);
            else v = env[src];
            x[e] = v * win[e];
        }
        __syncthreads();
        double a = 0.0, b = 0.0;
        if (owner) {
            for (int i = 0; i < kTpWin - la; ++i) a = a + x[i] * x[i + la];
            for (int i = 0; i < kTpWin - lb; ++i) b = b + x[i] * x[i + lb];
        }
        ms_tree_max(red, ms_max(fabs(a), fabs(b)));
        const double mx = red[0];
        if (mx >= 2.2250738585072014e-308) { a = a / mx; b = b / mx; }
        sa = sa + a;
        sb = sb + b;
        __syncthreads();
    }
    if (owner) {
        partial[g * kTpWin + la] = sa;
        partial[g * kTpWin + lb] = sb;
    }
}

__global__ void __launch_bounds__(kTpThreads)
tp_tempogram_final_kernel(const double* __restrict__ partial, int64_t G, int64_t F, double* __restrict__ tg) {
    for (int l = threadIdx.x; l < kTpWin; l += kTpThreads) {
        double acc = 0.0;
        for (int64_t g = 0; g < G; ++g) acc = acc + partial[g * kTpWin + l];
        tg[l] = acc / (double)F;
    }
}

// ls = scipy.signal.convolve(env / std, window, "same"), window of 2 period + 1 taps: ls[i] = sum_j window[j] env[i + period - j] / std
__global__ void __launch_bounds__(kTpThreads)
tp_local_score_kernel(const double* __restrict__ env, int64_t F, const double* __restrict__ stats, const double* __restrict__ win, int period,
                      double* __restrict__ ls) {
    const double sd = stats[2];
    for (int64_t i = (int64_t)blockIdx.x * kTpThreads + threadIdx.x; i < F; i += (int64_t)gridDim.x * kTpThreads) {
        double acc = 0.0;
        for (int j = 0; j <= 2 * period; ++j) {
            const int64_t s = i + period - j;
            if (s >= 0 && s < F) acc = acc + win[j] * (env[s] / sd);
        }
        ls[i] = acc;
    }
}

// the larger value, the lower index among equal ones; every lane ends with the wave's result
__device__ __forceinline__ void tp_wave_best(double* v, int* j) {
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(*v, o);
        const int oj = __shfl_xor(*j, o);
        if (ov > *v || (ov == *v && oj < *j)) { *v = ov; *j = oj; }
    }
}

// cand[j] = txwt[j] + (cum[i + w0 + j] or 0 before the start), j < W; b = the lowest index among the maxima; cum[i] = ls[i] + cand[b];
// back[i] = -1 until a frame reaches 0.01 max(ls), then i + w0 + b.  One wave.  w0 + W <= 0: a step reads earlier frames only.
__global__ void __launch_bounds__(64)
tp_beat_dp_kernel(const double* __restrict__ ls, int64_t F, const double* __restrict__ txwt, int w0, int W, double* __restrict__ cum,
                  int32_t* __restrict__ back) {
    double* ring = (double*)alsep_smem;                                      // [1024]: cum[i] at i & 1023
    const int lane = threadIdx.x;
    double top = -INFINITY;
    for (int64_t i = lane; i < F; i += 64) top = ms_max(top, ls[i]);
    for (int o = 32; o > 0; o >>= 1) top = ms_max(top, __shfl_xor(top, o));
    const double thresh = 0.01 * top;
    double tx[kTpDpPer];
#pragma unroll
    for (int c = 0; c < kTpDpPer; ++c) {
        const int j = lane + 64 * c;
        tx[c] = j < W ? txwt[j] : 0.0;
    }
    for (int e = lane; e < kTpRing; e += 64) ring[e] = 0.0;
    __syncthreads();
    bool first = true;
    for (int64_t i0 = 0; i0 < F; i0 += 64) {
        const int cnt = (int)(F - i0 < 64 ? F - i0 : 64);
        const double mine = lane < cnt ? ls[i0 + lane] : 0.0;
        double my_cum = 0.0;
        int32_t my_back = -1;
        for (int s = 0; s < cnt; ++s) {
            const int64_t i = i0 + s;
            const double score = __shfl(mine, s);
            double best = -INFINITY;
            int bj = 0x7fffffff;
#pragma unroll
            for (int c = 0; c < kTpDpPer; ++c) {                             // ascending j: a strict comparison keeps the lowest index
                const int j = lane + 64 * c;
                if (j < W) {
                    const int64_t src = i + w0 + j;
                    const double v = tx[c] + (src >= 0 ? ring[src & (kTpRing - 1)] : 0.0);
                    if (v > best) { best = v; bj = j; }
                }
            }
            tp_wave_best(&best, &bj);
            const double ci = score + best;
            int32_t bk = -1;
            if (!(first && score < thresh)) { bk = (int32_t)(i + w0 + bj); first = false; }
            if (lane == 0) ring[i & (kTpRing - 1)] = ci;
            if (lane == s) { my_cum = ci; my_back = bk; }
            __syncthreads();
        }
        if (lane < cnt) { cum[i0 + lane] = my_cum; back[i0 + lane] = my_back; }
    }
}

}  // namespace

// frames of a track of n samples at 22050 Hz, -1 when n < 1 or the track is longer than 60 minutes
extern "C" int64_t alsep_tempo_frames(int64_t n) { return n < 1 || n > kTpMaxSamples ? -1 : tp_frames(n); }

extern "C" int alsep_tempo_mel(alsep_ctx* ctx, const double* y, int64_t n, const double* window, const double* twiddle, const int32_t* bands,
                               const double* weights, int64_t n_weights, double* mel) {
    ALSEP_ENTER(ctx);
    if (!ctx || !y || !window || !twiddle || !bands || !weights || !mel || n_weights < 1)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_tempo_mel: bad argument");
    if (n < 1 || n > kTpMaxSamples) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_tempo_mel: %lld samples (1 .. %lld)", (long long)n, (long long)kTpMaxSamples);
    const int64_t F = tp_frames(n);
    hipLaunchKernelGGL(tp_mel_kernel, dim3((unsigned)((F + 1) / 2)), dim3(kTpThreads), (size_t)kTpN * sizeof(cplx), ctx->stream, y, n, window,
                       (const cplx*)twiddle, bands, weights, n_weights, F, mel);
    ALSEP_LAUNCH_CHECK(ctx, "tp_mel_kernel");
    return ALSEP_OK;
}

extern "C" int64_t alsep_tempo_flux_workspace_bytes(void) { return (kMsPeakBlocks + 1) * (int64_t)sizeof(double); }

// mel: float64 [128][frames]; db (the same shape): the decibel array the flux is taken from; env: float64 [frames]
extern "C" int alsep_tempo_flux(alsep_ctx* ctx, const double* mel, int64_t frames, double* db, double* env, void* ws, int64_t ws_bytes) {
    ALSEP_ENTER(ctx);
    if (!ctx || !mel || !db || !env || !ws || mel == db || !tp_frames_ok(frames)) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_tempo_flux: bad argument");
    if (ws_bytes < alsep_tempo_flux_workspace_bytes()) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_tempo_flux: workspace too small");
    const int64_t total = (int64_t)kTpMels * frames;
    double* partial = (double*)ws;
    double* peak = partial + kMsPeakBlocks;
    const unsigned blocks = ms_peak_blocks(total);
    const size_t lds = kMsThreads * sizeof(double);
    hipLaunchKernelGGL(ms_peak_partial_kernel, dim3(blocks), dim3(kMsThreads), lds, ctx->stream, mel, 1, total, total, partial);
    ALSEP_LAUNCH_CHECK(ctx, "ms_peak_partial_kernel");
    hipLaunchKernelGGL(ms_peak_final_kernel, dim3(1), dim3(kMsThreads), lds, ctx->stream, (const double*)partial, (int)blocks, peak);
    ALSEP_LAUNCH_CHECK(ctx, "ms_peak_final_kernel");
    hipLaunchKernelGGL(tp_db_kernel, dim3(rv_grid(total)), dim3(kTpThreads), 0, ctx->stream, mel, total, (const double*)peak, db);
    ALSEP_LAUNCH_CHECK(ctx, "tp_db_kernel");
    const int per = kTpThreads / 64;
    hipLaunchKernelGGL(tp_flux_kernel, dim3((unsigned)((frames + per - 1) / per)), dim3(kTpThreads), (size_t)per * kTpMels * sizeof(double), ctx->stream,
                       (const double*)db, frames, env);
    ALSEP_LAUNCH_CHECK(ctx, "tp_flux_kernel");
    return ALSEP_OK;
}

// stats (device) [3] = max|env|, mean(env), std(env, ddof = 1)
extern "C" int alsep_tempo_env_stats(alsep_ctx* ctx, const double* env, int64_t frames, double* stats) {
    ALSEP_ENTER(ctx);
    if (!ctx || !env || !stats || !tp_frames_ok(frames)) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_tempo_env_stats: bad argument");
    hipLaunchKernelGGL(tp_env_stats_kernel, dim3(1), dim3(kTpThreads), kTpThreads * sizeof(double), ctx->stream, env, frames, stats);
    ALSEP_LAUNCH_CHECK(ctx, "tp_env_stats_kernel");
    return ALSEP_OK;
}

extern "C" int64_t alsep_tempo_tempogram_workspace_bytes(void) { return (int64_t)kTpGroups * kTpWin * (int64_t)sizeof(double); }

// tg[344] = the mean over the frames of the normalised autocorrelation of the windowed envelope; window: float64 [344]
extern "C" int alsep_tempo_tempogram(alsep_ctx* ctx, const double* env, int64_t frames, const double* window, double* tg, void* ws, int64_t ws_bytes) {
    ALSEP_ENTER(ctx);
    if (!ctx || !env || !window || !tg || !ws || !tp_frames_ok(frames)) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_tempo_tempogram: bad argument");
    if (ws_bytes < alsep_tempo_tempogram_workspace_bytes()) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_tempo_tempogram: workspace too small");
    const int64_t G = frames < kTpGroups ? frames : kTpGroups;
    hipLaunchKernelGGL(tp_tempogram_kernel, dim3((unsigned)G), dim3(kTpThreads), (size_t)(kTpWin + kTpThreads) * sizeof(double), ctx->stream, env, frames,
                       window, (double*)ws);
    ALSEP_LAUNCH_CHECK(ctx, "tp_tempogram_kernel");
    hipLaunchKernelGGL(tp_tempogram_final_kernel, dim3(1), dim3(kTpThreads), 0, ctx->stream, (const double*)ws, G, frames, tg);
    ALSEP_LAUNCH_CHECK(ctx, "tp_tempogram_final_kernel");
    return ALSEP_OK;
}

// window: float64 [2 period + 1]; stats: what alsep_tempo_env_stats wrote
extern "C" int alsep_tempo_local_score(alsep_ctx* ctx, const double* env, int64_t frames, const double* stats, const double* window, int period,
                                       double* ls) {
    ALSEP_ENTER(ctx);
    if (!ctx || !env || !stats || !window || !ls || env == ls || !tp_frames_ok(frames))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_tempo_local_score: bad argument");
    if (period < 1 || period > kTpMaxPeriod) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_tempo_local_score: period %d (1 .. %d)", period, kTpMaxPeriod);
    hipLaunchKernelGGL(tp_local_score_kernel, dim3(rv_grid(frames)), dim3(kTpThreads), 0, ctx->stream, env, frames, stats, window, period, ls);
    ALSEP_LAUNCH_CHECK(ctx, "tp_local_score_kernel");
    return ALSEP_OK;
}

// txwt: float64 [count], the transition costs of the offsets first_offset .. first_offset + count - 1, all negative; cum: float64 [frames];
// back: int32 [frames]
extern "C" int alsep_tempo_beat_dp(alsep_ctx* ctx, const double* ls, int64_t frames, const double* txwt, int first_offset, int count, double* cum,
                                   int32_t* back) {
    ALSEP_ENTER(ctx);
    if (!ctx || !ls || !txwt || !cum || !back || ls == cum || !tp_frames_ok(frames)) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_tempo_beat_dp: bad argument");
    if (count < 1 || count > 64 * kTpDpPer || first_offset < -2 * kTpMaxPeriod || (int64_t)first_offset + count > 0)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_tempo_beat_dp: offsets %d .. %d (1 .. %d of them, within -%d .. -1)", first_offset,
                          first_offset + count - 1, 64 * kTpDpPer, 2 * kTpMaxPeriod);
    hipLaunchKernelGGL(tp_beat_dp_kernel, dim3(1), dim3(64), (size_t)kTpRing * sizeof(double), ctx->stream, ls, frames, txwt, first_offset, count, cum, back);
    ALSEP_LAUNCH_CHECK(ctx, "tp_beat_dp_kernel");
    return ALSEP_OK;
}
