// Reference-track mastering on the GPU: the arithmetic behind the reference's Remaster plugin (wrappers/remaster.py:67-76 hands the two files
// to the Matchering library) restated from the published design -- levels of the loudest pieces, an averaged magnitude spectrum per mid /
// side channel, a matching FIR applied by FFT convolution, a look-ahead brickwall limiter, 24-bit quantisation.  Parity unpinned: the
// specification is tests/remaster_oracle.py (scipy itself) and DESIGN section 4e.  Included at the end of reverb.hip: the convolution is
// that file's overlap-save core, the transforms use its butterflies.  gfx950 only.
//
// Arithmetic: double precision throughout.  Every reduction has an order that depends on the geometry alone (block partials in a
// workspace, one finishing block): no floating-point atomics, the same bits on every run.
//
// ms_spectrum_kernel<LOG2N>: mid and side of one n_fft-point frame are the real and the imaginary part of ONE complex transform, done in
// place in LDS (n_fft complex doubles: 64 KB of the 160 KB at 4096) by Stockham passes of radix 8, 8, .., then 4 or 2; a thread keeps all
// its butterflies of a pass in registers between the barrier after the reads and the writes (n_fft / 256 complex values: 32 at 8192).
// A workgroup walks a fixed range of frames and keeps |spectrum| sums per bin in registers; the ranges' sums are added in index order by
// ms_spectrum_final_kernel.
//
// First-order IIR y[i] = b0 x[i] + b1 x[i-1] - a1 y[i-1] as a scan, three launches, no workgroup waits for another:
//   1. ms_iir_local_kernel   one workgroup per chunk of C samples: the tile goes to LDS, every thread runs the recurrence over its E =
//                            ceil(C / 256) consecutive samples from a zero state, the threads' end values are scanned in LDS
//                            (v[t] += q^(E h) v[t - h], h = 1, 2, .. 128; q = -a1), every sample gets q^(i - i0 + 1) times the value at the
//                            end of the thread before; chunk 0 starts from the caller's state and is final
//   2. the carry pass        end[c] += q^C end[c - 1] over the chunk ends (3230 for 5 minutes at the default C) is the same recurrence with
//                            the pole q^C: ms_iir_local_kernel again, on the ends (one workgroup; a walk by one thread took 0.42 ms)
//   3. ms_iir_fix_kernel     y[i] += q^(i - i0 + 1) end[c - 1], the power by repeated squaring
//
// Sliding maxima (windows of up to 8191 samples): a tile of the signal with its halo in LDS (16384 doubles; 4096 for short windows), doubled in place --
// m[i] = max(m[i], m[i + h]), h = 1, 2, 4, .. -- until m holds the maxima over P = 2^floor(log2 W) samples; a window of W is the maximum
// of two of those.  Selections only: the result is exact.
namespace {

constexpr int kMsThreads = 256;
constexpr int kMsPieces = 64;                                                // pieces per track: d <= 61 for 900 s in pieces of 15 s
constexpr int kMsPieceBlocks = 128;                                          // block partials per piece
constexpr int kMsSpecGroups = 256;                                           // workgroups (frame ranges) of the averaged spectrum
constexpr int kMsMaxBins = 4097;
constexpr int kMsBinsPer = (kMsMaxBins + kMsThreads - 1) / kMsThreads;      // 17
constexpr int kMsSlideElems = 16384;                                         // LDS tile of the sliding maximum, 128 KB
constexpr int kMsSlidePer = kMsSlideElems / kMsThreads;                      // 64
constexpr int kMsSlideElemsShort = 4096, kMsSlideShort = 1024;               // windows of up to 1024 samples: a tile of 4096, 32 KB
constexpr int kMsMaxWindow = 8191;
constexpr int kMsIirDefaultChunk = 4096, kMsIirMaxChunk = 8192;              // two LDS rows of C + 256 doubles
constexpr int kMsPeakBlocks = 1024;
constexpr int kMsPad = 6;                                                    // filtfilt: 3 * max(len(a), len(b))
constexpr int64_t kMsMaxSamples = (int64_t)1 << 30;

struct MsPieces {
    int32_t idx[kMsPieces];
};

__device__ __forceinline__ double ms_clip1(double v) { return v < -1.0 ? -1.0 : v > 1.0 ? 1.0 : v; }
__device__ __forceinline__ double ms_max(double a, double b) { return a > b ? a : b; }

// max over the threads of a block, result in sv[0]
__device__ __forceinline__ void ms_tree_max(double* sv, double v) {
    sv[threadIdx.x] = v;
    __syncthreads();
    for (int s = kMsThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sv[threadIdx.x] = ms_max(sv[threadIdx.x], sv[threadIdx.x + s]);
        __syncthreads();
    }
}

// q^m, m >= 0, by repeated squaring: the same value wherever it is computed
__device__ __forceinline__ double ms_powi(double q, int64_t m) {
    double r = 1.0, b = q;
    while (m > 0) {
        if (m & 1) r = r * b;
        b = b * b;
        m >>= 1;
    }
    return r;
}

// ---- levels -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kMsThreads)
ms_midside_kernel(const double* __restrict__ l, const double* __restrict__ r, int64_t n, double divisor, double* __restrict__ mid,
                  double* __restrict__ side) {
    for (int64_t j = (int64_t)blockIdx.x * kMsThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kMsThreads) {
        const double a = l[j] / divisor, b = r[j] / divisor;
        mid[j] = (a + b) * 0.5;
        side[j] = (a - b) * 0.5;
    }
}

__global__ void __launch_bounds__(kMsThreads)
ms_leftright_kernel(const double* __restrict__ mid, const double* __restrict__ side, int64_t n, double scale, double* __restrict__ l,
                    double* __restrict__ r) {
    for (int64_t j = (int64_t)blockIdx.x * kMsThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kMsThreads) {
        const double m = mid[j] * scale, s = side[j] * scale;
        l[j] = m + s;
        r[j] = m - s;
    }
}

// piece blockIdx.y = samples [piece p, piece p + p); its block blockIdx.x of G sums a strided share in a fixed tree
__global__ void __launch_bounds__(kMsThreads)
ms_piece_partial_kernel(const double* __restrict__ x, int64_t p, double scale, int clip, double* __restrict__ partial) {
    const double* px = x + (int64_t)blockIdx.y * p;
    double acc = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * kMsThreads + threadIdx.x; j < p; j += (int64_t)gridDim.x * kMsThreads) {
        double v = px[j];
        if (clip) v = ms_clip1(v * scale);
        acc = acc + v * v;
    }
    cmp_tree_sum((double*)alsep_smem, acc);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((double*)alsep_smem)[0];
}

// out[row] = the sum of partial[row][0 .. count) in a fixed tree; one block per row
__global__ void __launch_bounds__(kMsThreads)
ms_rows_sum_kernel(const double* __restrict__ partial, int count, double* __restrict__ out) {
    double acc = 0.0;
    for (int j = threadIdx.x; j < count; j += kMsThreads) acc = acc + partial[(int64_t)blockIdx.x * count + j];
    cmp_tree_sum((double*)alsep_smem, acc);
    if (threadIdx.x == 0) out[blockIdx.x] = ((double*)alsep_smem)[0];
}

unsigned ms_piece_blocks(int64_t p) {
    const int64_t g = (p + 4 * kMsThreads - 1) / (4 * kMsThreads);
    return (unsigned)(g < 1 ? 1 : g > kMsPieceBlocks ? kMsPieceBlocks : g);
}

// ---- peak -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kMsThreads)
ms_peak_partial_kernel(const double* __restrict__ x, int rows, int64_t n, int64_t ld, double* __restrict__ partial) {
    const int64_t total = (int64_t)rows * n;
    double m = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kMsThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kMsThreads) {
        const int64_t r = i / n, j = i - r * n;
        m = ms_max(m, fabs(x[r * ld + j]));
    }
    ms_tree_max((double*)alsep_smem, m);
    if (threadIdx.x == 0) partial[blockIdx.x] = ((double*)alsep_smem)[0];
}

__global__ void __launch_bounds__(kMsThreads)
ms_peak_final_kernel(const double* __restrict__ partial, int count, double* __restrict__ out) {
    double m = 0.0;
    for (int j = threadIdx.x; j < count; j += kMsThreads) m = ms_max(m, partial[j]);
    ms_tree_max((double*)alsep_smem, m);
    if (threadIdx.x == 0) out[0] = ((double*)alsep_smem)[0];
}

unsigned ms_peak_blocks(int64_t work) {
    const int64_t g = (work + kMsThreads - 1) / kMsThreads;
    return (unsigned)(g < 1 ? 1 : g > kMsPeakBlocks ? kMsPeakBlocks : g);
}

// ---- the averaged magnitude spectrum ------------------------------------------------------------------------------------------------
// One in-place Stockham pass of radix R over N = 2^LOG2N points in LDS; ns = the length of the sub-transforms done so far.
// tw[m] = exp(-2 pi i m / N): w^(q k) with w = exp(-2 pi i / (R ns)) is entry q k (N / (R ns)).
template <int LOG2N, int R>
__device__ __forceinline__ void ms_fft_pass(cplx* z, const cplx* __restrict__ tw, int t, int ns) {
    constexpr int N = 1 << LOG2N, M = N / R, BPT = (M + kMsThreads - 1) / kMsThreads;
    cplx v[BPT][R];
#pragma unroll
    for (int b = 0; b < BPT; ++b) {
        const int j = t + b * kMsThreads;
        if (j < M) {
#pragma unroll
            for (int q = 0; q < R; ++q) v[b][q] = z[j + q * M];
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < BPT; ++b) {
        const int j = t + b * kMsThreads;
        if (j < M) {
            const int k = j & (ns - 1), step = M / ns;
            if (ns > 1) {
#pragma unroll
                for (int q = 1; q < R; ++q) v[b][q] = cmul(v[b][q], tw[q * k * step]);
            }
            dft_small<R>(v[b], -1.0);
            const int j0 = (j - k) * R + k;
#pragma unroll
            for (int q = 0; q < R; ++q) z[j0 + q * ns] = v[b][q];
        }
    }
    __syncthreads();
}

template <int LOG2N>
__device__ __forceinline__ void ms_fft_lds(cplx* z, const cplx* __restrict__ tw, int t) {
    constexpr int kEights = LOG2N / 3, kRest = LOG2N - 3 * kEights;
    int ns = 1;
#pragma unroll
    for (int s = 0; s < kEights; ++s) { ms_fft_pass<LOG2N, 8>(z, tw, t, ns); ns <<= 3; }
    if (kRest == 2) ms_fft_pass<LOG2N, 4>(z, tw, t, ns);
    if (kRest == 1) ms_fft_pass<LOG2N, 2>(z, tw, t, ns);
}

// frame f of the list = n_fft samples from piece pieces.idx[f / fpp] at offset (f % fpp) n_fft inside it, fpp = p / n_fft whole frames per
// piece.  Workgroup g sums the frames [g T / G, (g + 1) T / G) in ascending order: partial[g][0][k] for mid, [g][1][k] for side.
template <int LOG2N>
__global__ void __launch_bounds__(kMsThreads)
ms_spectrum_kernel(const double* __restrict__ mid, const double* __restrict__ side, int64_t p, MsPieces pieces, int64_t fpp, int64_t T,
                   double scale, const cplx* __restrict__ tw, double* __restrict__ partial) {
    constexpr int N = 1 << LOG2N, K = N / 2 + 1;
    cplx* z = (cplx*)alsep_smem;
    const int t = threadIdx.x;
    const int64_t G = gridDim.x, g = blockIdx.x, f0 = g * T / G, f1 = (g + 1) * T / G;
    const double inv = scale / (double)N;
    double am[kMsBinsPer], as[kMsBinsPer];
#pragma unroll
    for (int c = 0; c < kMsBinsPer; ++c) { am[c] = 0.0; as[c] = 0.0; }
    for (int64_t f = f0; f < f1; ++f) {
        const int64_t start = (int64_t)pieces.idx[f / fpp] * p + (f % fpp) * N;
        for (int j = t; j < N; j += kMsThreads) z[j] = cplx{mid[start + j], side[start + j]};
        __syncthreads();
        ms_fft_lds<LOG2N>(z, tw, t);
#pragma unroll
        for (int c = 0; c < kMsBinsPer; ++c) {
            const int k = t + c * kMsThreads;
            if (k < K) {
                cplx A, B;
                split_spectra(z[k], z[(N - k) & (N - 1)], &A, &B);
                am[c] = am[c] + hypot(A.x, A.y) * inv;
                as[c] = as[c] + hypot(B.x, B.y) * inv;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < kMsBinsPer; ++c) {
        const int k = t + c * kMsThreads;
        if (k < K) {
            partial[(g * 2 + 0) * K + k] = am[c];
            partial[(g * 2 + 1) * K + k] = as[c];
        }
    }
}

// out[ch][k] = (sum over the groups in index order of partial[g][ch][k]) / T
__global__ void __launch_bounds__(kMsThreads)
ms_spectrum_final_kernel(const double* __restrict__ partial, int64_t G, int64_t K, int64_t T, double* __restrict__ out) {
    const int64_t total = 2 * K;
    for (int64_t i = (int64_t)blockIdx.x * kMsThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kMsThreads) {
        double acc = 0.0;
        for (int64_t g = 0; g < G; ++g) acc = acc + partial[g * total + i];
        out[i] = acc / (double)T;
    }
}

bool ms_nfft_ok(int n_fft) { return n_fft >= 256 && n_fft <= 8192 && (n_fft & (n_fft - 1)) == 0; }

int64_t ms_spec_groups(int64_t T) { return T < kMsSpecGroups ? T : kMsSpecGroups; }

// ---- "same" convolution: the overlap-save blocks of reverb.hip, float64 in and out ---------------------------------------------------
// block b's outputs L-1 .. F-1 are samples t = (b0 + b) S + q of the full convolution; "same" keeps t - off in [0, n), off = (L - 1) / 2
__global__ void __launch_bounds__(kRvThreads)
ola_same_kernel(const cplx* __restrict__ z, double* __restrict__ y, int64_t n, int log2F, int64_t S, int64_t L, int64_t off, int64_t b0,
                int64_t blocks) {
    const int64_t total = blocks * S;
    for (int64_t i = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRvThreads) {
        const int64_t b = i / S, q = i - b * S, o = (b0 + b) * S + q - off;
        if (o < 0 || o >= n) continue;
        y[o] = z[(b << log2F) + (L - 1) + q].x;
    }
}

// ---- sliding maxima -----------------------------------------------------------------------------------------------------------------
// out[i] = max x[i - left .. i - left + W - 1] for i in the tile [i0, i0 + Tt); centred: W = 2 w - 1, indices outside [0, n) reflected about
// the edges with the edge sample repeated (scipy's "reflect"); trailing: W = w, indices below 0 left out.  left = w - 1 in both.
// PER: LDS elements per thread -- 64 (a tile of 16384, 128 KB) for the long windows, 16 (32 KB, five workgroups per CU) up to kMsSlideShort.
template <int PER>
__global__ void __launch_bounds__(kMsThreads)
ms_slide_max_kernel(const double* __restrict__ x, int64_t n, int w, int centred, int64_t Tt, double* __restrict__ out) {
    double* m = (double*)alsep_smem;
    const int t = threadIdx.x;
    const int W = centred ? 2 * w - 1 : w, left = w - 1;
    const int64_t i0 = (int64_t)blockIdx.x * Tt;
    const int64_t cnt = n - i0 < Tt ? n - i0 : Tt;
    const int E = (int)cnt + W - 1;                                          // <= PER * kMsThreads
    for (int e = t; e < E; e += kMsThreads) {
        int64_t s = i0 - left + e;
        double v = -INFINITY;
        if (centred) {
            if (s < 0) s = -s - 1;
            if (s >= n) s = 2 * n - 1 - s;
            v = x[s];
        } else if (s >= 0) {
            v = x[s];
        }
        m[e] = v;
    }
    __syncthreads();
    int P = 1;
    while (2 * P <= W) {
        double v[PER];
#pragma unroll
        for (int c = 0; c < PER; ++c) {
            const int e = t + c * kMsThreads;
            v[c] = 0.0;
            if (e < E) v[c] = e + P < E ? ms_max(m[e], m[e + P]) : m[e];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < PER; ++c) {
            const int e = t + c * kMsThreads;
            if (e < E) m[e] = v[c];
        }
        __syncthreads();
        P *= 2;
    }
    for (int j = t; j < (int)cnt; j += kMsThreads) out[i0 + j] = ms_max(m[j], m[j + W - P]);
}

// ---- first-order IIR ------------------------------------------------------------------------------------------------------------------
// sample i of the filter's own order is x[rev ? n - 1 - i : i], and so for y
__device__ __forceinline__ int64_t ms_at(int64_t i, int64_t n, int rev) { return rev ? n - 1 - i : i; }

// LDS rows of the tile are padded by one element per thread's run of E (element e lives at e + e / E): the threads walk their runs side by
// side, E + 1 elements apart instead of E (16 at the default chunk, where every lane would meet the same banks)
__global__ void __launch_bounds__(kMsThreads)
ms_iir_local_kernel(const double* __restrict__ x, int64_t n, int rev, int C, double b0, double b1, double q, double zi,
                    const double* __restrict__ zi_src, double* __restrict__ y, double* __restrict__ ends) {
    double* xs = (double*)alsep_smem;                                        // [C + 256]
    double* ys = xs + (C + kMsThreads);                                      // [C + 256]
    double* tail = ys + (C + kMsThreads);                                    // [256], then the sample before the chunk
    const int t = threadIdx.x;
    const int64_t c = blockIdx.x, i0 = c * C;
    const int len = (int)(n - i0 < C ? n - i0 : C);
    const int E = (C + kMsThreads - 1) / kMsThreads;
    for (int e = t; e < len; e += kMsThreads) xs[e + e / E] = x[ms_at(i0 + e, n, rev)];
    if (t == 0) tail[kMsThreads] = c > 0 ? x[ms_at(i0 - 1, n, rev)] : 0.0;
    __syncthreads();
    const int e0 = t * E, e1 = e0 + E < len ? e0 + E : len;
    // chunk 0 starts from the caller's state z = zi * (*zi_src): y[0] = b0 x[0] + z
    double prev = 0.0;
    if (e0 < e1) {
        double xp = t > 0 ? xs[e0 - 1 + (t - 1)] : tail[kMsThreads];
        for (int e = e0; e < e1; ++e) {
            const double xc = xs[e + t];
            double u = b0 * xc + b1 * xp;
            if (c == 0 && e == 0) u = b0 * xc + zi * (zi_src ? zi_src[0] : 1.0);
            prev = u + q * prev;
            ys[e + t] = prev;
            xp = xc;
        }
    }
    tail[t] = e0 < e1 ? prev : 0.0;
    __syncthreads();
    // inclusive scan of the threads' end values: a thread past the end of the tile carries q^E times its predecessor, which nobody reads
    double qh = ms_powi(q, E);
    for (int h = 1; h < kMsThreads; h <<= 1) {
        const double add = t >= h ? qh * tail[t - h] : 0.0;
        __syncthreads();
        tail[t] = tail[t] + add;
        __syncthreads();
        qh = qh * qh;
    }
    const double carry = t > 0 ? tail[t - 1] : 0.0;
    double pw = q;
    for (int e = e0; e < e1; ++e) {
        ys[e + t] = ys[e + t] + pw * carry;
        pw = pw * q;
    }
    __syncthreads();
    for (int e = t; e < len; e += kMsThreads) y[ms_at(i0 + e, n, rev)] = ys[e + e / E];
    if (t == 0) ends[c] = ys[len - 1 + (len - 1) / E];
}

__global__ void __launch_bounds__(kMsThreads)
ms_iir_fix_kernel(double* __restrict__ y, int64_t n, int rev, int C, double q, const double* __restrict__ ends) {
    for (int64_t i = (int64_t)C + (int64_t)blockIdx.x * kMsThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kMsThreads) {
        const int64_t c = i / C, o = ms_at(i, n, rev);
        y[o] = y[o] + ms_powi(q, i - c * C + 1) * ends[c - 1];
    }
}

// scipy.signal's odd extension by kMsPad samples on both sides
__global__ void __launch_bounds__(kMsThreads)
ms_odd_ext_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ ext) {
    const int64_t total = n + 2 * kMsPad;
    for (int64_t i = (int64_t)blockIdx.x * kMsThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kMsThreads) {
        const int64_t j = i - kMsPad;
        double v;
        if (j < 0) v = 2.0 * x[0] - x[-j];
        else if (j >= n) v = 2.0 * x[n - 1] - x[2 * (n - 1) - j];
        else v = x[j];
        ext[i] = v;
    }
}

int ms_iir_chunk(int chunk) { return chunk == 0 ? kMsIirDefaultChunk : chunk; }

// the scan's workspace in doubles: the chunk ends, and where there is more than one chunk their scanned values and that scan's own workspace
int64_t ms_iir_ws_doubles(int64_t n, int C) {
    const int64_t m = ceil_div64(n, C);
    return m > 1 ? 2 * m + ms_iir_ws_doubles(m, kMsIirDefaultChunk) : m;
}

// y = the filter over x.  The carry pass over the m chunk ends -- end[c] += q^C end[c - 1], every chunk but the last being full -- is the
// same recurrence with b0 = 1, b1 = 0 and the pole q^C: the scan of the ends is this function again, in chunks of 4096 (one workgroup up
// to 16.7 million samples at the default chunk)
int ms_iir_run(alsep_ctx* ctx, const double* x, int64_t n, double b0, double b1, double a1, double zi, const double* zi_src, int rev, int C,
               double* y, double* ws) {
    const double q = -a1;
    const int64_t chunks = ceil_div64(n, C);
    double* ends = ws;
    const size_t lds = ((size_t)2 * (C + kMsThreads) + kMsThreads + 1) * sizeof(double);
    ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)ms_iir_local_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ms_iir_local_kernel, dim3((unsigned)chunks), dim3(kMsThreads), lds, ctx->stream, x, n, rev, C, b0, b1, q, zi, zi_src, y, ends);
    ALSEP_LAUNCH_CHECK(ctx, "ms_iir_local_kernel");
    if (chunks > 1) {
        double qc = 1.0, b = q;                                              // q^C as ms_powi computes it
        for (int64_t m = C; m > 0; m >>= 1) { if (m & 1) qc = qc * b; b = b * b; }
        double* scanned = ws + chunks;
        if (int rc = ms_iir_run(ctx, ends, chunks, 1.0, 0.0, -qc, 0.0, nullptr, 0, kMsIirDefaultChunk, scanned, scanned + chunks)) return rc;
        hipLaunchKernelGGL(ms_iir_fix_kernel, dim3(rv_grid(n - C)), dim3(kMsThreads), 0, ctx->stream, y, n, rev, C, q, (const double*)scanned);
        ALSEP_LAUNCH_CHECK(ctx, "ms_iir_fix_kernel");
    }
    return ALSEP_OK;
}

bool ms_iir_args_ok(int64_t n, int chunk, double a1) {
    return n >= 1 && n <= kMsMaxSamples && (chunk == 0 || (chunk >= 1 && chunk <= kMsIirMaxChunk)) && a1 == a1 && fabs(a1) <= 1.0;
}

// ---- limiter front and back -----------------------------------------------------------------------------------------------------------
// g = 1 - 1 / rect, rect = max(max(|L|, |R|), threshold) / threshold; *over = 1 when some rect is not numpy.isclose to 1
__global__ void __launch_bounds__(kMsThreads)
ms_rectify_kernel(const double* __restrict__ l, const double* __restrict__ r, int64_t n, double threshold, double* __restrict__ g,
                  int32_t* __restrict__ over) {
    bool hit = false;
    for (int64_t j = (int64_t)blockIdx.x * kMsThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kMsThreads) {
        const double rect = ms_max(ms_max(fabs(l[j]), fabs(r[j])), threshold) / threshold;
        g[j] = 1.0 - 1.0 / rect;
        if (!(fabs(rect - 1.0) <= 1e-8 + 1e-5)) hit = true;
    }
    if (hit) over[0] = 1;                                                    // every writer stores the same word
}

__global__ void __launch_bounds__(kMsThreads)
ms_maximum_kernel(const double* __restrict__ a, const double* __restrict__ b, int64_t n, double* __restrict__ out) {
    for (int64_t j = (int64_t)blockIdx.x * kMsThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kMsThreads) out[j] = ms_max(a[j], b[j]);
}

// gain = 1 - max(s_h, g_a, max(h, rel)); out = [L, R] gain; block maxima of |out|
__global__ void __launch_bounds__(kMsThreads)
ms_limit_apply_kernel(const double* __restrict__ l, const double* __restrict__ r, int64_t n, const double* __restrict__ s_h,
                      const double* __restrict__ g_a, const double* __restrict__ h, const double* __restrict__ rel, double* __restrict__ ol,
                      double* __restrict__ orr, double* __restrict__ gain, double* __restrict__ partial) {
    double m = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * kMsThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kMsThreads) {
        const double k = 1.0 - ms_max(ms_max(s_h[j], g_a[j]), ms_max(h[j], rel[j]));
        const double a = l[j] * k, b = r[j] * k;
        ol[j] = a;
        orr[j] = b;
        if (gain) gain[j] = k;
        m = ms_max(m, ms_max(fabs(a), fabs(b)));
    }
    ms_tree_max((double*)alsep_smem, m);
    if (threadIdx.x == 0) partial[blockIdx.x] = ((double*)alsep_smem)[0];
}

// res = x / divisor; 24-bit PCM as libsndfile writes doubles: rint(res 8388607) (ties to even), clipped, little-endian, interleaved
__global__ void __launch_bounds__(kMsThreads)
ms_pcm24_kernel(const double* __restrict__ l, const double* __restrict__ r, int64_t n, double divisor, double* __restrict__ rl,
                double* __restrict__ rr, uint8_t* __restrict__ pcm) {
    for (int64_t j = (int64_t)blockIdx.x * kMsThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kMsThreads) {
        const double a = l[j] / divisor, b = r[j] / divisor;
        rl[j] = a;
        rr[j] = b;
        double qa = rint(a * 8388607.0), qb = rint(b * 8388607.0);
        qa = qa < -8388607.0 ? -8388607.0 : qa > 8388607.0 ? 8388607.0 : qa;
        qb = qb < -8388607.0 ? -8388607.0 : qb > 8388607.0 ? 8388607.0 : qb;
        const uint32_t ua = (uint32_t)(int32_t)qa, ub = (uint32_t)(int32_t)qb;
        uint8_t* o = pcm + 6 * j;
        o[0] = (uint8_t)ua; o[1] = (uint8_t)(ua >> 8); o[2] = (uint8_t)(ua >> 16);
        o[3] = (uint8_t)ub; o[4] = (uint8_t)(ub >> 8); o[5] = (uint8_t)(ub >> 16);
    }
}

bool ms_rows_ok(const void* p, int64_t n, int64_t ld) { return p && n >= 1 && n <= kMsMaxSamples && ld >= n; }

}  // namespace

extern "C" int alsep_master_midside(alsep_ctx* ctx, const double* lr, int64_t n, int64_t ld, double divisor, double* ms, int64_t ld_ms) {
    ALSEP_ENTER(ctx);
    if (!ctx || !ms_rows_ok(lr, n, ld) || !ms_rows_ok(ms, n, ld_ms) || !(divisor > 0.0))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_midside: bad argument");
    hipLaunchKernelGGL(ms_midside_kernel, dim3(rv_grid(n)), dim3(kMsThreads), 0, ctx->stream, lr, lr + ld, n, divisor, ms, ms + ld_ms);
    ALSEP_LAUNCH_CHECK(ctx, "ms_midside_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_master_leftright(alsep_ctx* ctx, const double* ms, int64_t n, int64_t ld_ms, double scale, double* lr, int64_t ld) {
    ALSEP_ENTER(ctx);
    if (!ctx || !ms_rows_ok(ms, n, ld_ms) || !ms_rows_ok(lr, n, ld) || !(scale == scale))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_leftright: bad argument");
    hipLaunchKernelGGL(ms_leftright_kernel, dim3(rv_grid(n)), dim3(kMsThreads), 0, ctx->stream, ms, ms + ld_ms, n, scale, lr, lr + ld);
    ALSEP_LAUNCH_CHECK(ctx, "ms_leftright_kernel");
    return ALSEP_OK;
}

extern "C" int64_t alsep_master_workspace_bytes(void) {
    const int64_t a = (int64_t)kMsPieces * kMsPieceBlocks, b = (int64_t)kMsSpecGroups * 2 * kMsMaxBins, c = kMsPeakBlocks;
    return (a > b ? (a > c ? a : c) : (b > c ? b : c)) * (int64_t)sizeof(double);
}

// sums[j] = the sum of the squares of x[j p .. (j + 1) p), or of clip(scale x, -1, 1) when clip != 0, j < d
extern "C" int alsep_master_piece_sumsq(alsep_ctx* ctx, const double* x, int64_t n, int d, int64_t p, double scale, int clip, double* sums,
                                        void* ws, int64_t ws_bytes) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !sums || !ws || n < 1 || n > kMsMaxSamples || d < 1 || d > kMsPieces || p < 1 || (int64_t)d * p > n || !(scale == scale))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_piece_sumsq: bad argument (1 <= d <= %d pieces of p samples inside n)", kMsPieces);
    if (ws_bytes < alsep_master_workspace_bytes()) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_piece_sumsq: workspace too small");
    const unsigned G = ms_piece_blocks(p);
    const size_t lds = kCmpThreads * sizeof(double);
    hipLaunchKernelGGL(ms_piece_partial_kernel, dim3(G, (unsigned)d), dim3(kMsThreads), lds, ctx->stream, x, p, scale, clip, (double*)ws);
    ALSEP_LAUNCH_CHECK(ctx, "ms_piece_partial_kernel");
    hipLaunchKernelGGL(ms_rows_sum_kernel, dim3((unsigned)d), dim3(kMsThreads), lds, ctx->stream, (const double*)ws, (int)G, sums);
    ALSEP_LAUNCH_CHECK(ctx, "ms_rows_sum_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_master_peak(alsep_ctx* ctx, const double* x, int rows, int64_t n, int64_t ld, double* peak, void* ws, int64_t ws_bytes) {
    ALSEP_ENTER(ctx);
    if (!ctx || !ms_rows_ok(x, n, ld) || rows < 1 || rows > 2 || !peak || !ws) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_peak: bad argument");
    if (ws_bytes < alsep_master_workspace_bytes()) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_peak: workspace too small");
    const unsigned blocks = ms_peak_blocks((int64_t)rows * n);
    const size_t lds = kMsThreads * sizeof(double);
    hipLaunchKernelGGL(ms_peak_partial_kernel, dim3(blocks), dim3(kMsThreads), lds, ctx->stream, x, rows, n, ld, (double*)ws);
    ALSEP_LAUNCH_CHECK(ctx, "ms_peak_partial_kernel");
    hipLaunchKernelGGL(ms_peak_final_kernel, dim3(1), dim3(kMsThreads), lds, ctx->stream, (const double*)ws, (int)blocks, peak);
    ALSEP_LAUNCH_CHECK(ctx, "ms_peak_final_kernel");
    return ALSEP_OK;
}

// out[0][k], out[1][k], k <= n_fft / 2: the mean over the listed pieces' whole n_fft-sample frames of |rfft(scale mid)| / n_fft and of side's
extern "C" int alsep_master_spectrum(alsep_ctx* ctx, const double* ms, int64_t n, int64_t ld_ms, int64_t p, const int32_t* pieces, int n_pieces,
                                     int n_fft, double scale, const double* twiddle, double* out, void* ws, int64_t ws_bytes) {
    ALSEP_ENTER(ctx);
    if (!ctx || !ms_rows_ok(ms, n, ld_ms) || !pieces || !twiddle || !out || !ws || n_pieces < 1 || n_pieces > kMsPieces || !(scale >= 0.0))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_spectrum: bad argument");
    if (!ms_nfft_ok(n_fft) || p < n_fft)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_spectrum: n_fft %d (a power of two, 256 .. 8192) in pieces of %lld samples", n_fft, (long long)p);
    if (ws_bytes < alsep_master_workspace_bytes()) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_spectrum: workspace too small");
    MsPieces list;
    for (int i = 0; i < kMsPieces; ++i) list.idx[i] = 0;
    for (int i = 0; i < n_pieces; ++i) {
        if (pieces[i] < 0 || ((int64_t)pieces[i] + 1) * p > n) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_spectrum: piece %d lies outside the track", pieces[i]);
        list.idx[i] = pieces[i];
    }
    const int64_t fpp = p / n_fft, T = fpp * n_pieces, G = ms_spec_groups(T), K = n_fft / 2 + 1;
    const size_t lds = (size_t)n_fft * sizeof(cplx);
    const dim3 grid((unsigned)G), block(kMsThreads);
    const double* mid = ms;
    const double* side = ms + ld_ms;
    const cplx* tw = (const cplx*)twiddle;
    double* partial = (double*)ws;
#define ALSEP_MS_SPECTRUM(L2)                                                                                                              \
    do {                                                                                                                                   \
        ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)ms_spectrum_kernel<L2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));    \
        hipLaunchKernelGGL(ms_spectrum_kernel<L2>, grid, block, lds, ctx->stream, mid, side, p, list, fpp, T, scale, tw, partial);         \
    } while (0)
    switch (n_fft) {
        case 256: ALSEP_MS_SPECTRUM(8); break;
        case 512: ALSEP_MS_SPECTRUM(9); break;
        case 1024: ALSEP_MS_SPECTRUM(10); break;
        case 2048: ALSEP_MS_SPECTRUM(11); break;
        case 4096: ALSEP_MS_SPECTRUM(12); break;
        default: ALSEP_MS_SPECTRUM(13); break;
    }
#undef ALSEP_MS_SPECTRUM
    ALSEP_LAUNCH_CHECK(ctx, "ms_spectrum_kernel");
    hipLaunchKernelGGL(ms_spectrum_final_kernel, dim3(rv_grid(2 * K)), block, 0, ctx->stream, (const double*)partial, G, K, T, out);
    ALSEP_LAUNCH_CHECK(ctx, "ms_spectrum_final_kernel");
    return ALSEP_OK;
}

extern "C" int64_t alsep_master_convolve_workspace_bytes(int64_t n_fir, int log2_block, int blocks_per_batch) {
    return alsep_reverb_apply_workspace_bytes(n_fir, log2_block, blocks_per_batch);
}

// out[c] = scale * scipy.signal.fftconvolve(x[c], fir[c], "same"), c < channels: float64 [channels][n] rows, fir float64 [channels][n_fir]
extern "C" int alsep_master_convolve_same(alsep_ctx* ctx, const double* x, int channels, int64_t n, int64_t ld, const double* fir, int64_t n_fir,
                                          double scale, int log2_block, double* out, int64_t ld_out, void* ws, int64_t ws_bytes) {
    ALSEP_ENTER(ctx);
    if (!ctx || !ms_rows_ok(x, n, ld) || !ms_rows_ok(out, n, ld_out) || !fir || !ws || channels < 1 || !(scale == scale))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_convolve_same: bad argument");
    const int k = ola_block_log2(n_fir, log2_block);
    if (k < 0)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_convolve_same: FIR of %lld taps (1 .. %lld) or block exponent %d (2^k >= 2 taps, k <= 21)",
                          (long long)n_fir, (long long)kMaxIrTaps, log2_block);
    const double *x_end = x + ((int64_t)(channels - 1) * ld + n), *out_end = out + ((int64_t)(channels - 1) * ld_out + n);
    if (x < out_end && out < x_end) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_convolve_same: out overlaps x");
    OlaPlan plan;
    if (!ola_plan(k, n_fir, ws, ws_bytes, &plan)) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_convolve_same: workspace too small");
    const int64_t off = (n_fir - 1) / 2, n_blocks = ceil_div64(off + n, plan.S);
    for (int c = 0; c < channels; ++c) {
        if (int rc = ola_ir_spectrum(ctx, plan, fir + (int64_t)c * n_fir, scale / (double)plan.F)) return rc;
        double* y = out + (int64_t)c * ld_out;
        auto finish = [&](const cplx* z, int64_t b0, int64_t nb) {
            hipLaunchKernelGGL(ola_same_kernel, dim3(rv_grid(nb * plan.S)), dim3(kRvThreads), 0, ctx->stream, z, y, n, plan.k, plan.S, plan.L, off, b0, nb);
            ALSEP_LAUNCH_CHECK(ctx, "ola_same_kernel");
            return (int)ALSEP_OK;
        };
        if (int rc = ola_run<double>(ctx, plan, x + (int64_t)c * ld, (const double*)nullptr, n, n_blocks, finish)) return rc;
    }
    return ALSEP_OK;
}

// out[i] = max x[i - (w - 1) .. i + (w - 1)] with scipy's "reflect" edges (centred != 0), or max x[max(0, i - w + 1) .. i]
extern "C" int alsep_master_slide_max(alsep_ctx* ctx, const double* x, int64_t n, int w, int centred, double* out) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !out || x == out || n < 1 || n > kMsMaxSamples || w < 1 || 2 * (int64_t)w - 1 > kMsMaxWindow)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_slide_max: bad argument (windows of up to %d samples)", kMsMaxWindow);
    if (n < 2 * (int64_t)w - 1) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_slide_max: %lld samples are fewer than 2 w - 1 = %d", (long long)n, 2 * w - 1);
    const int W = centred ? 2 * w - 1 : w;
    const bool small = W <= kMsSlideShort;
    const int64_t elems = small ? kMsSlideElemsShort : kMsSlideElems, Tt = elems - (W - 1);
    const size_t lds = (size_t)elems * sizeof(double);
    const dim3 grid((unsigned)ceil_div64(n, Tt)), block(kMsThreads);
    if (small) {
        hipLaunchKernelGGL(ms_slide_max_kernel<kMsSlideElemsShort / kMsThreads>, grid, block, lds, ctx->stream, x, n, w, centred, Tt, out);
    } else {
        ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)ms_slide_max_kernel<kMsSlidePer>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(ms_slide_max_kernel<kMsSlidePer>, grid, block, lds, ctx->stream, x, n, w, centred, Tt, out);
    }
    ALSEP_LAUNCH_CHECK(ctx, "ms_slide_max_kernel");
    return ALSEP_OK;
}

extern "C" int64_t alsep_master_iir_workspace_bytes(int64_t n, int chunk) {
    if (!ms_iir_args_ok(n, chunk, 0.0)) return -1;
    return ms_iir_ws_doubles(n, ms_iir_chunk(chunk)) * (int64_t)sizeof(double);
}

// scipy.signal.lfilter([b0, b1], [1, a1], x, zi=[zi]) (reverse == 0), or the same over x[::-1] with the result stored back in x's order
extern "C" int alsep_master_iir(alsep_ctx* ctx, const double* x, int64_t n, double b0, double b1, double a1, double zi, int reverse, int chunk,
                                double* y, void* ws, int64_t ws_bytes) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !y || !ws || x == y || !ms_iir_args_ok(n, chunk, a1))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_iir: bad argument (chunks of 1 .. %d samples, |a1| <= 1)", kMsIirMaxChunk);
    if (ws_bytes < alsep_master_iir_workspace_bytes(n, chunk)) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_iir: workspace too small");
    return ms_iir_run(ctx, x, n, b0, b1, a1, zi, nullptr, reverse ? 1 : 0, ms_iir_chunk(chunk), y, (double*)ws);
}

extern "C" int64_t alsep_master_filtfilt_workspace_bytes(int64_t n, int chunk) {
    if (!ms_iir_args_ok(n, chunk, 0.0)) return -1;
    const int64_t ne = n + 2 * kMsPad;
    return (2 * ne + ms_iir_ws_doubles(ne, ms_iir_chunk(chunk))) * (int64_t)sizeof(double);
}

// scipy.signal.filtfilt([b0, b1], [1, a1], x) with its defaults: odd extension by 6 samples, both passes started from zi times the first
// sample they see; zi = scipy.signal.lfilter_zi(b, a)[0], computed by the caller
extern "C" int alsep_master_filtfilt(alsep_ctx* ctx, const double* x, int64_t n, double b0, double b1, double a1, double zi, int chunk, double* y,
                                     void* ws, int64_t ws_bytes) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !y || !ws || !ms_iir_args_ok(n, chunk, a1))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_filtfilt: bad argument (chunks of 1 .. %d samples, |a1| <= 1)", kMsIirMaxChunk);
    if (n <= kMsPad) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_filtfilt: %lld samples; the padding needs more than %d", (long long)n, kMsPad);
    if (ws_bytes < alsep_master_filtfilt_workspace_bytes(n, chunk)) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_filtfilt: workspace too small");
    const int64_t ne = n + 2 * kMsPad;
    const int C = ms_iir_chunk(chunk);
    double* ext = (double*)ws;
    double* fwd = ext + ne;
    double* ends = fwd + ne;
    hipLaunchKernelGGL(ms_odd_ext_kernel, dim3(rv_grid(ne)), dim3(kMsThreads), 0, ctx->stream, x, n, ext);
    ALSEP_LAUNCH_CHECK(ctx, "ms_odd_ext_kernel");
    if (int rc = ms_iir_run(ctx, ext, ne, b0, b1, a1, zi, ext, 0, C, fwd, ends)) return rc;
    // backwards over the forward result, from zi times its last sample; the result lands over ext, in the signal's own order
    if (int rc = ms_iir_run(ctx, fwd, ne, b0, b1, a1, zi, fwd + (ne - 1), 1, C, ext, ends)) return rc;
    ALSEP_HIP(ctx, hipMemcpyAsync(y, ext + kMsPad, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return ALSEP_OK;
}

extern "C" int alsep_master_rectify(alsep_ctx* ctx, const double* lr, int64_t n, int64_t ld, double threshold, double* g, int32_t* over) {
    ALSEP_ENTER(ctx);
    if (!ctx || !ms_rows_ok(lr, n, ld) || !g || !over || !(threshold > 0.0)) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_rectify: bad argument");
    ALSEP_HIP(ctx, hipMemsetAsync(over, 0, sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(ms_rectify_kernel, dim3(rv_grid(n)), dim3(kMsThreads), 0, ctx->stream, lr, lr + ld, n, threshold, g, over);
    ALSEP_LAUNCH_CHECK(ctx, "ms_rectify_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_master_maximum(alsep_ctx* ctx, const double* a, const double* b, int64_t n, double* out) {
    ALSEP_ENTER(ctx);
    if (!ctx || !a || !b || !out || n < 1 || n > kMsMaxSamples) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_maximum: bad argument");
    hipLaunchKernelGGL(ms_maximum_kernel, dim3(rv_grid(n)), dim3(kMsThreads), 0, ctx->stream, a, b, n, out);
    ALSEP_LAUNCH_CHECK(ctx, "ms_maximum_kernel");
    return ALSEP_OK;
}

// gain = 1 - max(s_h, g_a, max(h, rel)) (optional output); out = lr * gain; *peak (device) = max|out|
extern "C" int alsep_master_limit_apply(alsep_ctx* ctx, const double* lr, int64_t n, int64_t ld, const double* s_h, const double* g_a, const double* h,
                                        const double* rel, double* out, int64_t ld_out, double* gain, double* peak, void* ws, int64_t ws_bytes) {
    ALSEP_ENTER(ctx);
    if (!ctx || !ms_rows_ok(lr, n, ld) || !ms_rows_ok(out, n, ld_out) || !s_h || !g_a || !h || !rel || !peak || !ws)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_limit_apply: bad argument");
    if (ws_bytes < alsep_master_workspace_bytes()) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_limit_apply: workspace too small");
    const unsigned blocks = ms_peak_blocks(n);
    const size_t lds = kMsThreads * sizeof(double);
    hipLaunchKernelGGL(ms_limit_apply_kernel, dim3(blocks), dim3(kMsThreads), lds, ctx->stream, lr, lr + ld, n, s_h, g_a, h, rel, out, out + ld_out, gain,
                       (double*)ws);
    ALSEP_LAUNCH_CHECK(ctx, "ms_limit_apply_kernel");
    hipLaunchKernelGGL(ms_peak_final_kernel, dim3(1), dim3(kMsThreads), lds, ctx->stream, (const double*)ws, (int)blocks, peak);
    ALSEP_LAUNCH_CHECK(ctx, "ms_peak_final_kernel");
    return ALSEP_OK;
}

// result = lr / divisor (float64 [2][n], not lr itself); pcm: uint8 [6 n]
extern "C" int alsep_master_pcm24(alsep_ctx* ctx, const double* lr, int64_t n, int64_t ld, double divisor, double* result, int64_t ld_res, uint8_t* pcm) {
    ALSEP_ENTER(ctx);
    if (!ctx || !ms_rows_ok(lr, n, ld) || !ms_rows_ok(result, n, ld_res) || !pcm || !(divisor > 0.0))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_master_pcm24: bad argument");
    hipLaunchKernelGGL(ms_pcm24_kernel, dim3(rv_grid(n)), dim3(kMsThreads), 0, ctx->stream, lr, lr + ld, n, divisor, result, result + ld_res, pcm);
    ALSEP_LAUNCH_CHECK(ctx, "ms_pcm24_kernel");
    return ALSEP_OK;
}
