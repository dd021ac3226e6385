// RVC's NSF-HiFiGAN vocoder (the reference's GeneratorNSF, modules/rvc/infer/lib/infer_pack/models.py:313-566) -- the operators the other
// networks' building blocks do not have.  Included at the end of nn.hip: float32 (the source's phase in float64), channels-last [L, C],
// built without packed float32.  gfx950 only.  The contractions are exact f32 on v_mfma_f32_16x16x4_f32 through mma.h;
// the context's split-contraction switch (alsep_nn_set_contraction) does NOT apply to these kernels.
//
//   source   : SourceModuleHnNSF / SineGen with no overtones.  The phase at the start of frame t is the sum of the per-frame steps before
//              it, taken modulo 1; the steps are the reference's float32 values, their sum is float64.  The scan runs in chunks of a
//              FIXED 1024 frames whatever the launch geometry: every chunk's exclusive prefix (a fixed tree per chunk), one thread's serial
//              scan over the at most 1024 chunk totals, then har = tanh(w (0.1 sin(2 pi rad) uv + amp noise) + b) per sample.
//   conv1d   : the pre-activation dilated convolution of ResBlock1 as an implicit GEMM.  A workgroup of 4 waves owns 128 positions by
//              16 NCO output channels (NCO = 4, 2 or 1 by what divides Cout; channel counts that are multiples of 8 but not of 16 -- the
//              last stage of a network that starts narrow -- run NCO = 1 with the missing channels masked to zero).  Input channels go
//              through LDS 32 (16) at a time: the tile's 128 + d (K - 1) rows are staged ONCE per chunk with the LeakyReLU applied while
//              staging (rows outside [0, L) are zero), rows 4 floats apart from a power of two so that the 16-byte fragment reads of 8
//              neighbouring lanes fall on distinct banks.
//              The K taps walk the staged rows.  In the MFMA the weights are the A operand (rows = output channels, read from L2 where
//              the packed [K][Cin][Cout] keeps 16 lanes contiguous) and the positions the B operand, so that a lane ends up with 4
//              consecutive channels of one position: bias, residual, running sum, tanh and scale are 16-byte accesses in the epilogue.
//   conv_post: LeakyReLU(0.01), 7 taps, C -> 1, tanh: a reduction.  4 lanes per position, each a 16-byte column slice, two shuffles.
//   tconv1d  : ConvTranspose1d(K, stride u, padding (K - u) / 2) of LeakyReLU(0.1)(x) + bias + the stage's noise convolution of the source.
//              Output row m u + r takes the inputs m - j through the taps r + p + j u: for one phase r that is a convolution with
//              ceil(K / u) taps or one fewer (at most 8) over the input rows, so the kernel above runs it with blockIdx.z = r, its tap
//              walk going down the weight taps by u and its epilogue writing row m u + r.  No [L][K Cout] intermediate and no fold pass; the noise convolution (2 s products per
//              output) is summed in the same epilogue.

namespace {

constexpr int kNsfThreads = 256, kNsfTL = 128, kNsfScan = 1024;
constexpr int64_t kNsfMaxFrames = (int64_t)1 << 20;
constexpr int kNsfMaxUpp = 1024;
constexpr int kNsfMaxPhaseTaps = 8;                                          // taps of one output phase of a transposed convolution: ceil(K / u)

// the reference's float32 step of frame t: fmod(f0 / sr * upp + 0.5, 1) - 0.5, every operation rounded on its own
__device__ __forceinline__ float nsf_step(float f0, float sr, float upp) {
#pragma clang fp contract(off)
    const float q = f0 / sr;
    const float r = q * upp;
    const float h = r + 0.5f;
    return fmodf(h, 1.0f) - 0.5f;
}

// chunk b = blockIdx.x of 1024 frames: loc [t] = the sum of the steps of the chunk's frames before t, part [b] = the chunk's total
__global__ void __launch_bounds__(kNsfThreads)
nsf_scan_local_kernel(const float* __restrict__ f0, int64_t T, float sr, float upp, double* __restrict__ loc, double* __restrict__ part) {
    double* sh = reinterpret_cast<double*>(alsep_smem);                       // [2][256]
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * kNsfScan + 4 * tid;
    double s[4];
    double run = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        s[e] = run;                                                          // exclusive inside the thread
        if (t0 + e < T) run += (double)nsf_step(f0[t0 + e], sr, upp);
    }
    int cur = 0;
    sh[tid] = run;
    __syncthreads();
    for (int o = 1; o < kNsfThreads; o <<= 1) {                               // inclusive scan of the 256 thread totals
        const double v = sh[cur * kNsfThreads + tid] + (tid >= o ? sh[cur * kNsfThreads + tid - o] : 0.0);
        sh[(cur ^ 1) * kNsfThreads + tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    const double before = tid ? sh[cur * kNsfThreads + tid - 1] : 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (t0 + e < T) loc[t0 + e] = before + s[e];
    if (tid == kNsfThreads - 1) part[blockIdx.x] = sh[cur * kNsfThreads + tid];
}

// part [nb] -> its exclusive prefix, in order
__global__ void nsf_scan_parts_kernel(double* __restrict__ part, int nb) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double run = 0.0;
    for (int b = 0; b < nb; ++b) {
        const double v = part[b];
        part[b] = run;
        run += v;
    }
}

__global__ void __launch_bounds__(kNsfThreads)
nsf_har_kernel(const float* __restrict__ f0, const float* __restrict__ noise, const double* __restrict__ loc, const double* __restrict__ part,
               int64_t n, int upp, float sr, float lw, float lb, float* __restrict__ har) {
    for (int64_t i = (int64_t)blockIdx.x * kNsfThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNsfThreads) {
        const int64_t t = i / upp;
        const int j = (int)(i - t * upp) + 1;
        const float f = f0[t];
        const double sum = part[t / kNsfScan] + loc[t];
        const double acc = sum - trunc(sum);                                 // fmod(., 1), truncating toward zero
        const double rad = (double)(f / sr) * (double)j + acc;
        const float sine = 0.1f * (float)sin(2.0 * M_PI * (rad - floor(rad)));
        const bool uv = f > 0.f;
        const float amp = uv ? 0.003f : 0.1f / 3.f;
        const float v = (uv ? sine : 0.f) + amp * noise[i];
        har[i] = tanhf(fmaf(lw, v, lb));
    }
}

struct NsfGemm {
    const float* x; const float* w; float* y;
    int64_t L;
    int Cin, Cout;
    float pre_slope;
    // convolution: nt taps, input row = position + off0 + t dstep, weight tap t
    int nt, off0, dstep;
    const float* bias; const float* res; const float* acc;
    int post;
    float out_scale;
    // transposed convolution: stride u, padding p, K taps; the noise convolution of har [Lh] by nw [ks][Cout] + nb, stride s, padding pn
    int u, p, K;
    const float* har; const float* nw; const float* nb;
    int64_t Lh;
    int s, ks, pn;
};

// MODE 0: y [L, Cout] = out_scale (acc + post(conv + bias + res)); MODE 1: phase blockIdx.z of the transposed convolution.
// LDS: [128 + (nt - 1) dstep][CK + 4] floats, CK = 32 where 32 divides Cin, else 16.
// FULL: 16 divides Cin and Cout; otherwise (multiples of 8) the channels beyond either read as zero and are not written.
template <int NCO, int MODE, bool FULL>
__global__ void __launch_bounds__(kNsfThreads)
nsf_gemm_kernel(NsfGemm g) {
    float* xs = reinterpret_cast<float*>(alsep_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    int nt = g.nt, off0 = g.off0, dstep = g.dstep, w0 = 0, wstep = 1;
    const int r = MODE == 1 ? (int)blockIdx.z : 0;
    if (MODE == 1) {                                                         // taps r + p + j u, j = jmax down to jmin, on the inputs m - j
        const int jmin = -((r + g.p) / g.u), jmax = (g.K - 1 - r - g.p) / g.u;
        nt = jmax - jmin + 1;
        off0 = -jmax;
        dstep = 1;
        w0 = r + g.p + jmax * g.u;
        wstep = -g.u;
    }
    const int64_t l0 = (int64_t)blockIdx.x * kNsfTL;
    const int co0 = (int)blockIdx.y * 16 * NCO;
    const int CK = g.Cin % 32 == 0 ? 32 : 16, ld = CK + 4, vec = CK / 4;
    const int rows = kNsfTL + (nt - 1) * dstep;
    const float slope = g.pre_slope;
    f32x4 acc[2][NCO];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int ct = 0; ct < NCO; ++ct) acc[pt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < g.Cin; c0 += CK) {
        for (int i = tid; i < rows * vec; i += kNsfThreads) {
            const int rr = i / vec, j = i - rr * vec;
            const int64_t pos = l0 + off0 + rr;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (pos >= 0 && pos < g.L && (FULL || c0 + 4 * j < g.Cin)) {
                v = *reinterpret_cast<const f32x4*>(g.x + pos * g.Cin + c0 + 4 * j);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? v[e] * slope : v[e];
            }
            *reinterpret_cast<f32x4*>(xs + rr * ld + 4 * j) = v;
        }
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const float* wt = g.w + ((int64_t)(w0 + t * wstep) * g.Cin + c0 + 4 * quad) * g.Cout + co0 + col;
            const float* xr = xs + (wave * 32 + t * dstep + col) * ld + 4 * quad;
            for (int s = 0; s < CK / 16; ++s) {
                const f32x4 b0 = lds_frag(xr + 16 * s), b1 = lds_frag(xr + 16 * ld + 16 * s);
#pragma unroll
                for (int ct = 0; ct < NCO; ++ct) {
                    f32x4 a;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        a[e] = (FULL || (c0 + 16 * s + 4 * quad + e < g.Cin && co0 + 16 * ct + col < g.Cout)) ? wt[(int64_t)(16 * s + e) * g.Cout + 16 * ct]
                                                                                                       : 0.f;
                    mma_step(acc[0][ct], a, b0);
                    mma_step(acc[1][ct], a, b1);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        const int64_t pos = l0 + wave * 32 + 16 * pt + col;
        if (pos >= g.L) continue;
        const int64_t row = MODE == 1 ? pos * g.u + r : pos;
#pragma unroll
        for (int ct = 0; ct < NCO; ++ct) {
            const int co = co0 + 16 * ct + 4 * quad;
            if (!FULL && co >= g.Cout) continue;
            float v[4] = {acc[pt][ct][0], acc[pt][ct][1], acc[pt][ct][2], acc[pt][ct][3]};
            float q[4];
            if (g.bias) {
                load4(g.bias + co, q);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += q[e];
            }
            if (MODE == 0) {
                if (g.res) {
                    load4(g.res + row * g.Cout + co, q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += q[e];
                }
                if (g.post == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = tanhf(v[e]);
                }
                if (g.acc) {
                    load4(g.acc + row * g.Cout + co, q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += q[e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] *= g.out_scale;
            } else {
                float sum[4];
                load4(g.nb + co, sum);
                const int64_t h0 = row * g.s - g.pn;
                for (int k = 0; k < g.ks; ++k) {
                    const int64_t hi = h0 + k;
                    if (hi < 0 || hi >= g.Lh) continue;
                    const float hv = g.har[hi];
                    load4(g.nw + (int64_t)k * g.Cout + co, q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) sum[e] = fmaf(hv, q[e], sum[e]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += sum[e];
            }
            store4(g.y + row * g.Cout + co, v);
        }
    }
}

// y [L] = tanh(sum over 7 taps and C channels of lrelu(x [l + k - 3][c], 0.01) w [k][c]); 4 lanes per position
__global__ void __launch_bounds__(kNsfThreads)
nsf_conv_post_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, int64_t L, int C) {
    const int sub = threadIdx.x & 3;
    const int64_t groups = (int64_t)gridDim.x * (kNsfThreads / 4);
    // every lane of a wave runs the same number of rounds: the shuffles below need all 64
    for (int64_t base = (int64_t)blockIdx.x * (kNsfThreads / 4); base < L; base += groups) {
        const int64_t l = base + (threadIdx.x >> 2);
        float sum = 0.f;
        if (l < L) {
            for (int k = 0; k < 7; ++k) {
                const int64_t pos = l + k - 3;
                if (pos < 0 || pos >= L) continue;
                const float* xr = x + pos * C;
                const float* wr = w + k * C;
                for (int c = 4 * sub; c < C; c += 16) {
                    float a[4], b[4];
                    load4(xr + c, a);
                    load4(wr + c, b);
#pragma unroll
                    for (int e = 0; e < 4; ++e) sum = fmaf(a[e] < 0.f ? a[e] * 0.01f : a[e], b[e], sum);
                }
            }
        }
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        if (l < L && sub == 0) y[l] = tanhf(sum);
    }
}

bool nsf_aligned(const void* p) { return !p || !((uintptr_t)p & 15); }

template <int MODE>
int nsf_launch_gemm(alsep_ctx* ctx, const NsfGemm& g, int nt_max, int dstep, unsigned phases, const char* name) {
    const int CK = g.Cin % 32 == 0 ? 32 : 16;
    const size_t lds = sizeof(float) * (size_t)(kNsfTL + (nt_max - 1) * dstep) * (CK + 4);
    const unsigned gx = (unsigned)ceil_div64(g.L, kNsfTL);
    if (g.Cin % 16 || g.Cout % 16)
        hipLaunchKernelGGL((nsf_gemm_kernel<1, MODE, false>), dim3(gx, (unsigned)((g.Cout + 15) / 16), phases), dim3(kNsfThreads), lds, ctx->stream, g);
    else if (g.Cout % 64 == 0)
        hipLaunchKernelGGL((nsf_gemm_kernel<4, MODE, true>), dim3(gx, (unsigned)(g.Cout / 64), phases), dim3(kNsfThreads), lds, ctx->stream, g);
    else if (g.Cout % 32 == 0)
        hipLaunchKernelGGL((nsf_gemm_kernel<2, MODE, true>), dim3(gx, (unsigned)(g.Cout / 32), phases), dim3(kNsfThreads), lds, ctx->stream, g);
    else
        hipLaunchKernelGGL((nsf_gemm_kernel<1, MODE, true>), dim3(gx, (unsigned)(g.Cout / 16), phases), dim3(kNsfThreads), lds, ctx->stream, g);
    ALSEP_LAUNCH_CHECK(ctx, name);
    return ALSEP_OK;
}

}  // namespace

extern "C" int64_t alsep_nsf_source_workspace_bytes(int64_t T) {
    if (T < 1 || T > kNsfMaxFrames) return -1;
    return (int64_t)sizeof(double) * (T + ceil_div64(T, kNsfScan));
}

extern "C" int alsep_nsf_source(alsep_ctx* ctx, const float* f0, int64_t T, int upp, int sr, const float* noise, float lin_w, float lin_b,
                                float* har, void* workspace, int64_t workspace_bytes) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && f0 && noise && har && workspace && noise != har && !((uintptr_t)workspace & 7), "alsep_nsf_source");
    if (T < 1 || T > kNsfMaxFrames || upp < 1 || upp > kNsfMaxUpp || sr < 1)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_source: %lld frames (1 .. %lld), upp %d (1 .. %d), sr %d", (long long)T,
                          (long long)kNsfMaxFrames, upp, kNsfMaxUpp, sr);
    if (workspace_bytes < alsep_nsf_source_workspace_bytes(T))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_source: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                          (long long)alsep_nsf_source_workspace_bytes(T));
    const int nb = (int)ceil_div64(T, kNsfScan);
    double* loc = static_cast<double*>(workspace);
    double* part = loc + T;
    hipLaunchKernelGGL(nsf_scan_local_kernel, dim3((unsigned)nb), dim3(kNsfThreads), sizeof(double) * 2 * kNsfThreads, ctx->stream, f0, T, (float)sr,
                       (float)upp, loc, part);
    ALSEP_LAUNCH_CHECK(ctx, "nsf_scan_local_kernel");
    hipLaunchKernelGGL(nsf_scan_parts_kernel, dim3(1), dim3(64), 0, ctx->stream, part, nb);
    ALSEP_LAUNCH_CHECK(ctx, "nsf_scan_parts_kernel");
    const int64_t n = T * upp;
    hipLaunchKernelGGL(nsf_har_kernel, dim3(ew_grid(n)), dim3(kNsfThreads), 0, ctx->stream, f0, noise, (const double*)loc, (const double*)part, n, upp,
                       (float)sr, lin_w, lin_b, har);
    ALSEP_LAUNCH_CHECK(ctx, "nsf_har_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_nsf_conv1d(alsep_ctx* ctx, const float* x, const float* w, const float* bias, const float* res, const float* acc, float* y,
                                int64_t L, int Cin, int Cout, int K, int dilation, float pre_slope, int post, float out_scale) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && x && w && y && x != y && L > 0 && L < ((int64_t)1 << 31), "alsep_nsf_conv1d");
    if (Cin < 8 || Cout < 8 || Cin % 8 || Cout % 8 || Cin > 4096 || Cout > 4096)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_conv1d: %d -> %d channels (multiples of 8, at most 4096)", Cin, Cout);
    if (K < 1 || K > 11 || K % 2 == 0) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_conv1d: kernel size %d (odd, 1 .. 11)", K);
    if (dilation < 1 || dilation > 5) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_conv1d: dilation %d (1 .. 5)", dilation);
    if (post != 0 && post != 1) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_conv1d: post %d (0 none, 1 tanh)", post);
    if (!(nsf_aligned(x) && nsf_aligned(w) && nsf_aligned(bias) && nsf_aligned(res) && nsf_aligned(acc) && nsf_aligned(y)))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_conv1d: a pointer is not 16-byte aligned");
    NsfGemm g{};
    g.x = x; g.w = w; g.y = y; g.L = L; g.Cin = Cin; g.Cout = Cout; g.pre_slope = pre_slope;
    g.nt = K; g.off0 = -dilation * (K - 1) / 2; g.dstep = dilation;
    g.bias = bias; g.res = res; g.acc = acc; g.post = post; g.out_scale = out_scale;
    ProfScope prof(ctx, ALSEP_PROF_NN_CONV);
    prof.work(2.0 * (double)L * Cin * Cout * K, 4.0 * ((double)L * Cin + (double)L * Cout * (1 + (res != nullptr) + (acc != nullptr)) + (double)K * Cin * Cout));
    return nsf_launch_gemm<0>(ctx, g, K, dilation, 1, "nsf_gemm_kernel");
}

extern "C" int alsep_nsf_conv_post(alsep_ctx* ctx, const float* x, const float* w, float* y, int64_t L, int C) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && x && w && y && x != y && L > 0 && L < ((int64_t)1 << 31) && nsf_aligned(x) && nsf_aligned(w), "alsep_nsf_conv_post");
    if (C < 8 || C % 8 || C > 4096) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_conv_post: %d channels (a multiple of 8, at most 4096)", C);
    int64_t blocks = ceil_div64(L, kNsfThreads / 4);
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(nsf_conv_post_kernel, dim3((unsigned)blocks), dim3(kNsfThreads), 0, ctx->stream, x, w, y, L, C);
    ALSEP_LAUNCH_CHECK(ctx, "nsf_conv_post_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_nsf_tconv1d(alsep_ctx* ctx, const float* x, const float* w, const float* bias, const float* har, const float* noise_w,
                                 const float* noise_b, float* y, int64_t L, int Cin, int Cout, int K, int u, int s) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && x && w && bias && har && noise_w && noise_b && y && x != y && L > 0, "alsep_nsf_tconv1d");
    if (Cin < 8 || Cout < 8 || Cin % 8 || Cout % 8 || Cin > 4096 || Cout > 4096)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_tconv1d: %d -> %d channels (multiples of 8, at most 4096)", Cin, Cout);
    if (u < 1 || u > 64 || K < u || K > kNsfMaxPhaseTaps * u || (K - u) % 2)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_tconv1d: kernel %d at stride %d (stride 1 .. 64, stride <= kernel <= %d stride, "
                                              "kernel - stride even)", K, u, kNsfMaxPhaseTaps);
    if (s < 1 || s > kNsfMaxUpp || (s > 1 && s % 2))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_tconv1d: source stride %d (1, or even up to %d)", s, kNsfMaxUpp);
    if (L * u >= ((int64_t)1 << 31) || L * u * s >= ((int64_t)1 << 40))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_tconv1d: %lld positions at stride %d, source stride %d: too long", (long long)L, u, s);
    if (!(nsf_aligned(x) && nsf_aligned(w) && nsf_aligned(bias) && nsf_aligned(noise_w) && nsf_aligned(noise_b) && nsf_aligned(y)))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nsf_tconv1d: a pointer is not 16-byte aligned");
    NsfGemm g{};
    g.x = x; g.w = w; g.y = y; g.L = L; g.Cin = Cin; g.Cout = Cout; g.pre_slope = 0.1f;
    g.bias = bias; g.u = u; g.p = (K - u) / 2; g.K = K;
    g.har = har; g.nw = noise_w; g.nb = noise_b; g.Lh = L * u * s; g.s = s; g.ks = s > 1 ? 2 * s : 1; g.pn = s > 1 ? s / 2 : 0;
    ProfScope prof(ctx, ALSEP_PROF_NN_CONV);
    prof.work(2.0 * (double)L * Cin * Cout * K + 2.0 * (double)L * u * Cout * g.ks, 4.0 * ((double)L * Cin + (double)L * u * Cout + (double)K * Cin * Cout));
    return nsf_launch_gemm<1>(ctx, g, (K + u - 1) / u, 1, (unsigned)u, "nsf_gemm_kernel");
}
