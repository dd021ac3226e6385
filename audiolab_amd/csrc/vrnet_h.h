// The VR networks in half precision (VRNet / VRNetNew(precision="f16")): channels-last IEEE half activations [B, H = bins, W = frames, C].
// Included by nn_half.hip (built without packed float32), inside its translation unit, after nn_demucs_h.h.
//
//   vr_conv_h_kernel      implicit-GEMM convolution on v_mfma_f32_16x16x32_f16, the tiling of nn_dconv_h_kernel (128 pixels x 16 NJ
//                         channels, K = (dy, dx, ci) in steps of 32, weights [Cout][Kp] half).  Beyond it: the folded BatchNorm as a
//                         float32 scale / shift per channel in the epilogue (not folded into the half weights: the reference's half model
//                         keeps BatchNorm apart), none / ReLU / LeakyReLU, output into a channel slice of a wider tensor, half or float32
//                         -- and, FUSED, the decoder's input read from its two sources: channels [0, Cu) interpolated on the fly (bilinear
//                         x2, align_corners) from the half-resolution map, channels [Cu, Cu + Cs) from the skip at its crop offset.  The
//                         interpolation is float32 from half inputs, rounded once to half as it is staged: the bits vr_resize_h_kernel
//                         writes (both call vr_bilerp), so the fused and the unfused path agree bit for bit.
//   vr_depthwise_h_kernel, vr_resize_h_kernel, vr_copy_slice_h_kernel, vr_mean_hh_kernel
//                         the small kernels of vrnet.hip on half tensors (float32 arithmetic, one rounding on the way out)

namespace {

// source index and weight of torch's area_pixel_compute_source_index(align_corners=True) along one axis.  The weight is ONE fused
// multiply-add, s o - i0, spelled out: written as a product and a difference hipcc contracts it in one kernel and not in another (a
// pragma does not stop it under -ffp-contract=fast), and the fused decoder input must stage the bits vr_resize_h_kernel writes.
// vr_bilerp likewise leaves no product next to a sum for the compiler to fuse.
__device__ __forceinline__ void vr_src_index(int o, int n_in, float s, int& i0, int& i1, float& l) {
    i0 = min((int)(s * (float)o), n_in - 1);
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l = fmaf(s, (float)o, -(float)i0);
}

// A float32 value that is about to be rounded to half stays a float32 value first.  Where hipcc sees a fused multiply-add and the
// conversion together it folds them into v_fma_mixlo_f16 -- ONE rounding instead of two -- and it does so in one kernel and not in
// another (seen: vr_resize_h_kernel yes, the fused staging of vr_conv_h_kernel no).  No instruction is emitted for this.
__device__ __forceinline__ float vr_pin(float v) {
#ifndef ALSEP_CPU_EMUL
    asm volatile("" : "+v"(v));
#endif
    return v;
}

// hy (hx v00 + lx v01) + ly (hx v10 + lx v11) with every fused multiply-add spelled out, rounded to float32 and then to half: the same
// bits wherever it is inlined
__device__ __forceinline__ _Float16 vr_bilerp(float v00, float v01, float v10, float v11, float ly, float lx) {
    const float hx = 1.f - lx, hy = 1.f - ly;
    const float t0 = fmaf(lx, v01, hx * v00), t1 = fmaf(lx, v11, hx * v10);
    return (_Float16)vr_pin(fmaf(ly, t1, hy * t0));
}

// ReLU as torch's: a NaN stays a NaN (fmaxf would return 0 and hide a half overflow's inf - inf from the runner's non-finite guard)
__device__ __forceinline__ float vr_act_h(float v, int act) {
    if (act == 1) return v < 0.f ? 0.f : v;
    if (act == 2) return v > 0.f ? v : 0.01f * v;
    return v;
}

struct VrConvHArgs {
    const _Float16* x;                  // the input [B, H, W, Cin]; FUSED: the half-resolution map [B, Hu, Wu, Cu]
    const _Float16* skip;               // FUSED: the skip [B, H, Ws, Cs], read at columns w_off + ix
    const _Float16* w; const float* scale; const float* shift; void* y;
    int npix, H, W, Cin, K, Kp, KW, stride, ph, pw, dh, dw, Ho, Wo, Cout, y_ct, y_c0;
    int act, y_f16, y_vec;
    int Hu, Wu, Cu, Ws, Cs, w_off;      // FUSED: H = 2 Hu, W = 2 Wu, Cin = Cu + Cs
    float sy, sx;                       // FUSED: (Hu - 1) / (H - 1), (Wu - 1) / (W - 1)
};

// VEC: a staging granule (8 consecutive k of one pixel) is one 16-byte load (Cin % 8 == 0; FUSED: Cu % 8 == 0 and Cs % 8 == 0, so a
// granule has one tap and one source); otherwise every element finds its own tap and source.
template <int NJ, bool VEC, bool FUSED>
__global__ void __launch_bounds__(kHThreads)
vr_conv_h_kernel(VrConvHArgs p) {
    constexpr int BN = 16 * NJ;
    constexpr int NBG = (BN * 4 + kHThreads - 1) / kHThreads;               // weight granules per thread
    constexpr int NR = FUSED && VEC ? 4 : 1;                                  // raw 16-byte loads per granule: the four corners
    _Float16* As = reinterpret_cast<_Float16*>(alsep_smem);                  // [128][40]
    _Float16* Bs = As + kDcBM * kDcLd;                                        // [BN][40]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int tiles_n = (p.Cout + BN - 1) / BN;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (wg / tiles_n) * kDcBM, n0 = (wg % tiles_n) * BN;
    const int ag = tid & 3, ar = tid >> 2;                                    // A granule (row ar + 64 h, k group ag)
    int pimg[2], py[2], px[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int pix = m0 + ar + 64 * h;
        const bool ok = pix < p.npix;
        const int pc = ok ? pix : 0;
        const int img = pc / (p.Ho * p.Wo), rem = pc - img * (p.Ho * p.Wo);
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        pimg[h] = img;
        py[h] = ok ? oy * p.stride - p.ph : -0x40000000;                      // a row beyond the last pixel: every tap "outside"
        px[h] = ox * p.stride - p.pw;
    }
    h16x8 zh;
#pragma unroll
    for (int e = 0; e < 8; ++e) zh[e] = (_Float16)0.f;
    h16x8 raw[2][NR], rb[NBG];
    int mode[2];                                                              // VEC: 0 zeros, 1 plain / skip granule, 2 interpolated
    float gly[2], glx[2];
    // one element of the convolution's input at (image, iy, ix, ci), inside the image
    auto elem = [&](int img, int iy, int ix, int ci) -> _Float16 {
        if constexpr (!FUSED) return p.x[(unsigned)(((img * p.H + iy) * p.W + ix) * p.Cin + ci)];
        if (ci >= p.Cu) return p.skip[(unsigned)(((img * p.H + iy) * p.Ws + p.w_off + ix) * p.Cs + ci - p.Cu)];
        int y0, y1, x0, x1;
        float ly, lx;
        vr_src_index(iy, p.Hu, p.sy, y0, y1, ly);
        vr_src_index(ix, p.Wu, p.sx, x0, x1, lx);
        const _Float16* xb = p.x + (unsigned)(img * p.Hu * p.Wu * p.Cu + ci);
        const unsigned r0 = (unsigned)(y0 * p.Wu), r1 = (unsigned)(y1 * p.Wu);
        return vr_bilerp((float)xb[(r0 + x0) * p.Cu], (float)xb[(r0 + x1) * p.Cu], (float)xb[(r1 + x0) * p.Cu],
                                   (float)xb[(r1 + x1) * p.Cu], ly, lx);
    };
    auto gload = [&](int k0) {
        const int k = k0 + 8 * ag;
        const int tap0 = k / p.Cin, ci0 = k - tap0 * p.Cin;
        const int dy0 = tap0 / p.KW, dx0 = tap0 - dy0 * p.KW;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (VEC) {
                const int iy = py[h] + dy0 * p.dh, ix = px[h] + dx0 * p.dw;
                const bool in = k < p.K && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
                if constexpr (!FUSED) {
                    const unsigned off = in ? (unsigned)(((pimg[h] * p.H + iy) * p.W + ix) * p.Cin + ci0) : 0u;
                    raw[h][0] = *reinterpret_cast<const h16x8*>(p.x + off);
                    mode[h] = in ? 1 : 0;
                } else {
                    // every load unconditional (a load under a branch collapses the prefetch): lanes that need no corner read element 0
                    const bool up = in && ci0 < p.Cu, sk = in && !up;
                    int y0, y1, x0, x1;
                    vr_src_index(in ? iy : 0, p.Hu, p.sy, y0, y1, gly[h]);
                    vr_src_index(in ? ix : 0, p.Wu, p.sx, x0, x1, glx[h]);
                    const unsigned base = (unsigned)(pimg[h] * p.Hu * p.Wu * p.Cu + ci0);
                    const unsigned r0 = (unsigned)(y0 * p.Wu), r1 = (unsigned)(y1 * p.Wu);
                    const unsigned o00 = up ? base + (r0 + x0) * p.Cu : 0u, o01 = up ? base + (r0 + x1) * p.Cu : 0u;
                    const unsigned o10 = up ? base + (r1 + x0) * p.Cu : 0u, o11 = up ? base + (r1 + x1) * p.Cu : 0u;
                    const unsigned os = sk ? (unsigned)(((pimg[h] * p.H + iy) * p.Ws + p.w_off + ix) * p.Cs + ci0 - p.Cu) : 0u;
                    const _Float16* first = sk ? p.skip + os : p.x + o00;
                    raw[h][0] = *reinterpret_cast<const h16x8*>(first);
                    raw[h][1] = *reinterpret_cast<const h16x8*>(p.x + o01);
                    raw[h][2] = *reinterpret_cast<const h16x8*>(p.x + o10);
                    raw[h][3] = *reinterpret_cast<const h16x8*>(p.x + o11);
                    mode[h] = up ? 2 : sk ? 1 : 0;
                }
            } else {
                int ci = ci0, dy = dy0, dx = dx0;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int iy = py[h] + dy * p.dh, ix = px[h] + dx * p.dw;
                    const bool in = k + e < p.K && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
                    raw[h][0][e] = in ? elem(pimg[h], iy, ix, ci) : (_Float16)0.f;
                    if (++ci == p.Cin) {
                        ci = 0;
                        if (++dx == p.KW) { dx = 0; ++dy; }
                    }
                }
                mode[h] = 1;
            }
        }
#pragma unroll
        for (int h = 0; h < NBG; ++h) {
            const int gi = tid + kHThreads * h;
            const int row = min(n0 + (gi >> 2), p.Cout - 1);                   // rows beyond Cout: products never stored
            if (gi < BN * 4) rb[h] = *reinterpret_cast<const h16x8*>(p.w + ((unsigned)row * (unsigned)p.Kp + (unsigned)(k0 + 8 * (gi & 3))));
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            h16x8 v = mode[h] ? raw[h][0] : zh;
            if constexpr (FUSED && VEC) {
                if (mode[h] == 2) {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        v[e] = vr_bilerp((float)raw[h][0][e], (float)raw[h][1][e], (float)raw[h][2][e],
                                                   (float)raw[h][3][e], gly[h], glx[h]);
                }
            }
            *reinterpret_cast<h16x8*>(As + (ar + 64 * h) * kDcLd + 8 * ag) = v;
        }
#pragma unroll
        for (int h = 0; h < NBG; ++h) {
            const int gi = tid + kHThreads * h;
            if (gi < BN * 4) *reinterpret_cast<h16x8*>(Bs + (gi >> 2) * kDcLd + 8 * (gi & 3)) = rb[h];
        }
    };
    f32x4 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nk = p.Kp / kDcBK;
    gload(0);
    for (int kt = 0; kt < nk; ++kt) {
        lstore();
        __syncthreads();
        if (kt + 1 < nk) gload((kt + 1) * kDcBK);
        h16x8 af[2], bf[NJ];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const h16x8*>(As + (wave * 32 + 16 * i + l15) * kDcLd + 8 * lq);
#pragma unroll
        for (int j = 0; j < NJ; ++j) bf[j] = *reinterpret_cast<const h16x8*>(Bs + (16 * j + l15) * kDcLd + 8 * lq);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[i][j], 0, 0, 0);
        __syncthreads();
    }
    // epilogue: channels n0 + 16 j + 4 lq + r of pixel m0 + 32 wave + 16 i + l15
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int pix = m0 + wave * 32 + 16 * i + l15;
        if (pix >= p.npix) continue;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = n0 + 16 * j + 4 * lq;
            if (col >= p.Cout) continue;
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = min(col + r, p.Cout - 1);
                v[r] = vr_pin(vr_act_h(fmaf(acc[i][j][r], p.scale[co], p.shift[co]), p.act));   // plain and FUSED instantiations round alike
            }
            const int64_t o = (int64_t)pix * p.y_ct + p.y_c0 + col;
            if (p.y_f16) {
                _Float16* y = reinterpret_cast<_Float16*>(p.y) + o;
                if (p.y_vec && col + 3 < p.Cout) {
                    h16x4 hv;
                    hv[0] = (_Float16)v[0]; hv[1] = (_Float16)v[1]; hv[2] = (_Float16)v[2]; hv[3] = (_Float16)v[3];
                    *reinterpret_cast<h16x4*>(y) = hv;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (col + r < p.Cout) y[r] = (_Float16)v[r];
                }
            } else {
                float* y = reinterpret_cast<float*>(p.y) + o;
                if (p.y_vec && col + 3 < p.Cout) {
                    *reinterpret_cast<f32x4*>(y) = v;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (col + r < p.Cout) y[r] = v[r];
                }
            }
        }
    }
}

// depthwise KH x KW (groups = C), stride 1, same-size output: x [B,H,W,C], w [C][KH][KW] half, float32 accumulation
__global__ void __launch_bounds__(kHThreads)
vr_depthwise_h_kernel(const _Float16* __restrict__ x, const _Float16* __restrict__ w, _Float16* __restrict__ y, unsigned n, int H, int W, int C,
                      int KH, int KW, int pad, int dil) {
    const unsigned i = blockIdx.x * kHThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned c = i % (unsigned)C, pp = i / (unsigned)C;
    const int ox = (int)(pp % (unsigned)W), oy = (int)((pp / (unsigned)W) % (unsigned)H);
    const unsigned b = pp / (unsigned)(W * H);
    const _Float16* xb = x + b * (unsigned)(H * W * C) + c;
    float s = 0.f;
    for (int ky = 0; ky < KH; ++ky)
        for (int kx = 0; kx < KW; ++kx) {
            const int iy = oy - pad + ky * dil, ix = ox - pad + kx * dil;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) s = fmaf((float)xb[(unsigned)((iy * W + ix) * C)], (float)w[(c * KH + ky) * KW + kx], s);
        }
    y[i] = (_Float16)s;
}

// bilinear resize, align_corners=True: x [B,H,W,C] -> y [B,Ho,Wo,y_ct] channel slice
__global__ void __launch_bounds__(kHThreads)
vr_resize_h_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ y, unsigned n, int H, int W, int C, int Ho, int Wo, int y_ct, int y_c0,
                   float sy, float sx) {
    const unsigned i = blockIdx.x * kHThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned c = i % (unsigned)C, pp = i / (unsigned)C;
    const int ox = (int)(pp % (unsigned)Wo), oy = (int)((pp / (unsigned)Wo) % (unsigned)Ho);
    const unsigned b = pp / (unsigned)(Wo * Ho);
    int y0, y1, x0, x1;
    float ly, lx;
    vr_src_index(oy, H, sy, y0, y1, ly);
    vr_src_index(ox, W, sx, x0, x1, lx);
    const _Float16* xb = x + b * (unsigned)(H * W * C) + c;
    const unsigned r0 = (unsigned)(y0 * W), r1 = (unsigned)(y1 * W);
    y[(int64_t)pp * y_ct + y_c0 + c] = vr_bilerp((float)xb[(r0 + x0) * C], (float)xb[(r0 + x1) * C], (float)xb[(r1 + x0) * C],
                                                          (float)xb[(r1 + x1) * C], ly, lx);
}

// y[b, h, wq, y_c0 + c] = x[b, h, w_off + wq, c]
__global__ void __launch_bounds__(kHThreads)
vr_copy_slice_h_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ y, unsigned n, int Wx, int C, int w_off, int Wy, int y_ct, int y_c0) {
    const unsigned i = blockIdx.x * kHThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned c = i % (unsigned)C, pp = i / (unsigned)C;
    const unsigned wq = pp % (unsigned)Wy, row = pp / (unsigned)Wy;
    y[(int64_t)pp * y_ct + y_c0 + c] = x[(row * Wx + w_off + wq) * C + c];
}

// y[b, 0, w, c] = mean_h x[b, h, w, c], summed in float32 in row order
__global__ void __launch_bounds__(kHThreads)
vr_mean_hh_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ y, unsigned n, int H, int W, int C) {
    const unsigned i = blockIdx.x * kHThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned wc_n = (unsigned)(W * C), b = i / wc_n, wc = i % wc_n;
    const _Float16* xb = x + b * (unsigned)H * wc_n + wc;
    float s = 0.f;
    for (int h = 0; h < H; ++h) s += (float)xb[(unsigned)h * wc_n];
    y[i] = (_Float16)(s / (float)H);
}

constexpr int64_t kVrhMax = (int64_t)1 << 31;                               // the kernels index with 32 bits

static int vr_conv_h_launch(alsep_ctx* ctx, VrConvHArgs& p, bool vec, bool fused, const char* what) {
    if (p.Kp < p.K || p.Kp % kDcBK) return alsep_fail(ctx, ALSEP_ERR_ARG, "%s: Kp must be >= KH KW Cin and a multiple of 32", what);
    if ((int64_t)p.Cout * p.Kp >= kVrhMax || (int64_t)p.npix * p.y_ct >= kVrhMax)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "%s: an operand of 2^31 or more elements (32-bit offsets)", what);
    if ((uintptr_t)p.w & 15) return alsep_fail(ctx, ALSEP_ERR_ARG, "%s: weights must be 16-byte aligned", what);
    p.y_vec = p.y_ct % 4 == 0 && p.y_c0 % 4 == 0 && !((uintptr_t)p.y & (p.y_f16 ? 7 : 15));
    // 16 NJ channels per workgroup: the widest tile that covers Cout, narrowed while the grid would leave most of the chip idle (the deep
    // levels of the U-Nets: a few thousand pixels, a long K loop)
    int NJ = p.Cout <= 16 ? 1 : p.Cout <= 32 ? 2 : p.Cout <= 64 ? 4 : 8;
    const int64_t tiles_m = ceil_div64(p.npix, kDcBM);
    while (NJ > 2 && tiles_m * ceil_div64(p.Cout, 16 * NJ) < 2 * device_cu_count(ctx)) NJ >>= 1;
    const int64_t n_wg = tiles_m * ceil_div64(p.Cout, 16 * NJ);
    if (n_wg > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "%s: too many tiles", what);
#define ALSEP_VC_GO(NJ_, VEC_, FUSED_)                                                                                                      \
    hipLaunchKernelGGL((vr_conv_h_kernel<NJ_, VEC_, FUSED_>), dim3((unsigned)n_wg), dim3(kHThreads), dconv_h_lds<NJ_>(), ctx->stream, p)
#define ALSEP_VC_NJ(VEC_, FUSED_)                                                                                                           \
    do {                                                                                                                                    \
        if (NJ == 1) ALSEP_VC_GO(1, VEC_, FUSED_); else if (NJ == 2) ALSEP_VC_GO(2, VEC_, FUSED_);                                          \
        else if (NJ == 4) ALSEP_VC_GO(4, VEC_, FUSED_); else ALSEP_VC_GO(8, VEC_, FUSED_);                                                  \
    } while (0)
    if (fused) {
        if (vec) ALSEP_VC_NJ(true, true); else ALSEP_VC_NJ(false, true);
    } else {
        if (vec) ALSEP_VC_NJ(true, false); else ALSEP_VC_NJ(false, false);
    }
#undef ALSEP_VC_NJ
#undef ALSEP_VC_GO
    return ALSEP_OK;
}

}  // namespace

// y[pixel][y_coff + co] = act(scale[co] sum_{tap, ci} x[pixel's tap][ci] w[co][tap ci] + shift[co]): x, w IEEE half, y half or float32
extern "C" int alsep_vr_conv_h(alsep_ctx* ctx, const void* x, const void* w, const float* scale, const float* shift, void* y, int y_f16, int64_t B,
                               int H, int W, int Cin, int Cout, int Kp, int KH, int KW, int stride, int pad_h, int pad_w, int dil_h, int dil_w,
                               int act, int y_ctotal, int y_coff) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !w || !scale || !shift || !y) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_conv_h: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad_h < 0 || pad_w < 0 || dil_h <= 0 ||
        dil_w <= 0 || act < 0 || act > 2 || y_coff < 0 || y_coff + Cout > y_ctotal)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_conv_h: bad shape");
    const int Ho = (H + 2 * pad_h - dil_h * (KH - 1) - 1) / stride + 1, Wo = (W + 2 * pad_w - dil_w * (KW - 1) - 1) / stride + 1;
    if (Ho <= 0 || Wo <= 0) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_conv_h: empty output");
    const int64_t npix = B * Ho * Wo;
    if (B * (int64_t)H * W * Cin >= kVrhMax || npix >= kVrhMax - kDcBM || (int64_t)KH * KW * Cin >= kVrhMax)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_conv_h: an operand of 2^31 or more elements (32-bit offsets)");
    VrConvHArgs p{};
    p.x = (const _Float16*)x; p.skip = nullptr; p.w = (const _Float16*)w; p.scale = scale; p.shift = shift; p.y = y;
    p.npix = (int)npix; p.H = H; p.W = W; p.Cin = Cin; p.K = KH * KW * Cin; p.Kp = Kp; p.KW = KW; p.stride = stride; p.ph = pad_h; p.pw = pad_w;
    p.dh = dil_h; p.dw = dil_w; p.Ho = Ho; p.Wo = Wo; p.Cout = Cout; p.y_ct = y_ctotal; p.y_c0 = y_coff; p.act = act; p.y_f16 = y_f16 ? 1 : 0;
    const bool vec = Cin % 8 == 0 && !((uintptr_t)x & 15);
    const int rc = vr_conv_h_launch(ctx, p, vec, false, "alsep_vr_conv_h");
    if (rc != ALSEP_OK) return rc;
    ALSEP_LAUNCH_CHECK(ctx, "vr_conv_h_kernel");
    return ALSEP_OK;
}

// The decoder's convolution (KH x KW, stride 1, padding pad, no dilation) over cat(upsample x2 of x [B, Hu, Wu, Cu], skip [B, 2 Hu, Ws, Cs]
// cropped to columns [w_off, w_off + 2 Wu)) without the concatenated tensor; w [Cout][Kp] over k = (dy, dx, ci), ci over Cu then Cs.
extern "C" int alsep_vr_decoder_conv_h(alsep_ctx* ctx, const void* x, const void* skip, const void* w, const float* scale, const float* shift, void* y,
                                       int y_f16, int64_t B, int Hu, int Wu, int Cu, int Ws, int Cs, int w_off, int Cout, int Kp, int KH, int KW,
                                       int pad, int act, int y_ctotal, int y_coff) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !skip || !w || !scale || !shift || !y) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_decoder_conv_h: null argument");
    if (B <= 0 || Hu <= 0 || Wu <= 0 || Cu <= 0 || Cs <= 0 || Ws <= 0 || w_off < 0 || w_off + 2 * (int64_t)Wu > Ws || Cout <= 0 || KH <= 0 ||
        KW <= 0 || pad < 0 || act < 0 || act > 2 || y_coff < 0 || y_coff + Cout > y_ctotal || Hu >= (1 << 29) || Wu >= (1 << 29))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_decoder_conv_h: bad shape");
    const int H = 2 * Hu, W = 2 * Wu, Cin = Cu + Cs;
    const int Ho = H + 2 * pad - (KH - 1), Wo = W + 2 * pad - (KW - 1);
    if (Ho <= 0 || Wo <= 0) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_decoder_conv_h: empty output");
    const int64_t npix = B * Ho * Wo;
    if (B * (int64_t)Hu * Wu * Cu >= kVrhMax || B * (int64_t)H * Ws * Cs >= kVrhMax || npix >= kVrhMax - kDcBM || (int64_t)KH * KW * Cin >= kVrhMax)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_decoder_conv_h: an operand of 2^31 or more elements (32-bit offsets)");
    VrConvHArgs p{};
    p.x = (const _Float16*)x; p.skip = (const _Float16*)skip; p.w = (const _Float16*)w; p.scale = scale; p.shift = shift; p.y = y;
    p.npix = (int)npix; p.H = H; p.W = W; p.Cin = Cin; p.K = KH * KW * Cin; p.Kp = Kp; p.KW = KW; p.stride = 1; p.ph = pad; p.pw = pad;
    p.dh = 1; p.dw = 1; p.Ho = Ho; p.Wo = Wo; p.Cout = Cout; p.y_ct = y_ctotal; p.y_c0 = y_coff; p.act = act; p.y_f16 = y_f16 ? 1 : 0;
    p.Hu = Hu; p.Wu = Wu; p.Cu = Cu; p.Ws = Ws; p.Cs = Cs; p.w_off = w_off;
    p.sy = (float)(Hu - 1) / (float)(H - 1);
    p.sx = (float)(Wu - 1) / (float)(W - 1);
    const bool vec = Cu % 8 == 0 && Cs % 8 == 0 && !(((uintptr_t)x | (uintptr_t)skip) & 15);
    const int rc = vr_conv_h_launch(ctx, p, vec, true, "alsep_vr_decoder_conv_h");
    if (rc != ALSEP_OK) return rc;
    ALSEP_LAUNCH_CHECK(ctx, "vr_decoder_conv_h_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_vr_depthwise_h(alsep_ctx* ctx, const void* x, const void* w, void* y, int64_t B, int H, int W, int C, int KH, int KW, int pad,
                                    int dil) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !w || !y) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_depthwise_h: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || KH <= 0 || KW <= 0 || pad < 0 || dil <= 0 || 2 * pad != dil * (KH - 1) || 2 * pad != dil * (KW - 1) ||
        B * (int64_t)H * W * C >= kVrhMax)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_depthwise_h: bad shape (same-size output, fewer than 2^31 elements)");
    const int64_t n = B * H * W * C;
    hipLaunchKernelGGL(vr_depthwise_h_kernel, dim3((unsigned)ceil_div64(n, kHThreads)), dim3(kHThreads), 0, ctx->stream, (const _Float16*)x,
                       (const _Float16*)w, (_Float16*)y, (unsigned)n, H, W, C, KH, KW, pad, dil);
    ALSEP_LAUNCH_CHECK(ctx, "vr_depthwise_h_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_vr_resize_bilinear_h(alsep_ctx* ctx, const void* x, void* y, int64_t B, int H, int W, int C, int Ho, int Wo, int y_ctotal,
                                          int y_coff) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !y) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_resize_bilinear_h: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || y_coff < 0 || y_coff + C > y_ctotal || B * (int64_t)H * W * C >= kVrhMax ||
        B * (int64_t)Ho * Wo * y_ctotal >= kVrhMax)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_resize_bilinear_h: bad shape");
    const int64_t n = B * Ho * Wo * C;
    const float sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f, sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    hipLaunchKernelGGL(vr_resize_h_kernel, dim3((unsigned)ceil_div64(n, kHThreads)), dim3(kHThreads), 0, ctx->stream, (const _Float16*)x, (_Float16*)y,
                       (unsigned)n, H, W, C, Ho, Wo, y_ctotal, y_coff, sy, sx);
    ALSEP_LAUNCH_CHECK(ctx, "vr_resize_h_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_vr_copy_slice_h(alsep_ctx* ctx, const void* x, void* y, int64_t BH, int Wx, int C, int w_off, int Wy, int y_ctotal, int y_coff) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !y) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_copy_slice_h: null argument");
    if (BH <= 0 || Wx <= 0 || C <= 0 || Wy <= 0 || w_off < 0 || w_off + Wy > Wx || y_coff < 0 || y_coff + C > y_ctotal ||
        BH * (int64_t)Wx * C >= kVrhMax || BH * (int64_t)Wy * y_ctotal >= kVrhMax)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_copy_slice_h: bad shape");
    const int64_t n = BH * Wy * C;
    hipLaunchKernelGGL(vr_copy_slice_h_kernel, dim3((unsigned)ceil_div64(n, kHThreads)), dim3(kHThreads), 0, ctx->stream, (const _Float16*)x,
                       (_Float16*)y, (unsigned)n, Wx, C, w_off, Wy, y_ctotal, y_coff);
    ALSEP_LAUNCH_CHECK(ctx, "vr_copy_slice_h_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_vr_mean_hh(alsep_ctx* ctx, const void* x, void* y, int64_t B, int H, int W, int C) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !y) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_mean_hh: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || B * (int64_t)H * W * C >= kVrhMax) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_vr_mean_hh: bad shape");
    const int64_t n = B * W * C;
    hipLaunchKernelGGL(vr_mean_hh_kernel, dim3((unsigned)ceil_div64(n, kHThreads)), dim3(kHThreads), 0, ctx->stream, (const _Float16*)x, (_Float16*)y,
                       (unsigned)n, H, W, C);
    ALSEP_LAUNCH_CHECK(ctx, "vr_mean_hh_kernel");
    return ALSEP_OK;
}
