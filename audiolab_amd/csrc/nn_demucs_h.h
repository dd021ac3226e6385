// HTDemucs in half precision (HTDemucs(precision="f16")): the kernels the network needs beyond nn_half.hip's GEMM / attention.  Included
// by nn_half.hip (built without packed float32), inside its translation unit.
//
//   nn_dconv_h_kernel     implicit-GEMM convolution on v_mfma_f32_16x16x32_f16 for Demucs geometries: any KH x KW, stride, padding and
//                         dilation per axis, any Cin (the reduction runs over (tap, ci) flattened and zero-padded to 32), input half or
//                         float32 (rounded to half as it is staged), epilogue + bias (+ GELU), half or float32 out with a row stride
//   nn_norm_h_*           GroupNorm / LayerNorm over G groups of R rows x C channels, statistics in double in a fixed order that does not
//                         depend on G (a sample gives the same bits alone and in a batch), result half or float32, + GELU / GLU
//   nn_xattn_h_kernel     nn_attn_h_kernel for cross-attention: queries and the packed k | v projection in separate buffers, Lq != Lk
//                         (no rotary table, no gates)

namespace {

// ------------------------------------------------------------------------------------------------------------------------------------
// Convolution.  GEMM view: M = output pixels (B Ho Wo, row-major), N = Cout, K = KH KW Cin ordered (dy, dx, ci) and zero-padded to Kp, a
// multiple of 32 (weights [Cout][Kp] IEEE half, padded by the host).  Workgroup tile 128 pixels x 16 NJ channels, four waves stacked
// along M (32 pixels each: 2 x NJ MFMA blocks), K in steps of 32 = one MFMA.  A slice is staged through LDS as rows of 32 halves padded
// to 40 (80-byte rows: the ds_read_b128 of 16 consecutive rows hit 16 different 16-byte bank groups); the next slice's global loads are
// issued before this slice's MFMAs.  A staging granule is 8 consecutive k of one pixel: with Cin % 8 == 0 (VEC) they lie in one tap and
// are one 16-byte (half) or two 16-byte (float32) loads; otherwise every element finds its own tap.  Taps outside the image -- or at
// input rows >= Hv, the zero padding on the right of the time branch -- and k >= K contribute zeros.  Images are Hv rows of W pixels of
// x_ld elements apart.  D rows = channels, D columns = pixels (operands swapped as in nn_gemm_hh_kernel): a lane holds four consecutive
// channels of one pixel, stored as one 8- / 16-byte store where alignment allows.
// ------------------------------------------------------------------------------------------------------------------------------------
constexpr int kDcBM = 128, kDcBK = 32, kDcLd = 40;

struct DconvHArgs {
    const void* x; const _Float16* w; const float* bias; void* y;
    int npix, Hv, W, x_ld, Cin, K, Kp, KW, sh, sw, ph, pw, dh, dw, Ho, Wo, Cout, y_ld;
    int act, y_f16, y_vec;
};

template <int NJ>
constexpr size_t dconv_h_lds() { return (size_t)(kDcBM + 16 * NJ) * kDcLd * sizeof(_Float16); }

template <bool IN_F16>
__device__ __forceinline__ _Float16 dc_elem(const void* x, unsigned off) {
    if (IN_F16) return reinterpret_cast<const _Float16*>(x)[off];
    return (_Float16)reinterpret_cast<const float*>(x)[off];
}

template <int NJ, bool IN_F16, bool VEC>
__global__ void __launch_bounds__(kHThreads)
nn_dconv_h_kernel(DconvHArgs p) {
    constexpr int BN = 16 * NJ;
    constexpr int NBG = (BN * 4 + kHThreads - 1) / kHThreads;               // weight granules per thread
    _Float16* As = reinterpret_cast<_Float16*>(alsep_smem);                  // [128][40]
    _Float16* Bs = As + kDcBM * kDcLd;                                        // [BN][40]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int tiles_n = (p.Cout + BN - 1) / BN;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (wg / tiles_n) * kDcBM, n0 = (wg % tiles_n) * BN;
    // staging duty: A granule (row ar + 64 h, k group ag); the row's image, first input row / column of its taps
    const int ag = tid & 3, ar = tid >> 2;
    int pimg[2], py[2], px[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int pix = m0 + ar + 64 * h;
        const bool ok = pix < p.npix;
        const int pc = ok ? pix : 0;
        const int img = pc / (p.Ho * p.Wo), rem = pc - img * (p.Ho * p.Wo);
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        pimg[h] = img;
        py[h] = ok ? oy * p.sh - p.ph : -0x40000000;                          // a row beyond the last pixel: every tap "outside"
        px[h] = ox * p.sw - p.pw;
    }
    h16x8 zh;
#pragma unroll
    for (int e = 0; e < 8; ++e) zh[e] = (_Float16)0.f;
    h16x8 ra[2], rb[NBG];
    auto tap_off = [&](int h, int k, bool& in) -> unsigned {                 // element offset of k = (tap, ci) for staging row h
        const int tap = k / p.Cin, ci = k - tap * p.Cin;
        const int dy = tap / p.KW, dx = tap - dy * p.KW;
        const int iy = py[h] + dy * p.dh, ix = px[h] + dx * p.dw;
        in = k < p.K && iy >= 0 && iy < p.Hv && ix >= 0 && ix < p.W;
        return in ? (unsigned)(((pimg[h] * p.Hv + iy) * p.W + ix) * p.x_ld + ci) : 0u;
    };
    auto gload = [&](int k0) {
        const int k = k0 + 8 * ag;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (VEC) {
                bool in;
                const unsigned off = tap_off(h, k, in);
                if (IN_F16) {
                    const h16x8 v = *reinterpret_cast<const h16x8*>(reinterpret_cast<const _Float16*>(p.x) + off);
                    ra[h] = in ? v : zh;
                } else {
                    const float* xf = reinterpret_cast<const float*>(p.x) + off;
                    const f32x4 a = *reinterpret_cast<const f32x4*>(xf), b = *reinterpret_cast<const f32x4*>(xf + 4);
                    ra[h] = in ? to_h8(a, b) : zh;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    bool in;
                    const unsigned off = tap_off(h, k + e, in);
                    const _Float16 v = dc_elem<IN_F16>(p.x, off);
                    ra[h][e] = in ? v : (_Float16)0.f;
                }
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
        for (int h = 0; h < 2; ++h) *reinterpret_cast<h16x8*>(As + (ar + 64 * h) * kDcLd + 8 * ag) = ra[h];
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
                float t = acc[i][j][r];
                if (p.bias && col + r < p.Cout) t += p.bias[col + r];
                v[r] = p.act == 3 ? gelu_erf_h(t) : t;
            }
            const int64_t o = (int64_t)pix * p.y_ld + col;
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

// ------------------------------------------------------------------------------------------------------------------------------------
// GroupNorm / LayerNorm to half.  Statistics: 1-D grid of G nb workgroups (group-major: any G, e.g. the B x 2688 token LayerNorms of a
// large batch), nb = partial ranges per group chosen from the group size alone (NOT from G,
// unlike alsep_nn_norm's), each a sum and a sum of squares in double, added in index order by the final kernel: a group's statistics
// are the same bits whatever the batch.  Apply: y = act((x - mean) rstd gamma + beta), half or float32.
// ------------------------------------------------------------------------------------------------------------------------------------
constexpr int64_t kNhChunk = 16384;
constexpr int kNhMaxParts = 256;

__device__ __forceinline__ double nh_block_sum(double v, double* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    return s;
}

__global__ void __launch_bounds__(kHThreads)
nn_norm_h_stats_kernel(const float* __restrict__ x, int64_t per_group, int nb, double* __restrict__ part) {
    double* red = reinterpret_cast<double*>(alsep_smem);
    const int g = blockIdx.x / nb, blk = blockIdx.x - g * nb;
    const float* xg = x + (int64_t)g * per_group;
    const int64_t chunk = (per_group + nb - 1) / nb;
    const int64_t lo = (int64_t)blk * chunk, hi = lo + chunk < per_group ? lo + chunk : per_group;
    double s = 0.0, q = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kHThreads) {
        const double v = (double)xg[i];
        s += v;
        q += v * v;
    }
    s = nh_block_sum(s, red);
    q = nh_block_sum(q, red);
    if (threadIdx.x == 0) {
        part[((int64_t)g * nb + blk) * 2] = s;
        part[((int64_t)g * nb + blk) * 2 + 1] = q;
    }
}

__global__ void nn_norm_h_final_kernel(const double* __restrict__ part, int nb, int64_t per_group, int G, float eps, float* __restrict__ stats) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double s = 0.0, q = 0.0;
    for (int b = 0; b < nb; ++b) {
        s += part[((int64_t)g * nb + b) * 2];
        q += part[((int64_t)g * nb + b) * 2 + 1];
    }
    const double n = (double)per_group, mean = s / n;
    double var = q / n - mean * mean;
    if (var < 0.0) var = 0.0;
    stats[2 * g] = (float)mean;
    stats[2 * g + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

// act 0 none, 3 GELU (erf), 4 GLU (C -> C / 2 channels); n_out < 2^31
__global__ void __launch_bounds__(kHThreads)
nn_norm_h_apply_kernel(const float* __restrict__ x, void* __restrict__ y, int y_f16, const float* __restrict__ gamma, const float* __restrict__ beta,
                       const float* __restrict__ stats, unsigned n_out, unsigned rows_per_group, int C, int act) {
    const unsigned Co = (unsigned)(act == 4 ? C / 2 : C);
    for (unsigned i = blockIdx.x * kHThreads + threadIdx.x; i < n_out; i += gridDim.x * kHThreads) {
        const unsigned row = i / Co, c = i - row * Co, g = row / rows_per_group;
        const float mean = stats[2 * g], rstd = stats[2 * g + 1];
        const float* xr = x + (int64_t)row * C;
        float v = (xr[c] - mean) * rstd;
        if (gamma) v = fmaf(v, gamma[c], beta[c]);
        if (act == 3) {
            v = 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
        } else if (act == 4) {
            float u = (xr[c + Co] - mean) * rstd;
            if (gamma) u = fmaf(u, gamma[c + Co], beta[c + Co]);
            v *= 1.f / (1.f + expf(-u));
        }
        if (y_f16) reinterpret_cast<_Float16*>(y)[i] = (_Float16)v;
        else reinterpret_cast<float*>(y)[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Cross-attention: nn_attn_h_kernel (see there) with the queries q [seq][Lq] and the packed k | v rows kv [seq][Lk] in separate buffers.
// A copy rather than a template variant: the Roformer instantiations of nn_attn_h_kernel keep their code exactly as it was.
// ------------------------------------------------------------------------------------------------------------------------------------
template <int QB>
__global__ void __launch_bounds__(kHThreads)
nn_xattn_h_kernel(const _Float16* __restrict__ qp, const _Float16* __restrict__ kvp, _Float16* __restrict__ out, int Lq, int Lk, int heads,
                  int64_t q_seq_stride, int64_t q_row_stride, int64_t kv_seq_stride, int64_t kv_row_stride, int64_t o_seq_stride,
                  int64_t o_row_stride, float scale) {
    _Float16* Ks = reinterpret_cast<_Float16*>(alsep_smem);                  // [64 keys][64 d], swizzled 16-byte groups
    _Float16* Vt = Ks + kAtKc * kAtD;                                         // [64 d][72]: V transposed, rows padded by 8
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    // 1-D grid over (sequence, head, query block), query block fastest, dealt to the XCDs in contiguous runs: the workgroups that read the
    // same keys / values share one L2
    constexpr int QW = 64 * QB;                                               // queries per workgroup
    const int qblocks = (Lq + QW - 1) / QW;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int qb = wg % qblocks, head = (wg / qblocks) % heads, seq = wg / (qblocks * heads);
    const int inner = heads * kAtD;
    const _Float16* base = qp + seq * q_seq_stride + head * kAtD;
    const _Float16* kbase = kvp + seq * kv_seq_stride + head * kAtD;
    const _Float16* vbase = kbase + inner;
    // Q fragments: B operand of S^T = K Q^T: lane (col = query l15, quarter lq) holds Q[q][32 s + 8 lq .. + 7], rotated, times
    // scale log2(e)
    const float qs = scale * 1.44269504088896340736f;
    h16x8 qf[QB][2];
    int qrow[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        qrow[b] = qb * QW + (wave * QB + b) * 16 + l15;                       // this lane's query of block b (the MFMA column)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, c = a;
            if (qrow[b] < Lq) h8_to_f(*reinterpret_cast<const h16x8*>(base + (int64_t)qrow[b] * q_row_stride + 32 * s2 + 8 * lq), a, c);
            qf[b][s2] = to_h8(a * qs, c * qs);
        }
    }
    f32x4 o[QB][4];
    float mrun[QB], lsum[QB];                                                 // running max (shared by a query's 4 lanes), this lane's partial sum
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        mrun[b] = -3.0e38f;
        lsum[b] = 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) o[b][d] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // staging duty per chunk.  K: keys kkey and kkey + 32, 8 d values from 8 kgrp (8 lanes = one 128-byte row: coalesced).  V: the key
    // PAIR (2 vpair, 2 vpair + 1), 8 d values from 8 vgrp, one 32-lane half per d group: its eight 4-byte stores (one per d, two keys
    // each) then fall into 32 different banks
    const int kkey = tid >> 3, kgrp = tid & 7;
    const int vpair = tid & 31, vgrp = tid >> 5;
    // the next chunk's K / V rows are requested while this chunk is multiplied (one register set ahead: a chunk's loads used to be waited
    // for right where they were issued, every iteration, with only the other resident workgroups to cover the latency)
    h16x8 kv[2], vv[2];
    auto request = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int kr = k0 + kkey + 32 * h, krc = kr < Lk ? kr : Lk - 1;   // clamped: the loads are unconditional; masked below
            kv[h] = *reinterpret_cast<const h16x8*>(kbase + (int64_t)krc * kv_row_stride + 8 * kgrp);
            const int vr = k0 + 2 * vpair + h, vrc = vr < Lk ? vr : Lk - 1;
            vv[h] = *reinterpret_cast<const h16x8*>(vbase + (int64_t)vrc * kv_row_stride + 8 * vgrp);
        }
    };
    request(0);
    for (int k0 = 0; k0 < Lk; k0 += kAtKc) {
        __syncthreads();                                                      // every wave is done with the previous chunk
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = kkey + 32 * h;
            *reinterpret_cast<h16x8*>(Ks + row * kAtD + 8 * (kgrp ^ (row & 7))) = kv[h];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
            h16x2 pr;
            pr[0] = vv[0][e];
            pr[1] = vv[1][e];
            *reinterpret_cast<h16x2*>(Vt + (8 * vgrp + e) * kAtVld + 2 * vpair) = pr;
        }
        __syncthreads();
        request(k0 + kAtKc < Lk ? k0 + kAtKc : k0);                           // past the end: this chunk again (unconditional loads)
        // S^T blocks (log2 domain): keys 16 kb + (4 lq + r), query l15 of block b; the K fragments serve both query blocks
        f32x4 sc[QB][4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int krow = 16 * kb + l15;
            h16x8 kf[2];
#pragma unroll
            for (int st = 0; st < 2; ++st) kf[st] = *reinterpret_cast<const h16x8*>(Ks + krow * kAtD + 8 * ((4 * st + lq) ^ (krow & 7)));
#pragma unroll
            for (int b = 0; b < QB; ++b) {
                sc[b][kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[0], qf[b][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                sc[b][kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[1], qf[b][1], sc[b][kb], 0, 0, 0);
            }
        }
        if (k0 + kAtKc > Lk) {                                                 // the last chunk only: keys beyond the sequence
#pragma unroll
            for (int b = 0; b < QB; ++b)
#pragma unroll
                for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k0 + 16 * kb + 4 * lq + r >= Lk) sc[b][kb][r] = -3.0e38f;
        }
        h16x8 pf[QB][2];
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            float cmax = fmaxf(fmaxf(sc[b][0][0], sc[b][0][1]), fmaxf(sc[b][0][2], sc[b][0][3]));
#pragma unroll
            for (int kb = 1; kb < 4; ++kb) cmax = fmaxf(cmax, fmaxf(fmaxf(sc[b][kb][0], sc[b][kb][1]), fmaxf(sc[b][kb][2], sc[b][kb][3])));
            cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
            cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
            const float mnew = fmaxf(mrun[b], cmax);
            const float corr = __builtin_amdgcn_exp2f(mrun[b] - mnew);
            mrun[b] = mnew;
            float psum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(sc[b][kb][r] - mnew);   // a masked key: exp2(-3e38) = 0
                    psum += pv;
                    pf[b][kb >> 1][4 * (kb & 1) + r] = (_Float16)pv;
                }
            lsum[b] = lsum[b] * corr + psum;
#pragma unroll
            for (int d = 0; d < 4; ++d) o[b][d] *= corr;
        }
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                // A operand: V^T rows d = 16 d + l15, contraction index e of quarter lq = key 32 ks + 16 (e / 4) + 4 lq + e % 4
                const _Float16* vr = Vt + (16 * d + l15) * kAtVld + 32 * ks + 4 * lq;
                const h16x4 v0 = *reinterpret_cast<const h16x4*>(vr), v1 = *reinterpret_cast<const h16x4*>(vr + 16);
                h16x8 vf;
                vf[0] = v0[0]; vf[1] = v0[1]; vf[2] = v0[2]; vf[3] = v0[3];
                vf[4] = v1[0]; vf[5] = v1[1]; vf[6] = v1[2]; vf[7] = v1[3];
#pragma unroll
                for (int b = 0; b < QB; ++b) o[b][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[b][ks], o[b][d], 0, 0, 0);
            }
    }
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        float ls = lsum[b];
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        const int q = qrow[b];
        if (q < Lq) {
            const float inv = 1.f / ls;
            _Float16* dst = out + seq * o_seq_stride + (int64_t)q * o_row_stride + head * kAtD;
#pragma unroll
            for (int d = 0; d < 4; ++d) {                                     // O^T rows d = 16 d + 4 lq + r
                h16x4 hv;
                hv[0] = (_Float16)(o[b][d][0] * inv); hv[1] = (_Float16)(o[b][d][1] * inv);
                hv[2] = (_Float16)(o[b][d][2] * inv); hv[3] = (_Float16)(o[b][d][3] * inv);
                *reinterpret_cast<h16x4*>(dst + 16 * d + 4 * lq) = hv;
            }
        }
    }
}

}  // namespace

static int norm_h_parts(int64_t per_group) {
    int64_t nb = ceil_div64(per_group, kNhChunk);
    if (nb > kNhMaxParts) nb = kNhMaxParts;
    return (int)(nb < 1 ? 1 : nb);
}

extern "C" int64_t alsep_nn_norm_h_workspace_bytes(int64_t G, int64_t per_group) {
    if (G <= 0 || per_group <= 0) return -1;
    return (int64_t)sizeof(double) * 2 * G * norm_h_parts(per_group) + (int64_t)sizeof(float) * 2 * G + 64;
}

extern "C" int alsep_nn_norm_h(alsep_ctx* ctx, const float* x, void* y, int y_f16, const float* gamma, const float* beta, int64_t G, int64_t R,
                               int C, float eps, int act, void* workspace) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !y || !workspace || G < 1 || R < 1 || C < 1 || !(act == 0 || act == 3 || (act == 4 && C % 2 == 0)) ||
        ((gamma == nullptr) != (beta == nullptr)) || ((uintptr_t)workspace & 7))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_norm_h: bad argument");
    const int64_t per_group = R * C;
    const int64_t n_out = G * R * (act == 4 ? C / 2 : C);
    if (n_out >= ((int64_t)1 << 31)) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_norm_h: 2^31 or more outputs");
    const int nb = norm_h_parts(per_group);
    if (G * nb > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_norm_h: too many groups");
    double* part = reinterpret_cast<double*>(workspace);
    float* stats = reinterpret_cast<float*>(part + 2 * G * nb);
    ProfScope prof(ctx, ALSEP_PROF_NN_NORM_H);
    prof.work(0.0, 4.0 * (double)G * per_group * 2.0 + (y_f16 ? 2.0 : 4.0) * (double)n_out);   // x read twice, y written once
    hipLaunchKernelGGL(nn_norm_h_stats_kernel, dim3((unsigned)(G * nb)), dim3(kHThreads), 64, ctx->stream, x, per_group, nb, part);
    ALSEP_LAUNCH_CHECK(ctx, "nn_norm_h_stats_kernel");
    hipLaunchKernelGGL(nn_norm_h_final_kernel, dim3((unsigned)ceil_div64(G, 64)), dim3(64), 0, ctx->stream, (const double*)part, nb, per_group,
                       (int)G, eps, stats);
    ALSEP_LAUNCH_CHECK(ctx, "nn_norm_h_final_kernel");
    int64_t grid = ceil_div64(n_out, kHThreads);
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(nn_norm_h_apply_kernel, dim3((unsigned)grid), dim3(kHThreads), 0, ctx->stream, x, y, y_f16, gamma, beta, (const float*)stats,
                       (unsigned)n_out, (unsigned)R, C, act);
    ALSEP_LAUNCH_CHECK(ctx, "nn_norm_h_apply_kernel");
    return ALSEP_OK;
}

// y[pixel][co] (row stride y_ld) = act(sum_{tap, ci} x[pixel's tap][ci] w[co][tap ci] + bias[co]) -- see nn_dconv_h_kernel
extern "C" int alsep_nn_conv_h(alsep_ctx* ctx, const void* x, int x_f16, const void* w, const float* bias, void* y, int y_f16, int64_t y_ld,
                               int64_t B, int H, int Hv, int W, int x_ld, int Cin, int Cout, int Kp, int KH, int KW, int stride_h, int stride_w,
                               int pad_h, int pad_w, int dil_h, int dil_w, int act) {
    ALSEP_ENTER(ctx);
    if (!ctx || !x || !w || !y || B < 1 || H < 1 || Hv < 1 || Hv > H || W < 1 || Cin < 1 || x_ld < Cin || Cout < 1 || KH < 1 || KW < 1 ||
        stride_h < 1 || stride_w < 1 || pad_h < 0 || pad_w < 0 || dil_h < 1 || dil_w < 1 || y_ld < Cout || !(act == 0 || act == 3))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_conv_h: bad argument");
    const int K = KH * KW * Cin;
    if (Kp < K || Kp % kDcBK) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_conv_h: Kp must be >= KH KW Cin and a multiple of 32");
    const int Ho = (H + 2 * pad_h - dil_h * (KH - 1) - 1) / stride_h + 1, Wo = (W + 2 * pad_w - dil_w * (KW - 1) - 1) / stride_w + 1;
    if (Ho < 1 || Wo < 1) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_conv_h: empty output");
    const int64_t npix = B * Ho * Wo;
    if (B * (int64_t)Hv * W * x_ld >= ((int64_t)1 << 31) || (int64_t)Cout * Kp >= ((int64_t)1 << 31) || npix >= ((int64_t)1 << 31) - kDcBM)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_conv_h: an operand of 2^31 or more elements (32-bit offsets)");
    const bool vec = Cin % 8 == 0 && x_ld % 8 == 0 && !((uintptr_t)x & 15);
    if (((uintptr_t)w & 15)) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_conv_h: weights must be 16-byte aligned");
    const int y_vec = y_ld % 4 == 0 && !((uintptr_t)y & (y_f16 ? 7 : 15));
    const int NJ = Cout <= 16 ? 1 : Cout <= 32 ? 2 : Cout <= 64 ? 4 : 8;
    const int64_t n_wg = ceil_div64(npix, kDcBM) * ceil_div64(Cout, 16 * NJ);
    if (n_wg > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_conv_h: too many tiles");
    DconvHArgs p{x, (const _Float16*)w, bias, y, (int)npix, Hv, W, x_ld, Cin, K, Kp, KW, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, Ho, Wo,
                 Cout, (int)y_ld, act, y_f16 ? 1 : 0, y_vec};
    ProfScope prof(ctx, ALSEP_PROF_NN_DCONV_H);
    prof.work(2.0 * (double)npix * Cout * K, (x_f16 ? 2.0 : 4.0) * (double)B * Hv * W * Cin + 2.0 * Cout * K + (y_f16 ? 2.0 : 4.0) * (double)npix * Cout);
#define ALSEP_DC_GO(NJ_, F16_, VEC_)                                                                                                        \
    hipLaunchKernelGGL((nn_dconv_h_kernel<NJ_, F16_, VEC_>), dim3((unsigned)n_wg), dim3(kHThreads), dconv_h_lds<NJ_>(), ctx->stream, p)
#define ALSEP_DC_NJ(F16_, VEC_)                                                                                                             \
    do {                                                                                                                                    \
        if (NJ == 1) ALSEP_DC_GO(1, F16_, VEC_); else if (NJ == 2) ALSEP_DC_GO(2, F16_, VEC_);                                              \
        else if (NJ == 4) ALSEP_DC_GO(4, F16_, VEC_); else ALSEP_DC_GO(8, F16_, VEC_);                                                      \
    } while (0)
    if (x_f16) {
        if (vec) ALSEP_DC_NJ(true, true); else ALSEP_DC_NJ(true, false);
    } else {
        if (vec) ALSEP_DC_NJ(false, true); else ALSEP_DC_NJ(false, false);
    }
#undef ALSEP_DC_NJ
#undef ALSEP_DC_GO
    ALSEP_LAUNCH_CHECK(ctx, "nn_dconv_h_kernel");
    return ALSEP_OK;
}

// softmax(Q K^T scale) V per (sequence, head): q [n_seq][Lq] rows, kv [n_seq][Lk] rows of k (heads x 64) then v (heads x 64), IEEE half;
// out IEEE half.  Strides in elements.
extern "C" int alsep_nn_xattention_f16(alsep_ctx* ctx, const void* q, const void* kv, void* out, int n_seq, int Lq, int Lk, int heads,
                                       int dim_head, int64_t q_seq_stride, int64_t q_row_stride, int64_t kv_seq_stride, int64_t kv_row_stride,
                                       int64_t o_seq_stride, int64_t o_row_stride, float scale) {
    ALSEP_ENTER(ctx);
    if (!ctx || !q || !kv || !out || n_seq < 1 || Lq < 1 || Lk < 1 || heads < 1)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_xattention_f16: bad argument");
    if (dim_head != kAtD) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_xattention_f16: head dimension %d (64 is implemented)", dim_head);
    if (q_seq_stride % 8 || q_row_stride % 8 || kv_seq_stride % 8 || kv_row_stride % 8 || o_seq_stride % 4 || o_row_stride % 4 ||
        (((uintptr_t)q | (uintptr_t)kv) & 15) || ((uintptr_t)out & 7))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_xattention_f16: strides / bases must be multiples of 16 (q, kv) / 8 (out) bytes");
    const int QB = Lq > 64 ? 2 : 1;
    const int64_t n_wg = ceil_div64(Lq, 64 * QB) * heads * n_seq;
    if (n_wg > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_nn_xattention_f16: too many workgroups");
    ProfScope prof(ctx, ALSEP_PROF_NN_ATTN_H);
    prof.work(4.0 * n_seq * heads * (double)Lq * Lk * kAtD, 2.0 * n_seq * heads * (double)(2 * Lq + 2 * Lk) * kAtD);
    if (QB == 2)
        hipLaunchKernelGGL(nn_xattn_h_kernel<2>, dim3((unsigned)n_wg), dim3(kHThreads), kAtLds, ctx->stream, (const _Float16*)q, (const _Float16*)kv,
                           (_Float16*)out, Lq, Lk, heads, q_seq_stride, q_row_stride, kv_seq_stride, kv_row_stride, o_seq_stride, o_row_stride, scale);
    else
        hipLaunchKernelGGL(nn_xattn_h_kernel<1>, dim3((unsigned)n_wg), dim3(kHThreads), kAtLds, ctx->stream, (const _Float16*)q, (const _Float16*)kv,
                           (_Float16*)out, Lq, Lk, heads, q_seq_stride, q_row_stride, kv_seq_stride, kv_row_stride, o_seq_stride, o_row_stride, scale);
    ALSEP_LAUNCH_CHECK(ctx, "nn_xattn_h_kernel");
    return ALSEP_OK;
}
