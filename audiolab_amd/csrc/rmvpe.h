// RMVPE pitch extraction (the reference's modules/rvc/infer/lib/rmvpe.py) -- the operators the VR / Demucs building blocks do not have.
// Included at the end of nn.hip: float32 (the decode in float64), built without packed float32.  gfx950 only.
//
//   mel       : the log-mel front end.  One workgroup of 256 threads per PAIR of frames; each frame (1024 samples every 160, the track
//               reflected at both ends) times the periodic Hann window is ONE real transform: the even / odd samples are the real /
//               imaginary part of a 512-point radix-2 transform in LDS (9 stages, 2 butterflies per thread and stage for the pair), the
//               513 bins come apart by conjugate symmetry, their magnitudes stay in LDS, and thread t sums band t & 127 of frame t >> 7
//               over the band's non-zero stretch of the dense filterbank.  Neither the frames nor the spectrum reach memory.
//   pad_frames: mel2hidden's reflection of the frame axis to a multiple of 32 with the network's input BatchNorm (one channel) folded in.
//   avgpool2  : nn.AvgPool2d(2) over channels-last [B, H, W, C]; the same pass copies its input, the level's skip, into the skip half of the
//               decoder's concatenation.
//   tconv3x3s2: nn.ConvTranspose2d(3 x 3, stride 2, padding 1, output_padding 1) + folded BatchNorm + ReLU, written into a channel slice
//               of the concatenation with the skip.  A work item is (input pixel, 4 output channels): the 2 x 2 output pixels it owns
//               take 1, 2, 2 and 4 taps of the 3 x 3 kernel, 9 weight vectors per input channel for 36 multiply-adds.
//   gru       : the recurrence of one bidirectional GRU layer (gate order r, z, n as torch.nn.GRU, b_hn inside the reset product).  The
//               input projection pre = x W_ih^T + b_ih is one GEMM beforehand (both directions side by side, [T, N, 6H]).  ONE launch: a
//               workgroup of 1024 threads owns (direction, sequence) for all T steps.  A step's 3H x H product is spread over all 16
//               waves: thread (j, s) sums hidden unit j's three gates over slice s of the KS = 1024 / H slices of k, the partial sums
//               meet in LDS, and the first H threads apply the gates.  h lives in LDS, two barriers per step; workgroups never wait on
//               each other.  W_hh^T (768 KB a direction at H = 256) does not fit a CU: at H = 256 half of it stays resident (20 of a
//               thread's 64 values of k in registers, 12 in LDS) and the other half is re-read from L2 every step (nn_gru_res_kernel);
//               other sizes re-read all of it (nn_gru_kernel).
//   sigmoid   : the salience of the last Linear, in place.
//   decode    : to_local_average_cents + decode, one wave per frame: the argmax over 360 bins (the lowest index wins a tie), the
//               float64 salience-weighted mean of the cents of the 9 bins around it -- the sums in numpy's order of 9 terms, the weight
//               sum in float32 as numpy keeps it for a float32 salience -- and f0 = 10 2^(cents / 1200), 0 where the frame is unvoiced.

namespace {

constexpr int kRvThreads = 256;
constexpr int kRvN = 1024, kRvHalf = 512, kRvLog2Half = 9, kRvHop = 160, kRvBins = 513, kRvMels = 128, kRvPad = 512;
constexpr int kRvClasses = 360;
constexpr int kGruThreads = 1024;
constexpr int64_t kRvMaxFrames = (int64_t)1 << 20;

__device__ __forceinline__ int rv_bitrev9(int v) {
    int r = 0;
#pragma unroll
    for (int b = 0; b < kRvLog2Half; ++b) r |= ((v >> b) & 1) << (kRvLog2Half - 1 - b);
    return r;
}

// sample q of the track reflected without repeating its ends (numpy's "reflect", folded as often as it takes), any q
__device__ __forceinline__ int64_t rv_reflect(int64_t q, int64_t n) {
    if (n == 1) return 0;
    const int64_t P = 2 * (n - 1);
    int64_t m = q % P;
    if (m < 0) m += P;
    return m < n ? m : P - m;
}

// frames fa = 2 blockIdx.x and fa + 1.  win [1024]; tw [512] = exp(-2 pi i k / 1024) as (re, im); basis [128][513]; bands int32 [128][2] =
// first bin, bin count of every band's non-zero stretch (a band that points outside is left at zero).  lin (may be NULL) / logm: [T][128]
__global__ void __launch_bounds__(kRvThreads)
rv_mel_kernel(const float* __restrict__ audio, int64_t n, const float* __restrict__ win, const float2* __restrict__ tw,
              const float* __restrict__ basis, const int32_t* __restrict__ bands, int64_t T, float* __restrict__ lin, float* __restrict__ logm) {
    float2* z = reinterpret_cast<float2*>(alsep_smem);                        // [2][512]
    float* mag = reinterpret_cast<float*>(alsep_smem) + 2 * 2 * kRvHalf;       // [2][513]
    const int t = threadIdx.x;
    const int64_t fa = 2 * (int64_t)blockIdx.x;
    for (int i = t; i < 2 * kRvHalf; i += kRvThreads) {
        const int which = i >> kRvLog2Half, m = i & (kRvHalf - 1);
        const int64_t f = fa + which;
        float2 c = {0.f, 0.f};
        if (f < T) {
            const int64_t q = f * kRvHop - kRvPad + 2 * m;
            c.x = audio[rv_reflect(q, n)] * win[2 * m];
            c.y = audio[rv_reflect(q + 1, n)] * win[2 * m + 1];
        }
        z[which * kRvHalf + rv_bitrev9(m)] = c;
    }
    __syncthreads();
    for (int s = 0; s < kRvLog2Half; ++s) {
        const int half = 1 << s, pos = t & (half - 1);
        const int i0 = ((t >> s) << (s + 1)) + pos;
        const float2 w = tw[pos << (kRvLog2Half - s)];
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            float2* zz = z + which * kRvHalf;
            const float2 a = zz[i0], b = zz[i0 + half];
            const float br = b.x * w.x - b.y * w.y, bi = b.x * w.y + b.y * w.x;
            zz[i0] = make_float2(a.x + br, a.y + bi);
            zz[i0 + half] = make_float2(a.x - br, a.y - bi);
        }
        __syncthreads();
    }
    for (int i = t; i < 2 * kRvBins; i += kRvThreads) {
        const int which = i / kRvBins, k = i - which * kRvBins;
        const float2 zk = z[which * kRvHalf + (k & (kRvHalf - 1))], zn = z[which * kRvHalf + ((kRvHalf - k) & (kRvHalf - 1))];
        const float er = 0.5f * (zk.x + zn.x), ei = 0.5f * (zk.y - zn.y);
        const float orr = 0.5f * (zk.y + zn.y), oi = -0.5f * (zk.x - zn.x);
        const float2 w = k < kRvHalf ? tw[k] : make_float2(-1.f, 0.f);
        const float re = er + (w.x * orr - w.y * oi), im = ei + (w.x * oi + w.y * orr);
        mag[i] = sqrtf(re * re + im * im);
    }
    __syncthreads();
    const int band = t & (kRvMels - 1), which = t >> 7;
    const int64_t f = fa + which;
    const int first = bands[2 * band];
    int cnt = bands[2 * band + 1];
    if (first < 0 || cnt < 0 || first + cnt > kRvBins) cnt = 0;
    const float* p = mag + which * kRvBins + first;
    const float* b = basis + band * kRvBins + first;
    float acc = 0.f;
    for (int j = 0; j < cnt; ++j) acc = fmaf(b[j], p[j], acc);
    if (f < T) {
        if (lin) lin[f * kRvMels + band] = acc;
        logm[f * kRvMels + band] = logf(fmaxf(acc, 1e-5f));
    }
}

// y [Tp][C] = x [reflect(t)][C] * scale + shift; the caller guarantees Tp - T <= T - 1
__global__ void __launch_bounds__(kRvThreads)
rv_pad_frames_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int64_t T, int C, float scale, float shift) {
    for (int64_t i = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRvThreads) {
        const int64_t t = i / C;
        const int c = (int)(i - t * C);
        const int64_t s = t < T ? t : 2 * (T - 1) - t;
        y[i] = fmaf(x[s * C + c], scale, shift);
    }
}

// y [B, H/2, W/2, C] = the mean of the 2 x 2 pixels (H, W even); cat (may be NULL): the four pixels are also copied into the channel slice
// [cat_off, cat_off + C) of [B, H, W, cat_ct], the skip half of the decoder's concatenation
__global__ void __launch_bounds__(kRvThreads)
rv_avgpool2_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int Ho, int Wo, int C, float* __restrict__ cat, int cat_ct,
                   int cat_off) {
    for (int64_t i = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRvThreads) {
        const int c = (int)(i % C);
        const int64_t p = i / C;
        const int ox = (int)(p % Wo);
        const int64_t r = p / Wo;                                            // (b, oy): input rows 2 r and 2 r + 1
        const int64_t pa = (2 * r) * (2 * (int64_t)Wo) + 2 * ox, pb = pa + 2 * (int64_t)Wo;
        const float a0 = x[pa * C + c], a1 = x[(pa + 1) * C + c], b0 = x[pb * C + c], b1 = x[(pb + 1) * C + c];
        y[i] = ((a0 + a1) + (b0 + b1)) * 0.25f;
        if (cat) {
            cat[pa * cat_ct + cat_off + c] = a0;
            cat[(pa + 1) * cat_ct + cat_off + c] = a1;
            cat[pb * cat_ct + cat_off + c] = b0;
            cat[(pb + 1) * cat_ct + cat_off + c] = b1;
        }
    }
}

// x [B, H, W, Cin], w [3][3][Cin][Cout] (w[ky][kx][ci][co] = the module's weight[ci][co][ky][kx]); output pixel (oy, ox) takes input
// (iy, ix) through tap (ky, kx) where oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx.  y [B, 2H, 2W, y_ct] at channel y_off.  Cout % 4 == 0.
__global__ void __launch_bounds__(kRvThreads)
rv_tconv3x3s2_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale, const float* __restrict__ shift,
                     float* __restrict__ y, int64_t items, int H, int W, int Cin, int Cout, int act, int y_ct, int y_off) {
    const int cg = Cout / 4;
    for (int64_t it = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; it < items; it += (int64_t)gridDim.x * kRvThreads) {
        const int co = (int)(it % cg) * 4;
        const int64_t p = it / cg;
        const int ix = (int)(p % W);
        const int64_t q = p / W;
        const int iy = (int)(q % H);
        const int64_t b = q / H;
        const bool right = ix + 1 < W, down = iy + 1 < H;
        const float* x00 = x + ((b * H + iy) * W + ix) * Cin;
        const float* x01 = right ? x00 + Cin : x00;
        const float* x10 = down ? x00 + (int64_t)W * Cin : x00;
        const float* x11 = x10 + (right ? Cin : 0);
        float a00[4] = {0.f, 0.f, 0.f, 0.f}, a01[4] = {0.f, 0.f, 0.f, 0.f}, a10[4] = {0.f, 0.f, 0.f, 0.f}, a11[4] = {0.f, 0.f, 0.f, 0.f};
        const int64_t tap = (int64_t)Cin * Cout;
        for (int ci = 0; ci < Cin; ++ci) {
            const float v00 = x00[ci], v01 = right ? x01[ci] : 0.f, v10 = down ? x10[ci] : 0.f, v11 = (right && down) ? x11[ci] : 0.f;
            const float* wc = w + (int64_t)ci * Cout + co;
            f32x4 k[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) k[j] = *reinterpret_cast<const f32x4*>(wc + j * tap);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a00[e] = fmaf(k[4][e], v00, a00[e]);                                          // (even, even): tap (1, 1)
                a01[e] = fmaf(k[3][e], v01, fmaf(k[5][e], v00, a01[e]));                      // (even, odd): taps (1, 0), (1, 2)
                a10[e] = fmaf(k[1][e], v10, fmaf(k[7][e], v00, a10[e]));                      // (odd, even): taps (0, 1), (2, 1)
                a11[e] = fmaf(k[0][e], v11, fmaf(k[2][e], v10, fmaf(k[6][e], v01, fmaf(k[8][e], v00, a11[e]))));
            }
        }
        float* y00 = y + ((b * 2 * H + 2 * iy) * (2 * (int64_t)W) + 2 * ix) * y_ct + y_off + co;
        float* y10 = y00 + 2 * (int64_t)W * y_ct;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float sc = scale[co + e], sh = shift[co + e];
            float r00 = fmaf(a00[e], sc, sh), r01 = fmaf(a01[e], sc, sh), r10 = fmaf(a10[e], sc, sh), r11 = fmaf(a11[e], sc, sh);
            if (act == 1) { r00 = fmaxf(r00, 0.f); r01 = fmaxf(r01, 0.f); r10 = fmaxf(r10, 0.f); r11 = fmaxf(r11, 0.f); }
            y00[e] = r00;
            y00[y_ct + e] = r01;
            y10[e] = r10;
            y10[y_ct + e] = r11;
        }
    }
}

// pre [T, N, 6H] (r, z, n of the forward direction, then of the reverse one); wt [2][H(k)][3H]; bhh [2][3H]; out [T, N, 2H].
// LDS: h [H], then the partial sums [KS][3][H].  KS slices of H / KS values of k; threads beyond H KS only keep the barriers.
__global__ void __launch_bounds__(kGruThreads)
nn_gru_kernel(const float* __restrict__ pre, const float* __restrict__ wt, const float* __restrict__ bhh, float* __restrict__ out, int T, int N,
              int H, int KS) {
    float* hbuf = reinterpret_cast<float*>(alsep_smem);
    float* part = hbuf + H;
    const int tid = threadIdx.x;
    const int dir = blockIdx.x & 1, n = blockIdx.x >> 1;
    const bool live = tid < H * KS, head = tid < H;
    const int j = tid % H, s = tid / H;
    const int per = H / KS, k0 = s * per;
    const float* w = wt + (int64_t)dir * H * 3 * H + j;
    const int64_t ldp = 6 * (int64_t)H, ldo = 2 * (int64_t)H;
    float br = 0.f, bz = 0.f, bn = 0.f;
    if (head) {
        br = bhh[dir * 3 * H + j];
        bz = bhh[dir * 3 * H + H + j];
        bn = bhh[dir * 3 * H + 2 * H + j];
        hbuf[j] = 0.f;
    }
    __syncthreads();
    for (int step = 0; step < T; ++step) {
        const int t = dir ? T - 1 - step : step;
        float pr = 0.f, pz = 0.f, pn = 0.f;
        if (head) {                                                          // in flight while the product runs
            const float* p = pre + ((int64_t)t * N + n) * ldp + dir * 3 * H + j;
            pr = p[0];
            pz = p[H];
            pn = p[2 * H];
        }
        if (live) {
            float ar = 0.f, az = 0.f, an = 0.f;
            const float* wk = w + (int64_t)k0 * 3 * H;
            for (int k = 0; k < per; ++k) {
                const float hv = hbuf[k0 + k];
                ar = fmaf(wk[0], hv, ar);
                az = fmaf(wk[H], hv, az);
                an = fmaf(wk[2 * H], hv, an);
                wk += 3 * H;
            }
            part[(s * 3) * H + j] = ar;
            part[(s * 3 + 1) * H + j] = az;
            part[(s * 3 + 2) * H + j] = an;
        }
        __syncthreads();                                                     // the partial sums are complete, h_{t-1} has been read
        if (head) {
            float ar = br, az = bz, an = bn;
            for (int q = 0; q < KS; ++q) {
                ar += part[(q * 3) * H + j];
                az += part[(q * 3 + 1) * H + j];
                an += part[(q * 3 + 2) * H + j];
            }
            const float r = sigmoidf_(pr + ar), zg = sigmoidf_(pz + az);
            const float c = tanhf(fmaf(r, an, pn));
            const float h = fmaf(zg, hbuf[j] - c, c);                        // (1 - z) c + z h
            hbuf[j] = h;
            out[((int64_t)t * N + n) * ldo + dir * H + j] = h;
        }
        __syncthreads();                                                     // h_t complete
    }
}

// The same step for H PER == ... == 1024 / KS threads all live (H = 256: PER = 64), with half of W_hh^T resident on the CU: a thread's
// slice of k is the same at every step, so KR of its PER values of k keep their three weights in registers for the whole launch and KL
// more in LDS ([KL][3][1024] floats after the partial sums, every thread its own column: no bank conflicts); only the remaining
// PER - KR - KL are re-read from L2 per step, two chunks of 4 k (24 loads) in flight.  KR = 20, KL = 12 is what 128 VGPRs (1024 threads)
// and 160 KB of LDS hold without scratch.
template <int PER, int KR, int KL>
__global__ void __launch_bounds__(kGruThreads)
nn_gru_res_kernel(const float* __restrict__ pre, const float* __restrict__ wt, const float* __restrict__ bhh, float* __restrict__ out, int T, int N,
                  int H) {
    float* hbuf = reinterpret_cast<float*>(alsep_smem);
    float* part = hbuf + H;
    const int tid = threadIdx.x;
    const int dir = blockIdx.x & 1, n = blockIdx.x >> 1;
    const bool head = tid < H;
    const int j = tid % H, s = tid / H, KS = kGruThreads / H;
    const int k0 = s * PER;
    const float* w = wt + (int64_t)dir * H * 3 * H + (int64_t)k0 * 3 * H + j;
    const int64_t ldp = 6 * (int64_t)H, ldo = 2 * (int64_t)H;
    float wr[KR], wz[KR], wn[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        wr[k] = w[(int64_t)k * 3 * H];
        wz[k] = w[(int64_t)k * 3 * H + H];
        wn[k] = w[(int64_t)k * 3 * H + 2 * H];
    }
    float* wl = part + KS * 3 * H;
#pragma unroll
    for (int k = 0; k < KL; ++k)
#pragma unroll
        for (int g = 0; g < 3; ++g) wl[(k * 3 + g) * kGruThreads + tid] = w[(int64_t)(KR + k) * 3 * H + g * H];
    float br = 0.f, bz = 0.f, bn = 0.f;
    if (head) {
        br = bhh[dir * 3 * H + j];
        bz = bhh[dir * 3 * H + H + j];
        bn = bhh[dir * 3 * H + 2 * H + j];
        hbuf[j] = 0.f;
    }
    __syncthreads();
    for (int step = 0; step < T; ++step) {
        const int t = dir ? T - 1 - step : step;
        float pr = 0.f, pz = 0.f, pn = 0.f;
        if (head) {                                                          // in flight while the product runs
            const float* p = pre + ((int64_t)t * N + n) * ldp + dir * 3 * H + j;
            pr = p[0];
            pz = p[H];
            pn = p[2 * H];
        }
        float ar = 0.f, az = 0.f, an = 0.f;
        const f32x4* h4 = reinterpret_cast<const f32x4*>(hbuf + k0);
#pragma unroll 2
        for (int k = KR + KL; k < PER; k += 4) {
            const f32x4 hv = h4[k / 4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* wk = w + (int64_t)(k + e) * 3 * H;
                ar = fmaf(wk[0], hv[e], ar);
                az = fmaf(wk[H], hv[e], az);
                an = fmaf(wk[2 * H], hv[e], an);
            }
        }
#pragma unroll
        for (int k = 0; k < KL; k += 4) {
            const f32x4 hv = h4[(KR + k) / 4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* wk = wl + ((k + e) * 3) * kGruThreads + tid;
                ar = fmaf(wk[0], hv[e], ar);
                az = fmaf(wk[kGruThreads], hv[e], az);
                an = fmaf(wk[2 * kGruThreads], hv[e], an);
            }
        }
#pragma unroll
        for (int k = 0; k < KR; k += 4) {
            const f32x4 hv = h4[k / 4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ar = fmaf(wr[k + e], hv[e], ar);
                az = fmaf(wz[k + e], hv[e], az);
                an = fmaf(wn[k + e], hv[e], an);
            }
        }
        part[(s * 3) * H + j] = ar;
        part[(s * 3 + 1) * H + j] = az;
        part[(s * 3 + 2) * H + j] = an;
        __syncthreads();                                                     // the partial sums are complete, h_{t-1} has been read
        if (head) {
            float cr = br, cz = bz, cn = bn;
            for (int q = 0; q < KS; ++q) {
                cr += part[(q * 3) * H + j];
                cz += part[(q * 3 + 1) * H + j];
                cn += part[(q * 3 + 2) * H + j];
            }
            const float r = sigmoidf_(pr + cr), zg = sigmoidf_(pz + cz);
            const float c = tanhf(fmaf(r, cn, pn));
            const float h = fmaf(zg, hbuf[j] - c, c);
            hbuf[j] = h;
            out[((int64_t)t * N + n) * ldo + dir * H + j] = h;
        }
        __syncthreads();                                                     // h_t complete
    }
}
constexpr int kGruPer = 64, kGruKR = 20, kGruKL = 12;
static_assert(kGruKR % 4 == 0 && kGruKL % 4 == 0 && (kGruPer - kGruKR - kGruKL) % 4 == 0 && kGruKR + kGruKL <= kGruPer, "chunks of 4 values of k");

__global__ void __launch_bounds__(kRvThreads)
rv_sigmoid_kernel(float* __restrict__ x, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kRvThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRvThreads) x[i] = sigmoidf_(x[i]);
}

// salience [T][360] float32 -> f0 [T] float64; wave w of a workgroup takes frame 4 blockIdx.x + w
__global__ void __launch_bounds__(kRvThreads)
rv_decode_kernel(const float* __restrict__ sal, int64_t T, float thred, double* __restrict__ f0) {
    const int lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * (kRvThreads / 64) + (threadIdx.x >> 6);
    if (f >= T) return;                                                      // whole waves leave together
    const float* row = sal + f * kRvClasses;
    float best = row[lane];
    int at = lane;
    for (int k = lane + 64; k < kRvClasses; k += 64) {
        const float v = row[k];
        if (v > best) { best = v; at = k; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (ov > best || (ov == best && oa < at)) { best = ov; at = oa; }
    }
    if (lane != 0) return;
    float sv[9];
    double pv[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int k = at - 4 + i;
        const bool in = k >= 0 && k < kRvClasses;
        sv[i] = in ? row[k] : 0.f;
        pv[i] = (double)sv[i] * (in ? 20.0 * (double)k + 1997.3794084376191 : 0.0);
    }
    const double ps = (((pv[0] + pv[1]) + (pv[2] + pv[3])) + ((pv[4] + pv[5]) + (pv[6] + pv[7]))) + pv[8];
    const float ws = (((sv[0] + sv[1]) + (sv[2] + sv[3])) + ((sv[4] + sv[5]) + (sv[6] + sv[7]))) + sv[8];
    double cents = ps / (double)ws;
    if (best <= thred) cents = 0.0;
    const double hz = 10.0 * exp2(cents / 1200.0);
    f0[f] = hz == 10.0 ? 0.0 : hz;
}

}  // namespace

extern "C" int64_t alsep_rmvpe_frames(int64_t n) { return n < 1 || n / kRvHop + 1 > kRvMaxFrames ? -1 : n / kRvHop + 1; }

extern "C" int alsep_rmvpe_mel(alsep_ctx* ctx, const float* audio, int64_t n, const float* window, const float* twiddle, const float* basis,
                               const int32_t* bands, float* mel_lin, float* mel_log) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && audio && window && twiddle && basis && bands && mel_log, "alsep_rmvpe_mel");
    const int64_t T = alsep_rmvpe_frames(n);
    if (T < 0) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_rmvpe_mel: %lld samples (1 .. %lld frames)", (long long)n, (long long)kRvMaxFrames);
    const size_t lds = sizeof(float) * (2 * 2 * kRvHalf + 2 * kRvBins);
    hipLaunchKernelGGL(rv_mel_kernel, dim3((unsigned)((T + 1) / 2)), dim3(kRvThreads), lds, ctx->stream, audio, n, window, (const float2*)twiddle, basis,
                       bands, T, mel_lin, mel_log);
    ALSEP_LAUNCH_CHECK(ctx, "rv_mel_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_rmvpe_pad_frames(alsep_ctx* ctx, const float* x, float* y, int64_t T, int64_t Tp, int C, float scale, float shift) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && x && y && x != y && T > 0 && Tp >= T && Tp <= kRvMaxFrames && C > 0, "alsep_rmvpe_pad_frames");
    if (Tp - T > T - 1)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_rmvpe_pad_frames: %lld frames cannot be reflected by %lld", (long long)T, (long long)(Tp - T));
    const int64_t n = Tp * C;
    hipLaunchKernelGGL(rv_pad_frames_kernel, dim3(ew_grid(n)), dim3(kRvThreads), 0, ctx->stream, x, y, n, T, C, scale, shift);
    ALSEP_LAUNCH_CHECK(ctx, "rv_pad_frames_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_rmvpe_avgpool2(alsep_ctx* ctx, const float* x, float* y, int64_t B, int H, int W, int C, float* cat, int cat_ctotal,
                                    int cat_coff) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && x && y && x != y && B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 &&
               (!cat || (cat != x && cat != y && cat_coff >= 0 && cat_coff + C <= cat_ctotal)),
           "alsep_rmvpe_avgpool2");
    const int64_t n = B * (H / 2) * (W / 2) * C;
    hipLaunchKernelGGL(rv_avgpool2_kernel, dim3(ew_grid(n)), dim3(kRvThreads), 0, ctx->stream, x, y, n, H / 2, W / 2, C, cat, cat_ctotal, cat_coff);
    ALSEP_LAUNCH_CHECK(ctx, "rv_avgpool2_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_rmvpe_tconv3x3s2(alsep_ctx* ctx, const float* x, const float* w, const float* scale, const float* shift, float* y, int64_t B,
                                      int H, int W, int Cin, int Cout, int act, int y_ctotal, int y_coff) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && x && w && scale && shift && y && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Cout % 4 == 0 && (act == 0 || act == 1) &&
               y_coff >= 0 && y_coff + Cout <= y_ctotal && !((uintptr_t)w & 15),
           "alsep_rmvpe_tconv3x3s2");
    const int64_t items = B * H * W * (Cout / 4);
    ProfScope prof(ctx, ALSEP_PROF_NN_CONV);
    prof.work(2.0 * 9.0 * (double)B * H * W * Cin * Cout, 4.0 * ((double)B * H * W * Cin + 4.0 * B * H * W * Cout + 9.0 * Cin * Cout));
    hipLaunchKernelGGL(rv_tconv3x3s2_kernel, dim3(ew_grid(items)), dim3(kRvThreads), 0, ctx->stream, x, w, scale, shift, y, items, H, W, Cin, Cout,
                       act, y_ctotal, y_coff);
    ALSEP_LAUNCH_CHECK(ctx, "rv_tconv3x3s2_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_nn_gru(alsep_ctx* ctx, const float* pre, const float* whh_t, const float* bhh, float* h, int T, int N, int H) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && pre && whh_t && bhh && h && T > 0 && N > 0 && N <= (1 << 20) && H >= 16 && H <= 512 && H % 16 == 0 &&
               (int64_t)N * 6 * H * T < ((int64_t)1 << 40),
           "alsep_nn_gru");
    int KS = 1;                                                              // slices of k: H KS <= 1024 threads, at least 4 values a slice
    while (2 * KS * H <= kGruThreads && H % (2 * KS) == 0 && H / (2 * KS) >= 4) KS *= 2;
    const size_t lds = sizeof(float) * ((size_t)H + (size_t)KS * 3 * H);
    ProfScope prof(ctx, ALSEP_PROF_NN_LSTM);
    if (H * KS == kGruThreads && H / KS == kGruPer) {                        // H = 256, RMVPE's: half of W_hh^T stays on the CU
        const size_t lds_res = lds + sizeof(float) * (size_t)kGruKL * 3 * kGruThreads;
        ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)nn_gru_res_kernel<kGruPer, kGruKR, kGruKL>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds_res));
        hipLaunchKernelGGL((nn_gru_res_kernel<kGruPer, kGruKR, kGruKL>), dim3((unsigned)(2 * N)), dim3(kGruThreads), lds_res, ctx->stream, pre, whh_t,
                           bhh, h, T, N, H);
        prof.work(2.0 * T * N * 2 * (double)H * 3 * H, 4.0 * T * (double)N * 2 * 3 * H * (kGruPer - kGruKR - kGruKL) * KS);
        ALSEP_LAUNCH_CHECK(ctx, "nn_gru_res_kernel");
        return ALSEP_OK;
    }
    hipLaunchKernelGGL(nn_gru_kernel, dim3((unsigned)(2 * N)), dim3(kGruThreads), lds, ctx->stream, pre, whh_t, bhh, h, T, N, H, KS);
    prof.work(2.0 * T * N * 2 * (double)H * 3 * H, 4.0 * T * (double)N * 2 * 3 * H * H);
    ALSEP_LAUNCH_CHECK(ctx, "nn_gru_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_rmvpe_sigmoid(alsep_ctx* ctx, float* x, int64_t n) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && x && n > 0, "alsep_rmvpe_sigmoid");
    hipLaunchKernelGGL(rv_sigmoid_kernel, dim3(ew_grid(n)), dim3(kRvThreads), 0, ctx->stream, x, n);
    ALSEP_LAUNCH_CHECK(ctx, "rv_sigmoid_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_rmvpe_decode(alsep_ctx* ctx, const float* salience, int64_t T, float thred, double* f0) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && salience && f0 && T > 0 && T <= kRvMaxFrames, "alsep_rmvpe_decode");
    hipLaunchKernelGGL(rv_decode_kernel, dim3((unsigned)ceil_div64(T, kRvThreads / 64)), dim3(kRvThreads), 0, ctx->stream, salience, T, thred, f0);
    ALSEP_LAUNCH_CHECK(ctx, "rv_decode_kernel");
    return ALSEP_OK;
}
