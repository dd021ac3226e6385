// HDemucs (Hybrid Demucs v3, demucs 4 hdemucs.py) -- the operators of its deepest DConv branches, which HTDemucs does not have.
// Included at the end of nn.hip: float32 only, built without packed float32.
//
//   lstm            : the recurrence of one bidirectional LSTM layer (gate order i, f, g, o as torch.nn.LSTM).  The input projection
//                     pre = x W_ih^T + b_ih + b_hh is one float32 GEMM beforehand (both directions side by side, [T, N, 8H]); this
//                     kernel adds h_{t-1} W_hh^T, applies the gates and writes h_t into [T, N, 2H] (forward direction first).  ONE launch
//                     per layer: a workgroup owns (direction, tile of 16 sequences) for all T steps; h_{t-1} lives in LDS (double buffer,
//                     one barrier per step), c in registers; W_hh^T is re-read from L2 every step.  Workgroups never wait on each other.
//   localstate_softmax : demucs.demucs.LocalState between its two products: scores + the distance-decay bias of the query, the
//                     diagonal set to -100, softmax over the keys -- one pass, no bias tensor.
//   blstm_unfold / blstm_stitch : demucs.demucs.BLSTM's framing (frames of `width` every `stride` steps, zero tail) as a gather into the
//                     LSTM's time-major layout, and the re-stitch of the frames plus the skip connection as the scatter back.
//   group_norm      : nn.GroupNorm(G, C) over channels-last [B, R, C] with GELU / GLU fused and an optional row window of the output
//                     (HDecLayer normalises the whole transposed-convolution output, then crops it).

namespace {

constexpr int kLstmThreads = 256;
constexpr int kLstmTile = 16;                 // sequences per workgroup

__device__ __forceinline__ float lstm_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// NS: sequences of the tile one work item carries (16, 8 or 4); a work item is (hidden unit j, group of NS sequences), a thread loops over
// P <= MAXP items, so c stays in registers (MAXP * NS <= 32 values).
template <int NS, int MAXP>
__global__ void __launch_bounds__(kLstmThreads)
nn_lstm_kernel(const float* __restrict__ pre, const float* __restrict__ wt, float* __restrict__ out, int T, int N, int H, int ntile) {
    // placement only (never correctness): workgroups are dealt round-robin over the 8 XCDs; XCDs 0-3 take direction 0, 4-7 direction 1,
    // so one XCD's L2 holds one direction's W_hh
    const int xcd = blockIdx.x & 7, dir = xcd >> 2;
    const int tile = (int)(blockIdx.x >> 3) * 4 + (xcd & 3);
    if (tile >= ntile) return;                                   // whole workgroup: no barrier is skipped by part of it
    float* hbuf = reinterpret_cast<float*>(alsep_smem);          // [2][H][16]
    const int tid = threadIdx.x;
    const int groups = kLstmTile / NS;
    const int items = H * groups;
    const int P = (items + kLstmThreads - 1) / kLstmThreads;
    const int n0 = tile * kLstmTile;
    const int64_t ldp = 8 * (int64_t)H, ldo = 2 * (int64_t)H;
    const float* w = wt + (int64_t)dir * H * 4 * H;              // [H(k)][4H]
    for (int i = tid; i < H * kLstmTile; i += kLstmThreads) hbuf[i] = 0.f;
    float c[MAXP][NS];
#pragma unroll
    for (int p = 0; p < MAXP; ++p)
#pragma unroll
        for (int s = 0; s < NS; ++s) c[p][s] = 0.f;
    __syncthreads();
    for (int step = 0; step < T; ++step) {
        const int t = dir ? T - 1 - step : step;
        const float* hp = hbuf + (step & 1) * H * kLstmTile;
        float* hn = hbuf + ((step + 1) & 1) * H * kLstmTile;
#pragma unroll
        for (int p = 0; p < MAXP; ++p) {
            const int item = tid + p * kLstmThreads;
            if (p >= P || item >= items) break;
            const int j = item % H, sg = (item / H) * NS;
            float acc[4][NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int n = n0 + sg + s;
                const float* pr = pre + ((int64_t)t * N + (n < N ? n : 0)) * ldp + dir * 4 * H + j;
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g][s] = n < N ? pr[g * H] : 0.f;
            }
            const float* wj = w + j;
            for (int k = 0; k < H; ++k) {
                const float w0 = wj[(int64_t)k * 4 * H], w1 = wj[(int64_t)k * 4 * H + H], w2 = wj[(int64_t)k * 4 * H + 2 * H],
                            w3 = wj[(int64_t)k * 4 * H + 3 * H];
                const float* hk = hp + k * kLstmTile + sg;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const float hv = hk[s];
                    acc[0][s] = fmaf(w0, hv, acc[0][s]);
                    acc[1][s] = fmaf(w1, hv, acc[1][s]);
                    acc[2][s] = fmaf(w2, hv, acc[2][s]);
                    acc[3][s] = fmaf(w3, hv, acc[3][s]);
                }
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float ig = lstm_sigmoid(acc[0][s]), fg = lstm_sigmoid(acc[1][s]), gg = tanhf(acc[2][s]), og = lstm_sigmoid(acc[3][s]);
                c[p][s] = fg * c[p][s] + ig * gg;
                const float h = og * tanhf(c[p][s]);
                hn[j * kLstmTile + sg + s] = h;
                const int n = n0 + sg + s;
                if (n < N) out[((int64_t)t * N + n) * ldo + dir * H + j] = h;
            }
        }
        __syncthreads();                                         // h_t complete; h_{t-1}'s buffer is free for step + 1
    }
}

// scores [B*heads, T, ld] (rows: queries s, columns: keys t, already scaled by 1/sqrt(head dim)) in place:
//   v = scores - |t - s| * D(s), D(s) = sum_f (f+1) / sqrt(nd) * sigmoid(qd[b, s, h*nd + f]) / 2;  v(s, s) = -100;  softmax over t.
// qd: the query_decay projection, channels-last rows of qd_ld floats.  One wave per row.
__global__ void __launch_bounds__(kNnThreads)
nn_localstate_softmax_kernel(float* __restrict__ x, const float* __restrict__ qd, int64_t rows, int heads, int T, int ld, int nd, int64_t qd_ld) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kNnThreads / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;                                       // whole waves leave together
    const int s = (int)(r % T);
    const int64_t bh = r / T;
    const int h = (int)(bh % heads);
    const int64_t b = bh / heads;
    const float* q = qd + (b * T + s) * qd_ld + (int64_t)h * nd;
    const float rs = 1.f / sqrtf((float)nd);
    float D = 0.f;
    for (int f = 0; f < nd; ++f) D += (float)(f + 1) * rs * (lstm_sigmoid(q[f]) * 0.5f);
    float* row = x + r * ld;
    float mx = -3.4e38f;
    for (int t = lane; t < T; t += 64) {
        const float v = t == s ? -100.f : row[t] - (float)abs(t - s) * D;
        mx = fmaxf(mx, v);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    double sum = 0.0;
    for (int t = lane; t < T; t += 64) {
        const float v = t == s ? -100.f : row[t] - (float)abs(t - s) * D;
        sum += (double)expf(v - mx);
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float inv = (float)(1.0 / sum);
    for (int t = lane; t < T; t += 64) {
        const float v = t == s ? -100.f : row[t] - (float)abs(t - s) * D;
        row[t] = expf(v - mx) * inv;
    }
}

// x [B, T, C] -> frames [width, B*nf, C] (time-major): frames[w][b*nf + k] = x[b][k*stride + w], zero where k*stride + w >= T
__global__ void __launch_bounds__(kNnThreads)
nn_blstm_unfold_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int64_t B, int T, int C, int width, int stride, int nf) {
    for (int64_t i = (int64_t)blockIdx.x * kNnThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNnThreads) {
        const int c = (int)(i % C);
        const int64_t q = i / C;
        const int64_t nn = q % (B * nf);
        const int w = (int)(q / (B * nf));
        const int k = (int)(nn % nf);
        const int64_t b = nn / nf;
        const int t = k * stride + w;
        y[i] = t < T ? x[(b * T + t) * C + c] : 0.f;
    }
}

// frames [width, B*nf, C] -> y [B, T, C] = stitched frames + skip: position t comes from frame k = clamp((t - stride/2) / stride, 0, nf-1)
// (the first frame keeps [:-stride/2], the middle ones [stride/2 : -stride/2], the last [stride/2:]), step t - k*stride of it
__global__ void __launch_bounds__(kNnThreads)
nn_blstm_stitch_kernel(const float* __restrict__ f, const float* __restrict__ skip, float* __restrict__ y, int64_t n, int64_t B, int T, int C,
                       int stride, int nf) {
    const int lim = stride / 2;
    for (int64_t i = (int64_t)blockIdx.x * kNnThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNnThreads) {
        const int c = (int)(i % C);
        const int64_t q = i / C;
        const int t = (int)(q % T);
        const int64_t b = q / T;
        int k = t < lim ? 0 : (t - lim) / stride;
        if (k > nf - 1) k = nf - 1;
        const int w = t - k * stride;
        y[i] = f[((int64_t)w * B * nf + b * nf + k) * C + c] + skip[i];
    }
}

// GroupNorm statistics: one workgroup per (sample, group) over R rows x C/G channels, fp64 sums; st[2 (b G + g)] = mean, [+1] = rstd
__global__ void __launch_bounds__(kNnThreads)
nn_group_norm_stats_kernel(const float* __restrict__ x, float* __restrict__ st, int R, int C, int G, float eps) {
    double* red = reinterpret_cast<double*>(alsep_smem);
    const int bg = blockIdx.x, g = bg % G;
    const int64_t b = bg / G;
    const int Cg = C / G;
    const float* xb = x + b * R * (int64_t)C + (int64_t)g * Cg;
    const int64_t cnt = (int64_t)R * Cg;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < cnt; i += kNnThreads) s += (double)xb[(i / Cg) * C + i % Cg];
    const double mean = block_sum(s, red) / (double)cnt;
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < cnt; i += kNnThreads) {
        const double d = (double)xb[(i / Cg) * C + i % Cg] - mean;
        v += d * d;
    }
    const double var = block_sum(v, red) / (double)cnt;
    if (threadIdx.x == 0) {
        st[2 * bg] = (float)mean;
        st[2 * bg + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

// y [B, Ro, Co] = act(GroupNorm(x [B, R, C]))[:, r0 : r0 + Ro]; act 0, 3 (GELU) or 4 (GLU: Co = C / 2)
__global__ void __launch_bounds__(kNnThreads)
nn_group_norm_apply_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ beta,
                           const float* __restrict__ st, int64_t n, int R, int C, int G, int act, int r0, int Ro) {
    const int Co = act == 4 ? C / 2 : C, Cg = C / G;
    for (int64_t i = (int64_t)blockIdx.x * kNnThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNnThreads) {
        const int c = (int)(i % Co);
        const int64_t q = i / Co;
        const int r = (int)(q % Ro) + r0;
        const int64_t b = q / Ro;
        const float* xr = x + (b * R + r) * C;
        const float* sa = st + 2 * (b * G + c / Cg);
        float v = fmaf((xr[c] - sa[0]) * sa[1], gamma[c], beta[c]);
        if (act == 3) v = gelu_erf(v);
        else if (act == 4) {
            const float* sb = st + 2 * (b * G + (c + Co) / Cg);
            v *= sigmoidf_(fmaf((xr[c + Co] - sb[0]) * sb[1], gamma[c + Co], beta[c + Co]));
        }
        y[i] = v;
    }
}

}  // namespace

extern "C" int alsep_nn_lstm(alsep_ctx* ctx, const float* pre, const float* whh_t, float* h, int T, int N, int H) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && pre && whh_t && h && T > 0 && N > 0 && H >= 16 && H <= 512 && H % 16 == 0 && (int64_t)N * 8 * H * T < ((int64_t)1 << 40),
           "alsep_nn_lstm");
    const int ntile = (N + kLstmTile - 1) / kLstmTile;
    const dim3 grid((unsigned)(8 * ((ntile + 3) / 4)));
    const size_t lds = 2 * sizeof(float) * H * kLstmTile;
    // items per thread x sequences per item: the fewest serial FMA chains; ties go to the wider item (fewer W_hh loads per FMA)
    int best = 0, cost = 1 << 30;
    const int ns[3] = {16, 8, 4};
    for (int v = 0; v < 3; ++v) {
        const int c = (H * (kLstmTile / ns[v]) + kLstmThreads - 1) / kLstmThreads * ns[v];
        if (c < cost) { cost = c; best = v; }
    }
    ProfScope prof(ctx, ALSEP_PROF_NN_LSTM);
    if (best == 0)
        hipLaunchKernelGGL((nn_lstm_kernel<16, 2>), grid, dim3(kLstmThreads), lds, ctx->stream, pre, whh_t, h, T, N, H, ntile);
    else if (best == 1)
        hipLaunchKernelGGL((nn_lstm_kernel<8, 4>), grid, dim3(kLstmThreads), lds, ctx->stream, pre, whh_t, h, T, N, H, ntile);
    else
        hipLaunchKernelGGL((nn_lstm_kernel<4, 8>), grid, dim3(kLstmThreads), lds, ctx->stream, pre, whh_t, h, T, N, H, ntile);
    prof.work(2.0 * T * N * 2 * (double)H * 4 * H, 4.0 * T * (double)ntile * 2 * 4 * H * H);
    ALSEP_LAUNCH_CHECK(ctx, "nn_lstm_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_nn_localstate_softmax(alsep_ctx* ctx, float* scores, const float* qd, int64_t B, int heads, int T, int ld, int nd,
                                           int64_t qd_ld) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && scores && qd && B > 0 && heads > 0 && T > 0 && ld >= T && nd > 0 && qd_ld >= (int64_t)heads * nd, "alsep_nn_localstate_softmax");
    const int64_t rows = B * heads * T;
    ProfScope prof(ctx, ALSEP_PROF_NN_LOCALSTATE);
    hipLaunchKernelGGL(nn_localstate_softmax_kernel, dim3((unsigned)ceil_div64(rows, kNnThreads / 64)), dim3(kNnThreads), 0, ctx->stream, scores,
                       qd, rows, heads, T, ld, nd, qd_ld);
    prof.work(0.0, 8.0 * rows * T + 4.0 * rows * nd);           // the score matrix read and written once, the decay projection read
    ALSEP_LAUNCH_CHECK(ctx, "nn_localstate_softmax_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_nn_blstm_unfold(alsep_ctx* ctx, const float* x, float* frames, int64_t B, int T, int C, int width, int stride, int nf) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && x && frames && B > 0 && T > 0 && C > 0 && width > 0 && stride > 0 && nf > 0 && (int64_t)(nf - 1) * stride + width >= T,
           "alsep_nn_blstm_unfold");
    const int64_t n = (int64_t)width * B * nf * C;
    hipLaunchKernelGGL(nn_blstm_unfold_kernel, dim3(ew_grid(n)), dim3(kNnThreads), 0, ctx->stream, x, frames, n, B, T, C, width, stride, nf);
    ALSEP_LAUNCH_CHECK(ctx, "nn_blstm_unfold_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_nn_blstm_stitch(alsep_ctx* ctx, const float* frames, const float* skip, float* y, int64_t B, int T, int C, int width,
                                     int stride, int nf) {
    ALSEP_ENTER(ctx);
    // every position must fall inside its frame: nf == 1 (no framing, T <= width) or frames of width 2 * stride covering T
    NN_ARG(ctx && frames && skip && y && B > 0 && T > 0 && C > 0 && stride > 0 && nf > 0 &&
               ((nf == 1 && T <= width) || (nf >= 2 && width == 2 * stride && T <= nf * stride)),
           "alsep_nn_blstm_stitch");
    const int64_t n = B * T * (int64_t)C;
    hipLaunchKernelGGL(nn_blstm_stitch_kernel, dim3(ew_grid(n)), dim3(kNnThreads), 0, ctx->stream, frames, skip, y, n, B, T, C, nf == 1 ? T : stride,
                       nf);
    ALSEP_LAUNCH_CHECK(ctx, "nn_blstm_stitch_kernel");
    return ALSEP_OK;
}

extern "C" int alsep_nn_group_norm(alsep_ctx* ctx, const float* x, float* y, const float* gamma, const float* beta, int64_t B, int R, int C, int G,
                                   float eps, int act, int r0, int Ro, float* stats) {
    ALSEP_ENTER(ctx);
    NN_ARG(ctx && x && y && gamma && beta && stats && B > 0 && B * G <= 0x7fffffff && R > 0 && C > 0 && G > 0 && C % G == 0 &&
               (act == 0 || act == 3 || (act == 4 && C % 2 == 0)) && r0 >= 0 && Ro > 0 && r0 + Ro <= R,
           "alsep_nn_group_norm");
    hipLaunchKernelGGL(nn_group_norm_stats_kernel, dim3((unsigned)(B * G)), dim3(kNnThreads), 64, ctx->stream, x, stats, R, C, G, eps);
    const int64_t n = B * Ro * (int64_t)(act == 4 ? C / 2 : C);
    hipLaunchKernelGGL(nn_group_norm_apply_kernel, dim3(ew_grid(n)), dim3(kNnThreads), 0, ctx->stream, x, y, gamma, beta, stats, n, R, C, G, act,
                       r0, Ro);
    ALSEP_LAUNCH_CHECK(ctx, "nn_group_norm kernels");
    return ALSEP_OK;
}
