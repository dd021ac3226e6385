// Stem mixdown with loudness matching on the signed integer grid (part of elementwise.hip; HBM-bound).
// Reference semantics: wrappers/merge.py:15-45,146-151, which runs pydub -- AudioSegment.overlay, effects.normalize, .dBFS,
// .apply_gain -- i.e. the C module audioop underneath: add (saturating, one stem after the other), max, rms (truncated) and mul
// (floor of the clipped double product).  Three passes over an int32 mix [channels][n] (one container for both widths, 16 and 32 bits):
//   sum     acc = clip(acc + v_k) stem by stem, v_k the stem's float sample quantised on its own width grid and shifted up; max|acc|
//   power   y1 = floor(clip(acc f1)); max|y1| and the exact sum of y1^2, y1 not written
//   finish  y2 = floor(clip(y1 f2)) as integers and, optionally, as float32 y2 / full scale
// int64 / double in registers; every result is a pure function of the operands (no float accumulation anywhere).
#pragma once
#include "alsep_common.h"

namespace mixdown {
constexpr int kMixThreads = 256;
constexpr int kMixMaxBlocks = 1024;   // power pass: block partials, finished by one block

struct MixStems {
    const float* p[ALSEP_MIX_MAX_STEMS];
    int64_t n[ALSEP_MIX_MAX_STEMS], ld[ALSEP_MIX_MAX_STEMS];
    double scale[ALSEP_MIX_MAX_STEMS];     // 2^(b_s - 1)
    int up[ALSEP_MIX_MAX_STEMS];           // 2^(bits - b_s)
    int mono[ALSEP_MIX_MAX_STEMS], vec[ALSEP_MIX_MAX_STEMS];   // vec: every row of the stem starts on a 16-byte boundary
    int count;
};

// q_b(x) << (bits - b): round half even, NaN -> 0, +-inf -> the clip
__device__ __forceinline__ int64_t mix_quant(float x, double scale, int up) {
    double v = rint((double)x * scale);
    v = v != v ? 0.0 : fmin(fmax(v, -scale), scale - 1.0);
    return (int64_t)v * up;
}
// audioop's fbound(value * factor): clip, then floor.  A NaN product (0 * inf) is undefined there; 0 here.
__device__ __forceinline__ int64_t mix_gain(int64_t a, double f, double full) {
    double v = (double)a * f;
    v = v != v ? 0.0 : fmin(fmax(v, -full), full - 1.0);
    return (int64_t)floor(v);
}
__device__ __forceinline__ unsigned mix_abs(int64_t a) { return (unsigned)(a < 0 ? -a : a); }   // |-2^31| = 2^31 fits

// W consecutive samples of row c starting at i (W = 4: i is a multiple of 4, i + 4 <= n, acc rows 16-byte aligned)
template <int W>
__device__ __forceinline__ unsigned mix_sum_span(const int32_t* prev, int64_t ld_prev, int prev_vec, const MixStems& s, int c, int64_t i,
                                                 int64_t full, int32_t* acc, int64_t ld_acc) {
    int64_t a[W];
#pragma unroll
    for (int j = 0; j < W; ++j) a[j] = 0;
    if (prev) {
        const int32_t* row = prev + (int64_t)c * ld_prev + i;
        bool done = false;
        if constexpr (W == 4) {
            if (prev_vec) {
                const int4 v = *reinterpret_cast<const int4*>(row);
                a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
                done = true;
            }
        }
        if (!done) {
#pragma unroll
            for (int j = 0; j < W; ++j) a[j] = row[j];
        }
    }
    for (int k = 0; k < s.count; ++k) {
        const int64_t nk = s.n[k];
        if (i >= nk) continue;                                // beyond its end a stem adds zero: the mix stays as it is
        const float* row = s.p[k] + (s.mono[k] ? 0 : (int64_t)c * s.ld[k]) + i;
        float x[W];
        bool done = false;
        if constexpr (W == 4) {
            if (s.vec[k] && i + 4 <= nk) {
                const float4 v = *reinterpret_cast<const float4*>(row);
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
                done = true;
            }
        }
        if (!done) {
#pragma unroll
            for (int j = 0; j < W; ++j) x[j] = i + j < nk ? row[j] : 0.f;
        }
        const double scale = s.scale[k];
        const int up = s.up[k];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int64_t t = a[j] + mix_quant(x[j], scale, up);
            a[j] = t < -full ? -full : t > full - 1 ? full - 1 : t;   // audioop.add saturates after every add
        }
    }
    unsigned pk = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) { const unsigned m = mix_abs(a[j]); pk = m > pk ? m : pk; }
    int32_t* dst = acc + (int64_t)c * ld_acc + i;
    if constexpr (W == 4) {
        int4 v;
        v.x = (int)a[0]; v.y = (int)a[1]; v.z = (int)a[2]; v.w = (int)a[3];
        *reinterpret_cast<int4*>(dst) = v;
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) dst[j] = (int)a[j];
    }
    return pk;
}

// prev may be acc itself (every thread reads the samples it writes, nothing else)
__global__ void __launch_bounds__(kMixThreads)
mix_sum_kernel(const int32_t* prev, int64_t ld_prev, int prev_vec, MixStems s, int channels, int64_t n, int64_t full, int32_t* acc,
               int64_t ld_acc, int acc_vec, unsigned* peak) {
    unsigned* red = reinterpret_cast<unsigned*>(alsep_smem);
    const int64_t stride = (int64_t)gridDim.x * kMixThreads, first = (int64_t)blockIdx.x * kMixThreads + threadIdx.x;
    const int64_t nq = acc_vec ? n >> 2 : 0, tail = n - (nq << 2);
    unsigned pk = 0;
    for (int64_t idx = first; idx < channels * nq; idx += stride) {
        const int c = (int)(idx / nq);
        const unsigned m = mix_sum_span<4>(prev, ld_prev, prev_vec, s, c, (idx - c * nq) << 2, full, acc, ld_acc);
        pk = m > pk ? m : pk;
    }
    for (int64_t idx = first; idx < channels * tail; idx += stride) {
        const int c = (int)(idx / tail);
        const unsigned m = mix_sum_span<1>(prev, ld_prev, 0, s, c, (nq << 2) + (idx - c * tail), full, acc, ld_acc);
        pk = m > pk ? m : pk;
    }
    red[threadIdx.x] = pk;
    __syncthreads();
    for (int o = kMixThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { const unsigned m = red[threadIdx.x + o]; if (m > red[threadIdx.x]) red[threadIdx.x] = m; }
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(peak, red[0]);
}

struct MixPower { unsigned pk; uint64_t hi, lo; };
__device__ __forceinline__ void mix_power_one(MixPower& r, int32_t a, double f1, double full) {
    const int64_t y = mix_gain(a, f1, full);
    const unsigned m = mix_abs(y);
    r.pk = m > r.pk ? m : r.pk;
    const uint64_t sq = (uint64_t)(y * y);                    // <= 2^62
    r.hi += sq >> 32;
    r.lo += sq & 0xffffffffull;
}
// red: [3][kMixThreads] uint64 (peak, high limbs, low limbs); the block's totals land in dst[0..2]
__device__ __forceinline__ void mix_power_reduce(const MixPower& r, uint64_t* dst) {
    uint64_t* red = reinterpret_cast<uint64_t*>(alsep_smem);
    const int t = (int)threadIdx.x;
    red[t] = r.pk; red[kMixThreads + t] = r.hi; red[2 * kMixThreads + t] = r.lo;
    __syncthreads();
    for (int o = kMixThreads / 2; o > 0; o >>= 1) {
        if (t < o) {
            if (red[t + o] > red[t]) red[t] = red[t + o];
            red[kMixThreads + t] += red[kMixThreads + t + o];
            red[2 * kMixThreads + t] += red[2 * kMixThreads + t + o];
        }
        __syncthreads();
    }
    if (t < 3) dst[t] = red[t * kMixThreads];
}
__global__ void __launch_bounds__(kMixThreads)
mix_power_kernel(const int32_t* __restrict__ acc, int channels, int64_t n, int64_t ld, int vec, double f1, double full,
                 uint64_t* __restrict__ part) {
    const int64_t stride = (int64_t)gridDim.x * kMixThreads, first = (int64_t)blockIdx.x * kMixThreads + threadIdx.x;
    const int64_t nq = vec ? n >> 2 : 0, tail = n - (nq << 2);
    MixPower r = {0u, 0ull, 0ull};
    for (int64_t idx = first; idx < channels * nq; idx += stride) {
        const int64_t c = idx / nq;
        const int4 v = *reinterpret_cast<const int4*>(acc + c * ld + ((idx - c * nq) << 2));
        mix_power_one(r, v.x, f1, full); mix_power_one(r, v.y, f1, full); mix_power_one(r, v.z, f1, full); mix_power_one(r, v.w, f1, full);
    }
    for (int64_t idx = first; idx < channels * tail; idx += stride) {
        const int64_t c = idx / tail;
        mix_power_one(r, acc[c * ld + (nq << 2) + (idx - c * tail)], f1, full);
    }
    mix_power_reduce(r, part + 3 * (int64_t)blockIdx.x);
}
__global__ void __launch_bounds__(kMixThreads)
mix_power_final_kernel(const uint64_t* __restrict__ part, int nblocks, uint64_t* __restrict__ out) {
    MixPower r = {0u, 0ull, 0ull};
    for (int b = (int)threadIdx.x; b < nblocks; b += kMixThreads) {
        const unsigned m = (unsigned)part[3 * b];
        r.pk = m > r.pk ? m : r.pk;
        r.hi += part[3 * b + 1];
        r.lo += part[3 * b + 2];
    }
    mix_power_reduce(r, out);
}

__global__ void __launch_bounds__(kMixThreads)
mix_finish_kernel(const int32_t* acc, int channels, int64_t n, int64_t ld, int vec, double f1, double f2, double full, int32_t* out_i,
                  int64_t ld_i, float* __restrict__ out_f, int64_t ld_f) {
    const int64_t stride = (int64_t)gridDim.x * kMixThreads, first = (int64_t)blockIdx.x * kMixThreads + threadIdx.x;
    const int64_t nq = vec ? n >> 2 : 0, tail = n - (nq << 2);
    const double inv = 1.0 / full;
    for (int64_t idx = first; idx < channels * nq; idx += stride) {
        const int64_t c = idx / nq, i = (idx - c * nq) << 2;
        const int4 v = *reinterpret_cast<const int4*>(acc + c * ld + i);
        int4 y;
        y.x = (int)mix_gain(mix_gain(v.x, f1, full), f2, full); y.y = (int)mix_gain(mix_gain(v.y, f1, full), f2, full);
        y.z = (int)mix_gain(mix_gain(v.z, f1, full), f2, full); y.w = (int)mix_gain(mix_gain(v.w, f1, full), f2, full);
        *reinterpret_cast<int4*>(out_i + c * ld_i + i) = y;
        if (out_f) {
            float4 g;
            g.x = (float)((double)y.x * inv); g.y = (float)((double)y.y * inv); g.z = (float)((double)y.z * inv); g.w = (float)((double)y.w * inv);
            *reinterpret_cast<float4*>(out_f + c * ld_f + i) = g;
        }
    }
    for (int64_t idx = first; idx < channels * tail; idx += stride) {
        const int64_t c = idx / tail, i = (nq << 2) + (idx - c * tail);
        const int y = (int)mix_gain(mix_gain(acc[c * ld + i], f1, full), f2, full);
        out_i[c * ld_i + i] = y;
        if (out_f) out_f[c * ld_f + i] = (float)((double)y * inv);
    }
}

inline bool rows_aligned(const void* p, int64_t ld, int rows, size_t elem) {
    return ((uintptr_t)p & 15) == 0 && (rows == 1 || (ld * (int64_t)elem) % 16 == 0);
}
inline unsigned mix_grid(int64_t items, unsigned cap) {
    int64_t b = ceil_div64(items, (int64_t)kMixThreads * 4);
    if (b < 1) b = 1;
    return (unsigned)(b > cap ? cap : b);
}
inline bool mix_shape_ok(int channels, int64_t n, int64_t ld, int bits) {
    return channels >= 1 && n >= 1 && ld >= n && (bits == 16 || bits == 32) && (int64_t)channels * n <= ((int64_t)1 << 31);
}
}  // namespace mixdown

extern "C" int alsep_mix_sum(alsep_ctx* ctx, const int32_t* prev, int64_t ld_prev, const alsep_mix_stem* stems, int n_stems, int channels,
                             int64_t n, int bits, int32_t* acc, int64_t ld_acc, uint32_t* peak) {
    using namespace mixdown;
    ALSEP_ENTER(ctx);
    if (!ctx || !acc || !peak || !mix_shape_ok(channels, n, ld_acc, bits) || n_stems < 0 || n_stems > ALSEP_MIX_MAX_STEMS ||
        (n_stems > 0 && !stems) || (!prev && n_stems == 0) || (prev && ld_prev < n))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_mix_sum: bad argument");
    MixStems s;
    memset(&s, 0, sizeof(s));
    s.count = n_stems;
    for (int k = 0; k < n_stems; ++k) {
        const alsep_mix_stem& m = stems[k];
        if (!m.data || m.n < 1 || (m.channels != 1 && m.channels != channels) || (m.channels > 1 && m.ld < m.n) || m.bits < 2 || m.bits > bits)
            return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_mix_sum: stem %d: %d channel(s) into %d, %lld samples, width %d into %d", k, m.channels,
                              channels, (long long)m.n, m.bits, bits);
        s.p[k] = m.data; s.n[k] = m.n; s.ld[k] = m.ld;
        s.scale[k] = (double)((int64_t)1 << (m.bits - 1));
        s.up[k] = 1 << (bits - m.bits);
        s.mono[k] = m.channels == 1 && channels > 1;
        s.vec[k] = rows_aligned(m.data, m.ld, m.channels, sizeof(float));
    }
    ALSEP_HIP(ctx, hipMemsetAsync(peak, 0, sizeof(uint32_t), ctx->stream));
    const int acc_vec = rows_aligned(acc, ld_acc, channels, sizeof(int32_t));
    const int prev_vec = prev && rows_aligned(prev, ld_prev, channels, sizeof(int32_t));
    hipLaunchKernelGGL(mix_sum_kernel, dim3(mix_grid((int64_t)channels * n, 2048)), dim3(kMixThreads), kMixThreads * sizeof(unsigned), ctx->stream,
                       prev, ld_prev, prev_vec, s, channels, n, (int64_t)1 << (bits - 1), acc, ld_acc, acc_vec, (unsigned*)peak);
    ALSEP_LAUNCH_CHECK(ctx, "mix_sum_kernel");
    return ALSEP_OK;
}

extern "C" int64_t alsep_mix_power_workspace_bytes(int channels, int64_t n) {
    if (channels < 1 || n < 1) return -1;
    return 3 * (int64_t)sizeof(uint64_t) * mixdown::mix_grid((int64_t)channels * n, mixdown::kMixMaxBlocks);
}

extern "C" int alsep_mix_power(alsep_ctx* ctx, const int32_t* acc, int channels, int64_t n, int64_t ld, int bits, double f1, void* ws,
                               int64_t ws_bytes, uint64_t* out) {
    using namespace mixdown;
    ALSEP_ENTER(ctx);
    if (!ctx || !acc || !ws || !out || !mix_shape_ok(channels, n, ld, bits) || ((uintptr_t)ws & 7) ||
        ws_bytes < alsep_mix_power_workspace_bytes(channels, n))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_mix_power: bad argument");
    const unsigned nb = mix_grid((int64_t)channels * n, kMixMaxBlocks);
    const double full = (double)((int64_t)1 << (bits - 1));
    hipLaunchKernelGGL(mix_power_kernel, dim3(nb), dim3(kMixThreads), 3 * kMixThreads * sizeof(uint64_t), ctx->stream, acc, channels, n, ld,
                       (int)rows_aligned(acc, ld, channels, sizeof(int32_t)), f1, full, (uint64_t*)ws);
    hipLaunchKernelGGL(mix_power_final_kernel, dim3(1), dim3(kMixThreads), 3 * kMixThreads * sizeof(uint64_t), ctx->stream,
                       (const uint64_t*)ws, (int)nb, out);
    ALSEP_LAUNCH_CHECK(ctx, "mix_power kernels");
    return ALSEP_OK;
}

extern "C" int alsep_mix_finish(alsep_ctx* ctx, const int32_t* acc, int channels, int64_t n, int64_t ld, int bits, double f1, double f2,
                                int32_t* out_i, int64_t ld_i, float* out_f, int64_t ld_f) {
    using namespace mixdown;
    ALSEP_ENTER(ctx);
    if (!ctx || !acc || !out_i || !mix_shape_ok(channels, n, ld, bits) || ld_i < n || (out_f && ld_f < n))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_mix_finish: bad argument");
    const int vec = rows_aligned(acc, ld, channels, sizeof(int32_t)) && rows_aligned(out_i, ld_i, channels, sizeof(int32_t)) &&
                    (!out_f || rows_aligned(out_f, ld_f, channels, sizeof(float)));
    hipLaunchKernelGGL(mix_finish_kernel, dim3(mix_grid((int64_t)channels * n, 2048)), dim3(kMixThreads), 0, ctx->stream, acc, channels, n, ld,
                       vec, f1, f2, (double)((int64_t)1 << (bits - 1)), out_i, ld_i, out_f, ld_f);
    ALSEP_LAUNCH_CHECK(ctx, "mix_finish_kernel");
    return ALSEP_OK;
}

// ---- the sum pass for operands of differing sample rates -------------------------------------------------------------------------------
// audioop.ratecv(weightA = 1, weightB = 0, no state) is linear interpolation on 32-bit values, and every output has a closed form
// (include/alsep.h): output k reads x[j - 1], x[j] with j = ceil(k inr / outr) and the weight d = j outr - k inr.  A thread finds (j, d)
// of its first output once and walks the routine's own recurrence for the other three: d -= inr, then j advances until d >= 0 -- by
// inr / outr or one more, both known on the host.  The quotient is the routine's own double division: the numerator is an integer below
// 2^31 outr <= 2^51, exact in a double, and a correctly rounded quotient truncates like the exact one while outr < 2^21.
namespace mixdown {
struct MixRateOps {
    const void* p[ALSEP_MIX_MAX_STEMS];    // float32 stems, or the int32 mix (is_mix)
    int64_t n[ALSEP_MIX_MAX_STEMS], ld[ALSEP_MIX_MAX_STEMS];
    int64_t kout[ALSEP_MIX_MAX_STEMS];     // the operand's length after resampling
    double scale[ALSEP_MIX_MAX_STEMS];     // stems: 2^(b_s - 1)
    int up[ALSEP_MIX_MAX_STEMS];           // 2^(bits - b_s)
    int up32[ALSEP_MIX_MAX_STEMS];         // 2^(32 - b_s): ratecv works on samples shifted to 32 bits
    int sh[ALSEP_MIX_MAX_STEMS];           // 32 - b_s
    int down[ALSEP_MIX_MAX_STEMS];         // bits - b_s (the mix is brought to the grid it is resampled on)
    int inr[ALSEP_MIX_MAX_STEMS], outr[ALSEP_MIX_MAX_STEMS];   // the reduced pair; outr = 0: the operand is added as it is
    int q[ALSEP_MIX_MAX_STEMS], r[ALSEP_MIX_MAX_STEMS];        // inr / outr, inr % outr
    int mono[ALSEP_MIX_MAX_STEMS], vec[ALSEP_MIX_MAX_STEMS], is_mix[ALSEP_MIX_MAX_STEMS];
    int count;
};

// sample j of an operand's row, on its own grid, shifted to 32 bits: an integer of magnitude <= 2^31, held in a double (the routine
// multiplies it as one; no 64-bit integer conversions on the way)
__device__ __forceinline__ double mix_rate_load(const MixRateOps& s, int k, const void* row, int64_t j) {
    if (s.is_mix[k]) return (double)((reinterpret_cast<const int32_t*>(row)[j] >> s.down[k]) * s.up32[k]);   // fits 32 bits
    const double scale = s.scale[k];
    double v = rint((double)reinterpret_cast<const float*>(row)[j] * scale);
    v = v != v ? 0.0 : fmin(fmax(v, -scale), scale - 1.0);                   // mix_quant's rule
    return v * (double)s.up32[k];
}

// W consecutive outputs of row c starting at i (W = 4: i is a multiple of 4, i + 4 <= n_out, acc rows 16-byte aligned)
template <int W>
__device__ __forceinline__ unsigned mix_rate_span(const MixRateOps& s, int c, int64_t i, int64_t full, int32_t* acc, int64_t ld_acc) {
    int64_t a[W];
#pragma unroll
    for (int j = 0; j < W; ++j) a[j] = 0;
    for (int k = 0; k < s.count; ++k) {
        const int64_t kout = s.kout[k];
        if (i >= kout) continue;                              // beyond its (resampled) end an operand adds zero
        const char* row = reinterpret_cast<const char*>(s.p[k]) + (s.mono[k] ? 0 : (int64_t)c * s.ld[k]) * 4;   // float32 and int32 alike
        int64_t v[W];
        if (s.outr[k] == 0) {
            if (s.is_mix[k]) {
                const int32_t* x = reinterpret_cast<const int32_t*>(row) + i;
                bool done = false;
                if constexpr (W == 4) {
                    if (s.vec[k] && i + 4 <= kout) {
                        const int4 t = *reinterpret_cast<const int4*>(x);
                        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                        done = true;
                    }
                }
                if (!done) {
#pragma unroll
                    for (int j = 0; j < W; ++j) v[j] = i + j < kout ? x[j] : 0;
                }
            } else {
                const float* xr = reinterpret_cast<const float*>(row) + i;
                float x[W];
                bool done = false;
                if constexpr (W == 4) {
                    if (s.vec[k] && i + 4 <= kout) {
                        const float4 t = *reinterpret_cast<const float4*>(xr);
                        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
                        done = true;
                    }
                }
                if (!done) {
#pragma unroll
                    for (int j = 0; j < W; ++j) x[j] = i + j < kout ? xr[j] : 0.f;
                }
                const double scale = s.scale[k];
                const int up = s.up[k];
#pragma unroll
                for (int j = 0; j < W; ++j) v[j] = mix_quant(x[j], scale, up);
            }
        } else {
            // i < 2^31, the rates < 2^21: k inr and j outr are integers below 2^52, exact in doubles; d, q, r fit 32 bits
            const int outr = s.outr[k], q = s.q[k], r = s.r[k], sh = s.sh[k], down = s.down[k];
            const double den = (double)outr, t = (double)(int32_t)i * (double)s.inr[k];
            double jf = floor((t + (den - 1.0)) / den);                               // ceil(t / outr), at most one off: put right below
            int d = (int)(jf * den - t);
            if (d < 0) { jf += 1.0; d += outr; }
            if (d >= outr) { jf -= 1.0; d -= outr; }
            int64_t j = (int32_t)jf;
            double prev = j > 0 ? mix_rate_load(s, k, row, j - 1) : 0.0, cur = mix_rate_load(s, k, row, j);
#pragma unroll
            for (int o = 0; o < W; ++o) {
                v[o] = 0;
                if (i + o < kout) {                           // k < K keeps j <= n - 1
                    if (o > 0) {
                        int adv = q;
                        d -= r;
                        if (d < 0) { d += outr; ++adv; }
                        if (adv == 1) {
                            prev = cur;
                            cur = mix_rate_load(s, k, row, j + 1);
                        } else if (adv > 1) {
                            prev = mix_rate_load(s, k, row, j + adv - 1);
                            cur = mix_rate_load(s, k, row, j + adv);
                        }
                        j += adv;
                    }
                    const int y = (int)((prev * (double)d + cur * (double)(outr - d)) / den);
                    v[o] = (y >> sh) * (1 << down);           // on the grid of the mix again: fits 32 bits
                }
            }
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int64_t t = a[j] + v[j];
            a[j] = t < -full ? -full : t > full - 1 ? full - 1 : t;   // audioop.add saturates after every add
        }
    }
    unsigned pk = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) { const unsigned m = mix_abs(a[j]); pk = m > pk ? m : pk; }
    int32_t* dst = acc + (int64_t)c * ld_acc + i;
    if constexpr (W == 4) {
        int4 t;
        t.x = (int)a[0]; t.y = (int)a[1]; t.z = (int)a[2]; t.w = (int)a[3];
        *reinterpret_cast<int4*>(dst) = t;
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) dst[j] = (int)a[j];
    }
    return pk;
}

// an operand that is resampled must not overlap acc: a thread reads samples that its neighbours write
__global__ void __launch_bounds__(kMixThreads)
mix_sum_rate_kernel(MixRateOps s, int channels, int64_t n, int64_t full, int32_t* acc, int64_t ld_acc, int acc_vec, unsigned* peak) {
    unsigned* red = reinterpret_cast<unsigned*>(alsep_smem);
    const int64_t stride = (int64_t)gridDim.x * kMixThreads, first = (int64_t)blockIdx.x * kMixThreads + threadIdx.x;
    const int64_t nq = acc_vec ? n >> 2 : 0, tail = n - (nq << 2);
    unsigned pk = 0;
    for (int64_t idx = first; idx < channels * nq; idx += stride) {
        const int c = (int)(idx / nq);
        const unsigned m = mix_rate_span<4>(s, c, (idx - c * nq) << 2, full, acc, ld_acc);
        pk = m > pk ? m : pk;
    }
    for (int64_t idx = first; idx < channels * tail; idx += stride) {
        const int c = (int)(idx / tail);
        const unsigned m = mix_rate_span<1>(s, c, (nq << 2) + (idx - c * tail), full, acc, ld_acc);
        pk = m > pk ? m : pk;
    }
    red[threadIdx.x] = pk;
    __syncthreads();
    for (int o = kMixThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { const unsigned m = red[threadIdx.x + o]; if (m > red[threadIdx.x]) red[threadIdx.x] = m; }
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(peak, red[0]);
}

constexpr int64_t kRateMax = (int64_t)1 << 20;   // of a reduced rate
inline int64_t rate_gcd(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }
// -> false for a bad pair; inr = outr = 0 when nothing is to be resampled
inline bool rate_pair(int64_t in_rate, int64_t out_rate, int64_t& inr, int64_t& outr) {
    inr = outr = 0;
    if (in_rate == out_rate && in_rate >= 0) return true;
    if (in_rate < 1 || out_rate < 1) return false;
    const int64_t g = rate_gcd(in_rate, out_rate);
    inr = in_rate / g; outr = out_rate / g;
    return inr <= kRateMax && outr <= kRateMax;
}
inline int64_t ratecv_length(int64_t n, int64_t inr, int64_t outr) { return outr ? (n - 1) * outr / inr + 1 : n; }
}  // namespace mixdown

extern "C" int64_t alsep_mix_ratecv_length(int64_t n, int64_t in_rate, int64_t out_rate) {
    int64_t inr, outr;
    if (n < 1 || n > ((int64_t)1 << 31) || in_rate < 1 || out_rate < 1 || !mixdown::rate_pair(in_rate, out_rate, inr, outr)) return -1;
    return mixdown::ratecv_length(n, inr, outr);
}

extern "C" int alsep_mix_sum_rates(alsep_ctx* ctx, const alsep_mix_operand* operands, int n_operands, int channels, int64_t n_out, int bits,
                                   int32_t* acc, int64_t ld_acc, uint32_t* peak) {
    using namespace mixdown;
    ALSEP_ENTER(ctx);
    if (!ctx || !acc || !peak || !operands || n_operands < 1 || n_operands > ALSEP_MIX_MAX_STEMS || !mix_shape_ok(channels, n_out, ld_acc, bits))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_mix_sum_rates: bad argument");
    MixRateOps s;
    memset(&s, 0, sizeof(s));
    s.count = n_operands;
    const uintptr_t acc_lo = (uintptr_t)acc, acc_hi = acc_lo + (size_t)((channels - 1) * ld_acc + n_out) * sizeof(int32_t);
    for (int k = 0; k < n_operands; ++k) {
        const alsep_mix_operand& m = operands[k];
        const bool mix = m.is_mix != 0;
        if (!m.data || m.n < 1 || m.n > ((int64_t)1 << 31) || (mix ? k != 0 || m.channels != channels : m.channels != 1 && m.channels != channels) ||
            (m.channels > 1 && m.ld < m.n) || m.bits < 2 || m.bits > bits)
            return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_mix_sum_rates: operand %d: %d channel(s) into %d, %lld samples, width %d into %d%s", k,
                              m.channels, channels, (long long)m.n, m.bits, bits, mix && k ? ", the mix is operand 0" : "");
        int64_t inr, outr;
        if (!rate_pair(m.in_rate, m.out_rate, inr, outr))
            return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_mix_sum_rates: operand %d: rates %lld -> %lld (both >= 1, at most 2^20 once reduced)", k,
                              (long long)m.in_rate, (long long)m.out_rate);
        if (outr && m.bits != 16 && m.bits != 32)
            return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_mix_sum_rates: operand %d: width %d is resampled on no grid (16 or 32)", k, m.bits);
        const uintptr_t lo = (uintptr_t)m.data, hi = lo + (size_t)((m.channels - 1) * m.ld + m.n) * 4;
        if (outr && lo < acc_hi && acc_lo < hi)
            return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_mix_sum_rates: operand %d is resampled and overlaps acc", k);
        s.p[k] = m.data; s.n[k] = m.n; s.ld[k] = m.ld;
        s.kout[k] = ratecv_length(m.n, inr, outr);
        s.scale[k] = (double)((int64_t)1 << (m.bits - 1));
        s.up[k] = 1 << (bits - m.bits);
        s.sh[k] = 32 - m.bits;
        s.up32[k] = outr ? 1 << (32 - m.bits) : 0;
        s.down[k] = bits - m.bits;
        s.inr[k] = (int)inr; s.outr[k] = (int)outr;
        s.q[k] = outr ? (int)(inr / outr) : 0; s.r[k] = outr ? (int)(inr % outr) : 0;
        s.mono[k] = m.channels == 1 && channels > 1;
        s.vec[k] = rows_aligned(m.data, m.ld, m.channels, 4);
        s.is_mix[k] = mix;
    }
    if (s.kout[0] != n_out)
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_mix_sum_rates: operand 0 has %lld samples once resampled, n_out is %lld", (long long)s.kout[0],
                          (long long)n_out);
    ALSEP_HIP(ctx, hipMemsetAsync(peak, 0, sizeof(uint32_t), ctx->stream));
    const int acc_vec = rows_aligned(acc, ld_acc, channels, sizeof(int32_t));
    hipLaunchKernelGGL(mix_sum_rate_kernel, dim3(mix_grid((int64_t)channels * n_out, 2048)), dim3(kMixThreads), kMixThreads * sizeof(unsigned),
                       ctx->stream, s, channels, n_out, (int64_t)1 << (bits - 1), acc, ld_acc, acc_vec, (unsigned*)peak);
    ALSEP_LAUNCH_CHECK(ctx, "mix_sum_rate_kernel");
    return ALSEP_OK;
}
