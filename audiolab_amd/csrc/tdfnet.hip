// TFC-TDF U-Net ("ConvTDFNet", MDX-Net) forward on gfx950: MFMA implicit-GEMM convolutions,
// TDF linears as MFMA GEMMs, fused BatchNorm/ReLU/skip/residual epilogues.
//
// What it replaces: the ONNX network executed per chunk through MDXSeparator.model_run
// (reference handlers/patch_separate.py:52,58-62; loaded at modules/separator/stem_separator.py:394,512).
// Topology: see oracle/tdfnet_oracle.py (published KUIELab TFC-TDF v2; parity unpinned).
//
// Activation layout: channels-last [B, T, F, C] ("NHWC"; T = frames, F = bins).  A lane's
// 16-byte k-group is then 8 (bf16) / 4 (f32) consecutive input channels of one pixel/tap, so
// the 3x3 convolution is an implicit GEMM over K = (tap, ci) with no im2col buffer: the halo
// patch of a 256-pixel tile sits in LDS once and all 9 taps read it.
//   conv3x3 : D[co][pixel]  = sum_{tap,ci} W[co][tap,ci] * patch[pixel+tap][ci]
//   ds 2x2/2: D[co][pixel'] = sum_{dy,dx,ci} W * X[2t'+dy][2f'+dx][ci]           (K = 4c, two runs of 2c)
//   us 2x2^T: D[(dy,dx,co)][pixel'] = sum_ci W * X[pixel'][ci]; store scatters to (2t'+dy, 2f'+dx), * skip
//   TDF     : D[c][f'] = sum_f X[bt][f][c] * W[f'][f]        (activations are the A operand;
//             their k axis is strided in memory, so the stage transposes through LDS)
// Weights are always the operand with rows = output features; the epilogue therefore holds
// 4 consecutive output channels per lane and stores them as one 8/16-byte vector.
#include "mma.h"
#include <alsep_gfx950_asm.h>

#include <map>
#include <type_traits>

namespace {

constexpr int kThreads = 256;

// ------------------------------------------------------------------------------------------
// first 1x1 conv (4 -> g) + BN + ReLU, and final 1x1 conv (c -> 4) + bias: memory-bound VALU.
// ------------------------------------------------------------------------------------------
// 16-byte vectors of T
template <typename T> struct Vec16;
template <> struct Vec16<float> { static constexpr int N = 4; };
template <> struct Vec16<bf16_t> { static constexpr int N = 8; };
__device__ __forceinline__ void store_vec(float* p, const float* y) { *reinterpret_cast<float4*>(p) = make_float4(y[0], y[1], y[2], y[3]); }
__device__ __forceinline__ void store_vec(bf16_t* p, const float* y) {
    bf16x8 q;
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = (bf16_t)y[e];
    *reinterpret_cast<bf16x8*>(p) = q;
}
__device__ __forceinline__ void load_vec(const float* p, float* x) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
}
__device__ __forceinline__ void load_vec(const bf16_t* p, float* x) {
    const bf16x8 q = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (float)q[e];
}

// first 1x1 conv: a thread owns one 16-byte group of output channels for its whole life (its
// 4 x VN weights, scales and shifts stay in registers) and walks pixels with a grid stride;
// consecutive threads hold consecutive groups of one pixel, so a wave's stores are contiguous.
constexpr int kFirstThreads = 192;                          // divisible by g/VN = 6 (bf16) and 12 (f32) at g = 48
template <typename T>
__global__ void __launch_bounds__(kFirstThreads)
first_conv_kernel(const T* __restrict__ X, T* __restrict__ Y, const float* __restrict__ W,
                  const float* __restrict__ scale, const float* __restrict__ shift, int64_t npix, int g,
                  float in_scale) {
    constexpr int VN = Vec16<T>::N;
    const int q = g / VN;                                    // groups per pixel
    const int ppb = kFirstThreads / q;                       // pixels per block per pass (threads beyond ppb*q idle)
    const int tg = threadIdx.x % q, tp = threadIdx.x / q;
    if (tp >= ppb) return;
    const int co = tg * VN;
    float4 w[VN];
    float sc[VN], sh[VN];
#pragma unroll
    for (int r = 0; r < VN; ++r) {
        w[r] = *reinterpret_cast<const float4*>(W + (co + r) * 4);
        sc[r] = scale[co + r] * in_scale;                    // scale * (in_scale * a) + shift
        sh[r] = shift[co + r];
    }
    for (int64_t p = (int64_t)blockIdx.x * ppb + tp; p < npix; p += (int64_t)gridDim.x * ppb) {
        float x[4];
        load4(X + p * 4, x);
        float y[VN];
#pragma unroll
        for (int r = 0; r < VN; ++r) {
            float a = w[r].x * x[0];
            a = fmaf(w[r].y, x[1], a);
            a = fmaf(w[r].z, x[2], a);
            a = fmaf(w[r].w, x[3], a);
            y[r] = fmaxf(fmaf(a, sc[r], sh[r]), 0.f);
        }
        store_vec(Y + p * g + co, y);
    }
}

// final 1x1 conv (c -> 4) + bias: a wave copies 64 pixels x c channels (contiguous) into LDS with
// coalesced 16-byte loads, then every lane reduces its own pixel from LDS and writes 4 values.
template <typename T>
__global__ void __launch_bounds__(kThreads)
final_conv_kernel(const T* __restrict__ X, T* __restrict__ Y, const float* __restrict__ W,
                  const float* __restrict__ bias, int64_t npix, int c, float alpha, float beta) {
    constexpr int VN = Vec16<T>::N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gpp = c / VN;                                   // 16-byte groups per pixel
    T* stg = reinterpret_cast<T*>(alsep_smem) + (size_t)wave * 64 * c;
    const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * 64;
    for (int i = lane; i < 64 * gpp; i += 64) {
        const int64_t pix = p0 + i / gpp;
        vec16 v = zero16();
        if (pix < npix) v = *reinterpret_cast<const vec16*>(X + p0 * c + (int64_t)i * VN);
        *reinterpret_cast<vec16*>(stg + (size_t)i * VN) = v;
    }
    __builtin_amdgcn_wave_barrier();                          // wave-private staging
    const int64_t p = p0 + lane;
    float y[4] = {bias[0], bias[1], bias[2], bias[3]};
    for (int ci = 0; ci < c; ci += VN) {
        float x[VN];
        load_vec(stg + (size_t)lane * c + ci, x);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int e = 0; e < VN; ++e) y[r] = fmaf(W[r * c + ci + e], x[e], y[r]);
    }
    if (p >= npix) return;
    if (beta != 0.f) {                                      // Y = alpha * net + beta * Y (denoise average)
        float o[4];
        load4(Y + p * 4, o);
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = fmaf(alpha, y[r], beta * o[r]);
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] *= alpha;
    }
    store4(Y + p * 4, y);
}

// ------------------------------------------------------------------------------------------
// 3x3 convolution (pad 1) + scale/shift + ReLU.
// Tile: 256 output pixels (TH x TW) x BN output channels per workgroup; 4 waves, wave w owns
// pixels [64w, 64w+64) of the tile.  K loop over chunks of KC input channels: the halo patch
// chunk [(TH+2)(TW+2)][KC] and the packed weight block [BN][9*KC] are staged in LDS.
// ------------------------------------------------------------------------------------------
template <typename T, int KC, int BN, int TW>
struct ConvCfg {
    static constexpr int G = Frag<T>::G;
    static constexpr int TH = 256 / TW;
    static constexpr int PW = TW + 2, PH = TH + 2;
    static constexpr int CG = KC / G;                  // k-groups per pixel per chunk
    static constexpr int KCP = KC + G;                 // padded pixel stride (odd in 16-B units)
    static constexpr int NG = 9 * CG;                  // k-groups per chunk
    static constexpr int NS = (NG + 3) / 4;            // k-steps per chunk
    static constexpr int KP = NS * 4 * G + G;          // padded weight row stride
    static constexpr int MR = BN / 16;
    static constexpr size_t lds_bytes = sizeof(T) * ((size_t)PH * PW * KCP + (size_t)BN * KP);
    static_assert(KC % G == 0 && BN % 16 == 0 && 256 % TW == 0 && TW % 16 == 0, "bad conv tile");
};

template <typename T, int KC, int BN, int TW>
__global__ void __launch_bounds__(kThreads)
conv3x3_kernel(const T* __restrict__ X, T* __restrict__ Y, const T* __restrict__ Wp,
               const float* __restrict__ scale, const float* __restrict__ shift, int Th, int Fw, int Cin,
               int Cout, int tiles_t, int tiles_f, int ntiles) {
    typedef ConvCfg<T, KC, BN, TW> Cf;
    constexpr int G = Cf::G;
    T* patch = reinterpret_cast<T*>(alsep_smem);
    T* wts = patch + (size_t)Cf::PH * Cf::PW * Cf::KCP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;

    int tile = xcd_remap(blockIdx.x, ntiles);
    const int tf = tile % tiles_f;  tile /= tiles_f;
    const int tt = tile % tiles_t;
    const int64_t b = tile / tiles_t;
    const int t0 = tt * Cf::TH, f0 = tf * TW;
    const int ny = blockIdx.y;
    const int nq = Cin / KC;

    int pbase[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int pm = wave * 64 + ni * 16 + l15;
        pbase[ni] = ((pm / TW) * Cf::PW + (pm % TW)) * Cf::KCP;
    }
    f32x4 acc[Cf::MR][4];
#pragma unroll
    for (int mi = 0; mi < Cf::MR; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    const T* xb = X + b * (int64_t)Th * Fw * Cin;
    for (int q = 0; q < nq; ++q) {
        __syncthreads();                                     // previous chunk's reads are done
        for (int it = tid; it < Cf::PH * Cf::PW * Cf::CG; it += kThreads) {
            const int pix = it / Cf::CG, g = it % Cf::CG;
            const int t = t0 - 1 + pix / Cf::PW, f = f0 - 1 + pix % Cf::PW;
            vec16 v = zero16();
            if (t >= 0 && t < Th && f >= 0 && f < Fw)
                v = *reinterpret_cast<const vec16*>(xb + ((int64_t)t * Fw + f) * Cin + q * KC + g * G);
            *reinterpret_cast<vec16*>(patch + pix * Cf::KCP + g * G) = v;
        }
        const T* wsrc = Wp + ((int64_t)ny * nq + q) * BN * Cf::KP;
        for (int it = tid; it < BN * Cf::KP / G; it += kThreads)
            *reinterpret_cast<vec16*>(wts + it * G) = *reinterpret_cast<const vec16*>(wsrc + it * G);
        __syncthreads();
#pragma unroll 2
        for (int s = 0; s < Cf::NS; ++s) {
            const int grp = 4 * s + lq;
            const int gc = grp < Cf::NG ? grp : Cf::NG - 1;   // padded groups: weights are zero there
            const int tap = gc / Cf::CG, cg = gc % Cf::CG;
            const int koff = ((tap / 3) * Cf::PW + (tap % 3)) * Cf::KCP + cg * G;
            typename Frag<T>::type xf[4], wf[Cf::MR];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) xf[ni] = lds_frag<T>(patch + pbase[ni] + koff);
#pragma unroll
            for (int mi = 0; mi < Cf::MR; ++mi) wf[mi] = lds_frag<T>(wts + (mi * 16 + l15) * Cf::KP + grp * G);
#pragma unroll
            for (int mi = 0; mi < Cf::MR; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) mma_step(acc[mi][ni], wf[mi], xf[ni]);
        }
    }
    // epilogue: lane holds channels co..co+3 (rows 4*lq+r) of pixel column l15
    T* yb = Y + b * (int64_t)Th * Fw * Cout;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int pm = wave * 64 + ni * 16 + l15;
        const int t = t0 + pm / TW, f = f0 + pm % TW;
        if (t < Th && f < Fw) {
#pragma unroll
            for (int mi = 0; mi < Cf::MR; ++mi) {
                const int co = ny * BN + mi * 16 + 4 * lq;
                float y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[mi][ni][r], scale[co + r], shift[co + r]), 0.f);
                store4(yb + ((int64_t)t * Fw + f) * Cout + co, y);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// bf16 3x3 convolution, main path (Cin, Cout multiples of 48): same tiling as conv3x3_kernel but
//  * the halo patch chunk and the weight block are written to LDS by LDS-DMA
//    (global_load_lds_dwordx4: no VGPR staging, all loads of a stage in flight at once); lanes
//    that fall outside the image read a 16-byte zero page instead, so padding costs no branch
//    in the math loop;
//  * LDS images are conflict-free for ds_read_b128 without padding: pixel stride 96 B for the
//    patch (6 slots: the 16-lane read groups land on 16 distinct slots), weight rows (896 B)
//    XOR-swizzled by (row>>1)&7 on the 16-byte group index (pre-swizzled in the packed image,
//    LDS-DMA writes linearly; cdna_hip_programming.md rule 21);
//  * 79.1 KiB of LDS per workgroup -> two workgroups per CU, so one stages while the other
//    runs its MFMAs.
// ------------------------------------------------------------------------------------------
template <int TW>
struct ConvB16 {
    static constexpr int KC = 48, BN = 48, G = 8, CG = 6, NG = 54, NS = 14, WG = 56;   // WG: groups per weight row
    static constexpr int TH = 256 / TW, PW = TW + 2, PH = TH + 2;
    static constexpr int PGROUPS = PH * PW * CG;
    static constexpr int WGROUPS = BN * WG;
    static constexpr size_t lds_bytes = 16 * (size_t)(PGROUPS + WGROUPS);
};

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    // per-lane 16-byte source, wave-uniform LDS base: lane l lands at base + 16*l
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <int TW>
__global__ void __launch_bounds__(kThreads, 2)
conv3x3_bf16_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wp,
                    const float* __restrict__ scale, const float* __restrict__ shift,
                    const bf16_t* __restrict__ zero_page, int Th, int Fw, int Cin, int Cout, int tiles_t,
                    int tiles_f, int ntiles, int ablate, int stagger, int ny_fastest) {
    typedef ConvB16<TW> Cf;
    // `ablate` (bit 0 no LDS-DMA, bit 1 no MFMA loop, bit 2 no stores) and `stagger` are the arguments of two finished timing experiments
    // (profiles/r01_conv_ablation_*, r01_conv_stagger_experiment.txt); the library always passes 0.  They stay because the kernel
    // compiled without them measured 1.2 % slower per launch at levels 3+ (profiles/conv_cleanup_ab.txt).  The cause was not looked for
    // (only scalar control flow and moves differed: probably code layout); they can go once that is re-measured, e.g. with another compiler.
    // co-resident workgroups start together and would run their fill / MFMA / store phases in lockstep:
    // delay every other workgroup by about half a stage so that one fills while the other computes
    if (stagger > 0 && (blockIdx.x & 1))
        for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(16);
    bf16_t* patch = reinterpret_cast<bf16_t*>(alsep_smem);
    bf16_t* wts = patch + (size_t)Cf::PGROUPS * 8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;

    // ny_fastest (1-D grid, ntiles % 8 == 0): the Cout/48 workgroups of one tile are dispatched back to back onto the
    // same XCD, so the tile's halo patch comes from HBM once and from that XCD's L2 afterwards
    int tile, ny;
    if (ny_fastest) {
        const int nyc = Cout / Cf::BN, x = blockIdx.x & 7, i = blockIdx.x >> 3;
        tile = x * (ntiles >> 3) + i / nyc;
        ny = i % nyc;
    } else {
        tile = xcd_remap(blockIdx.x, ntiles);
        ny = blockIdx.y;
    }
    const int tf = tile % tiles_f;  tile /= tiles_f;
    const int tt = tile % tiles_t;
    const int64_t b = tile / tiles_t;
    const int t0 = tt * Cf::TH, f0 = tf * TW;
    const int nq = Cin / Cf::KC;

    int pbase[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int pm = wave * 64 + ni * 16 + l15;
        pbase[ni] = ((pm / TW) * Cf::PW + (pm % TW)) * Cf::KC;
    }
    const int wswz = l15 >> 1;                               // (row >> 1) & 7 for row = 16*mi + l15
    f32x4 acc[3][4];
#pragma unroll
    for (int mi = 0; mi < 3; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    const bf16_t* xb = X + b * (int64_t)Th * Fw * Cin;
    for (int q = 0; q < nq; ++q) {
        __syncthreads();                                     // previous chunk's fragment reads are done
        if (!(ablate & 1))
        for (int i = wave; i * 64 < Cf::PGROUPS; i += 4) {
            const int gidx = i * 64 + lane;
            if (gidx < Cf::PGROUPS) {
                const int pix = gidx / Cf::CG, g = gidx % Cf::CG;
                const int t = t0 - 1 + pix / Cf::PW, f = f0 - 1 + pix % Cf::PW;
                const bf16_t* src = (t >= 0 && t < Th && f >= 0 && f < Fw)
                                        ? xb + ((int64_t)t * Fw + f) * Cin + q * Cf::KC + g * 8
                                        : zero_page;
                glds16(src, patch + (size_t)i * 64 * 8);
            }
        }
        const bf16_t* wsrc = Wp + ((int64_t)ny * nq + q) * (Cf::WGROUPS * 8);
        if (!(ablate & 1))
        for (int i = wave; i < Cf::WGROUPS / 64; i += 4) glds16(wsrc + ((size_t)i * 64 + lane) * 8, wts + (size_t)i * 64 * 8);
        __syncthreads();                                     // drains the LDS-DMA (vmcnt(0)) before the barrier
        if (!(ablate & 2))
#pragma unroll 2
        for (int s = 0; s < Cf::NS; ++s) {
            const int grp = 4 * s + lq;
            const int gc = grp < Cf::NG ? grp : Cf::NG - 1;   // padded groups: weights are zero there
            const int tap = gc / Cf::CG, cg = gc % Cf::CG;
            const int koff = ((tap / 3) * Cf::PW + (tap % 3)) * Cf::KC + cg * 8;
            bf16x8 xf[4], wf[3];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) xf[ni] = lds_frag<bf16_t>(patch + pbase[ni] + koff);
#pragma unroll
            for (int mi = 0; mi < 3; ++mi) wf[mi] = lds_frag<bf16_t>(wts + ((mi * 16 + l15) * Cf::WG + (grp ^ wswz)) * 8);
#pragma unroll
            for (int mi = 0; mi < 3; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) mma_step(acc[mi][ni], wf[mi], xf[ni]);
        }
    }
    bf16_t* yb = Y + b * (int64_t)Th * Fw * Cout;
    if (ablate & 4) return;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int pm = wave * 64 + ni * 16 + l15;
        const int t = t0 + pm / TW, f = f0 + pm % TW;
        if (t < Th && f < Fw) {
#pragma unroll
            for (int mi = 0; mi < 3; ++mi) {
                const int co = ny * Cf::BN + mi * 16 + 4 * lq;
                float y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[mi][ni][r], scale[co + r], shift[co + r]), 0.f);
                store4(yb + ((int64_t)t * Fw + f) * Cout + co, y);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// bf16 3x3 convolution, shallow levels (Cin = 48 or 96): persistent, weights in registers.
// Measured on conv3x3_bf16_kernel (profiles/r01_conv_ablation_*): a workgroup's LDS fill, MFMA and store
// phases do not overlap (the two co-resident workgroups run in lockstep), and the fill is the
// longest phase because every 256-pixel tile re-stages its 43 KiB weight block.  Here
//  * a workgroup owns one 48-channel output block (ny = blockIdx.y) for its whole life and keeps
//    that block's weights for all NQ input chunks in VGPRs (NQ x 14 k-steps x 3 fragments), read
//    once from the packed image -- LDS carries only halo patches;
//  * it walks tiles blockIdx.x, +gridDim.x, ... with a 3-deep ring of patch chunks filled by
//    LDS-DMA two stages ahead: counted s_waitcnt vmcnt + raw s_barrier keep the DMA in flight
//    across barriers while the MFMAs of the current stage and the stores of the last tile run.
// vmcnt bookkeeping (in-order counter; every wave issues exactly GL LDS-DMA per stage and ST
// stores per tile, tiles are never partial): see wait_stage below.
// ------------------------------------------------------------------------------------------
template <int NQ, int RING_ = 3, int TW_ = 64>
struct ConvRW {
    static constexpr int TW = TW_, TH = 4, KC = 48, BN = 48, CG = 6, NG = 54, NS = 14, WGRP = 56;
    static constexpr int NI = TW_ / 16;                     // 16-pixel MFMA column blocks per wave (one tile row)
    static constexpr int PW = TW + 2, PH = TH + 2;
    static constexpr int PGROUPS = PH * PW * CG;            // real 16-byte groups per patch chunk (2376 / 1224)
    static constexpr int GL = (PGROUPS + 255) / 256;        // LDS-DMA instructions per wave per stage (10 / 5)
    static constexpr int STAGE_GROUPS = GL * 4 * 64;        // 2560 / 1280
    static constexpr int RING = RING_, AHEAD = RING_ - 1;   // ring slots, prefetch distance in stages
    static constexpr int ST = 3 * NI;                       // stores per wave per tile
    static_assert(GL <= NS, "one LDS-DMA per k-step");
    static constexpr size_t ring_bytes = 16 * (size_t)STAGE_GROUPS * RING;  // 120 KiB
    static constexpr size_t lds_bytes = ring_bytes + 2 * BN * sizeof(float);   // + scale/shift of this output block
};

// RING_ = 3, OCC = 1: one workgroup per CU, prefetch two stages ahead.  RING_ = 2, OCC = 2 (NQ = 1): two workgroups per CU,
// prefetch one stage ahead -- with ONE wave per SIMD the MFMA loop, the LDS-DMA issue and the epilogue of a stage run back to
// back (each near its own hardware limit, profiles/r01_conv_ablation_*); a second, independent workgroup on the same SIMDs
// fills those gaps.
template <int NQ, int RING_ = 3, int OCC = 1, int TW_ = 64>
__global__ void __launch_bounds__(kThreads, OCC)
conv3x3_bf16_regw_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wp,
                         const float* __restrict__ scale, const float* __restrict__ shift,
                         const bf16_t* __restrict__ zero_page, int Th, int Fw, int Cin, int Cout, int tiles_t,
                         int tiles_f, int ntiles) {
    typedef ConvRW<NQ, RING_, TW_> Cf;
    bf16_t* ring = reinterpret_cast<bf16_t*>(alsep_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int ny = blockIdx.y;

    // weights of this output block, straight from the packed (swizzled) image into registers
    bf16x8 wf[NQ][Cf::NS][3];
    {
        const int wswz = l15 >> 1;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const bf16_t* wsrc = Wp + ((int64_t)ny * NQ + q) * (Cf::BN * Cf::WGRP * 8);
#pragma unroll
            for (int s = 0; s < Cf::NS; ++s)
#pragma unroll
                for (int mi = 0; mi < 3; ++mi)
                    wf[q][s][mi] = *reinterpret_cast<const bf16x8*>(wsrc + ((mi * 16 + l15) * Cf::WGRP + ((4 * s + lq) ^ wswz)) * 8);
        }
    }
    float* ss = reinterpret_cast<float*>(alsep_smem + Cf::ring_bytes);      // [scale 48 | shift 48]
    if (tid < Cf::BN) {
        ss[tid] = scale[ny * Cf::BN + tid];
        ss[Cf::BN + tid] = shift[ny * Cf::BN + tid];
    }
    int pbase[Cf::NI];
#pragma unroll
    for (int ni = 0; ni < Cf::NI; ++ni) pbase[ni] = (wave * Cf::PW + ni * 16 + l15) * Cf::KC;   // wave w = tile row w
    // patch offset of k-group (4s + lq): groups advance by 4 per step -> (tap, cg) by incremental update
    auto koff_of = [&](int s) {
        const int grp = 4 * s + lq;
        const int gc = grp < Cf::NG ? grp : Cf::NG - 1;
        const int tap = gc / Cf::CG, cg = gc % Cf::CG;
        return ((tap / 3) * Cf::PW + (tap % 3)) * Cf::KC + cg * 8;
    };
    wait_vmcnt<0>();                                         // weights are in registers, scale/shift on their way to LDS
    __syncthreads();

    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int nstage = my_tiles * NQ;

    // LDS-DMA descriptors of this lane: instruction j of a stage moves 16-byte group gidx = (wave + 4 j) * 64 + lane of
    // the halo patch; its offset from the patch origin (pixel (t0-1, f0-1), chunk q) does not depend on the tile.  With
    // them the per-stage address work is one add per instruction (it was two divisions, a bounds test and a 64-bit
    // multiply per instruction: ~250 VALU instructions per stage on a kernel with ONE wave per SIMD, where nothing
    // overlaps the MFMAs unless it is interleaved with them).
    // (two workgroups per CU: 256 registers per wave, the descriptors are recomputed -- constant divisions -- instead)
    constexpr bool DESC_REGS = OCC == 1;
    int doff[DESC_REGS ? Cf::GL : 1], dpos[DESC_REGS ? Cf::GL : 1];   // element offset; pr | pc << 8 | real-group bit << 16
    auto desc = [&](int j, int& off, int& pos) {
        const int gidx = (wave + 4 * j) * 64 + lane;
        const int pix = gidx / Cf::CG, g = gidx % Cf::CG;
        const int pr = pix / Cf::PW, pc = pix % Cf::PW;
        off = (pr * Fw + pc) * Cin + g * 8;
        pos = pr | (pc << 8) | ((gidx < Cf::PGROUPS ? 1 : 0) << 16);
    };
    if (DESC_REGS) {
#pragma unroll
        for (int j = 0; j < Cf::GL; ++j) desc(j, doff[DESC_REGS ? j : 0], dpos[DESC_REGS ? j : 0]);
    }
    // tile origin of the stage being prefetched (wave-uniform), set by issue_prep, used by issue_one
    const bf16_t* iss_org = X;
    bf16_t* iss_dst = ring;
    int iss_t0 = 0, iss_f0 = 0;
    bool iss_interior = false;
    auto issue_prep = [&](int st, int slot) {
        int tile = (int)blockIdx.x + (st / NQ) * (int)gridDim.x;
        const int q = st % NQ;
        const int tf = tile % tiles_f;  tile /= tiles_f;
        const int tt = tile % tiles_t;
        const int64_t b = tile / tiles_t;
        iss_t0 = tt * Cf::TH - 1;
        iss_f0 = tf * Cf::TW - 1;
        iss_org = X + b * (int64_t)Th * Fw * Cin + q * Cf::KC + ((int64_t)iss_t0 * Fw + iss_f0) * Cin;
        iss_interior = iss_t0 >= 0 && iss_t0 + Cf::PH <= Th && iss_f0 >= 0 && iss_f0 + Cf::PW <= Fw;
        iss_dst = ring + (size_t)slot * Cf::STAGE_GROUPS * 8;
    };
    auto issue_one = [&](int j) {
        // branch-free: these few VALU instructions sit between MFMAs (unsigned compare = both bounds at once)
        int off, pos;
        if (DESC_REGS) { off = doff[DESC_REGS ? j : 0]; pos = dpos[DESC_REGS ? j : 0]; }
        else desc(j, off, pos);
        const unsigned t = (unsigned)(iss_t0 + (pos & 255)), f = (unsigned)(iss_f0 + ((pos >> 8) & 255));
        const bool inb = (pos >> 16) != 0 && (iss_interior || (t < (unsigned)Th && f < (unsigned)Fw));
        const bf16_t* src = inb ? iss_org + off : zero_page;
        glds16(src, iss_dst + (size_t)(wave + 4 * j) * 64 * 8);
    };
    auto issue = [&](int st, int slot) {
        issue_prep(st, slot);
#pragma unroll
        for (int j = 0; j < Cf::GL; ++j) issue_one(j);
    };

    f32x4 acc[3][Cf::NI];
    // Stage body; SLOT and the position of the stage in the pattern are compile-time constants.  One barrier per stage:
    // after it every wave has finished stage st-1, so slot (st+2) % 3 (read by stage st-1) may be refilled, and the
    // prefetch of stage st+2 is issued one LDS-DMA per k-step BETWEEN the MFMAs of stage st.
    // vmcnt (in-order): younger than the DMA of stage st are the DMA of st+1 (GL) and the stores of the tiles finished in
    // stages st-2 and st-1; the first two and the last stage simply drain.
#define ALSEP_RW_STAGE(st_, SLOT_, Q_)                                                             \
    do {                                                                                           \
        if (Cf::AHEAD == 2) {                                                                      \
            if ((st_) >= 2 && (st_) + 1 < nstage) wait_vmcnt<Cf::GL + ((Q_) == 0 ? (NQ == 1 ? 2 : 1) : 1) * Cf::ST>();   \
            else wait_vmcnt<0>();                                                                  \
        } else {                                /* AHEAD == 1 (NQ == 1): only the stores of stage st-1 are younger */ \
            if ((st_) >= 1) wait_vmcnt<Cf::ST>();                                                  \
            else wait_vmcnt<0>();                                                                  \
        }                                                                                          \
        barrier_nodrain();                                                                         \
        const bool pre_ = (st_) + Cf::AHEAD < nstage;                                              \
        if (pre_) issue_prep((st_) + Cf::AHEAD, ((SLOT_) + Cf::AHEAD) % Cf::RING);                 \
        {                                                                                          \
            const bf16_t* patch = ring + (size_t)(SLOT_) * Cf::STAGE_GROUPS * 8;                   \
            if ((Q_) == 0) {                                                                       \
                _Pragma("unroll") for (int mi = 0; mi < 3; ++mi)                                   \
                    _Pragma("unroll") for (int ni = 0; ni < Cf::NI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f}; \
            }                                                                                      \
            _Pragma("unroll") for (int s = 0; s < Cf::NS; ++s) {                                   \
                bf16x8 xf[Cf::NI];                                                                 \
                const int ko = koff_of(s);                                                         \
                _Pragma("unroll") for (int ni = 0; ni < Cf::NI; ++ni) xf[ni] = lds_frag<bf16_t>(patch + pbase[ni] + ko); \
                _Pragma("unroll") for (int mi = 0; mi < 3; ++mi)                                   \
                    _Pragma("unroll") for (int ni = 0; ni < Cf::NI; ++ni) mma_step(acc[mi][ni], wf[Q_][s][mi], xf[ni]); \
                if (s < Cf::GL && pre_) issue_one(s);                                              \
            }                                                                                      \
        }                                                                                          \
        if ((Q_) == NQ - 1) store_tile((st_) / NQ);                                                \
    } while (0)

    auto store_tile = [&](int k) {
        int tile = (int)blockIdx.x + k * (int)gridDim.x;
        const int tf = tile % tiles_f;  tile /= tiles_f;
        const int tt = tile % tiles_t;
        const int64_t b = tile / tiles_t;
        bf16_t* yb = Y + ((b * Th + tt * Cf::TH + wave) * (int64_t)Fw + tf * Cf::TW) * Cout + ny * Cf::BN;
#pragma unroll
        for (int ni = 0; ni < Cf::NI; ++ni)
#pragma unroll
            for (int mi = 0; mi < 3; ++mi) {
                // ext-vector loads on purpose: a HIP float4 (struct) load from LDS makes hipcc put
                // s_waitcnt vmcnt(0) in front of it while an LDS-DMA is in flight, draining the ring
                const f32x4 scv = *reinterpret_cast<const f32x4*>(ss + mi * 16 + 4 * lq);
                const f32x4 shv = *reinterpret_cast<const f32x4*>(ss + Cf::BN + mi * 16 + 4 * lq);
                float y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[mi][ni][r], scv[r], shv[r]), 0.f);
                store4(yb + (int64_t)(ni * 16 + l15) * Cout + mi * 16 + 4 * lq, y);
            }
    };

    if (nstage > 0) issue(0, 0);
    if (Cf::AHEAD == 2 && nstage > 1) issue(1, 1);
    if (Cf::RING == 2) {                                     // NQ == 1: slots alternate
        static_assert(Cf::RING == 3 || NQ == 1, "two-slot ring: single input chunk only");
        for (int st = 0; st < nstage; st += 2) {
            ALSEP_RW_STAGE(st, 0, 0);
            if (st + 1 < nstage) ALSEP_RW_STAGE(st + 1, 1, 0);
        }
        return;
    }
    // the ring slot advances by one per stage and the chunk index by one mod NQ: period lcm(3, NQ)
    for (int st = 0; st < nstage; st += 3 * NQ) {
        if (NQ == 1) {
            ALSEP_RW_STAGE(st, 0, 0);
            if (st + 1 < nstage) ALSEP_RW_STAGE(st + 1, 1, 0);
            if (st + 2 < nstage) ALSEP_RW_STAGE(st + 2, 2, 0);
        } else {
            ALSEP_RW_STAGE(st, 0, 0);
            ALSEP_RW_STAGE(st + 1, 1, 1);
            if (st + 2 < nstage) { ALSEP_RW_STAGE(st + 2, 2, 0); ALSEP_RW_STAGE(st + 3, 0, 1); }
            if (st + 4 < nstage) { ALSEP_RW_STAGE(st + 4, 1, 0); ALSEP_RW_STAGE(st + 5, 2, 1); }
        }
    }
#undef ALSEP_RW_STAGE
}

// ------------------------------------------------------------------------------------------
// bf16 3x3 convolution, levels >= 1 (Cout = 48*NY, NY = 2..4): big-tile persistent kernel.
// The ablations (profiles/r01_conv_ablation_*) show the plain kernel bounded by what goes through
// LDS: 81 KB of LDS-DMA per 10.6 MFLOP stage plus 7 fragment reads per 12 MFMAs.  This kernel cuts
// the bytes instead of trying to hide them:
//  * 8 waves, 512-pixel tile (8 x 64): one 43 KB weight block now feeds twice the MFMAs and the halo
//    overhead drops from 1.55x to 1.29x;
//  * the halo patch of (tile, q) is staged once and all NY output blocks are accumulated against it
//    (NY*48 accumulator registers) instead of re-staging it per block;
//  * the next weight block is prefetched into the other slot of a 2-slot ring while the current one is
//    consumed (counted s_waitcnt vmcnt, raw s_barrier); two waves per SIMD hide the LDS latency.
// LDS: 63,360 (patch) + 2 * 43,008 (weights) + scale/shift = 149.9 KiB, one workgroup per CU.
// ------------------------------------------------------------------------------------------
constexpr int kBigThreads = 512;
template <int NY>
struct ConvBig {
    static constexpr int TW = 64, TH = 8, KC = 48, BN = 48, CG = 6, NG = 54, NS = 14, WGRP = 56;
    static constexpr int PW = TW + 2, PH = TH + 2;
    static constexpr int PGROUPS = PH * PW * CG;            // 3960
    static constexpr int WGROUPS = BN * WGRP;               // 2688
    static constexpr int PINST = (PGROUPS + 63) / 64;       // 62
    static constexpr int WINST = WGROUPS / 64;              // 42: waves 0,1 issue 6, waves 2..7 issue 5
    static constexpr size_t ring_bytes = 16 * (size_t)(PGROUPS + 2 * WGROUPS);
    static constexpr size_t lds_bytes = ring_bytes + 2 * NY * BN * sizeof(float);
    static_assert(lds_bytes <= 160 * 1024, "ConvBig: LDS budget");
    // Output-channel order of the packed weight rows.  An MFMA leaves a lane with rows 4 lq .. 4 lq + 3 of each 16-row block: with the
    // natural order that is 8 bytes of a pixel record per block and 24 (36) scattered 8-byte stores per tile and wave.  Here the 16-row
    // blocks b = 3 yy + mi are paired: rows (4 lq + r) of blocks 2 j and 2 j + 1 hold channels 32 j + 8 lq + {r, 4 + r}, so a lane owns
    // 8 consecutive channels per pair = one 16-byte store, and the four lq lanes of a pixel write 64 contiguous bytes.  An odd last block
    // (NY = 3: b = 8) keeps 4 channels per lane: 128 + 4 lq + r.
    static constexpr int NB = 3 * NY, NPAIR = NB / 2;
    __host__ __device__ static constexpr int channel_of_row(int R) {
        const int b = R / 16, lq = (R % 16) / 4, r = R % 4;
        return b < 2 * NPAIR ? (b >> 1) * 32 + lq * 8 + (b & 1) * 4 + r : b * 16 + lq * 4 + r;
    }
};

template <int NY>
__global__ void __launch_bounds__(kBigThreads, 2)
conv3x3_bf16_big_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wp,
                        const float* __restrict__ scale, const float* __restrict__ shift,
                        const bf16_t* __restrict__ zero_page, int Th, int Fw, int Cin, int Cout, int tiles_t,
                        int tiles_f, int ntiles) {
    typedef ConvBig<NY> Cf;
    bf16_t* patch = reinterpret_cast<bf16_t*>(alsep_smem);
    bf16_t* wring = patch + (size_t)Cf::PGROUPS * 8;
    float* ss = reinterpret_cast<float*>(alsep_smem + Cf::ring_bytes);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int nq = Cin / Cf::KC;
    const int wswz = l15 >> 1;
    for (int i = tid; i < NY * Cf::BN; i += kBigThreads) {
        ss[i] = scale[i];
        ss[NY * Cf::BN + i] = shift[i];
    }
    __syncthreads();

    int pbase[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) pbase[ni] = (wave * Cf::PW + ni * 16 + l15) * Cf::KC;
    auto koff_of = [&](int s) {
        const int grp = 4 * s + lq;
        const int gc = grp < Cf::NG ? grp : Cf::NG - 1;
        const int tap = gc / Cf::CG, cg = gc % Cf::CG;
        return ((tap / 3) * Cf::PW + (tap % 3)) * Cf::KC + cg * 8;
    };
    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int nstage = my_tiles * NY * nq;

    auto tile_coords = [&](int k, int& t0, int& f0, int64_t& b) {
        int tile = (int)blockIdx.x + k * (int)gridDim.x;
        const int tf = tile % tiles_f;  tile /= tiles_f;
        const int tt = tile % tiles_t;
        b = tile / tiles_t;
        t0 = tt * Cf::TH;
        f0 = tf * Cf::TW;
    };
    // LDS-DMA descriptors of the halo patch, computed once: piece j of this wave is instruction i = wave + 8 j of the PINST = 62 that
    // cover the patch; lane -> (pixel, channel group) never changes, so the element offset from the tile's first pixel and the four
    // "outside the image if the tile touches that border" bits are per-lane constants.  (Computed per patch, the divisions and 64-bit
    // address arithmetic of 8 pieces cost each wave ~4,000 cycles per patch: 14 % of the kernel, in-kernel stamps of round 2.)
    constexpr int PJ = (Cf::PINST + 7) / 8;
    int prel[PJ];
    unsigned pflags = 0;                                     // 4 bits per piece: top row, bottom row, left column, right column of the halo
    bool plast_ok = true;                                    // lanes of the last, partial instruction that hold a patch group
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
        const int gidx = (wave + 8 * j) * 64 + lane;
        const int gi = gidx < Cf::PGROUPS ? gidx : Cf::PGROUPS - 1;
        const int pix = gi / Cf::CG, g = gi % Cf::CG;
        const int dt = pix / Cf::PW - 1, df = pix % Cf::PW - 1;
        prel[j] = (dt * Fw + df) * Cin + g * 8;
        pflags |= (unsigned)((dt < 0) | ((dt >= Cf::TH) << 1) | ((df < 0) << 2) | ((df >= Cf::TW) << 3)) << (4 * j);
        if (j == PJ - 1) plast_ok = gidx < Cf::PGROUPS;
    }
    auto issue_patch = [&](int ps) {                         // (tile ps / nq, chunk ps % nq); waited with vmcnt(0)
        int t0, f0; int64_t b;
        tile_coords(ps / nq, t0, f0, b);
        const bf16_t* xb = X + ((b * Th + t0) * (int64_t)Fw + f0) * Cin + (ps % nq) * Cf::KC;
        const unsigned border = (unsigned)(t0 == 0) | ((unsigned)(t0 + Cf::TH >= Th) << 1) | ((unsigned)(f0 == 0) << 2) |
                                ((unsigned)(f0 + Cf::TW >= Fw) << 3);
#pragma unroll
        for (int j = 0; j < PJ; ++j) {
            const int i = wave + 8 * j;
            if (j < PJ - 1 || i < Cf::PINST) {
                const bool out = (pflags & (border << (4 * j))) != 0;
                const bf16_t* src = out ? zero_page : xb + prel[j];
                if (j < PJ - 1 || plast_ok) glds16(src, patch + (size_t)i * 64 * 8);
            }
        }
    };
    // weight block of stage s -> slot s & 1: 42 LDS-DMA instructions over 8 waves (waves 0, 1: six; the others five)
    const bf16_t* wsrc_next = Wp;
    bf16_t* wdst_next = wring;
    auto weights_prep = [&](int s) {
        const int ny = s % NY, q = (s / NY) % nq;
        wsrc_next = Wp + ((int64_t)ny * nq + q) * (Cf::WGROUPS * 8);
        wdst_next = wring + (size_t)(s & 1) * Cf::WGROUPS * 8;
    };
    auto weights_one = [&](int j) {
        const int i = wave + 8 * j;
        if (i < Cf::WINST) glds16(wsrc_next + ((size_t)i * 64 + lane) * 8, wdst_next + (size_t)i * 64 * 8);
    };

    // Stage s: ny = s % NY, patch ps = s / NY (tile ps / nq, input chunk q = ps % nq).  In-order vmcnt bookkeeping:
    //  * the weight block of stage s+1 is issued one LDS-DMA per k-step BETWEEN the MFMAs of stage s (its slot was read
    //    by stage s-1, which every wave has left once it is past stage s's barrier);
    //  * after the last stage of a patch: barrier (patch free), LDS-DMA of the next patch, THEN the epilogue stores of a
    //    finished tile -- the next stage waits with vmcnt(ST), i.e. for the patch and weights but not for the stores.
    // Barriers: one per stage plus one per patch (was two per stage plus one per patch, with every tile's stores and every
    // patch's DMA latency drained at vmcnt(0)).
    constexpr int ST = 4 * (Cf::NPAIR + Cf::NB % 2);         // epilogue stores per wave
    f32x4 acc[NY][3][4];
    if (nstage > 0) {
        issue_patch(0);
        weights_prep(0);
#pragma unroll
        for (int j = 0; j < 6; ++j) weights_one(j);
    }
    for (int s = 0; s < nstage; ++s) {
        const int ny = s % NY, ps = s / NY, q = ps % nq;
        const bool last = s + 1 >= nstage;
        const bool after_epilogue = ny == 0 && q == 0 && s > 0;   // the previous stage ended a tile: its stores are younger
        if (after_epilogue) wait_vmcnt<ST>();
        else wait_vmcnt<0>();
        barrier_nodrain();
        if (!last) weights_prep(s + 1);
        {
            const bf16_t* wts = wring + (size_t)(s & 1) * Cf::WGROUPS * 8;
#pragma unroll
            for (int yy = 0; yy < NY; ++yy) {
                if (yy == ny) {
                    if (q == 0) {
#pragma unroll
                        for (int mi = 0; mi < 3; ++mi)
#pragma unroll
                            for (int ni = 0; ni < 4; ++ni) acc[yy][mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
#pragma unroll 2
                    for (int st = 0; st < Cf::NS; ++st) {
                        const int ko = koff_of(st);
                        bf16x8 xf[4], wf[3];
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni) xf[ni] = lds_frag<bf16_t>(patch + pbase[ni] + ko);
#pragma unroll
                        for (int mi = 0; mi < 3; ++mi)
                            wf[mi] = lds_frag<bf16_t>(wts + ((mi * 16 + l15) * Cf::WGRP + ((4 * st + lq) ^ wswz)) * 8);
#pragma unroll
                        for (int mi = 0; mi < 3; ++mi)
#pragma unroll
                            for (int ni = 0; ni < 4; ++ni) mma_step(acc[yy][mi][ni], wf[mi], xf[ni]);
                        if (st < 6 && !last) weights_one(st);
                    }
                }
            }
        }
        if (ny == NY - 1) {
            barrier_nodrain();                               // every wave has left the patch: it may be refilled
            if (!last) issue_patch(ps + 1);
            if (q == nq - 1) {
                int t0, f0; int64_t b;
                tile_coords(ps / nq, t0, f0, b);
                bf16_t* yb = Y + ((b * Th + t0 + wave) * (int64_t)Fw + f0) * Cout;
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    bf16_t* yp = yb + (int64_t)(ni * 16 + l15) * Cout;
#pragma unroll
                    for (int j = 0; j < Cf::NPAIR; ++j) {            // blocks 2 j, 2 j + 1: channels 32 j + 8 lq + [0, 8) (ConvBig::channel_of_row)
                        const int co = j * 32 + lq * 8;
                        float y[8];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int bb = 2 * j + h;
                            const f32x4 scv = *reinterpret_cast<const f32x4*>(ss + co + 4 * h);      // ext-vector load: see regw kernel
                            const f32x4 shv = *reinterpret_cast<const f32x4*>(ss + NY * Cf::BN + co + 4 * h);
#pragma unroll
                            for (int r = 0; r < 4; ++r) y[4 * h + r] = fmaxf(fmaf(acc[bb / 3][bb % 3][ni][r], scv[r], shv[r]), 0.f);
                        }
                        store8(yp + co, y);
                    }
                    if constexpr (Cf::NB % 2 == 1) {
                        constexpr int bb = Cf::NB - 1;
                        const int co = bb * 16 + lq * 4;
                        const f32x4 scv = *reinterpret_cast<const f32x4*>(ss + co);
                        const f32x4 shv = *reinterpret_cast<const f32x4*>(ss + NY * Cf::BN + co);
                        float y[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[bb / 3][bb % 3][ni][r], scv[r], shv[r]), 0.f);
                        store4(yp + co, y);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// bf16 3x3 convolution, level 1 (c = 96): everything double-buffered.
// Stamps of the merged kernel (profiles/r02_big_conv_stamps.txt): with its k-loop at 89 % of the MFMA issue floor, 17 % of the launch is
// the halo patch's LDS-DMA (62 KB after a barrier, at the ~18 B/clk a CU's LDS-DMA path delivers) with nothing to overlap it --
// a second 63 KB patch does not fit beside two 43 KB weight slots.  Cutting the input channels into chunks of 32 instead of 48 makes
// both fit: patch 10 x 66 pixels x 64 B = 42 KB (x 2), weight slot 96 rows x 5 taps x 64 B = 30 KB (x 2), 147 KB in all.  A chunk's
// nine taps are nine k-steps of exactly one tap each (no padded k-groups: 648 instead of 672 MFMAs per tile and wave), run as two
// stages of 5 + 4 taps; the next patch and the next weight slot arrive by LDS-DMA spread over the k-steps; ONE barrier per stage,
// none per patch.  64-byte pixel records: k-group cg of pixel P sits at position cg ^ (((P >> 2) & 1) << 1), which makes the
// ds_read_b128 of 16 consecutive pixels x {lq, lq ^ 1} conflict-free (scripts/lds_bank_sim.py).  The k order inside a layer differs from
// the 48-channel kernels' (chunks of 32 channels, tap-major inside): same products, another fp32 summation order -- equal to them up
// to flipped bf16 roundings, not bit-identical.
// ------------------------------------------------------------------------------------------
struct ConvMq {
    static constexpr int NY = 2, TW = 64, TH = 8, KC = 32, CG = 4, NS = 9, PW = TW + 2, PH = TH + 2;
    static constexpr int PARTS = 2, KS = 5;                 // taps 0..4, 5..8
    static constexpr int WG = 4 * KS, ROWS = 96, NB = 6, NPAIR = 3;
    static constexpr int PGROUPS = PH * PW * CG, PINST = (PGROUPS + 63) / 64, PJ = (PINST + 7) / 8;       // 2640, 42, 6
    static constexpr int WGROUPS = ROWS * WG, WINST = WGROUPS / 64, WJ = (WINST + 7) / 8;                 // 1920, 30, 4
    static constexpr int PBUF = PINST * 64;                 // a patch buffer holds whole LDS-DMA instructions (48 dead units at its end)
    static constexpr size_t ring_bytes = 16 * (size_t)(2 * PBUF + 2 * WGROUPS);
    static constexpr size_t lds_bytes = ring_bytes + 2 * ROWS * sizeof(float) + 1024;   // + 1 KiB scratch (surplus DMA pieces)
    static_assert(lds_bytes <= 160 * 1024, "ConvMq: LDS budget");
    __host__ __device__ static constexpr int ksteps_of_part(int pt) { return pt == 0 ? KS : NS - KS; }
    __host__ __device__ static constexpr int wswz(int row) { return (4 - ((row >> 2) & 3)) & 3; }
    __host__ __device__ static constexpr int pswz(int pix) { return ((pix >> 2) & 1) << 1; }
};

template <int TAP, int STL>
__device__ __forceinline__ void mq_issue_reads(bf16x8 (&xf)[4], bf16x8 (&wf)[6], const bf16_t* patch, const int (&pk)[9], const bf16_t* wl) {
    typedef ConvMq Cf;
    const bf16_t* pl = patch + pk[TAP];
    lds_read_async_b128<0 * 16 * Cf::KC * 2>(xf[0], pl);
    lds_read_async_b128<1 * 16 * Cf::KC * 2>(xf[1], pl);
    lds_read_async_b128<2 * 16 * Cf::KC * 2>(xf[2], pl);
    lds_read_async_b128<3 * 16 * Cf::KC * 2>(xf[3], pl);
    lds_read_async_b128<(0 * 16 * Cf::WG * 8 + STL * 32) * 2>(wf[0], wl);
    lds_read_async_b128<(1 * 16 * Cf::WG * 8 + STL * 32) * 2>(wf[1], wl);
    lds_read_async_b128<(2 * 16 * Cf::WG * 8 + STL * 32) * 2>(wf[2], wl);
    lds_read_async_b128<(3 * 16 * Cf::WG * 8 + STL * 32) * 2>(wf[3], wl);
    lds_read_async_b128<(4 * 16 * Cf::WG * 8 + STL * 32) * 2>(wf[4], wl);
    lds_read_async_b128<(5 * 16 * Cf::WG * 8 + STL * 32) * 2>(wf[5], wl);
}
__device__ __forceinline__ void mq_mma(f32x4 (&acc)[6][4], const bf16x8 (&wf)[6], const bf16x8 (&xf)[4]) {
#pragma unroll
    for (int b = 0; b < 6; ++b)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) mma_step(acc[b][ni], wf[b], xf[ni]);
}
template <int PT, int STL, typename Dma>
__device__ __forceinline__ void mq_steps(f32x4 (&acc)[6][4], bf16x8 (&xa)[4], bf16x8 (&wa)[6], bf16x8 (&xb)[4], bf16x8 (&wb)[6],
                                         const bf16_t* patch, const int (&pk)[9], const bf16_t* wl, Dma dma) {
    constexpr int N = ConvMq::ksteps_of_part(PT), T0 = PT * ConvMq::KS;
    if constexpr (STL < N) {
        if constexpr (STL == 0) mq_issue_reads<T0, 0>(xa, wa, patch, pk, wl);
        lds_wait_n<0>();
        if constexpr (STL + 1 < N) mq_issue_reads<T0 + STL + 1, STL + 1>(xb, wb, patch, pk, wl);
        mq_mma(acc, wa, xa);
        dma(STL);
        sched_fence();
        if constexpr (STL + 1 < N) {
            lds_wait_n<0>();
            if constexpr (STL + 2 < N) mq_issue_reads<T0 + STL + 2, STL + 2>(xa, wa, patch, pk, wl);
            mq_mma(acc, wb, xb);
            dma(STL + 1);
            sched_fence();
            mq_steps<PT, STL + 2>(acc, xa, wa, xb, wb, patch, pk, wl, dma);
        }
    }
}

__global__ void __launch_bounds__(kBigThreads, 2)
conv3x3_bf16_mq_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wp, const float* __restrict__ scale,
                       const float* __restrict__ shift, const bf16_t* __restrict__ zero_page, int Th, int Fw, int Cin, int Cout, int tiles_t,
                       int tiles_f, int ntiles) {
    typedef ConvMq Cf;
    bf16_t* const patch0 = reinterpret_cast<bf16_t*>(alsep_smem);
    bf16_t* const wring = patch0 + (size_t)2 * Cf::PBUF * 8;
    float* ss = reinterpret_cast<float*>(alsep_smem + Cf::ring_bytes);
    bf16_t* const scratch = reinterpret_cast<bf16_t*>(alsep_smem + Cf::lds_bytes - 1024);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int nq = Cin / Cf::KC;
    for (int i = tid; i < Cf::ROWS; i += kBigThreads) {
        ss[i] = scale[i];
        ss[Cf::ROWS + i] = shift[i];
    }
    __syncthreads();

    // per-lane LDS element offsets of the nine taps (pixel row = wave + dy, column = l15 + dx; + 16 pixels per ni: an immediate)
    int pk[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int P = (wave + tap / 3) * Cf::PW + (tap % 3) + l15;
        pk[tap] = (P * Cf::CG + (lq ^ Cf::pswz(P))) * 8;
    }
    const int wl_off = (l15 * Cf::WG + (lq ^ Cf::wswz(l15))) * 8;

    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int npatch = my_tiles * nq, nstage = npatch * Cf::PARTS;
    auto tile_coords = [&](int k, int& t0, int& f0, int64_t& b) {
        int tile = (int)blockIdx.x + k * (int)gridDim.x;
        const int tf = tile % tiles_f;  tile /= tiles_f;
        const int tt = tile % tiles_t;
        b = tile / tiles_t;
        t0 = tt * Cf::TH;
        f0 = tf * Cf::TW;
    };
    // LDS-DMA descriptors of a halo patch, computed once: lane -> 16-byte unit u of the patch image -> (pixel, position) -> channel group
    int prel[Cf::PJ];
    unsigned pflags = 0;
#pragma unroll
    for (int j = 0; j < Cf::PJ; ++j) {
        const int u = (wave + 8 * j) * 64 + lane;
        const int uu = u < Cf::PGROUPS ? u : Cf::PGROUPS - 1;
        const int P = uu / Cf::CG, cg = (uu % Cf::CG) ^ Cf::pswz(P);
        const int dt = P / Cf::PW - 1, df = P % Cf::PW - 1;
        prel[j] = (dt * Fw + df) * Cin + cg * 8;
        // the dead units at the end of the buffer (u >= PGROUPS) read the zero page: flagged as outside on every side
        pflags |= (u < Cf::PGROUPS ? (unsigned)((dt < 0) | ((dt >= Cf::TH) << 1) | ((df < 0) << 2) | ((df >= Cf::TW) << 3)) : 16u) << (5 * j);
    }
    // patch ps (tile ps / nq, chunk ps % nq) -> buffer ps & 1; piece j of this wave.  Past the last patch the last one is fetched again
    // into the free buffer (keeps the per-stage LDS-DMA count constant: the vmcnt waits below count instructions)
    const bf16_t* psrc = X;
    unsigned pborder = 0;
    bf16_t* pdst = patch0;
    auto patch_prep = [&](int ps) {
        const int pc = ps < npatch ? ps : npatch - 1;
        int t0, f0; int64_t b;
        tile_coords(pc / nq, t0, f0, b);
        psrc = X + ((b * Th + t0) * (int64_t)Fw + f0) * Cin + (pc % nq) * Cf::KC;
        pborder = (unsigned)(t0 == 0) | ((unsigned)(t0 + Cf::TH >= Th) << 1) | ((unsigned)(f0 == 0) << 2) | ((unsigned)(f0 + Cf::TW >= Fw) << 3);
        pdst = patch0 + (size_t)(ps & 1) * Cf::PBUF * 8;
    };
    auto patch_one = [&](int j) {                            // 5 flag bits per piece: the four borders + "dead unit"
        const int i = wave + 8 * j;
        const bool out = (pflags & ((pborder | 16u) << (5 * j))) != 0;
        const bool real = j < Cf::PJ - 1 || i < Cf::PINST;   // instructions 40, 41: waves 0 and 1 only
        const bf16_t* src = (out || !real) ? zero_page : psrc + prel[j];
        glds16(src, real ? pdst + (size_t)i * 64 * 8 : scratch);
    };
    const bf16_t* wsrc_next = Wp;
    bf16_t* wdst_next = wring;
    auto weights_prep = [&](int s) {
        const int pt = s % Cf::PARTS, q = (s / Cf::PARTS) % nq;
        wsrc_next = Wp + ((int64_t)q * Cf::PARTS + pt) * (Cf::WGROUPS * 8);
        wdst_next = wring + (size_t)(s & 1) * Cf::WGROUPS * 8;
    };
    auto weights_one = [&](int j) {
        const int i = wave + 8 * j;
        const bool real = i < Cf::WINST;
        glds16(wsrc_next + ((size_t)(real ? i : 0) * 64 + lane) * 8, real ? wdst_next + (size_t)i * 64 * 8 : scratch);
    };

    constexpr int ST = 4 * Cf::NPAIR;                        // epilogue stores per wave
    f32x4 acc[Cf::NB][4];
    if (nstage > 0) {
        patch_prep(0);
#pragma unroll
        for (int j = 0; j < Cf::PJ; ++j) patch_one(j);
        weights_prep(0);
#pragma unroll
        for (int j = 0; j < Cf::WJ; ++j) weights_one(j);
    }
    for (int s = 0; s < nstage; ++s) {
        const int pt = s % Cf::PARTS, ps = s / Cf::PARTS, q = ps % nq;
        // In flight, oldest first: [this stage's weights (and patch)] [part 1: the PJ pieces of the next patch] [after an epilogue: ST stores]
        if (pt == 1) wait_vmcnt<Cf::PJ>();
        else if (q == 0 && s > 0) wait_vmcnt<ST>();
        else wait_vmcnt<0>();
        barrier_nodrain();
        weights_prep(s + 1);
        if (pt == 0) patch_prep(ps + 1);
        if (q == 0 && pt == 0) {
#pragma unroll
            for (int b = 0; b < Cf::NB; ++b)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[b][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        {
            const bf16_t* patch = patch0 + (size_t)(ps & 1) * Cf::PBUF * 8;
            const bf16_t* wl = wring + (size_t)(s & 1) * Cf::WGROUPS * 8 + wl_off;
            bf16x8 xa[4], wa[Cf::NB], xb[4], wb[Cf::NB];
#pragma unroll
            for (int k = 0; k < Cf::PARTS; ++k) {
                if (k == pt) {
                    // LDS-DMA schedule.  Part 0 (5 taps): the next weight slot first, then the WHOLE next patch (not needed before
                    // the stage after next: still in flight at the next stage's vmcnt(PJ)); part 1 (4 taps): only its weights, early
                    if (k == 0)
                        mq_steps<0, 0>(acc, xa, wa, xb, wb, patch, pk, wl, [&](int st) {
                            if (st == 0) { weights_one(0); weights_one(1); }
                            if (st == 1) { weights_one(2); weights_one(3); }
                            if (st == 2) { patch_one(0); patch_one(1); }
                            if (st == 3) { patch_one(2); patch_one(3); }
                            if (st == 4) { patch_one(4); patch_one(5); }
                        });
                    if (k == 1)
                        mq_steps<1, 0>(acc, xa, wa, xb, wb, patch, pk, wl, [&](int st) {
                            if (st == 0) { weights_one(0); weights_one(1); }
                            if (st == 1) { weights_one(2); weights_one(3); }
                        });
                }
            }
        }
        if (pt == Cf::PARTS - 1 && q == nq - 1) {
            int t0, f0; int64_t b;
            tile_coords(ps / nq, t0, f0, b);
            bf16_t* yb = Y + ((b * Th + t0 + wave) * (int64_t)Fw + f0) * Cout;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                bf16_t* yp = yb + (int64_t)(ni * 16 + l15) * Cout;
#pragma unroll
                for (int j = 0; j < Cf::NPAIR; ++j) {            // blocks 2 j, 2 j + 1: channels 32 j + 8 lq + [0, 8) (ConvBig::channel_of_row)
                    const int co = j * 32 + lq * 8;
                    float y[8];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f32x4 scv = *reinterpret_cast<const f32x4*>(ss + co + 4 * h);
                        const f32x4 shv = *reinterpret_cast<const f32x4*>(ss + Cf::ROWS + co + 4 * h);
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[4 * h + r] = fmaxf(fmaf(acc[2 * j + h][ni][r], scv[r], shv[r]), 0.f);
                    }
                    store8(yp + co, y);
                }
            }
        }
    }
    wait_vmcnt<0>();                                         // the surplus LDS-DMA of the last stages lands before the wave ends
}

// ------------------------------------------------------------------------------------------
// bf16 3x3 convolution, level 0 (c = 48), in the structure of conv3x3_bf16_mq_kernel: 8 waves, 8 x 48-pixel tiles (one row of three
// 16-pixel blocks per wave), the 43 KB weight block resident in LDS for the life of the workgroup (loaded once: no weight stream at
// all), two 48 KB halo patches (the next tile's arrives by LDS-DMA during this tile's k-loop), one barrier per tile, no VALU in the
// k-loop (per-lane LDS bases + immediates, asm reads one k-step ahead), 16- and 8-byte epilogue stores.  Against the register-weight
// kernel: halo 1.30 x instead of 1.59 x through the LDS-DMA path, 126 MFMAs per barrier instead of 84, descriptors computed once.
// Same k order as every 48-channel kernel: bit-identical to the plain kernel.
// ------------------------------------------------------------------------------------------
struct ConvM0 {
    static constexpr int TW = 48, TH = 8, KC = 48, CG = 6, NG = 54, NS = 14, WGRP = 56, NI = 3, NB = 3, ROWS = 48;
    static constexpr int PW = TW + 2, PH = TH + 2;
    static constexpr int PGROUPS = PH * PW * CG, PINST = (PGROUPS + 63) / 64, PJ = (PINST + 7) / 8, PBUF = PINST * 64;   // 3000, 47, 6, 3008
    static constexpr int WGROUPS = ROWS * WGRP, WINST = WGROUPS / 64;                                                  // 2688, 42
    static constexpr size_t ring_bytes = 16 * (size_t)(2 * PBUF + WGROUPS);
    static constexpr size_t lds_bytes = ring_bytes + 2 * ROWS * sizeof(float) + 1024;   // + 1 KiB scratch (surplus DMA pieces)
    static_assert(lds_bytes <= 160 * 1024, "ConvM0: LDS budget");
};

template <int ST>
__device__ __forceinline__ void m0_issue_reads(bf16x8 (&xf)[3], bf16x8 (&wf)[3], const bf16_t* patch, const int (&pk)[14], const bf16_t* we,
                                               const bf16_t* wo) {
    typedef ConvM0 Cf;
    const bf16_t* pl = patch + pk[ST];
    lds_read_async_b128<0 * 16 * Cf::KC * 2>(xf[0], pl);
    lds_read_async_b128<1 * 16 * Cf::KC * 2>(xf[1], pl);
    lds_read_async_b128<2 * 16 * Cf::KC * 2>(xf[2], pl);
    const bf16_t* wl = (ST & 1) ? wo : we;
    lds_read_async_b128<(0 * 16 * Cf::WGRP * 8 + ST * 32) * 2>(wf[0], wl);
    lds_read_async_b128<(1 * 16 * Cf::WGRP * 8 + ST * 32) * 2>(wf[1], wl);
    lds_read_async_b128<(2 * 16 * Cf::WGRP * 8 + ST * 32) * 2>(wf[2], wl);
}
__device__ __forceinline__ void m0_mma(f32x4 (&acc)[3][3], const bf16x8 (&wf)[3], const bf16x8 (&xf)[3]) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int ni = 0; ni < 3; ++ni) mma_step(acc[b][ni], wf[b], xf[ni]);
}
template <int ST, typename Dma>
__device__ __forceinline__ void m0_steps(f32x4 (&acc)[3][3], bf16x8 (&xa)[3], bf16x8 (&wa)[3], bf16x8 (&xb)[3], bf16x8 (&wb)[3],
                                         const bf16_t* patch, const int (&pk)[14], const bf16_t* we, const bf16_t* wo, Dma dma) {
    constexpr int N = ConvM0::NS;
    if constexpr (ST < N) {
        if constexpr (ST == 0) m0_issue_reads<0>(xa, wa, patch, pk, we, wo);
        lds_wait_n<0>();
        if constexpr (ST + 1 < N) m0_issue_reads<ST + 1>(xb, wb, patch, pk, we, wo);
        m0_mma(acc, wa, xa);
        dma(ST);
        sched_fence();
        if constexpr (ST + 1 < N) {
            lds_wait_n<0>();
            if constexpr (ST + 2 < N) m0_issue_reads<ST + 2>(xa, wa, patch, pk, we, wo);
            m0_mma(acc, wb, xb);
            dma(ST + 1);
            sched_fence();
            m0_steps<ST + 2>(acc, xa, wa, xb, wb, patch, pk, we, wo, dma);
        }
    }
}

__global__ void __launch_bounds__(kBigThreads, 2)
conv3x3_bf16_m0_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wp, const float* __restrict__ scale,
                       const float* __restrict__ shift, const bf16_t* __restrict__ zero_page, int Th, int Fw, int Cin, int Cout, int tiles_t,
                       int tiles_f, int ntiles) {
    typedef ConvM0 Cf;
    bf16_t* const patch0 = reinterpret_cast<bf16_t*>(alsep_smem);
    bf16_t* const wts = patch0 + (size_t)2 * Cf::PBUF * 8;
    float* ss = reinterpret_cast<float*>(alsep_smem + Cf::ring_bytes);
    bf16_t* const scratch = reinterpret_cast<bf16_t*>(alsep_smem + Cf::lds_bytes - 1024);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    for (int i = tid; i < Cf::ROWS; i += kBigThreads) {
        ss[i] = scale[i];
        ss[Cf::ROWS + i] = shift[i];
    }
    // the weight block, once: 42 LDS-DMA instructions (waves 0, 1: six; the others five + one into the scratch)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int i = wave + 8 * j;
        const bool real = i < Cf::WINST;
        glds16(Wp + ((size_t)(real ? i : 0) * 64 + lane) * 8, real ? wts + (size_t)i * 64 * 8 : scratch);
    }
    wait_vmcnt<0>();
    __syncthreads();

    int pk[Cf::NS];
#pragma unroll
    for (int st = 0; st < Cf::NS; ++st) {
        const int grp = 4 * st + lq;
        const int gc = grp < Cf::NG ? grp : Cf::NG - 1;
        const int tap = gc / Cf::CG, cg = gc % Cf::CG;
        pk[st] = ((wave + tap / 3) * Cf::PW + (tap % 3) + l15) * Cf::KC + cg * 8;
    }
    // weight row l15, swizzled group of an even / odd k-step (see conv3x3_bf16_big_kernel)
    const int wswz = l15 >> 1;
    const int b32 = (wswz >> 2) * 32, c8 = (lq ^ (wswz & 3)) * 8;
    const bf16_t* const we = wts + l15 * Cf::WGRP * 8 + c8 + b32;
    const bf16_t* const wo = wts + l15 * Cf::WGRP * 8 + c8 - b32;

    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    auto tile_coords = [&](int k, int& t0, int& f0, int64_t& b) {
        int tile = (int)blockIdx.x + k * (int)gridDim.x;
        const int tf = tile % tiles_f;  tile /= tiles_f;
        const int tt = tile % tiles_t;
        b = tile / tiles_t;
        t0 = tt * Cf::TH;
        f0 = tf * Cf::TW;
    };
    int prel[Cf::PJ];
    unsigned pflags = 0;
#pragma unroll
    for (int j = 0; j < Cf::PJ; ++j) {
        const int u = (wave + 8 * j) * 64 + lane;
        const int uu = u < Cf::PGROUPS ? u : Cf::PGROUPS - 1;
        const int P = uu / Cf::CG, cg = uu % Cf::CG;
        const int dt = P / Cf::PW - 1, df = P % Cf::PW - 1;
        prel[j] = (dt * Fw + df) * Cin + cg * 8;
        pflags |= (u < Cf::PGROUPS ? (unsigned)((dt < 0) | ((dt >= Cf::TH) << 1) | ((df < 0) << 2) | ((df >= Cf::TW) << 3)) : 16u) << (5 * j);
    }
    const bf16_t* psrc = X;
    unsigned pborder = 0;
    bf16_t* pdst = patch0;
    auto patch_prep = [&](int k) {                           // tile k of this workgroup -> buffer k & 1 (past the last one: the last again)
        const int kc = k < my_tiles ? k : my_tiles - 1;
        int t0, f0; int64_t b;
        tile_coords(kc, t0, f0, b);
        psrc = X + ((b * Th + t0) * (int64_t)Fw + f0) * Cin;
        pborder = (unsigned)(t0 == 0) | ((unsigned)(t0 + Cf::TH >= Th) << 1) | ((unsigned)(f0 == 0) << 2) | ((unsigned)(f0 + Cf::TW >= Fw) << 3);
        pdst = patch0 + (size_t)(k & 1) * Cf::PBUF * 8;
    };
    auto patch_one = [&](int j) {
        const int i = wave + 8 * j;
        const bool out = (pflags & ((pborder | 16u) << (5 * j))) != 0;
        const bool real = j < Cf::PJ - 1 || i < Cf::PINST;
        const bf16_t* src = (out || !real) ? zero_page : psrc + prel[j];
        glds16(src, real ? pdst + (size_t)i * 64 * 8 : scratch);
    };

    constexpr int ST = 2 * Cf::NI;                           // epilogue stores per wave and tile
    f32x4 acc[3][3];
    if (my_tiles > 0) {
        patch_prep(0);
#pragma unroll
        for (int j = 0; j < Cf::PJ; ++j) patch_one(j);
    }
    auto epilogue = [&](int k) {
        int t0, f0; int64_t b;
        tile_coords(k, t0, f0, b);
        bf16_t* yb = Y + ((b * Th + t0 + wave) * (int64_t)Fw + f0) * Cout;
#pragma unroll
        for (int ni = 0; ni < Cf::NI; ++ni) {
            bf16_t* yp = yb + (int64_t)(ni * 16 + l15) * Cout;
            {                                                // blocks 0, 1: channels 8 lq + [0, 8) (ConvBig<1>::channel_of_row)
                const int co = lq * 8;
                float y[8];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f32x4 scv = *reinterpret_cast<const f32x4*>(ss + co + 4 * h);
                    const f32x4 shv = *reinterpret_cast<const f32x4*>(ss + Cf::ROWS + co + 4 * h);
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[4 * h + r] = fmaxf(fmaf(acc[h][ni][r], scv[r], shv[r]), 0.f);
                }
                store8(yp + co, y);
            }
            {                                                // block 2: channels 32 + 4 lq + [0, 4)
                const int co = 32 + lq * 4;
                const f32x4 scv = *reinterpret_cast<const f32x4*>(ss + co);
                const f32x4 shv = *reinterpret_cast<const f32x4*>(ss + Cf::ROWS + co);
                float y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[2][ni][r], scv[r], shv[r]), 0.f);
                store4(yp + co, y);
            }
        }
    };
    for (int k = 0; k < my_tiles; ++k) {
        // in flight, oldest first: [this tile's patch (and, k = 0, the weights)] [the ST stores of the previous tile]
        if (k > 0) wait_vmcnt<ST>();
        else wait_vmcnt<0>();
        barrier_nodrain();
        patch_prep(k + 1);
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int ni = 0; ni < 3; ++ni) acc[b][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            const bf16_t* patch = patch0 + (size_t)(k & 1) * Cf::PBUF * 8;
            bf16x8 xa[3], wa[3], xb[3], wb[3];
            m0_steps<0>(acc, xa, wa, xb, wb, patch, pk, we, wo, [&](int st) {
                if (st < Cf::PJ) patch_one(st);              // the next tile's patch, one piece per k-step
            });
        }
        epilogue(k);
    }
    wait_vmcnt<0>();
}

// ------------------------------------------------------------------------------------------
// generic tile GEMM: 64 weight rows x 128 activation columns per workgroup, BK = 8 k-groups.
// ------------------------------------------------------------------------------------------
template <typename T>
struct GemmCfg {
    static constexpr int G = Frag<T>::G;
    static constexpr int BR = 64, BC = 128;
    static constexpr int KG = 8;                        // k-groups per tile (2 k-steps)
    static constexpr int BK = KG * G;
    static constexpr int LD = BK + G;                   // padded LDS row stride (9 groups: odd)
    static constexpr size_t lds_bytes = sizeof(T) * (size_t)(BR + BC) * LD;
};

template <typename T, bool W_IS_A>
__device__ __forceinline__ void gemm_tile_compute(const T* Ws, const T* Xs, f32x4 (&acc)[4][2], int wave, int l15, int lq) {
    typedef GemmCfg<T> Gc;
#pragma unroll
    for (int ks = 0; ks < Gc::KG / 4; ++ks) {
        typename Frag<T>::type wf[4], xf[2];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) wf[mi] = lds_frag<T>(Ws + (mi * 16 + l15) * Gc::LD + (ks * 4 + lq) * Gc::G);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) xf[ni] = lds_frag<T>(Xs + (wave * 32 + ni * 16 + l15) * Gc::LD + (ks * 4 + lq) * Gc::G);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                if (W_IS_A) mma_step(acc[mi][ni], wf[mi], xf[ni]);
                else mma_step(acc[mi][ni], xf[ni], wf[mi]);
            }
    }
}

template <typename T>
__device__ __forceinline__ void stage_weights(T* Ws, const T* __restrict__ Wp, int row0, int k0, int Kp, int tid) {
    typedef GemmCfg<T> Gc;
    for (int it = tid; it < Gc::BR * Gc::KG; it += kThreads) {
        const int r = it / Gc::KG, g = it % Gc::KG;
        *reinterpret_cast<vec16*>(Ws + r * Gc::LD + g * Gc::G) =
            *reinterpret_cast<const vec16*>(Wp + (int64_t)(row0 + r) * Kp + k0 + g * Gc::G);
    }
}

enum { PIX_DS = 0, PIX_US = 1 };

// ds: X [B,2T',2F',C] -> Y [B,T',F',M], K = 4C;  us: X [B,T',F',K] -> Y [B,2T',2F',C2] * skip, M = 4*C2.
template <typename T, int MODE>
__global__ void __launch_bounds__(kThreads)
pix_gemm_kernel(const T* __restrict__ X, T* __restrict__ Y, const T* __restrict__ Wp,
                const float* __restrict__ scale, const float* __restrict__ shift, const T* __restrict__ skip,
                int M, int K, int Kp, int64_t ncols, int Tp, int Fp, int C, int C2) {
    typedef GemmCfg<T> Gc;
    constexpr int G = Gc::G;
    T* Ws = reinterpret_cast<T*>(alsep_smem);
    T* Xs = Ws + Gc::BR * Gc::LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int64_t col0 = (int64_t)blockIdx.x * Gc::BC;
    const int row0 = blockIdx.y * Gc::BR;

    // this thread stages k-group (tid % 8) of columns tid/8 + 32*j, j < 4
    int64_t cbase[4];
    bool cvalid[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t col = col0 + tid / Gc::KG + 32 * j;
        cvalid[j] = col < ncols;
        if (MODE == PIX_DS) {
            const int64_t fp = col % Fp, tp = (col / Fp) % Tp, bb = col / ((int64_t)Fp * Tp);
            cbase[j] = ((bb * 2 * Tp + 2 * tp) * (2 * (int64_t)Fp) + 2 * fp) * C;
        } else {
            cbase[j] = col * K;
        }
    }
    f32x4 acc[4][2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < Kp; k0 += Gc::BK) {
        __syncthreads();
        stage_weights<T>(Ws, Wp, row0, k0, Kp, tid);
        const int k = k0 + (tid % Gc::KG) * G;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            vec16 v = zero16();
            if (cvalid[j] && k < K) {
                int64_t off = k;
                if (MODE == PIX_DS) {                        // two contiguous runs of 2C (dy = 0, 1)
                    const int seg = 2 * C;
                    off = (int64_t)(k / seg) * (2 * (int64_t)Fp * C) + (k % seg);
                }
                v = *reinterpret_cast<const vec16*>(X + cbase[j] + off);
            }
            *reinterpret_cast<vec16*>(Xs + (tid / Gc::KG + 32 * j) * Gc::LD + (tid % Gc::KG) * G) = v;
        }
        __syncthreads();
        gemm_tile_compute<T, true>(Ws, Xs, acc, wave, l15, lq);
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int64_t col = col0 + wave * 32 + ni * 16 + l15;
        if (col >= ncols) continue;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int row = row0 + mi * 16 + 4 * lq;
            if (row >= M) continue;
            float y[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[mi][ni][r], scale[row + r], shift[row + r]), 0.f);
            if (MODE == PIX_DS) {
                store4(Y + col * M + row, y);
            } else {
                const int d = row / C2, co = row % C2;
                const int64_t fp = col % Fp, tp = (col / Fp) % Tp, bb = col / ((int64_t)Fp * Tp);
                const int64_t o = ((bb * 2 * Tp + 2 * tp + (d >> 1)) * (2 * (int64_t)Fp) + 2 * fp + (d & 1)) * C2 + co;
                float s[4];
                load4(skip + o, s);
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] *= s[r];
                store4(Y + o, y);
            }
        }
    }
}

// TDF linear over the F axis: Y[bt][f'][c] = act(scale[c]*(sum_f W[f'][f] X[bt][f][c] + bias[f']) + shift[c]) (+ R)
// columns are "units" of 16 channels of one (b,t): unit u -> bt = u / (C/16), c0 = 16*(u % (C/16)).
template <typename T, bool RESIDUAL>
__global__ void __launch_bounds__(kThreads)
tdf_gemm_kernel(const T* __restrict__ X, T* __restrict__ Y, const T* __restrict__ Wp,
                const float* __restrict__ bias, const float* __restrict__ scale, const float* __restrict__ shift,
                const T* __restrict__ R, int M, int K, int Kp, int64_t nunits, int C) {
    typedef GemmCfg<T> Gc;
    constexpr int G = Gc::G;
    constexpr int CGU = 16 / G;                              // 16-byte groups per unit row
    T* Ws = reinterpret_cast<T*>(alsep_smem);
    T* Xs = Ws + Gc::BR * Gc::LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * 8;
    const int row0 = blockIdx.y * Gc::BR;
    const int upc = C / 16;

    // staging item (kk, ul, cgi): cgi fastest, then unit, then k -> coalesced channel runs
    const int cgi = tid % CGU, ul = (tid / CGU) % 8, kk0 = tid / (CGU * 8);
    constexpr int KSTEP = kThreads / (CGU * 8);              // k rows covered per pass
    const int64_t u = u0 + ul;
    const bool uvalid = u < nunits;
    const int64_t xbase = uvalid ? ((u / upc) * (int64_t)K) * C + (u % upc) * 16 + cgi * G : 0;

    f32x4 acc[4][2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < Kp; k0 += Gc::BK) {
        __syncthreads();
        stage_weights<T>(Ws, Wp, row0, k0, Kp, tid);
#pragma unroll
        for (int j = 0; j < Gc::BK / KSTEP; ++j) {
            const int kk = kk0 + j * KSTEP;
            vec16 v = zero16();
            if (uvalid && k0 + kk < K) v = *reinterpret_cast<const vec16*>(X + xbase + (int64_t)(k0 + kk) * C);
            const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
            for (int i = 0; i < G; ++i) Xs[(ul * 16 + cgi * G + i) * Gc::LD + kk] = e[i];   // transpose
        }
        __syncthreads();
        gemm_tile_compute<T, false>(Ws, Xs, acc, wave, l15, lq);
    }
    // D rows = channel within unit (4*lq + r), D cols = weight row f' (l15)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int64_t uu = u0 + wave * 2 + ni;
        if (uu >= nunits) continue;
        const int64_t bt = uu / upc;
        const int c = (int)(uu % upc) * 16 + 4 * lq;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int fo = row0 + mi * 16 + l15;
            if (fo >= M) continue;
            const float bv = bias ? bias[fo] : 0.f;
            const int64_t o = (bt * M + fo) * C + c;
            float y[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[mi][ni][r] + bv, scale[c + r], shift[c + r]), 0.f);
            if (RESIDUAL) {
                float x[4];
                load4(R + o, x);
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] += x[r];
            }
            store4(Y + o, y);
        }
    }
}

// ------------------------------------------------------------------------------------------
// bf16 TDF linear, main path (C multiple of 48):  Y[bt][f'][c] = act(...sum_f W[f'][f] X[bt][f][c])
// Workgroup tile: 128 weight rows (f') x 4 column units (a unit = 48 channels of one (b,t));
// wave w owns unit w.  Activations are the MFMA A operand (D rows = channels, so a lane ends up
// with 4 consecutive channels = one 8-byte store); their k axis (f) is strided in memory, so the
// tile is copied as it lies -- [64 f][48 c], 6 KiB per unit, by LDS-DMA -- and fragments are
// gathered with ds_read_b64_tr_b16 (hardware transpose read).  Each lane quarter lq takes
// k rows {4lq..4lq+3} and {16+4lq..16+4lq+3} of a 32-wide k-step: eight consecutive 96-byte
// rows per 32-lane half, which is bank-conflict free; the weight image is packed in the same
// k order, row-swizzled like the conv weights, and read with ds_read_b128.
// ------------------------------------------------------------------------------------------
struct TdfB16 {
    static constexpr int BM = 128, UN = 4, UC = 48, BK = 64;
    static constexpr int SS = 52;                              // epilogue row stride (floats): conflict-free accumulator writes, as TdfWide::SS
    static constexpr int WGROUPS = BM * (BK / 8);              // 1024
    static constexpr int XGROUPS = BK * (UC / 8);              // 384 per unit
    static constexpr int STAGE_ELEMS = 8 * (WGROUPS + UN * XGROUPS);             // one stage: W tile + 4 unit tiles
    static constexpr size_t lds_bytes = 2 * sizeof(bf16_t) * (size_t)STAGE_ELEMS;  // two stages: 80 KiB (the epilogue image, 4 x 64 x SS floats, aliases them)
    static_assert(4 * 64 * SS * sizeof(float) <= lds_bytes, "epilogue image fits the ring");
};

template <bool RESIDUAL>
__global__ void __launch_bounds__(kThreads, 2)
tdf_bf16_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wp,
                const float* __restrict__ bias, const float* __restrict__ scale, const float* __restrict__ shift,
                const bf16_t* __restrict__ R, const bf16_t* __restrict__ zero_page, int M, int K, int Kp,
                int64_t nunits, int C) {
    typedef TdfB16 Tc;
    bf16_t* Ws = reinterpret_cast<bf16_t*>(alsep_smem);
    bf16_t* Xs = Ws + (size_t)Tc::WGROUPS * 8 + (size_t)(threadIdx.x >> 6) * Tc::XGROUPS * 8;   // this wave's unit
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int row0 = blockIdx.y * Tc::BM;
    const int upc = C / Tc::UC;
    const int64_t u = (int64_t)blockIdx.x * Tc::UN + wave;
    const bool uvalid = u < nunits;
    const int64_t bt = uvalid ? u / upc : 0;
    const int cb = uvalid ? (int)(u % upc) * Tc::UC : 0;
    const bf16_t* xu = X + (bt * K) * (int64_t)C + cb;
    const int klim = uvalid ? K : 0;

    f32x4 acc[3][8];
#pragma unroll
    for (int ni = 0; ni < 3; ++ni)
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

    // transpose-read addressing inside the unit tile [64 k][48 c]: lane j of a 16-lane group
    // supplies row (j>>2), columns 4*(j&3)..+3 of the 4 x 16 block
    const int trow = l15 >> 2, tcol = (l15 & 3) * 4;
    const int wswz = l15 >> 1;

    // Two-stage LDS ring over the K tiles: the LDS-DMA of tile it+1 is issued before tile it is
    // consumed and stays in flight across the barriers (counted vmcnt + raw s_barrier; a
    // __syncthreads() here would drain vmcnt(0), cdna_hip_programming.md "Pipelining across barriers").
    // Every wave issues exactly GLDS_PER_TILE LDS-DMA instructions per tile and nothing else that
    // counts on vmcnt inside the loop.
    constexpr int GLDS_PER_TILE = Tc::WGROUPS / 64 / 4 + Tc::XGROUPS / 64;      // 4 + 6
    const int ntile = Kp / Tc::BK;
    // the stage index is a compile-time constant in every access (loop unrolled by two): with a
    // run-time stage offset hipcc cannot tell the stage being read from the one in flight and
    // puts s_waitcnt vmcnt(0) in front of the first ds_read
    auto issue = [&](int it, int stage) {
        const int k0 = it * Tc::BK;
        bf16_t* wdst = Ws + (size_t)stage * Tc::STAGE_ELEMS;
        bf16_t* xdst = Xs + (size_t)stage * Tc::STAGE_ELEMS;
#pragma unroll
        for (int j = 0; j < Tc::WGROUPS / 64 / 4; ++j) {
            const int i = wave + 4 * j;
            const int gidx = i * 64 + lane;
            glds16(Wp + (int64_t)(row0 + (gidx >> 3)) * Kp + k0 + (gidx & 7) * 8, wdst + (size_t)i * 64 * 8);
        }
#pragma unroll
        for (int i = 0; i < Tc::XGROUPS / 64; ++i) {
            const int gidx = i * 64 + lane;
            const int kk = gidx / 6, g = gidx % 6;
            // one per-lane select, no wave-uniform branch: every wave issues every LDS-DMA (klim = 0 for a
            // wave without a unit), which is what the counted waits below rely on
            const bf16_t* src = (k0 + kk < klim) ? xu + (int64_t)(k0 + kk) * C + g * 8 : zero_page;
            glds16(src, xdst + (size_t)i * 64 * 8);
        }
    };
    auto compute = [&](int stage) {
        const bf16_t* Wc = Ws + (size_t)stage * Tc::STAGE_ELEMS;
        const bf16_t* Xc = Xs + (size_t)stage * Tc::STAGE_ELEMS;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 xf[3], wf[8];
#pragma unroll
            for (int ni = 0; ni < 3; ++ni) {
                const bf16_t* p0 = Xc + (ks * 32 + 4 * lq + trow) * Tc::UC + ni * 16 + tcol;
                const bf16x4 lo = lds_read_tr16_b64(p0);
                const bf16x4 hi = lds_read_tr16_b64(p0 + 16 * Tc::UC);
                xf[ni] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int mi = 0; mi < 8; ++mi) wf[mi] = lds_frag<bf16_t>(Wc + ((mi * 16 + l15) * 8 + ((ks * 4 + lq) ^ wswz)) * 8);
            lds_read_tr16_wait();
#pragma unroll
            for (int ni = 0; ni < 3; ++ni)
#pragma unroll
                for (int mi = 0; mi < 8; ++mi) mma_step(acc[ni][mi], xf[ni], wf[mi]);
        }
    };
    // step(it, S): tile it sits in stage S; prefetch tile it+1 into stage 1-S, consume, release
#define ALSEP_TDF_STEP(it_, S_)                                                                   \
    do {                                                                                          \
        if ((it_) + 1 < ntile) {                                                                  \
            issue((it_) + 1, 1 - (S_));                                                           \
            wait_vmcnt<GLDS_PER_TILE>();          /* this wave's tile it_ has landed */           \
        } else {                                                                                  \
            wait_vmcnt<0>();                                                                      \
        }                                                                                         \
        barrier_nodrain();                        /* ... and every other wave's */                \
        compute(S_);                                                                              \
        barrier_nodrain();                        /* stage S_ is free for tile it_+2 */           \
    } while (0)
    issue(0, 0);
    for (int it = 0; it < ntile; it += 2) {
        ALSEP_TDF_STEP(it, 0);
        if (it + 1 < ntile) ALSEP_TDF_STEP(it + 1, 1);
    }
#undef ALSEP_TDF_STEP
    // Epilogue through LDS: a lane's accumulator fragment is 4 channels of one f' row (8 bytes,
    // 16 different rows per store instruction); re-laid out as [f'][48 c] in this wave's private
    // 12 KiB of LDS it leaves as whole 96-byte rows -- 16-byte loads of the residual and 16-byte
    // stores, contiguous across lanes (a full 6 KiB run when C = 48).  fp32 staging, two halves of
    // 64 rows, so the residual add and the single bf16 rounding stay exactly as before.
    // (all waves are past the last barrier of the k loop: the stage buffers are free; the region is
    // private to the wave, so only its own LDS operations need ordering)
    float* stg = reinterpret_cast<float*>(alsep_smem) + (size_t)wave * (64 * Tc::SS);
    float bvv[8];
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
        const int fo = row0 + mi * 16 + l15;
        bvv[mi] = (bias && fo < M) ? bias[fo] : 0.f;
    }
    float sc[3][4], sh[3][4];
#pragma unroll
    for (int ni = 0; ni < 3; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sc[ni][r] = uvalid ? scale[cb + ni * 16 + 4 * lq + r] : 0.f;
            sh[ni][r] = uvalid ? shift[cb + ni * 16 + 4 * lq + r] : 0.f;
        }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int ni = 0; ni < 3; ++ni)
#pragma unroll
            for (int m4 = 0; m4 < 4; ++m4) {
                const int mi = half * 4 + m4;
                float4 v;
                v.x = fmaxf(fmaf(acc[ni][mi][0] + bvv[mi], sc[ni][0], sh[ni][0]), 0.f);
                v.y = fmaxf(fmaf(acc[ni][mi][1] + bvv[mi], sc[ni][1], sh[ni][1]), 0.f);
                v.z = fmaxf(fmaf(acc[ni][mi][2] + bvv[mi], sc[ni][2], sh[ni][2]), 0.f);
                v.w = fmaxf(fmaf(acc[ni][mi][3] + bvv[mi], sc[ni][3], sh[ni][3]), 0.f);
                *reinterpret_cast<float4*>(stg + (m4 * 16 + l15) * Tc::SS + ni * 16 + 4 * lq) = v;
            }
        __builtin_amdgcn_wave_barrier();                    // wave-private region: program order suffices on hardware
        // rows [half*64, half*64+64) x 6 groups of 8 channels = 384 16-byte output groups
#pragma unroll
        for (int it = 0; it < 6; ++it) {
            const int gidx = it * 64 + lane;
            const int fr = gidx / 6, cg = gidx % 6;
            const int fo = row0 + half * 64 + fr;
            const float4 lo = *reinterpret_cast<const float4*>(stg + fr * Tc::SS + cg * 8);
            const float4 hi = *reinterpret_cast<const float4*>(stg + fr * Tc::SS + cg * 8 + 4);
            if (uvalid && fo < M) {
                const int64_t o = (bt * M + fo) * (int64_t)C + cb + cg * 8;
                float y[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                if (RESIDUAL) {
                    const bf16x8 xr = *reinterpret_cast<const bf16x8*>(R + o);
#pragma unroll
                    for (int e = 0; e < 8; ++e) y[e] += (float)xr[e];
                }
                bf16x8 q;
#pragma unroll
                for (int e = 0; e < 8; ++e) q[e] = (bf16_t)y[e];
                stream_store(reinterpret_cast<bf16x8*>(Y + o), q);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------
// bf16 TDF linear, wide-tile path (C multiple of 48, M multiple of 192): same math and k order as
// tdf_bf16_kernel, different traffic.  Workgroup tile: 48*WM weight rows x 4 column units; wave w owns
// weight rows [48w, 48w+48) of the tile and ALL four units (acc 4 x 3 x 3 fragments = 144 VGPRs).
//   * the weight tile never goes through LDS: every wave needs a different 48-row slice, so it loads its
//     fragments straight from the fragment-order image (make_tdf_frag_weights: 3 KiB contiguous per
//     wave and 32-wide k-step) into registers one K tile ahead -- LDS-DMA traffic per flop drops 2.5x
//     against the 128-row kernel and the L2 -> CU traffic by a third;
//   * only activations are staged: [4 units][64 f][48 c] = 24 KiB per K tile, three-stage ring, the
//     LDS-DMA of tile it+2 issued while tile it is consumed (one raw barrier per tile, counted vmcnt;
//     issue order W(it+1), X(it+2) so that waiting for W(it) never waits for the youngest X tile);
//   * WM = 4: 256 threads, 72 KiB -> 2 workgroups per CU, one in its epilogue while the other computes
//     (second linear: output + residual traffic dominates); WM = 8: 512 threads, 384 rows -- the whole
//     first linear of level 0 in one row block, so X is read from HBM exactly once.
// ------------------------------------------------------------------------------------------
template <int WM>
struct TdfWide {
    static constexpr int TR = 48, BM = TR * WM, UN = 4, UC = 48, BK = 64, NST = 3;
    static constexpr int THREADS = 64 * WM;
    static constexpr int UNIT_ELEMS = BK * UC;                       // 3072 bf16 = 6 KiB
    static constexpr int STAGE_ELEMS = UN * UNIT_ELEMS;              // 24 KiB
    static constexpr int PIECES = STAGE_ELEMS / 8 / 64;              // 24 wave-instructions of 1 KiB per stage
    static constexpr int GLDS = PIECES / WM;                         // per wave and tile: 6 (WM = 4) / 3 (WM = 8)
    static constexpr int WLOADS = 6;                                 // weight fragments per wave and tile
    static constexpr size_t ring_bytes = (size_t)NST * STAGE_ELEMS * sizeof(bf16_t);
    static constexpr int SS = 52;                                     // epilogue row stride in floats: 48 + 4 makes the ds_write_b128 of the
                                                                      // accumulator fragments conflict-free (stride 48: 4-way; SQ_LDS_BANK_CONFLICT was 44 % of the LDS cycles)
    static constexpr size_t stage_bytes = (size_t)WM * TR * SS * sizeof(float);    // epilogue: one unit per wave, fp32
    static constexpr size_t lds_bytes = ring_bytes > stage_bytes ? ring_bytes : stage_bytes;
    static_assert(PIECES % WM == 0 && 6 % GLDS == 0, "a wave's LDS-DMA pieces stay inside one unit");
    // FINAL epilogue: the rounded rows of one unit per wave, [48 f'][48 c] in the storage type, behind the fp32 staging rows.
    // Row stride 56 elements = 7 16-byte slots (odd): the sixteen lanes of a ds_read_b128 group, one row each, hit distinct slots.
    static constexpr int FS = 56;
    static constexpr size_t final_bytes = (size_t)WM * TR * FS * sizeof(bf16_t);
    static constexpr int FWN = 192;                                  // floats per wave behind those: the final conv's W [4][48]
};

// A-operand fragments of one unit and k-step: byte offset OFF from the lane's base inside the stage
template <int OFF>
__device__ __forceinline__ bf16x8 tdfw_read_frag(const bf16_t* base) {
    const bf16x4 lo = lds_read_tr16_b64_off<OFF>(base);
    const bf16x4 hi = lds_read_tr16_b64_off<OFF + 16 * 48 * 2>(base);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
template <int KS, int U>
__device__ __forceinline__ void tdfw_read_x(bf16x8 (&xf)[3], const bf16_t* base) {
    constexpr int OFF = (U * 64 * 48 + KS * 32 * 48) * 2;
    xf[0] = tdfw_read_frag<OFF>(base);
    xf[1] = tdfw_read_frag<OFF + 32>(base);
    xf[2] = tdfw_read_frag<OFF + 64>(base);
}

// FINAL (last block of the network, C == 48 so that a unit is one frame with all its channels): the rounded output rows are
// not stored; they stay in this wave's LDS, where each of the 48 pixels (one f' row) is reduced over its 48 channels exactly
// as final_conv_kernel does it -- y[r] = bias[r], fmaf over ci ascending, one float32 chain per (pixel, r), then * alpha --
// and leaves as a [B, T, F, 4] record: the 48-channel activation never reaches memory.  Y is not touched.  FW [4][48], FB [4]
// (float32), FOUT and falpha are the final convolution's.  Each wave copies W into LDS once (three floats per lane, requested
// ahead of the residual rows) and the chains read it back as broadcast ds_read_b128: read from memory inside the unit loop the
// weights cost a dozen dependent round trips per unit (vector loads under the lane predicate, or scalar loads that the SGPR
// budget serialises), which made the folded launch 0.74 ms slower than the store it replaces.
template <int WM, bool RESIDUAL, int RPF = 2, bool FINAL = false>   // RPF: units of residual rows requested ahead of the stores
__global__ void __launch_bounds__(64 * WM, 2)
tdf_bf16_wide_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wf,
                     const float* __restrict__ bias, const float* __restrict__ scale, const float* __restrict__ shift,
                     const bf16_t* __restrict__ R, int M, int K, int64_t nunits, int C, int nyb,
                     const float* __restrict__ FW, const float* __restrict__ FB, bf16_t* __restrict__ FOUT, float falpha) {
    typedef TdfWide<WM> Tc;
    static_assert(!FINAL || (RESIDUAL && Tc::stage_bytes + Tc::final_bytes + WM * Tc::FWN * sizeof(float) <= Tc::lds_bytes),
                  "FINAL: rounded rows and the final weights behind the staging rows");
    bf16_t* ring = reinterpret_cast<bf16_t*>(alsep_smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // scalar: row block, DMA duty and their bases live in SGPRs
    const int l15 = lane & 15, lq = lane >> 4;
    // nyb > 0 (1-D grid, column tiles % 8 == 0): the nyb row blocks that read the same four units are dispatched back to
    // back onto one XCD (ids b, b+8, ... share an L2), so the activations come from HBM once instead of once per row
    // block -- with row blocks on blockIdx.y they are re-streamed M/BM times, a whole grid.x apart
    int bx = blockIdx.x, by = blockIdx.y;
    if (nyb > 0) {
        const int i = (int)blockIdx.x >> 3;
        by = i % nyb;
        bx = (i / nyb) * 8 + ((int)blockIdx.x & 7);
    }
    const int rowblk = by * WM + wave;                               // 48-row block of the weight matrix
    const int upc = C / Tc::UC;
    const int64_t u0 = (int64_t)bx * Tc::UN;
    const int ntile = K / Tc::BK;
    if (ntile <= 0) return;                                          // (the launcher never does this; removes the zero-trip path)

    // LDS-DMA duty of this wave: GLDS consecutive 1-KiB pieces of one unit's [64 f][48 c] tile.  The launcher
    // guarantees K % 64 == 0 and nunits % 4 == 0, so there is no padding select.  Three pieces are exactly 32
    // rows of 96 bytes: piece p reads (p / 3) * 32 rows below piece p % 3, so three 32-bit lane offsets and a
    // scalar base (SGPR pair, advanced per tile) address everything -- nothing here is worth a 64-bit VGPR.
    const int du = (wave * Tc::GLDS) / 6, dp0 = (wave * Tc::GLDS) % 6;
    const int64_t dU = u0 + du;
    const char* xu = reinterpret_cast<const char*>(X + ((dU / upc) * K) * (int64_t)C + (int)(dU % upc) * Tc::UC) +
                     (size_t)(dp0 / 3) * 32 * C * sizeof(bf16_t);
    unsigned xoff[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int within = j * 64 + lane;
        xoff[j] = (unsigned)(((within / 6) * C + (within % 6) * 8) * (int)sizeof(bf16_t));
    }
    auto issue_x = [&](int it, int stage) {
        bf16_t* dst = ring + (size_t)stage * Tc::STAGE_ELEMS + (size_t)du * Tc::UNIT_ELEMS + (size_t)dp0 * 64 * 8;
        const char* xk = opaque_uniform_ptr(xu + (size_t)it * (Tc::BK * sizeof(bf16_t)) * C);
#pragma unroll
        for (int j = 0; j < Tc::GLDS; ++j)
            glds16(xk + (size_t)(j / 3) * 32 * C * sizeof(bf16_t) + xoff[j % 3], dst + (size_t)j * 64 * 8);
    };
    const char* wrow = reinterpret_cast<const char*>(Wf) + (size_t)rowblk * ntile * (Tc::WLOADS * 1024);
    const unsigned woff = (unsigned)lane * 16u;
    bf16x8 wf[2][2][3];                                              // [tile parity][k-step][m-tile]
    auto issue_w = [&](int it, int par) {
        const char* wp = opaque_uniform_ptr(wrow + (size_t)it * (Tc::WLOADS * 1024));
        const char* wq = wp + 4096;
        global_load_async_bf16x8<0>(wf[par][0][0], wp, woff);
        global_load_async_bf16x8<1024>(wf[par][0][1], wp, woff);
        global_load_async_bf16x8<2048>(wf[par][0][2], wp, woff);
        global_load_async_bf16x8<3072>(wf[par][1][0], wp, woff);
        global_load_async_bf16x8<0>(wf[par][1][1], wq, woff);
        global_load_async_bf16x8<1024>(wf[par][1][2], wq, woff);
    };

    f32x4 acc[Tc::UN][3][3];
#pragma unroll
    for (int u = 0; u < Tc::UN; ++u)
#pragma unroll
        for (int ni = 0; ni < 3; ++ni)
#pragma unroll
            for (int mi = 0; mi < 3; ++mi) acc[u][ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int trow = l15 >> 2, tcol = (l15 & 3) * 4;
    const bf16_t* xlane = ring + (4 * lq + trow) * Tc::UC + tcol;
    auto mma_unit = [&](int u, const bf16x8 (&xf)[3], int par, int ks) {
#pragma unroll
        for (int ni = 0; ni < 3; ++ni)
#pragma unroll
            for (int mi = 0; mi < 3; ++mi) mma_step(acc[u][ni][mi], xf[ni], wf[par][ks][mi]);
    };
    // tile it sits in stage S_ (= it % 3), its weights in wf[P_] (P_ = it % 2); all indices compile-time
#define ALSEP_TDFW_STEP(it_, S_, P_)                                                              \
    do {                                                                                          \
        wait_vmcnt<Tc::GLDS>();            /* all but X(it+1): W(it) and X(it) have landed */     \
        if ((it_) + 1 >= ntile) wait_vmcnt<0>();         /* last tile: nothing was issued behind */ \
        barrier_nodrain();                 /* every wave's part of X(it); compute(it-1) finished */ \
        if ((it_) + 1 < ntile) issue_w((it_) + 1, 1 - (P_));                                     \
        if ((it_) + 2 < ntile) issue_x((it_) + 2, ((S_) + 2) % 3);                               \
        const bf16_t* xs_ = xlane + (size_t)(S_) * Tc::STAGE_ELEMS;                               \
        bf16x8 xa[3], xb[3];                                                                      \
        tdfw_read_x<0, 0>(xa, xs_);                                                               \
        tdfw_read_x<0, 1>(xb, xs_);                                                               \
        lds_read_tr16_wait_n<6>();  mma_unit(0, xa, P_, 0);                                       \
        tdfw_read_x<0, 2>(xa, xs_);                                                               \
        lds_read_tr16_wait_n<6>();  mma_unit(1, xb, P_, 0);                                       \
        tdfw_read_x<0, 3>(xb, xs_);                                                               \
        lds_read_tr16_wait_n<6>();  mma_unit(2, xa, P_, 0);                                       \
        tdfw_read_x<1, 0>(xa, xs_);                                                               \
        lds_read_tr16_wait_n<6>();  mma_unit(3, xb, P_, 0);                                       \
        tdfw_read_x<1, 1>(xb, xs_);                                                               \
        lds_read_tr16_wait_n<6>();  mma_unit(0, xa, P_, 1);                                       \
        tdfw_read_x<1, 2>(xa, xs_);                                                               \
        lds_read_tr16_wait_n<6>();  mma_unit(1, xb, P_, 1);                                       \
        tdfw_read_x<1, 3>(xb, xs_);                                                               \
        lds_read_tr16_wait_n<6>();  mma_unit(2, xa, P_, 1);                                       \
        lds_read_tr16_wait_n<0>();  mma_unit(3, xb, P_, 1);                                       \
    } while (0)
    issue_x(0, 0);
    issue_w(0, 0);
    if (1 < ntile) issue_x(1, 1);
    for (int it = 0; it < ntile; it += 6) {
        ALSEP_TDFW_STEP(it, 0, 0);
        if (it + 1 < ntile) ALSEP_TDFW_STEP(it + 1, 1, 1);
        if (it + 2 < ntile) ALSEP_TDFW_STEP(it + 2, 2, 0);
        if (it + 3 < ntile) ALSEP_TDFW_STEP(it + 3, 0, 1);
        if (it + 4 < ntile) ALSEP_TDFW_STEP(it + 4, 1, 0);
        if (it + 5 < ntile) ALSEP_TDFW_STEP(it + 5, 2, 1);
    }
#undef ALSEP_TDFW_STEP
    wait_vmcnt<0>();                                     // already true; states it on every path for check_async_regs.py
    // keep the fragment registers live up to here: the epilogue's first values must not be allocated to (and
    // scheduled above the wait into) registers that, as far as the control-flow graph can tell, may be in flight
#pragma unroll
    for (int i = 0; i < 12; ++i) keep_vgprs_live(wf[i / 6][(i / 3) % 2][i % 3]);
    barrier_nodrain();                                   // the ring is free: every wave is past its last read

    // Epilogue, one unit at a time through this wave's private 9 KiB of LDS (fp32 [48 f'][48 c]): the
    // accumulator fragment of a lane is 4 channels of one f' row; re-laid out it leaves as whole
    // 96-byte rows (16-byte residual loads and stores).  Arithmetic as in tdf_bf16_kernel: bias, BN,
    // ReLU and the residual add in fp32, one rounding to bf16.
    float* stg = reinterpret_cast<float*>(alsep_smem) + (size_t)wave * (Tc::TR * Tc::SS);
    bf16_t* frow = reinterpret_cast<bf16_t*>(alsep_smem + Tc::stage_bytes) + (size_t)wave * (Tc::TR * Tc::FS);   // FINAL only
    float* fwl = reinterpret_cast<float*>(alsep_smem + Tc::stage_bytes + Tc::final_bytes) + wave * Tc::FWN;                // FINAL only
    float fw[3], fbs[4];
    if (FINAL) {                                                    // requested first: the wait for them leaves the residual rows in flight
#pragma unroll
        for (int j = 0; j < 3; ++j) fw[j] = FW[j * 64 + lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) fbs[r] = FB[r];                 // uniform, ahead of every store: scalar loads
    }
    float bvv[3];
#pragma unroll
    for (int mi = 0; mi < 3; ++mi) bvv[mi] = bias ? bias[rowblk * Tc::TR + mi * 16 + l15] : 0.f;
    // 48 rows x 6 groups of 8 channels = 288 16-byte output groups per unit, 5 per lane (the last one half-filled)
    // unit u: wave-uniform base (SGPR pair) + five 32-bit lane offsets shared by every unit and by R and Y
    auto unit_base = [&](int u) {
        const int64_t U = u0 + u;
        return ((U / upc) * M + rowblk * Tc::TR) * (int64_t)C + (int)(U % upc) * Tc::UC;
    };
    unsigned loff[5];
#pragma unroll
    for (int it = 0; it < 5; ++it) {
        const int gidx = it * 64 + lane;
        loff[it] = (unsigned)(((gidx / 6) * C + (gidx % 6) * 8) * (int)sizeof(bf16_t));
    }
    // The residual rows are the only HBM reads of the epilogue and nothing else hides their latency (two waves per SIMD):
    // unit u+PF's rows are requested before unit u is written, instead of one dependent load -> add -> store chain per unit.
    constexpr int PF = RESIDUAL ? RPF : 0;
    bf16x8 rr[Tc::UN][5];
    auto load_res = [&](int u) {
        const ALSEP_GLOBAL char* rb = opaque_uniform_gptr(reinterpret_cast<const char*>(R + unit_base(u)));   // global_load, counted vmcnt
#pragma unroll
        for (int it = 0; it < 5; ++it)
            if (it * 64 + lane < Tc::TR * 6) rr[u][it] = *reinterpret_cast<const ALSEP_GLOBAL bf16x8*>(rb + loff[it]);
    };
    if (RESIDUAL) {
#pragma unroll
        for (int u = 0; u < PF && u < Tc::UN; ++u) {
            load_res(u);
            if (FINAL && u == 0) {                                  // here, not later: three registers less while two units of rows are in flight
#pragma unroll
                for (int j = 0; j < 3; ++j) fwl[j * 64 + lane] = fw[j];     // read after the first unit's wave barrier
            }
        }
    }
#pragma unroll
    for (int u = 0; u < Tc::UN; ++u) {
        const int cb = (int)((u0 + u) % upc) * Tc::UC;
        if (RESIDUAL && u + PF < Tc::UN) load_res(u + PF);
        ALSEP_GLOBAL char* yb = const_cast<ALSEP_GLOBAL char*>(opaque_uniform_gptr(reinterpret_cast<const char*>(Y + unit_base(u))));
#pragma unroll
        for (int ni = 0; ni < 3; ++ni) {
            const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + cb + ni * 16 + 4 * lq);
            const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + cb + ni * 16 + 4 * lq);
#pragma unroll
            for (int mi = 0; mi < 3; ++mi) {
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(fmaf(acc[u][ni][mi][r] + bvv[mi], sc[r], sh[r]), 0.f);
                *reinterpret_cast<f32x4*>(stg + (mi * 16 + l15) * Tc::SS + ni * 16 + 4 * lq) = v;
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 5; ++it) {
            const int gidx = it * 64 + lane;
            const int fr = gidx / 6, cg = gidx % 6;
            if (gidx < Tc::TR * 6) {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(stg + fr * Tc::SS + cg * 8);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(stg + fr * Tc::SS + cg * 8 + 4);
                float y[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                if (RESIDUAL) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) y[e] += (float)rr[u][it][e];
                }
                bf16x8 q;
#pragma unroll
                for (int e = 0; e < 8; ++e) q[e] = (bf16_t)y[e];
                if (FINAL) *reinterpret_cast<bf16x8*>(frow + fr * Tc::FS + cg * 8) = q;
                else stream_store(reinterpret_cast<ALSEP_GLOBAL bf16x8*>(yb + loff[it]), q);
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (FINAL) {
            // lane = f' row = one pixel of frame u0 + u (C == 48: unit == frame); 48 lanes x 4 values = 384 contiguous bytes
            const int frl = lane < Tc::TR ? lane : Tc::TR - 1;
            float y[4] = {fbs[0], fbs[1], fbs[2], fbs[3]};
#pragma unroll 2                                             // whole: the W rows of six groups in flight spill (254 VGPRs without)
            for (int ci = 0; ci < Tc::UC; ci += 8) {
                const bf16x8 xv = *reinterpret_cast<const bf16x8*>(frow + frl * Tc::FS + ci);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const f32x4 w0 = *reinterpret_cast<const f32x4*>(fwl + r * Tc::UC + ci);
                    const f32x4 w1 = *reinterpret_cast<const f32x4*>(fwl + r * Tc::UC + ci + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[r] = fmaf(w0[e], (float)xv[e], y[r]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[r] = fmaf(w1[e], (float)xv[4 + e], y[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] *= falpha;
            if (lane < Tc::TR) store4(FOUT + (((u0 + u) * M + rowblk * Tc::TR + lane) << 2), y);
            __builtin_amdgcn_wave_barrier();                 // the next unit's rounded rows overwrite these
        }
    }
}

// ------------------------------------------------------------------------------------------
// Residual TDF linear of levels 0 and 1, persistent over the row blocks (C = 48 or 96, M multiple of 384, K = 64 NT): same
// math, k order and epilogue arithmetic as tdf_bf16_wide_kernel<4, true>, different traffic.  A work item is two consecutive
// units x ALL M rows; workgroups stride statically over the items (no atomics, no hand-off between workgroups).
//   * the item's hidden activations [NT][2 units][64 f][48 c] (72 KiB at K = 384) come into LDS ONCE by LDS-DMA and stay
//     there; the wide kernel streams them through its ring once per 192-row block, 16 times at level 0 -- L2 -> LDS traffic
//     as large as the launch's whole HBM traffic;
//   * after that fill the waves never meet again inside the item: wave w walks the 48-row blocks w, w + 8, ... on its own
//     (weights straight into registers two K tiles ahead, three buffers; K tiles are a multiple of three, so the buffer of a
//     tile is the same in every row block and the first two tiles of the next row block are requested under the last MFMAs
//     of this one), so one wave's epilogue runs beside another wave's MFMAs;
//   * the residual rows and the bias of a row block are requested behind the weight loads of its first K tile: their HBM
//     latency sits under that row block's MFMAs (acc 2 x 3 x 3 = 72 VGPRs leaves room for the 40 they take);
//   * BN scale / shift of the two units (the same for every item: C / 48 is 1 or 2) are read from LDS, not from memory;
//   * FINAL: as in the wide kernel; the rounded rows reuse the wave's fp32 staging rows (read whole, then overwritten).
// LDS: 72 KiB tile + 8 x 9.75 KiB staging + 0.75 KiB scale/shift (+ 6 KiB final weights) = 156.75 KiB: one workgroup of
// eight waves per CU, two waves per SIMD.
// ------------------------------------------------------------------------------------------
struct TdfPersist {
    static constexpr int WV = 8, TR = 48, BM = TR * WV, UN = 2, UC = 48, BK = 64;
    static constexpr int THREADS = 64 * WV;
    static constexpr int STAGE_ELEMS = UN * BK * UC;                 // one K tile of both units: 12 KiB
    static constexpr int SS = TdfWide<4>::SS, FS = TdfWide<4>::FS, FWN = TdfWide<4>::FWN;
    static constexpr size_t stage_bytes = (size_t)WV * TR * SS * sizeof(float);
    static constexpr size_t bn_bytes = (size_t)UN * 2 * UC * sizeof(float);
    static constexpr size_t tile_bytes(int nt) { return (size_t)nt * STAGE_ELEMS * sizeof(bf16_t); }
    static constexpr size_t lds_bytes(int nt, bool fin) { return tile_bytes(nt) + stage_bytes + bn_bytes + (fin ? WV * FWN * sizeof(float) : 0); }
    static_assert((size_t)TR * FS * sizeof(bf16_t) <= (size_t)TR * SS * sizeof(float), "FINAL: the rounded rows fit in the staging rows");
};

// glds16 with the source as wave-uniform global base + 32-bit lane offset (one address VGPR, no 64-bit lane pointer)
__device__ __forceinline__ void glds16_base(const ALSEP_GLOBAL char* gbase, unsigned lane_off, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const ALSEP_GLOBAL void*)(gbase + lane_off), (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <int NT, bool FINAL>
__global__ void __launch_bounds__(TdfPersist::THREADS, 1)
tdf_bf16_persist_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wf,
                        const float* __restrict__ bias, const float* __restrict__ scale, const float* __restrict__ shift,
                        const bf16_t* __restrict__ R, int M, int64_t nitems, int C,
                        const float* __restrict__ FW, const float* __restrict__ FB, bf16_t* __restrict__ FOUT, float falpha) {
    typedef TdfPersist Tc;
    static_assert(NT % 3 == 0 && NT >= 3, "three weight buffers: a K tile's buffer is the same in every row block");
    static_assert(Tc::lds_bytes(NT, FINAL) <= 160 * 1024, "LDS of a CU");
    constexpr int K = NT * Tc::BK;
    bf16_t* tile = reinterpret_cast<bf16_t*>(alsep_smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    float* stg = reinterpret_cast<float*>(alsep_smem + Tc::tile_bytes(NT)) + (size_t)wave * (Tc::TR * Tc::SS);
    bf16_t* frow = reinterpret_cast<bf16_t*>(stg);                   // FINAL only: over the staging rows, once they are read
    float* bnl = reinterpret_cast<float*>(alsep_smem + Tc::tile_bytes(NT) + Tc::stage_bytes);     // [unit][scale | shift][48]
    float* fwl = bnl + Tc::UN * 2 * Tc::UC + wave * Tc::FWN;         // FINAL only
    const int ush = C / Tc::UC - 1;                                  // units per frame 1 or 2 (launcher), as a shift: unit u of every item has
                                                                     // channel base (u & ush) * 48 and frame (u0 + u) >> ush
    const int nrb = M / Tc::BM;

    if (tid < Tc::UN * 2 * Tc::UC) {
        const int u = tid / (2 * Tc::UC), which = (tid / Tc::UC) & 1, c = tid % Tc::UC;
        bnl[tid] = (which ? shift : scale)[(u & ush) * Tc::UC + c];
    }
    float fbs[4];
    if (FINAL) {
#pragma unroll
        for (int j = 0; j < 3; ++j) fwl[j * 64 + lane] = FW[j * 64 + lane];     // wave-private, read after this wave's first wave barrier
#pragma unroll
        for (int r = 0; r < 4; ++r) fbs[r] = FB[r];
    }
    // 48 rows x 6 groups of 8 channels = 288 16-byte output groups per unit, 5 per lane (the last one half-filled)
    unsigned loff[5], xoff[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int within = j * 64 + lane;
        xoff[j] = (unsigned)(((within / 6) * C + (within % 6) * 8) * (int)sizeof(bf16_t));
    }
#pragma unroll
    for (int it = 0; it < 5; ++it) {
        const int gidx = it * 64 + lane;
        loff[it] = (unsigned)(((gidx / 6) * C + (gidx % 6) * 8) * (int)sizeof(bf16_t));
    }
    const unsigned woff = (unsigned)lane * 16u;
    const int trow = l15 >> 2, tcol = (l15 & 3) * 4;
    const bf16_t* xlane = tile + (4 * lq + trow) * Tc::UC + tcol;

    bf16x8 wf[3][2][3];                                              // [K tile % 3][k-step][m-tile]
    auto load_w = [&](int buf, int rowblk, int it) {                 // 6 KiB contiguous per wave and K tile (make_tdf_frag_weights)
        const ALSEP_GLOBAL char* wp = opaque_uniform_gptr(reinterpret_cast<const char*>(Wf) + ((size_t)rowblk * NT + it) * (6 * 1024));
#pragma unroll
        for (int i = 0; i < 6; ++i) wf[buf][i / 3][i % 3] = *reinterpret_cast<const ALSEP_GLOBAL bf16x8*>(wp + woff + i * 1024);
    };

    for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int64_t u0 = item * Tc::UN;
        load_w(0, wave, 0);
        load_w(1, wave, 1);
        barrier_nodrain();                                           // every wave has left the previous item's tile (first item: bnl is written)
        // fill: 12 NT pieces of 1 KiB, piece p = ((K tile * 2 + unit) * 6 + j) lands at p KiB; three pieces are 32 rows of 96 bytes
        constexpr int NP = NT * Tc::UN * 6;
#pragma unroll 1                                             // rolled: unrolled, the nine 64-bit lane addresses are hoisted out of the item loop and spill
        for (int p = wave; p < NP; p += Tc::WV) {
            {
                const int tu = p / 6, j = p % 6, it = tu / Tc::UN, u = tu % Tc::UN;
                const ALSEP_GLOBAL char* src = opaque_uniform_gptr(reinterpret_cast<const char*>(
                    X + (((u0 + u) >> ush) * K + it * Tc::BK + (j / 3) * 32) * (int64_t)C + (u & ush) * Tc::UC));
                const int j3 = j % 3;
                glds16_base(src, j3 == 0 ? xoff[0] : (j3 == 1 ? xoff[1] : xoff[2]), tile + (size_t)p * 64 * 8);
            }
        }
        wait_vmcnt<0>();
        barrier_nodrain();                                           // every wave's pieces have landed

        for (int rb = 0; rb < nrb; ++rb) {
            const int rowblk = rb * Tc::WV + wave;                   // 48-row block of the weight matrix
            const int rownext = (rb + 1 < nrb ? rb + 1 : rb) * Tc::WV + wave;      // last row block: a harmless reload instead of a branch
            auto unit_base = [&](int u) {
                return (((u0 + u) >> ush) * M + rowblk * Tc::TR) * (int64_t)C + (u & ush) * Tc::UC;
            };
            f32x4 acc[Tc::UN][3][3];
#pragma unroll
            for (int u = 0; u < Tc::UN; ++u)
#pragma unroll
                for (int ni = 0; ni < 3; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 3; ++mi) acc[u][ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
            bf16x8 rr[Tc::UN][5];
            float bvv[3];
            bf16x8 xa[3], xb[3];
            auto mma_unit = [&](int u, const bf16x8 (&xf)[3], int buf, int ks) {
#pragma unroll
                for (int ni = 0; ni < 3; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 3; ++mi) mma_step(acc[u][ni][mi], xf[ni], wf[buf][ks][mi]);
            };
#pragma unroll
            for (int it = 0; it < NT; ++it) {
                if (it + 2 < NT) load_w((it + 2) % 3, rowblk, it + 2);
                else load_w((it + 2) % 3, rownext, it + 2 - NT);
                if (it == 0) {                                       // behind W(2): the waits for W(0) and W(1) leave these in flight
                    // FINAL has no register to keep these two lane offsets across the loops (they spilled): recomputed per row block
                    const int ln = FINAL ? opaque_vgpr(lane) : lane;
                    const unsigned roff4 = FINAL ? (unsigned)((((256 + ln) / 6) * C + ((256 + ln) % 6) * 8) * (int)sizeof(bf16_t)) : loff[4];
                    const unsigned boff = (unsigned)((ln & 15) * (int)sizeof(float));
#pragma unroll
                    for (int u = 0; u < Tc::UN; ++u) {
                        const ALSEP_GLOBAL char* rp = opaque_uniform_gptr(reinterpret_cast<const char*>(R + unit_base(u)));
#pragma unroll
                        for (int g = 0; g < 4; ++g) rr[u][g] = *reinterpret_cast<const ALSEP_GLOBAL bf16x8*>(rp + loff[g]);
                        if (lane < Tc::TR * 6 - 256) rr[u][4] = *reinterpret_cast<const ALSEP_GLOBAL bf16x8*>(rp + roff4);
                    }
#pragma unroll
                    for (int mi = 0; mi < 3; ++mi) bvv[mi] = 0.f;
                    if (bias) {                                      // scalar base + 32-bit lane offset: no 64-bit lane pointer kept across the loops
                        const ALSEP_GLOBAL char* bp = opaque_uniform_gptr(reinterpret_cast<const char*>(bias + rowblk * Tc::TR));
#pragma unroll
                        for (int mi = 0; mi < 3; ++mi)
                            bvv[mi] = *reinterpret_cast<const ALSEP_GLOBAL float*>(bp + boff + mi * 16 * (int)sizeof(float));
                    }
                }
                const bf16_t* xs = xlane + (size_t)it * Tc::STAGE_ELEMS;
                if (it == 0) {
                    tdfw_read_x<0, 0>(xa, xs);
                    tdfw_read_x<0, 1>(xb, xs);
                }
                lds_read_tr16_wait_n<6>();  mma_unit(0, xa, it % 3, 0);
                tdfw_read_x<1, 0>(xa, xs);
                lds_read_tr16_wait_n<6>();  mma_unit(1, xb, it % 3, 0);
                tdfw_read_x<1, 1>(xb, xs);
                if (it + 1 < NT) {                                   // the next K tile's first fragments: the tile is resident, nothing to wait for
                    lds_read_tr16_wait_n<6>();  mma_unit(0, xa, it % 3, 1);
                    tdfw_read_x<0, 0>(xa, xs + Tc::STAGE_ELEMS);
                    lds_read_tr16_wait_n<6>();  mma_unit(1, xb, it % 3, 1);
                    tdfw_read_x<0, 1>(xb, xs + Tc::STAGE_ELEMS);
                } else {
                    lds_read_tr16_wait_n<6>();  mma_unit(0, xa, it % 3, 1);
                    lds_read_tr16_wait_n<0>();  mma_unit(1, xb, it % 3, 1);
                }
            }

            // Epilogue of this wave's 48 rows, one unit at a time through its private staging rows: arithmetic exactly as in
            // tdf_bf16_wide_kernel (bias, BN, ReLU and the residual add in fp32, one rounding).
#pragma unroll
            for (int u = 0; u < Tc::UN; ++u) {
                ALSEP_GLOBAL char* yb = const_cast<ALSEP_GLOBAL char*>(opaque_uniform_gptr(reinterpret_cast<const char*>(Y + unit_base(u))));
#pragma unroll
                for (int ni = 0; ni < 3; ++ni) {
                    const f32x4 sc = *reinterpret_cast<const f32x4*>(bnl + u * 2 * Tc::UC + ni * 16 + 4 * lq);
                    const f32x4 sh = *reinterpret_cast<const f32x4*>(bnl + u * 2 * Tc::UC + Tc::UC + ni * 16 + 4 * lq);
#pragma unroll
                    for (int mi = 0; mi < 3; ++mi) {
                        f32x4 v;
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = fmaxf(fmaf(acc[u][ni][mi][r] + bvv[mi], sc[r], sh[r]), 0.f);
                        *reinterpret_cast<f32x4*>(stg + (mi * 16 + l15) * Tc::SS + ni * 16 + 4 * lq) = v;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                bf16x8 q[5];
#pragma unroll
                for (int g = 0; g < 5; ++g) {
                    const int gidx = g * 64 + lane;
                    const int fr = gidx / 6, cg = gidx % 6;
                    if (gidx < Tc::TR * 6) {
                        const f32x4 lo = *reinterpret_cast<const f32x4*>(stg + fr * Tc::SS + cg * 8);
                        const f32x4 hi = *reinterpret_cast<const f32x4*>(stg + fr * Tc::SS + cg * 8 + 4);
                        float y[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                        for (int e = 0; e < 8; ++e) y[e] += (float)rr[u][g][e];
#pragma unroll
                        for (int e = 0; e < 8; ++e) q[g][e] = (bf16_t)y[e];
                        if (!FINAL) stream_store(reinterpret_cast<ALSEP_GLOBAL bf16x8*>(yb + loff[g]), q[g]);
                    }
                }
                __builtin_amdgcn_wave_barrier();
                if (FINAL) {
                    // every staging row is read: the rounded rows [48 f'][48 c] (row stride FS) take their place, then the chains
                    // of final_conv_kernel as in the wide kernel -- lane = f' row = one pixel of frame u0 + u (C == 48)
#pragma unroll
                    for (int g = 0; g < 5; ++g) {
                        const int gidx = g * 64 + lane;
                        if (gidx < Tc::TR * 6) *reinterpret_cast<bf16x8*>(frow + (gidx / 6) * Tc::FS + (gidx % 6) * 8) = q[g];
                    }
                    __builtin_amdgcn_wave_barrier();
                    const int ln = opaque_vgpr(lane);                // recomputed here, not kept (or spilled) across the k loop
                    const int frl = ln < Tc::TR ? ln : Tc::TR - 1;
                    float y[4] = {fbs[0], fbs[1], fbs[2], fbs[3]};
#pragma unroll 2
                    for (int ci = 0; ci < Tc::UC; ci += 8) {
                        const bf16x8 xv = *reinterpret_cast<const bf16x8*>(frow + frl * Tc::FS + ci);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const f32x4 w0 = *reinterpret_cast<const f32x4*>(fwl + r * Tc::UC + ci);
                            const f32x4 w1 = *reinterpret_cast<const f32x4*>(fwl + r * Tc::UC + ci + 4);
#pragma unroll
                            for (int e = 0; e < 4; ++e) y[r] = fmaf(w0[e], (float)xv[e], y[r]);
#pragma unroll
                            for (int e = 0; e < 4; ++e) y[r] = fmaf(w1[e], (float)xv[4 + e], y[r]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] *= falpha;
                    ALSEP_GLOBAL char* fo = const_cast<ALSEP_GLOBAL char*>(
                        opaque_uniform_gptr(reinterpret_cast<const char*>(FOUT + (((u0 + u) * M + rowblk * Tc::TR) << 2))));
                    bf16x4 yq;                                       // one rounding, as store4
#pragma unroll
                    for (int r = 0; r < 4; ++r) yq[r] = (bf16_t)y[r];
                    if (ln < Tc::TR) *reinterpret_cast<ALSEP_GLOBAL bf16x4*>(fo + (unsigned)ln * (4u * (unsigned)sizeof(bf16_t))) = yq;
                    __builtin_amdgcn_wave_barrier();                 // the next unit's staging rows overwrite these
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// bf16 ds (2x2/2 conv, 48 -> 96) and us (2x2 transposed conv, 96 -> 48, * skip) between levels 0 and 1,
// the two largest resampling layers.  Every input element feeds exactly one output pixel (no halo,
// no reuse), so nothing is staged: a wave keeps its weight fragments in registers for its whole
// life, reads activation fragments (16 contiguous bytes per lane) straight from global memory into
// the MFMA B operand, and only the epilogue goes through LDS to leave as whole contiguous rows.
// Weights are packed in fragment order [m-tile][k-step][lane][8].
// ------------------------------------------------------------------------------------------
// Epilogue image of the ds kernels: [64 px][MS] bf16 with MS = M + 4.  A ds_write_b64 group is 16 lanes = 16 consecutive
// pixels; with rows of M bf16 (M/2 dwords, a multiple of 16) they fall on two bank pairs (8-way; SQ_LDS_BANK_CONFLICT was
// 67-91 % of these kernels' LDS cycles), with M/2 + 2 dwords per row on sixteen distinct ones.  Rows are then only 8-byte
// aligned, so the copy-out reads its 16 bytes as two ds_read_b64.
struct Ds48 { static constexpr int C = 48, M = 96, MS = M + 4, K = 192, MT = 6, KS = 6; };
__device__ __forceinline__ vec16 lds_read16_align8(const bf16_t* p) {
    struct alignas(8) half16 { uint32_t w[2]; };
    const half16 a = *reinterpret_cast<const half16*>(p), b = *reinterpret_cast<const half16*>(p + 4);
    vec16 v;
    v.w[0] = a.w[0]; v.w[1] = a.w[1]; v.w[2] = b.w[0]; v.w[3] = b.w[1];
    return v;
}

__global__ void __launch_bounds__(kThreads, 1)
ds48_stream_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wf,
                   const float* __restrict__ scale, const float* __restrict__ shift, int64_t npix, int Tp, int Fp) {
    typedef Ds48 D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    bf16_t* stg = reinterpret_cast<bf16_t*>(alsep_smem) + (size_t)wave * 64 * D::MS;    // wave-private [64 px][96 ch (+4)]
    bf16x8 wf[D::MT][D::KS];
#pragma unroll
    for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
        for (int ks = 0; ks < D::KS; ++ks)
            wf[mt][ks] = *reinterpret_cast<const bf16x8*>(Wf + ((size_t)(mt * D::KS + ks) * 64 + lane) * 8);
    float sc[D::MT][4], sh[D::MT][4];
#pragma unroll
    for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { sc[mt][r] = scale[mt * 16 + 4 * lq + r]; sh[mt][r] = shift[mt * 16 + 4 * lq + r]; }
    const int64_t ntile = npix / 64;                         // Fp % 64 == 0: a tile is 64 consecutive f' of one row
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntile; tile += (int64_t)gridDim.x * 4) {
        const int64_t p0 = tile * 64;
        const int64_t fp0 = p0 % Fp, tp = (p0 / Fp) % Tp, bb = p0 / ((int64_t)Fp * Tp);
        // input pixel (2tp + dy, 2(fp0 + j) + dx): k = (dy*2 + dx)*48 + ci -> two runs of 96 per dy
        const bf16_t* xrow = X + ((bb * 2 * Tp + 2 * tp) * (2 * (int64_t)Fp) + 2 * fp0) * D::C;
        f32x4 acc[D::MT][4];
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mt][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < D::KS; ++ks) {
            const int k = ks * 32 + lq * 8;
            const int dy = k / (2 * D::C), rem = k % (2 * D::C);
            bf16x8 xf[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                xf[ni] = *reinterpret_cast<const bf16x8*>(xrow + (int64_t)dy * (2 * (int64_t)Fp * D::C) + (int64_t)(ni * 16 + l15) * (2 * D::C) + rem);
#pragma unroll
            for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) mma_step(acc[mt][ni], wf[mt][ks], xf[ni]);
        }
#pragma unroll
        for (int mt = 0; mt < D::MT; ++mt)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                float y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[mt][ni][r], sc[mt][r], sh[mt][r]), 0.f);
                store4(stg + (ni * 16 + l15) * D::MS + mt * 16 + 4 * lq, y);
            }
        __builtin_amdgcn_wave_barrier();
        bf16_t* yrow = Y + p0 * D::M;                        // 64 pixels x 96 channels = 12 KiB contiguous
#pragma unroll
        for (int it = 0; it < 64 * D::M / 8 / 64; ++it) {
            const int gidx = it * 64 + lane;
            *reinterpret_cast<vec16*>(yrow + (size_t)gidx * 8) = lds_read16_align8(stg + (gidx / (D::M / 8)) * D::MS + (gidx % (D::M / 8)) * 8);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ds for the deeper levels (C -> C + 48, C = 96): the weight block no longer fits one wave's registers, so the four
// waves of a workgroup share a tile of 64 output pixels and split the OUTPUT channels (m-tiles w, w + 4, w + 8): each
// keeps its 16-row weight fragments in registers for its whole life and streams the same activation fragments from
// global memory (the re-read by the other three waves is served by L1); the epilogue goes through one LDS image of the
// tile so that it leaves as whole contiguous rows.
template <int C_> struct DsSplitCfg {
    static constexpr int C = C_, M = C_ + 48, MS = M + 4, K = 4 * C_, MT = M / 16, KS = K / 32, MTW = (MT + 3) / 4;
    static_assert(M % 16 == 0 && K % 32 == 0, "ds stream geometry");
};
template <int C_, int OCC>
__global__ void __launch_bounds__(kThreads, OCC)
ds_split_stream_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wf,
                       const float* __restrict__ scale, const float* __restrict__ shift, int64_t npix, int Tp, int Fp) {
    typedef DsSplitCfg<C_> D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    bf16_t* stg = reinterpret_cast<bf16_t*>(alsep_smem);                                // [64 px][M ch]
    bf16x8 wf[D::MTW][D::KS];
#pragma unroll
    for (int j = 0; j < D::MTW; ++j) {
        const int mt = wave + 4 * j;
#pragma unroll
        for (int ks = 0; ks < D::KS; ++ks)
            wf[j][ks] = mt < D::MT ? *reinterpret_cast<const bf16x8*>(Wf + ((size_t)(mt * D::KS + ks) * 64 + lane) * 8) : bf16x8{};
    }
    const int64_t ntile = npix / 64;                         // Fp % 64 == 0: a tile is 64 consecutive f' of one row
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t p0 = tile * 64;
        const int64_t fp0 = p0 % Fp, tp = (p0 / Fp) % Tp, bb = p0 / ((int64_t)Fp * Tp);
        // input pixel (2tp + dy, 2(fp0 + j) + dx): k = (dy*2 + dx)*C + ci -> two runs of 2C per dy
        const bf16_t* xrow = X + ((bb * 2 * Tp + 2 * tp) * (2 * (int64_t)Fp) + 2 * fp0) * D::C;
        f32x4 acc[D::MTW][4];
#pragma unroll
        for (int j = 0; j < D::MTW; ++j)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[j][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < D::KS; ++ks) {
            const int k = ks * 32 + lq * 8;
            const int dy = k / (2 * D::C), rem = k % (2 * D::C);
            bf16x8 xf[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                xf[ni] = *reinterpret_cast<const bf16x8*>(xrow + (int64_t)dy * (2 * (int64_t)Fp * D::C) + (int64_t)(ni * 16 + l15) * (2 * D::C) + rem);
#pragma unroll
            for (int j = 0; j < D::MTW; ++j)
                if (wave + 4 * j < D::MT) {                  // wave-uniform
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) mma_step(acc[j][ni], wf[j][ks], xf[ni]);
                }
        }
#pragma unroll
        for (int j = 0; j < D::MTW; ++j) {
            const int mt = wave + 4 * j;
            if (mt < D::MT) {
                const f32x4 scv = *reinterpret_cast<const f32x4*>(scale + mt * 16 + 4 * lq);   // L1-resident, once per tile
                const f32x4 shv = *reinterpret_cast<const f32x4*>(shift + mt * 16 + 4 * lq);
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    float y[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[j][ni][r], scv[r], shv[r]), 0.f);
                    store4(stg + (ni * 16 + l15) * D::MS + mt * 16 + 4 * lq, y);
                }
            }
        }
        __syncthreads();
        bf16_t* yrow = Y + p0 * D::M;                        // 64 pixels x M channels, contiguous
        for (int it = tid; it < 64 * D::M / 8; it += kThreads)
            *reinterpret_cast<vec16*>(yrow + (size_t)it * 8) = lds_read16_align8(stg + (it / (D::M / 8)) * D::MS + (it % (D::M / 8)) * 8);
        __syncthreads();
    }
}

// Us<CIN, C2, NI>: CIN input channels -> C2 output channels per tap, tiles of 16 NI input pixels; K = CIN padded to a
// multiple of 32 (the fragment of the padded k-groups is zero on both sides: weights packed with zeros, activations not
// loaded).  Wave w owns tap (dy, dx) = (w >> 1, w & 1) of the 2x2 transposed kernel.
template <int CIN, int C2_, int NI_> struct UsCfg {
    static constexpr int C = CIN, C2 = C2_, NI = NI_, PX = 16 * NI_, MT = C2_ / 16, KS = (CIN + 31) / 32;
    // epilogue image [dy][2 PX output pixels][PS] fp32.  PS = C2 + 4: the lanes of a ds_write_b128 group hold consecutive
    // input pixels, i.e. rows 2 PS floats apart -- with PS = C2 (a multiple of 16) all eight fall on the same four banks
    // (8-way; SQ_LDS_BANK_CONFLICT was 83 % of this kernel's LDS cycles), with the pad it is 2-way
    static constexpr int PS = C2_ + 4;
    static constexpr size_t lds_bytes = 2 * (size_t)(2 * PX) * PS * sizeof(float);
    static_assert(C2_ % 16 == 0 && CIN % 8 == 0 && (2 * 2 * PX * (C2_ / 8)) % kThreads == 0, "us stream geometry");
};
template <int CIN, int C2_, int NI_, int OCC = 1>
__global__ void __launch_bounds__(kThreads, OCC)
us_stream_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wf,
                 const float* __restrict__ scale, const float* __restrict__ shift, const bf16_t* __restrict__ skip,
                 int64_t npix, int Tp, int Fp) {
    typedef UsCfg<CIN, C2_, NI_> U;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int dy = wave >> 1, dx = wave & 1;
    float* stg = reinterpret_cast<float*>(alsep_smem);
    bf16x8 wf[U::MT][U::KS];
#pragma unroll
    for (int mt = 0; mt < U::MT; ++mt)
#pragma unroll
        for (int ks = 0; ks < U::KS; ++ks)
            wf[mt][ks] = *reinterpret_cast<const bf16x8*>(Wf + ((size_t)((wave * U::MT + mt) * U::KS + ks) * 64 + lane) * 8);
    // scale / shift of this lane's rows: registers while they fit beside the weight fragments, L1 otherwise
    constexpr bool SS_REGS = U::MT <= 3;
    constexpr int SSN = SS_REGS ? U::MT : 1;
    float sc[SSN][4], sh[SSN][4];
    if (SS_REGS) {
#pragma unroll
        for (int mt = 0; mt < SSN; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { sc[mt][r] = scale[mt * 16 + 4 * lq + r]; sh[mt][r] = shift[mt * 16 + 4 * lq + r]; }
    }
    const int64_t ntile = npix / U::PX;                      // Fp % PX == 0: a tile is PX consecutive f' of one row
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t p0 = tile * U::PX;
        const int64_t fp0 = p0 % Fp, tp = (p0 / Fp) % Tp, bb = p0 / ((int64_t)Fp * Tp);
        f32x4 acc[U::MT][U::NI];
#pragma unroll
        for (int mt = 0; mt < U::MT; ++mt)
#pragma unroll
            for (int ni = 0; ni < U::NI; ++ni) acc[mt][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < U::KS; ++ks) {
            bf16x8 xf[U::NI];
#pragma unroll
            for (int ni = 0; ni < U::NI; ++ni) {
                if (U::C % 32 == 0 || ks * 32 + lq * 8 < U::C)
                    xf[ni] = *reinterpret_cast<const bf16x8*>(X + (p0 + ni * 16 + l15) * U::C + ks * 32 + lq * 8);
                else
                    xf[ni] = bf16x8{};                           // k-groups beyond CIN: zero weights, nothing to read
            }
#pragma unroll
            for (int mt = 0; mt < U::MT; ++mt)
#pragma unroll
                for (int ni = 0; ni < U::NI; ++ni) mma_step(acc[mt][ni], wf[mt][ks], xf[ni]);
        }
        // relu(bn(.)) in fp32 to LDS at output pixel 2j + dx of row dy
#pragma unroll
        for (int mt = 0; mt < U::MT; ++mt)
#pragma unroll
            for (int ni = 0; ni < U::NI; ++ni) {
                f32x4 y;
                if (SS_REGS) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[mt][ni][r], sc[SS_REGS ? mt : 0][r], sh[SS_REGS ? mt : 0][r]), 0.f);
                } else {
                    const f32x4 scv = *reinterpret_cast<const f32x4*>(scale + mt * 16 + 4 * lq);
                    const f32x4 shv = *reinterpret_cast<const f32x4*>(shift + mt * 16 + 4 * lq);
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[mt][ni][r], scv[r], shv[r]), 0.f);
                }
                *reinterpret_cast<f32x4*>(stg + ((size_t)dy * (2 * U::PX) + 2 * (ni * 16 + l15) + dx) * U::PS + mt * 16 + 4 * lq) = y;
            }
        __syncthreads();
        // 2 rows x 2 PX pixels x C2/8 groups of 8 channels; each output row is contiguous (2 PX x 2 C2 bytes)
        constexpr int NG = U::C2 / 8, ROWG = 2 * U::PX * NG;
#pragma unroll
        for (int it = 0; it < 2 * ROWG / kThreads; ++it) {
            const int gidx = it * kThreads + tid;
            const int row = gidx / ROWG, rem = gidx % ROWG;
            const int64_t o = ((bb * 2 * Tp + 2 * tp + row) * (2 * (int64_t)Fp) + 2 * fp0) * U::C2 + (int64_t)rem * 8;
            const float* src = stg + ((size_t)row * (2 * U::PX) + rem / NG) * U::PS + (rem % NG) * 8;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(src);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(src + 4);
            const bf16x8 sk = *reinterpret_cast<const bf16x8*>(skip + o);
            bf16x8 q;
#pragma unroll
            for (int e = 0; e < 4; ++e) { q[e] = (bf16_t)(lo[e] * (float)sk[e]); q[4 + e] = (bf16_t)(hi[e] * (float)sk[4 + e]); }
            stream_store(reinterpret_cast<bf16x8*>(Y + o), q);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// ds / us of the middle levels, pipelined across tiles (ALSEP_PIX_PIPE).  Same arithmetic as ds_split_stream_kernel and
// us_stream_kernel -- the same weight fragments in registers, the same wave owns the same m-tiles (ds) or tap (us), every
// accumulator runs over ks ascending, the same fp32 epilogue values and one rounding -- but the memory traffic of tile i + D
// is requested before tile i is computed:
//   * persistent workgroups of four waves, one per CU, striding statically over the tiles;
//   * the activation tile (and, for us, the skip tile) comes into an LDS ring by LDS-DMA, D tiles ahead; the B fragments are
//     ds_read_b128 from a swizzled image (LDS-DMA writes linearly, so the permutation is on the SOURCE address and on the
//     read), once per wave from LDS instead of four times from L1;
//   * one workgroup barrier per tile: behind it tile i's slot is complete, the slot of tile i - 1 is free for tile i + D, and
//     the output image of tile i - 1 is complete -- it leaves as whole rows of 16-byte stores under tile i's MFMAs;
//   * every wait in the tile loop is counted (vmcnt is in order: the stores issued behind an LDS-DMA are not waited for), and
//     every LDS access in it is asm with our own lgkmcnt waits: a compiler-tracked LDS access would be given s_waitcnt vmcnt
//     for ALL LDS-DMA in flight, i.e. drain the ring.
// ------------------------------------------------------------------------------------------
#ifdef ALSEP_CPU_EMUL
static inline void lds_write_async_b64(bf16_t* lds_ptr, const bf16x4& v) { std::memcpy(lds_ptr, &v, 8); }
template <int OFF>
static inline void lds_read_async_f32x4(f32x4& dst, const float* lds_ptr) { std::memcpy(&dst, reinterpret_cast<const char*>(lds_ptr) + OFF, 16); }
#else
// lds_read_async_b128 for four floats
template <int OFF>
__device__ __forceinline__ void lds_read_async_f32x4(f32x4& dst, const float* lds_ptr) {
    static_assert(OFF >= 0 && OFF < 65536 && OFF % 16 == 0, "ds offset field");
    const unsigned addr = (unsigned)(unsigned long long)(__attribute__((address_space(3))) const void*)lds_ptr;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
// 8-byte LDS write invisible to hipcc's waitcnt bookkeeping (completed by the lgkmcnt(0) of barrier_nodrain / lds_wait_n<0>)
__device__ __forceinline__ void lds_write_async_b64(bf16_t* lds_ptr, const bf16x4& v) {
    const unsigned addr = (unsigned)(unsigned long long)(__attribute__((address_space(3))) void*)lds_ptr;
    asm volatile("ds_write_b64 %0, %1" : : "v"(addr), "v"(v) : "memory");
}
#endif
template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
// f(std::integral_constant<int, 0>) ... f(std::integral_constant<int, N - 1>): loop indices that instruction immediates need
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}
// counted wait at the top of tile i of a workgroup's n tiles: DMA(i) has landed.  Behind DMA(i) this wave has issued, in
// order, the DMAs of the next D - 1 tiles (ND each) and the stores of one earlier tile per iteration since (NS each, none
// in iteration 0); without all D - 1 successors (the last tiles) everything is waited for.
template <int D, int ND, int NS>
__device__ __forceinline__ void pipe_wait_tile(int i, int n) {
    static_assert(D >= 1 && D * NS + (D - 1) * ND < 64, "vmcnt is a 6-bit counter");
    if (i + D - 1 < n) {
        if (i > D) wait_vmcnt<D * NS + (D - 1) * ND>();
        else wait_vmcnt<(D - 1) * ND>();
    } else {
        wait_vmcnt<0>();
    }
}

// ds: tiles of PX output pixels of one row.  The input of a tile is two runs (dy = 0, 1) of PX * 2C contiguous channels; slot
// image [dy][PX px][SR 16-byte groups], group g of pixel row r at position g ^ swz(r): conflict-free for the ds_read_b128
// lane groups (16 pixels x 2 adjacent k-groups) at both pixel strides -- 24 groups (C = 96: 8 distinct rows mod 16 slots) and
// 36 groups (C = 144: 4 distinct).  Output image [PX][M + 8] bf16, two of them.
template <int C_, int PX_, int D_> struct DsPipeCfg {
    typedef DsSplitCfg<C_> S;
    static constexpr int C = C_, M = S::M, MT = S::MT, KS = S::KS, MTW = S::MTW, PX = PX_, NI = PX_ / 16, D = D_, NSLOT = D_ + 1;
    static constexpr int SR = C_ / 4, HALF_G = PX * SR, TILE_G = 2 * HALF_G, ND = TILE_G / kThreads;
    static constexpr int MS = M + 8, OUT_GW = PX * M / 8 / 4, NS = (OUT_GW + 63) / 64;
    static constexpr size_t tile_bytes = (size_t)TILE_G * 16, img_bytes = (size_t)PX * MS * sizeof(bf16_t);
    static constexpr size_t lds_bytes = NSLOT * tile_bytes + 2 * img_bytes;
    __host__ __device__ static constexpr int swz(int row) { return SR % 8 == 0 ? (row & 7) : ((row >> 2) & 2); }
    static_assert(PX % 16 == 0 && HALF_G % 64 == 0 && TILE_G % kThreads == 0 && KS % 2 == 0 && SR % 4 == 0 && (PX * M / 8) % 4 == 0,
                  "ds pipe geometry");
    static_assert(lds_bytes <= 160 * 1024 && tile_bytes < 65536, "LDS of a CU; ds offset field");
};
template <int C_, int PX_, int D_>
__global__ void __launch_bounds__(kThreads, 1)
ds_pipe_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wf,
               const float* __restrict__ scale, const float* __restrict__ shift, int64_t npix, int Tp, int Fp) {
    typedef DsPipeCfg<C_, PX_, D_> P;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    char* ring = alsep_smem;
    bf16_t* img = reinterpret_cast<bf16_t*>(alsep_smem + P::NSLOT * P::tile_bytes);
    bf16x8 wf[P::MTW][P::KS];
    f32x4 sc[P::MTW], sh[P::MTW];
#pragma unroll
    for (int j = 0; j < P::MTW; ++j) {
        const int mt = wave + 4 * j;
#pragma unroll
        for (int ks = 0; ks < P::KS; ++ks)
            wf[j][ks] = mt < P::MT ? *reinterpret_cast<const bf16x8*>(Wf + ((size_t)(mt * P::KS + ks) * 64 + lane) * 8) : bf16x8{};
        sc[j] = mt < P::MT ? *reinterpret_cast<const f32x4*>(scale + mt * 16 + 4 * lq) : f32x4{0.f, 0.f, 0.f, 0.f};
        sh[j] = mt < P::MT ? *reinterpret_cast<const f32x4*>(shift + mt * 16 + 4 * lq) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // LDS-DMA duty of this wave: ND consecutive 1 KiB pieces of the slot; lane offsets from the tile's first input pixel
    unsigned xoff[P::ND];
#pragma unroll
    for (int q = 0; q < P::ND; ++q) {
        const int pg = (wave * P::ND + q) * 64 + lane;
        const int dy = pg / P::HALF_G, row = (pg % P::HALF_G) / P::SR, gp = pg % P::SR;
        xoff[q] = (unsigned)dy * (2u * (unsigned)Fp * P::C * (unsigned)sizeof(bf16_t)) + (unsigned)((row * P::SR + (gp ^ P::swz(row))) * 16);
    }
    // B fragment of k-step kk of either dy: pixel row l15 (+ 16 ni), group 4 kk + lq, at its swizzled position
    unsigned bk[P::KS / 2];
#pragma unroll
    for (int kk = 0; kk < P::KS / 2; ++kk) bk[kk] = (unsigned)((l15 * P::SR + ((kk * 4 + lq) ^ P::swz(l15))) * 16);
    // output: wave w copies groups [w, w + 1) * OUT_GW of the image's PX * M / 8
    unsigned ioff[P::NS];
#pragma unroll
    for (int t = 0; t < P::NS; ++t) {
        const int g = wave * P::OUT_GW + t * 64 + lane;
        ioff[t] = (unsigned)(((g / (P::M / 8)) * P::MS + (g % (P::M / 8)) * 8) * (int)sizeof(bf16_t));
    }

    const int64_t ntile = npix / P::PX;                      // Fp % PX == 0: a tile is PX consecutive f' of one row
    const int nmy = (int)((ntile - (int64_t)blockIdx.x + gridDim.x - 1) / gridDim.x);
    auto issue = [&](int j) {
        const int64_t p0 = ((int64_t)blockIdx.x + (int64_t)j * gridDim.x) * P::PX;
        const int64_t fp0 = p0 % Fp, tp = (p0 / Fp) % Tp, bb = p0 / ((int64_t)Fp * Tp);
        // input pixel (2tp + dy, 2(fp0 + j) + dx): k = (dy*2 + dx)*C + ci -> one run of PX * 2C per dy
        const ALSEP_GLOBAL char* src = opaque_uniform_gptr(
            reinterpret_cast<const char*>(X + ((bb * 2 * Tp + 2 * tp) * (2 * (int64_t)Fp) + 2 * fp0) * P::C));
        char* dst = ring + (size_t)(j % P::NSLOT) * P::tile_bytes + (size_t)wave * (P::ND * 1024);
#pragma unroll
        for (int q = 0; q < P::ND; ++q) glds16_base(src, xoff[q], dst + q * 1024);
    };
    auto copy_out = [&](int j) {
        const int64_t p0 = ((int64_t)blockIdx.x + (int64_t)j * gridDim.x) * P::PX;
        ALSEP_GLOBAL char* yb = const_cast<ALSEP_GLOBAL char*>(
            opaque_uniform_gptr(reinterpret_cast<const char*>(Y + p0 * P::M + (int64_t)wave * (P::OUT_GW * 8))));
        const char* im = reinterpret_cast<const char*>(img) + (size_t)(j & 1) * P::img_bytes;
        bf16x8 q[P::NS];
#pragma unroll
        for (int t = 0; t < P::NS; ++t)
            if (t * 64 + lane < P::OUT_GW) lds_read_async_b128<0>(q[t], reinterpret_cast<const bf16_t*>(im + ioff[t]));
        lds_wait_n<0>();
#pragma unroll
        for (int t = 0; t < P::NS; ++t)
            if (t * 64 + lane < P::OUT_GW) stream_store(reinterpret_cast<ALSEP_GLOBAL bf16x8*>(yb + (unsigned)(t * 64 + lane) * 16u), q[t]);
    };

    wait_vmcnt<0>();                                         // weights, scale and shift are in registers
#pragma unroll
    for (int j = 0; j < P::D; ++j)
        if (j < nmy) issue(j);
    for (int i = 0; i < nmy; ++i) {
        pipe_wait_tile<P::D, P::ND, P::NS>(i, nmy);
        barrier_nodrain();                                   // tile i is in LDS for every wave; tile i - 1 is computed, its slot free
        if (i + P::D < nmy) issue(i + P::D);
        if (i > 0) copy_out(i - 1);
        const bf16_t* slot = reinterpret_cast<const bf16_t*>(ring + (size_t)(i % P::NSLOT) * P::tile_bytes);
        f32x4 acc[P::MTW][P::NI];
#pragma unroll
        for (int j = 0; j < P::MTW; ++j)
#pragma unroll
            for (int ni = 0; ni < P::NI; ++ni) acc[j][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
        bf16x8 xf[2][P::NI];
        static_for<P::NI>([&](auto nic) {
            constexpr int ni = decltype(nic)::value;
            lds_read_async_b128<ni * 16 * P::SR * 16>(xf[0][ni], slot + bk[0] / sizeof(bf16_t));
        });
        static_for<P::KS>([&](auto ksc) {
            constexpr int ks = decltype(ksc)::value, b = ks & 1;
            if constexpr (ks + 1 < P::KS) {
                constexpr int dy1 = (ks + 1) / (P::KS / 2), kk1 = (ks + 1) % (P::KS / 2);
                static_for<P::NI>([&](auto nic) {
                    constexpr int ni = decltype(nic)::value;
                    lds_read_async_b128<dy1 * P::HALF_G * 16 + ni * 16 * P::SR * 16>(xf[1 - b][ni], slot + bk[kk1] / sizeof(bf16_t));
                });
                lds_wait_n<P::NI>();                         // step ks has landed, step ks + 1 is in flight
            } else {
                lds_wait_n<0>();
            }
#pragma unroll
            for (int j = 0; j < P::MTW; ++j)
                if (wave + 4 * j < P::MT) {                  // wave-uniform
#pragma unroll
                    for (int ni = 0; ni < P::NI; ++ni) mma_step(acc[j][ni], wf[j][ks], xf[b][ni]);
                }
        });
        bf16_t* im = img + (size_t)(i & 1) * (P::PX * P::MS);
#pragma unroll
        for (int j = 0; j < P::MTW; ++j) {
            const int mt = wave + 4 * j;
            if (mt < P::MT) {
#pragma unroll
                for (int ni = 0; ni < P::NI; ++ni) {
                    bf16x4 q;                                // one rounding, as store4
#pragma unroll
                    for (int r = 0; r < 4; ++r) q[r] = (bf16_t)fmaxf(fmaf(acc[j][ni][r], sc[j][r], sh[j][r]), 0.f);
                    lds_write_async_b64(im + (ni * 16 + l15) * P::MS + mt * 16 + 4 * lq, q);
                }
            }
        }
    }
    barrier_nodrain();
    copy_out(nmy - 1);
}

// us: tiles of PX input pixels of one row.  X slot: wave w's quarter of the pixel rows (PX / 4 rows of SRX 16-byte groups, padded
// to whole 1 KiB pieces: the surplus lanes re-read the quarter's last group into the pad) at w * XREG; group g of row r at
// g ^ swz(r) (24 groups: 8 distinct rows mod 16 slots; 18 groups are conflict-free as they are).  S slot: the skip tile
// [dy][2 PX output pixels][NG groups], group g of pixel p at position (g + rot(p)) mod NG, so that the eight-byte accesses of the
// MFMA lanes (16 pixels 2 C2 elements apart) spread over the banks.  The epilogue multiplies there: lane (tap, pixel, 4 channels)
// reads its skip values, forms relu(bn(acc)) * skip in fp32 -- the product us_stream_kernel forms in its copy-out -- rounds once
// and writes the result over them, so the slot becomes the output image and leaves by the addresses it came from.
template <int CIN, int C2_, int NI_, int D_> struct UsPipeCfg {
    typedef UsCfg<CIN, C2_, NI_> U;
    static constexpr int C = CIN, C2 = C2_, NI = NI_, PX = 16 * NI_, MT = U::MT, KS = U::KS, D = D_, NSX = D_ + 1, NSS = D_ + 2;
    static constexpr int SRX = CIN / 8, XW_G = (PX / 4) * SRX, NDX = (XW_G + 63) / 64, XREG = NDX * 1024;
    static constexpr int NG = C2_ / 8, ROW_G = 2 * PX * NG, S_G = 2 * ROW_G, NDS = S_G / kThreads;
    static constexpr int ND = NDX + NDS, NS = NDS;
    static constexpr size_t x_bytes = 4 * (size_t)XREG, s_bytes = (size_t)S_G * 16, bn_bytes = 2 * (size_t)C2_ * sizeof(float);
    static constexpr size_t lds_bytes = NSX * x_bytes + NSS * s_bytes + bn_bytes;
    __host__ __device__ static constexpr int swz(int row) { return SRX % 8 == 0 ? (row & 7) : 0; }
    __host__ __device__ static constexpr int rot(int px) { return NG % 4 == 0 ? ((px >> 2) & 7) : ((px >> 3) & 3); }
    static_assert(PX % 32 == 0 && ROW_G % 64 == 0 && S_G % kThreads == 0 && (NG % 4 == 0 ? NG >= 8 : NG >= 4), "us pipe geometry");
    static_assert(lds_bytes <= 160 * 1024 && x_bytes < 65536 && s_bytes < 65536, "LDS of a CU; ds offset field");
};
template <int CIN, int C2_, int NI_, int D_>
__global__ void __launch_bounds__(kThreads, 1)
us_pipe_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wf,
               const float* __restrict__ scale, const float* __restrict__ shift, const bf16_t* __restrict__ skip,
               int64_t npix, int Tp, int Fp) {
    typedef UsPipeCfg<CIN, C2_, NI_, D_> P;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int dy = wave >> 1, dx = wave & 1;
    char* xring = alsep_smem;
    char* sring = alsep_smem + P::NSX * P::x_bytes;
    float* bn = reinterpret_cast<float*>(alsep_smem + P::NSX * P::x_bytes + P::NSS * P::s_bytes);   // [scale | shift][C2]
    bf16x8 wf[P::MT][P::KS];
#pragma unroll
    for (int mt = 0; mt < P::MT; ++mt)
#pragma unroll
        for (int ks = 0; ks < P::KS; ++ks)
            wf[mt][ks] = *reinterpret_cast<const bf16x8*>(Wf + ((size_t)((wave * P::MT + mt) * P::KS + ks) * 64 + lane) * 8);
    for (int c = tid; c < 2 * P::C2; c += kThreads) bn[c] = c < P::C2 ? scale[c] : shift[c - P::C2];
    // LDS-DMA duty of this wave: its quarter of the X rows, and NDS consecutive 1 KiB pieces of the S slot
    unsigned xoff[P::NDX], soff[P::NDS];
#pragma unroll
    for (int q = 0; q < P::NDX; ++q) {
        const int gi = q * 64 + lane < P::XW_G ? q * 64 + lane : P::XW_G - 1;
        const int row = gi / P::SRX, gp = gi % P::SRX;
        xoff[q] = (unsigned)(((wave * (P::PX / 4) + row) * P::SRX + (gp ^ P::swz(row))) * 16);
    }
#pragma unroll
    for (int q = 0; q < P::NDS; ++q) {
        const int pg = (wave * P::NDS + q) * 64 + lane;
        const int row = pg / P::ROW_G, px = (pg % P::ROW_G) / P::NG, gp = pg % P::NG;
        soff[q] = (unsigned)row * (2u * (unsigned)Fp * P::C2 * (unsigned)sizeof(bf16_t)) + (unsigned)((px * P::NG + (gp - P::rot(px) + P::NG) % P::NG) * 16);
    }
    // B fragment of k-step ks: pixel row l15 (+ 16 ni), group 4 ks + lq at its swizzled position.  CIN % 32 != 0: the last step's
    // groups beyond CIN (zero weights) read a valid group and are zeroed.
    unsigned bk[P::KS];
#pragma unroll
    for (int ks = 0; ks < P::KS; ++ks) {
        const int g = ks * 4 + lq < P::SRX ? ks * 4 + lq : P::SRX - 1;
        bk[ks] = (unsigned)((l15 >> 3) * P::XREG + ((l15 & 7) * P::SRX + (g ^ P::swz(l15 & 7))) * 16);
    }
    const bool klast_ok = P::C % 32 == 0 || (P::KS - 1) * 4 + lq < P::SRX;
    // epilogue: output pixel 2 (16 ni + l15) + dx of row dy, channels 16 mt + 4 lq ..: half (lq & 1) of group 2 mt + (lq >> 1)
    const int opx = 2 * l15 + dx;
    const unsigned ebase = (unsigned)((dy * P::ROW_G + opx * P::NG) * 16);
    const int erot = (lq >> 1) + P::rot(opx);

    const int64_t ntile = npix / P::PX;                      // Fp % PX == 0: a tile is PX consecutive f' of one row
    const int nmy = (int)((ntile - (int64_t)blockIdx.x + gridDim.x - 1) / gridDim.x);
    auto out_base = [&](int j) {
        const int64_t p0 = ((int64_t)blockIdx.x + (int64_t)j * gridDim.x) * P::PX;
        const int64_t fp0 = p0 % Fp, tp = (p0 / Fp) % Tp, bb = p0 / ((int64_t)Fp * Tp);
        return ((bb * 2 * Tp + 2 * tp) * (2 * (int64_t)Fp) + 2 * fp0) * P::C2;
    };
    auto issue = [&](int j) {
        const int64_t p0 = ((int64_t)blockIdx.x + (int64_t)j * gridDim.x) * P::PX;
        const ALSEP_GLOBAL char* xs = opaque_uniform_gptr(reinterpret_cast<const char*>(X + p0 * P::C));
        const ALSEP_GLOBAL char* ss = opaque_uniform_gptr(reinterpret_cast<const char*>(skip + out_base(j)));
        char* xd = xring + (size_t)(j % P::NSX) * P::x_bytes + (size_t)wave * P::XREG;
        char* sd = sring + (size_t)(j % P::NSS) * P::s_bytes + (size_t)wave * (P::NDS * 1024);
#pragma unroll
        for (int q = 0; q < P::NDX; ++q) glds16_base(xs, xoff[q], xd + q * 1024);
#pragma unroll
        for (int q = 0; q < P::NDS; ++q) glds16_base(ss, soff[q], sd + q * 1024);
    };
    auto copy_out = [&](int j) {
        ALSEP_GLOBAL char* yb = const_cast<ALSEP_GLOBAL char*>(opaque_uniform_gptr(reinterpret_cast<const char*>(Y + out_base(j))));
        const bf16_t* sd = reinterpret_cast<const bf16_t*>(sring + (size_t)(j % P::NSS) * P::s_bytes + (size_t)wave * (P::NDS * 1024)) + lane * 8;
        bf16x8 q[P::NDS];
        static_for<P::NDS>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            lds_read_async_b128<t * 1024>(q[t], sd);
        });
        lds_wait_n<0>();
#pragma unroll
        for (int t = 0; t < P::NDS; ++t) stream_store(reinterpret_cast<ALSEP_GLOBAL bf16x8*>(yb + soff[t]), q[t]);
    };

    wait_vmcnt<0>();                                         // weights are in registers
#pragma unroll
    for (int j = 0; j < P::D; ++j)
        if (j < nmy) issue(j);
    for (int i = 0; i < nmy; ++i) {
        pipe_wait_tile<P::D, P::ND, P::NS>(i, nmy);
        barrier_nodrain();               // tile i (X, skip) is in LDS for every wave (first tile: bn too); tile i - 1 is an output image
        if (i + P::D < nmy) issue(i + P::D);
        if (i > 0) copy_out(i - 1);
        const bf16_t* xs = reinterpret_cast<const bf16_t*>(xring + (size_t)(i % P::NSX) * P::x_bytes);
        f32x4 acc[P::MT][P::NI];
#pragma unroll
        for (int mt = 0; mt < P::MT; ++mt)
#pragma unroll
            for (int ni = 0; ni < P::NI; ++ni) acc[mt][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
        bf16x8 xf[2][P::NI];
        static_for<P::NI>([&](auto nic) {
            constexpr int ni = decltype(nic)::value;
            lds_read_async_b128<ni * 2 * P::XREG>(xf[0][ni], xs + bk[0] / sizeof(bf16_t));
        });
        static_for<P::KS>([&](auto ksc) {
            constexpr int ks = decltype(ksc)::value, b = ks & 1;
            if constexpr (ks + 1 < P::KS) {
                static_for<P::NI>([&](auto nic) {
                    constexpr int ni = decltype(nic)::value;
                    lds_read_async_b128<ni * 2 * P::XREG>(xf[1 - b][ni], xs + bk[ks + 1] / sizeof(bf16_t));
                });
                lds_wait_n<P::NI>();                         // step ks has landed, step ks + 1 is in flight
            } else {
                lds_wait_n<0>();
                if (P::C % 32 != 0) {
#pragma unroll
                    for (int ni = 0; ni < P::NI; ++ni) xf[b][ni] = klast_ok ? xf[b][ni] : bf16x8{};
                }
            }
#pragma unroll
            for (int mt = 0; mt < P::MT; ++mt)
#pragma unroll
                for (int ni = 0; ni < P::NI; ++ni) mma_step(acc[mt][ni], wf[mt][ks], xf[b][ni]);
        });
        // relu(bn(.)) * skip in fp32, one rounding, over the skip values; m-tile mt + 1's operands are requested under mt's arithmetic
        bf16_t* sl = reinterpret_cast<bf16_t*>(sring + (size_t)(i % P::NSS) * P::s_bytes + ebase);
        const float* bnl = bn + 4 * lq;
        auto eoff = [&](int mt) {                            // group (2 mt + (lq >> 1) + rot) mod NG of this lane's pixel, in elements
            int t = 2 * mt + erot;
            t = t >= P::NG ? t - P::NG : t;
            return t * 8;
        };
        bf16x8 ev[2][P::NI];
        f32x4 scv[2], shv[2];
        auto eread = [&](auto mtc) {
            constexpr int mt = decltype(mtc)::value, eb = mt & 1;
            const bf16_t* p = sl + eoff(mt);
            static_for<P::NI>([&](auto nic) {
                constexpr int ni = decltype(nic)::value;
                lds_read_async_b128<ni * 32 * P::NG * 16>(ev[eb][ni], p);
            });
            lds_read_async_f32x4<0>(scv[eb], bnl + mt * 16);
            lds_read_async_f32x4<P::C2 * 4>(shv[eb], bnl + mt * 16);
        };
        eread(std::integral_constant<int, 0>{});
        static_for<P::MT>([&](auto mtc) {
            constexpr int mt = decltype(mtc)::value, b = mt & 1;
            if constexpr (mt + 1 < P::MT) {
                eread(std::integral_constant<int, mt + 1>{});
                lds_wait_n<P::NI + 2>();
            } else {
                lds_wait_n<0>();
            }
            bf16_t* p = sl + eoff(mt) + (lq & 1) * 4;
            static_for<P::NI>([&](auto nic) {
                constexpr int ni = decltype(nic)::value;
                const bf16x4 sk = (lq & 1) ? __builtin_shufflevector(ev[b][ni], ev[b][ni], 4, 5, 6, 7)
                                           : __builtin_shufflevector(ev[b][ni], ev[b][ni], 0, 1, 2, 3);
                bf16x4 q;
#pragma unroll
                for (int r = 0; r < 4; ++r) q[r] = (bf16_t)(fmaxf(fmaf(acc[mt][ni][r], scv[b][r], shv[b][r]), 0.f) * (float)sk[r]);
                lds_write_async_b64(p + ni * 32 * P::NG * 8, q);
            });
        });
    }
    barrier_nodrain();
    copy_out(nmy - 1);
}

// ------------------------------------------------------------------------------------------
// bf16 3x3 convolution, levels 2 and 3 (c = 144 / 192): all output channels against one patch, everything streamed.
// The plain kernel at c = 192 stages 81 KB per 10.6 MFLOP and re-stages the halo patch for each 48-channel output block;
// conv3x3_bf16_big_kernel<3> has one patch buffer (its 63 KB DMA is exposed every third stage) and reads 7 fragments per 12 MFMAs.
// Here, in the structure of conv3x3_bf16_m0_kernel (8 waves, 8 x TW tiles, one pixel row per wave, two patch buffers):
//  * a wave accumulates ALL Cout = 16 NM channels of its row: NM x TW / 16 accumulator tiles, TW / 16 + NM fragment reads per
//    NM TW / 16 MFMAs (12 per 27 at c = 144, 15 per 36 at c = 192);
//  * the weights are a k-step-major image (ConvLayer::w_ac): one k-step of all rows is Cout x 64 B, streamed through a ring of NSLOT
//    slots of KS k-steps each, DIST = NSLOT - 1 stages ahead.  Each wave copies the same eighth of every slot (whole LDS-DMA
//    instructions plus one with fewer lanes), so the LDS-DMA count per stage is a constant and nothing is copied twice;
//  * the patch of the next (tile, chunk) arrives one piece per stage in the other buffer;
//  * ONE barrier per stage, none per patch.  The barrier of stage s guarantees stage s + 1 (every wave has waited for its pieces of
//    it), so the fragment reads run one unit (a third or a quarter of a k-step: three 16-row weight blocks) ahead ACROSS the barrier
//    (within a patch; the first unit of the next patch is requested after a finished tile's stores);
//  * weight fragments come three at a time in two sets, and there is ONE set of patch fragments: in the last unit of a k-step the
//    MFMAs run pixel block by pixel block, and a patch fragment that has fed its last MFMA is requested again for the next k-step;
//    a whole second k-step set would not fit beside 144 accumulators.
// The k order is the plain kernel's (48-channel chunks, 14 k-steps of groups 4 s + lq, the two padded groups zero): every output
// element sees the same MFMA sequence -- bit-identical to conv3x3_bf16_kernel.
// Output groups (NGRP > 1): a layer of Cout = NGRP x 16 NM channels runs on the instance of 16 NM rows.  A work item is (tile, group); a
// workgroup takes the NGRP groups of one tile back to back -- item it is tile blockIdx.x + (it / NGRP) gridDim.x, group it % NGRP -- so
// the patch pieces of a tile's later groups come from the cache that its first group filled.  The weight image is one group image after
// another (pack_conv3x3_allco of each 16 NM-row slice), scale / shift of all Cout rows sit in LDS, and the epilogue adds the group's
// channel offset; the rings, the counted waits, the barrier per stage and the read-ahead run over items as they run over tiles, so
// every output element still sees the plain kernel's MFMA sequence.  The price: the patch is staged once per group, not once per tile.
// Instances: <9, 48> in one group (c = 144, level 2), <6, 48> and <6, 64> in two groups (c = 192, level 3) and in three (c = 288,
// tests only).  One group of 12 row blocks at c = 192 -- conv3x3_bf16_allco_kernel<12, 48>, 144 accumulators -- needs 256 VGPRs and
// spills 15 more to scratch and is not built (profiles/conv_allco_ab.txt); the arithmetic for UPK = 4 stays from that compile.
// ------------------------------------------------------------------------------------------
template <int NM_, int TW_, int NGRP_ = 1>
struct ConvAllco {
    static constexpr int NGRP = NGRP_, COUT = NGRP_ * 16 * NM_;       // output groups of 16 NM rows each; the layer's channels
    static constexpr int NM = NM_, TW = TW_, TH = 8, KC = 48, CG = 6, NG = 54, NS = 14, NI = TW / 16, ROWS = 16 * NM, NB = NM, NPAIR = NB / 2;
    static constexpr int UPK = NM % 4 == 0 ? 4 : 3, G = NM / UPK;   // units per k-step, weight fragments per unit
    static constexpr int KS = 1, NSLOT = 4, DIST = NSLOT - 1, NSTG = NS / KS, UPS = UPK * KS;  // k-steps per slot, slots, units per stage
    static constexpr int PW = TW + 2, PH = TH + 2;
    static constexpr int PGROUPS = PH * PW * CG, PINST = (PGROUPS + 63) / 64, PJ = (PINST + 7) / 8, PBUF = PINST * 64;
    static constexpr int KSTEP_BYTES = ROWS * 64, SLOT_BYTES = KS * KSTEP_BYTES;
    static constexpr int WPW = SLOT_BYTES / 8;               // a wave's share of a slot
    static constexpr int WJ = (WPW + 1023) / 1024, WLAST = (WPW - (WJ - 1) * 1024) / 16;        // its LDS-DMA instructions; lanes of the last
    static constexpr int ST = NI * (NPAIR + NB % 2);         // epilogue stores per wave and tile
    static constexpr size_t ring_bytes = 16 * (size_t)(2 * PBUF) + (size_t)NSLOT * SLOT_BYTES;
    static constexpr size_t lds_bytes = ring_bytes + 2 * COUT * sizeof(float) + 1024;   // + 1 KiB scratch (surplus patch pieces)
    static_assert(NGRP >= 1 && NM % 3 == 0 && NM % UPK == 0 && TW % 16 == 0 && NS % KS == 0 && SLOT_BYTES % (8 * 16) == 0, "ConvAllco: shape");
    static_assert(DIST >= 2 && DIST < NSTG && WJ < UPS && PJ - 1 <= NSTG - DIST && NSTG - 1 >= PJ, "ConvAllco: DMA schedule");
    static_assert(lds_bytes <= 160 * 1024, "ConvAllco: LDS budget");
    // 64-byte weight rows: lane (l15, lq) reads position lq ^ wswz(row) of row 16 m + l15.  The 16-lane groups of ds_read_b128 hold every
    // l15 once, {0-3, 12-15} from one lq and {4-11} from its neighbour lq ^ 1: rows l15 & 3 pick the 64-byte quarter of the 256-byte bank
    // line, and within a quarter the four rows l15 >> 2 = 0, 1, 2, 3 sit at lq, lq ^ 1, lq ^ 1 ^ 2, lq ^ 2 -- four distinct positions.
    // Enumerated over every row block, slot and lane group: each group touches each of the 64 banks once (profiles/conv_allco_ab.txt).
    __host__ __device__ static constexpr int wswz(int row) { return ((row >> 3) & 1) << 1; }
    // Patch fragment of k-step st, lane (l15, lq): group 4 st + lq of the 54 tap-major groups of pixel (wave, l15), i.e. byte
    // ((wave + tap / 3) PW + tap % 3 + l15) 96 + 16 cg.  Consecutive taps of a patch row are consecutive pixels, so the groups of a
    // k-step are 16 lq bytes apart from a constant -- xconst(st), an instruction immediate, over the per-lane base
    // (wave PW + l15) 96 + 16 lq -- except where the k-step crosses from tap 2 to tap 3 (st = 4: the next patch row) and at the two
    // padded groups (st = 13, lq >= 2: group 53 again, whose weights are zero as in the plain kernel).  Those two k-steps have bases
    // of their own: three registers instead of NS.
    __host__ __device__ static constexpr int tapoff(int tap) { return ((tap / 3) * PW + tap % 3) * KC * 2; }
    __host__ __device__ static constexpr int xconst(int st) { return tapoff(4 * st / CG) + 16 * (4 * st % CG); }
    __host__ __device__ static constexpr int xkind(int st) { return st == 4 ? 1 : st == NS - 1 ? 2 : 0; }
    __host__ __device__ static constexpr int xbase(int kind, int wave, int l15, int lq) {
        const int a = (wave * PW + l15) * KC * 2 + 16 * lq;
        return kind == 0 ? a : kind == 1 ? a + (lq >= 2 ? (PW - 3) * KC * 2 : 0) : a - (lq >= 2 ? 16 * (lq - 1) : 0);
    }
    static_assert(CG == 6 && NS == 14 && NG == 54, "xconst / xkind are written for 54 groups in 14 k-steps");
    // LDS-DMA instructions of one wave in stage sc of a chunk: its weight pieces, and one patch piece in the first PJ stages
    __host__ __device__ static constexpr int dma_of_stage(int sc) { return WJ + (sc < PJ ? 1 : 0); }
    // what may still be in flight at the barrier of stage sc: the DIST - 2 stages before it (stores of a finished tile not counted)
    __host__ __device__ static constexpr int inflight_at(int sc) {
        int n = 0;
        for (int i = 1; i <= DIST - 2; ++i) n += dma_of_stage((sc - i + NSTG) % NSTG);
        return n;
    }
};

// weight fragment reads of unit U = UPK st + t of a chunk: rows 16 (t G + g) + l15 of k-step st
template <typename Cf, int U>
__device__ __forceinline__ void allco_read_w(bf16x8 (&wf)[2][Cf::G], const bf16_t* wl) {
    constexpr int st = U / Cf::UPK, t = U % Cf::UPK;
    static_for<Cf::G>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        lds_read_async_b128<(t * Cf::G + g) * 1024 + (st % Cf::KS) * Cf::KSTEP_BYTES>(wf[U & 1][g], wl);
    });
}
// patch fragment ni of k-step ST; pb: the patch buffer's LDS address plus the lane's base of that k-step's kind (ConvAllco::xbase)
template <typename Cf, int ST, int NI>
__device__ __forceinline__ void allco_read_x(bf16x8& xf, const bf16_t* pb) {
    lds_read_async_b128<NI * 16 * Cf::KC * 2 + Cf::xconst(ST)>(xf, pb);
}

template <int NM, int TW, int NGRP>
__global__ void __launch_bounds__(kBigThreads, 2)
conv3x3_bf16_allco_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wp, const float* __restrict__ scale,
                          const float* __restrict__ shift, const bf16_t* __restrict__ zero_page, int Th, int Fw, int Cin, int Cout, int tiles_t,
                          int tiles_f, int ntiles) {
    typedef ConvAllco<NM, TW, NGRP> Cf;
    bf16_t* const patch0 = reinterpret_cast<bf16_t*>(alsep_smem);
    bf16_t* const wring = patch0 + (size_t)2 * Cf::PBUF * 8;
    float* ss = reinterpret_cast<float*>(alsep_smem + Cf::ring_bytes);
    bf16_t* const scratch = reinterpret_cast<bf16_t*>(alsep_smem + Cf::lds_bytes - 1024);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // wave: in a scalar register
    const int l15 = lane & 15, lq = lane >> 4;
    const int nq = Cin / Cf::KC;
    for (int i = tid; i < Cf::COUT; i += kBigThreads) {
        ss[i] = scale[i];
        ss[Cf::COUT + i] = shift[i];
    }
    __syncthreads();

    int xb[3];                                               // elements
#pragma unroll
    for (int kind = 0; kind < 3; ++kind) xb[kind] = Cf::xbase(kind, wave, l15, lq) / 2;
    const int wl_off = l15 * 32 + (lq ^ Cf::wswz(l15)) * 8;

    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int npatch = my_tiles * Cf::NGRP * nq;             // a patch per (item, chunk); item it = (tile it / NGRP, group it % NGRP)
    auto tile_coords = [&](int k, int& t0, int& f0, int64_t& b) {
        int tile = (int)blockIdx.x + k * (int)gridDim.x;
        const int tf = tile % tiles_f;  tile /= tiles_f;
        const int tt = tile % tiles_t;
        b = tile / tiles_t;
        t0 = tt * Cf::TH;
        f0 = tf * Cf::TW;
    };
    // LDS-DMA descriptors of a halo patch, computed once (see conv3x3_bf16_m0_kernel)
    int prel[Cf::PJ];
    unsigned pflags[(Cf::PJ + 5) / 6] = {};                  // 5 bits per piece, 6 pieces per word
#pragma unroll
    for (int j = 0; j < Cf::PJ; ++j) {
        const int u = (wave + 8 * j) * 64 + lane;
        const int uu = u < Cf::PGROUPS ? u : Cf::PGROUPS - 1;
        const int P = uu / Cf::CG, cg = uu % Cf::CG;
        const int dt = P / Cf::PW - 1, df = P % Cf::PW - 1;
        prel[j] = (dt * Fw + df) * Cin + cg * 8;
        pflags[j / 6] |= (u < Cf::PGROUPS ? (unsigned)((dt < 0) | ((dt >= Cf::TH) << 1) | ((df < 0) << 2) | ((df >= Cf::TW) << 3)) : 16u) << (5 * (j % 6));
    }
    // patch ps (item ps / nq, chunk ps % nq) -> buffer ps & 1; past the last patch the last one is fetched again into the free buffer
    const bf16_t* psrc = X;
    unsigned pborder = 0;
    bf16_t* pdst = patch0;
    auto patch_prep = [&](int ps) {
        const int pc = ps < npatch ? ps : npatch - 1;
        int t0, f0; int64_t b;
        tile_coords(pc / nq / Cf::NGRP, t0, f0, b);
        psrc = X + ((b * Th + t0) * (int64_t)Fw + f0) * Cin + (pc % nq) * Cf::KC;
        pborder = (unsigned)(t0 == 0) | ((unsigned)(t0 + Cf::TH >= Th) << 1) | ((unsigned)(f0 == 0) << 2) | ((unsigned)(f0 + Cf::TW >= Fw) << 3);
        pdst = patch0 + (size_t)(ps & 1) * Cf::PBUF * 8;
    };
    auto patch_one = [&](int j) {
        const int i = wave + 8 * j;
        const bool out = (pflags[j / 6] & ((pborder | 16u) << (5 * (j % 6)))) != 0;
        const bool real = j < Cf::PJ - 1 || i < Cf::PINST;
        const bf16_t* src = (out || !real) ? zero_page : psrc + opaque_vgpr(prel[j]);      // opaque: sign-extended here, not kept as a pair
        glds16(src, real ? pdst + (size_t)i * 64 * 8 : scratch);
    };
    // weights of stage sc of chunk q of group g -> ring slot: this wave's eighth, WJ instructions (the last one with WLAST lanes)
    const unsigned wlane = lane * 8;                         // elements
    const bf16_t* wsrc_next = Wp;                            // wave-uniform: scalar base + 32-bit lane offset
    bf16_t* wdst_next = wring;
    auto weights_prep = [&](int g, int q, int sc, int slot) {
        const int gq = Cf::NGRP > 1 ? g * nq + q : q;        // group images one after another, nq chunks each
        wsrc_next = Wp + ((size_t)gq * Cf::NSTG + sc) * (Cf::SLOT_BYTES / 2) + wave * (Cf::WPW / 2);
        wdst_next = wring + (size_t)slot * (Cf::SLOT_BYTES / 2) + wave * (Cf::WPW / 2);
    };
    auto weights_one = [&](int j) {
        if (j < Cf::WJ - 1 || Cf::WLAST == 64 || lane < Cf::WLAST) glds16(wsrc_next + (wlane + j * 512u), wdst_next + j * 512);
    };

    f32x4 acc[Cf::NB][Cf::NI];
    bf16x8 xf[Cf::NI], wf[2][Cf::G];
    // the reads of a k-step's first unit, always requested in this order: its weight fragments, then the patch fragments
    auto read_first = [&](const bf16_t* patch, const bf16_t* wl) {
        allco_read_w<Cf, 0>(wf, wl);
        static_for<Cf::NI>([&](auto nic) { allco_read_x<Cf, 0, decltype(nic)::value>(xf[decltype(nic)::value], patch + xb[0]); });
    };
    if (npatch > 0) {
        patch_prep(0);
#pragma unroll
        for (int j = 0; j < Cf::PJ; ++j) patch_one(j);
#pragma unroll
        for (int d = 0; d < Cf::DIST; ++d) {
            weights_prep(0, 0, d, d);
#pragma unroll
            for (int j = 0; j < Cf::WJ; ++j) weights_one(j);
        }
        wait_vmcnt<0>();
        barrier_nodrain();                                   // patch 0 and stages 0 .. DIST - 1 are in LDS for every wave
        read_first(patch0, wring + wl_off);
    }
    // block pairs outermost: a pair's scale / shift quads are read once and are dead before the next pair's (held across the pixel
    // blocks for all pairs at once they are 8 NB registers that the accumulators leave no room for)
    auto epilogue = [&](int k, int g) {
        int t0, f0; int64_t b;
        tile_coords(k, t0, f0, b);
        // the lane's coordinates again, opaque: everything the stores derive from them is computed here, not kept across the k-loops
        const int le = opaque_vgpr(lane), l15 = le & 15, lq = le >> 4;
        const int c0 = Cf::NGRP > 1 ? g * Cf::ROWS : 0;      // the group's first channel
        bf16_t* yb = Y + ((b * Th + t0 + wave) * (int64_t)Fw + f0 + l15) * Cout + c0;
        const float* const ssg = ss + c0;                    // the group's scale rows; its shift rows are COUT further on
#pragma unroll
        for (int j = 0; j < Cf::NPAIR; ++j) {                // blocks 2 j, 2 j + 1: channels 32 j + 8 lq + [0, 8) (ConvBig::channel_of_row)
            const int co = j * 32 + lq * 8;
            f32x4 scv[2], shv[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                scv[h] = *reinterpret_cast<const f32x4*>(ssg + co + 4 * h);
                shv[h] = *reinterpret_cast<const f32x4*>(ssg + Cf::COUT + co + 4 * h);
            }
#pragma unroll
            for (int ni = 0; ni < Cf::NI; ++ni) {
                float y[8];
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[4 * h + r] = fmaxf(fmaf(acc[2 * j + h][ni][r], scv[h][r], shv[h][r]), 0.f);
                store8(yb + (int64_t)ni * 16 * Cout + co, y);
            }
        }
        if constexpr (Cf::NB % 2 == 1) {
            constexpr int bb = Cf::NB - 1;
            const int co = bb * 16 + lq * 4;
            const f32x4 scv = *reinterpret_cast<const f32x4*>(ssg + co);
            const f32x4 shv = *reinterpret_cast<const f32x4*>(ssg + Cf::COUT + co);
#pragma unroll
            for (int ni = 0; ni < Cf::NI; ++ni) {
                float y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(acc[bb][ni][r], scv[r], shv[r]), 0.f);
                store4(yb + (int64_t)ni * 16 * Cout + co, y);
            }
        }
    };

    // Stage (p, sc): k-steps KS sc .. of patch p (item p / nq = (tile k, group g), chunk q = p % nq); its weights sit in slot
    // (p NSTG + sc) % NSLOT.  Issued in it, in this order: the weights of stage + DIST (into the slot that the stage before this one has
    // just left), one piece of patch p + 1, and after the last stage of an item that item's stores.  vmcnt counts in order, so the wait
    // at the barrier of a stage allows exactly what the DIST - 2 stages before it issued (Cf::inflight_at) and, behind those, a finished
    // item's stores.
    int slot = 0, q = 0, k = 0, g = 0;                       // ring slot of the current stage; chunk, tile and group of the current patch
    for (int p = 0; p < npatch; ++p) {
        const bf16_t* const patch = patch0 + (size_t)(p & 1) * Cf::PBUF * 8;
        const bf16_t* const patch_nx = patch0 + (size_t)((p + 1) & 1) * Cf::PBUF * 8;
        const int qn = q + 1 == nq ? 0 : q + 1;
        const int gn = Cf::NGRP > 1 && qn == 0 ? (g + 1 == Cf::NGRP ? 0 : g + 1) : g;      // the group of patch p + 1
        static_for<Cf::NSTG>([&](auto scc) {
            constexpr int sc = decltype(scc)::value;
            if (sc < Cf::DIST - 1 && q == 0 && p > 0) wait_vmcnt<Cf::inflight_at(sc) + Cf::ST>();    // an item ended inside the window
            else wait_vmcnt<Cf::inflight_at(sc)>();
            // raw barrier, no lgkmcnt(0) in front of it: the only LDS reads in flight are those of the next unit, from a slot and a patch
            // buffer that no wave writes before the barrier after this one
            __builtin_amdgcn_s_barrier();
            const int slot_prev = slot == 0 ? Cf::NSLOT - 1 : slot - 1, slot_nx = slot + 1 == Cf::NSLOT ? 0 : slot + 1;
            weights_prep((sc + Cf::DIST) / Cf::NSTG ? gn : g, (sc + Cf::DIST) / Cf::NSTG ? qn : q, (sc + Cf::DIST) % Cf::NSTG, slot_prev);
            if (sc == 0) {
                patch_prep(p + 1);
                if (q == 0) {
#pragma unroll
                    for (int b = 0; b < Cf::NB; ++b)
#pragma unroll
                        for (int ni = 0; ni < Cf::NI; ++ni) acc[b][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
            const bf16_t* const wl = wring + (size_t)slot * (Cf::SLOT_BYTES / 2) + wl_off;
            const bf16_t* const wl_nx = wring + (size_t)slot_nx * (Cf::SLOT_BYTES / 2) + wl_off;
            static_for<Cf::UPS>([&](auto uic) {
                constexpr int ui = decltype(uic)::value, U = sc * Cf::UPS + ui, t = U % Cf::UPK, st = U / Cf::UPK;
                constexpr bool chunk_end = U + 1 == Cf::UPK * Cf::NS;
                constexpr int U1 = chunk_end ? 0 : U + 1, st1 = U1 / Cf::UPK;     // the chunk's last unit requests nothing: see below
                // in flight, in order: this unit's weight fragments and, with t = 0, the patch fragments behind them
                if constexpr (t == 0) lds_wait_n<Cf::NI - 1>();
                else lds_wait_n<0>();
                if constexpr (!chunk_end) allco_read_w<Cf, U1>(wf, ui + 1 < Cf::UPS ? wl : wl_nx);
                if constexpr (t == 0) {
                    // pixel blocks outermost: block ni may still be on its way behind ni - 1
                    static_for<Cf::NI>([&](auto nic) {
                        constexpr int ni = decltype(nic)::value;
                        if constexpr (ni > 0) lds_wait_n<Cf::G + Cf::NI - 1 - ni>();
#pragma unroll
                        for (int g = 0; g < Cf::G; ++g) mma_step(acc[t * Cf::G + g][ni], wf[U & 1][g], xf[ni]);
                    });
                } else if constexpr (t == Cf::UPK - 1 && !chunk_end) {
                    // the k-step's last unit, pixel blocks outermost: a patch fragment that has fed its last MFMA is requested again
                    // for the next k-step into the same registers (one set of patch fragments, not two)
                    const bf16_t* const pb = patch + xb[Cf::xkind(st1)];
                    static_for<Cf::NI>([&](auto nic) {
                        constexpr int ni = decltype(nic)::value;
#pragma unroll
                        for (int g = 0; g < Cf::G; ++g) mma_step(acc[t * Cf::G + g][ni], wf[U & 1][g], xf[ni]);
                        sched_fence();
                        allco_read_x<Cf, st1, ni>(xf[ni], pb);
                    });
                } else {
#pragma unroll
                    for (int g = 0; g < Cf::G; ++g)
#pragma unroll
                        for (int ni = 0; ni < Cf::NI; ++ni) mma_step(acc[t * Cf::G + g][ni], wf[U & 1][g], xf[ni]);
                }
                if constexpr (ui < Cf::WJ) weights_one(ui);
                if constexpr (ui == Cf::WJ && sc < Cf::PJ) patch_one(sc);
                sched_fence();
            });
            slot = slot_nx;
            if (sc == Cf::NSTG - 1 && q == nq - 1) epilogue(k, g);
        });
        // the first fragments of the next patch, behind the epilogue: 24 registers that the stores' arithmetic needs (after the last
        // patch they are read from the refetched copy and never used)
        read_first(patch_nx, wring + (size_t)slot * (Cf::SLOT_BYTES / 2) + wl_off);
        q = qn;
        g = gn;
        if (q == 0 && g == 0) ++k;                           // the tile's last group is done
    }
    lds_wait_n<0>();
    wait_vmcnt<0>();                                         // the surplus LDS-DMA of the last stages lands before the wave ends
}

#ifndef ALSEP_F16_TU
#include "tdfnet_f32s.h"     // float32 storage with split-half contractions (the float32 network lives in the main translation unit)
#endif

// ------------------------------------------------------------------------------------------
// host side: packing + orchestration
// ------------------------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

struct ConvLayer {       // 3x3
    DevBuf w, scale, shift;
    DevBuf w_big;            // rows in ConvBig::channel_of_row order: conv3x3_bf16_m0_kernel's image (c = 48), conv3x3_bf16_big_kernel<3>'s (c = 144)
    DevBuf w_mq;             // conv3x3_bf16_mq_kernel's image (c = 96)
    DevBuf w_ac;             // conv3x3_bf16_allco_kernel's k-step-major image (c = 144; c = 192 / 288: one image per group of 96 rows)
    int cin = 0, cout = 0;
    bool dma_path = false;   // packed for conv3x3_bf16_kernel (swizzled, unpadded)
    int split = 0;           // float32 storage, split-half contraction (tdfnet_f32s.h): 24 = <24, 48> tiles, 16 = <16, 16>
    unsigned* range_flag = nullptr;   // the network's range word (split layers)
};
struct GemmLayer {       // ds / us / tdf
    DevBuf w, bias, scale, shift;
    int M = 0, K = 0, Kp = 0, Mp = 0;
    bool has_bias = false;
    bool split = false;      // float32 storage, split-half contraction: w = [hi | lo][Mp][Kp] halves (tdfnet_f32s.h)
    unsigned* range_flag = nullptr;
    bool dma_path = false;   // packed for tdf_bf16_kernel
    DevBuf wfrag;            // [m-tile][k-step][lane][8] for the streaming ds/us kernels (bf16, levels 0 <-> 1 <-> 2)
    DevBuf wwide;            // fragment-order image for tdf_bf16_wide_kernel (bf16, M % 192 == 0)
};
struct Block {
    std::vector<ConvLayer> tfc;
    std::vector<GemmLayer> tdf;
};

}  // namespace

struct alsep_net {
    alsep_ctx* ctx = nullptr;
    alsep_net_config cfg{};
    int n = 0;
    bool split = false;      // cfg.flags & ALSEP_NET_SPLIT_F16 on a float32 network
    DevBuf range_flag;       // split networks: one word the kernels raise when an operand leaves the half range
    std::vector<DevBuf> owned;
    DevBuf first_w, first_scale, first_shift, final_w, final_b, zero_page;
    std::vector<Block> enc, dec;
    Block bott;
    std::vector<GemmLayer> ds, us;
};

namespace {

typedef std::map<std::string, std::vector<float>> TensorMap;

template <typename T> T host_cast(float v);
template <> float host_cast<float>(float v) { return v; }
template <> bf16_t host_cast<bf16_t>(float v) { return (bf16_t)v; }

int upload(alsep_net* net, const void* src, size_t bytes, DevBuf* out) {
    void* d = nullptr;
    if (hipMalloc(&d, bytes ? bytes : 16) != hipSuccess) return alsep_fail(net->ctx, ALSEP_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    out->p = d;
    out->bytes = bytes;
    net->owned.push_back(*out);
    if (bytes) ALSEP_HIP(net->ctx, hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    return ALSEP_OK;
}

const std::vector<float>* find(const TensorMap& tm, const std::string& name, int64_t numel, alsep_ctx* ctx, bool required = true) {
    auto it = tm.find(name);
    if (it == tm.end()) {
        if (required) alsep_fail(ctx, ALSEP_ERR_ARG, "missing tensor '%s'", name.c_str());
        return nullptr;
    }
    if ((int64_t)it->second.size() != numel) {
        alsep_fail(ctx, ALSEP_ERR_ARG, "tensor '%s' has %zu elements, expected %lld", name.c_str(), it->second.size(), (long long)numel);
        return nullptr;
    }
    return &it->second;
}

// conv tile parameters per dtype (must match the launch in run_conv)
template <typename T> struct ConvSel;
template <> struct ConvSel<bf16_t> { static constexpr int KC = 48, BN = 48; };
template <> struct ConvSel<float> { static constexpr int KC = 16, BN = 48; };
// fall-back tiles for channel counts that are multiples of 16 / 32 only
template <typename T> struct ConvSel16;
template <> struct ConvSel16<bf16_t> { static constexpr int KC = 16, BN = 16; };
template <> struct ConvSel16<float> { static constexpr int KC = 16, BN = 16; };

template <typename T> bool conv_uses_main(int cin, int cout) {
    return cin % ConvSel<T>::KC == 0 && cout % ConvSel<T>::BN == 0;
}

template <typename T, int KC, int BN>
std::vector<T> pack_conv3x3(const std::vector<float>& w, int cin, int cout) {
    typedef ConvCfg<T, KC, BN, 64> Cf;      // KP, CG, NG do not depend on TW
    const int nq = cin / KC, nn = cout / BN;
    std::vector<T> out((size_t)nn * nq * BN * Cf::KP, host_cast<T>(0.f));
    for (int j = 0; j < nn; ++j)
        for (int q = 0; q < nq; ++q)
            for (int r = 0; r < BN; ++r)
                for (int grp = 0; grp < Cf::NG; ++grp)
                    for (int e = 0; e < Cf::G; ++e) {
                        const int tap = grp / Cf::CG, cg = grp % Cf::CG;
                        const int ci = q * KC + cg * Cf::G + e, co = j * BN + r;
                        const float v = w[(((size_t)co * cin + ci) * 3 + tap / 3) * 3 + tap % 3];
                        out[(((size_t)j * nq + q) * BN + r) * Cf::KP + grp * Cf::G + e] = host_cast<T>(v);
                    }
    return out;
}

// packed image for conv3x3_bf16_kernel: [ny][q][48 rows][56 groups of 8], group index XOR (row>>1)&7
std::vector<bf16_t> pack_conv3x3_dma(const std::vector<float>& w, int cin, int cout) {
    typedef ConvB16<64> Cf;
    const int nq = cin / Cf::KC, nn = cout / Cf::BN;
    std::vector<bf16_t> out((size_t)nn * nq * Cf::WGROUPS * 8, host_cast<bf16_t>(0.f));
    for (int j = 0; j < nn; ++j)
        for (int q = 0; q < nq; ++q)
            for (int r = 0; r < Cf::BN; ++r)
                for (int grp = 0; grp < Cf::NG; ++grp)
                    for (int e = 0; e < 8; ++e) {
                        const int tap = grp / Cf::CG, cg = grp % Cf::CG;
                        const int ci = q * Cf::KC + cg * 8 + e, co = j * Cf::BN + r;
                        const float v = w[(((size_t)co * cin + ci) * 3 + tap / 3) * 3 + tap % 3];
                        const int pg = grp ^ ((r >> 1) & 7);
                        out[((((size_t)j * nq + q) * Cf::BN + r) * Cf::WG + pg) * 8 + e] = host_cast<bf16_t>(v);
                    }
    return out;
}

// the same image with the output channels in the row order of conv3x3_bf16_big_kernel<NY> (ConvBig::channel_of_row)
template <int NY>
std::vector<bf16_t> pack_conv3x3_big(const std::vector<float>& w, int cin) {
    const int cout = 48 * NY;
    std::vector<float> wp(w.size());
    const size_t row = (size_t)cin * 9;
    for (int R = 0; R < cout; ++R) std::copy(w.begin() + ConvBig<NY>::channel_of_row(R) * row, w.begin() + (ConvBig<NY>::channel_of_row(R) + 1) * row, wp.begin() + R * row);
    return pack_conv3x3_dma(wp, cin, cout);
}

// image of conv3x3_bf16_mq_kernel (c_out = 96): [q][part][96 rows][20 groups][8]; k-step stl of part pt is tap 5 pt + stl, its group lq
// (input channels 32 q + 8 lq ..) sits at 4 stl + (lq ^ wswz(R)); row R holds output channel ConvBig<2>::channel_of_row(R)
std::vector<bf16_t> pack_conv3x3_mq(const std::vector<float>& w, int cin) {
    typedef ConvMq Cf;
    const int nq = cin / Cf::KC;
    std::vector<bf16_t> out((size_t)nq * Cf::PARTS * Cf::WGROUPS * 8, host_cast<bf16_t>(0.f));
    for (int q = 0; q < nq; ++q)
        for (int pt = 0; pt < Cf::PARTS; ++pt)
            for (int R = 0; R < Cf::ROWS; ++R)
                for (int stl = 0; stl < Cf::ksteps_of_part(pt); ++stl)
                    for (int lq = 0; lq < 4; ++lq) {
                        const int tap = pt * Cf::KS + stl, co = ConvBig<2>::channel_of_row(R);
                        const size_t dst = ((((size_t)q * Cf::PARTS + pt) * Cf::ROWS + R) * Cf::WG + 4 * stl + (lq ^ Cf::wswz(R))) * 8;
                        for (int e = 0; e < 8; ++e) {
                            const int ci = q * Cf::KC + lq * 8 + e;
                            out[dst + e] = host_cast<bf16_t>(w[(((size_t)co * cin + ci) * 3 + tap / 3) * 3 + tap % 3]);
                        }
                    }
    return out;
}

// image of conv3x3_bf16_allco_kernel (c_out = 16 NM): [q][k-step st][16 NM rows][4 groups][8]; row R holds output channel
// ConvBig<NM / 3>::channel_of_row(R), its group 4 st + lq (tap-major in the 48-channel chunk q, groups 54 and 55 zero) sits at
// position lq ^ wswz(R)
template <int NM>
std::vector<bf16_t> pack_conv3x3_allco(const std::vector<float>& w, int cin) {
    typedef ConvAllco<NM, 48> Cf;                           // the image does not depend on TW
    const int nq = cin / Cf::KC;
    std::vector<bf16_t> out((size_t)nq * Cf::NS * Cf::ROWS * 32, host_cast<bf16_t>(0.f));
    for (int q = 0; q < nq; ++q)
        for (int st = 0; st < Cf::NS; ++st)
            for (int R = 0; R < Cf::ROWS; ++R)
                for (int lq = 0; lq < 4; ++lq) {
                    const int grp = 4 * st + lq;
                    if (grp >= Cf::NG) continue;
                    const int tap = grp / Cf::CG, cg = grp % Cf::CG, co = ConvBig<NM / 3>::channel_of_row(R);
                    const size_t dst = ((((size_t)q * Cf::NS + st) * Cf::ROWS + R) * 4 + (lq ^ Cf::wswz(R))) * 8;
                    for (int e = 0; e < 8; ++e) {
                        const int ci = q * Cf::KC + cg * 8 + e;
                        out[dst + e] = host_cast<bf16_t>(w[(((size_t)co * cin + ci) * 3 + tap / 3) * 3 + tap % 3]);
                    }
                }
    return out;
}

template <typename T> constexpr bool is_bf16() { return false; }
template <> constexpr bool is_bf16<bf16_t>() { return true; }

template <typename T>
int make_conv(alsep_net* net, const TensorMap& tm, const std::string& p, int c, ConvLayer* L) {
    auto w = find(tm, p + ".weight", (int64_t)c * c * 9, net->ctx);
    auto sc = find(tm, p + ".scale", c, net->ctx);
    auto sh = find(tm, p + ".shift", c, net->ctx);
    if (!w || !sc || !sh) return ALSEP_ERR_ARG;
    L->cin = L->cout = c;
    int rc;
#ifndef ALSEP_F16_TU
    if (!is_bf16<T>() && net->split && (c % 48 == 0 || c % 16 == 0)) {
        L->split = c % 48 == 0 ? 24 : 16;
        L->range_flag = (unsigned*)net->range_flag.p;
        const std::vector<hs_t> pk = L->split == 24 ? pack_conv3x3_split<24, 48>(*w, c, c) : pack_conv3x3_split<16, 16>(*w, c, c);
        rc = upload(net, pk.data(), pk.size() * sizeof(hs_t), &L->w);
    } else
#endif
    if (is_bf16<T>() && c % 48 == 0) {
        L->dma_path = true;
        auto pk = pack_conv3x3_dma(*w, c, c);
        rc = upload(net, pk.data(), pk.size() * sizeof(bf16_t), &L->w);
        // a second image for the level's 8-wave persistent kernel (its own output-channel order)
        if (!rc && c == 48) {                                // level 0: the LDS-resident-weight kernel
            auto p0 = pack_conv3x3_big<1>(*w, c);
            rc = upload(net, p0.data(), p0.size() * sizeof(bf16_t), &L->w_big);
        }
        if (!rc && c == 96) {                                // level 1: the double-buffered kernel
            auto pq = pack_conv3x3_mq(*w, c);
            rc = upload(net, pq.data(), pq.size() * sizeof(bf16_t), &L->w_mq);
        }
        if (!rc && c == 144) {                               // level 2: the big-tile kernel
            auto pb = pack_conv3x3_big<3>(*w, c);
            rc = upload(net, pb.data(), pb.size() * sizeof(bf16_t), &L->w_big);
        }
        if (!rc && c == 144) {                               // level 2 again: the all-channels kernel
            auto pa = pack_conv3x3_allco<9>(*w, c);
            rc = upload(net, pa.data(), pa.size() * sizeof(bf16_t), &L->w_ac);
        }
        if (!rc && (c == 192 || c == 288)) {                 // the all-channels kernel in output groups of 96 rows: one image per group
            std::vector<bf16_t> pa;
            const size_t slice = (size_t)96 * c * 9;
            for (int g = 0; g < c / 96; ++g) {
                auto pg = pack_conv3x3_allco<6>(std::vector<float>(w->begin() + g * slice, w->begin() + (g + 1) * slice), c);
                pa.insert(pa.end(), pg.begin(), pg.end());
            }
            rc = upload(net, pa.data(), pa.size() * sizeof(bf16_t), &L->w_ac);
        }
    } else if (conv_uses_main<T>(c, c)) {
        auto pk = pack_conv3x3<T, ConvSel<T>::KC, ConvSel<T>::BN>(*w, c, c);
        rc = upload(net, pk.data(), pk.size() * sizeof(T), &L->w);
    } else {
        auto pk = pack_conv3x3<T, ConvSel16<T>::KC, ConvSel16<T>::BN>(*w, c, c);
        rc = upload(net, pk.data(), pk.size() * sizeof(T), &L->w);
    }
    if (rc) return rc;
    if ((rc = upload(net, sc->data(), c * sizeof(float), &L->scale))) return rc;
    return upload(net, sh->data(), c * sizeof(float), &L->shift);
}

// pack a [M][K] row-major fp32 matrix into [Mp][Kp] of T, zero padded to tile multiples
template <typename T>
int make_gemm_weights(alsep_net* net, const std::vector<float>& wmk, int M, int K, GemmLayer* L) {
    typedef GemmCfg<T> Gc;
    L->M = M; L->K = K;
#ifndef ALSEP_F16_TU
    if (!is_bf16<T>() && net->split) {
        L->split = true;
        L->range_flag = (unsigned*)net->range_flag.p;
        const std::vector<hs_t> pk = pack_gemm_split(wmk, M, K, &L->Mp, &L->Kp);
        return upload(net, pk.data(), pk.size() * sizeof(hs_t), &L->w);
    }
#endif
    L->Mp = (int)ceil_div64(M, Gc::BR) * Gc::BR;
    L->Kp = (int)ceil_div64(K, Gc::BK) * Gc::BK;
    std::vector<T> pk((size_t)L->Mp * L->Kp, host_cast<T>(0.f));
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < K; ++k) pk[(size_t)m * L->Kp + k] = host_cast<T>(wmk[(size_t)m * K + k]);
    return upload(net, pk.data(), pk.size() * sizeof(T), &L->w);
}

// packed image for tdf_bf16_kernel: [Mp=ceil128][Kp=ceil64]; inside every 64-wide k tile the eight
// 16-byte groups are stored at (group ^ ((row>>1)&7)); group (ks, lq) holds, for a 32-wide k-step ks,
// k = {4lq..4lq+3, 16+4lq..16+4lq+3} (the order the transposed activation reads deliver).
int make_tdf_dma_weights(alsep_net* net, const std::vector<float>& wmk, int M, int K, GemmLayer* L) {
    typedef TdfB16 Tc;
    L->M = M; L->K = K;
    L->Mp = (int)ceil_div64(M, Tc::BM) * Tc::BM;
    L->Kp = (int)ceil_div64(K, Tc::BK) * Tc::BK;
    L->dma_path = true;
    std::vector<bf16_t> pk((size_t)L->Mp * L->Kp, host_cast<bf16_t>(0.f));
    for (int m = 0; m < M; ++m)
        for (int kt = 0; kt < L->Kp / Tc::BK; ++kt)
            for (int g = 0; g < 8; ++g) {
                const int ks = g >> 2, lq = g & 3, pg = g ^ ((m >> 1) & 7);
                for (int e = 0; e < 8; ++e) {
                    const int k = kt * Tc::BK + ks * 32 + (e < 4 ? 4 * lq + e : 16 + 4 * lq + (e - 4));
                    if (k < K) pk[(size_t)m * L->Kp + kt * Tc::BK + pg * 8 + e] = host_cast<bf16_t>(wmk[(size_t)m * K + k]);
                }
            }
    return upload(net, pk.data(), pk.size() * sizeof(bf16_t), &L->w);
}

// fragment-order image for tdf_bf16_wide_kernel: [M/48][Kp/64][k-step 2][m-tile 3][lane 64][8]; lane (l15, lq) of
// (m-tile mi, k-step ks) holds W[48 rb + 16 mi + l15][64 kt + 32 ks + {4lq..4lq+3, 16+4lq..16+4lq+3}] -- the same
// k order as the LDS image above, so both kernels sum in the same order.
int make_tdf_wide_weights(alsep_net* net, const std::vector<float>& wmk, int M, int K, GemmLayer* L) {
    const int KT = (int)ceil_div64(K, 64);
    std::vector<bf16_t> pk((size_t)(M / 48) * KT * 6 * 512, host_cast<bf16_t>(0.f));
    for (int rb = 0; rb < M / 48; ++rb)
        for (int kt = 0; kt < KT; ++kt)
            for (int ks = 0; ks < 2; ++ks)
                for (int mi = 0; mi < 3; ++mi)
                    for (int l = 0; l < 64; ++l)
                        for (int e = 0; e < 8; ++e) {
                            const int lq = l >> 4, m = rb * 48 + mi * 16 + (l & 15);
                            const int k = kt * 64 + ks * 32 + (e < 4 ? 4 * lq + e : 16 + 4 * lq + (e - 4));
                            if (k < K)
                                pk[((((size_t)rb * KT + kt) * 2 + ks) * 3 + mi) * 512 + l * 8 + e] =
                                    host_cast<bf16_t>(wmk[(size_t)m * K + k]);
                        }
    return upload(net, pk.data(), pk.size() * sizeof(bf16_t), &L->wwide);
}

// fragment-order image of a [M][K] matrix for register-resident A operands: lane l of (m-tile, k-step) holds
// W[16*mt + (l & 15)][32*ks + 8*(l >> 4) + e], e < 8 (zero beyond M / K)
int make_frag_weights(alsep_net* net, const std::vector<float>& wmk, int M, int K, DevBuf* out) {
    const int MT = (M + 15) / 16, KS = (K + 31) / 32;
    std::vector<bf16_t> pk((size_t)MT * KS * 64 * 8, host_cast<bf16_t>(0.f));
    for (int mt = 0; mt < MT; ++mt)
        for (int ks = 0; ks < KS; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int m = mt * 16 + (l & 15), k = ks * 32 + (l >> 4) * 8 + e;
                    if (m < M && k < K) pk[(((size_t)mt * KS + ks) * 64 + l) * 8 + e] = host_cast<bf16_t>(wmk[(size_t)m * K + k]);
                }
    return upload(net, pk.data(), pk.size() * sizeof(bf16_t), out);
}

template <typename T>
int make_block(alsep_net* net, const TensorMap& tm, const std::string& p, int c, int f, Block* blk) {
    const alsep_net_config& cfg = net->cfg;
    blk->tfc.resize(cfg.l);
    for (int j = 0; j < cfg.l; ++j) {
        int rc = make_conv<T>(net, tm, p + ".tfc." + std::to_string(j), c, &blk->tfc[j]);
        if (rc) return rc;
    }
    const int n_lin = cfg.bn == 0 ? 1 : 2;
    blk->tdf.resize(n_lin);
    for (int j = 0; j < n_lin; ++j) {
        const int fi = (j == 0) ? f : f / cfg.bn;
        const int fo = (n_lin == 1 || j == 1) ? f : f / cfg.bn;
        const std::string q = p + ".tdf." + std::to_string(j);
        auto w = find(tm, q + ".weight", (int64_t)fo * fi, net->ctx);
        auto sc = find(tm, q + ".scale", c, net->ctx);
        auto sh = find(tm, q + ".shift", c, net->ctx);
        if (!w || !sc || !sh) return ALSEP_ERR_ARG;
        GemmLayer* L = &blk->tdf[j];
        int rc = (is_bf16<T>() && c % 48 == 0) ? make_tdf_dma_weights(net, *w, fo, fi, L)
                                               : make_gemm_weights<T>(net, *w, fo, fi, L);
        if (rc) return rc;
        if (L->dma_path && fo % 192 == 0 && (rc = make_tdf_wide_weights(net, *w, fo, fi, L))) return rc;
        if ((rc = upload(net, sc->data(), c * sizeof(float), &L->scale))) return rc;
        if ((rc = upload(net, sh->data(), c * sizeof(float), &L->shift))) return rc;
        auto bi = find(tm, q + ".bias", fo, net->ctx, false);
        if (tm.count(q + ".bias") && !bi) return ALSEP_ERR_ARG;
        L->has_bias = bi != nullptr;
        if (bi && (rc = upload(net, bi->data(), fo * sizeof(float), &L->bias))) return rc;
    }
    return ALSEP_OK;
}

template <typename T>
int build_net(alsep_net* net, const TensorMap& tm) {
    const alsep_net_config& cfg = net->cfg;
    alsep_ctx* ctx = net->ctx;
    const int g = cfg.g, n = net->n;
    int rc;
    {
        auto w = find(tm, "first_conv.weight", (int64_t)g * 4, ctx);
        auto sc = find(tm, "first_conv.scale", g, ctx);
        auto sh = find(tm, "first_conv.shift", g, ctx);
        if (!w || !sc || !sh) return ALSEP_ERR_ARG;
        if ((rc = upload(net, w->data(), w->size() * 4, &net->first_w))) return rc;
        if ((rc = upload(net, sc->data(), g * 4, &net->first_scale))) return rc;
        if ((rc = upload(net, sh->data(), g * 4, &net->first_shift))) return rc;
        auto fw = find(tm, "final_conv.weight", (int64_t)4 * g, ctx);
        auto fb = find(tm, "final_conv.bias", 4, ctx);
        if (!fw || !fb) return ALSEP_ERR_ARG;
        if ((rc = upload(net, fw->data(), fw->size() * 4, &net->final_w))) return rc;
        if ((rc = upload(net, fb->data(), 16, &net->final_b))) return rc;
        const std::vector<char> zeros(256, 0);
        if ((rc = upload(net, zeros.data(), zeros.size(), &net->zero_page))) return rc;
        if ((rc = upload(net, zeros.data(), 16, &net->range_flag))) return rc;
    }
    net->enc.resize(n); net->dec.resize(n); net->ds.resize(n); net->us.resize(n);
    int c = g, f = cfg.dim_f;
    for (int i = 0; i < n; ++i) {
        if ((rc = make_block<T>(net, tm, "encoding_blocks." + std::to_string(i), c, f, &net->enc[i]))) return rc;
        // ds: torch Conv2d weight [c+g][c][2][2] -> rows co, k = (dy*2+dx)*c + ci
        const int c2 = c + g;
        const std::string p = "ds." + std::to_string(i);
        auto w = find(tm, p + ".weight", (int64_t)c2 * c * 4, ctx);
        auto sc = find(tm, p + ".scale", c2, ctx);
        auto sh = find(tm, p + ".shift", c2, ctx);
        if (!w || !sc || !sh) return ALSEP_ERR_ARG;
        std::vector<float> mk((size_t)c2 * 4 * c);
        for (int co = 0; co < c2; ++co)
            for (int ci = 0; ci < c; ++ci)
                for (int d = 0; d < 4; ++d) mk[(size_t)co * 4 * c + d * c + ci] = (*w)[((size_t)co * c + ci) * 4 + d];
        if ((rc = make_gemm_weights<T>(net, mk, c2, 4 * c, &net->ds[i]))) return rc;
        if (is_bf16<T>() && (c == 48 || c == 96 || c == 144) && (rc = make_frag_weights(net, mk, c2, 4 * c, &net->ds[i].wfrag))) return rc;
        if ((rc = upload(net, sc->data(), c2 * 4, &net->ds[i].scale))) return rc;
        if ((rc = upload(net, sh->data(), c2 * 4, &net->ds[i].shift))) return rc;
        c = c2; f /= 2;
    }
    if ((rc = make_block<T>(net, tm, "bottleneck_block", c, f, &net->bott))) return rc;
    for (int i = 0; i < n; ++i) {
        // us: torch ConvTranspose2d weight [c][c-g][2][2] -> rows (d*c2 + co), k = ci; scale/shift per row
        const int c2 = c - g;
        const std::string p = "us." + std::to_string(i);
        auto w = find(tm, p + ".weight", (int64_t)c * c2 * 4, ctx);
        auto sc = find(tm, p + ".scale", c2, ctx);
        auto sh = find(tm, p + ".shift", c2, ctx);
        if (!w || !sc || !sh) return ALSEP_ERR_ARG;
        std::vector<float> mk((size_t)4 * c2 * c), sc4((size_t)4 * c2), sh4((size_t)4 * c2);
        for (int ci = 0; ci < c; ++ci)
            for (int co = 0; co < c2; ++co)
                for (int d = 0; d < 4; ++d) mk[((size_t)d * c2 + co) * c + ci] = (*w)[((size_t)ci * c2 + co) * 4 + d];
        for (int d = 0; d < 4; ++d)
            for (int co = 0; co < c2; ++co) { sc4[d * c2 + co] = (*sc)[co]; sh4[d * c2 + co] = (*sh)[co]; }
        if ((rc = make_gemm_weights<T>(net, mk, 4 * c2, c, &net->us[i]))) return rc;
        if (is_bf16<T>() && (c == 96 || c == 144 || c == 192) && (rc = make_frag_weights(net, mk, 4 * c2, c, &net->us[i].wfrag))) return rc;
        if ((rc = upload(net, sc4.data(), sc4.size() * 4, &net->us[i].scale))) return rc;
        if ((rc = upload(net, sh4.data(), sh4.size() * 4, &net->us[i].shift))) return rc;
        c = c2; f *= 2;
        if ((rc = make_block<T>(net, tm, "decoding_blocks." + std::to_string(i), c, f, &net->dec[i]))) return rc;
    }
    return ALSEP_OK;
}

// ---- launches ------------------------------------------------------------------------------
template <typename T, int KC, int BN, int TW>
int launch_conv(alsep_ctx* ctx, const ConvLayer& L, const T* X, T* Y, int64_t B, int Th, int Fw) {
    typedef ConvCfg<T, KC, BN, TW> Cf;
    const int tiles_t = (int)ceil_div64(Th, Cf::TH), tiles_f = (int)ceil_div64(Fw, TW);
    const int64_t ntiles = B * tiles_t * tiles_f;
    if (ntiles > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "conv3x3: too many tiles");
    ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)conv3x3_kernel<T, KC, BN, TW>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cf::lds_bytes));
    ProfScope prof(ctx, TW == 64 ? ALSEP_PROF_CONV3X3 : ALSEP_PROF_CONV3X3_SMALL);
    prof.work(18.0 * (double)L.cin * L.cout * B * Th * Fw, (double)sizeof(*X) * B * Th * Fw * (L.cin + L.cout));
    hipLaunchKernelGGL((conv3x3_kernel<T, KC, BN, TW>), dim3((unsigned)ntiles, L.cout / BN), dim3(kThreads),
                       Cf::lds_bytes, ctx->stream, X, Y, (const T*)L.w.p, (const float*)L.scale.p,
                       (const float*)L.shift.p, Th, Fw, L.cin, L.cout, tiles_t, tiles_f, (int)ntiles);
    ALSEP_LAUNCH_CHECK(ctx, "conv3x3_kernel");
    return ALSEP_OK;
}

template <typename T, int KC, int BN>
int run_conv_tw(alsep_ctx* ctx, const ConvLayer& L, const T* X, T* Y, int64_t B, int Th, int Fw) {
    if (Fw >= 64 && Fw % 64 == 0) return launch_conv<T, KC, BN, 64>(ctx, L, X, Y, B, Th, Fw);
    if (Fw >= 32) return launch_conv<T, KC, BN, 32>(ctx, L, X, Y, B, Th, Fw);
    return launch_conv<T, KC, BN, 16>(ctx, L, X, Y, B, Th, Fw);
}

int conv_ny_fastest() {
    static const int v = env_int("ALSEP_CONV_NYFAST", 1);
    return v;
}

template <int TW>
int launch_conv_dma(alsep_ctx* ctx, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B,
                    int Th, int Fw) {
    typedef ConvB16<TW> Cf;
    const int tiles_t = (int)ceil_div64(Th, Cf::TH), tiles_f = (int)ceil_div64(Fw, TW);
    const int64_t ntiles = B * tiles_t * tiles_f;
    if (ntiles > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "conv3x3: too many tiles");
    ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)conv3x3_bf16_kernel<TW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)Cf::lds_bytes));
    ProfScope prof(ctx, TW == 64 ? ALSEP_PROF_CONV3X3 : ALSEP_PROF_CONV3X3_SMALL);
    prof.work(18.0 * (double)L.cin * L.cout * B * Th * Fw, (double)sizeof(*X) * B * Th * Fw * (L.cin + L.cout));
    const int nyc = L.cout / Cf::BN;
    const int ny_fastest = conv_ny_fastest() && ntiles % 8 == 0 && nyc > 1 && ntiles * nyc <= 0x7fffffff;
    hipLaunchKernelGGL((conv3x3_bf16_kernel<TW>), ny_fastest ? dim3((unsigned)(ntiles * nyc)) : dim3((unsigned)ntiles, nyc),
                       dim3(kThreads), Cf::lds_bytes,
                       ctx->stream, X, Y, (const bf16_t*)L.w.p, (const float*)L.scale.p, (const float*)L.shift.p, zero_page,
                       Th, Fw, L.cin, L.cout, tiles_t, tiles_f, (int)ntiles, /*ablate*/ 0, /*stagger*/ 0, ny_fastest);
    note_launch(ctx, TW == 64 ? "conv3x3_bf16_kernel<64>" : "conv3x3_bf16_kernel<small>");
    ALSEP_LAUNCH_CHECK(ctx, "conv3x3_bf16_kernel");
    return ALSEP_OK;
}

template <int NQ, int RING_ = 3, int OCC = 1, int TW_ = 64>
int launch_conv_regw(alsep_ctx* ctx, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B,
                     int Th, int Fw) {
    typedef ConvRW<NQ, RING_, TW_> Cf;
    const int tiles_t = Th / Cf::TH, tiles_f = Fw / Cf::TW;
    const int64_t ntiles = B * tiles_t * tiles_f;
    if (ntiles > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "conv3x3: too many tiles");
    ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)conv3x3_bf16_regw_kernel<NQ, RING_, OCC, TW_>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cf::lds_bytes));
    const int ny = L.cout / Cf::BN;
    int gx = OCC * 256 / ny;                                // OCC workgroups per CU over the whole grid
    if (gx > ntiles) gx = (int)ntiles;
    ProfScope prof(ctx, ALSEP_PROF_CONV3X3_REGW);
    prof.work(18.0 * (double)L.cin * L.cout * B * Th * Fw, (double)sizeof(*X) * B * Th * Fw * (L.cin + L.cout));
    hipLaunchKernelGGL((conv3x3_bf16_regw_kernel<NQ, RING_, OCC, TW_>), dim3((unsigned)gx, ny), dim3(kThreads), Cf::lds_bytes, ctx->stream, X, Y,
                       (const bf16_t*)L.w.p, (const float*)L.scale.p, (const float*)L.shift.p, zero_page, Th, Fw, L.cin,
                       L.cout, tiles_t, tiles_f, (int)ntiles);
    ALSEP_LAUNCH_CHECK(ctx, "conv3x3_bf16_regw_kernel");
    return ALSEP_OK;
}

// The three 8-wave persistent convs (conv3x3_bf16_m0_kernel, _mq_kernel, _big_kernel<3>) share their argument list and their launch: one
// workgroup per CU, each walking the tiles blockIdx.x, blockIdx.x + gridDim.x, ...  Cf is the kernel's tile configuration, wimg its weight
// image; the caller has checked that the layer fits the kernel.
template <typename Cf, typename Kern>
int launch_conv_persist(alsep_ctx* ctx, Kern kern, const ConvLayer& L, const DevBuf& wimg, int prof_class, const char* name, const bf16_t* X,
                        bf16_t* Y, const bf16_t* zero_page, int64_t B, int Th, int Fw, int grid_cap = 0) {
    const int tiles_t = Th / Cf::TH, tiles_f = Fw / Cf::TW;
    const int64_t ntiles = B * tiles_t * tiles_f;
    if (ntiles > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "conv3x3: too many tiles");
    ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cf::lds_bytes));
    int gx = ntiles < 256 ? (int)ntiles : 256;
    if (grid_cap > 0 && gx > grid_cap) gx = grid_cap;
    ProfScope prof(ctx, prof_class);
    prof.work(18.0 * (double)L.cin * L.cout * B * Th * Fw, (double)sizeof(*X) * B * Th * Fw * (L.cin + L.cout));
    hipLaunchKernelGGL(kern, dim3((unsigned)gx), dim3(kBigThreads), Cf::lds_bytes, ctx->stream, X, Y, (const bf16_t*)wimg.p,
                       (const float*)L.scale.p, (const float*)L.shift.p, zero_page, Th, Fw, L.cin, L.cout, tiles_t, tiles_f, (int)ntiles);
    ALSEP_LAUNCH_CHECK(ctx, name);
    return ALSEP_OK;
}

int launch_conv_big3(alsep_ctx* ctx, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B, int Th, int Fw) {
    if (!L.w_big.p) return alsep_fail(ctx, ALSEP_ERR_STATE, "conv3x3: no big-tile weight image for this layer");
    if (int rc = launch_conv_persist<ConvBig<3>>(ctx, conv3x3_bf16_big_kernel<3>, L, L.w_big, ALSEP_PROF_CONV3X3_BIG3, "conv3x3_bf16_big_kernel",
                                                 X, Y, zero_page, B, Th, Fw))
        return rc;
    note_launch(ctx, "conv3x3_bf16_big_kernel<3>");
    return ALSEP_OK;
}

int launch_conv_mq(alsep_ctx* ctx, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B, int Th, int Fw) {
    if (!L.w_mq.p || L.cout != ConvMq::ROWS || L.cin % ConvMq::KC) return alsep_fail(ctx, ALSEP_ERR_STATE, "conv3x3: no mq weight image for this layer");
    return launch_conv_persist<ConvMq>(ctx, conv3x3_bf16_mq_kernel, L, L.w_mq, ALSEP_PROF_CONV3X3_BIG, "conv3x3_bf16_mq_kernel", X, Y, zero_page,
                                       B, Th, Fw);
}

int launch_conv_m0(alsep_ctx* ctx, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B, int Th, int Fw) {
    if (!L.w_big.p || L.cout != ConvM0::ROWS || L.cin != ConvM0::KC) return alsep_fail(ctx, ALSEP_ERR_STATE, "conv3x3: no m0 weight image for this layer");
    return launch_conv_persist<ConvM0>(ctx, conv3x3_bf16_m0_kernel, L, L.w_big, ALSEP_PROF_CONV3X3_REGW, "conv3x3_bf16_m0_kernel", X, Y, zero_page,
                                       B, Th, Fw);
}

int conv_allco_grid() {
    static const int v = env_int("ALSEP_CONV_ALLCO_GRID", 0);
    return v;
}

// The pinned launch names count layer launches, whichever instance serves them (as launch_tdf_persist does): the names of the kernel
// that this one replaces at its level are noted beside its own.
// <9, 48, 1> replaces conv3x3_bf16_big_kernel<3> (c = 144); the instances in output groups, <6, 48 | 64, 2 | 3> (c = 192 / 288), replace
// conv3x3_bf16_kernel<64 | small> and keep its profiling class, so that a level's class does not depend on the instance that serves it.
template <int NM, int TW, int NGRP>
int launch_conv_allco(alsep_ctx* ctx, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B, int Th, int Fw) {
    typedef ConvAllco<NM, TW, NGRP> Cf;
    static_assert((NM == 9 && TW == 48 && NGRP == 1) || (NM == 6 && NGRP >= 2), "an instance that has a weight image, names and a class below");
    if (!L.w_ac.p || L.cout != Cf::COUT || L.cin != L.cout || Th % Cf::TH || Fw % TW)
        return alsep_fail(ctx, ALSEP_ERR_STATE, "conv3x3: no all-channels weight image for this layer, or not its shape");
    const bool plain64 = Fw >= 64 && Fw % 64 == 0;           // run_conv_dma's choice between conv3x3_bf16_kernel<64> and <small>
    const int prof_class = NGRP == 1 ? ALSEP_PROF_CONV3X3_BIG3 : plain64 ? ALSEP_PROF_CONV3X3 : ALSEP_PROF_CONV3X3_SMALL;
    if (int rc = launch_conv_persist<Cf>(ctx, conv3x3_bf16_allco_kernel<NM, TW, NGRP>, L, L.w_ac, prof_class, "conv3x3_bf16_allco_kernel", X, Y,
                                         zero_page, B, Th, Fw, conv_allco_grid()))
        return rc;
    if (NGRP == 1) {
        note_launch(ctx, "conv3x3_bf16_big_kernel");
        note_launch(ctx, "conv3x3_bf16_big_kernel<3>");
    } else {
        note_launch(ctx, TW == 48 ? "conv3x3_bf16_allco_kernel<6,48>" : "conv3x3_bf16_allco_kernel<6,64>");
        note_launch(ctx, "conv3x3_bf16_kernel");
        note_launch(ctx, plain64 ? "conv3x3_bf16_kernel<64>" : "conv3x3_bf16_kernel<small>");
    }
    return ALSEP_OK;
}

// Which kernel runs a bf16 / f16 3x3 conv with c % 48 == 0.  Every switch is an environment variable read once per process; each one only
// chooses between kernels that compute the same layer (all but mq bit-identically to the plain kernel).
//   ALSEP_CONV_M0     1 (default): c = 48 with T % 8 == 0, F % 48 == 0 and >= 256 tiles on conv3x3_bf16_m0_kernel (LDS-resident weights);
//                     2: without the minimum tile count (tests); 0: off.  Same-box A/B at the bench shape (profiles/r02_conv_level0_ab.txt):
//                     register-weight kernel 268.5 us -> 233 us per 1.12 GB launch (4.8 TB/s = 60 % of 8 TB/s).
//   ALSEP_CONV_REGW   what m0 leaves, with T % 4 == 0 and F % 64 == 0, on conv3x3_bf16_regw_kernel.  1 (default): c = 48 on 4 x 32 tiles, two
//                     workgroups per CU; 2: also c = 96; 3: as 2, with c = 48 on 4 x 64 tiles, one workgroup per CU; 0: off.
//   ALSEP_CONV_BIG    1 (default): c = 96 / 144 with T % 8 == 0, F % 64 == 0 and >= 96 tiles on the 8-wave kernel of its level (_MQ, _BIG3);
//                     2: without the minimum tile count (tests); 0: off.
//   ALSEP_CONV_MQ     1 (default): c = 96 on conv3x3_bf16_mq_kernel (everything double-buffered); 0: the plain kernel.  Same-box A/B at the
//                     bench shape (profiles/r02_conv_level1_ab.txt): big-tile 316 us -> merged 262 us -> this 210-219 us per launch
//                     (1.13 PFLOP/s = 45 % of 2.5 PF).
//   ALSEP_CONV_BIG3   1 (default): c = 144 on conv3x3_bf16_big_kernel<3> (8 VGPRs spill, outside the MFMA loops); 0: the plain kernel.
//   ALSEP_CONV_ALLCO  under ALSEP_CONV_BIG and ALSEP_CONV_BIG3 (either at 0 keeps meaning "plain kernel"): c = 144 with T % 8 == 0 and
//                     F % 48 == 0 on conv3x3_bf16_allco_kernel<9, 48> (all output channels per patch, k-step-major weight ring, two patch
//                     buffers).  1 (default): the levels in kConvAllcoRouted, at exactly the shapes big<3> would take (F % 64 == 0 as
//                     well, >= 96 tiles of 8 x 64 or ALSEP_CONV_BIG=2) -- the kernel was measured against big<3> only, so a shape with
//                     F % 48 == 0 but F % 64 != 0 stays on the plain kernel; 0: never; 2: every shape the kernel serves, without the
//                     minimum tile count (tests).  ALSEP_CONV_ALLCO_GRID=n caps its grid (tests).  Same-box traces at the bench shape
//                     (profiles/conv_allco_kernel_stats.txt): big<3> 1051 us (min 1002) -> 773 us (max 828) per launch = 1.23 PFLOP/s =
//                     0.49 of 2.5 PF.  Its launches also count under big<3>'s pinned names (layer launches, whichever instance serves them).
//                     Under ALSEP_CONV_BIG alone: c = 192 / 288 with T % 8 == 0 and F % TW == 0 on conv3x3_bf16_allco_kernel<6, TW, 2 | 3>,
//                     the same kernel in two / three output groups of 96 channels (a work item is (tile, group); the patch is staged once
//                     per group).  1 (default): c = 192 if kConvAllcoRouted has its bit, at the shapes it was measured against
//                     conv3x3_bf16_kernel<64> (F % 64 == 0 as well, >= 96 tiles of 8 x 64 or ALSEP_CONV_BIG=2); c = 288 never (level 5 is
//                     0.24 ms per forward: nothing to gain); 0: never; 2: every shape an instance serves, c = 288 too, without the minimum
//                     tile count (tests).  These launches keep the plain kernel's profiling class and also count under its pinned names,
//                     and under conv3x3_bf16_allco_kernel<6,48> or <6,64>.  Same-box traces at the bench shape
//                     (profiles/conv_allco_groups_kernel_stats.txt): conv3x3_bf16_kernel<64> 523 us (min 493) -> <6, 64, 2> 346 us
//                     (max 381) per launch = 1.23 PFLOP/s = 0.49 of 2.5 PF; <6, 48, 2> 377 us (max 410) = 0.45.
//   ALSEP_CONV_ALLCO_TW  48 | 64 (default 64, the width that measured faster): the tile width of the instances in output groups (tests, A/B).
//   ALSEP_CONV_NYFAST 1 (default): the plain kernel's Cout / 48 workgroups of one tile run back to back on one XCD (1-D grid, needs
//                     ntiles % 8 == 0); 0: the tile index is the fastest grid dimension.
// Everything else -- c = 240 and up, shapes that miss a divisibility above -- runs conv3x3_bf16_kernel<64 | 32 | 16>.  At c = 192 both
// 8-wave structures need scratch at 2 waves / SIMD with ROCm 7.2 when one wave holds all 192 channels, and are not built that way:
// big<4> spills heavily, and conv3x3_bf16_allco_kernel<12, 48> (144 accumulators) needs 256 VGPRs and spills 15 more (64 bytes of
// scratch per lane, hipcc -Rpass-analysis=kernel-resource-usage; profiles/conv_allco_ab.txt).  In two groups of 96 channels the
// all-channels kernel holds 72 (8 x 48) or 96 (8 x 64) accumulators: 158 / 201 VGPRs, no scratch (profiles/conv_allco_groups_ab.txt).
int conv_m0_enabled() {
    static const int v = env_int("ALSEP_CONV_M0", 1);
    return v;
}
int conv_regw_enabled() {
    static const int v = env_int("ALSEP_CONV_REGW", 1);
    return v;
}
int conv_big_enabled() {
    static const int v = env_int("ALSEP_CONV_BIG", 1);
    return v;
}
int conv_mq_enabled() {
    static const int v = env_int("ALSEP_CONV_MQ", 1);
    return v;
}
int conv_big3_enabled() {
    static const int v = env_int("ALSEP_CONV_BIG3", 1);
    return v;
}

int conv_allco_enabled() {
    static const int v = env_int("ALSEP_CONV_ALLCO", 1);
    return v;
}
// Levels that measured faster on conv3x3_bf16_allco_kernel than on their kernel, same box, bench shape (profiles/conv_allco_kernel_stats.txt,
// conv_allco_ab.txt; c = 192: conv_allco_groups_kernel_stats.txt, conv_allco_groups_ab.txt); only these are routed there by default.
constexpr int kConvAllco144 = 1, kConvAllco192 = 2;
constexpr int kConvAllcoRouted = kConvAllco144 | kConvAllco192;
// the tile width of the instances in output groups (c = 192 / 288): 48 or 64
constexpr int kConvAllcoTw = 64;
int conv_allco_tw() {
    static const int v = env_int("ALSEP_CONV_ALLCO_TW", kConvAllcoTw) == 48 ? 48 : 64;
    return v;
}

int run_conv_dma(alsep_ctx* ctx, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zp, int64_t B, int Th, int Fw) {
    if (conv_m0_enabled() && L.cin == 48 && L.cout == 48 && Th % 8 == 0 && Fw % 48 == 0 &&
        (conv_m0_enabled() >= 2 || B * (Th / 8) * (Fw / 48) >= 256))
        return launch_conv_m0(ctx, L, X, Y, zp, B, Th, Fw);
    if (conv_regw_enabled() && Th % 4 == 0 && Fw % 64 == 0 && L.cin == L.cout) {
        if (L.cin == 48 && conv_regw_enabled() == 3) return launch_conv_regw<1>(ctx, L, X, Y, zp, B, Th, Fw);
        if (L.cin == 48) return launch_conv_regw<1, 3, 2, 32>(ctx, L, X, Y, zp, B, Th, Fw);
        if (L.cin == 96 && conv_regw_enabled() >= 2) return launch_conv_regw<2>(ctx, L, X, Y, zp, B, Th, Fw);
    }
    if (conv_big_enabled() && conv_big3_enabled() && conv_allco_enabled() && Th % 8 == 0 && Fw % 48 == 0 && L.cin == 144 && L.cout == 144) {
        const int mode = conv_allco_enabled();
        // by default only what big<3> served (F % 64 == 0 too, its tile floor): the shapes the routing was measured at
        const bool big3_shape = Fw % 64 == 0 && (conv_big_enabled() >= 2 || B * (Th / 8) * (Fw / 64) >= 96);
        if (mode >= 2 || ((kConvAllcoRouted & kConvAllco144) && big3_shape)) return launch_conv_allco<9, 48, 1>(ctx, L, X, Y, zp, B, Th, Fw);
    }
    if (conv_big_enabled() && conv_allco_enabled() && L.cin == L.cout && (L.cout == 192 || L.cout == 288)) {
        const int mode = conv_allco_enabled(), tw = conv_allco_tw();
        // by default only c = 192, and only where conv3x3_bf16_kernel<64> ran it with the tile floor of the other 8-wave kernels
        const bool measured_shape = L.cout == 192 && Fw % 64 == 0 && (conv_big_enabled() >= 2 || B * (Th / 8) * (Fw / 64) >= 96);
        if (Th % 8 == 0 && Fw % tw == 0 && (mode >= 2 || ((kConvAllcoRouted & kConvAllco192) && measured_shape))) {
            if (L.cout == 192) return tw == 48 ? launch_conv_allco<6, 48, 2>(ctx, L, X, Y, zp, B, Th, Fw) : launch_conv_allco<6, 64, 2>(ctx, L, X, Y, zp, B, Th, Fw);
            return tw == 48 ? launch_conv_allco<6, 48, 3>(ctx, L, X, Y, zp, B, Th, Fw) : launch_conv_allco<6, 64, 3>(ctx, L, X, Y, zp, B, Th, Fw);
        }
    }
    if (conv_big_enabled() && Th % 8 == 0 && Fw % 64 == 0 && L.cin == L.cout &&
        (conv_big_enabled() >= 2 || B * (Th / 8) * (Fw / 64) >= 96)) {
        if (L.cout == 96 && conv_mq_enabled()) return launch_conv_mq(ctx, L, X, Y, zp, B, Th, Fw);
        if (L.cout == 144 && conv_big3_enabled()) return launch_conv_big3(ctx, L, X, Y, zp, B, Th, Fw);
    }
    if (Fw >= 64 && Fw % 64 == 0) return launch_conv_dma<64>(ctx, L, X, Y, zp, B, Th, Fw);
    if (Fw >= 32) return launch_conv_dma<32>(ctx, L, X, Y, zp, B, Th, Fw);
    return launch_conv_dma<16>(ctx, L, X, Y, zp, B, Th, Fw);
}
int run_conv_dma(alsep_ctx* ctx, const ConvLayer&, const float*, float*, const float*, int64_t, int, int) {
    return alsep_fail(ctx, ALSEP_ERR_STATE, "LDS-DMA conv path is bf16 only");
}

#ifndef ALSEP_F16_TU
template <int KC, int BN, int TW>
int launch_conv_split(alsep_ctx* ctx, const ConvLayer& L, const float* X, float* Y, int64_t B, int Th, int Fw) {
    typedef ConvSCfg<KC, BN, TW> Cf;
    const int tiles_t = (int)ceil_div64(Th, Cf::TH), tiles_f = (int)ceil_div64(Fw, TW);
    const int64_t ntiles = B * tiles_t * tiles_f;
    const int nyc = L.cout / BN;
    if (ntiles * nyc > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "conv3x3: too many tiles");
    ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)conv3x3_f32s_kernel<KC, BN, TW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)Cf::lds_bytes));
    ProfScope prof(ctx, TW >= 32 ? ALSEP_PROF_CONV3X3 : ALSEP_PROF_CONV3X3_SMALL);
    prof.work(18.0 * (double)L.cin * L.cout * B * Th * Fw, 4.0 * B * Th * Fw * (L.cin + L.cout));
    const int nyf = (ntiles % 8 == 0 && nyc > 1) ? 1 : 0;
    const dim3 grid = nyf ? dim3((unsigned)(ntiles * nyc)) : dim3((unsigned)ntiles, nyc);
    hipLaunchKernelGGL((conv3x3_f32s_kernel<KC, BN, TW>), grid, dim3(kThreads), Cf::lds_bytes, ctx->stream, X, Y,
                       (const hs_t*)L.w.p, (const float*)L.scale.p, (const float*)L.shift.p, Th, Fw, L.cin, L.cout, tiles_t, tiles_f,
                       (int)ntiles, nyf, L.range_flag);
    ALSEP_LAUNCH_CHECK(ctx, "conv3x3_f32s_kernel");
    return ALSEP_OK;
}
template <int KC, int BN>
int run_conv_split_tw(alsep_ctx* ctx, const ConvLayer& L, const float* X, float* Y, int64_t B, int Th, int Fw) {
    if (Fw >= 32) return launch_conv_split<KC, BN, 32>(ctx, L, X, Y, B, Th, Fw);      // 8 x 32 tiles: 76 KiB, two workgroups per CU
    return launch_conv_split<KC, BN, 16>(ctx, L, X, Y, B, Th, Fw);
}
int run_conv_split(alsep_ctx* ctx, const ConvLayer& L, const float* X, float* Y, int64_t B, int Th, int Fw) {
    return L.split == 24 ? run_conv_split_tw<24, 48>(ctx, L, X, Y, B, Th, Fw) : run_conv_split_tw<16, 16>(ctx, L, X, Y, B, Th, Fw);
}
int run_conv_split(alsep_ctx* ctx, const ConvLayer&, const bf16_t*, bf16_t*, int64_t, int, int) {
    return alsep_fail(ctx, ALSEP_ERR_STATE, "split contraction is a float32 mode");
}
#endif

template <typename T>
int run_conv(alsep_ctx* ctx, const ConvLayer& L, const T* X, T* Y, int64_t B, int Th, int Fw, const void* zero_page) {
#ifndef ALSEP_F16_TU
    if (L.split) return run_conv_split(ctx, L, X, Y, B, Th, Fw);
#endif
    if (L.dma_path) return run_conv_dma(ctx, L, X, Y, (const T*)zero_page, B, Th, Fw);
    if (conv_uses_main<T>(L.cin, L.cout)) return run_conv_tw<T, ConvSel<T>::KC, ConvSel<T>::BN>(ctx, L, X, Y, B, Th, Fw);
    return run_conv_tw<T, ConvSel16<T>::KC, ConvSel16<T>::BN>(ctx, L, X, Y, B, Th, Fw);
}

int pix_stream_enabled() {
    static const int v = env_int("ALSEP_PIX_STREAM", 1);
    return v;
}
// ALSEP_PIX_PIPE: 1 (default) = the ds / us of the middle levels run on ds_pipe_kernel / us_pipe_kernel for the instances in
// kPixPipeRouted (each is routed there only where it measured faster than its stream kernel on the same box:
// profiles/pix_pipe_kernel_stats.txt); 0 = never (the stream kernels, as before); 2 = every instance (measurements, tests).
// ALSEP_PIX_PIPE_GRID=n caps their grid (tests: several tiles per workgroup at small shapes).
enum { kPixPipeDs96 = 1, kPixPipeDs144 = 2, kPixPipeUs192 = 4, kPixPipeUs144 = 8 };
constexpr int kPixPipeRouted = kPixPipeDs96 | kPixPipeDs144 | kPixPipeUs192 | kPixPipeUs144;
bool pix_pipe_routed(int kind) {
    static const int v = env_int("ALSEP_PIX_PIPE", 1);
    return v >= 2 || (v == 1 && (kPixPipeRouted & kind));
}
unsigned pix_pipe_grid(alsep_ctx* ctx, int64_t ntile) {     // more than 128 KiB of LDS: one workgroup per CU
    static const int cap = env_int("ALSEP_PIX_PIPE_GRID", 0);
    int64_t grid = device_cu_count(ctx);
    if (cap > 0 && cap < grid) grid = cap;
    return (unsigned)std::min<int64_t>(grid, ntile);
}
template <int C_, int PX_, int D_>
hipError_t launch_ds_pipe(alsep_ctx* ctx, const GemmLayer& L, const bf16_t* X, bf16_t* Y, int64_t ncols, int Tp, int Fp) {
    typedef DsPipeCfg<C_, PX_, D_> P;
    const hipError_t e = hipFuncSetAttribute((const void*)ds_pipe_kernel<C_, PX_, D_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P::lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((ds_pipe_kernel<C_, PX_, D_>), dim3(pix_pipe_grid(ctx, ncols / P::PX)), dim3(kThreads), P::lds_bytes, ctx->stream, X, Y,
                       (const bf16_t*)L.wfrag.p, (const float*)L.scale.p, (const float*)L.shift.p, ncols, Tp, Fp);
    return hipSuccess;
}
template <int CIN, int C2_, int NI_, int D_>
hipError_t launch_us_pipe(alsep_ctx* ctx, const GemmLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* skip, int64_t ncols, int Tp, int Fp) {
    typedef UsPipeCfg<CIN, C2_, NI_, D_> P;
    const hipError_t e = hipFuncSetAttribute((const void*)us_pipe_kernel<CIN, C2_, NI_, D_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P::lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((us_pipe_kernel<CIN, C2_, NI_, D_>), dim3(pix_pipe_grid(ctx, ncols / P::PX)), dim3(kThreads), P::lds_bytes, ctx->stream, X, Y,
                       (const bf16_t*)L.wfrag.p, (const float*)L.scale.p, (const float*)L.shift.p, skip, ncols, Tp, Fp);
    return hipSuccess;
}
int run_pix_stream(alsep_ctx* ctx, int mode, const GemmLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* skip, int64_t ncols,
                   int Tp, int Fp) {
    ProfScope prof(ctx, ALSEP_PROF_PIX);
    const int64_t ntile = ncols / 64;
    // the pipelined kernels: one more launch-count name each, the pinned names below are noted as before
    if (mode == PIX_DS && L.M == DsSplitCfg<96>::M && pix_pipe_routed(kPixPipeDs96)) {
        ALSEP_HIP(ctx, (launch_ds_pipe<96, 64, 1>(ctx, L, X, Y, ncols, Tp, Fp)));
        note_launch(ctx, "ds_pipe_kernel<96>");
        note_launch(ctx, "ds_split_stream_kernel<96>");
    } else if (mode == PIX_DS && L.M == DsSplitCfg<144>::M && pix_pipe_routed(kPixPipeDs144)) {
        ALSEP_HIP(ctx, (launch_ds_pipe<144, 32, 2>(ctx, L, X, Y, ncols, Tp, Fp)));
        note_launch(ctx, "ds_pipe_kernel<144>");
        note_launch(ctx, "ds_split_stream_kernel<144>");
    } else if (mode != PIX_DS && L.K == 192 && pix_pipe_routed(kPixPipeUs192)) {
        ALSEP_HIP(ctx, (launch_us_pipe<192, 144, 2, 1>(ctx, L, X, Y, skip, ncols, Tp, Fp)));
        note_launch(ctx, "us_pipe_kernel<192,144>");
        note_launch(ctx, "us_stream_kernel<192,144>");
    } else if (mode != PIX_DS && L.K == 144 && pix_pipe_routed(kPixPipeUs144)) {
        ALSEP_HIP(ctx, (launch_us_pipe<144, 96, 2, 2>(ctx, L, X, Y, skip, ncols, Tp, Fp)));
        note_launch(ctx, "us_pipe_kernel<144,96>");
        note_launch(ctx, "us_stream_kernel<144,96>");
    } else if (mode == PIX_DS && L.M == Ds48::M) {
        const size_t lds = 4 * 64 * Ds48::MS * sizeof(bf16_t);
        const int64_t gx = std::min<int64_t>(ceil_div64(ntile, 4), 256);
        hipLaunchKernelGGL(ds48_stream_kernel, dim3((unsigned)gx), dim3(kThreads), lds, ctx->stream, X, Y, (const bf16_t*)L.wfrag.p,
                           (const float*)L.scale.p, (const float*)L.shift.p, ncols, Tp, Fp);
        note_launch(ctx, "ds48_stream_kernel");
    } else if (mode == PIX_DS && L.M == DsSplitCfg<96>::M) { // 96 -> 144
        const size_t lds = 64 * DsSplitCfg<96>::MS * sizeof(bf16_t);
        const int64_t gx = std::min<int64_t>(ntile, 512);
        hipLaunchKernelGGL((ds_split_stream_kernel<96, 2>), dim3((unsigned)gx), dim3(kThreads), lds, ctx->stream, X, Y,
                           (const bf16_t*)L.wfrag.p, (const float*)L.scale.p, (const float*)L.shift.p, ncols, Tp, Fp);
        note_launch(ctx, "ds_split_stream_kernel<96>");
    } else if (mode == PIX_DS) {                             // 144 -> 192
        const size_t lds = 64 * DsSplitCfg<144>::MS * sizeof(bf16_t);
        const int64_t gx = std::min<int64_t>(ntile, 512);
        hipLaunchKernelGGL((ds_split_stream_kernel<144, 1>), dim3((unsigned)gx), dim3(kThreads), lds, ctx->stream, X, Y,
                           (const bf16_t*)L.wfrag.p, (const float*)L.scale.p, (const float*)L.shift.p, ncols, Tp, Fp);
        note_launch(ctx, "ds_split_stream_kernel<144>");
    } else {
#define ALSEP_US(CIN_, C2_, NI_, OCC_, GX_)                                                                                 \
    {                                                                                                                       \
        typedef UsCfg<CIN_, C2_, NI_> U;                                                                                    \
        ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)us_stream_kernel<CIN_, C2_, NI_, OCC_>,                             \
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)U::lds_bytes));                 \
        const int64_t gx = std::min<int64_t>(ncols / U::PX, GX_);                                                           \
        hipLaunchKernelGGL((us_stream_kernel<CIN_, C2_, NI_, OCC_>), dim3((unsigned)gx), dim3(kThreads), U::lds_bytes,      \
                           ctx->stream, X, Y, (const bf16_t*)L.wfrag.p, (const float*)L.scale.p, (const float*)L.shift.p,   \
                           skip, ncols, Tp, Fp);                                                                            \
        note_launch(ctx, "us_stream_kernel<" #CIN_ "," #C2_ ">");                                                          \
    }
        if (L.K == 96) ALSEP_US(96, 48, 4, 1, 512)               // 96 -> 48
        else if (L.K == 144) ALSEP_US(144, 96, 2, 2, 512)        // 144 -> 96: 32-pixel tiles, two workgroups per CU
        else ALSEP_US(192, 144, 2, 1, 256)                       // 192 -> 144: 32-pixel tiles (accumulators beside 54 fragments)
#undef ALSEP_US
    }
    note_launch(ctx, mode == PIX_DS ? "ds_stream_kernel" : "us_stream_kernel");
    ALSEP_LAUNCH_CHECK(ctx, "pix stream kernel");
    return ALSEP_OK;
}
int run_pix_stream(alsep_ctx* ctx, int, const GemmLayer&, const float*, float*, const float*, int64_t, int, int) {
    return alsep_fail(ctx, ALSEP_ERR_STATE, "streaming ds/us path is bf16 only");
}

#ifndef ALSEP_F16_TU
template <int MODE>
int run_pix_split(alsep_ctx* ctx, const GemmLayer& L, const float* X, float* Y, const float* skip, int64_t ncols, int Tp, int Fp, int C, int C2) {
    typedef GemmSCfg Gc;
    const int64_t gx = ceil_div64(ncols, Gc::BC);
    if (gx > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "pix_gemm: too many column tiles");
    ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)pix_gemm_f32s_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Gc::lds_bytes));
    ProfScope prof(ctx, ALSEP_PROF_PIX);
    const int nrb = L.Mp / Gc::BR;
    const int fast = (nrb > 1 && gx % 8 == 0 && gx * nrb <= 0x7fffffff) ? nrb : 0;
    hipLaunchKernelGGL((pix_gemm_f32s_kernel<MODE>), fast ? dim3((unsigned)(gx * nrb)) : dim3((unsigned)gx, nrb), dim3(kThreads), Gc::lds_bytes,
                       ctx->stream, X, Y, (const hs_t*)L.w.p, (const float*)L.scale.p, (const float*)L.shift.p, skip, L.M, L.Mp, L.K, L.Kp, ncols,
                       Tp, Fp, C, C2, L.range_flag, fast);
    ALSEP_LAUNCH_CHECK(ctx, "pix_gemm_f32s_kernel");
    return ALSEP_OK;
}
template <int MODE>
int run_pix_split(alsep_ctx* ctx, const GemmLayer&, const bf16_t*, bf16_t*, const bf16_t*, int64_t, int, int, int, int) {
    return alsep_fail(ctx, ALSEP_ERR_STATE, "split contraction is a float32 mode");
}
int run_tdf_split(alsep_ctx* ctx, const GemmLayer& L, const float* X, float* Y, const float* R, int64_t BT, int C) {
    typedef GemmSCfg Gc;
    const int64_t nunits = BT * (C / 16);
    const int64_t gx = ceil_div64(nunits, 8);
    if (gx > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "tdf_gemm: too many column tiles");
    const float* bias = L.has_bias ? (const float*)L.bias.p : nullptr;
    ProfScope prof(ctx, ALSEP_PROF_TDF);
    const int nrb = L.Mp / Gc::BR;
    const int fast = (nrb > 1 && gx % 8 == 0 && gx * nrb <= 0x7fffffff) ? nrb : 0;
    const dim3 grid = fast ? dim3((unsigned)(gx * nrb)) : dim3((unsigned)gx, nrb);
    if (R) {
        ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)tdf_gemm_f32s_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Gc::lds_bytes));
        hipLaunchKernelGGL((tdf_gemm_f32s_kernel<true>), grid, dim3(kThreads), Gc::lds_bytes, ctx->stream, X, Y, (const hs_t*)L.w.p, bias,
                           (const float*)L.scale.p, (const float*)L.shift.p, R, L.M, L.Mp, L.K, L.Kp, nunits, C, L.range_flag, fast);
    } else {
        ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)tdf_gemm_f32s_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Gc::lds_bytes));
        hipLaunchKernelGGL((tdf_gemm_f32s_kernel<false>), grid, dim3(kThreads), Gc::lds_bytes, ctx->stream, X, Y, (const hs_t*)L.w.p, bias,
                           (const float*)L.scale.p, (const float*)L.shift.p, R, L.M, L.Mp, L.K, L.Kp, nunits, C, L.range_flag, fast);
    }
    ALSEP_LAUNCH_CHECK(ctx, "tdf_gemm_f32s_kernel");
    return ALSEP_OK;
}
int run_tdf_split(alsep_ctx* ctx, const GemmLayer&, const bf16_t*, bf16_t*, const bf16_t*, int64_t, int) {
    return alsep_fail(ctx, ALSEP_ERR_STATE, "split contraction is a float32 mode");
}
#endif

template <typename T, int MODE>
int run_pix(alsep_ctx* ctx, const GemmLayer& L, const T* X, T* Y, const T* skip, int64_t ncols, int Tp, int Fp, int C, int C2) {
    typedef GemmCfg<T> Gc;
#ifndef ALSEP_F16_TU
    if (L.split) return run_pix_split<MODE>(ctx, L, X, Y, skip, ncols, Tp, Fp, C, C2);
#endif
    if (L.wfrag.p && pix_stream_enabled() && Fp % 64 == 0) return run_pix_stream(ctx, MODE, L, X, Y, skip, ncols, Tp, Fp);
    const int64_t gx = ceil_div64(ncols, Gc::BC);
    if (gx > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "pix_gemm: too many column tiles");
    ProfScope prof(ctx, ALSEP_PROF_PIX);
    hipLaunchKernelGGL((pix_gemm_kernel<T, MODE>), dim3((unsigned)gx, L.Mp / Gc::BR), dim3(kThreads), Gc::lds_bytes,
                       ctx->stream, X, Y, (const T*)L.w.p, (const float*)L.scale.p, (const float*)L.shift.p, skip,
                       L.M, L.K, L.Kp, ncols, Tp, Fp, C, C2);
    ALSEP_LAUNCH_CHECK(ctx, "pix_gemm_kernel");
    return ALSEP_OK;
}

// ALSEP_TDF_WIDE: 0 = 128-row kernel only; 1 (default) = wide kernel where M % 192 == 0, 384 rows per workgroup for a
// first linear whose whole M is 384; 4 / 8 = force 192 / 384 rows wherever M allows (experiments, tests)
int tdf_wide_mode() {
    static const int v = env_int("ALSEP_TDF_WIDE", 1);
    return v;
}
// The final 1x1 convolution of a forward, offered to the last residual TDF launch (run_block's `fin`): the launcher that
// can fold it (tdf_bf16_wide_kernel<4, true, RPF, FINAL>) sets `done`, and forward_impl() then skips final_conv_kernel.
struct FinalFold {
    const float* w;
    const float* b;
    void* out;
    float alpha;
    bool done;
};
// ALSEP_TDF_FINAL: 1 (default) = fold the final 1x1 conv into the last residual TDF launch where the wide 192-row kernel
// serves it and C == 48; 0 = always the separate final_conv_kernel
int tdf_final_mode() {
    static const int v = env_int("ALSEP_TDF_FINAL", 1);
    return v;
}
// ALSEP_TDF_PERSIST: 1 (default) = the residual linear of levels 0 and 1 runs on tdf_bf16_persist_kernel for the launch kinds
// in kTdfPersistRouted (each kind is routed there only where it measured faster than the wide kernel on the same box:
// profiles/tdf_persist_kernel_stats.txt); 0 = never (the wide kernel, as before); 2 = every kind the kernel serves
// (measurements, tests).  ALSEP_TDF_PERSIST_GRID=n caps its grid (tests: several items per workgroup at small shapes).
enum { kTdfPersistK384 = 1, kTdfPersistK192 = 2, kTdfPersistFinal = 4 };
constexpr int kTdfPersistRouted = kTdfPersistK384 | kTdfPersistK192 | kTdfPersistFinal;
int tdf_persist_mode() {
    static const int v = env_int("ALSEP_TDF_PERSIST", 1);
    return v;
}
template <int NT, bool FINAL>
void launch_tdf_persist_inst(alsep_ctx* ctx, hipError_t& attr, unsigned grid, const GemmLayer& L, const bf16_t* X, bf16_t* Y,
                             const bf16_t* R, int64_t nitems, int C, const FinalFold* fin) {
    constexpr int lds = (int)TdfPersist::lds_bytes(NT, FINAL);
    attr = hipFuncSetAttribute((const void*)tdf_bf16_persist_kernel<NT, FINAL>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr != hipSuccess) return;
    hipLaunchKernelGGL((tdf_bf16_persist_kernel<NT, FINAL>), dim3(grid), dim3(TdfPersist::THREADS), lds, ctx->stream, X, Y,
                       (const bf16_t*)L.wwide.p, L.has_bias ? (const float*)L.bias.p : nullptr, (const float*)L.scale.p,
                       (const float*)L.shift.p, R, L.M, nitems, C, fin ? fin->w : nullptr, fin ? fin->b : nullptr,
                       fin ? (bf16_t*)fin->out : nullptr, fin ? fin->alpha : 0.f);
}
// caller: R != nullptr, M % 384 == 0, K 384 or 192, C 48 or 96, nunits % 4 == 0, inside its ProfScope; fin only where C == 48
int launch_tdf_persist(alsep_ctx* ctx, const GemmLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* R, int64_t nunits, int C,
                       FinalFold* fin) {
    static const int cap = env_int("ALSEP_TDF_PERSIST_GRID", 0);
    const int64_t nitems = nunits / TdfPersist::UN;
    int64_t grid = device_cu_count(ctx);                             // 156.75 KiB of LDS: one workgroup per CU
    if (cap > 0 && cap < grid) grid = cap;
    if (nitems < grid) grid = nitems;
    hipError_t attr = hipSuccess;
    if (fin && L.K == 384) launch_tdf_persist_inst<6, true>(ctx, attr, (unsigned)grid, L, X, Y, R, nitems, C, fin);
    else if (fin) launch_tdf_persist_inst<3, true>(ctx, attr, (unsigned)grid, L, X, Y, R, nitems, C, fin);
    else if (L.K == 384) launch_tdf_persist_inst<6, false>(ctx, attr, (unsigned)grid, L, X, Y, R, nitems, C, nullptr);
    else launch_tdf_persist_inst<3, false>(ctx, attr, (unsigned)grid, L, X, Y, R, nitems, C, nullptr);
    ALSEP_HIP(ctx, attr);
    if (fin) {
        fin->done = true;
        note_launch(ctx, "tdf_bf16_wide_kernel<res,final>");
    }
    note_launch(ctx, "tdf_bf16_wide_kernel<res>");                   // one per layer launch, whichever instance serves it
    ALSEP_LAUNCH_CHECK(ctx, "tdf_bf16_persist_kernel");
    return ALSEP_OK;
}

template <int WM>
int launch_tdf_wide(alsep_ctx* ctx, const GemmLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* R, int64_t nunits, int C,
                    FinalFold* fin) {
    typedef TdfWide<WM> Tc;
    const int64_t gx = ceil_div64(nunits, Tc::UN);
    if (gx > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "tdf: too many column tiles");
    const float* bias = L.has_bias ? (const float*)L.bias.p : nullptr;
    static const int yfast = env_int("ALSEP_TDF_YFAST", 1);
    const int nrb = L.M / Tc::BM;
    const int nyb = (yfast && nrb > 1 && gx % 8 == 0 && gx * nrb <= 0x7fffffff) ? nrb : 0;
    const dim3 grid = nyb ? dim3((unsigned)(gx * nrb)) : dim3((unsigned)gx, nrb);
    ProfScope prof(ctx, ALSEP_PROF_TDF);
    static const int rpf = env_int("ALSEP_TDF_RPF", 2);
    const bool fold = WM == 4 && R && rpf != 0 && fin && C == Tc::UC && tdf_final_mode();
    if (WM == 4 && R && rpf != 0 && tdf_wide_mode() == 1 && L.M % TdfPersist::BM == 0 && (C == Tc::UC || C == 2 * Tc::UC) &&
        (L.K == 384 || L.K == 192)) {
        const int kind = fold ? kTdfPersistFinal : (L.K == 384 ? kTdfPersistK384 : kTdfPersistK192);
        const int mode = tdf_persist_mode();
        if (mode >= 2 || (mode == 1 && (kTdfPersistRouted & kind)))
            return launch_tdf_persist(ctx, L, X, Y, R, nunits, C, fold ? fin : nullptr);
    }
    if (fold) {
        ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)tdf_bf16_wide_kernel<4, true, 2, true>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)TdfWide<4>::lds_bytes));
        hipLaunchKernelGGL((tdf_bf16_wide_kernel<4, true, 2, true>), grid, dim3(TdfWide<4>::THREADS), TdfWide<4>::lds_bytes,
                           ctx->stream, X, Y, (const bf16_t*)L.wwide.p, bias, (const float*)L.scale.p, (const float*)L.shift.p, R,
                           L.M, L.K, nunits, C, nyb, fin->w, fin->b, (bf16_t*)fin->out, fin->alpha);
        fin->done = true;
        note_launch(ctx, "tdf_bf16_wide_kernel<res,final>");
    } else if (R && rpf == 0) {                                     // timing comparison only: residual rows loaded where they are used
        ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)tdf_bf16_wide_kernel<WM, true, 0>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)Tc::lds_bytes));
        hipLaunchKernelGGL((tdf_bf16_wide_kernel<WM, true, 0>), grid, dim3(Tc::THREADS), Tc::lds_bytes, ctx->stream, X, Y,
                           (const bf16_t*)L.wwide.p, bias, (const float*)L.scale.p, (const float*)L.shift.p, R, L.M, L.K,
                           nunits, C, nyb, (const float*)nullptr, (const float*)nullptr, (bf16_t*)nullptr, 0.f);
    } else if (R) {
        ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)tdf_bf16_wide_kernel<WM, true>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)Tc::lds_bytes));
        hipLaunchKernelGGL((tdf_bf16_wide_kernel<WM, true>), grid, dim3(Tc::THREADS), Tc::lds_bytes, ctx->stream, X, Y,
                           (const bf16_t*)L.wwide.p, bias, (const float*)L.scale.p, (const float*)L.shift.p, R, L.M, L.K,
                           nunits, C, nyb, (const float*)nullptr, (const float*)nullptr, (bf16_t*)nullptr, 0.f);
    } else {
        ALSEP_HIP(ctx, hipFuncSetAttribute((const void*)tdf_bf16_wide_kernel<WM, false>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)Tc::lds_bytes));
        hipLaunchKernelGGL((tdf_bf16_wide_kernel<WM, false>), grid, dim3(Tc::THREADS), Tc::lds_bytes, ctx->stream, X, Y,
                           (const bf16_t*)L.wwide.p, bias, (const float*)L.scale.p, (const float*)L.shift.p, R, L.M, L.K,
                           nunits, C, nyb, (const float*)nullptr, (const float*)nullptr, (bf16_t*)nullptr, 0.f);
    }
    note_launch(ctx, R ? "tdf_bf16_wide_kernel<res>" : "tdf_bf16_wide_kernel<nores>");
    ALSEP_LAUNCH_CHECK(ctx, "tdf_bf16_wide_kernel");
    return ALSEP_OK;
}

int run_tdf_dma(alsep_ctx* ctx, const GemmLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* R, const bf16_t* zp,
                int64_t BT, int C, FinalFold* fin) {
    typedef TdfB16 Tc;
    const int64_t nunits = BT * (C / Tc::UC);
    if (L.wwide.p && tdf_wide_mode() && L.K % 64 == 0 && nunits % 4 == 0) {
        const int mode = tdf_wide_mode();
        const bool can8 = L.M % 384 == 0;
        const bool use8 = mode == 8 ? can8 : (mode == 4 ? false : (can8 && L.M == 384 && !R));
        return use8 ? launch_tdf_wide<8>(ctx, L, X, Y, R, nunits, C, nullptr) : launch_tdf_wide<4>(ctx, L, X, Y, R, nunits, C, fin);
    }
    const int64_t gx = ceil_div64(nunits, Tc::UN);
    if (gx > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "tdf: too many column tiles");
    const float* bias = L.has_bias ? (const float*)L.bias.p : nullptr;
    ProfScope prof(ctx, ALSEP_PROF_TDF);
    const dim3 grid((unsigned)gx, L.Mp / Tc::BM);
    if (R)
        hipLaunchKernelGGL((tdf_bf16_kernel<true>), grid, dim3(kThreads), Tc::lds_bytes, ctx->stream, X, Y, (const bf16_t*)L.w.p,
                           bias, (const float*)L.scale.p, (const float*)L.shift.p, R, zp, L.M, L.K, L.Kp, nunits, C);
    else
        hipLaunchKernelGGL((tdf_bf16_kernel<false>), grid, dim3(kThreads), Tc::lds_bytes, ctx->stream, X, Y, (const bf16_t*)L.w.p,
                           bias, (const float*)L.scale.p, (const float*)L.shift.p, R, zp, L.M, L.K, L.Kp, nunits, C);
    ALSEP_LAUNCH_CHECK(ctx, "tdf_bf16_kernel");
    return ALSEP_OK;
}
int run_tdf_dma(alsep_ctx* ctx, const GemmLayer&, const float*, float*, const float*, const float*, int64_t, int, FinalFold*) {
    return alsep_fail(ctx, ALSEP_ERR_STATE, "LDS-DMA TDF path is bf16 only");
}

template <typename T>
int run_tdf(alsep_ctx* ctx, const GemmLayer& L, const T* X, T* Y, const T* R, int64_t BT, int C, const void* zero_page,
            FinalFold* fin = nullptr) {
    typedef GemmCfg<T> Gc;
#ifndef ALSEP_F16_TU
    if (L.split) return run_tdf_split(ctx, L, X, Y, R, BT, C);
#endif
    if (L.dma_path) return run_tdf_dma(ctx, L, X, Y, R, (const T*)zero_page, BT, C, fin);
    const int64_t nunits = BT * (C / 16);
    const int64_t gx = ceil_div64(nunits, 8);
    if (gx > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "tdf_gemm: too many column tiles");
    const float* bias = L.has_bias ? (const float*)L.bias.p : nullptr;
    ProfScope prof(ctx, ALSEP_PROF_TDF);
    if (R)
        hipLaunchKernelGGL((tdf_gemm_kernel<T, true>), dim3((unsigned)gx, L.Mp / Gc::BR), dim3(kThreads), Gc::lds_bytes,
                           ctx->stream, X, Y, (const T*)L.w.p, bias, (const float*)L.scale.p, (const float*)L.shift.p, R,
                           L.M, L.K, L.Kp, nunits, C);
    else
        hipLaunchKernelGGL((tdf_gemm_kernel<T, false>), dim3((unsigned)gx, L.Mp / Gc::BR), dim3(kThreads), Gc::lds_bytes,
                           ctx->stream, X, Y, (const T*)L.w.p, bias, (const float*)L.scale.p, (const float*)L.shift.p, R,
                           L.M, L.K, L.Kp, nunits, C);
    ALSEP_LAUNCH_CHECK(ctx, "tdf_gemm_kernel");
    return ALSEP_OK;
}

// TFC_TDF block: cur -> dest, using scratch a, b (cur may alias b), hidden h.  fin (last block of the network only): the
// residual TDF launch may produce the network's output instead of dest (FinalFold).
template <typename T>
int run_block(alsep_ctx* ctx, const alsep_net* net, const Block& blk, const T* cur, T* a, T* b, T* h, T* dest,
              int64_t B, int Th, int Fw, int c, FinalFold* fin = nullptr) {
    const T* src = cur;
    T* pp[2] = {a, b};
    int rc;
    const int l = (int)blk.tfc.size();
    for (int j = 0; j < l; ++j) {
        T* dst = pp[j & 1];
        if ((rc = run_conv<T>(ctx, blk.tfc[j], src, dst, B, Th, Fw, net->zero_page.p))) return rc;
        src = dst;
    }
    if (blk.tdf.size() == 2) {
        if ((rc = run_tdf<T>(ctx, blk.tdf[0], src, h, (const T*)nullptr, B * Th, c, net->zero_page.p))) return rc;
        return run_tdf<T>(ctx, blk.tdf[1], h, dest, src, B * Th, c, net->zero_page.p, fin);
    }
    return run_tdf<T>(ctx, blk.tdf[0], src, dest, src, B * Th, c, net->zero_page.p, fin);
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct WsLayout {
    size_t p0, p1, p2, h, total;
    std::vector<size_t> skip;
};

WsLayout ws_layout(const alsep_net* net, int64_t B) {
    const alsep_net_config& cfg = net->cfg;
    const size_t es = cfg.dtype == ALSEP_F32 ? 4 : 2;
    WsLayout w;
    const size_t s0 = align256((size_t)B * cfg.dim_t * cfg.dim_f * cfg.g * es);
    size_t off = 0;
    w.p0 = off; off += s0;
    w.p1 = off; off += s0;
    w.p2 = off; off += s0;
    w.h = off;  off += align256(cfg.bn > 0 ? s0 / cfg.bn : 16);
    int c = cfg.g;
    size_t t = cfg.dim_t, f = cfg.dim_f;
    for (int i = 0; i < net->n; ++i) {
        w.skip.push_back(off);
        off += align256((size_t)B * t * f * c * es);
        c += cfg.g; t /= 2; f /= 2;
    }
    w.total = off;
    return w;
}

// the PCM side of a fused front end: frames of `plan` cut from pcm as alsep_stft cuts them
struct PcmFront {
    const alsep_plan* plan;
    const float* pcm;
    int64_t ch_stride, chunk_stride;
    int zero_low;
};

template <typename T>
int forward_impl(alsep_ctx* ctx, const alsep_net* net, const T* in, T* out, int64_t B, char* ws, float in_scale,
                 float out_alpha, float out_beta, const PcmFront* front = nullptr) {
    const alsep_net_config& cfg = net->cfg;
    const WsLayout L = ws_layout(net, B);
    T* P[3] = {(T*)(ws + L.p0), (T*)(ws + L.p1), (T*)(ws + L.p2)};
    T* H = (T*)(ws + L.h);
    int Th = cfg.dim_t, Fw = cfg.dim_f, c = cfg.g;
    const int64_t npix0 = B * Th * Fw;
    int rc;
    if (front) {
        // STFT + first 1x1 convolution in one kernel: the level-0 activation straight from the PCM, no spectrogram in HBM
        if ((rc = ALSEP_TU_NAME(alsep_stft_first_conv)(ctx, front->plan, front->pcm, front->ch_stride, front->chunk_stride, B, P[0],
                                                       (const float*)net->first_w.p, (const float*)net->first_scale.p,
                                                       (const float*)net->first_shift.p, cfg.g, in_scale, front->zero_low)))
            return rc;
    } else {
        ProfScope prof(ctx, ALSEP_PROF_POINTWISE);
        const int ppb = kFirstThreads / (cfg.g / Vec16<T>::N);
        const int64_t nblk = std::min<int64_t>(ceil_div64(npix0, ppb), 256 * 16);
        hipLaunchKernelGGL((first_conv_kernel<T>), dim3((unsigned)nblk), dim3(kFirstThreads), 0,
                           ctx->stream, in, P[0], (const float*)net->first_w.p, (const float*)net->first_scale.p,
                           (const float*)net->first_shift.p, npix0, cfg.g, in_scale);
        ALSEP_LAUNCH_CHECK(ctx, "first_conv_kernel");
    }
    // the last block may write `out` itself; the accumulating pass of a denoise pair (out_beta != 0) keeps the separate kernel
    FinalFold fold = {(const float*)net->final_w.p, (const float*)net->final_b.p, out, out_alpha, false};
    FinalFold* const fin = (!std::is_same<T, float>::value && out_beta == 0.f) ? &fold : nullptr;
    // rotating buffers: cur = P[ic]; the block uses the other two as scratch
    int ic = 0;
    for (int i = 0; i < net->n; ++i) {
        T* skip = (T*)(ws + L.skip[i]);
        if ((rc = run_block<T>(ctx, net, net->enc[i], P[ic], P[(ic + 1) % 3], P[(ic + 2) % 3], H, skip, B, Th, Fw, c))) return rc;
        // ds: skip [B,Th,Fw,c] -> P[ic] [B,Th/2,Fw/2,c+g]
        const int Tp = Th / 2, Fp = Fw / 2;
        if ((rc = run_pix<T, PIX_DS>(ctx, net->ds[i], skip, P[ic], (const T*)nullptr, B * Tp * Fp, Tp, Fp, c, c + cfg.g))) return rc;
        Th = Tp; Fw = Fp; c += cfg.g;
    }
    {
        T* dest = P[(ic + 1) % 3];
        if ((rc = run_block<T>(ctx, net, net->bott, P[ic], P[(ic + 2) % 3], P[ic], H, dest, B, Th, Fw, c, net->n == 0 ? fin : nullptr)))
            return rc;
        ic = (ic + 1) % 3;
    }
    for (int i = 0; i < net->n; ++i) {
        const T* skip = (const T*)(ws + L.skip[net->n - 1 - i]);
        const int c2 = c - cfg.g;
        T* up = P[(ic + 1) % 3];
        // us: P[ic] [B,Th,Fw,c] -> up [B,2Th,2Fw,c2] * skip
        if ((rc = run_pix<T, PIX_US>(ctx, net->us[i], P[ic], up, skip, B * Th * Fw, Th, Fw, c, c2))) return rc;
        Th *= 2; Fw *= 2; c = c2;
        T* dest = P[ic];                                   // old input is dead after the up conv
        if ((rc = run_block<T>(ctx, net, net->dec[i], up, P[(ic + 2) % 3], up, H, dest, B, Th, Fw, c, i == net->n - 1 ? fin : nullptr)))
            return rc;
    }
    if (fold.done) return ALSEP_OK;
    ProfScope prof(ctx, ALSEP_PROF_POINTWISE);
    hipLaunchKernelGGL((final_conv_kernel<T>), dim3((unsigned)ceil_div64(npix0, kThreads)), dim3(kThreads),
                       (size_t)kThreads * cfg.g * sizeof(T), ctx->stream,
                       (const T*)P[ic], out, (const float*)net->final_w.p, (const float*)net->final_b.p, npix0, cfg.g, out_alpha, out_beta);
    ALSEP_LAUNCH_CHECK(ctx, "final_conv_kernel");      // also counts the launch under that name
    return ALSEP_OK;
}

}  // namespace

// the IEEE-half twins of the four entry points below, defined by tdfnet_f16.hip (this file compiled with ALSEP_F16_TU)
extern "C" int alsep_net_create_f16tu(alsep_ctx*, const alsep_net_config*, const alsep_tensor*, int64_t, alsep_net**);
extern "C" int alsep_net_destroy_f16tu(alsep_net*);
extern "C" int64_t alsep_net_workspace_bytes_f16tu(const alsep_net*, int64_t);
extern "C" int alsep_net_forward_f16tu(alsep_ctx*, const alsep_net*, const void*, void*, int64_t, void*, int64_t, float, float, float);

extern "C" int ALSEP_TU_NAME(alsep_net_create)(alsep_ctx* ctx, const alsep_net_config* cfg, const alsep_tensor* tensors,
                                int64_t n_tensors, alsep_net** out) {
    ALSEP_ENTER(ctx);
#ifndef ALSEP_F16_TU
    if (ctx && cfg && cfg->dtype == ALSEP_F16) return alsep_net_create_f16tu(ctx, cfg, tensors, n_tensors, out);
#endif
    if (!ctx || !cfg || !tensors || !out) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_create: null argument");
    const int n = cfg->num_blocks / 2;
    if (cfg->num_blocks < 1 || cfg->l < 1 || cfg->g < 16 || cfg->g % 16 != 0 || cfg->bn < 0 ||
        (cfg->dtype != ALSEP_F32 && cfg->dtype != ALSEP_HALF_DTYPE))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_create: unsupported config (g must be a multiple of 16)");
    if ((cfg->flags & ~ALSEP_NET_SPLIT_F16) != 0 || ((cfg->flags & ALSEP_NET_SPLIT_F16) && cfg->dtype != ALSEP_F32))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_create: unknown flags, or ALSEP_NET_SPLIT_F16 on a network that is not float32");
    if (cfg->dim_f % (1 << n) != 0 || cfg->dim_t % (1 << n) != 0 ||
        (cfg->bn > 0 && (cfg->dim_f >> n) % cfg->bn != 0))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_create: dim_f/dim_t not divisible by 2^%d (and bn)", n);
    TensorMap tm;
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (!tensors[i].name || !tensors[i].data || tensors[i].numel < 0)
            return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_create: bad tensor entry %lld", (long long)i);
        std::vector<float> h((size_t)tensors[i].numel);
        if (tensors[i].numel)
            ALSEP_HIP(ctx, hipMemcpy(h.data(), tensors[i].data, sizeof(float) * h.size(), hipMemcpyDeviceToHost));
        tm[tensors[i].name] = std::move(h);
    }
    alsep_net* net = new alsep_net();
    net->ctx = ctx;
    net->cfg = *cfg;
    net->n = n;
    net->split = cfg->dtype == ALSEP_F32 && (cfg->flags & ALSEP_NET_SPLIT_F16) != 0;
    const int rc = cfg->dtype == ALSEP_F32 ? build_net<float>(net, tm) : build_net<bf16_t>(net, tm);
    if (rc) {
        const std::string keep = ctx->err;
        ALSEP_TU_NAME(alsep_net_destroy)(net);
        ctx->err = keep;
        return rc;
    }
    *out = net;
    return ALSEP_OK;
}

extern "C" int ALSEP_TU_NAME(alsep_net_destroy)(alsep_net* net) {
    if (!net) return ALSEP_OK;
#ifndef ALSEP_F16_TU
    if (net->cfg.dtype == ALSEP_F16) return alsep_net_destroy_f16tu(net);
#endif
    for (auto& b : net->owned)
        if (b.p) (void)hipFree(b.p);
    delete net;
    return ALSEP_OK;
}

extern "C" int64_t ALSEP_TU_NAME(alsep_net_workspace_bytes)(const alsep_net* net, int64_t B) {
    if (!net || B <= 0) return 0;
#ifndef ALSEP_F16_TU
    if (net->cfg.dtype == ALSEP_F16) return alsep_net_workspace_bytes_f16tu(net, B);
#endif
    return (int64_t)ws_layout(net, B).total;
}

extern "C" int ALSEP_TU_NAME(alsep_net_forward)(alsep_ctx* ctx, const alsep_net* net, const void* spec_in, void* spec_out,
                                 int64_t B, void* workspace, int64_t workspace_bytes, float in_scale,
                                 float out_alpha, float out_beta) {
    ALSEP_ENTER(ctx);
#ifndef ALSEP_F16_TU
    if (net && net->cfg.dtype == ALSEP_F16)
        return alsep_net_forward_f16tu(ctx, net, spec_in, spec_out, B, workspace, workspace_bytes, in_scale, out_alpha, out_beta);
#endif
    if (!ctx || !net || !spec_in || !spec_out || !workspace) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_forward: null argument");
    if (B == 0) return ALSEP_OK;
    if (B < 0) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_forward: negative batch");
    if (workspace_bytes < ALSEP_TU_NAME(alsep_net_workspace_bytes)(net, B))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_forward: workspace too small (%lld < %lld)",
                          (long long)workspace_bytes, (long long)ALSEP_TU_NAME(alsep_net_workspace_bytes)(net, B));
    if (((uintptr_t)workspace & 255) != 0) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_forward: workspace must be 256-byte aligned");
    if (net->cfg.dtype == ALSEP_F32)
        return forward_impl<float>(ctx, net, (const float*)spec_in, (float*)spec_out, B, (char*)workspace, in_scale, out_alpha, out_beta);
    return forward_impl<bf16_t>(ctx, net, (const bf16_t*)spec_in, (bf16_t*)spec_out, B, (char*)workspace, in_scale, out_alpha, out_beta);
}

// 1 when a float32 network with split-half contractions (ALSEP_NET_SPLIT_F16) has met an operand beyond the half range (|x| > 65504, or
// not a number) in any forward since the last call -- its results are then invalid; reads and clears the word (synchronises the stream).
// 0 for every other network.
#ifndef ALSEP_F16_TU
extern "C" int alsep_net_range_flag(alsep_ctx* ctx, alsep_net* net, int32_t* out) {
    ALSEP_ENTER(ctx);
    if (!ctx || !net || !out) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_range_flag: null argument");
    *out = 0;
    if (!net->split || !net->range_flag.p) return ALSEP_OK;
    unsigned v = 0;
    ALSEP_HIP(ctx, hipMemcpyAsync(&v, net->range_flag.p, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    ALSEP_HIP(ctx, hipMemsetAsync(net->range_flag.p, 0, sizeof(v), ctx->stream));
    ALSEP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out = v != 0;
    return ALSEP_OK;
}
#endif

extern "C" int alsep_net_forward_pcm_f16tu(alsep_ctx*, const alsep_net*, const alsep_plan*, const float*, int64_t, int64_t, void*, int64_t, void*,
                                           int64_t, float, float, float, int);

// alsep_stft + alsep_net_forward in one call for the half-precision networks, with the STFT and the network's first layer fused into ONE
// kernel (fft_r16.h, FUSE): the same results bit for bit, without the spectrogram's HBM round trip.  ALSEP_ERR_STATE when this
// (plan, network) pair has no fused kernel (float32 network, g != 48, n_fft other than 4096 / 6144 / 7680): call the two functions then.
extern "C" int ALSEP_TU_NAME(alsep_net_forward_pcm)(alsep_ctx* ctx, const alsep_net* net, const alsep_plan* plan, const float* pcm,
                                                    int64_t ch_stride, int64_t chunk_stride, void* spec_out, int64_t B, void* workspace,
                                                    int64_t workspace_bytes, float in_scale, float out_alpha, float out_beta, int zero_low_bins) {
    ALSEP_ENTER(ctx);
#ifndef ALSEP_F16_TU
    if (net && net->cfg.dtype == ALSEP_F16)
        return alsep_net_forward_pcm_f16tu(ctx, net, plan, pcm, ch_stride, chunk_stride, spec_out, B, workspace, workspace_bytes, in_scale,
                                           out_alpha, out_beta, zero_low_bins);
#endif
    if (!ctx || !net || !plan || !pcm || !spec_out || !workspace) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_forward_pcm: null argument");
    if (net->cfg.dtype == ALSEP_F32) return ALSEP_ERR_STATE;
    if (B == 0) return ALSEP_OK;
    if (B < 0 || zero_low_bins < 0) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_forward_pcm: bad argument");
    if (workspace_bytes < ALSEP_TU_NAME(alsep_net_workspace_bytes)(net, B))
        return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_forward_pcm: workspace too small");
    if (((uintptr_t)workspace & 255) != 0) return alsep_fail(ctx, ALSEP_ERR_ARG, "alsep_net_forward_pcm: workspace must be 256-byte aligned");
    const PcmFront front{plan, pcm, ch_stride, chunk_stride, zero_low_bins};
    return forward_impl<bf16_t>(ctx, net, (const bf16_t*)nullptr, (bf16_t*)spec_out, B, (char*)workspace, in_scale, out_alpha, out_beta, &front);
}
