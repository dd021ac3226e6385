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
// The four persistent 8-wave 3x3 convolutions (big, mq, m0, allco) and the scaffold they share are in tdfnet_conv8.h; their weight
// packers, launchers and the dispatch (run_conv_dma) are here.
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

#include "tdfnet_conv8.h"   // the persistent 8-wave 3x3 convolutions (big, mq, m0, allco) and the scaffold they share

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
//   * USF (NT = 3, C = 96): the 2x2 stride-2 transposed conv 96 -> 48 that follows the block, times the level-0 skip, is
//     computed here and Y is never written.  An item is one frame (both 48-channel halves), so after the epilogue above a wave
//     holds 48 whole level-1 pixels, rounded once to the storage type as the store would have: unit 0's stay in registers
//     while unit 1 goes through the staging rows, then both take the staging rows' place as [48 px][96 c] and become the B
//     fragments (9 x 16 bytes per lane).  The us weights (A operand, 36 KiB in fragment order, in LDS once per workgroup) meet
//     them in chunks of one output row dy x 16 input pixels = 32 output pixels x 48 channels: one accumulator per (tap, m-tile,
//     16-pixel block) over ks = 0, 1, 2 -- us_stream_kernel<96, 48>'s chains -- then relu(bn(.)) in fp32 through the staging
//     rows, times the skip in fp32, one rounding, whole 3 KiB runs of 16-byte stores (the 48 rows are 9216 contiguous bytes
//     of frame 2t and of frame 2t + 1).  The skip runs are requested kUsfAhead chunks ahead, the first ones behind unit 0's
//     TDF epilogue.  No LDS-DMA is in flight in a row block, so these compiler-tracked loads get counted waits.
// LDS: 72 KiB tile + 8 x 9.75 KiB staging + 0.75 KiB scale/shift (+ 6 KiB final weights) = 156.75 KiB: one workgroup of
// eight waves per CU, two waves per SIMD.  USF: 36 + 78 + 0.75 + 36.4 = 151.1 KiB.
// ------------------------------------------------------------------------------------------
struct TdfPersist {
    static constexpr int WV = 8, TR = 48, BM = TR * WV, UN = 2, UC = 48, BK = 64;
    static constexpr int THREADS = 64 * WV;
    static constexpr int STAGE_ELEMS = UN * BK * UC;                 // one K tile of both units: 12 KiB
    static constexpr int SS = TdfWide<4>::SS, FS = TdfWide<4>::FS, FWN = TdfWide<4>::FWN;
    static constexpr size_t stage_bytes = (size_t)WV * TR * SS * sizeof(float);
    static constexpr size_t bn_bytes = (size_t)UN * 2 * UC * sizeof(float);
    static constexpr size_t tile_bytes(int nt) { return (size_t)nt * STAGE_ELEMS * sizeof(bf16_t); }
    // USF (C = 96 -> 48 upsampling folded in): XS = row stride of the wave's rounded pixels [48 f'][96 c] bf16, which take the
    // place of its fp32 staging rows; the us layer's fragment-order weights [4 taps][3 m-tiles][3 k-steps][64 lanes][8] and its
    // scale | shift lie behind the TDF scale / shift
    static constexpr int XS = 104, USC = 96, USC2 = 48, US_MT = 3, US_KS = 3, US_NB = TR / 16;
    static constexpr size_t usw_bytes = (size_t)4 * US_MT * US_KS * 64 * 8 * sizeof(bf16_t);
    static constexpr size_t usf_bytes = usw_bytes + 2 * USC2 * sizeof(float);
    static constexpr size_t lds_bytes(int nt, bool fin, bool usf = false) {
        return tile_bytes(nt) + stage_bytes + bn_bytes + (fin ? WV * FWN * sizeof(float) : 0) + (usf ? usf_bytes : 0);
    }
    static_assert((size_t)TR * FS * sizeof(bf16_t) <= (size_t)TR * SS * sizeof(float), "FINAL: the rounded rows fit in the staging rows");
    static_assert((size_t)TR * XS * sizeof(bf16_t) <= (size_t)TR * SS * sizeof(float) && XS >= USC && XS % 8 == 0,
                  "USF: the rounded pixels fit in the staging rows, 16-byte aligned");
    static_assert((size_t)32 * SS * sizeof(float) <= (size_t)TR * SS * sizeof(float), "USF: 32 output pixels of a chunk in the staging rows");
};
// The 96 -> 48 upsampling that follows a level-1 block, folded into tdf_bf16_persist_kernel<3, false, true>: the us layer's
// fragment-order weights, BN scale / shift, the level-0 skip it multiplies by and the level-0 activation it writes.
struct UsFoldArgs {
    const bf16_t* w;
    const float* scale;
    const float* shift;
    const bf16_t* skip;
    bf16_t* out;
};

// glds16 with the source as wave-uniform global base + 32-bit lane offset (one address VGPR, no 64-bit lane pointer)
__device__ __forceinline__ void glds16_base(const ALSEP_GLOBAL char* gbase, unsigned lane_off, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const ALSEP_GLOBAL void*)(gbase + lane_off), (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

constexpr int kUsfAhead = 3;                                         // USF: skip runs requested this many chunks ahead (12 VGPRs each)

template <int NT, bool FINAL, bool USF = false>
__global__ void __launch_bounds__(TdfPersist::THREADS, 1)
tdf_bf16_persist_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ Wf,
                        const float* __restrict__ bias, const float* __restrict__ scale, const float* __restrict__ shift,
                        const bf16_t* __restrict__ R, int M, int64_t nitems, int C,
                        const float* __restrict__ FW, const float* __restrict__ FB, bf16_t* __restrict__ FOUT, float falpha,
                        UsFoldArgs UF) {
    typedef TdfPersist Tc;
    static_assert(NT % 3 == 0 && NT >= 3, "three weight buffers: a K tile's buffer is the same in every row block");
    static_assert(Tc::lds_bytes(NT, FINAL, USF) <= 160 * 1024, "LDS of a CU");
    static_assert(!USF || (NT == 3 && !FINAL), "USF: the level-1 residual linear (K = 192), launched with C = 96");
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
    // USF only: behind the TDF scale / shift; both are complete behind the first item's barrier
    bf16_t* usw = reinterpret_cast<bf16_t*>(alsep_smem + Tc::tile_bytes(NT) + Tc::stage_bytes + Tc::bn_bytes);
    float* usbn = reinterpret_cast<float*>(alsep_smem + Tc::tile_bytes(NT) + Tc::stage_bytes + Tc::bn_bytes + Tc::usw_bytes);   // [scale | shift][48]
    if constexpr (USF) {
        for (int i = tid; i < (int)(Tc::usw_bytes / 16); i += Tc::THREADS)
            *reinterpret_cast<bf16x8*>(usw + (size_t)i * 8) = *reinterpret_cast<const bf16x8*>(UF.w + (size_t)i * 8);
        if (tid < 2 * Tc::USC2) usbn[tid] = (tid < Tc::USC2 ? UF.scale : UF.shift)[tid % Tc::USC2];
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
            // USF: chunk ch = dy * 3 + nb is output row 2 t + dy, output pixels 2 (48 rowblk + 16 nb) + [0, 32): 3 KiB, contiguous
            // in the skip and in the output alike; lane l moves bytes [16 l, 16 l + 16) of each of its three KiB
            constexpr int USF_CHUNKS = 2 * Tc::US_NB;
            auto usf_chunk_off = [&](int ch) {
                return ((2 * (u0 >> 1) + ch / Tc::US_NB) * (2 * (int64_t)M) + 2 * (rowblk * Tc::TR + (ch % Tc::US_NB) * 16)) * Tc::USC2;
            };
            bf16x8 skv[USF ? USF_CHUNKS : 1][3];
            auto usf_load_skip = [&](int ch) {
                const ALSEP_GLOBAL char* sp = opaque_uniform_gptr(reinterpret_cast<const char*>(UF.skip + usf_chunk_off(ch)));
#pragma unroll
                for (int g = 0; g < 3; ++g) skv[ch][g] = *reinterpret_cast<const ALSEP_GLOBAL bf16x8*>(sp + woff + g * 1024);
            };
            bf16x8 qq[Tc::UN][5];                                    // USF: both units' rounded rows
#pragma unroll
            for (int u = 0; u < Tc::UN; ++u) {
                ALSEP_GLOBAL char* yb = const_cast<ALSEP_GLOBAL char*>(                    // USF: Y is null and never written
                    opaque_uniform_gptr(reinterpret_cast<const char*>(USF ? (const bf16_t*)nullptr : Y + unit_base(u))));
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
                        if (!FINAL && !USF) stream_store(reinterpret_cast<ALSEP_GLOBAL bf16x8*>(yb + loff[g]), q[g]);
                        if (USF) qq[u][g] = q[g];
                    }
                }
                __builtin_amdgcn_wave_barrier();
                if constexpr (USF) {
                    // the first skip runs, under unit 1's epilogue (unit 0's accumulators and residual rows are dead: room for them)
                    if (u == 0) {
#pragma unroll
                        for (int ch = 0; ch < kUsfAhead && ch < USF_CHUNKS; ++ch) usf_load_skip(ch);
                    }
                }
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
            if constexpr (USF) {
                // every staging row is read: the wave's 48 rounded pixels [48 f'][96 c] take their place (unit u = channels 48 u ..)
                // lane coordinates recomputed here, not kept (or spilled) across the k loop
                const int ln = opaque_vgpr(lane), ul15 = ln & 15, ulq = ln >> 4;
                bf16_t* xr = reinterpret_cast<bf16_t*>(stg);
#pragma unroll
                for (int u = 0; u < Tc::UN; ++u)
#pragma unroll
                    for (int g = 0; g < 5; ++g) {
                        const int gidx = g * 64 + ln;
                        if (gidx < Tc::TR * 6) *reinterpret_cast<bf16x8*>(xr + (gidx / 6) * Tc::XS + u * Tc::UC + (gidx % 6) * 8) = qq[u][g];
                    }
                __builtin_amdgcn_wave_barrier();
                bf16x8 xb[Tc::US_NB][Tc::US_KS];                     // B fragments: pixel 16 nb + l15, channels 32 ks + 8 lq ..
#pragma unroll
                for (int nb = 0; nb < Tc::US_NB; ++nb)
#pragma unroll
                    for (int ks = 0; ks < Tc::US_KS; ++ks)
                        xb[nb][ks] = *reinterpret_cast<const bf16x8*>(xr + (nb * 16 + ul15) * Tc::XS + ks * 32 + ulq * 8);
                __builtin_amdgcn_wave_barrier();                     // the chunks' fp32 rows overwrite these
#pragma unroll
                for (int ch = 0; ch < USF_CHUNKS; ++ch) {
                    const int dy = ch / Tc::US_NB, nb = ch % Tc::US_NB;
                    if (ch + kUsfAhead < USF_CHUNKS) usf_load_skip(ch + kUsfAhead);
                    f32x4 ua[2][Tc::US_MT];
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
                        for (int mt = 0; mt < Tc::US_MT; ++mt) ua[dx][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    // six independent chains side by side, each over ks ascending (us_stream_kernel: tap = wave, wf[mt][ks])
#pragma unroll
                    for (int ks = 0; ks < Tc::US_KS; ++ks)
#pragma unroll
                        for (int dx = 0; dx < 2; ++dx)
#pragma unroll
                            for (int mt = 0; mt < Tc::US_MT; ++mt) {
                                const bf16x8 wa = *reinterpret_cast<const bf16x8*>(
                                    usw + ((size_t)(((dy * 2 + dx) * Tc::US_MT + mt) * Tc::US_KS + ks) * 64 + ln) * 8);
                                mma_step(ua[dx][mt], wa, xb[nb][ks]);
                            }
                    // relu(bn(.)) in fp32 at output pixel 2 j + dx of the chunk's 32
#pragma unroll
                    for (int mt = 0; mt < Tc::US_MT; ++mt) {
                        const f32x4 sc = *reinterpret_cast<const f32x4*>(usbn + mt * 16 + 4 * ulq);
                        const f32x4 sh = *reinterpret_cast<const f32x4*>(usbn + Tc::USC2 + mt * 16 + 4 * ulq);
#pragma unroll
                        for (int dx = 0; dx < 2; ++dx) {
                            f32x4 y;
#pragma unroll
                            for (int r = 0; r < 4; ++r) y[r] = fmaxf(fmaf(ua[dx][mt][r], sc[r], sh[r]), 0.f);
                            *reinterpret_cast<f32x4*>(stg + (2 * l15 + dx) * Tc::SS + mt * 16 + 4 * ulq) = y;
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    ALSEP_GLOBAL char* ob = const_cast<ALSEP_GLOBAL char*>(
                        opaque_uniform_gptr(reinterpret_cast<const char*>(UF.out + usf_chunk_off(ch))));
#pragma unroll
                    for (int g = 0; g < 3; ++g) {                    // 32 pixels x 6 groups of 8 channels = 3 per lane
                        const int gidx = g * 64 + ln;
                        const float* src = stg + (gidx / 6) * Tc::SS + (gidx % 6) * 8;
                        const f32x4 lo = *reinterpret_cast<const f32x4*>(src);
                        const f32x4 hi = *reinterpret_cast<const f32x4*>(src + 4);
                        const bf16x8 sk = skv[ch][g];
                        bf16x8 q;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { q[e] = (bf16_t)(lo[e] * (float)sk[e]); q[4 + e] = (bf16_t)(hi[e] * (float)sk[4 + e]); }
                        stream_store(reinterpret_cast<ALSEP_GLOBAL bf16x8*>(ob + (unsigned)ln * 16u + g * 1024), q);
                    }
                    __builtin_amdgcn_wave_barrier();                 // the next chunk's rows overwrite these
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
// Both TDF linears of a block in one launch (levels 2 and 3: F = 768 / 384, hidden H = F / 8, C a multiple of 48):
//   y = x + relu(bn2(W2 . relu(bn1(W1 . x + b1)) + b2))
// with the arithmetic of the two tdf_bf16_kernel launches it replaces -- x fragments are the MFMA A operand by transpose read, a
// 32-wide k-step is composed as there, k ascends within every accumulator, the hidden tile is rounded to the storage type, bias,
// BN, ReLU and the residual add are fp32 with one rounding -- so the output is the same bits.  Different traffic: x is read from
// memory once, y is written once, the hidden tensor never leaves the CU.
//   * a work item is 768 tile rows of 48 channels: one unit (one (b, t), one 48-channel group) at F = 768, two consecutive units at
//     F = 384; persistent 8-wave workgroups, one per CU, stride statically over the items;
//   * the item's tile (72 KiB) comes into one of two LDS buffers by LDS-DMA, nine 1 KiB pieces per wave, requested behind the
//     first barrier of the item before -- it lands under that item's MFMAs and stores; it is the A operand of the first linear and
//     the residual of the second;
//   * ALL weight fragments stay in registers for the whole launch, loaded once per wave from fragment-order images
//     (make_tdf_fused_weights): waves 0..5 own one 16-row m-tile of the hidden tile each (F / 32 fragments: 96 VGPRs at F = 768), every
//     wave owns tile rows [96 w, 96 w + 96) of the second linear (6 m-tiles x ceil(H / 32) fragments: 72 VGPRs).  Inside the item
//     loop a wave issues nothing that counts on vmcnt but its nine LDS-DMAs and, behind them, its nine stores, so the one wait per
//     item is vmcnt(9): the tile has landed, the stores of the item before may still be in flight;
//   * phase A: waves 0..5, 3 accumulators over F / 32 k-steps, fragment reads one k-step ahead; relu(bn1(.)) rounded into the hidden
//     tile [H (+ zero rows up to a multiple of 32)][48] in LDS.  Barrier.  Phase B: per 16-row m-tile 3 accumulators over the hidden
//     tile's k-steps (the all-zero k-step that Kp = 128 adds at H = 96 is left out: it adds +0 to accumulators that are never -0);
//     the lane reads its residual values from the tile, adds, rounds once and writes the result over them; then the wave's 96 rows
//     leave as nine whole-row 16-byte stores per lane;
//   * two barriers per item (tile landed / hidden tile complete); every LDS access in the item loop is asm with its own lgkmcnt
//     wait (a compiler-tracked one would be given s_waitcnt vmcnt(0) for the LDS-DMA in flight, as in ds_pipe_kernel).
// LDS: 2 x 72 KiB + 9 / 12 KiB hidden + 3 KiB scale / shift = 156 / 159 KiB.
// ------------------------------------------------------------------------------------------
template <int F_>
struct TdfFused {
    static constexpr int F = F_, H = F_ / 8, UC = 48, WV = 8, THREADS = 64 * WV;
    static constexpr int ROWS = 768, NU = ROWS / F_;                 // tile rows of an item; units per item
    static constexpr int KS1 = F_ / 32, HM = H / 16;                 // k-steps of the first linear; m-tiles of a unit's hidden tile
    static constexpr int HR = (H + 31) / 32 * 32, KS2 = HR / 32;     // hidden rows per unit in LDS (zero beyond H); k-steps of the second
    static constexpr int WR = ROWS / WV, MT2 = WR / 16;              // tile rows and m-tiles of a wave in phase B
    static constexpr int ND = WR * UC * (int)sizeof(bf16_t) / 1024;  // LDS-DMA pieces, and stores, per wave and item: 9
    static constexpr int WA = NU * HM;                               // waves of phase A
    static constexpr int CMAX = 192;                                 // channels the scale / shift table holds
    static constexpr size_t tile_bytes = (size_t)ROWS * UC * sizeof(bf16_t);
    static constexpr size_t h_bytes = (size_t)NU * HR * UC * sizeof(bf16_t);
    static constexpr size_t lds_bytes = 2 * tile_bytes + h_bytes + 4 * CMAX * sizeof(float);
    static_assert(NU * F_ == ROWS && H % 16 == 0 && WA <= WV && F_ % WR == 0 && ND * 1024 == WR * UC * (int)sizeof(bf16_t) && WR % 32 == 0,
                  "fused TDF geometry");
    static_assert(lds_bytes <= 160 * 1024, "LDS of a CU");
};

#ifdef ALSEP_CPU_EMUL
template <int OFF>
static inline void lds_read_async_b64(bf16x4& dst, const bf16_t* lds_ptr) { std::memcpy(&dst, reinterpret_cast<const char*>(lds_ptr) + OFF, 8); }
#else
// lds_read_async_b128 for four 16-bit values
template <int OFF>
__device__ __forceinline__ void lds_read_async_b64(bf16x4& dst, const bf16_t* lds_ptr) {
    static_assert(OFF >= 0 && OFF < 65536 && OFF % 8 == 0, "ds offset field");
    const unsigned addr = (unsigned)(unsigned long long)(__attribute__((address_space(3))) const void*)lds_ptr;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
#endif

template <int F_>
__global__ void __launch_bounds__(TdfFused<F_>::THREADS, 1)
tdf_bf16_fused_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y, const bf16_t* __restrict__ W1f,
                      const bf16_t* __restrict__ W2f, const float* __restrict__ bias1, const float* __restrict__ scale1,
                      const float* __restrict__ shift1, const float* __restrict__ bias2, const float* __restrict__ scale2,
                      const float* __restrict__ shift2, int nitems, int C) {
    typedef TdfFused<F_> P;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    char* tiles = alsep_smem;
    bf16_t* ht = reinterpret_cast<bf16_t*>(alsep_smem + 2 * P::tile_bytes);
    float* bnl = reinterpret_cast<float*>(alsep_smem + 2 * P::tile_bytes + P::h_bytes);      // [scale1 | shift1 | scale2 | shift2][CMAX]
    const int upc = C / P::UC;

    for (int i = tid; i < 4 * C; i += P::THREADS) {
        const int w = i / C, c = i % C;
        bnl[w * P::CMAX + c] = (w == 0 ? scale1 : (w == 1 ? shift1 : (w == 2 ? scale2 : shift2)))[c];
    }
    if (P::HR > P::H) {                                              // the k rows beyond H of the second linear's last k-step
        constexpr int ZG = (P::HR - P::H) * P::UC / 8;
        for (int i = tid; i < P::NU * ZG; i += P::THREADS)
            *reinterpret_cast<bf16x8*>(ht + ((i / ZG) * P::HR + P::H) * P::UC + (i % ZG) * 8) = bf16x8{};
    }

    // phase A: wave w < WA owns m-tile mia of unit ua's hidden tile; phase B: every wave owns tile rows [WR w, WR w + WR) = rows
    // [f0, f0 + WR) of unit ub -- the same rows it fills and stores
    const bool wa = wave < P::WA;
    const int ua = wa ? wave / P::HM : 0, mia = wa ? wave % P::HM : 0;
    const int ub = (wave * P::WR) / P::F, f0 = (wave * P::WR) % P::F;
    bf16x8 w1[P::KS1], w2[P::MT2][P::KS2];
#pragma unroll
    for (int ks = 0; ks < P::KS1; ++ks)
        w1[ks] = wa ? *reinterpret_cast<const bf16x8*>(W1f + ((size_t)(mia * P::KS1 + ks) * 64 + lane) * 8) : bf16x8{};
    float b2[P::MT2];
#pragma unroll
    for (int mi = 0; mi < P::MT2; ++mi) {
#pragma unroll
        for (int ks = 0; ks < P::KS2; ++ks)
            w2[mi][ks] = *reinterpret_cast<const bf16x8*>(W2f + ((size_t)((f0 / 16 + mi) * P::KS2 + ks) * 64 + lane) * 8);
        b2[mi] = bias2 ? bias2[f0 + mi * 16 + l15] : 0.f;
    }
    const float b1 = (wa && bias1) ? bias1[mia * 16 + l15] : 0.f;

    // three pieces of 1 KiB are 32 rows of 96 bytes: piece q of a wave's nine lies (q / 3) * 32 rows below piece q % 3
    unsigned xoff[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int within = j * 64 + lane;
        xoff[j] = (unsigned)(((within / 6) * C + (within % 6) * 8) * (int)sizeof(bf16_t));
    }
    const int trow = l15 >> 2, tcol = (l15 & 3) * 4;
    const unsigned xa_off = (unsigned)(((ua * P::F + 4 * lq + trow) * P::UC + tcol) * (int)sizeof(bf16_t));     // phase A fragments, in the tile
    const bf16_t* hl = ht + (ub * P::HR + 4 * lq + trow) * P::UC + tcol;                                       // phase B fragments
    bf16_t* hw = ht + (ua * P::HR + mia * 16 + l15) * P::UC + 4 * lq;                                          // phase A result
    const unsigned eb_off = (unsigned)(((wave * P::WR + l15) * P::UC + 4 * lq) * (int)sizeof(bf16_t));        // phase B residual / result
    const unsigned co_off = (unsigned)(wave * P::ND * 1024 + lane * 16);                                       // copy-out

    const int nmy = (nitems - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    // unit u of this workgroup's item i: its first channel, and the element offset in X / Y of its row 0 there
    auto unit_cb = [&](int i, int u) { return ((((int)blockIdx.x + i * (int)gridDim.x) * P::NU + u) % upc) * P::UC; };
    auto unit_base = [&](int i, int u) {
        const int un = ((int)blockIdx.x + i * (int)gridDim.x) * P::NU + u;
        return ((int64_t)(un / upc) * P::F) * C + (un % upc) * P::UC;
    };
    auto issue = [&](int i) {
        const ALSEP_GLOBAL char* src = opaque_uniform_gptr(reinterpret_cast<const char*>(X + unit_base(i, ub) + (int64_t)f0 * C));
        char* dst = tiles + (size_t)(i & 1) * P::tile_bytes + (size_t)wave * (P::ND * 1024);
#pragma unroll
        for (int q = 0; q < P::ND; ++q) glds16_base(src + (size_t)(q / 3) * 32 * C * sizeof(bf16_t), xoff[q % 3], dst + q * 1024);
    };

    wait_vmcnt<0>();                                                 // weights and biases are in registers
    if (nmy > 0) issue(0);
    for (int i = 0; i < nmy; ++i) {
        if (i > 0) wait_vmcnt<P::ND>();                              // behind DMA(i) this wave has issued the ND stores of item i - 1, nothing else
        else wait_vmcnt<0>();
        barrier_nodrain();        // tile i is in LDS for every wave (first item: the tables too); item i - 1 is computed and copied out of its buffer
        if (i + 1 < nmy) issue(i + 1);
        char* tile = tiles + (size_t)(i & 1) * P::tile_bytes;

        if (wa) {
            const bf16_t* xl = reinterpret_cast<const bf16_t*>(tile + xa_off);
            const bf16_t* xl2 = xl + 12 * 32 * P::UC;                // k-steps 12 and up: the ds offset field ends at 64 KiB
            f32x4 acc[3];
#pragma unroll
            for (int ni = 0; ni < 3; ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
            bf16x8 xf[2][3];
            static_for<3>([&](auto nic) {
                constexpr int ni = decltype(nic)::value;
                xf[0][ni] = tdfw_read_frag<ni * 32>(xl);
            });
            static_for<P::KS1>([&](auto ksc) {
                constexpr int ks = decltype(ksc)::value, b = ks & 1;
                if constexpr (ks + 1 < P::KS1) {
                    constexpr int k1 = ks + 1;
                    const bf16_t* bp = k1 >= 12 ? xl2 : xl;
                    static_for<3>([&](auto nic) {
                        constexpr int ni = decltype(nic)::value;
                        xf[1 - b][ni] = tdfw_read_frag<(k1 % 12) * 32 * P::UC * 2 + ni * 32>(bp);
                    });
                    lds_read_tr16_wait_n<6>();                       // step ks has landed, step ks + 1 is in flight
                } else {
                    lds_read_tr16_wait_n<0>();
                }
#pragma unroll
                for (int ni = 0; ni < 3; ++ni) mma_step(acc[ni], xf[b][ni], w1[ks]);
            });
            // relu(bn1(acc + b1)), rounded as tdf_bf16_kernel<false> stores it
            const float* bp = bnl + unit_cb(i, ua) + 4 * lq;
            f32x4 sc[3], sh[3];
            static_for<3>([&](auto nic) {
                constexpr int ni = decltype(nic)::value;
                lds_read_async_f32x4<ni * 64>(sc[ni], bp);
                lds_read_async_f32x4<P::CMAX * 4 + ni * 64>(sh[ni], bp);
            });
            lds_wait_n<0>();
            static_for<3>([&](auto nic) {
                constexpr int ni = decltype(nic)::value;
                bf16x4 q;
#pragma unroll
                for (int r = 0; r < 4; ++r) q[r] = (bf16_t)fmaxf(fmaf(acc[ni][r] + b1, sc[ni][r], sh[ni][r]), 0.f);
                lds_write_async_b64(hw + ni * 16, q);
            });
        }
        barrier_nodrain();                                           // the hidden tile is complete

        {
            const float* bp = bnl + 2 * P::CMAX + unit_cb(i, ub) + 4 * lq;
            bf16_t* el = reinterpret_cast<bf16_t*>(tile + eb_off);
            static_for<P::MT2>([&](auto mic) {
                constexpr int mi = decltype(mic)::value;
                bf16x8 hf[P::KS2][3];
                static_for<P::KS2 * 3>([&](auto jc) {
                    constexpr int ks = decltype(jc)::value / 3, ni = decltype(jc)::value % 3;
                    hf[ks][ni] = tdfw_read_frag<ks * 32 * P::UC * 2 + ni * 32>(hl);
                });
                f32x4 acc[3];
#pragma unroll
                for (int ni = 0; ni < 3; ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
                lds_read_tr16_wait_n<0>();
#pragma unroll
                for (int ks = 0; ks < P::KS2; ++ks)
#pragma unroll
                    for (int ni = 0; ni < 3; ++ni) mma_step(acc[ni], hf[ks][ni], w2[mi][ks]);
                // fmaxf(fmaf(acc + b2, scale, shift), 0) + x in fp32, one rounding, as tdf_bf16_kernel<true>; over the residual values
                bf16x4 xr[3];
                f32x4 sc[3], sh[3];
                static_for<3>([&](auto nic) {
                    constexpr int ni = decltype(nic)::value;
                    lds_read_async_b64<(mi * 16 * P::UC + ni * 16) * 2>(xr[ni], el);
                    lds_read_async_f32x4<ni * 64>(sc[ni], bp);
                    lds_read_async_f32x4<P::CMAX * 4 + ni * 64>(sh[ni], bp);
                });
                lds_wait_n<0>();
                static_for<3>([&](auto nic) {
                    constexpr int ni = decltype(nic)::value;
                    bf16x4 q;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        q[r] = (bf16_t)(fmaxf(fmaf(acc[ni][r] + b2[mi], sc[ni][r], sh[ni][r]), 0.f) + (float)xr[ni][r]);
                    lds_write_async_b64(el + mi * 16 * P::UC + ni * 16, q);
                });
            });
            // the wave's rows, complete: whole 96-byte rows in 16-byte pieces (the LDS operations of a wave execute in order)
            __builtin_amdgcn_wave_barrier();
            const bf16_t* cl = reinterpret_cast<const bf16_t*>(tile + co_off);
            bf16x8 q[P::ND];
            static_for<P::ND>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                lds_read_async_b128<t * 1024>(q[t], cl);
            });
            lds_wait_n<0>();
            ALSEP_GLOBAL char* yb = const_cast<ALSEP_GLOBAL char*>(
                opaque_uniform_gptr(reinterpret_cast<const char*>(Y + unit_base(i, ub) + (int64_t)f0 * C)));
#pragma unroll
            for (int t = 0; t < P::ND; ++t)
                stream_store(reinterpret_cast<ALSEP_GLOBAL bf16x8*>(yb + (size_t)(t / 3) * 32 * C * sizeof(bf16_t) + xoff[t % 3]), q[t]);
        }
    }
}

#ifndef ALSEP_F16_TU
#include "tdfnet_f32s.h"    // float32 storage with split-half contractions (the float32 network lives in the main translation unit)
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
    DevBuf wfused;           // fragment-order image for tdf_bf16_fused_kernel (both linears of a block with F = 768 / 384, H = F / 8)
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

// fragment-order image for tdf_bf16_fused_kernel: [M/16][ceil(K/32)][lane 64][8]; lane (l15, lq) of (m-tile mt, k-step ks) holds
// W[16 mt + l15][32 ks + {4lq..4lq+3, 16+4lq..16+4lq+3}], zero beyond K -- the k order of the two images above
int make_tdf_fused_weights(alsep_net* net, const std::vector<float>& wmk, int M, int K, GemmLayer* L) {
    const int MT = M / 16, KS = (K + 31) / 32;
    std::vector<bf16_t> pk((size_t)MT * KS * 512, host_cast<bf16_t>(0.f));
    for (int mt = 0; mt < MT; ++mt)
        for (int ks = 0; ks < KS; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int lq = l >> 4, m = mt * 16 + (l & 15);
                    const int k = ks * 32 + (e < 4 ? 4 * lq + e : 16 + 4 * lq + (e - 4));
                    if (k < K) pk[(((size_t)mt * KS + ks) * 64 + l) * 8 + e] = host_cast<bf16_t>(wmk[(size_t)m * K + k]);
                }
    return upload(net, pk.data(), pk.size() * sizeof(bf16_t), &L->wfused);
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
        if (L->dma_path && n_lin == 2 && cfg.bn == 8 && (f == 768 || f == 384) && (rc = make_tdf_fused_weights(net, *w, fo, fi, L)))
            return rc;
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

// ---- switches ------------------------------------------------------------------------------
// Which kernel runs a layer of a bf16 / f16 network on the DMA and stream paths.  Every switch is an environment variable (atoi of it, or
// the default where it is not set), read once per process by switches(); each one only chooses between kernels that compute the same
// layer (all but mq bit-identically).  The routing itself is route_conv_dma, route_pix_stream, route_tdf_dma and route_tdf_fused below.
//
// 3x3 convs with c % 48 == 0
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
//
// ds / us
//   ALSEP_PIX_STREAM  1 (default): a ds / us layer that has a fragment-order image (bf16 / f16, levels 0 <-> 1 <-> 2 <-> 3) runs on the
//                     streaming kernels where F' % 64 == 0; 0: pix_gemm_kernel.
//   ALSEP_PIX_PIPE    1 (default) = the ds / us of the middle levels run on ds_pipe_kernel / us_pipe_kernel for the instances in
//                     kPixPipeRouted (each is routed there only where it measured faster than its stream kernel on the same box:
//                     profiles/pix_pipe_kernel_stats.txt); 0 = never (the stream kernels, as before); 2 = every instance (measurements, tests).
//                     ALSEP_PIX_PIPE_GRID=n caps their grid (tests: several tiles per workgroup at small shapes).
//
// TDF linears
//   ALSEP_TDF_WIDE    0 = 128-row kernel only; 1 (default) = wide kernel where M % 192 == 0, 384 rows per workgroup for a
//                     first linear whose whole M is 384; 4 / 8 = force 192 / 384 rows wherever M allows (experiments, tests)
//   ALSEP_TDF_YFAST   1 (default): the wide kernel's M / BM row blocks of one column tile run back to back (1-D grid, needs gx % 8 == 0);
//                     0: the column tile is the fastest grid dimension.
//   ALSEP_TDF_RPF     2 (default): the wide kernel requests residual rows two units ahead of the stores; 0: residual rows loaded where they
//                     are used (timing comparison only; such a launch neither folds the final conv nor goes to the persistent kernel).
//   ALSEP_TDF_FINAL   1 (default) = fold the final 1x1 conv into the last residual TDF launch where the wide 192-row kernel
//                     serves it and C == 48; 0 = always the separate final_conv_kernel
//   ALSEP_TDF_PERSIST 1 (default) = the residual linear of levels 0 and 1 runs on tdf_bf16_persist_kernel for the launch kinds
//                     in kTdfPersistRouted (each kind is routed there only where it measured faster than the wide kernel on the same box:
//                     profiles/tdf_persist_kernel_stats.txt); 0 = never (the wide kernel, as before); 2 = every kind the kernel serves
//                     (measurements, tests).  ALSEP_TDF_PERSIST_GRID=n caps its grid (tests: several items per workgroup at small shapes).
//   ALSEP_TDF_US_FOLD 1 = the 96 -> 48 upsampling between levels 1 and 0 is folded into the residual TDF launch of the block
//                     under it (tdf_bf16_persist_kernel<3, false, true>: the block's output never reaches memory) where that launch goes to
//                     the persistent kernel at C = 96, K = 192 and the upsampling would run on us_stream_kernel<96, 48>; 0 = two
//                     launches, as before.  Same bits either way.  ALSEP_TDF_PERSIST_GRID caps this launch's grid too.
//   ALSEP_TDF_FUSED   1 (default) = the two TDF linears of a block run as one launch of tdf_bf16_fused_kernel at the levels in
//                     kTdfFusedRouted (a level is routed there only where, in kernel traces of one session, the fused launch's mean and max lay below
//                     the sum of the two old launches' minima: profiles/tdf_fused_kernel_stats.txt), and only at no fewer items than the level was
//                     measured at (kTdfFusedFloor: the bench's 52 windows -- 9984 items at F = 768, 3328 at F = 384; below that the workgroups run
//                     fewer rounds and nothing was measured); 0 = never (two launches of tdf_bf16_kernel, as before); 2 = every shape an instance
//                     serves (bf16 / f16 on the DMA path, bn = 8, F = 768 or 384, C a multiple of 48 up to 192), without the floor (tests).
//                     ALSEP_TDF_FUSED_GRID=n caps its grid (tests: several items per workgroup at small shapes).
struct Switches {
    int conv_m0, conv_regw, conv_big, conv_mq, conv_big3, conv_allco, conv_allco_tw, conv_allco_grid, conv_nyfast;
    int pix_stream, pix_pipe, pix_pipe_grid;
    int tdf_wide, tdf_yfast, tdf_rpf, tdf_final, tdf_persist, tdf_persist_grid, tdf_us_fold, tdf_fused, tdf_fused_grid;
};
// Levels that measured faster on conv3x3_bf16_allco_kernel than on their kernel, same box, bench shape (profiles/conv_allco_kernel_stats.txt,
// conv_allco_ab.txt; c = 192: conv_allco_groups_kernel_stats.txt, conv_allco_groups_ab.txt); only these are routed there by default.
constexpr int kConvAllco144 = 1, kConvAllco192 = 2;
constexpr int kConvAllcoRouted = kConvAllco144 | kConvAllco192;
// the tile width of the instances in output groups (c = 192 / 288): 48 or 64
constexpr int kConvAllcoTw = 64;
enum { kPixPipeDs96 = 1, kPixPipeDs144 = 2, kPixPipeUs192 = 4, kPixPipeUs144 = 8 };
constexpr int kPixPipeRouted = kPixPipeDs96 | kPixPipeDs144 | kPixPipeUs192 | kPixPipeUs144;
enum { kTdfPersistK384 = 1, kTdfPersistK192 = 2, kTdfPersistFinal = 4 };
constexpr int kTdfPersistRouted = kTdfPersistK384 | kTdfPersistK192 | kTdfPersistFinal;
enum { kTdfFusedF768 = 1, kTdfFusedF384 = 2 };
constexpr int kTdfFusedRouted = kTdfFusedF768 | kTdfFusedF384;
constexpr int64_t kTdfFusedFloor[2] = {9984, 3328};
// ALSEP_TDF_US_FOLD where it is not set (profiles/tdf_us_fold_kernel_stats.txt, tdf_us_fold_ab.txt)
constexpr int kTdfUsFold = 1;

const Switches& switches() {
    static const Switches s = [] {
        Switches v;
        v.conv_m0 = env_int("ALSEP_CONV_M0", 1);
        v.conv_regw = env_int("ALSEP_CONV_REGW", 1);
        v.conv_big = env_int("ALSEP_CONV_BIG", 1);
        v.conv_mq = env_int("ALSEP_CONV_MQ", 1);
        v.conv_big3 = env_int("ALSEP_CONV_BIG3", 1);
        v.conv_allco = env_int("ALSEP_CONV_ALLCO", 1);
        v.conv_allco_tw = env_int("ALSEP_CONV_ALLCO_TW", kConvAllcoTw) == 48 ? 48 : 64;
        v.conv_allco_grid = env_int("ALSEP_CONV_ALLCO_GRID", 0);
        v.conv_nyfast = env_int("ALSEP_CONV_NYFAST", 1);
        v.pix_stream = env_int("ALSEP_PIX_STREAM", 1);
        v.pix_pipe = env_int("ALSEP_PIX_PIPE", 1);
        v.pix_pipe_grid = env_int("ALSEP_PIX_PIPE_GRID", 0);
        v.tdf_wide = env_int("ALSEP_TDF_WIDE", 1);
        v.tdf_yfast = env_int("ALSEP_TDF_YFAST", 1);
        v.tdf_rpf = env_int("ALSEP_TDF_RPF", 2);
        v.tdf_final = env_int("ALSEP_TDF_FINAL", 1);
        v.tdf_persist = env_int("ALSEP_TDF_PERSIST", 1);
        v.tdf_persist_grid = env_int("ALSEP_TDF_PERSIST_GRID", 0);
        v.tdf_us_fold = env_int("ALSEP_TDF_US_FOLD", kTdfUsFold);
        v.tdf_fused = env_int("ALSEP_TDF_FUSED", 1);
        v.tdf_fused_grid = env_int("ALSEP_TDF_FUSED_GRID", 0);
        return v;
    }();
    return s;
}
// a switch over a mask of measured kinds (_PIX_PIPE, _TDF_PERSIST): 2 and up = every kind, 1 = the kinds in `routed`, else none
bool mask_routed(int mode, int routed, int kind) { return mode >= 2 || (mode == 1 && (routed & kind)); }

// ---- routes --------------------------------------------------------------------------------
// What a route_*() function answers for one layer launch: the kernel instance (K: the enum of the layer kind), the profiling class, and
// the names the launch is counted under -- `check`, which ALSEP_LAUNCH_CHECK reports and counts, and `also`.  The pinned launch names
// (bench.py and the tests read them) count LAYER launches, whichever instance serves them: `also` holds the instance's own name where it
// has one and the pinned names of the kernel it replaces -- an all-channels conv counts under big<3>'s or the plain kernel's names, a
// persistent TDF launch under the wide kernel's, a fused TDF launch twice under tdf_bf16_kernel (it is two layers), a residual TDF launch
// with the upsampling folded in also under the us layer's names (it is that layer too).  finish_launch() is the only place that notes them.  A route function launches nothing and touches no ctx.
template <typename K>
struct Route {
    K kernel;
    int prof_class;
    const char* check;
    const char* also[5];
};
template <typename K>
int finish_launch(alsep_ctx* ctx, const Route<K>& r) {
    for (const char* name : r.also)
        if (name) note_launch(ctx, name);
    ALSEP_LAUNCH_CHECK(ctx, r.check);
    return ALSEP_OK;
}
// The float32 launchers (exact and split) have no route: each counts one pinned name, whichever instance and grid order ran.  Beside it
// they note alias names -- the conv instance ("conv3x3_f32s_kernel<24,48,32>", "conv3x3_kernel<f32,16,48,64>"), "<ny_fastest>" /
// "<nrb_fast>" for the 1-D grid orders, "<res>" / "<nores>", "<ds>" / "<us>" -- so that a test asserts the branch it means to reach.
void note_instance(alsep_ctx* ctx, const char* fmt, int a, int b, int c) {
    char name[64];
    snprintf(name, sizeof(name), fmt, a, b, c);
    note_launch(ctx, name);
}

// ---- launches ------------------------------------------------------------------------------
// One kernel launch on ctx->stream; kLdsRaise first raises the kernel's dynamic-LDS limit to `lds` (the launches above 64 KiB).
enum LdsLimit { kLdsAsIs, kLdsRaise };
template <typename... P, typename... A>
hipError_t launch(alsep_ctx* ctx, void (*kern)(P...), dim3 grid, dim3 block, size_t lds, LdsLimit limit, A... args) {
    static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
    if (limit == kLdsRaise) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, block, lds, ctx->stream, static_cast<P>(args)...);
    return hipSuccess;
}
// f(std::true_type) or f(std::false_type): a template instance chosen by a run-time bool, with one argument list
template <typename F>
auto dispatch_bool(bool v, F f) {
    return v ? f(std::true_type()) : f(std::false_type());
}
// the grid of a persistent kernel that fills a CU's LDS: one workgroup per CU, at most `cap` (a *_GRID switch; 0 = none), one per item
unsigned per_cu_grid(alsep_ctx* ctx, int cap, int64_t nitems) {
    int64_t grid = device_cu_count(ctx);
    if (cap > 0 && cap < grid) grid = cap;
    return (unsigned)std::min<int64_t>(grid, nitems);
}

// work of a 3x3 convolution for the profile: 2 x 9 flops per input channel, output channel and pixel; every activation read and written once
void conv_work(ProfScope& prof, const ConvLayer& L, size_t elem_bytes, int64_t B, int Th, int Fw) {
    prof.work(18.0 * (double)L.cin * L.cout * B * Th * Fw, (double)elem_bytes * B * Th * Fw * (L.cin + L.cout));
}

template <typename T, int KC, int BN, int TW>
int launch_conv(alsep_ctx* ctx, const ConvLayer& L, const T* X, T* Y, int64_t B, int Th, int Fw) {
    typedef ConvCfg<T, KC, BN, TW> Cf;
    const int tiles_t = (int)ceil_div64(Th, Cf::TH), tiles_f = (int)ceil_div64(Fw, TW);
    const int64_t ntiles = B * tiles_t * tiles_f;
    if (ntiles > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "conv3x3: too many tiles");
    ProfScope prof(ctx, TW == 64 ? ALSEP_PROF_CONV3X3 : ALSEP_PROF_CONV3X3_SMALL);
    conv_work(prof, L, sizeof(*X), B, Th, Fw);
    ALSEP_HIP(ctx, launch(ctx, conv3x3_kernel<T, KC, BN, TW>, dim3((unsigned)ntiles, L.cout / BN), dim3(kThreads), Cf::lds_bytes, kLdsRaise, X, Y,
                          (const T*)L.w.p, (const float*)L.scale.p, (const float*)L.shift.p, Th, Fw, L.cin, L.cout, tiles_t, tiles_f, (int)ntiles));
    if constexpr (std::is_same<T, float>::value) note_instance(ctx, "conv3x3_kernel<f32,%d,%d,%d>", KC, BN, TW);
    ALSEP_LAUNCH_CHECK(ctx, "conv3x3_kernel");
    return ALSEP_OK;
}

template <typename T, int KC, int BN>
int run_conv_tw(alsep_ctx* ctx, const ConvLayer& L, const T* X, T* Y, int64_t B, int Th, int Fw) {
    if (Fw >= 64 && Fw % 64 == 0) return launch_conv<T, KC, BN, 64>(ctx, L, X, Y, B, Th, Fw);
    if (Fw >= 32) return launch_conv<T, KC, BN, 32>(ctx, L, X, Y, B, Th, Fw);
    return launch_conv<T, KC, BN, 16>(ctx, L, X, Y, B, Th, Fw);
}

// The instances that serve a bf16 / f16 3x3 conv with c % 48 == 0 (L.dma_path), in the order route_conv_dma tries them.
enum class ConvKernel { M0, Regw48x64, Regw48x32, Regw96, Allco144, Allco192x48, Allco192x64, Allco288x48, Allco288x64, Mq, Big3, Plain64, Plain32, Plain16 };
typedef Route<ConvKernel> ConvRoute;

ConvRoute route_conv_dma(const Switches& s, const ConvLayer& L, int64_t B, int Th, int Fw) {
    typedef ConvKernel K;
    const int c = L.cout;
    const bool plain64 = Fw >= 64 && Fw % 64 == 0;           // the plain kernel's choice between <64> and <small>
    const int plain_class = plain64 ? ALSEP_PROF_CONV3X3 : ALSEP_PROF_CONV3X3_SMALL;
    const char* const plain_name = plain64 ? "conv3x3_bf16_kernel<64>" : "conv3x3_bf16_kernel<small>";
    if (s.conv_m0 && L.cin == 48 && c == 48 && Th % 8 == 0 && Fw % 48 == 0 && (s.conv_m0 >= 2 || B * (Th / 8) * (Fw / 48) >= 256))
        return {K::M0, ALSEP_PROF_CONV3X3_REGW, "conv3x3_bf16_m0_kernel", {}};
    if (s.conv_regw && Th % 4 == 0 && Fw % 64 == 0 && L.cin == c) {
        const K k = c == 48 ? (s.conv_regw == 3 ? K::Regw48x64 : K::Regw48x32) : K::Regw96;
        if (c == 48 || (c == 96 && s.conv_regw >= 2)) return {k, ALSEP_PROF_CONV3X3_REGW, "conv3x3_bf16_regw_kernel", {}};
    }
    if (s.conv_big && L.cin == c && Th % 8 == 0) {           // the 8-wave kernels
        // the shapes mq and big<3> take (their tile floor), and the only ones the all-channels instances were measured at
        const bool big_shape = Fw % 64 == 0 && (s.conv_big >= 2 || B * (Th / 8) * (Fw / 64) >= 96);
        if (c == 144 && s.conv_big3 && s.conv_allco && Fw % 48 == 0 && (s.conv_allco >= 2 || ((kConvAllcoRouted & kConvAllco144) && big_shape)))
            return {K::Allco144, ALSEP_PROF_CONV3X3_BIG3, "conv3x3_bf16_allco_kernel", {"conv3x3_bf16_big_kernel", "conv3x3_bf16_big_kernel<3>"}};
        // in output groups: by default only c = 192; replaces the plain kernel and keeps its profiling class, so that a level's class
        // does not depend on the instance that serves it
        const int tw = s.conv_allco_tw;
        if ((c == 192 || c == 288) && s.conv_allco && Fw % tw == 0 &&
            (s.conv_allco >= 2 || ((kConvAllcoRouted & kConvAllco192) && c == 192 && big_shape))) {
            const K k = c == 192 ? (tw == 48 ? K::Allco192x48 : K::Allco192x64) : (tw == 48 ? K::Allco288x48 : K::Allco288x64);
            return {k, plain_class, "conv3x3_bf16_allco_kernel",
                    {tw == 48 ? "conv3x3_bf16_allco_kernel<6,48>" : "conv3x3_bf16_allco_kernel<6,64>", "conv3x3_bf16_kernel", plain_name}};
        }
        if (big_shape && c == 96 && s.conv_mq) return {K::Mq, ALSEP_PROF_CONV3X3_BIG, "conv3x3_bf16_mq_kernel", {}};
        if (big_shape && c == 144 && s.conv_big3) return {K::Big3, ALSEP_PROF_CONV3X3_BIG3, "conv3x3_bf16_big_kernel", {"conv3x3_bf16_big_kernel<3>"}};
    }
    return {plain64 ? K::Plain64 : Fw >= 32 ? K::Plain32 : K::Plain16, plain_class, "conv3x3_bf16_kernel", {plain_name}};
}

template <int TW>
int launch_conv_dma(alsep_ctx* ctx, const ConvRoute& r, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B,
                    int Th, int Fw) {
    typedef ConvB16<TW> Cf;
    const int tiles_t = (int)ceil_div64(Th, Cf::TH), tiles_f = (int)ceil_div64(Fw, TW);
    const int64_t ntiles = B * tiles_t * tiles_f;
    if (ntiles > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "conv3x3: too many tiles");
    ProfScope prof(ctx, r.prof_class);
    conv_work(prof, L, sizeof(*X), B, Th, Fw);
    const int nyc = L.cout / Cf::BN;
    const int ny_fastest = switches().conv_nyfast && ntiles % 8 == 0 && nyc > 1 && ntiles * nyc <= 0x7fffffff;
    ALSEP_HIP(ctx, launch(ctx, conv3x3_bf16_kernel<TW>, ny_fastest ? dim3((unsigned)(ntiles * nyc)) : dim3((unsigned)ntiles, nyc), dim3(kThreads),
                          Cf::lds_bytes, kLdsRaise, X, Y, (const bf16_t*)L.w.p, (const float*)L.scale.p, (const float*)L.shift.p, zero_page,
                          Th, Fw, L.cin, L.cout, tiles_t, tiles_f, (int)ntiles, /*ablate*/ 0, /*stagger*/ 0, ny_fastest));
    return finish_launch(ctx, r);
}

template <int NQ, int RING_ = 3, int OCC = 1, int TW_ = 64>
int launch_conv_regw(alsep_ctx* ctx, const ConvRoute& r, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B,
                     int Th, int Fw) {
    typedef ConvRW<NQ, RING_, TW_> Cf;
    const int tiles_t = Th / Cf::TH, tiles_f = Fw / Cf::TW;
    const int64_t ntiles = B * tiles_t * tiles_f;
    if (ntiles > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "conv3x3: too many tiles");
    const int ny = L.cout / Cf::BN;
    int gx = OCC * 256 / ny;                                // OCC workgroups per CU over the whole grid
    if (gx > ntiles) gx = (int)ntiles;
    ProfScope prof(ctx, r.prof_class);
    conv_work(prof, L, sizeof(*X), B, Th, Fw);
    ALSEP_HIP(ctx, launch(ctx, conv3x3_bf16_regw_kernel<NQ, RING_, OCC, TW_>, dim3((unsigned)gx, ny), dim3(kThreads), Cf::lds_bytes, kLdsRaise, X, Y,
                          (const bf16_t*)L.w.p, (const float*)L.scale.p, (const float*)L.shift.p, zero_page, Th, Fw, L.cin, L.cout, tiles_t,
                          tiles_f, (int)ntiles));
    return finish_launch(ctx, r);
}

// The 8-wave persistent convs (conv3x3_bf16_m0_kernel, _mq_kernel, _big_kernel<3>, _allco_kernel) share their argument list and their
// launch: one workgroup per CU, each walking the tiles blockIdx.x, blockIdx.x + gridDim.x, ...  Cf is the kernel's tile configuration, wimg
// its weight image; the caller has checked that the layer fits the kernel.
template <typename Cf, typename Kern>
int launch_conv_persist(alsep_ctx* ctx, Kern kern, const ConvRoute& r, const ConvLayer& L, const DevBuf& wimg, const bf16_t* X, bf16_t* Y,
                        const bf16_t* zero_page, int64_t B, int Th, int Fw, int grid_cap = 0) {
    const int tiles_t = Th / Cf::TH, tiles_f = Fw / Cf::TW;
    const int64_t ntiles = B * tiles_t * tiles_f;
    if (ntiles > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "conv3x3: too many tiles");
    int gx = ntiles < 256 ? (int)ntiles : 256;
    if (grid_cap > 0 && gx > grid_cap) gx = grid_cap;
    ProfScope prof(ctx, r.prof_class);
    conv_work(prof, L, sizeof(*X), B, Th, Fw);
    ALSEP_HIP(ctx, launch(ctx, kern, dim3((unsigned)gx), dim3(kBigThreads), Cf::lds_bytes, kLdsRaise, X, Y, (const bf16_t*)wimg.p,
                          (const float*)L.scale.p, (const float*)L.shift.p, zero_page, Th, Fw, L.cin, L.cout, tiles_t, tiles_f, (int)ntiles));
    return finish_launch(ctx, r);
}

int launch_conv_big3(alsep_ctx* ctx, const ConvRoute& r, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B, int Th, int Fw) {
    if (!L.w_big.p) return alsep_fail(ctx, ALSEP_ERR_STATE, "conv3x3: no big-tile weight image for this layer");
    return launch_conv_persist<ConvBig<3>>(ctx, conv3x3_bf16_big_kernel<3>, r, L, L.w_big, X, Y, zero_page, B, Th, Fw);
}

int launch_conv_mq(alsep_ctx* ctx, const ConvRoute& r, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B, int Th, int Fw) {
    if (!L.w_mq.p || L.cout != ConvMq::ROWS || L.cin % ConvMq::KC) return alsep_fail(ctx, ALSEP_ERR_STATE, "conv3x3: no mq weight image for this layer");
    return launch_conv_persist<ConvMq>(ctx, conv3x3_bf16_mq_kernel, r, L, L.w_mq, X, Y, zero_page, B, Th, Fw);
}

int launch_conv_m0(alsep_ctx* ctx, const ConvRoute& r, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B, int Th, int Fw) {
    if (!L.w_big.p || L.cout != ConvM0::ROWS || L.cin != ConvM0::KC) return alsep_fail(ctx, ALSEP_ERR_STATE, "conv3x3: no m0 weight image for this layer");
    return launch_conv_persist<ConvM0>(ctx, conv3x3_bf16_m0_kernel, r, L, L.w_big, X, Y, zero_page, B, Th, Fw);
}

// <9, 48, 1> serves c = 144; the instances in output groups, <6, 48 | 64, 2 | 3>, c = 192 / 288
template <int NM, int TW, int NGRP>
int launch_conv_allco(alsep_ctx* ctx, const ConvRoute& r, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zero_page, int64_t B, int Th, int Fw) {
    typedef ConvAllco<NM, TW, NGRP> Cf;
    static_assert((NM == 9 && TW == 48 && NGRP == 1) || (NM == 6 && NGRP >= 2), "an instance that has a weight image and a route");
    if (!L.w_ac.p || L.cout != Cf::COUT || L.cin != L.cout || Th % Cf::TH || Fw % TW)
        return alsep_fail(ctx, ALSEP_ERR_STATE, "conv3x3: no all-channels weight image for this layer, or not its shape");
    return launch_conv_persist<Cf>(ctx, conv3x3_bf16_allco_kernel<NM, TW, NGRP>, r, L, L.w_ac, X, Y, zero_page, B, Th, Fw,
                                   switches().conv_allco_grid);
}

int run_conv_dma(alsep_ctx* ctx, const ConvLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* zp, int64_t B, int Th, int Fw) {
    const ConvRoute r = route_conv_dma(switches(), L, B, Th, Fw);
    switch (r.kernel) {
    case ConvKernel::M0: return launch_conv_m0(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Regw48x64: return launch_conv_regw<1>(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Regw48x32: return launch_conv_regw<1, 3, 2, 32>(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Regw96: return launch_conv_regw<2>(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Allco144: return launch_conv_allco<9, 48, 1>(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Allco192x48: return launch_conv_allco<6, 48, 2>(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Allco192x64: return launch_conv_allco<6, 64, 2>(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Allco288x48: return launch_conv_allco<6, 48, 3>(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Allco288x64: return launch_conv_allco<6, 64, 3>(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Mq: return launch_conv_mq(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Big3: return launch_conv_big3(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Plain64: return launch_conv_dma<64>(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Plain32: return launch_conv_dma<32>(ctx, r, L, X, Y, zp, B, Th, Fw);
    case ConvKernel::Plain16: return launch_conv_dma<16>(ctx, r, L, X, Y, zp, B, Th, Fw);
    }
    return alsep_fail(ctx, ALSEP_ERR_STATE, "conv3x3: no such route");
}

#ifndef ALSEP_F16_TU
template <int KC, int BN, int TW>
int launch_conv_split(alsep_ctx* ctx, const ConvLayer& L, const float* X, float* Y, int64_t B, int Th, int Fw) {
    typedef ConvSCfg<KC, BN, TW> Cf;
    const int tiles_t = (int)ceil_div64(Th, Cf::TH), tiles_f = (int)ceil_div64(Fw, TW);
    const int64_t ntiles = B * tiles_t * tiles_f;
    const int nyc = L.cout / BN;
    if (ntiles * nyc > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "conv3x3: too many tiles");
    ProfScope prof(ctx, TW >= 32 ? ALSEP_PROF_CONV3X3 : ALSEP_PROF_CONV3X3_SMALL);
    conv_work(prof, L, 4, B, Th, Fw);
    const int nyf = (ntiles % 8 == 0 && nyc > 1) ? 1 : 0;
    const dim3 grid = nyf ? dim3((unsigned)(ntiles * nyc)) : dim3((unsigned)ntiles, nyc);
    ALSEP_HIP(ctx, launch(ctx, conv3x3_f32s_kernel<KC, BN, TW>, grid, dim3(kThreads), Cf::lds_bytes, kLdsRaise, X, Y, (const hs_t*)L.w.p,
                          (const float*)L.scale.p, (const float*)L.shift.p, Th, Fw, L.cin, L.cout, tiles_t, tiles_f, (int)ntiles, nyf, L.range_flag));
    note_instance(ctx, "conv3x3_f32s_kernel<%d,%d,%d>", KC, BN, TW);
    if (nyf) note_launch(ctx, "conv3x3_f32s_kernel<ny_fastest>");
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
#endif

// make_conv sets `split` only in a float32 network and `dma_path` only in a bf16 / f16 one (and make_block / build_net the TDF and
// ds / us images -- dma_path, wwide, wfused, wfrag -- likewise), so each storage type compiles only the paths it can take.
template <typename T>
int run_conv(alsep_ctx* ctx, const ConvLayer& L, const T* X, T* Y, int64_t B, int Th, int Fw, const void* zero_page) {
    if constexpr (std::is_same<T, float>::value) {
#ifndef ALSEP_F16_TU
        if (L.split) return run_conv_split(ctx, L, X, Y, B, Th, Fw);
#endif
    } else {
        if (L.dma_path) return run_conv_dma(ctx, L, X, Y, (const T*)zero_page, B, Th, Fw);
    }
    if (conv_uses_main<T>(L.cin, L.cout)) return run_conv_tw<T, ConvSel<T>::KC, ConvSel<T>::BN>(ctx, L, X, Y, B, Th, Fw);
    return run_conv_tw<T, ConvSel16<T>::KC, ConvSel16<T>::BN>(ctx, L, X, Y, B, Th, Fw);
}

// The instances that serve a ds / us layer on the stream path (L.wfrag): the pipelined kernels of the middle levels, the stream kernels
enum class PixKernel { DsPipe96, DsPipe144, UsPipe192, UsPipe144, Ds48, DsSplit96, DsSplit144, Us96, Us144, Us192 };
typedef Route<PixKernel> PixRoute;

PixRoute route_pix_stream(const Switches& s, int mode, const GemmLayer& L) {
    typedef PixKernel K;
    const int cls = ALSEP_PROF_PIX;
    const char* const chk = "pix stream kernel";
    const auto pipe = [&](int kind) { return mask_routed(s.pix_pipe, kPixPipeRouted, kind); };
    if (mode == PIX_DS) {
        const char* const any = "ds_stream_kernel";
        if (L.M == DsSplitCfg<96>::M && pipe(kPixPipeDs96)) return {K::DsPipe96, cls, chk, {any, "ds_split_stream_kernel<96>", "ds_pipe_kernel<96>"}};
        if (L.M == DsSplitCfg<144>::M && pipe(kPixPipeDs144)) return {K::DsPipe144, cls, chk, {any, "ds_split_stream_kernel<144>", "ds_pipe_kernel<144>"}};
        if (L.M == Ds48::M) return {K::Ds48, cls, chk, {any, "ds48_stream_kernel"}};                                      // 48 -> 96
        if (L.M == DsSplitCfg<96>::M) return {K::DsSplit96, cls, chk, {any, "ds_split_stream_kernel<96>"}};                // 96 -> 144
        return {K::DsSplit144, cls, chk, {any, "ds_split_stream_kernel<144>"}};                                            // 144 -> 192
    }
    const char* const any = "us_stream_kernel";
    if (L.K == 192 && pipe(kPixPipeUs192)) return {K::UsPipe192, cls, chk, {any, "us_stream_kernel<192,144>", "us_pipe_kernel<192,144>"}};
    if (L.K == 144 && pipe(kPixPipeUs144)) return {K::UsPipe144, cls, chk, {any, "us_stream_kernel<144,96>", "us_pipe_kernel<144,96>"}};
    if (L.K == 96) return {K::Us96, cls, chk, {any, "us_stream_kernel<96,48>"}};                  // 96 -> 48
    if (L.K == 144) return {K::Us144, cls, chk, {any, "us_stream_kernel<144,96>"}};               // 144 -> 96: 32-pixel tiles, two workgroups per CU
    return {K::Us192, cls, chk, {any, "us_stream_kernel<192,144>"}};                              // 192 -> 144: 32-pixel tiles (accumulators beside 54 fragments)
}

int run_pix_stream(alsep_ctx* ctx, int mode, const GemmLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* skip, int64_t ncols,
                   int Tp, int Fp) {
    typedef PixKernel K;
    const Switches& s = switches();
    const PixRoute r = route_pix_stream(s, mode, L);
    ProfScope prof(ctx, r.prof_class);
    const int64_t ntile = ncols / 64;
    const bf16_t* const w = (const bf16_t*)L.wfrag.p;
    const float* const sc = (const float*)L.scale.p;
    const float* const sh = (const float*)L.shift.p;
    // every ds kernel takes the first argument list, every us kernel the second
    const auto ds = [&](auto kern, int64_t gx, size_t lds, LdsLimit limit) {
        return launch(ctx, kern, dim3((unsigned)gx), dim3(kThreads), lds, limit, X, Y, w, sc, sh, ncols, Tp, Fp);
    };
    const auto us = [&](auto kern, int64_t gx, size_t lds) {
        return launch(ctx, kern, dim3((unsigned)gx), dim3(kThreads), lds, kLdsRaise, X, Y, w, sc, sh, skip, ncols, Tp, Fp);
    };
    const auto pipe_grid = [&](int px) { return per_cu_grid(ctx, s.pix_pipe_grid, ncols / px); };   // more than 128 KiB of LDS
    hipError_t e = hipSuccess;
    switch (r.kernel) {
    case K::DsPipe96: e = ds(ds_pipe_kernel<96, 64, 1>, pipe_grid(DsPipeCfg<96, 64, 1>::PX), DsPipeCfg<96, 64, 1>::lds_bytes, kLdsRaise); break;
    case K::DsPipe144: e = ds(ds_pipe_kernel<144, 32, 2>, pipe_grid(DsPipeCfg<144, 32, 2>::PX), DsPipeCfg<144, 32, 2>::lds_bytes, kLdsRaise); break;
    case K::UsPipe192: e = us(us_pipe_kernel<192, 144, 2, 1>, pipe_grid(UsPipeCfg<192, 144, 2, 1>::PX), UsPipeCfg<192, 144, 2, 1>::lds_bytes); break;
    case K::UsPipe144: e = us(us_pipe_kernel<144, 96, 2, 2>, pipe_grid(UsPipeCfg<144, 96, 2, 2>::PX), UsPipeCfg<144, 96, 2, 2>::lds_bytes); break;
    case K::Ds48: e = ds(ds48_stream_kernel, std::min<int64_t>(ceil_div64(ntile, 4), 256), 4 * 64 * Ds48::MS * sizeof(bf16_t), kLdsAsIs); break;
    case K::DsSplit96: e = ds(ds_split_stream_kernel<96, 2>, std::min<int64_t>(ntile, 512), 64 * DsSplitCfg<96>::MS * sizeof(bf16_t), kLdsAsIs); break;
    case K::DsSplit144: e = ds(ds_split_stream_kernel<144, 1>, std::min<int64_t>(ntile, 512), 64 * DsSplitCfg<144>::MS * sizeof(bf16_t), kLdsAsIs); break;
    case K::Us96: e = us(us_stream_kernel<96, 48, 4, 1>, std::min<int64_t>(ncols / UsCfg<96, 48, 4>::PX, 512), UsCfg<96, 48, 4>::lds_bytes); break;
    case K::Us144: e = us(us_stream_kernel<144, 96, 2, 2>, std::min<int64_t>(ncols / UsCfg<144, 96, 2>::PX, 512), UsCfg<144, 96, 2>::lds_bytes); break;
    case K::Us192: e = us(us_stream_kernel<192, 144, 2, 1>, std::min<int64_t>(ncols / UsCfg<192, 144, 2>::PX, 256), UsCfg<192, 144, 2>::lds_bytes); break;
    }
    ALSEP_HIP(ctx, e);
    return finish_launch(ctx, r);
}

#ifndef ALSEP_F16_TU
template <int MODE>
int run_pix_split(alsep_ctx* ctx, const GemmLayer& L, const float* X, float* Y, const float* skip, int64_t ncols, int Tp, int Fp, int C, int C2) {
    typedef GemmSCfg Gc;
    const int64_t gx = ceil_div64(ncols, Gc::BC);
    if (gx > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "pix_gemm: too many column tiles");
    ProfScope prof(ctx, ALSEP_PROF_PIX);
    const int nrb = L.Mp / Gc::BR;
    const int fast = (nrb > 1 && gx % 8 == 0 && gx * nrb <= 0x7fffffff) ? nrb : 0;
    ALSEP_HIP(ctx, launch(ctx, pix_gemm_f32s_kernel<MODE>, fast ? dim3((unsigned)(gx * nrb)) : dim3((unsigned)gx, nrb), dim3(kThreads), Gc::lds_bytes,
                          kLdsRaise, X, Y, (const hs_t*)L.w.p, (const float*)L.scale.p, (const float*)L.shift.p, skip, L.M, L.Mp, L.K, L.Kp, ncols,
                          Tp, Fp, C, C2, L.range_flag, fast));
    note_launch(ctx, MODE == PIX_DS ? "pix_gemm_f32s_kernel<ds>" : "pix_gemm_f32s_kernel<us>");
    if (fast) note_launch(ctx, "pix_gemm_f32s_kernel<nrb_fast>");
    ALSEP_LAUNCH_CHECK(ctx, "pix_gemm_f32s_kernel");
    return ALSEP_OK;
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
    const hipError_t e = dispatch_bool(R != nullptr, [&](auto res) {
        return launch(ctx, tdf_gemm_f32s_kernel<decltype(res)::value>, grid, dim3(kThreads), Gc::lds_bytes, kLdsRaise, X, Y, (const hs_t*)L.w.p,
                      bias, (const float*)L.scale.p, (const float*)L.shift.p, R, L.M, L.Mp, L.K, L.Kp, nunits, C, L.range_flag, fast);
    });
    ALSEP_HIP(ctx, e);
    note_launch(ctx, R ? "tdf_gemm_f32s_kernel<res>" : "tdf_gemm_f32s_kernel<nores>");
    if (fast) note_launch(ctx, "tdf_gemm_f32s_kernel<nrb_fast>");
    ALSEP_LAUNCH_CHECK(ctx, "tdf_gemm_f32s_kernel");
    return ALSEP_OK;
}
#endif

template <typename T, int MODE>
int run_pix(alsep_ctx* ctx, const GemmLayer& L, const T* X, T* Y, const T* skip, int64_t ncols, int Tp, int Fp, int C, int C2) {
    typedef GemmCfg<T> Gc;
    if constexpr (std::is_same<T, float>::value) {
#ifndef ALSEP_F16_TU
        if (L.split) return run_pix_split<MODE>(ctx, L, X, Y, skip, ncols, Tp, Fp, C, C2);
#endif
    } else {
        if (L.wfrag.p && switches().pix_stream && Fp % 64 == 0) return run_pix_stream(ctx, MODE, L, X, Y, skip, ncols, Tp, Fp);
    }
    const int64_t gx = ceil_div64(ncols, Gc::BC);
    if (gx > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "pix_gemm: too many column tiles");
    ProfScope prof(ctx, ALSEP_PROF_PIX);
    ALSEP_HIP(ctx, launch(ctx, pix_gemm_kernel<T, MODE>, dim3((unsigned)gx, L.Mp / Gc::BR), dim3(kThreads), Gc::lds_bytes, kLdsAsIs, X, Y,
                          (const T*)L.w.p, (const float*)L.scale.p, (const float*)L.shift.p, skip, L.M, L.K, L.Kp, ncols, Tp, Fp, C, C2));
    if constexpr (std::is_same<T, float>::value) note_launch(ctx, MODE == PIX_DS ? "pix_gemm_kernel<f32,ds>" : "pix_gemm_kernel<f32,us>");
    ALSEP_LAUNCH_CHECK(ctx, "pix_gemm_kernel");
    return ALSEP_OK;
}

// The final 1x1 convolution of a forward, offered to the last residual TDF launch (run_block's `fin`): the launcher that
// can fold it (tdf_bf16_wide_kernel<4, true, RPF, FINAL>, tdf_bf16_persist_kernel<NT, FINAL>) sets `done`, and forward_impl() then skips
// final_conv_kernel.
struct FinalFold {
    const float* w;
    const float* b;
    void* out;
    float alpha;
    bool done;
};
// The 96 -> 48 upsampling between levels 1 and 0, offered in the same way to the last TDF launch of the block whose output it reads
// (forward_impl offers it only where run_pix would launch us_stream_kernel<96, 48>): tdf_bf16_persist_kernel<3, false, true> writes
// relu(bn(convT(block output))) * skip to `out` -- [2 BT][2 Fp][48], the block's own output buffer, which the launch never reads --
// instead of the block's output, sets `done`, and forward_impl() then skips the us launch and takes `out` as its result.
struct UsFold {
    const GemmLayer* us;
    const void* skip;
    void* out;
    int64_t BT;                                                // level-1 frames B Tp, each of Fp pixels x 96 channels
    int Fp;
    bool done;
};

// The instances that serve one TDF linear of a bf16 / f16 network with c % 48 == 0 (L.dma_path).  Wide<WM>: Nores = no residual,
// Res = residual rows requested ahead, Rpf0 = residual rows loaded where they are used, Final = Res with the final 1x1 conv folded in,
// Persist192Us = Persist192 with the 96 -> 48 upsampling folded in.
enum class TdfKernel { Plain, Wide4Nores, Wide4Res, Wide4Rpf0, Wide4Final, Wide8Nores, Wide8Res, Wide8Rpf0,
                       Persist384, Persist192, Persist384Final, Persist192Final, Persist192Us };
typedef Route<TdfKernel> TdfRoute;

// residual: the launch adds R; final_offered: the caller offers the final 1x1 conv (FinalFold); us_offered: the caller offers the
// 96 -> 48 upsampling (UsFold); nunits = B T (C / 48)
TdfRoute route_tdf_dma(const Switches& s, const GemmLayer& L, bool residual, bool final_offered, int64_t nunits, int C,
                       bool us_offered = false) {
    typedef TdfKernel K;
    typedef TdfWide<4> W4;
    const int cls = ALSEP_PROF_TDF;
    const char* const wide = "tdf_bf16_wide_kernel";
    const char* const persist = "tdf_bf16_persist_kernel";
    const char* const res = "tdf_bf16_wide_kernel<res>";
    if (!(L.wwide.p && s.tdf_wide && L.K % 64 == 0 && nunits % 4 == 0)) return {K::Plain, cls, "tdf_bf16_kernel", {}};
    const bool can8 = L.M % 384 == 0;
    const bool use8 = s.tdf_wide == 8 ? can8 : (s.tdf_wide == 4 ? false : (can8 && L.M == 384 && !residual));
    if (!residual) return {use8 ? K::Wide8Nores : K::Wide4Nores, cls, wide, {"tdf_bf16_wide_kernel<nores>"}};
    if (s.tdf_rpf == 0) return {use8 ? K::Wide8Rpf0 : K::Wide4Rpf0, cls, wide, {res}};
    if (use8) return {K::Wide8Res, cls, wide, {res}};
    const bool fold = final_offered && C == W4::UC && s.tdf_final;
    if (s.tdf_wide == 1 && L.M % TdfPersist::BM == 0 && (C == W4::UC || C == 2 * W4::UC) && (L.K == 384 || L.K == 192)) {
        const int kind = fold ? kTdfPersistFinal : (L.K == 384 ? kTdfPersistK384 : kTdfPersistK192);
        if (mask_routed(s.tdf_persist, kTdfPersistRouted, kind)) {
            if (fold) return {L.K == 384 ? K::Persist384Final : K::Persist192Final, cls, persist, {res, "tdf_bf16_wide_kernel<res,final>"}};
            // two layer launches in one: its own name, and the pinned names of the us layer it serves (route_pix_stream's Us96 row)
            if (us_offered && s.tdf_us_fold && C == 2 * W4::UC && L.K == 192)
                return {K::Persist192Us, cls, persist, {res, "tdf_bf16_persist_kernel<us>", "us_stream_kernel", "us_stream_kernel<96,48>", "pix stream kernel"}};
            return {L.K == 384 ? K::Persist384 : K::Persist192, cls, persist, {res}};
        }
    }
    if (fold) return {K::Wide4Final, cls, wide, {res, "tdf_bf16_wide_kernel<res,final>"}};
    return {K::Wide4Res, cls, wide, {res}};
}

int launch_tdf_plain(alsep_ctx* ctx, const TdfRoute& r, const GemmLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* R, const bf16_t* zp,
                     int64_t nunits, int C) {
    typedef TdfB16 Tc;
    const float* bias = L.has_bias ? (const float*)L.bias.p : nullptr;
    ProfScope prof(ctx, r.prof_class);
    const dim3 grid((unsigned)ceil_div64(nunits, Tc::UN), L.Mp / Tc::BM);
    const hipError_t e = dispatch_bool(R != nullptr, [&](auto res) {
        return launch(ctx, tdf_bf16_kernel<decltype(res)::value>, grid, dim3(kThreads), Tc::lds_bytes, kLdsAsIs, X, Y, (const bf16_t*)L.w.p, bias,
                      (const float*)L.scale.p, (const float*)L.shift.p, R, zp, L.M, L.K, L.Kp, nunits, C);
    });
    ALSEP_HIP(ctx, e);
    return finish_launch(ctx, r);
}

// fin: FINAL only (where C == 48)
template <int WM, bool RES, int RPF, bool FINAL>
int launch_tdf_wide(alsep_ctx* ctx, const TdfRoute& r, const GemmLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* R, int64_t nunits, int C,
                    FinalFold* fin) {
    typedef TdfWide<WM> Tc;
    const int64_t gx = ceil_div64(nunits, Tc::UN);
    const int nrb = L.M / Tc::BM;
    const int nyb = (switches().tdf_yfast && nrb > 1 && gx % 8 == 0 && gx * nrb <= 0x7fffffff) ? nrb : 0;
    const dim3 grid = nyb ? dim3((unsigned)(gx * nrb)) : dim3((unsigned)gx, nrb);
    ProfScope prof(ctx, r.prof_class);
    const hipError_t e = launch(ctx, tdf_bf16_wide_kernel<WM, RES, RPF, FINAL>, grid, dim3(Tc::THREADS), Tc::lds_bytes, kLdsRaise, X, Y,
                                (const bf16_t*)L.wwide.p, L.has_bias ? (const float*)L.bias.p : nullptr, (const float*)L.scale.p,
                                (const float*)L.shift.p, R, L.M, L.K, nunits, C, nyb, fin ? fin->w : nullptr, fin ? fin->b : nullptr,
                                fin ? (bf16_t*)fin->out : nullptr, fin ? fin->alpha : 0.f);
    ALSEP_HIP(ctx, e);
    if (fin) fin->done = true;
    return finish_launch(ctx, r);
}

// route_tdf_dma has checked: R != nullptr, M % 384 == 0, K = 64 NT (384 or 192), C 48 or 96, nunits % 4 == 0; fin: FINAL only (C == 48)
template <int NT, bool FINAL>
int launch_tdf_persist(alsep_ctx* ctx, const TdfRoute& r, const GemmLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* R, int64_t nunits, int C,
                       FinalFold* fin) {
    const int64_t nitems = nunits / TdfPersist::UN;
    ProfScope prof(ctx, r.prof_class);
    const hipError_t e = launch(ctx, tdf_bf16_persist_kernel<NT, FINAL>, dim3(per_cu_grid(ctx, switches().tdf_persist_grid, nitems)),   // 156.75 KiB of LDS
                                dim3(TdfPersist::THREADS), TdfPersist::lds_bytes(NT, FINAL), kLdsRaise, X, Y, (const bf16_t*)L.wwide.p,
                                L.has_bias ? (const float*)L.bias.p : nullptr, (const float*)L.scale.p, (const float*)L.shift.p, R, L.M, nitems, C,
                                fin ? fin->w : nullptr, fin ? fin->b : nullptr, fin ? (bf16_t*)fin->out : nullptr, fin ? fin->alpha : 0.f,
                                UsFoldArgs{});
    ALSEP_HIP(ctx, e);
    if (fin) fin->done = true;
    return finish_launch(ctx, r);
}

// route_tdf_dma has checked as for launch_tdf_persist, and C == 96, K == 192; forward_impl that usf->us is the 96 -> 48 layer with its
// fragment-order image and that usf->out is neither X nor R.  The block's output is not written: Y is not passed on.
int launch_tdf_persist_us(alsep_ctx* ctx, const TdfRoute& r, const GemmLayer& L, const bf16_t* X, const bf16_t* R, int64_t nunits, int C,
                          UsFold* usf) {
    const int64_t nitems = nunits / TdfPersist::UN;
    if (usf->Fp != L.M || usf->BT != nitems || usf->out == (const void*)X || usf->out == (const void*)R)
        return alsep_fail(ctx, ALSEP_ERR_STATE, "tdf: the offered upsampling does not fit the launch");
    const UsFoldArgs ua = {(const bf16_t*)usf->us->wfrag.p, (const float*)usf->us->scale.p, (const float*)usf->us->shift.p,
                           (const bf16_t*)usf->skip, (bf16_t*)usf->out};
    ProfScope prof(ctx, r.prof_class);
    const hipError_t e = launch(ctx, tdf_bf16_persist_kernel<3, false, true>, dim3(per_cu_grid(ctx, switches().tdf_persist_grid, nitems)),   // 151.1 KiB of LDS
                                dim3(TdfPersist::THREADS), TdfPersist::lds_bytes(3, false, true), kLdsRaise, X, (bf16_t*)nullptr, (const bf16_t*)L.wwide.p,
                                L.has_bias ? (const float*)L.bias.p : nullptr, (const float*)L.scale.p, (const float*)L.shift.p, R, L.M, nitems, C,
                                (const float*)nullptr, (const float*)nullptr, (bf16_t*)nullptr, 0.f, ua);
    ALSEP_HIP(ctx, e);
    usf->done = true;
    return finish_launch(ctx, r);
}

int run_tdf_dma(alsep_ctx* ctx, const GemmLayer& L, const bf16_t* X, bf16_t* Y, const bf16_t* R, const bf16_t* zp,
                int64_t BT, int C, FinalFold* fin, UsFold* usf) {
    typedef TdfKernel K;
    static_assert(TdfWide<4>::UN == TdfB16::UN && TdfWide<8>::UN == TdfB16::UN, "one column-tile count for every instance");
    const int64_t nunits = BT * (C / TdfB16::UC);
    if (ceil_div64(nunits, TdfB16::UN) > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "tdf: too many column tiles");
    const TdfRoute r = route_tdf_dma(switches(), L, R != nullptr, fin != nullptr, nunits, C, usf != nullptr);
    switch (r.kernel) {
    case K::Plain: return launch_tdf_plain(ctx, r, L, X, Y, R, zp, nunits, C);
    case K::Wide4Nores: return launch_tdf_wide<4, false, 2, false>(ctx, r, L, X, Y, R, nunits, C, nullptr);
    case K::Wide4Res: return launch_tdf_wide<4, true, 2, false>(ctx, r, L, X, Y, R, nunits, C, nullptr);
    case K::Wide4Rpf0: return launch_tdf_wide<4, true, 0, false>(ctx, r, L, X, Y, R, nunits, C, nullptr);
    case K::Wide4Final: return launch_tdf_wide<4, true, 2, true>(ctx, r, L, X, Y, R, nunits, C, fin);
    case K::Wide8Nores: return launch_tdf_wide<8, false, 2, false>(ctx, r, L, X, Y, R, nunits, C, nullptr);
    case K::Wide8Res: return launch_tdf_wide<8, true, 2, false>(ctx, r, L, X, Y, R, nunits, C, nullptr);
    case K::Wide8Rpf0: return launch_tdf_wide<8, true, 0, false>(ctx, r, L, X, Y, R, nunits, C, nullptr);
    case K::Persist384: return launch_tdf_persist<6, false>(ctx, r, L, X, Y, R, nunits, C, nullptr);
    case K::Persist192: return launch_tdf_persist<3, false>(ctx, r, L, X, Y, R, nunits, C, nullptr);
    case K::Persist384Final: return launch_tdf_persist<6, true>(ctx, r, L, X, Y, R, nunits, C, fin);
    case K::Persist192Final: return launch_tdf_persist<3, true>(ctx, r, L, X, Y, R, nunits, C, fin);
    case K::Persist192Us: return launch_tdf_persist_us(ctx, r, L, X, R, nunits, C, usf);
    }
    return alsep_fail(ctx, ALSEP_ERR_STATE, "tdf: no such route");
}

template <typename T>
int run_tdf(alsep_ctx* ctx, const GemmLayer& L, const T* X, T* Y, const T* R, int64_t BT, int C, const void* zero_page,
            FinalFold* fin = nullptr, UsFold* usf = nullptr) {
    typedef GemmCfg<T> Gc;
    if constexpr (std::is_same<T, float>::value) {
#ifndef ALSEP_F16_TU
        if (L.split) return run_tdf_split(ctx, L, X, Y, R, BT, C);
#endif
    } else {
        if (L.dma_path) return run_tdf_dma(ctx, L, X, Y, R, (const T*)zero_page, BT, C, fin, usf);
    }
    const int64_t nunits = BT * (C / 16);
    const int64_t gx = ceil_div64(nunits, 8);
    if (gx > 0x7fffffff) return alsep_fail(ctx, ALSEP_ERR_ARG, "tdf_gemm: too many column tiles");
    const float* bias = L.has_bias ? (const float*)L.bias.p : nullptr;
    ProfScope prof(ctx, ALSEP_PROF_TDF);
    const hipError_t e = dispatch_bool(R != nullptr, [&](auto res) {
        return launch(ctx, tdf_gemm_kernel<T, decltype(res)::value>, dim3((unsigned)gx, L.Mp / Gc::BR), dim3(kThreads), Gc::lds_bytes, kLdsAsIs,
                      X, Y, (const T*)L.w.p, bias, (const float*)L.scale.p, (const float*)L.shift.p, R, L.M, L.K, L.Kp, nunits, C);
    });
    ALSEP_HIP(ctx, e);
    if constexpr (std::is_same<T, float>::value) note_launch(ctx, R ? "tdf_gemm_kernel<f32,res>" : "tdf_gemm_kernel<f32,nores>");
    ALSEP_LAUNCH_CHECK(ctx, "tdf_gemm_kernel");
    return ALSEP_OK;
}

// Both TDF linears of a block (A, then B with the residual) as one launch: None = the caller runs them one by one
enum class TdfFusedKernel { None, F768, F384 };
typedef Route<TdfFusedKernel> TdfFusedRoute;

TdfFusedRoute route_tdf_fused(const Switches& s, const GemmLayer& A, const GemmLayer& B, int64_t BT, int C) {
    typedef TdfFusedKernel K;
    const TdfFusedRoute none = {K::None, ALSEP_PROF_TDF, nullptr, {}};
    const int mode = s.tdf_fused;
    if (mode <= 0 || !A.dma_path || !B.dma_path || !A.wfused.p || !B.wfused.p || C % 48 != 0 || C > TdfFused<768>::CMAX) return none;
    const bool f768 = B.M == 768;
    const int64_t nunits = BT * (C / 48);
    const int nu = f768 ? TdfFused<768>::NU : TdfFused<384>::NU;
    if (nunits <= 0 || nunits % nu != 0 || nunits > 0x7fffffff) return none;
    const int64_t nitems = nunits / nu;
    if (mode == 1 && (!(kTdfFusedRouted & (f768 ? kTdfFusedF768 : kTdfFusedF384)) || nitems < kTdfFusedFloor[f768 ? 0 : 1])) return none;
    return {f768 ? K::F768 : K::F384, ALSEP_PROF_TDF, "tdf_bf16_fused_kernel", {"tdf_bf16_kernel", "tdf_bf16_kernel"}};   // two layer launches
}

template <int F_>
int launch_tdf_fused(alsep_ctx* ctx, const TdfFusedRoute& r, const GemmLayer& A, const GemmLayer& B, const bf16_t* X, bf16_t* Y, int64_t BT, int C) {
    typedef TdfFused<F_> P;
    const int64_t nitems = BT * (C / 48) / P::NU;
    ProfScope prof(ctx, r.prof_class);
    const hipError_t e = launch(ctx, tdf_bf16_fused_kernel<F_>, dim3(per_cu_grid(ctx, switches().tdf_fused_grid, nitems)),   // 156 / 159 KiB of LDS
                                dim3(P::THREADS), P::lds_bytes, kLdsRaise, X, Y, (const bf16_t*)A.wfused.p, (const bf16_t*)B.wfused.p,
                                A.has_bias ? (const float*)A.bias.p : nullptr, (const float*)A.scale.p, (const float*)A.shift.p,
                                B.has_bias ? (const float*)B.bias.p : nullptr, (const float*)B.scale.p, (const float*)B.shift.p, (int)nitems, C);
    ALSEP_HIP(ctx, e);
    return finish_launch(ctx, r);
}
// Both linears of blk as one launch where ALSEP_TDF_FUSED routes it (*done); otherwise nothing is launched and the caller runs them.
int run_tdf_fused(alsep_ctx* ctx, const Block& blk, const bf16_t* X, bf16_t* Y, int64_t BT, int C, bool* done) {
    const GemmLayer& A = blk.tdf[0];
    const GemmLayer& B = blk.tdf[1];
    const TdfFusedRoute r = route_tdf_fused(switches(), A, B, BT, C);
    *done = r.kernel != TdfFusedKernel::None;
    switch (r.kernel) {
    case TdfFusedKernel::None: break;
    case TdfFusedKernel::F768: return launch_tdf_fused<768>(ctx, r, A, B, X, Y, BT, C);
    case TdfFusedKernel::F384: return launch_tdf_fused<384>(ctx, r, A, B, X, Y, BT, C);
    }
    return ALSEP_OK;
}

// TFC_TDF block: cur -> dest, using scratch a, b (cur may alias b), hidden h.  fin (last block of the network only): the
// residual TDF launch may produce the network's output instead of dest (FinalFold).  usf (the block under the last upsampling only):
// that launch may write the upsampled level-0 activation into dest instead of the block's output (UsFold; usf->out == dest).
template <typename T>
int run_block(alsep_ctx* ctx, const alsep_net* net, const Block& blk, const T* cur, T* a, T* b, T* h, T* dest,
              int64_t B, int Th, int Fw, int c, FinalFold* fin = nullptr, UsFold* usf = nullptr) {
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
        if constexpr (!std::is_same<T, float>::value) {      // a float32 block has no fused image
            bool fused = false;
            if ((rc = run_tdf_fused(ctx, blk, src, dest, B * Th, c, &fused)) || fused) return rc;
        }
        if ((rc = run_tdf<T>(ctx, blk.tdf[0], src, h, (const T*)nullptr, B * Th, c, net->zero_page.p))) return rc;
        return run_tdf<T>(ctx, blk.tdf[1], h, dest, src, B * Th, c, net->zero_page.p, fin, usf);
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
        ALSEP_HIP(ctx, launch(ctx, first_conv_kernel<T>, dim3((unsigned)nblk), dim3(kFirstThreads), 0, kLdsAsIs, in, P[0], (const float*)net->first_w.p,
                              (const float*)net->first_scale.p, (const float*)net->first_shift.p, npix0, cfg.g, in_scale));
        ALSEP_LAUNCH_CHECK(ctx, "first_conv_kernel");
    }
    // the last block may write `out` itself; the accumulating pass of a denoise pair (out_beta != 0) keeps the separate kernel
    FinalFold fold = {(const float*)net->final_w.p, (const float*)net->final_b.p, out, out_alpha, false};
    FinalFold* const fin = (!std::is_same<T, float>::value && out_beta == 0.f) ? &fold : nullptr;
    // the block under the last upsampling may write the upsampled level-0 activation itself (UsFold), offered exactly where run_pix
    // would launch us_stream_kernel<96, 48> for that layer
    UsFold ufold = {};
    UsFold* usf = nullptr;
    if constexpr (!std::is_same<T, float>::value) {
        if (net->n >= 1) {
            const GemmLayer& U = net->us[net->n - 1];
            const int Fp = cfg.dim_f / 2;
            if (U.wfrag.p && U.K == 2 * TdfPersist::UC && U.M == 4 * TdfPersist::UC && switches().pix_stream && Fp % 64 == 0) {
                ufold = {&U, ws + L.skip[0], nullptr, B * (cfg.dim_t / 2), Fp, false};
                usf = &ufold;
            }
        }
    }
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
        UsFold* const uf = net->n == 1 ? usf : nullptr;
        if (uf) uf->out = dest;
        if ((rc = run_block<T>(ctx, net, net->bott, P[ic], P[(ic + 2) % 3], P[ic], H, dest, B, Th, Fw, c, net->n == 0 ? fin : nullptr, uf)))
            return rc;
        ic = (ic + 1) % 3;
    }
    for (int i = 0; i < net->n; ++i) {
        const T* skip = (const T*)(ws + L.skip[net->n - 1 - i]);
        const int c2 = c - cfg.g;
        // a folded upsampling (the last one only) has left its result where the block's output would be: P[ic] is `up` already
        const bool folded = i == net->n - 1 && ufold.done;
        const int iu = folded ? ic : (ic + 1) % 3, id = folded ? (ic + 1) % 3 : ic;
        T* up = P[iu];
        // us: P[ic] [B,Th,Fw,c] -> up [B,2Th,2Fw,c2] * skip
        if (!folded && (rc = run_pix<T, PIX_US>(ctx, net->us[i], P[ic], up, skip, B * Th * Fw, Th, Fw, c, c2))) return rc;
        Th *= 2; Fw *= 2; c = c2;
        T* dest = P[id];                                   // old input is dead after the up conv
        UsFold* const uf = i == net->n - 2 ? usf : nullptr;
        if (uf) uf->out = dest;
        if ((rc = run_block<T>(ctx, net, net->dec[i], up, P[(ic + 2) % 3], up, H, dest, B, Th, Fw, c, i == net->n - 1 ? fin : nullptr, uf)))
            return rc;
        ic = id;                                           // the block's output (unchanged unless the upsampling was folded)
    }
    if (fold.done) return ALSEP_OK;
    ProfScope prof(ctx, ALSEP_PROF_POINTWISE);
    ALSEP_HIP(ctx, launch(ctx, final_conv_kernel<T>, dim3((unsigned)ceil_div64(npix0, kThreads)), dim3(kThreads), (size_t)kThreads * cfg.g * sizeof(T),
                          kLdsAsIs, (const T*)P[ic], out, (const float*)net->final_w.p, (const float*)net->final_b.p, npix0, cfg.g, out_alpha, out_beta));
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
