// The persistent 8-wave bf16 / f16 3x3 convolutions of the TFC-TDF U-Net: conv3x3_bf16_big_kernel, _mq_kernel, _m0_kernel and
// _allco_kernel (device code only; included by tdfnet.hip, which keeps their weight packers, launchers and dispatch).  They have one
// argument list and one skeleton -- a workgroup of 8 waves walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ..., a wave owns one
// pixel row of an 8 x TW tile, the halo patch arrives by LDS-DMA through descriptors computed once -- and share what is below: the
// tile decode, the halo descriptors and stager, and the epilogue.  A kernel keeps what is its own: its k-loop, its weight ring and
// its counted vmcnt waits.
#pragma once

constexpr int kBigThreads = 512;

// ------------------------------------------------------------------------------------------
// shared scaffold; Cf is the kernel's configuration struct
// ------------------------------------------------------------------------------------------
// tile k of this workgroup: its first row and column and its batch index (tiles run f fastest, then t, then batch)
template <typename Cf>
__device__ __forceinline__ void conv8_tile(int k, int tiles_t, int tiles_f, int& t0, int& f0, int64_t& b) {
    int tile = (int)blockIdx.x + k * (int)gridDim.x;
    const int tf = tile % tiles_f;  tile /= tiles_f;
    const int tt = tile % tiles_t;
    b = tile / tiles_t;
    t0 = tt * Cf::TH;
    f0 = tf * Cf::TW;
}

// LDS-DMA descriptor of 16-byte unit u of a patch image, a per-lane constant: unit -> (pixel P, position) -> channel group
// (Cf::pswz: the position swizzle of the pixel record) -> prel, the element offset from the tile's first pixel.  Returns the four
// "outside the image if the tile touches that border" bits (top row, bottom row, left column, right column of the halo), to be
// matched against halo_border of a tile.  Units past the image (the tail of the last instruction) are clamped to the last one.
template <typename Cf>
__device__ __forceinline__ unsigned halo_unit(int u, int Fw, int Cin, int& prel) {
    const int uu = u < Cf::PGROUPS ? u : Cf::PGROUPS - 1;
    const int P = uu / Cf::CG, cg = (uu % Cf::CG) ^ Cf::pswz(P);
    const int dt = P / Cf::PW - 1, df = P % Cf::PW - 1;
    prel = (dt * Fw + df) * Cin + cg * 8;
    return (unsigned)((dt < 0) | ((dt >= Cf::TH) << 1) | ((df < 0) << 2) | ((df >= Cf::TW) << 3));
}
template <typename Cf>
__device__ __forceinline__ unsigned halo_border(int t0, int f0, int Th, int Fw) {
    return (unsigned)(t0 == 0) | ((unsigned)(t0 + Cf::TH >= Th) << 1) | ((unsigned)(f0 == 0) << 2) | ((unsigned)(f0 + Cf::TW >= Fw) << 3);
}

// Halo stager of the kernels with two patch buffers (mq, m0, allco).  Piece j of a wave is instruction i = wave + 8 j of the PINST
// that cover a patch buffer of PBUF units; every wave issues PJ pieces per patch, so that the counted vmcnt waits see a constant.  A
// piece has 5 flag bits, the four halo bits and "dead unit" (the units of the buffer past the image: they read the zero page, i.e.
// count as outside on every side); a surplus piece (i >= PINST) copies the zero page into the kernel's 1 KiB scratch.
// conv3x3_bf16_big_kernel does not use it: one patch buffer, no scratch, its surplus lanes and pieces are skipped, not redirected.
template <typename Cf>
struct HaloStager {
    static constexpr int NW = (Cf::PJ + 5) / 6;             // flag words: 6 pieces each
    const bf16_t* X; const bf16_t* zero_page;
    bf16_t* patch0; bf16_t* scratch;
    int Th, Fw, Cin, tiles_t, tiles_f, wave;
    int prel[Cf::PJ];
    unsigned pflags[NW];
    const bf16_t* psrc;                                      // set by prep, used by one
    unsigned pborder;
    bf16_t* pdst;

    // the descriptors, computed once: per patch, the divisions and 64-bit address arithmetic of the pieces cost a wave ~4,000 cycles
    __device__ __forceinline__ void init(const bf16_t* X_, const bf16_t* zero_page_, bf16_t* patch0_, bf16_t* scratch_, int Th_, int Fw_,
                                         int Cin_, int tiles_t_, int tiles_f_, int wave_, int lane) {
        X = X_; zero_page = zero_page_; patch0 = patch0_; scratch = scratch_;
        Th = Th_; Fw = Fw_; Cin = Cin_; tiles_t = tiles_t_; tiles_f = tiles_f_; wave = wave_;
#pragma unroll
        for (int w = 0; w < NW; ++w) pflags[w] = 0;
#pragma unroll
        for (int j = 0; j < Cf::PJ; ++j) {
            const int u = (wave + 8 * j) * 64 + lane;
            const unsigned bits = halo_unit<Cf>(u, Fw, Cin, prel[j]);
            pflags[j / 6] |= (u < Cf::PGROUPS ? bits : 16u) << (5 * (j % 6));
        }
        psrc = X; pborder = 0; pdst = patch0;
    }
    // Patch ps of the workgroup's npatch -> buffer ps & 1.  A patch is (item, chunk ps % nq of Cf::KC input channels) and an item one
    // of the Cf::NGRP output groups of a tile, a tile's groups back to back.  Past the last patch the last one is fetched again into
    // the free buffer: the LDS-DMA count per stage stays constant (the kernels' vmcnt waits count instructions).
    __device__ __forceinline__ void prep(int ps, int npatch, int nq) {
        const int pc = ps < npatch ? ps : npatch - 1;
        int t0, f0; int64_t b;
        conv8_tile<Cf>(pc / nq / Cf::NGRP, tiles_t, tiles_f, t0, f0, b);
        psrc = X + ((b * Th + t0) * (int64_t)Fw + f0) * Cin + (pc % nq) * Cf::KC;
        pborder = halo_border<Cf>(t0, f0, Th, Fw);
        pdst = patch0 + (size_t)(ps & 1) * Cf::PBUF * 8;
    }
    __device__ __forceinline__ void one(int j) {            // piece j of the patch of the last prep
        const int i = wave + 8 * j;
        const bool out = (pflags[j / 6] & ((pborder | 16u) << (5 * (j % 6)))) != 0;
        const bool real = j < Cf::PJ - 1 || i < Cf::PINST;
        // PREL_OPAQUE (allco, which has no register to spare): the offset is sign-extended here, not kept as a 64-bit pair
        const bf16_t* src = (out || !real) ? zero_page : psrc + (Cf::PREL_OPAQUE ? opaque_vgpr(prel[j]) : prel[j]);
        glds16(src, real ? pdst + (size_t)i * 64 * 8 : scratch);
    }
};

// Epilogue of one wave: y = max(acc * scale + shift, 0) for NI blocks of 16 pixels x NB blocks of 16 weight rows.  The packed weight
// rows are in the order ConvBig::channel_of_row (the packers depend on it): the lane's rows of blocks 2 j, 2 j + 1 are channels
// 32 j + 8 lq + [0, 8), one 16-byte store, and an odd last block keeps channels 16 (NB - 1) + 4 lq + [0, 4), one 8-byte store.  Below,
// N = 2 is such a pair and N = 1 the odd block, b0 the first block: channels 16 b0 + 4 N lq + [0, 4 N).
template <int N>
__device__ __forceinline__ void conv8_quads(const float* sc, const float* sh, int b0, int lq, f32x4 (&scv)[N], f32x4 (&shv)[N]) {
    const int co = b0 * 16 + lq * 4 * N;
#pragma unroll
    for (int h = 0; h < N; ++h) {
        scv[h] = *reinterpret_cast<const f32x4*>(sc + co + 4 * h);               // ext-vector load: see regw kernel
        shv[h] = *reinterpret_cast<const f32x4*>(sh + co + 4 * h);
    }
}
template <int N, int NB, int NI>
__device__ __forceinline__ void conv8_store(bf16_t* yp, int Cout, const f32x4 (&acc)[NB][NI], const f32x4 (&scv)[N], const f32x4 (&shv)[N],
                                            int b0, int lq, int ni) {
    float y[4 * N];
#pragma unroll
    for (int h = 0; h < N; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) y[4 * h + r] = fmaxf(fmaf(acc[b0 + h][ni][r], scv[h][r], shv[h][r]), 0.f);
    bf16_t* p = yp + (int64_t)ni * 16 * Cout + b0 * 16 + lq * 4 * N;
    if constexpr (N == 2) store8(p, y);
    else store4(p, y);
}
// yp: the lane's pixel (tile row wave, column l15) at the first of the 16 NB channels; sc, sh: their scale and shift rows in LDS.
// Loop order and the life of the scale / shift quads:
//   kPixelsHold    pixel blocks outermost, the quads of all blocks held across them (8 NB registers: m0, which has them);
//   kPixelsReread  pixel blocks outermost, the pairs' quads read again for every pixel block (mq, big: 244 and 227 VGPRs);
//   kPairsOuter    block pairs outermost: a pair's quads are read once and are dead before the next pair's (allco: the accumulators
//                  of the all-channels kernel leave no room for more).
enum Conv8Order { kPixelsHold, kPixelsReread, kPairsOuter };
template <Conv8Order ORDER, int NB, int NI>
__device__ __forceinline__ void conv8_epilogue(bf16_t* yp, int Cout, const float* sc, const float* sh, int lq, const f32x4 (&acc)[NB][NI]) {
    f32x4 scv[2], shv[2], sco[1], sho[1];
    if constexpr (ORDER == kPairsOuter) {
#pragma unroll
        for (int j = 0; j < NB / 2; ++j) {
            conv8_quads<2>(sc, sh, 2 * j, lq, scv, shv);
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) conv8_store<2>(yp, Cout, acc, scv, shv, 2 * j, lq, ni);
        }
        if constexpr (NB % 2 == 1) {
            conv8_quads<1>(sc, sh, NB - 1, lq, sco, sho);
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) conv8_store<1>(yp, Cout, acc, sco, sho, NB - 1, lq, ni);
        }
    } else {
        if constexpr (NB % 2 == 1) conv8_quads<1>(sc, sh, NB - 1, lq, sco, sho);     // the odd block's two quads are held in both orders
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int lqr = ORDER == kPixelsReread ? opaque_vgpr(lq) : lq;       // opaque: nothing read through it is kept
#pragma unroll
            for (int j = 0; j < NB / 2; ++j) {
                conv8_quads<2>(sc, sh, 2 * j, lqr, scv, shv);
                conv8_store<2>(yp, Cout, acc, scv, shv, 2 * j, lq, ni);
            }
            if constexpr (NB % 2 == 1) conv8_store<1>(yp, Cout, acc, sco, sho, NB - 1, lq, ni);
        }
    }
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
    __host__ __device__ static constexpr int pswz(int) { return 0; }     // pixel records are not swizzled
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

    // LDS-DMA descriptors of the halo patch (halo_unit), computed once: piece j of this wave is instruction i = wave + 8 j of the
    // PINST = 62 that cover the patch.  (Computed per patch they cost each wave 14 % of the kernel, in-kernel stamps of round 2.)
    constexpr int PJ = (Cf::PINST + 7) / 8;
    int prel[PJ];
    unsigned pflags = 0;                                     // the 4 halo bits per piece
    bool plast_ok = true;                                    // lanes of the last, partial instruction that hold a patch group
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
        const int gidx = (wave + 8 * j) * 64 + lane;
        pflags |= halo_unit<Cf>(gidx, Fw, Cin, prel[j]) << (4 * j);
        if (j == PJ - 1) plast_ok = gidx < Cf::PGROUPS;
    }
    auto issue_patch = [&](int ps) {                         // (tile ps / nq, chunk ps % nq); waited with vmcnt(0)
        int t0, f0; int64_t b;
        conv8_tile<Cf>(ps / nq, tiles_t, tiles_f, t0, f0, b);
        const bf16_t* xb = X + ((b * Th + t0) * (int64_t)Fw + f0) * Cin + (ps % nq) * Cf::KC;
        const unsigned border = halo_border<Cf>(t0, f0, Th, Fw);
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
                conv8_tile<Cf>(ps / nq, tiles_t, tiles_f, t0, f0, b);
                bf16_t* yp = Y + ((b * Th + t0 + wave) * (int64_t)Fw + f0 + l15) * Cout;
                conv8_epilogue<kPixelsReread>(yp, Cout, ss, ss + NY * Cf::BN, lq, reinterpret_cast<const f32x4 (&)[Cf::NB][4]>(acc));   // block 3 yy + mi
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
    static constexpr int NGRP = 1;                          // HaloStager: one item per tile
    static constexpr bool PREL_OPAQUE = false;
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
    // patch ps = (tile ps / nq, chunk ps % nq); its last instructions, 40 and 41, are real for waves 0 and 1 only
    HaloStager<Cf> halo;
    halo.init(X, zero_page, patch0, scratch, Th, Fw, Cin, tiles_t, tiles_f, wave, lane);
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
        halo.prep(0, npatch, nq);
#pragma unroll
        for (int j = 0; j < Cf::PJ; ++j) halo.one(j);
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
        if (pt == 0) halo.prep(ps + 1, npatch, nq);
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
                            if (st == 2) { halo.one(0); halo.one(1); }
                            if (st == 3) { halo.one(2); halo.one(3); }
                            if (st == 4) { halo.one(4); halo.one(5); }
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
            conv8_tile<Cf>(ps / nq, tiles_t, tiles_f, t0, f0, b);
            bf16_t* yp = Y + ((b * Th + t0 + wave) * (int64_t)Fw + f0 + l15) * Cout;
            conv8_epilogue<kPixelsReread>(yp, Cout, ss, ss + Cf::ROWS, lq, acc);
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
    static constexpr int NGRP = 1;                          // HaloStager: one item per tile, plain pixel records
    static constexpr bool PREL_OPAQUE = false;
    __host__ __device__ static constexpr int pswz(int) { return 0; }
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
    HaloStager<Cf> halo;                                     // a patch per tile: my_tiles patches of one chunk (Cin = KC)
    halo.init(X, zero_page, patch0, scratch, Th, Fw, Cin, tiles_t, tiles_f, wave, lane);

    constexpr int ST = 2 * Cf::NI;                           // epilogue stores per wave and tile
    f32x4 acc[3][3];
    if (my_tiles > 0) {
        halo.prep(0, my_tiles, 1);
#pragma unroll
        for (int j = 0; j < Cf::PJ; ++j) halo.one(j);
    }
    auto epilogue = [&](int k) {
        int t0, f0; int64_t b;
        conv8_tile<Cf>(k, tiles_t, tiles_f, t0, f0, b);
        bf16_t* yp = Y + ((b * Th + t0 + wave) * (int64_t)Fw + f0 + l15) * Cout;
        conv8_epilogue<kPixelsHold>(yp, Cout, ss, ss + Cf::ROWS, lq, acc);
    };
    for (int k = 0; k < my_tiles; ++k) {
        // in flight, oldest first: [this tile's patch (and, k = 0, the weights)] [the ST stores of the previous tile]
        if (k > 0) wait_vmcnt<ST>();
        else wait_vmcnt<0>();
        barrier_nodrain();
        halo.prep(k + 1, my_tiles, 1);
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int ni = 0; ni < 3; ++ni) acc[b][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            const bf16_t* patch = patch0 + (size_t)(k & 1) * Cf::PBUF * 8;
            bf16x8 xa[3], wa[3], xb[3], wb[3];
            m0_steps<0>(acc, xa, wa, xb, wb, patch, pk, we, wo, [&](int st) {
                if (st < Cf::PJ) halo.one(st);              // the next tile's patch, one piece per k-step
            });
        }
        epilogue(k);
    }
    wait_vmcnt<0>();
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
    static constexpr bool PREL_OPAQUE = true;               // HaloStager: plain pixel records, offsets kept as 32 bits
    __host__ __device__ static constexpr int pswz(int) { return 0; }
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
    HaloStager<Cf> halo;
    halo.init(X, zero_page, patch0, scratch, Th, Fw, Cin, tiles_t, tiles_f, wave, lane);
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
        halo.prep(0, npatch, nq);
#pragma unroll
        for (int j = 0; j < Cf::PJ; ++j) halo.one(j);
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
    auto epilogue = [&](int k, int g) {
        int t0, f0; int64_t b;
        conv8_tile<Cf>(k, tiles_t, tiles_f, t0, f0, b);
        // the lane's coordinates again, opaque: everything the stores derive from them is computed here, not kept across the k-loops
        const int le = opaque_vgpr(lane), l15 = le & 15, lq = le >> 4;
        const int c0 = Cf::NGRP > 1 ? g * Cf::ROWS : 0;      // the group's first channel
        bf16_t* yp = Y + ((b * Th + t0 + wave) * (int64_t)Fw + f0 + l15) * Cout + c0;
        const float* const ssg = ss + c0;                    // the group's scale rows; its shift rows are COUT further on
        conv8_epilogue<kPairsOuter>(yp, Cout, ssg, ssg + Cf::COUT, lq, acc);
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
                halo.prep(p + 1, npatch, nq);
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
                if constexpr (ui == Cf::WJ && sc < Cf::PJ) halo.one(sc);
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

