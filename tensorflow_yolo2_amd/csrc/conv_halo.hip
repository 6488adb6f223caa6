// 3x3 stride-1 SAME convolution as an im2col-free implicit GEMM with an LDS-resident
// HALO tile (gfx950).  Replaces tf.nn.conv2d(..., 'SAME') + bias for filter_size 3
// (reference src/yolo2_nets/darknet.py:20-21,32-36) and its dgrad.
//
// Why: in the per-tap implicit GEMM every one of the 9 taps re-stages the (shifted)
// pixel tile -- measured on MI355X those strided 128-byte row gathers, not the MFMAs,
// set the kernel time.  Here the block stages ONE contiguous range of the bordered
// pixel space per K-chunk: all interior pixels of the tile plus one row/column of halo
// (the shared-border layout of common.h makes that range contiguous), and the nine
// taps are nine row-shifted views of that single LDS image:
//     LDS row of (pixel p, tap kh,kw) = arow_tl(p) + kh*pitch + kw.
// Pixel-side global->LDS traffic drops by ~6x at 13x13 (9 taps x 128 rows -> 184 rows),
// and the L2 sees long contiguous reads instead of per-tap gathers.  Only the filter
// tile streams per (tap, chunk) step, through an NSB-deep global_load_lds ring with a
// counted vmcnt and raw s_barrier (loads stay in flight across the barrier).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "common.h"
#include "conv_epilogue.h"
#include "kernels.h"

namespace y2 {

template <typename T, int WP, int WC, int TP, int TC, int BKB, int NSB, bool ADB>
struct HaloCfg {
    static constexpr int NW = WP * WC, NT = NW * 64;
    static constexpr int BP = WP * TP * 32, BC = WC * TC * 32;
    static constexpr int SZ = sizeof(T);
    static constexpr int LPR = BKB / 16, RPI = 64 / LPR, RPB = 256 / BKB;
    static constexpr int NI_C = BC / RPI;
    static constexpr int IPWB = (NI_C + NW - 1) / NW;
    static constexpr int IPW_MIN = NI_C / NW;
    static constexpr int BSTAGE = BC * BKB;
    static constexpr int KG = BKB / 32;
    static constexpr int NA = ADB ? 2 : 1;
};

template <typename T, int WP, int WC, int TP, int TC, int BKB, int NSB, bool ADB, int ABL = 0>
__global__ __launch_bounds__(WP* WC * 64) void conv_halo_kernel(ConvArgs a, int arows) {
    typedef HaloCfg<T, WP, WC, TP, TC, BKB, NSB, ADB> Cfg;
    typedef typename Elem<T>::frag frag_t;
    constexpr int NW = Cfg::NW, BP = Cfg::BP, BC = Cfg::BC, SZ = Cfg::SZ;
    constexpr int LPR = Cfg::LPR, RPI = Cfg::RPI, RPB = Cfg::RPB, KG = Cfg::KG, IPWB = Cfg::IPWB;
    constexpr bool PRIO = (ABL & 32) != 0;   // dev: s_setprio(1) around the MFMA clusters
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = w / WC, wc = w % WC;
    const int nCT = (a.Cout + BC - 1) / BC;
    const int bx = xcd_block(blockIdx.x, gridDim.x, a.xcd);
    const int ct = bx % nCT, pt = bx / nCT;
    const int m0 = pt * BP, n0 = ct * BC;
    const int pitch = a.W + 1, hw = a.H * a.W;
    const int Ktot = 9 * a.C;
    const char* __restrict__ xg = (const char*)a.x;
    const char* __restrict__ wg = (const char*)a.w;

    auto bpos = [&](int p) -> long {  // bordered position of interior pixel p (linear n,h,w index)
        const int n = p / hw, rem = p - n * hw;
        const int h = rem / a.W, ww = rem - h * a.W;
        return (long)bpix(n, h, ww, a.H, a.W);
    };
    // the A image covers bordered positions [lo, lo + nrows): top-left tap of the first pixel
    // ... bottom-right tap of the last pixel
    const int p_last = (m0 + BP - 1 < a.M) ? m0 + BP - 1 : a.M - 1;
    const long lo = bpos(m0) - pitch - 1;
    const int nrows = (int)(bpos(p_last) + pitch + 1 - lo) + 1;
    const int npieces = (nrows + RPI - 1) / RPI;
    const int abytes = arows * BKB;
    char* const bbase = smem + Cfg::NA * abytes;

    const int lrow = lane / LPR, lslot = lane % LPR;
    const int rowbytes = a.C * SZ;
    auto issueA = [&](int c, int ab) {
        const char* xs = xg + lo * (long)rowbytes + (long)c * BKB;
        char* dst = smem + ab * abytes;
        for (int i = w; i < npieces; i += NW) {
            const int row = i * RPI + lrow;
            const uint32_t off = (uint32_t)row * (uint32_t)rowbytes + (uint32_t)((lslot ^ ((row / RPB) % LPR)) * 16);
            if (!(ABL & 1)) glds16(xs + off, dst + i * 1024);
        }
    };
    uint32_t voffB[IPWB];
#pragma unroll
    for (int i = 0; i < IPWB; ++i) {
        const int r = (i * NW + w) * RPI + lrow;
        voffB[i] = (uint32_t)(n0 + r) * (uint32_t)(Ktot * SZ) + (uint32_t)((lslot ^ ((r / RPB) % LPR)) * 16);
    }
    auto issueB = [&](int c, int t, int buf) {
        const char* ws = wg + (size_t)(t * rowbytes + c * BKB);
        char* dst = bbase + buf * Cfg::BSTAGE;
#pragma unroll
        for (int i = 0; i < IPWB; ++i) {
            const int ii = i * NW + w;
            if (!(ABL & 2) && ((i + 1) * NW <= Cfg::NI_C || ii < Cfg::NI_C)) glds16(ws + voffB[i], dst + ii * 1024);
        }
    };

    // fragment addressing
    const int r32 = lane & 31, hh = lane >> 5;
    int arow_tl[TP];
#pragma unroll
    for (int j = 0; j < TP; ++j) {
        int p = m0 + (wp * TP + j) * 32 + r32;
        if (p > a.M - 1) p = a.M - 1;
        arow_tl[j] = (int)(bpos(p) - pitch - 1 - lo);
    }
    int foffB[KG];
#pragma unroll
    for (int g = 0; g < KG; ++g) foffB[g] = r32 * BKB + (((2 * g + hh) ^ ((r32 / RPB) % LPR)) * 16);
    const int cbase = (wc * TC) * 32 * BKB;

    f32x16 acc[TC][TP];
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
        for (int j = 0; j < TP; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    const int nchunks = rowbytes / BKB;
    const int steps = nchunks * 9;
    // prologue: A(0) first (oldest), then NSB-1 filter stages
    issueA(0, 0);
    {
        int c0 = 0, t0 = 0;
#pragma unroll
        for (int s0 = 0; s0 < NSB - 1; ++s0) {
            if (s0 < steps) issueB(c0, t0, s0);
            if (++t0 == 9) { t0 = 0; ++c0; }
        }
    }
    int c = 0, t = 0, kh = 0, kw = 0;          // current step
    int ci = 0, ti = NSB - 1;                  // step being issued (NSB-1 ahead)
    while (ti >= 9) { ti -= 9; ++ci; }
    int bbuf = 0, ibuf = NSB - 1;
    for (int s = 0; s < steps; ++s) {
        if (s + NSB - 2 < steps) wait_vmcnt<(NSB - 2) * Cfg::IPW_MIN>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (s + NSB - 1 < steps) issueB(ci, ti, ibuf);
        if (t == 0) {
            if (ADB) {
                if (c + 1 < nchunks) issueA(c + 1, (c + 1) & 1);
            } else if (c > 0) {
                issueA(c, 0);          // single image: everyone is past the barrier, the old one is dead
                wait_vmcnt<0>();
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
        }
        const char* ab = smem + (ADB ? (c & 1) : 0) * abytes;
        const char* bb = bbase + bbuf * Cfg::BSTAGE;
        const int shift = kh * pitch + kw;
        int aoff[TP], asw[TP];
#pragma unroll
        for (int j = 0; j < TP; ++j) {
            const int row = arow_tl[j] + shift;
            aoff[j] = row * BKB;
            asw[j] = (row / RPB) % LPR;
        }
        // Fragment double-buffering across the k-groups: the LDS reads of group g+1 are in flight
        // while the TC*TP MFMAs of group g issue (the compiler's own schedule keeps the reads
        // just-in-time, which exposes the LDS latency once per group).
        auto load_frags = [&](int g, frag_t (&fc)[TC], frag_t (&fp)[TP]) {
            if (ABL & 8) {
#pragma unroll
                for (int i = 0; i < TC; ++i)
#pragma unroll
                    for (int e = 0; e < Elem<T>::kPerFrag; ++e) fc[i][e] = (T)(float)(s + e);
#pragma unroll
                for (int j = 0; j < TP; ++j)
#pragma unroll
                    for (int e = 0; e < Elem<T>::kPerFrag; ++e) fp[j][e] = (T)(float)(s - e + aoff[j]);
            } else {
#pragma unroll
                for (int i = 0; i < TC; ++i) fc[i] = *(const frag_t*)(bb + cbase + i * 32 * BKB + foffB[g]);
#pragma unroll
                for (int j = 0; j < TP; ++j) fp[j] = *(const frag_t*)(ab + aoff[j] + (((2 * g + hh) ^ asw[j]) * 16));
            }
        };
        auto mma_group = [&](frag_t (&fc)[TC], frag_t (&fp)[TP]) {
            if (ABL & 4) {
#pragma unroll
                for (int i = 0; i < TC; ++i) asm volatile("" ::"v"(fc[i]));
#pragma unroll
                for (int j = 0; j < TP; ++j) asm volatile("" ::"v"(fp[j]));
            } else {
                if (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int i = 0; i < TC; ++i)
#pragma unroll
                    for (int j = 0; j < TP; ++j) mma32(acc[i][j], fc[i], fp[j]);
                if (PRIO) __builtin_amdgcn_s_setprio(0);
            }
        };
        frag_t fc0[TC], fp0[TP], fc1[TC], fp1[TP];
        load_frags(0, fc0, fp0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < KG; g += 2) {
            load_frags(g + 1, fc1, fp1);
            mma_group(fc0, fp0);
            __builtin_amdgcn_sched_barrier(0);
            if (g + 2 < KG) load_frags(g + 2, fc0, fp0);
            mma_group(fc1, fp1);
            __builtin_amdgcn_sched_barrier(0);
        }
        // advance
        if (++kw == 3) { kw = 0; ++kh; }
        if (++t == 9) { t = 0; kh = 0; ++c; }
        if (++ti == 9) { ti = 0; ++ci; }
        bbuf = (bbuf + 1 == NSB) ? 0 : bbuf + 1;
        ibuf = (ibuf + 1 == NSB) ? 0 : ibuf + 1;
    }
    __syncthreads();
    if (ABL & 16) {   // skip the epilogue (keep the accumulators alive)
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int j = 0; j < TP; ++j) t += acc[i][j][0] + acc[i][j][7];
        if (t == 123.456f) ((float*)a.y)[0] = t;
        return;
    }
    conv_epilogue<T, WP, WC, TP, TC>(a, acc, smem, w, lane, m0, n0, pt, ct);
}

template <typename T, int WP, int WC, int TP, int TC, int BKB, int NSB, bool ADB, int ABL = 0>
static hipError_t halo_launch(const ConvArgs& a, int arows, hipStream_t s) {
    typedef HaloCfg<T, WP, WC, TP, TC, BKB, NSB, ADB> Cfg;
    typedef EpiCfg<T, WP, WC, TP, TC> Epi;
    size_t lds = (size_t)Cfg::NA * arows * BKB + (size_t)NSB * Cfg::BSTAGE;
    if (lds < (size_t)Epi::LDS) lds = Epi::LDS;
    if (lds > 160 * 1024) return hipErrorInvalidValue;      // (plan_conv only picks tiles that fit)
    auto kern = conv_halo_kernel<T, WP, WC, TP, TC, BKB, NSB, ADB, ABL>;
    static size_t attr = 0;
    if (lds > attr) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        attr = lds;
    }
    const int nPT = (a.M + Cfg::BP - 1) / Cfg::BP;
    const int nCT = (a.Cout + Cfg::BC - 1) / Cfg::BC;
    hipLaunchKernelGGL(kern, dim3(nPT * nCT), dim3(Cfg::NT), lds, s, a, arows);
    return hipGetLastError();
}

// double-buffer the A image when there is more than one K-chunk and LDS allows it
template <typename T, int WP, int WC, int TP, int TC, int BKB, int NSB, int ABL = 0>
static hipError_t halo_pick(const ConvArgs& a, hipStream_t s) {
    typedef HaloCfg<T, WP, WC, TP, TC, BKB, NSB, true> Cfg;
    if ((a.C * (int)sizeof(T)) % BKB != 0) return hipErrorInvalidValue;
    const int nchunks = a.C * (int)sizeof(T) / BKB;
    const int arows = halo_image_rows(a.H, a.W, Cfg::BP, Cfg::RPI);
    const size_t lds2 = 2 * (size_t)arows * BKB + (size_t)NSB * Cfg::BSTAGE;
    if (nchunks > 1 && lds2 <= 150 * 1024) return halo_launch<T, WP, WC, TP, TC, BKB, NSB, true, ABL>(a, arows, s);
    return halo_launch<T, WP, WC, TP, TC, BKB, NSB, false, ABL>(a, arows, s);
}

#ifdef Y2_DEVBUILD
hipError_t launch_conv_halo_variant(int variant, const ConvArgs& a, hipStream_t s, int* bp, bool run);
#endif

// the tiles plan_conv picks from (halo_tile, below)
template <typename T>
static hipError_t halo_run(int cfg, const ConvArgs& a, hipStream_t s) {
#define HT(WP, WC, TP, TC, BKB, NSB) \
    case conv_tile(WP, WC, TP, TC, BKB, NSB): return halo_pick<T, WP, WC, TP, TC, BKB, NSB>(a, s);
    switch (cfg) {
        HT(4, 2, 3, 1, 128, 2)
        HT(4, 2, 3, 2, 128, 2)
        HT(4, 2, 3, 2, 64, 2)
        HT(4, 2, 2, 2, 64, 2)
        HT(2, 2, 2, 2, 64, 2)
        HT(4, 1, 2, 2, 128, 3)
        HT(4, 1, 2, 2, 64, 3)
        HT(4, 1, 2, 1, 128, 3)
        HT(4, 1, 2, 1, 64, 3)
    }
#undef HT
    return hipErrorInvalidValue;
}

hipError_t launch_conv_halo(int dtype, const ConvPlan& p, const ConvArgs& a, hipStream_t s) {
    if (a.taps != 9 || p.kind != CK_HALO) return hipErrorInvalidValue;
#ifdef Y2_DEVBUILD
    if (p.cfg < conv_tile(0, 0, 0, 0, 64, 0)) return dtype == 1 ? launch_conv_halo_variant(p.cfg, a, s, nullptr, true) : hipErrorInvalidValue;
#endif
    switch (dtype) {
        case 0: return halo_run<float>(p.cfg, a, s);
        case 1: return halo_run<half_t>(p.cfg, a, s);
        case 2: return halo_run<bf16_t>(p.cfg, a, s);
    }
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------
// Kernel policy of the convolution launches (forward and dgrad): plan_conv (below) decides the kernel family, its tile, the filter
// pack the kernel reads, the K split of small launches and the BN record size -- host arithmetic only.  The bind-time
// filter pack (net.hip), the dgrad's BN-backward fuse decision, the inference-fold eligibility and launch_conv all read
// the same answer, and launch_conv refuses filters packed in another layout than the plan's.
//
// Measured on MI355X (scripts/bench_conv.py and profile_layers.py):
//   3x3, rows <= 52 / 104 / the 208-wide 32-channel dgrad : conv_haloq (halo image + register filters)
//   3x3, what conv_haloq's K-chunk sizes do not divide     : conv_halo  (halo image + LDS filter ring)
//   3x3 208-wide forward, and every 1x1                    : conv_igemm (per-tap staging)
//   the 208-wide 32 <-> 64 and the 128-cout 104-wide layers (16-bit) : conv_rf (filters resident in registers)
// ---------------------------------------------------------------------------
constexpr int kLdsMax = 160 * 1024;

int halo_image_rows(int H, int W, int BP, int RPI, int pool) {
    const int pitch = W + 1;
    if (pool) {     // a run of BP / 4 windows touches at most ceil((Wo - 1 + BP / 4) / Wo) row pairs
        const int Wo = W / 2, Ho = H / 2, nwin = BP / 4;
        const int pairs = (nwin + 2 * Wo - 2) / Wo;
        const int img_cross = (nwin - 1) / (Ho * Wo) + 1;
        const int nrows = 2 * pairs * pitch + img_cross * pitch + 2 * (pitch + 1) + 1;
        return (nrows + RPI - 1) / RPI * RPI;
    }
    const int rows_cross = (BP - 1) / W + 1;
    const int img_cross = (BP - 1) / (H * W) + 1;
    const int span = (BP - 1) + rows_cross + img_cross * pitch;
    const int nrows = span + 2 * (pitch + 1) + 1;
    return (nrows + RPI - 1) / RPI * RPI;
}
static int image_rows(const ConvTile& t, const ConvArgs& a, int pool) {
    return halo_image_rows(a.H, a.W, t.bp(), 64 / (t.bkb / 16), pool);
}
// bytes of what the kernels store (the epilogue patch): f32 and the fp32-wide split modes 4, f16 / bf16 and dtype 5 2
static int out_size(int dtype) { return (dtype == 0 || dtype == 3 || dtype == 4) ? 4 : 2; }

// ---- conv_rf.hip
// 0: not this form (16-bit launches only: row_bytes = input channels * 2).
//   1: 32 -> 64 on 208-wide maps (forward of the second layer)      8 waves x 32 pixels x 64 couts, one workgroup per CU
//   2: 64 -> 32 on 208-wide maps (its dgrad)                        8 waves x 32 pixels x 32 couts, one workgroup per CU
static int rf_config(int taps, int W, int row_bytes, int Cout, int M) {
    static const bool off = getenv("Y2_NO_CONV_RF") != nullptr;
    if (off || taps != 9 || W <= 104 || W + 2 >= 256 || M < 256 * 1024) return 0;
    if (row_bytes == 64 && Cout > 32 && Cout <= 64) return 1;
    if (row_bytes == 128 && Cout <= 32) return 2;
    return 0;
}
// the tile and LDS of each config (bw: with the fused BN-backward reduce), the template arguments of conv_rf.hip rf_T
struct RfForm { int bp, bc, lds; };
static RfForm rf_form(int cfg, bool bw) {
    switch (cfg) {
        case 1: return {256, 64, rf_lds(2, 32, 2, 8, 1, 32)};
        case 2: return {256, 32, rf_lds(2, 64, 1, 8, 1, 32)};
        case 3: return {128, 128, rfn_lds(2, 64, 2, 4, 2, 4, bw)};
        default: return {64, 128, rfn_lds(2, 64, 1, 4, 2, 6, bw)};      // 4: the development build's six-slot ring
    }
}
// 3: the 128-cout form: forward (with statistics), plain, and dgrad with the fused BN-backward reduce (bw), where its LDS fits
static int rfn_config(int taps, int W, int row_bytes, int Cout, int M, int dgrad, bool bw) {
    static const bool off = getenv("Y2_NO_CONV_RF") != nullptr;
    static const bool nodg = getenv("Y2_NO_CONV_RFN_DGRAD") != nullptr;
    if (off || (dgrad && nodg) || taps != 9 || W <= 52 || W + 2 > 128 || M < 128 * 1024) return 0;
    if (!(row_bytes == 128 && Cout > 64 && Cout <= 128)) return 0;
#ifdef Y2_DEVBUILD
    static const int alt = getenv("Y2DEV_RF_ALT") ? atoi(getenv("Y2DEV_RF_ALT")) : 0;
    const int cfg = alt == 1 ? 4 : 3;
#else
    const int cfg = 3;
#endif
    return rf_form(cfg, bw).lds <= kLdsMax ? cfg : 0;
}

// ---- K split of small launches (conv_haloq_kernel / conv_igemm_kernel <.., KS>): the depth fills ~one round of the chip
static int ks_depth(int wgs, int wgs_max, int nchunks) {
    static const bool off = getenv("Y2_NO_KSPLIT") != nullptr;
    if (off || wgs >= wgs_max || nchunks < 4) return 1;
    int d = 256 / wgs;
    d = d > 8 ? 8 : d;
    d = d > nchunks / 2 ? nchunks / 2 : d;
    return d < 2 ? 1 : d;
}
size_t conv_ks_scratch_floats(int taps, int M, int ldy, int row_bytes) {
    if ((taps != 9 && taps != 1) || M >= 384 * 8 || (row_bytes % 128) != 0 || ldy <= 64) return 0;
    return (size_t)8 * M * ldy;
}
// what the launch can take of the split: the refusals of the K-split form, then the depth its scratch holds
static int ks_clamp(int depth, const ConvArgs& a) {
    if (depth < 2 || !a.ks_scratch || a.bw_psum || a.nonfinite || (a.ldy % 4) != 0) return 1;
    while (depth > 1 && (size_t)depth * a.M * a.ldy > a.ks_floats) --depth;
    return depth < 2 ? 1 : depth;
}

// ---- conv_haloq.hip tiles
constexpr int HQ_384x128_M16 = conv_tile(4, 2, 3, 2, 128, 1), HQ_256x128_M16 = conv_tile(4, 2, 2, 2, 128, 1),
              HQ_384x64 = conv_tile(4, 2, 3, 1, 128, 0), HQ_512x128 = conv_tile(4, 2, 4, 2, 128, 0),
              HQ_256x128 = conv_tile(4, 2, 2, 2, 128, 0), HQ_512x64 = conv_tile(4, 2, 4, 1, 128, 0),
              HQ_256x64 = conv_tile(4, 2, 2, 1, 128, 0);
// Tile choice of conv_haloq on the short-row layers.  Rounds 1-3 tuned the launch policy on the 416x416 batch-64 shapes
// only: 384 x 128 tiles (384 x 64 where fewer than 160 of them exist).  At 224x224 batch 128 (configs[2]) that puts 264
// workgroups of the 14x14 layers on 256 CUs -- two rounds, the second with eight workgroups -- and 136 / 272 on the
// 7x7 ones: those layers ran at 0.5-0.6 PFLOP/s against 1.0-1.1 for their 26x26 / 13x13 siblings
// (profiles/r04_layers_c3_round_start.txt).  Cost model fitted to a sweep of six tile shapes over the six 3x3 shapes
// of configs[2] (scripts/sweep_c3.sh, profiles/r04_sweep_c3_tiles.txt; rms error 7 %):
//     time ~ rounds * BP * BC / (eff(tile) * (1 + (1 - fill)))     rounds = ceil(workgroups / 256), fill = wgs / (rounds * 256)
// (one 8-wave workgroup per CU; a partly filled chip runs each workgroup faster: clocks and L2 share).  The legacy
// choice stays unless the model sees more than 8 % in another tile, so every configs[3] layer keeps its kernel.
static double hq_cost(int M, int Cout, int bp, int bc, double eff) {
    const long n = (long)((M + bp - 1) / bp) * ((Cout + bc - 1) / bc);
    const long r = (n + 255) / 256;
    const double fill = (double)n / (double)(r * 256);
    return (double)r * bp * bc / (eff * (2.0 - fill));
}
// 0: not this class (W <= 52, more than 64 couts, 128-byte K chunks, 3072 pixels and more).  The 52-wide layers joined
// in round 3 (with the leaner tap step of that round conv_haloq beats conv_halo's LDS filter ring there).
// elem_size 6 = the split-operand mode (fp32 output, but its 16x16-tile kernel runs the epilogue in two passes over
// halves of the wave's couts -- conv_haloq.hip EPI2 -- so the 384 x 128 tile is available; the 512 x 128 one is not);
// the exact-f32 mode takes the two-pass epilogue too (round 5)
static int haloq_tile_choice(int W, int row_bytes, int Cout, int M, int elem_size) {
    if (!(W <= 52 && Cout > 64 && M >= 384 * 8 && (row_bytes % 128) == 0)) return 0;
    const bool narrow = ((M + 383) / 384) * ((Cout + 127) / 128) < 160;
    const bool split = elem_size == 6 || elem_size == 4;
    const int legacy = narrow ? HQ_384x64 : HQ_384x128_M16;
    struct Cand { int id, bp, bc; double eff; bool split_ok; };
    static const Cand cand[] = {{HQ_384x128_M16, 384, 128, 1.00, true}, {HQ_256x128_M16, 256, 128, 0.95, true},
                                {HQ_384x64, 384, 64, 0.80, true},        {HQ_512x128, 512, 128, 1.02, false},
                                {HQ_256x128, 256, 128, 0.92, true},      {HQ_512x64, 512, 64, 0.90, true},
                                {HQ_256x64, 256, 64, 0.74, true}};
    double lc = 0.0, bc = 0.0;
    int best = legacy;
    for (const Cand& c : cand)
        if (c.id == legacy) lc = bc = hq_cost(M, Cout, c.bp, c.bc, c.eff);
    for (const Cand& c : cand) {
        if (split ? !c.split_ok : c.id == HQ_256x128_M16) continue;
        const double v = hq_cost(M, Cout, c.bp, c.bc, c.eff);
        if (v < bc) { bc = v; best = c.id; }
    }
    return bc < 0.92 * lc ? best : legacy;
}
// LDS of the single-buffered image and of the epilogue patch (16x16 tiles with fp32 outputs: two passes over halves of the
// couts where the whole patch does not fit, conv_haloq16_kernel EPI2)
static bool haloq_fits(int tile, const ConvArgs& a, int ysz) {
    const ConvTile t(tile);
    const bool epi2 = ysz == 4 && t.aux && t.tc % 2 == 0 && epi_lds(4, t.wp, t.wc, t.tp, t.tc) > kLdsMax;
    const int epi = epi_lds(ysz, t.wp, t.wc, t.tp, epi2 ? t.tc / 2 : t.tc);
    return (size_t)image_rows(t, a, a.aff_pool) * t.bkb <= (size_t)kLdsMax && epi <= kLdsMax;
}
static int haloq_tile(int dtype, const ConvArgs& a, int kb) {
    const bool k128 = (kb % 128) == 0, split = dtype_split(dtype);
    const int ysz = out_size(dtype), bkb = k128 ? 128 : 64;
    if (a.W > 52) {
        // long rows (104, 208): 512-pixel tiles amortise the two-row halo; one K-chunk per tile where it fits.
        // (split-operand forward, round 6: the fp32 epilogue patch sizes the LDS either way, so the two-plane form takes
        //  128-byte chunks -- 32 channels of both planes, half the tap steps of the 64-byte form; the hi-plane dgrads of
        //  f16x2f keep the 64-byte chunks: one 128-byte chunk is their whole K -- no second image to load behind the
        //  first -- and measured 216 against 200 us)
        // (64-byte K chunks on the 64-cout tiles, so that the 512-pixel image at W = 104 can be double-buffered, measured
        //  12 % SLOWER than the single-buffered 128-byte ones: half the MFMAs per tap step for the same step overhead)
        const int t = a.Cout > 64 ? conv_tile(4, 2, 2, 2, dtype == 3 && k128 ? 128 : 64, 0)
                                  : (a.Cout > 32 ? conv_tile(4, 2, 4, 1, bkb, 0) : conv_tile(8, 1, 2, 1, bkb, 0));
        if (haloq_fits(t, a, ysz)) return t;
    }
    if (a.Cout > 64) {
        // the tile (and with it the filter pack: 16-row fragments for the 16x16 tiles, 32-row ones otherwise) is decided
        // here for bind and launch time alike.  (Round 2 fell through to a 32x32-tile kernel on the 16-row pack in the f32
        // mode -- wrong outputs from batch 24 up at 416x416.)
        const int t = haloq_tile_choice(a.W, kb, a.Cout, a.M, split ? 6 : ysz);
        if (t) return t;
        // Fewer than 3072 pixels (the reference's own training shape, 224x224 at batch 24: 1176 on the 7x7 maps; single
        // images: 49): the launch is a stream of the FILTERS through a few workgroups, each bound by its serial K loop
        // (~110 ns per tap step: 72 us for K = 9216 whatever the tile).  64-cout tiles double the workgroups of the 128 x 128
        // form of rounds 1-3 on the same fragment pack: 7x7 1024 -> 1024 at batch 24 148 -> 81 us, one image 147 -> 72
        // (profiles/r04_sweep_small_m.txt; 128 x 64, 256 x 32 and 256 x 64 tie -- what is left there is a K split)
        if (k128 && a.M < 384 * 8) return HQ_256x64;
        // what the cost model does not cover (64-byte K chunks; long rows that did not fit above)
        const int big = a.M >= 384 * 8 ? conv_tile(4, 2, 3, 2, bkb, 0) : (a.M >= 256 * 8 ? conv_tile(4, 2, 2, 2, bkb, 0) : 0);
        if (big && haloq_fits(big, a, ysz)) return big;
        return conv_tile(2, 2, 2, 2, 64, 0);
    }
    return a.Cout > 32 ? conv_tile(4, 1, 2, 2, bkb, 0) : conv_tile(4, 1, 2, 1, bkb, 0);
}

// ---- conv_halo.hip tiles (16-bit and f32 launches of the 3x3 layers up to 52 wide that conv_haloq does not take)
static bool halo_fits(int tile, const ConvArgs& a, int sz) {
    const ConvTile t(tile);
    const size_t lds = (size_t)image_rows(t, a, 0) * t.bkb + (size_t)t.aux * t.bc() * t.bkb;
    return lds <= (size_t)kLdsMax && epi_lds(sz, t.wp, t.wc, t.tp, t.tc) <= kLdsMax;
}
static int halo_tile(int dtype, const ConvArgs& a, int kb) {
    const bool k128 = (kb % 128) == 0;
    const int bkb = k128 ? 128 : 64;
    if (a.Cout > 64) {
        // measured on the Darknet-19 shapes (scripts/bench_conv.py): big pixel tiles (the filter ring is re-streamed
        // once per pixel tile) with 8 waves; 128 x 128 where LDS runs out
        int t = 0;
        if (a.W <= 13 && a.M >= 384 * 8) {
            // 384 x 128 tiles would leave half the CUs idle when Cout <= 512 (the 1024 -> 512 dgrads at 13x13: 116
            // blocks); 384 x 64 tiles fill them (232 blocks, 184 -> 133 us)
            const bool narrow = ((a.M + 383) / 384) * ((a.Cout + 127) / 128) < 160 && k128;
            t = narrow ? conv_tile(4, 2, 3, 1, 128, 2) : conv_tile(4, 2, 3, 2, bkb, 2);
        } else if (a.M >= 256 * 8) {
            t = conv_tile(4, 2, 2, 2, 64, 2);
        }
        if (t && halo_fits(t, a, (int)dtype_size(dtype))) return t;
        return conv_tile(2, 2, 2, 2, 64, 2);
    }
    return a.Cout > 32 ? conv_tile(4, 1, 2, 2, bkb, 3) : conv_tile(4, 1, 2, 1, bkb, 3);
}

// ---- conv_igemm.hip tiles
static int igemm_tile(int dtype, const ConvArgs& a, int kb) {
    bool k128 = (kb % 128) == 0;
    // round 6: a two-plane (PL2) chunk of 128 bytes is [64 B hi | 64 B lo] = 32 channels of BOTH planes, so the 32-channel
    // layer of the split-operand forward (208x208 32 -> 64) takes ONE K step per tap instead of two of half the depth -- half
    // the barriers and stage waits per matrix instruction
    static const bool no_pl2 = getenv("Y2_NO_CONV_PL2") != nullptr;
    if (dtype == 3 && !no_pl2 && kb == 64) k128 = true;
    const int bkb = k128 ? 128 : 64;
    // 2 LDS stages and two blocks per CU beat deeper rings here (global->LDS fill rate, not latency, bounds this kernel);
    // 8 waves of 64x32 beat 4 waves of 64x64 by ~5-8 %
    if (a.Cout > 64) {
        // round 6: launches of at most one workgroup per CU have nobody to hide a stage's latency behind -- a ring of three
        // stages keeps two K steps in flight (LDS is free at one workgroup per CU).  Same box, alternating: the ResNet swap's
        // step 9.90 / 10.00 -> 9.66 / 9.82 ms (its 14x14 / 7x7 units and the 28x28 ones with 128 couts), configs[2] 4.47 -> 4.45;
        // four stages 9.89 / 9.83.  No configs[3] launch has so few workgroups.
        constexpr long kCUs = 256;     // the MI355X's CU count, as measured (not the device's own count on other parts)
        const long wgs = (long)((a.M + 127) / 128) * ((a.Cout + 127) / 128);
        return conv_tile(2, 4, 2, 1, bkb, !dtype_split(dtype) && k128 && wgs <= kCUs ? 3 : 2);
    }
    return a.Cout > 32 ? conv_tile(4, 1, 2, 2, bkb, 2) : conv_tile(4, 1, 2, 1, bkb, 2);
}

#ifdef Y2_DEVBUILD
// development library only (make dev): Y2DEV_CONV="W:Cout:variant,..." forces a halo variant for (W, Cout), f16
static int dev_rule(int W, int Cout) {
    static int n = -1;
    static int rules[32][3];
    if (n < 0) {
        n = 0;
        const char* e = getenv("Y2DEV_CONV");
        while (e && *e && n < 32) {
            int w, c, v, used = 0;
            if (sscanf(e, "%d:%d:%d%n", &w, &c, &v, &used) != 3) break;
            rules[n][0] = w; rules[n][1] = c; rules[n][2] = v; ++n;
            e += used;
            if (*e == ',') ++e;
        }
    }
    for (int i = 0; i < n; ++i)
        if (rules[i][0] == W && rules[i][1] == Cout) return rules[i][2];
    return -1;
}
#endif

static ConvPlan plan_route(int dtype, const ConvArgs& a) {
    ConvPlan p{CK_IGEMM, 0, 0, 0, 1};
    const int kb = a.C * dtype_kbytes(dtype);       // bytes of one operand plane per pixel: what the K chunks divide
    const bool split = dtype_split(dtype);
    const int rf = rf_config(a.taps, a.W, kb, a.Cout, a.M);
    const int rfn = rfn_config(a.taps, a.W, kb, a.Cout, a.M, a.is_dgrad, a.bw_psum != nullptr);
    if ((dtype == 1 || dtype == 2) && ((!a.bw_psum && rf) || rfn)) {
        p.kind = rf && !a.bw_psum ? CK_RF : CK_RFN;
        p.cfg = p.kind == CK_RF ? rf : rfn;
        // the persistent grid: two workgroups per CU where the LDS allows, whole tiles per workgroup, one record each
        const RfForm f = rf_form(p.cfg, a.bw_psum != nullptr);
        const int ntiles = (int)(((long)a.N * (a.H + 1) * (a.W + 1) + f.bp - 1) / f.bp);
        const int nblk = std::min((f.lds <= 80 * 1024 ? 512 : 256) / ((a.Cout + f.bc - 1) / f.bc), ntiles);
        p.rf_tiles = (ntiles + nblk - 1) / nblk;
        p.records = (ntiles + p.rf_tiles - 1) / p.rf_tiles;
        p.block_pixels = f.bp;
        p.lds = f.lds;
        return p;
    }
    // conv_haloq: 3x3 up to 104 wide and the 208-wide 32-cout dgrad, where the register-filter form does not apply (not
    // in the split-operand mode: three filter planes per product do not fit the register file; those shapes run here).
    // Measured (scripts/bench_conv.py, rotating buffers; round 3: scripts/ab_layers.sh): wins up to 52x52 and again at
    // 104x104 (big 512-pixel tiles); at 208x208 only the 32-channel dgrad gains.
    if (a.taps == 9 && !(!split && (rf || rfn)) && (a.W <= 104 || a.Cout <= 32)) {
        p.kind = CK_HALOQ;
        p.cfg = haloq_tile(dtype, a, kb);
        p.filter_layout = ConvTile(p.cfg).aux ? 2 : 1;
        p.block_pixels = ConvTile(p.cfg).bp();
        if (p.cfg == HQ_256x64 && !split && a.M < 384 * 8) {
            const int depth = ks_clamp(ks_depth(((a.M + 255) / 256) * ((a.Cout + 63) / 64), 128, kb / 128), a);
            // the split image (not double-buffered by the launcher when it does not fit) must fit LDS
            if (depth >= 2 && (size_t)image_rows(ConvTile(p.cfg), a, 0) * 128 <= (size_t)kLdsMax) {
                p.kind = CK_HALOQ_KS;
                p.ks_depth = depth;
                p.block_pixels = 128;     // records of conv_ks_stats_kernel
            }
        }
        return p;
    }
#ifdef Y2_DEVBUILD
    if (a.taps == 9 && dtype == 1 && dev_rule(a.W, a.Cout) >= 0) {
        p.kind = CK_HALO;
        p.cfg = dev_rule(a.W, a.Cout);
        (void)launch_conv_halo_variant(p.cfg, a, 0, &p.block_pixels, false);      // only *bp: the launch refuses an unknown variant
        return p;
    }
#endif
    if (a.taps == 9 && a.W <= 52 && !split) {
        p.kind = CK_HALO;
        p.cfg = halo_tile(dtype, a, kb);
        p.block_pixels = ConvTile(p.cfg).bp();
        return p;
    }
    p.cfg = igemm_tile(dtype, a, kb);
    p.block_pixels = ConvTile(p.cfg).bp();
    // small 1x1 launches: K split over workgroups below 48 workgroups of the 128 x 128 tile (single images, the
    // reference's batch 24 at 7x7: 40).  (Measured: at 52 .. 208 workgroups -- the ResNet swap's 7x7 units at batch 32 --
    // the split is neutral to slightly negative: its partial tiles and the two extra launches cost what the shorter K
    // loops save; configs[0] gains 2.5 %.)  Its BN records cover 128 pixels, as the 128-cout tiles' do.
    if (a.taps == 1 && dtype <= 2 && a.M < 384 * 8 && kb % 128 == 0 && a.Cout > 64) {
        const int depth = ks_clamp(ks_depth(((a.M + 127) / 128) * ((a.Cout + 127) / 128), 48, kb / 128), a);
        if (depth >= 2) {
            p.kind = CK_IGEMM_KS;
            p.cfg = conv_tile(2, 4, 2, 1, 128, 2);
            p.ks_depth = depth;
        }
    }
    return p;
}
ConvPlan plan_conv(int dtype, const ConvArgs& a) {
    ConvPlan p = plan_route(dtype, a);
    if (p.kind != CK_RF && p.kind != CK_RFN) p.records = (a.M + p.block_pixels - 1) / p.block_pixels;
    return p;
}

// ---- the launch log (kernels.h): a host vector behind a mutex, touched only while the log is on
std::atomic<bool> g_launch_log_on{false};
static std::mutex g_launch_log_mu;
static std::vector<int> g_launch_log;
constexpr size_t kLaunchLogMaxRecords = (size_t)1 << 20;
void launch_log_append(int op, int dtype, int f2, int f3, int f4, int f5, int f6) {
    std::lock_guard<std::mutex> lock(g_launch_log_mu);
    if (g_launch_log.size() >= kLaunchLogMaxRecords * Y2_LAUNCH_LOG_INTS) return;
    const int rec[Y2_LAUNCH_LOG_INTS] = {op, dtype, f2, f3, f4, f5, f6};
    g_launch_log.insert(g_launch_log.end(), rec, rec + Y2_LAUNCH_LOG_INTS);
}
void launch_log_enable(bool on) {
    std::lock_guard<std::mutex> lock(g_launch_log_mu);
    if (on) g_launch_log.clear();
    g_launch_log_on.store(on, std::memory_order_relaxed);
}
int launch_log_read(int* out, int max_records) {
    std::lock_guard<std::mutex> lock(g_launch_log_mu);
    const size_t n = g_launch_log.size() / Y2_LAUNCH_LOG_INTS;
    const size_t c = std::min(n, (size_t)std::max(max_records, 0));
    if (out && c) memcpy(out, g_launch_log.data(), c * Y2_LAUNCH_LOG_INTS * sizeof(int));
    return (int)n;
}

hipError_t launch_conv(int dtype, const ConvArgs& a0, hipStream_t s, int filter_layout) {
    // XCD-aware workgroup order: measured +1..4 % on every 3x3 layer up to 104x104 (common.h xcd_block)
    static const int xcd_mode = getenv("Y2_XCD_CONV") ? atoi(getenv("Y2_XCD_CONV")) : 1;
    ConvArgs a = a0;
    a.xcd = xcd_mode;
    const ConvPlan p = plan_conv(dtype, a);
    if (filter_layout != p.filter_layout) return hipErrorInvalidValue;     // the filters were packed for another kernel
    if (g_launch_log_on.load(std::memory_order_relaxed))
        launch_log_append(0, dtype, a.is_dgrad, (int)p.kind, p.cfg, p.ks_depth > 1, a.bw_psum ? 2 : (a.part_mean ? 1 : 0));
    switch (p.kind) {
        case CK_RF: case CK_RFN: return launch_conv_rf(dtype, p, a, s);
        case CK_HALOQ: case CK_HALOQ_KS: return launch_conv_haloq(dtype, p, a, s);
        case CK_HALO: return launch_conv_halo(dtype, p, a, s);
        default: return launch_conv_igemm(dtype, p, a, s);
    }
}

#ifdef Y2_DEVBUILD
// development variants (f16) for scripts/bench_conv.py
// (run = false: only *bp, for plan_conv's Y2DEV_CONV rule)
#define HV(id, WP, TPARGS...) \
    case id: if (bp) *bp = halo_bp<WP, TPARGS>(); return run ? halo_pick<T, WP, TPARGS>(a, s) : hipSuccess;
template <int WP, int WC, int TP, int TC, int BKB, int NSB, int ABL = 0>
static constexpr int halo_bp() { return WP * TP * 32; }
hipError_t launch_conv_halo_variant(int variant, const ConvArgs& a, hipStream_t s, int* bp, bool run) {
    typedef half_t T;
    switch (variant) {
        HV(86, 4, 2, 4, 1, 64, 2)       // 512 x 64, 8 waves, 64-byte chunks
        HV(87, 4, 2, 3, 1, 64, 2)       // 384 x 64
        HV(88, 4, 2, 2, 1, 64, 2)       // 256 x 64
        HV(89, 4, 1, 4, 1, 128, 2)      // 512 x 32, 4 waves
        HV(90, 8, 1, 2, 1, 128, 2)      // 512 x 32, 8 waves
        HV(91, 8, 1, 4, 1, 128, 2)      // 1024 x 32, 8 waves
        HV(92, 8, 1, 2, 1, 64, 2)
        HV(93, 8, 1, 4, 1, 64, 2)
        HV(94, 4, 2, 4, 2, 128, 2)      // 512 x 128, 128-byte chunks
        HV(95, 8, 1, 2, 2, 128, 2)      // 512 x 64, 8 waves of 64x64
        HV(96, 8, 1, 2, 2, 64, 2)
        HV(20, 2, 2, 2, 2, 128, 3)
        HV(21, 2, 2, 2, 2, 128, 2)
        HV(22, 2, 4, 2, 1, 128, 3)
        HV(23, 2, 4, 2, 1, 128, 2)
        HV(24, 4, 2, 2, 2, 128, 3)
        HV(25, 2, 4, 2, 2, 128, 3)
        HV(26, 2, 4, 2, 2, 128, 2)
        HV(27, 2, 2, 2, 2, 128, 4)
        HV(28, 2, 2, 2, 2, 64, 3)
        HV(29, 2, 2, 2, 2, 64, 2)
        HV(40, 2, 2, 2, 2, 64, 4)
        HV(41, 2, 4, 2, 1, 64, 3)
        HV(42, 4, 1, 1, 4, 128, 2)   // wave = 32 px x 128 co
        HV(43, 1, 4, 4, 1, 128, 2)   // wave = 128 px x 32 co
        // ablations of variant 29 (128x128, 64-byte chunks, NSB 2: the product choice)
        HV(50, 2, 2, 2, 2, 64, 2, 3)    // no loads
        HV(51, 2, 2, 2, 2, 64, 2, 4)    // no MFMA
        HV(52, 2, 2, 2, 2, 64, 2, 8)    // no LDS reads
        HV(53, 2, 2, 2, 2, 64, 2, 11)   // MFMA only
        HV(54, 2, 2, 2, 2, 64, 2, 12)   // loads only
        HV(55, 2, 2, 2, 2, 64, 2, 16)   // no epilogue
        HV(56, 2, 2, 2, 2, 64, 2, 2)    // no B loads
        HV(57, 2, 2, 3, 2, 64, 2)       // 192 x 128 tile
        HV(58, 2, 2, 4, 2, 64, 2)       // 256 x 128 tile, 4 waves
        HV(59, 2, 2, 2, 4, 64, 2)       // 128 x 256 tile, 4 waves
        HV(60, 4, 2, 3, 2, 64, 3)       // 384 x 128, 8 waves
        HV(61, 4, 2, 3, 2, 64, 2)
        HV(62, 4, 2, 2, 2, 64, 3)       // 256 x 128, 8 waves
        HV(63, 4, 2, 2, 2, 64, 2)
        HV(64, 4, 2, 4, 2, 64, 2)       // 512 x 128, 8 waves
        HV(65, 4, 2, 3, 2, 128, 2)      // 384 x 128, 128-byte chunks
        HV(80, 4, 1, 2, 2, 128, 2)      // 256 x 64, 4 waves
        HV(81, 2, 2, 2, 1, 128, 2)      // 128 x 64, 4 waves
        HV(82, 4, 2, 2, 1, 128, 2)      // 256 x 64, 8 waves
        HV(83, 4, 2, 3, 1, 128, 2)      // 384 x 64, 8 waves
        HV(84, 4, 1, 3, 2, 128, 2)      // 384 x 64, 4 waves
        HV(85, 4, 2, 4, 1, 128, 2)      // 512 x 64, 8 waves
        HV(76, 4, 2, 3, 2, 128, 2, 32)  // v65 + setprio
        HV(77, 4, 2, 2, 2, 64, 2, 32)   // v63 + setprio
        HV(70, 4, 2, 3, 2, 128, 2, 3)   // v65 without loads
        HV(71, 4, 2, 3, 2, 128, 2, 4)   // v65 without MFMA
        HV(72, 4, 2, 3, 2, 128, 2, 2)   // v65 without filter loads
        HV(73, 4, 2, 3, 2, 128, 2, 1)   // v65 without image loads
        HV(74, 4, 2, 3, 2, 128, 2, 16)  // v65 without epilogue
        HV(75, 4, 2, 3, 2, 128, 2, 8)   // v65 without LDS reads
        HV(66, 2, 4, 3, 1, 64, 2)       // 192 x 128, 8 waves of 96x32
        HV(67, 4, 2, 1, 2, 64, 2)       // 128 x 128, 8 waves of 32x64
        // ablations of variant 24 (256x128, 8 waves, NSB 3)
        HV(30, 4, 2, 2, 2, 128, 3, 3)    // no loads
        HV(31, 4, 2, 2, 2, 128, 3, 4)    // no MFMA
        HV(32, 4, 2, 2, 2, 128, 3, 8)    // no LDS reads
        HV(33, 4, 2, 2, 2, 128, 3, 16)   // no epilogue
        HV(34, 4, 2, 2, 2, 128, 3, 11)   // MFMA only
        HV(35, 4, 2, 2, 2, 128, 3, 27)   // MFMA only, no epilogue
        HV(36, 4, 2, 2, 2, 128, 3, 12)   // loads only
        HV(37, 4, 2, 2, 2, 128, 3, 1)    // no A loads
        HV(38, 4, 2, 2, 2, 128, 3, 2)    // no B loads
    }
    return hipErrorInvalidValue;
}
#endif  // Y2_DEVBUILD

}  // namespace y2
