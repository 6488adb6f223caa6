// MXFP8 inference forms (include/yolo2_hip.h Y2_FP8): the block quantiser, the filter pack, and an implicit-GEMM
// stride-1 SAME convolution (3x3 or 1x1) on gfx950's block-scaled matrix pipe, v_mfma_scale_f32_32x32x64_f8f6f4 with
// OCP e4m3fn operands -- twice the f16 MFMA rate per clock.
//
// Number format (OCP MX): e4m3fn elements, one E8M0 scale byte (2^(byte - 127)) per block of 32 values.
//   activations: 32 consecutive channels of one pixel; filters: 32 consecutive input channels of one tap and one output
//   channel (the K axis of the GEMM).  Scale of a block: the smallest e with amax <= 448 * 2^e (exactly: frexp(amax) =
//   m * 2^E, e = E - 9 if m <= 0.875 else E - 8), clamped to [-127, 127]; an all-zero block takes -127.  Elements:
//   RNE_e4m3(min(max(v / 2^e, -448), 448)), e4m3 subnormals kept.
//
// The convolution is conv_igemm.hip's structure (per-tap global_load_lds staging of pixel rows and filter rows, XOR
// swizzle, NS = 2) on bytes: one K step of the MFMA is 64 channels of one tap = two MX blocks; lane half hh supplies the
// scale byte of block hh (its 32 K values are two 16-channel halves, one of each block: see the fragment reads).  The
// scale bytes are read per lane from the scale planes ([pixel][C/32] beside the bordered tensor, [cout][tap][C/32] beside the packed filters), one 16- or
// 32-bit load per operand tile and K step, issued a step ahead.  The epilogue is the f16 / f32 kernels' shared one
// (conv_epilogue.h): the 32x32 accumulator layout does not depend on the operand type.
#include <math.h>
#include "common.h"
#include "conv_epilogue.h"
#include "kernels.h"

namespace y2 {

// ---- the number format (device and host)
__host__ __device__ inline int mx_scale_exp(float amax) {
    if (!(amax > 0.f)) return -127;
    int E;
    const float m = frexpf(amax, &E);
    int e = m <= 0.875f ? E - 9 : E - 8;
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}
// v already divided by the block scale; RNE to e4m3fn (OCP), subnormals kept
__host__ __device__ inline uint32_t mx_e4m3(float v) {
    v = fminf(fmaxf(v, -448.f), 448.f);
    const uint32_t sign = v < 0.f ? 0x80u : 0u;
    const float a = fabsf(v);
    int E;
    (void)frexpf(a, &E);        // a = m * 2^E, m in [0.5, 1): floor(log2 a) = E - 1 (frexp(0) has E = 0: excluded)
    int eb = a > 0.f ? E - 1 : -6;
    if (eb < -6) eb = -6;       // subnormals share the quantum of the smallest binade
    const float q = rintf(ldexpf(a, 3 - eb));       // in [0, 16]: 3 mantissa bits, RNE
    const uint32_t code = (uint32_t)((eb + 6) * 8) + (uint32_t)q;   // q = 16 carries into the next binade
    return sign | code;
}

// ---- standalone quantiser: [rows][ldin] of TI -> elements [rows][ldq] + scales [rows][ldq / 32]; blocks beyond ldin
// (channel padding) are zero with the smallest scale
template <typename TI>
__global__ __launch_bounds__(256) void mx_quant_kernel(const TI* __restrict__ x, size_t rows, int ldin, int ldq,
                                                      uint8_t* __restrict__ q, uint8_t* __restrict__ sc) {
    const int nb = ldq / 32;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * (size_t)nb) return;
    const size_t row = i / nb;
    const int b = (int)(i - row * nb);
    float v[32];
    float amax = 0.f;
    if (b * 32 < ldin) {
        const TI* src = x + row * (size_t)ldin + b * 32;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            v[k] = (float)src[k];
            amax = fmaxf(amax, fabsf(v[k]));
        }
    } else {
#pragma unroll
        for (int k = 0; k < 32; ++k) v[k] = 0.f;
    }
    const int e = mx_scale_exp(amax);
    u32x4 o[2];
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) word |= mx_e4m3(ldexpf(v[4 * w + k], -e)) << (8 * k);
        o[w >> 2][w & 3] = word;
    }
    u32x4* dst = (u32x4*)(q + row * (size_t)ldq + b * 32);
    dst[0] = o[0];
    dst[1] = o[1];
    sc[row * nb + b] = (uint8_t)(e + 127);
}

// ---- filter pack: fp32 HWIO [taps][Cin][Cout] -> e4m3 [Cout_pad][taps][C8] + scales [Cout_pad][taps][C8 / 32]; the
// output channel runs fastest over the threads (coalesced reads of the HWIO rows); padding rows and channels are zero
__global__ __launch_bounds__(256) void mx_pack_filter_kernel(const float* __restrict__ w, int taps, int Cin, int Cout,
                                                            int Cout_pad, int C8, uint8_t* __restrict__ q,
                                                            uint8_t* __restrict__ sc) {
    const int nb = C8 / 32;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Cout_pad * taps * nb) return;
    const int co = (int)(i % Cout_pad);
    const int tb = (int)(i / Cout_pad);
    const int t = tb / nb, b = tb - t * nb;
    float v[32];
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const int ci = b * 32 + k;
        v[k] = (co < Cout && ci < Cin) ? w[((size_t)t * Cin + ci) * Cout + co] : 0.f;
        amax = fmaxf(amax, fabsf(v[k]));
    }
    const int e = mx_scale_exp(amax);
    u32x4 o[2];
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) {
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) word |= mx_e4m3(ldexpf(v[4 * ww + k], -e)) << (8 * k);
        o[ww >> 2][ww & 3] = word;
    }
    const size_t row = (size_t)co * taps + t;
    u32x4* dst = (u32x4*)(q + row * C8 + b * 32);
    dst[0] = o[0];
    dst[1] = o[1];
    sc[row * nb + b] = (uint8_t)(e + 127);
}

// ---- the convolution.  Tile: 2 x 4 waves, 2 pixel tiles x 1 cout tile of 32 x 32 per wave (128 pixels x 128 couts per
// workgroup); BKB bytes (= channels) of one tap per K step: 128 where C % 128 == 0, else 64
typedef int i32x8 __attribute__((ext_vector_type(8)));
constexpr int kMxWP = 2, kMxWC = 4, kMxTP = 2, kMxTC = 1;
// staging geometry (conv_igemm.hip ConvCfg with one-byte elements, two stages)
template <int WP, int WC, int TP, int TC, int BKB>
struct ConvCfg8 {
    static constexpr int NW = WP * WC;
    static constexpr int NT = NW * 64;
    static constexpr int BP = WP * TP * 32;  // pixels per block
    static constexpr int BC = WC * TC * 32;  // output channels per block
    static constexpr int LPR = BKB / 16;     // lanes per staged row
    static constexpr int RPI = 64 / LPR;     // rows per glds wave-instruction
    static constexpr int RPB = 256 / BKB;    // rows per 256-B LDS bank row
    static constexpr int NI_P = BP / RPI;
    static constexpr int NI_C = BC / RPI;
    static constexpr int NI = NI_P + NI_C;
    static constexpr int IPW = (NI + NW - 1) / NW;
    static constexpr int STAGE = (BP + BC) * BKB;
    static constexpr int LDS_MAIN = 2 * STAGE;
    static_assert(NI_P % NW == 0, "pixel rows must split evenly over waves");
    static_assert((32 / RPB) % LPR == 0, "the swizzle term must not depend on the 32-row tile");
};
int mx8_block_couts() { return kMxWC * kMxTC * 32; }

// Q: the MXFP8 epilogue.  Each wave's cout tile is 32 wide -- one MX block of the consumer's channels -- and a lane holds
// 16 of one pixel's 32 couts (the other 16 in lane ^ 32), so the block maximum is one cross-half exchange.  Per value:
// leaky(f16(conv + bias) * scale + shift) (the folded inference batch norm, as conv_epilogue.h stores it in f16), then the
// quantiser above over the 32 couts of the pixel, written into the consumer's bordered e4m3 tensor q [cell][ldq] and its
// scale plane [cell][ldq / 32] (ConvArgs::aff_* give scale, shift, slope and the bordered index).
template <typename YT, int BKB, bool Q>
__global__ __launch_bounds__(kMxWP* kMxWC * 64) void conv_mx8_kernel(ConvArgs a, const uint8_t* __restrict__ xsc,
                                                                     const uint8_t* __restrict__ wsc, Mx8Out qo) {
    constexpr int WP = kMxWP, WC = kMxWC, TP = kMxTP, TC = kMxTC, NS = 2;
    typedef ConvCfg8<WP, WC, TP, TC, BKB> Cfg;
    constexpr int NW = Cfg::NW, BP = Cfg::BP, BC = Cfg::BC;
    constexpr int LPR = Cfg::LPR, RPI = Cfg::RPI, RPB = Cfg::RPB, IPW = Cfg::IPW;
    constexpr int MS = BKB / 64;             // MFMAs (K = 64) per K step
    typedef typename std::conditional<BKB == 128, uint32_t, uint16_t>::type ST;     // the scale bytes of one K step
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = w / WC, wc = w % WC;
    const int nCT = (a.Cout + BC - 1) / BC;
    const int bx = xcd_block(blockIdx.x, gridDim.x, a.xcd);
    const int ct = bx % nCT, pt = bx / nCT;
    const int m0 = pt * BP, n0 = ct * BC;
    const int Ktot = a.taps * a.C;           // bytes per packed filter row
    const int nbk = a.C / 32;                // scale bytes per pixel / per filter tap
    const char* __restrict__ xg = (const char*)a.x;
    const char* __restrict__ wg = (const char*)a.w;
    const int hw = a.H * a.W;
    auto top_left = [&](int p) -> uint32_t {      // bordered index of the 3x3 window's top-left cell of pixel p
        if (p >= a.M) return 0;
        const int n = p / hw, rem = p - n * hw;
        const int h = rem / a.W, ww = rem - h * a.W;
        return (uint32_t)(bpix(n, h, ww, a.H, a.W) - (size_t)(a.W + 2));
    };

    // ---- staging offsets (conv_igemm.hip)
    uint32_t voff[IPW];
    const int lrow = lane / LPR, lslot = lane % LPR;
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
        const int ii = i * NW + w;
        const int row = ii * RPI + lrow;
        if (i * NW < Cfg::NI_P) {
            voff[i] = top_left(m0 + row) * (uint32_t)a.C + (uint32_t)((lslot ^ ((row / RPB) % LPR)) * 16);
        } else {
            const int r = row - BP;
            voff[i] = (uint32_t)(n0 + r) * (uint32_t)Ktot + (uint32_t)((lslot ^ ((r / RPB) % LPR)) * 16);
        }
    }
    const int cpt = a.C / BKB;
    const int nK = a.taps * cpt;
    const int pitch = a.W + 1;
    auto tap_px = [&](int t) -> int {
        if (a.taps == 9) { const int kh = t / 3; return kh * pitch + (t - kh * 3); }
        return pitch + 1;
    };
    auto stage = [&](int kk, int buf) {
        const int t = kk / cpt, c = kk - t * cpt;
        const char* xs = xg + (size_t)tap_px(t) * a.C + c * BKB;
        const char* ws = wg + (size_t)t * a.C + c * BKB;
        char* lbase = smem + buf * Cfg::STAGE;
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
            const int ii = i * NW + w;
            if (i * NW < Cfg::NI_P) glds16(xs + voff[i], lbase + ii * 1024);
            else if ((i + 1) * NW <= Cfg::NI || ii < Cfg::NI) glds16(ws + voff[i], lbase + ii * 1024);
        }
    };

    // ---- this lane's rows: its pixel in each pixel tile, its cout in each cout tile, and their scale-plane offsets
    const int r32 = lane & 31, hh = lane >> 5;
    uint32_t xs_px[TP];
#pragma unroll
    for (int j = 0; j < TP; ++j) xs_px[j] = top_left(m0 + (wp * TP + j) * 32 + r32);
    uint32_t ws_row[TC];
#pragma unroll
    for (int i = 0; i < TC; ++i) ws_row[i] = (uint32_t)(n0 + (wc * TC + i) * 32 + r32) * (uint32_t)a.taps;
    auto load_scales = [&](int kk, ST (&sx)[TP], ST (&sw)[TC]) {
        const int t = kk / cpt, c = kk - t * cpt;
        const int b0 = c * (BKB / 32);
#pragma unroll
        for (int j = 0; j < TP; ++j) sx[j] = *(const ST*)(xsc + (size_t)(xs_px[j] + tap_px(t)) * nbk + b0);
#pragma unroll
        for (int i = 0; i < TC; ++i) sw[i] = *(const ST*)(wsc + (size_t)(ws_row[i] + t) * nbk + b0);
    };
    // fragment reads.  Operand map of the 32x32x64 f8 form (measured with one-hot data and per-half scales): lane half
    // hh holds k = 16 hh .. 16 hh + 15 in bytes 0-15 and k = 32 + 16 hh .. in bytes 16-31, and the scale of K block b
    // (k = 32 b .. 32 b + 31) of row r comes from lane r + 32 b.  So the lane reads 16-byte chunks hh and 2 + hh of each
    // 64-byte MFMA step (swizzled as staged) and supplies the scale of block hh.
    const int swz = (r32 / RPB) % LPR;
    int foff[MS][2];
#pragma unroll
    for (int g = 0; g < MS; ++g)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) foff[g][h2] = r32 * BKB + (((4 * g + 2 * h2 + hh) ^ swz) * 16);
    const int pbase = (wp * TP) * 32 * BKB;
    const int cbase = BP * BKB + (wc * TC) * 32 * BKB;
    auto frag = [&](const char* p, int g) -> i32x8 {
        const u32x4 lo = *(const u32x4*)(p + foff[g][0]);
        const u32x4 hi = *(const u32x4*)(p + foff[g][1]);
        return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    };

    f32x16 acc[TC][TP];
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
        for (int j = 0; j < TP; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    ST sx[TP], sw[TC], nx[TP], nw[TC];
    stage(0, 0);
    load_scales(0, sx, sw);
    int cbuf = 0;
    for (int kk = 0; kk < nK; ++kk) {
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (kk + 1 < nK) {
            stage(kk + 1, cbuf ^ 1);
            load_scales(kk + 1, nx, nw);
        }
        const char* lb = smem + cbuf * Cfg::STAGE;
#pragma unroll
        for (int g = 0; g < MS; ++g) {
            i32x8 fc[TC], fp[TP];
#pragma unroll
            for (int i = 0; i < TC; ++i) fc[i] = frag(lb + cbase + i * 32 * BKB, g);
#pragma unroll
            for (int j = 0; j < TP; ++j) fp[j] = frag(lb + pbase + j * 32 * BKB, g);
            const int sh = 8 * (2 * g + hh);      // this lane's block of the step
#pragma unroll
            for (int i = 0; i < TC; ++i)
#pragma unroll
                for (int j = 0; j < TP; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                        fc[i], fp[j], acc[i][j], 0, 0, 0, (int)(((uint32_t)sw[i] >> sh) & 0xffu), 0,
                        (int)(((uint32_t)sx[j] >> sh) & 0xffu));
        }
        if (kk + 1 < nK) {
#pragma unroll
            for (int j = 0; j < TP; ++j) sx[j] = nx[j];
#pragma unroll
            for (int i = 0; i < TC; ++i) sw[i] = nw[i];
        }
        cbuf ^= 1;
    }
    if constexpr (Q) {
        static_assert(TC == 1, "one MX block of couts per wave");
        const int cb = n0 + wc * 32;                 // first cout of this wave = the block's first channel
        if (cb >= a.ldy) return;                     // wave-uniform
        float sc[16], sh[16], bi[16];
        bool cv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = cb + (r & 3) + 8 * (r >> 2) + 4 * hh;
            cv[r] = co < a.Cout;
            sc[r] = cv[r] ? a.aff_scale[co] : 0.f;
            sh[r] = cv[r] ? a.aff_shift[co] : 0.f;
            bi[r] = (cv[r] && a.bias) ? a.bias[co] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < TP; ++j) {
            float z[16];
            float amax = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float h = (float)(half_t)(acc[0][j][r] + bi[r]);
                z[r] = cv[r] ? leaky_s(h * sc[r] + sh[r], a.aff_slope) : 0.f;
                amax = fmaxf(amax, fabsf(z[r]));
            }
            amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
            const int e = mx_scale_exp(amax);
            const uint32_t m = (uint32_t)(m0 + (wp * TP + j) * 32 + r32);
            if ((int)m >= a.M) continue;
            const uint32_t rr = (uint32_t)(((uint64_t)m * a.aff_magW) >> a.aff_shW);
            const uint32_t n = (uint32_t)(((uint64_t)rr * a.aff_magH) >> a.aff_shH);
            const size_t bp = (size_t)m + rr + (size_t)(n + 1) * (uint32_t)(a.W + 1) + 1;
            uint8_t* dst = qo.q + bp * qo.ldq + cb + 4 * hh;
#pragma unroll
            for (int g = 0; g < 4; ++g) {            // registers 4g .. 4g + 3: couts cb + 8g + 4hh .. + 3
                uint32_t word = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) word |= mx_e4m3(ldexpf(z[4 * g + k], -e)) << (8 * k);
                *(uint32_t*)(dst + 8 * g) = word;
            }
            if (hh == 0) qo.sc[bp * (qo.ldq / 32) + cb / 32] = (uint8_t)(e + 127);
        }
        return;
    }
    __syncthreads();
    conv_epilogue<YT, WP, WC, TP, TC>(a, acc, smem, w, lane, m0, n0, pt, ct);
}

template <typename YT, int BKB, bool Q>
static hipError_t launch_mx8_cfg(const ConvArgs& a, const uint8_t* xsc, const uint8_t* wsc, const Mx8Out& qo,
                                 hipStream_t s) {
    typedef ConvCfg8<kMxWP, kMxWC, kMxTP, kMxTC, BKB> Cfg;
    constexpr int LDS = Cfg::LDS_MAIN > epi_lds(sizeof(YT), kMxWP, kMxWC, kMxTP, kMxTC)
                            ? Cfg::LDS_MAIN : epi_lds(sizeof(YT), kMxWP, kMxWC, kMxTP, kMxTC);
    static_assert(LDS <= 160 * 1024, "LDS budget");
    void (*kern)(ConvArgs, const uint8_t*, const uint8_t*, Mx8Out) = conv_mx8_kernel<YT, BKB, Q>;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    const int nPT = (a.M + Cfg::BP - 1) / Cfg::BP;
    const int nCT = (a.Cout + Cfg::BC - 1) / Cfg::BC;
    hipLaunchKernelGGL(kern, dim3(nPT * nCT), dim3(Cfg::NT), LDS, s, a, xsc, wsc, qo);
    return hipGetLastError();
}

int mx8_channels(int C) { return C % 128 == 0 ? C : (C + 63) / 64 * 64; }

hipError_t launch_conv_mx8(int out_f32, const ConvArgs& a, const uint8_t* xsc, const uint8_t* wsc, const Mx8Out* qo,
                           hipStream_t s) {
    if (a.C % 64 != 0 || a.part_cnt || a.aff_pool || a.is_dgrad || (a.taps != 1 && a.taps != 9)) return hipErrorInvalidValue;
    if (out_f32 && (a.aff_out || qo)) return hipErrorInvalidValue;
    const bool k128 = a.C % 128 == 0;
    if (qo) {   // the MXFP8 epilogue: needs the folded batch norm's constants and bordered-index magic (conv_set_affine)
        if (!a.aff_scale || !a.aff_shift || !qo->q || !qo->sc || qo->ldq % 32 != 0 || qo->ldq < a.ldy) return hipErrorInvalidValue;
        return k128 ? launch_mx8_cfg<half_t, 128, true>(a, xsc, wsc, *qo, s) : launch_mx8_cfg<half_t, 64, true>(a, xsc, wsc, *qo, s);
    }
    const Mx8Out none{};
    if (out_f32) return k128 ? launch_mx8_cfg<float, 128, false>(a, xsc, wsc, none, s) : launch_mx8_cfg<float, 64, false>(a, xsc, wsc, none, s);
    return k128 ? launch_mx8_cfg<half_t, 128, false>(a, xsc, wsc, none, s) : launch_mx8_cfg<half_t, 64, false>(a, xsc, wsc, none, s);
}

// bordered e4m3 [cell][Cs] + scales [cell][Cs / 32] (cell-0 pointers) -> fp32 NHWC [N][H][W][C] (debug reads, tests)
__global__ __launch_bounds__(256) void mx_unpack_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ sc,
                                                       float* __restrict__ out, int N, int H, int W, int C, int Cs) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * H * W * C) return;
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int w = (int)(p % W), h = (int)((p / W) % H), n = (int)(p / ((size_t)W * H));
    const size_t bp = bpix(n, h, w, H, W);
    const uint32_t v = q[bp * Cs + c];
    const int ex = (v >> 3) & 15, mt = v & 7;
    float f = ex ? ldexpf((float)(8 + mt), ex - 10) : ldexpf((float)mt, -9);
    f = ldexpf(f, (int)sc[bp * (Cs / 32) + c / 32] - 127);
    out[i] = (v & 0x80) ? -f : f;
}
hipError_t launch_mx_unpack(const uint8_t* q, const uint8_t* sc, float* out, int N, int H, int W, int C, int Cs,
                            hipStream_t s) {
    const size_t n = (size_t)N * H * W * C;
    hipLaunchKernelGGL(mx_unpack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q, sc, out, N, H, W, C, Cs);
    return hipGetLastError();
}

hipError_t launch_mx_quantize(int in_f16, const void* x, size_t rows, int ldin, int ldq, uint8_t* q, uint8_t* sc,
                              hipStream_t s) {
    if (ldq % 32 != 0 || ldin % 32 != 0 || ldin > ldq) return hipErrorInvalidValue;
    const size_t n = rows * (size_t)(ldq / 32);
    if (n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (in_f16) hipLaunchKernelGGL(mx_quant_kernel<half_t>, dim3(blocks), dim3(256), 0, s, (const half_t*)x, rows, ldin, ldq, q, sc);
    else hipLaunchKernelGGL(mx_quant_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)x, rows, ldin, ldq, q, sc);
    return hipGetLastError();
}

hipError_t launch_mx_pack_filter(const float* w, int taps, int Cin, int Cout, int Cout_pad, int C8, uint8_t* q,
                                 uint8_t* sc, hipStream_t s) {
    if (C8 % 32 != 0 || C8 < Cin || Cout_pad < Cout) return hipErrorInvalidValue;
    const size_t n = (size_t)Cout_pad * taps * (C8 / 32);
    hipLaunchKernelGGL(mx_pack_filter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, taps, Cin, Cout,
                       Cout_pad, C8, q, sc);
    return hipGetLastError();
}

}  // namespace y2
