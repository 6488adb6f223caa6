// The wide head: a 1x1 convolution whose output row is wider than the executor's 2,048 columns (YOLO9000's last layer,
// 1024 -> 28,269), as an operator of its own behind the head stack.  This file is its forward; wide_head_train.hip trains it.
//
//   out[m][c] = bias[c] + sum_k f16(x[m][k]) * f16(W[k][c])        fp32 accumulate on v_mfma_f32_32x32x16_f16
//
//   x      : fp32 [M][K], what y2_forward writes for the stack in front of it; converted to f16 inside the kernel
//            (global -> registers -> v_cvt_pk -> LDS), no convert pass and no f16 copy of the activations
//   packed : f16 [Cp][Kp], Cp = Cout rounded up to the 256-column tile, Kp = K rounded up to the 64-element K step, the
//            padding zero (y2_wide_head_pack): a filter's K range is contiguous, so a staged row is one 128-byte read by
//            global_load_lds and the operand loads need no mask
//   out    : fp32 [M][Cout], row stride Cout exactly (the word-tree head and the detect entries read packed rows); Cout is
//            odd in the model this is for, so a row is 4-byte aligned only and every store is one dword per lane
//
// GEMM view: D[m][c] += X[m][k] Wp[c][k].  The accumulator tile keeps the COLUMN on the lane (C/D layout of common.h: col =
// lane & 31) and the row in the register, so one accumulator register of a wave is two runs of 32 consecutive floats of two
// output rows: 128-byte store segments without an LDS round trip.
// Workgroup: 512 threads = 2 x 4 waves, each 128 rows x 64 columns (4 x 2 MFMA tiles, 128 accumulator registers); tile 256
// x 256; K step 64.  The tile is this large because x is read as fp32: per K step a workgroup loads 64 KiB of x and 32 KiB
// of filters for 2 * 256 * 256 * 64 FLOP; at 128 x 128 the same bytes feed a quarter of the FLOP and the loads, not the
// matrix pipe, bound the launch ("The wide head").  A 32-row MFMA tile that lies wholly behind row M is
// skipped (wave-uniform): at M = 289 the second row tile holds 33 rows.
// LDS: two stages of [256 x rows | 256 filter rows] x 128 bytes = 128 KiB, XOR-swizzled in 16-byte chunks on both sides
// (the filter rows on the per-lane SOURCE address of global_load_lds, the x rows on the ds_write address), so the
// ds_read_b128 fragment reads are conflict-free as in conv_igemm.hip.  One barrier per K step: the loads of step k + 1 are
// issued behind it, the MFMAs of step k run under them, the converted x rows of step k + 1 are written after the MFMAs.
// Grid order: the row tiles of one 256-filter panel are consecutive logical workgroups, and xcd_block() gives each XCD one
// contiguous run of the logical grid, so a panel's row tiles meet in one L2 and the filters cross HBM once.
#include <stdio.h>
#include <stdarg.h>
#include "common.h"
#include "../../include/yolo2_hip.h"

namespace y2 {
int set_error(int code, const char* msg);   // net.hip (y2_last_error)

namespace {

constexpr int kWhBM = 256, kWhBN = 256, kWhBK = 64;          // tile rows, tile columns, K elements per step
constexpr int kWhNT = 512;                                   // threads: 2 (rows) x 4 (columns) waves
constexpr int kWhRowB = kWhBK * 2;                           // bytes of a staged row: 128
constexpr int kWhStage = (kWhBM + kWhBN) * kWhRowB;          // 64 KiB
constexpr int kWhLds = 2 * kWhStage;
constexpr int kWhXPasses = kWhBM * kWhBK / 4 / kWhNT;        // float4 loads per thread and K step: 8
constexpr int kWhWInstr = kWhBN * kWhRowB / 1024 / (kWhNT / 64);   // global_load_lds instructions per wave and K step: 4
constexpr int kWhTM = 4, kWhTN = 2;                          // MFMA tiles of a wave: 4 x 32 rows, 2 x 32 columns

// 16-byte chunk `c` of staged row `r` stands at chunk position c ^ swz(r): two 128-byte rows share a 256-byte bank row
Y2_DEV int wh_swz(int r) { return (r >> 1) & 7; }

__global__ __launch_bounds__(kWhNT) void wide_head_forward_kernel(const float* __restrict__ x, const char* __restrict__ packed,
                                                                  const float* __restrict__ bias, float* __restrict__ out,
                                                                  int M, int K, int Cout, int nMT) {
    __shared__ __attribute__((aligned(16))) char smem[kWhLds];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 2, wc = w & 3;
    const int bx = xcd_block(blockIdx.x, gridDim.x, 1);
    const int ct = bx / nMT, mt = bx - ct * nMT;             // the row tiles of a filter panel are neighbours
    const int m0 = mt * kWhBM, n0 = ct * kWhBN;
    const int Kp = (K + kWhBK - 1) / kWhBK * kWhBK;
    const int nK = Kp / kWhBK;
    // 32-row MFMA tiles of this wave that hold a row below M (wave-uniform)
    const int rows_left = M - (m0 + wm * kWhTM * 32);
    const int live = rows_left <= 0 ? 0 : (rows_left >= kWhTM * 32 ? kWhTM : (rows_left + 31) >> 5);

    // ---- x: pass p of a K step loads floats [4 xj, 4 xj + 4) of tile row p * 32 + xr; rows past M read row M - 1 (their
    // results are never stored), the K tail of a K that is no multiple of 64 is zero without a load
    const int xr = tid >> 4, xj = tid & 15;
    const int mlast = M - 1 - m0;                            // >= 0: the grid holds no row tile behind M
    const float* xbase_g = x + (size_t)m0 * K + 4 * xj;
    int xoff[kWhXPasses], xdst[kWhXPasses];
#pragma unroll
    for (int p = 0; p < kWhXPasses; ++p) {
        const int r = p * 32 + xr;
        xoff[p] = (r < mlast ? r : mlast) * K;               // at most 255 * 4096 floats
        xdst[p] = r * kWhRowB + (((xj >> 1) ^ wh_swz(r)) << 4) + ((xj & 1) << 3);
    }
    const bool x_tail_ok = 4 * xj < K - (nK - 1) * kWhBK;    // whether this thread's floats exist in the last K step
    // ---- filters: instruction i of wave w stages rows (w * 4 + i) * 8 + lane / 8, lane % 8 the chunk position
    const char* wbase_g = packed + (size_t)n0 * ((size_t)Kp * 2);
    int woff[kWhWInstr];
#pragma unroll
    for (int i = 0; i < kWhWInstr; ++i) {
        const int r = (w * kWhWInstr + i) * 8 + (lane >> 3);
        woff[i] = r * Kp * 2 + (((lane & 7) ^ wh_swz(r)) << 4);   // at most 255 * 8192 + 127 bytes
    }
    auto stage_w = [&](int kk, int buf) {
        char* lbase = smem + buf * kWhStage + kWhBM * kWhRowB;
#pragma unroll
        for (int i = 0; i < kWhWInstr; ++i) glds16(wbase_g + woff[i] + kk * kWhRowB, lbase + (w * kWhWInstr + i) * 1024);
    };
    f32x4 xv[kWhXPasses];
    auto load_x = [&](int kk) {
        const bool ok = kk + 1 < nK || x_tail_ok;
#pragma unroll
        for (int p = 0; p < kWhXPasses; ++p)
            xv[p] = ok ? *(const f32x4*)(xbase_g + xoff[p] + kk * kWhBK) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto store_x = [&](int buf) {
        char* lbase = smem + buf * kWhStage;
#pragma unroll
        for (int p = 0; p < kWhXPasses; ++p)
            *(u32x2*)(lbase + xdst[p]) = u32x2{pack2<half_t>(xv[p][0], xv[p][1]), pack2<half_t>(xv[p][2], xv[p][3])};
    };

    // ---- fragment read offsets: lane (r32, hh) reads chunk 2 g + hh of row r32 (+ 32 per MFMA tile: the swizzle term of
    // rows 32 apart is the same)
    const int r32 = lane & 31, hh = lane >> 5;
    int foff[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) foff[g] = r32 * kWhRowB + (((2 * g + hh) ^ wh_swz(r32)) << 4);
    const int xbase = wm * kWhTM * 32 * kWhRowB;
    const int wbase = kWhBM * kWhRowB + wc * kWhTN * 32 * kWhRowB;

    f32x16 acc[kWhTM][kWhTN];
#pragma unroll
    for (int i = 0; i < kWhTM; ++i)
#pragma unroll
        for (int j = 0; j < kWhTN; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    stage_w(0, 0);
    load_x(0);
    store_x(0);
    for (int kk = 0; kk < nK; ++kk) {
        const int cur = kk & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's filter rows of step kk have landed
        __syncthreads();                                      // everyone's have, and everyone's x rows; step kk - 1 is read
        const bool more = kk + 1 < nK;
        if (more) {
            stage_w(kk + 1, cur ^ 1);
            load_x(kk + 1);
        }
        const char* lb = smem + cur * kWhStage;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f16x8 fx[kWhTM], fw[kWhTN];
#pragma unroll
            for (int j = 0; j < kWhTN; ++j) fw[j] = *(const f16x8*)(lb + wbase + j * 32 * kWhRowB + foff[g]);
#pragma unroll
            for (int i = 0; i < kWhTM; ++i)
                if (i < live) fx[i] = *(const f16x8*)(lb + xbase + i * 32 * kWhRowB + foff[g]);
#pragma unroll
            for (int i = 0; i < kWhTM; ++i)
                if (i < live) {
#pragma unroll
                    for (int j = 0; j < kWhTN; ++j) mma32(acc[i][j], fx[i], fw[j]);
                }
        }
        if (more) store_x(cur ^ 1);
    }

    // ---- epilogue: bias, the ragged M and Cout tails masked; register q of tile (i, j) is row acc_row(q, hh), column r32
#pragma unroll
    for (int j = 0; j < kWhTN; ++j) {
        const int c = n0 + (wc * kWhTN + j) * 32 + r32;
        if (c >= Cout) continue;
        const float b = bias[c];
#pragma unroll
        for (int i = 0; i < kWhTM; ++i) {
            const int mb = m0 + (wm * kWhTM + i) * 32;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int m = mb + acc_row(q, hh);
                if (m < M) out[(size_t)m * Cout + c] = acc[i][j][q] + b;
            }
        }
    }
}

// W fp32 [K][Cout] -> packed f16 [Cp][Kp] through a 32 x 32 LDS tile: reads run along Cout, writes along K; the padding
// (c >= Cout, k >= K) is written as zero, so the whole image is defined by one launch
__global__ __launch_bounds__(256) void wide_head_pack_kernel(const float* __restrict__ W, half_t* __restrict__ packed, int K,
                                                             int Cout, int Kp) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, c = c0 + tx;
        tile[r][tx] = (k < K && c < Cout) ? W[(size_t)k * Cout + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = ty; r < 32; r += 8) packed[(size_t)(c0 + r) * Kp + k0 + tx] = (half_t)tile[tx][r];
}

int wh_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return set_error(code, buf);
}

int wh_check(const char* me, int K, int Cout) {
    if (K < 32 || K % 32 || K > Y2_WIDE_HEAD_MAX_K)
        return wh_fail(Y2_ERR_ARG, "%s: K = %d: a multiple of 32, at most %d", me, K, Y2_WIDE_HEAD_MAX_K);
    if (Cout < 1 || Cout > Y2_WIDE_HEAD_MAX_COUT)
        return wh_fail(Y2_ERR_ARG, "%s: Cout = %d outside 1..%d", me, Cout, Y2_WIDE_HEAD_MAX_COUT);
    return Y2_OK;
}

size_t wh_cp(int Cout) { return ((size_t)Cout + kWhBN - 1) / kWhBN * kWhBN; }
size_t wh_kp(int K) { return ((size_t)K + kWhBK - 1) / kWhBK * kWhBK; }

}  // namespace
}  // namespace y2

using namespace y2;

#define WHCHK(expr)                                                                            \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return wh_fail(Y2_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

extern "C" {

size_t y2_wide_head_packed_bytes(int K, int Cout) {
    if (K < 32 || K % 32 || K > Y2_WIDE_HEAD_MAX_K || Cout < 1 || Cout > Y2_WIDE_HEAD_MAX_COUT) return 0;
    return wh_cp(Cout) * wh_kp(K) * sizeof(half_t);
}

int y2_wide_head_pack(const float* W, int K, int Cout, void* packed, size_t packed_bytes, void* stream) {
    const char* me = "y2_wide_head_pack";
    if (!W || !packed) return wh_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wh_check(me, K, Cout)) return e;
    const size_t need = y2_wide_head_packed_bytes(K, Cout);
    if (packed_bytes < need)
        return wh_fail(Y2_ERR_ARG, "%s: packed_bytes = %zu, K = %d and Cout = %d need %zu", me, packed_bytes, K, Cout, need);
    if ((uintptr_t)packed % 16) return wh_fail(Y2_ERR_ARG, "%s: packed is not 16-byte aligned", me);
    hipLaunchKernelGGL(wide_head_pack_kernel, dim3((unsigned)(wh_cp(Cout) / 32), (unsigned)(wh_kp(K) / 32)), dim3(256), 0,
                       (hipStream_t)stream, W, (half_t*)packed, K, Cout, (int)wh_kp(K));
    WHCHK(hipGetLastError());
    return Y2_OK;
}

int y2_wide_head_forward(const float* x, const void* packed, const float* bias, int M, int K, int Cout, float* out,
                         void* stream) {
    const char* me = "y2_wide_head_forward";
    if (!x || !packed || !bias || !out) return wh_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wh_check(me, K, Cout)) return e;
    if (M < 1) return wh_fail(Y2_ERR_ARG, "%s: M = %d: at least 1", me, M);
    if ((uintptr_t)x % 16 || (uintptr_t)packed % 16)
        return wh_fail(Y2_ERR_ARG, "%s: x and packed must be 16-byte aligned", me);
    const long long nMT = ((long long)M + kWhBM - 1) / kWhBM, nCT = (long long)(wh_cp(Cout) / kWhBN);
    if (nMT * nCT > 0x7fffffffLL)
        return wh_fail(Y2_ERR_ARG, "%s: M = %d, Cout = %d: %lld tiles are beyond one grid", me, M, Cout, nMT * nCT);
    hipLaunchKernelGGL(wide_head_forward_kernel, dim3((unsigned)(nMT * nCT)), dim3(kWhNT), 0, (hipStream_t)stream, x,
                       (const char*)packed, bias, out, M, K, Cout, (int)nMT);
    WHCHK(hipGetLastError());
    return Y2_OK;
}

}  // extern "C"
