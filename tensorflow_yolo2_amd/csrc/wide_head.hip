// The wide head: a 1x1 convolution whose output row is wider than the executor's 2,048 columns (YOLO9000's last layer,
// 1024 -> 28,269), as an operator of its own behind the head stack.  This file is its forward; wide_head_train.hip trains it;
// wide_gemm.h is the GEMM both stand on (the staged rows, the swizzle, the main loop, the accumulator layout).
//
//   out[m][c] = bias[c] + sum_k f16(x[m][k]) * f16(W[k][c])        fp32 accumulate on v_mfma_f32_32x32x16_f16
//
//   x      : fp32 [M][K], what y2_forward writes for the stack in front of it; converted to f16 inside the kernel
//   packed : f16 [Cp][Kp], Cp = Cout rounded up to the 256-column tile, Kp = K rounded up to the 64-element K step, the
//            padding zero (y2_wide_head_pack): a filter's K range is contiguous, so a staged row is one 128-byte read by
//            global_load_lds and the operand loads need no mask
//   out    : fp32 [M][Cout], row stride Cout exactly (the word-tree head and the detect entries read packed rows); Cout is
//            odd in the model this is for, so a row is 4-byte aligned only
//
// The kernel is wide_gemm.h at WideFwdTile (256 x 256, 2 x 4 waves of 4 x 2 MFMA tiles) with A = x, B = packed, the whole
// reduction in one workgroup and the bias in the epilogue.  A 32-row MFMA tile that lies wholly behind row M is skipped
// (wave-uniform): at M = 289 the second row tile holds 33 rows.
// Grid order: the row tiles of one 256-filter panel are consecutive logical workgroups, and xcd_block() gives each XCD one
// contiguous run of the logical grid, so a panel's row tiles meet in one L2 and the filters cross HBM once.
#include "wide_gemm.h"

namespace y2 {
namespace {

typedef WideFwdTile T;

__global__ __launch_bounds__(T::kNT) void wide_head_forward_kernel(const float* __restrict__ x, const char* __restrict__ packed,
                                                                   const float* __restrict__ bias, float* __restrict__ out,
                                                                   int M, int K, int Cout, int nMT) {
    __shared__ __attribute__((aligned(16))) char smem[T::kLds];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = xcd_block(blockIdx.x, gridDim.x, 1);
    const int ct = bx / nMT, mt = bx - ct * nMT;             // the row tiles of a filter panel are neighbours
    const int m0 = mt * T::kBM, n0 = ct * T::kBN;
    const int Kp = (K + T::kBK - 1) / T::kBK * T::kBK;
    const int nK = Kp / T::kBK;
    // 32-row MFMA tiles of this wave that hold a row below M (wave-uniform)
    const int rows_left = M - (m0 + w / T::kWN * T::kTM * 32);
    const int live = rows_left <= 0 ? 0 : (rows_left >= T::kTM * 32 ? T::kTM : (rows_left + 31) >> 5);

    // ---- x: aligned float4 rows; rows past M read row M - 1 (their results are never stored), the K tail of a K that is no
    // multiple of 64 is zero without a load.  WideQuads, with the destinations formed here beside the row offsets: taken from
    // wide_quads() this kernel measured slower at M = 289 (profiles/wide_head_refactor.txt section 6)
    WideQuads<T> a;
    a.xr = tid >> 4;
    a.xj = tid & 15;
    const int mlast = M - 1 - m0;                            // >= 0: the grid holds no row tile behind M
    const float* xbase_g = x + (size_t)m0 * K + 4 * a.xj;
    int xoff[T::kPasses];
#pragma unroll
    for (int p = 0; p < T::kPasses; ++p) {
        const int r = p * T::kQuadRows + a.xr;
        xoff[p] = (r < mlast ? r : mlast) * K;               // at most 255 * 4096 floats
        a.dst[p] = r * T::kRowB + (((a.xj >> 1) ^ wide_swz(r)) << 4) + ((a.xj & 1) << 3);
    }
    const bool x_tail_ok = 4 * a.xj < K - (nK - 1) * T::kBK;   // whether this thread's floats exist in the last K step
    const WideRows<T> b = wide_rows<T>(packed + (size_t)n0 * ((size_t)Kp * 2), Kp * 2, lane, w);
    f32x4 xv[T::kPasses];
    auto issue = [&](int kk, int buf) {
        wide_stage_rows<T, int>(b, kk, smem + buf * T::kStage, w);
        const bool ok = kk + 1 < nK || x_tail_ok;
#pragma unroll
        for (int p = 0; p < T::kPasses; ++p)
            xv[p] = ok ? *(const f32x4*)(xbase_g + xoff[p] + kk * T::kBK) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int p = 0; p < T::kPasses; ++p)
            wide_store_quad(smem + buf * T::kStage + a.dst[p], xv[p][0], xv[p][1], xv[p][2], xv[p][3]);
    };

    const WideFrag f = wide_frag<T>(lane, w);
    f32x16 acc[T::kTM][T::kTN];
    wide_zero<T>(acc);
    wide_main_loop<T, true>(acc, smem, f, 0, nK, live, issue, store);
    wide_epilogue<T>(acc, f, m0, n0, M, Cout, [&](int c) {
        const float bc = bias[c];
        return [=](int m, float v) { out[(size_t)m * Cout + c] = v + bc; };
    });
}

// W fp32 [K][Cout] -> packed f16 [Cp][Kp]; the padding (c >= Cout, k >= K) is written as zero, so the whole image is defined
// by one launch
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
    wide_put_image(tile, packed, Kp, c0, k0, tx, ty);
}

}  // namespace
}  // namespace y2

using namespace y2;

extern "C" {

size_t y2_wide_head_packed_bytes(int K, int Cout) {
    if (wide_check(nullptr, K, Cout)) return 0;
    return wide_cp(Cout) * wide_kp(K) * sizeof(half_t);
}

int y2_wide_head_pack(const float* W, int K, int Cout, void* packed, size_t packed_bytes, void* stream) {
    const char* me = "y2_wide_head_pack";
    if (!W || !packed) return wide_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wide_check(me, K, Cout)) return e;
    const size_t need = y2_wide_head_packed_bytes(K, Cout);
    if (packed_bytes < need)
        return wide_fail(Y2_ERR_ARG, "%s: packed_bytes = %zu, K = %d and Cout = %d need %zu", me, packed_bytes, K, Cout, need);
    if ((uintptr_t)packed % 16) return wide_fail(Y2_ERR_ARG, "%s: packed is not 16-byte aligned", me);
    hipLaunchKernelGGL(wide_head_pack_kernel, dim3((unsigned)(wide_cp(Cout) / 32), (unsigned)(wide_kp(K) / 32)), dim3(256), 0,
                       (hipStream_t)stream, W, (half_t*)packed, K, Cout, (int)wide_kp(K));
    WIDE_CHK(hipGetLastError());
    return Y2_OK;
}

int y2_wide_head_forward(const float* x, const void* packed, const float* bias, int M, int K, int Cout, float* out,
                         void* stream) {
    const char* me = "y2_wide_head_forward";
    if (!x || !packed || !bias || !out) return wide_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wide_check(me, K, Cout)) return e;
    if (M < 1) return wide_fail(Y2_ERR_ARG, "%s: M = %d: at least 1", me, M);
    if ((uintptr_t)x % 16 || (uintptr_t)packed % 16)
        return wide_fail(Y2_ERR_ARG, "%s: x and packed must be 16-byte aligned", me);
    const long long nMT = ((long long)M + T::kBM - 1) / T::kBM, nCT = (long long)(wide_cp(Cout) / T::kBN);
    if (nMT * nCT > 0x7fffffffLL)
        return wide_fail(Y2_ERR_ARG, "%s: M = %d, Cout = %d: %lld tiles are beyond one grid", me, M, Cout, nMT * nCT);
    hipLaunchKernelGGL(wide_head_forward_kernel, dim3((unsigned)(nMT * nCT)), dim3(T::kNT), 0, (hipStream_t)stream, x,
                       (const char*)packed, bias, out, M, K, Cout, (int)nMT);
    WIDE_CHK(hipGetLastError());
    return Y2_OK;
}

}  // extern "C"
