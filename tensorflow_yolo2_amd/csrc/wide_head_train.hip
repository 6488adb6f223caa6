// Training the wide head (wide_head.hip is its forward): the two backward products of out = x W + b, the bias gradient,
// Darknet's SGD on W and b fused with the re-pack of both operand images, and the second image itself.  Both products are
// wide_gemm.h at WideBwdTile (128 x 128, 2 x 2 waves of 2 x 2 MFMA tiles).
//
//   dx[m][k] = (1/s) sum_c f16(s dy[m][c]) f16(W[k][c])          y2_wide_head_backward_input   (reduction over Cout)
//   dW[k][c] = (1/s) sum_m f16(x[m][k]) f16(s dy[m][c])          y2_wide_head_backward_filter  (reduction over M)
//   db[c]    = sum_m dy[m][c]                                    fp32, from the unconverted dy, the same entry
//   s = grad_scale > 0, the loss scale of the half-precision modes; the results are unscaled (y2_backward_input's contract)
//
//   dy      : fp32 [M][Cout], row stride Cout exactly (what the tree loss writes): rows are 4-byte aligned only, so every
//             read is one dword per lane under a mask (m < M, c < Cout); times s and to f16 in registers
//   packed2 : f16 [Kp2][Cp2], Kp2 = K rounded up to the 128-column tile of dx, Cp2 = Cout rounded up to the 64-element
//             reduction step, padding zero (y2_wide_head_pack2; kept current by y2_wide_head_sgd_step): a filter row's Cout
//             range is contiguous -- the forward image [Cp][Kp] has K contiguous, the wrong way round for dx.  With it the
//             data gradient IS the forward kernel with the roles of K and Cout exchanged: A = dy, B = packed2
//   x       : fp32 [M][K], 16-byte aligned (the head stack's training output): float4 reads
//
// Data gradient: rows m, columns k, reduction c.  K = 1024 gives 8 column tiles and M = 289 three row tiles: 24 workgroups
// for 442 reduction steps, so the reduction is SPLIT across workgroups (y2_wide_head_train_plan; wide_split_product), and
// wide_head_sum_kernel adds the partials and divides by s.
// Filter gradient: rows k, columns c, reduction m -- the slow index of BOTH operands.  A thread loads EIGHT consecutive
// rows m of four k (float4) or four c (dwords 32 apart: a wave's read is 128 contiguous bytes of a dy row) and writes, per
// k or c, ONE 16-byte chunk of eight m: the transposition happens in registers on the way into LDS, and the fragment reads
// are the forward kernel's.  Rows m >= M are ZERO (not a copy of row M - 1: they are summed here).  The accumulator keeps c
// on the lane, so a store instruction writes two runs of 32 consecutive floats of two dW rows.  Its split is over M.
// Bias gradient: a launch of its own (wide_head_db_kernel).  Folded into the filter gradient it would either run in every
// one of the K / 128 row tiles of a column panel or make one of them the slow tile of its panel, and under a split over M
// it would need partials of its own; alone it reads dy once more (32 MB at the real width and M = 289, about 7 us).
#include "wide_gemm.h"
#include "optim_math.h"

namespace y2 {
namespace {

typedef WideBwdTile T;

// what a product's epilogue stores in column c of `out` (row stride C): the result itself, divided by s, or a raw partial
Y2_DEV auto wt_column(float* out, int C, bool fin, float s) {
    return [=](int c) { return [=](int r, float v) { out[(size_t)r * C + c] = fin ? v / s : v; }; };
}

// ---- data gradient: D[m][k] = sum_c f16(s dy[m][c]) P2[k][c]; dst = dx (nsplit == 1: divided by s) or the partials
__global__ __launch_bounds__(T::kNT) void wide_head_dgrad_kernel(const float* __restrict__ dy, const char* __restrict__ packed2,
                                                                 float* __restrict__ dst, int M, int K, int Cout, int Cp2,
                                                                 int nMT, int per, int nsplit, float s) {
    __shared__ __attribute__((aligned(16))) char smem[T::kLds];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = xcd_block(blockIdx.x, gridDim.x, 1);
    // the row tiles of one (column tile, split) read the same filter rows: neighbours in the logical grid
    const int mt = bx % nMT, rest = bx / nMT;
    const int sp = rest % nsplit, kt = rest / nsplit;
    const int m0 = mt * T::kBM, n0 = kt * T::kBN;
    const int nC = Cp2 / T::kBK;
    const int kk0 = sp * per, kk1 = kk0 + per < nC ? kk0 + per : nC;      // kk0 < nC: nsplit = ceil(nC / per)

    // ---- dy: masked dwords; behind M and behind Cout: zero
    const WideQuads<T> a = wide_quads<T>(tid);
    const WideRows<T> b = wide_rows<T>(packed2 + (size_t)n0 * ((size_t)Cp2 * 2), Cp2 * 2, lane, w);
    float xv[T::kPasses][4];
    auto issue = [&](int kk, int buf) {
        wide_stage_rows<T, size_t>(b, kk, smem + buf * T::kStage, w);
        const int c = kk * T::kBK + 4 * a.xj;
#pragma unroll
        for (int p = 0; p < T::kPasses; ++p) {
            const int m = m0 + p * T::kQuadRows + a.xr;
            const float* row = dy + (size_t)m * Cout + c;
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[p][e] = (m < M && c + e < Cout) ? row[e] : 0.f;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int p = 0; p < T::kPasses; ++p)
            wide_store_quad(smem + buf * T::kStage + a.dst[p], xv[p][0] * s, xv[p][1] * s, xv[p][2] * s, xv[p][3] * s);
    };

    const WideFrag f = wide_frag<T>(lane, w);
    f32x16 acc[T::kTM][T::kTN];
    wide_zero<T>(acc);
    wide_main_loop<T, true>(acc, smem, f, kk0, kk1, T::kTM, issue, store);
    wide_epilogue<T>(acc, f, m0, n0, M, K, wt_column(dst + (nsplit > 1 ? (size_t)sp * M * K : 0), K, nsplit == 1, s));
}

// ---- filter gradient: D[k][c] = sum_m f16(x[m][k]) f16(s dy[m][c]); dst = dW (nsplit == 1: divided by s) or the partials
__global__ __launch_bounds__(T::kNT) void wide_head_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 float* __restrict__ dst, int M, int K, int Cout, int nKT,
                                                                 int per, int nsplit, float s) {
    __shared__ __attribute__((aligned(16))) char smem[T::kLds];
    constexpr int kRows = 8;                                 // rows m of a step a thread holds: one 16-byte chunk of f16
    static_assert(T::kNT / 32 * kRows == T::kBK && T::kBM == 128 && T::kBN == 128, "the register transpose is written for this tile");
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = xcd_block(blockIdx.x, gridDim.x, 1);
    // the row tiles (k) of one (column panel, split) read the same dy rows, the larger operand: neighbours
    const int kt = bx % nKT, rest = bx / nKT;
    const int sp = rest % nsplit, ct = rest / nsplit;
    const int k0 = kt * T::kBM, n0 = ct * T::kBN;
    const int nM = (M + T::kBK - 1) / T::kBK;
    const int ms0 = sp * per, ms1 = ms0 + per < nM ? ms0 + per : nM;

    // ---- both operands: thread (mg, q) holds rows mg * 8 .. mg * 8 + 7 of the step; of x the floats 4 q .. 4 q + 3 of the
    // tile's k range, of dy the dwords q, q + 32, q + 64, q + 96 of its c range.  Value e of the eight rows is chunk mg of
    // staged row 4 q + e (x) or q + 32 e (dy)
    const int mg = tid >> 5, q = tid & 31;
    int adst[4], bdst[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ra = 4 * q + e, rb = q + 32 * e;
        adst[e] = ra * T::kRowB + ((mg ^ wide_swz(ra)) << 4);
        bdst[e] = T::kBM * T::kRowB + rb * T::kRowB + ((mg ^ wide_swz(rb)) << 4);
    }
    const bool k_ok = k0 + 4 * q < K;                        // K is a multiple of 32: a quad is whole or absent
    f32x4 xv[kRows];
    float dv[kRows][4];
    auto issue = [&](int ms, int) {
#pragma unroll
        for (int p = 0; p < kRows; ++p) {
            const int m = ms * T::kBK + mg * 8 + p;
            const bool row_ok = m < M;
            xv[p] = (row_ok && k_ok) ? *(const f32x4*)(x + (size_t)m * K + k0 + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
            const float* row = dy + (size_t)m * Cout + n0 + q;
#pragma unroll
            for (int e = 0; e < 4; ++e) dv[p][e] = (row_ok && n0 + q + 32 * e < Cout) ? row[32 * e] : 0.f;
        }
    };
    auto store = [&](int buf) {
        char* lbase = smem + buf * T::kStage;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            *(u32x4*)(lbase + adst[e]) = u32x4{pack2<half_t>(xv[0][e], xv[1][e]), pack2<half_t>(xv[2][e], xv[3][e]),
                                               pack2<half_t>(xv[4][e], xv[5][e]), pack2<half_t>(xv[6][e], xv[7][e])};
            *(u32x4*)(lbase + bdst[e]) =
                u32x4{pack2<half_t>(dv[0][e] * s, dv[1][e] * s), pack2<half_t>(dv[2][e] * s, dv[3][e] * s),
                      pack2<half_t>(dv[4][e] * s, dv[5][e] * s), pack2<half_t>(dv[6][e] * s, dv[7][e] * s)};
        }
    };

    const WideFrag f = wide_frag<T>(lane, w);
    f32x16 acc[T::kTM][T::kTN];
    wide_zero<T>(acc);
    wide_main_loop<T, false>(acc, smem, f, ms0, ms1, T::kTM, issue, store);
    wide_epilogue<T>(acc, f, k0, n0, K, Cout, wt_column(dst + (nsplit > 1 ? (size_t)sp * K * Cout : 0), Cout, nsplit == 1, s));
}

// dst[i] = (part[0][i] + part[1][i] + ... in that order) / s: the finish pass of a split product
__global__ __launch_bounds__(256) void wide_head_sum_kernel(const float* __restrict__ part, float* __restrict__ dst, size_t n,
                                                            int nsplit, float s) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float a = part[i];
        for (int sp = 1; sp < nsplit; ++sp) a += part[(size_t)sp * n + i];
        dst[i] = a / s;
    }
}

// db[c] = sum_m dy[m][c]: 32 columns x 8 row lanes per workgroup; lane ty adds rows ty, ty + 8, ... in order, then row lane 0
// adds the eight sums in order
__global__ __launch_bounds__(256) void wide_head_db_kernel(const float* __restrict__ dy, float* __restrict__ db, int M, int Cout) {
    __shared__ float part[8][32];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + tx;
    float a = 0.f;
    if (c < Cout)
        for (int m = ty; m < M; m += 8) a += dy[(size_t)m * Cout + c];
    part[ty][tx] = a;
    __syncthreads();
    if (ty == 0 && c < Cout) {
        float t = part[0][tx];
#pragma unroll
        for (int r = 1; r < 8; ++r) t += part[r][tx];
        db[c] = t;
    }
}

// W fp32 [K][Cout] -> packed2 f16 [Kp2][Cp2]: both sides run along Cout; the padding is written as zero
__global__ __launch_bounds__(256) void wide_head_pack2_kernel(const float* __restrict__ W, half_t* __restrict__ packed2, int K,
                                                              int Cout, int Cp2, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t k = i / Cp2, c = i - k * Cp2;
        wide_put_image2(packed2, Cp2, k, c, (k < (size_t)K && c < (size_t)Cout) ? W[k * Cout + c] : 0.f);
    }
}

struct WtCtrlView { int found_inf, step, skipped, reserved; float lr_t; };

// Darknet's SGD on W (decayed) and b (not) + both operand images from the new W, per 32 x 32 tile of [K][Cout].  The grid
// covers [Kp2][Cp]: the padding of both images is rewritten as zero.  ctrl (nullable): found_inf set -> return at once (the
// images are current already); else lr_t from the control block
__global__ __launch_bounds__(256) void wide_head_sgd_kernel(float* __restrict__ W, float* __restrict__ b, float* __restrict__ accum,
                                                            const float* __restrict__ dW, const float* __restrict__ db,
                                                            half_t* __restrict__ packed, half_t* __restrict__ packed2, int K,
                                                            int Cout, int Kp, int Cp2, const WtCtrlView* ctrl, float lr_t,
                                                            float mom, float decay, float gscale) {
    __shared__ float tile[32][33];
    if (ctrl) {
        if (ctrl->found_inf) return;
        lr_t = ctrl->lr_t;
    }
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, c = c0 + tx;
        float p = 0.f;
        if (k < K && c < Cout) {
            const size_t i = (size_t)k * Cout + c;
            p = W[i];
            float a = accum[i];
            sgd_update(p, a, dW[i] * gscale, lr_t, mom, decay, true);
            accum[i] = a;
            W[i] = p;
        }
        tile[r][tx] = p;
        if (c < Cp2) wide_put_image2(packed2, Cp2, k, c, p);              // k < Kp2: the grid's height
    }
    __syncthreads();
    if (k0 + tx < Kp) wide_put_image(tile, packed, Kp, c0, k0, tx, ty);   // c0 + r < Cp: the grid's width
    if (blockIdx.y == 0 && ty == 0 && c0 + tx < Cout) {
        const int c = c0 + tx;
        float p = b[c], a = accum[(size_t)K * Cout + c];
        sgd_update(p, a, db[c] * gscale, lr_t, mom, decay, false);
        accum[(size_t)K * Cout + c] = a;
        b[c] = p;
    }
}

int wt_check_ms(const char* me, int M, float s) {
    if (M < 1) return wide_fail(Y2_ERR_ARG, "%s: M = %d: at least 1", me, M);
    if (!(s > 0.f && s < __builtin_huge_valf())) return wide_fail(Y2_ERR_ARG, "%s: grad_scale = %g: finite and above 0", me, (double)s);
    return Y2_OK;
}

// the launch of wide_head_sum_kernel, as wide_split_product calls it
auto wt_sum(float s, void* stream) {
    return [=](const float* part, float* dst, size_t n, int ns) {
        size_t nb = (n + 255) / 256;
        if (nb > 4096) nb = 4096;
        hipLaunchKernelGGL(wide_head_sum_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, part, dst, n, ns, s);
    };
}

}  // namespace
}  // namespace y2

using namespace y2;

extern "C" {

int y2_wide_head_train_plan(int M, int K, int Cout, int cus, int* dx_split, int* dw_split) {
    const char* me = "y2_wide_head_train_plan";
    if (!dx_split || !dw_split) return wide_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wide_check(me, K, Cout)) return e;
    if (M < 1) return wide_fail(Y2_ERR_ARG, "%s: M = %d: at least 1", me, M);
    if (cus < 1) return wide_fail(Y2_ERR_ARG, "%s: cus = %d: at least 1", me, cus);
    int per;
    const WideProduct dx = wide_dx_product(M, K, Cout), dw = wide_dw_product(M, K, Cout);
    wide_normalise(wide_up(cus, dx.tiles), dx.steps, &per, dx_split);
    wide_normalise(wide_up(cus, dw.tiles), dw.steps, &per, dw_split);
    return Y2_OK;
}

size_t y2_wide_head_packed2_bytes(int K, int Cout) {
    if (wide_check(nullptr, K, Cout)) return 0;
    return wide_kp2(K) * wide_cp2(Cout) * sizeof(half_t);
}

int y2_wide_head_pack2(const float* W, int K, int Cout, void* packed2, size_t packed2_bytes, void* stream) {
    const char* me = "y2_wide_head_pack2";
    if (!W || !packed2) return wide_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wide_check(me, K, Cout)) return e;
    const size_t need = y2_wide_head_packed2_bytes(K, Cout);
    if (packed2_bytes < need)
        return wide_fail(Y2_ERR_ARG, "%s: packed2_bytes = %zu, K = %d and Cout = %d need %zu", me, packed2_bytes, K, Cout, need);
    if ((uintptr_t)packed2 % 16) return wide_fail(Y2_ERR_ARG, "%s: packed2 is not 16-byte aligned", me);
    const size_t total = need / sizeof(half_t);
    size_t nb = (total + 1023) / 1024;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(wide_head_pack2_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, W, (half_t*)packed2, K, Cout,
                       (int)wide_cp2(Cout), total);
    WIDE_CHK(hipGetLastError());
    return Y2_OK;
}

size_t y2_wide_head_backward_input_workspace_bytes(int M, int K, int Cout, int split) {
    if (wide_check(nullptr, K, Cout) || M < 1 || split < 0) return 0;
    int per, ns;
    return wide_split(wide_dx_product(M, K, Cout), split, &per, &ns);
}

size_t y2_wide_head_backward_filter_workspace_bytes(int M, int K, int Cout, int split) {
    if (wide_check(nullptr, K, Cout) || M < 1 || split < 0) return 0;
    int per, ns;
    return wide_split(wide_dw_product(M, K, Cout), split, &per, &ns);
}

int y2_wide_head_backward_input(const float* dy, const void* packed2, int M, int K, int Cout, float grad_scale, float* dx,
                                void* workspace, size_t workspace_bytes, int split, void* stream) {
    const char* me = "y2_wide_head_backward_input";
    if (!dy || !packed2 || !dx) return wide_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wide_check(me, K, Cout)) return e;
    if (int e = wt_check_ms(me, M, grad_scale)) return e;
    if (split < 0) return wide_fail(Y2_ERR_ARG, "%s: split = %d: 0 for the plan's, or at least 1", me, split);
    if ((uintptr_t)packed2 % 16) return wide_fail(Y2_ERR_ARG, "%s: packed2 must be 16-byte aligned", me);
    if ((uintptr_t)dy % 4 || (uintptr_t)dx % 4) return wide_fail(Y2_ERR_ARG, "%s: dy and dx must be 4-byte aligned", me);
    return wide_split_product(
        me, wide_dx_product(M, K, Cout), split, dx, workspace, workspace_bytes,
        [=](unsigned blocks, float* dst, int per, int ns) {
            hipLaunchKernelGGL(wide_head_dgrad_kernel, dim3(blocks), dim3(T::kNT), 0, (hipStream_t)stream, dy, (const char*)packed2,
                               dst, M, K, Cout, (int)wide_cp2(Cout), (int)wide_up(M, T::kBM), per, ns, grad_scale);
        },
        wt_sum(grad_scale, stream));
}

int y2_wide_head_backward_filter(const float* x, const float* dy, int M, int K, int Cout, float grad_scale, float* dW, float* db,
                                 void* workspace, size_t workspace_bytes, int split, void* stream) {
    const char* me = "y2_wide_head_backward_filter";
    if (!x || !dy || !dW || !db) return wide_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wide_check(me, K, Cout)) return e;
    if (int e = wt_check_ms(me, M, grad_scale)) return e;
    if (split < 0) return wide_fail(Y2_ERR_ARG, "%s: split = %d: 0 for the plan's, or at least 1", me, split);
    if ((uintptr_t)x % 16) return wide_fail(Y2_ERR_ARG, "%s: x must be 16-byte aligned", me);
    if ((uintptr_t)dy % 4 || (uintptr_t)dW % 4 || (uintptr_t)db % 4)
        return wide_fail(Y2_ERR_ARG, "%s: dy, dW and db must be 4-byte aligned", me);
    if (int e = wide_split_product(
            me, wide_dw_product(M, K, Cout), split, dW, workspace, workspace_bytes,
            [=](unsigned blocks, float* dst, int per, int ns) {
                hipLaunchKernelGGL(wide_head_wgrad_kernel, dim3(blocks), dim3(T::kNT), 0, (hipStream_t)stream, x, dy, dst, M, K,
                                   Cout, (int)wide_up(K, T::kBM), per, ns, grad_scale);
            },
            wt_sum(grad_scale, stream)))
        return e;
    hipLaunchKernelGGL(wide_head_db_kernel, dim3((unsigned)wide_up(Cout, 32)), dim3(256), 0, (hipStream_t)stream, dy, db, M, Cout);
    WIDE_CHK(hipGetLastError());
    return Y2_OK;
}

int y2_wide_head_sgd_step(float* W, float* b, float* accum, const float* dW, const float* db, int K, int Cout, void* packed,
                          size_t packed_bytes, void* packed2, size_t packed2_bytes, const void* ctrl, float lr, float momentum,
                          float decay, float grad_mult, void* stream) {
    const char* me = "y2_wide_head_sgd_step";
    if (!W || !b || !accum || !dW || !db || !packed || !packed2) return wide_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wide_check(me, K, Cout)) return e;
    const float inf = __builtin_huge_valf();
    if (!ctrl && !(lr >= 0.f && lr < inf)) return wide_fail(Y2_ERR_ARG, "%s: lr = %g: finite and >= 0", me, (double)lr);
    if (!(momentum >= 0.f && momentum < 1.f)) return wide_fail(Y2_ERR_ARG, "%s: momentum = %g outside [0, 1)", me, (double)momentum);
    if (!(decay >= 0.f && decay < inf)) return wide_fail(Y2_ERR_ARG, "%s: decay = %g: finite and >= 0", me, (double)decay);
    const size_t need = wide_cp(Cout) * wide_kp(K) * sizeof(half_t), need2 = y2_wide_head_packed2_bytes(K, Cout);
    if (packed_bytes < need)
        return wide_fail(Y2_ERR_ARG, "%s: packed_bytes = %zu, K = %d and Cout = %d need %zu", me, packed_bytes, K, Cout, need);
    if (packed2_bytes < need2)
        return wide_fail(Y2_ERR_ARG, "%s: packed2_bytes = %zu, K = %d and Cout = %d need %zu", me, packed2_bytes, K, Cout, need2);
    if ((uintptr_t)packed % 16 || (uintptr_t)packed2 % 16)
        return wide_fail(Y2_ERR_ARG, "%s: packed and packed2 must be 16-byte aligned", me);
    hipLaunchKernelGGL(wide_head_sgd_kernel, dim3((unsigned)(wide_cp(Cout) / 32), (unsigned)(wide_kp2(K) / 32)), dim3(256), 0,
                       (hipStream_t)stream, W, b, accum, dW, db, (half_t*)packed, (half_t*)packed2, K, Cout, (int)wide_kp(K),
                       (int)wide_cp2(Cout), (const WtCtrlView*)ctrl, lr, momentum, decay, grad_mult);
    WIDE_CHK(hipGetLastError());
    return Y2_OK;
}

}  // extern "C"
