// Training the wide head (wide_head.hip is its forward): the two backward products of out = x W + b, the bias gradient,
// Darknet's SGD on W and b fused with the re-pack of both operand images, and the second image itself.
//
//   dx[m][k] = (1/s) sum_c f16(s dy[m][c]) f16(W[k][c])          y2_wide_head_backward_input   (reduction over Cout)
//   dW[k][c] = (1/s) sum_m f16(x[m][k]) f16(s dy[m][c])          y2_wide_head_backward_filter  (reduction over M)
//   db[c]    = sum_m dy[m][c]                                    fp32, from the unconverted dy, the same entry
//   s = grad_scale > 0, the loss scale of the half-precision modes; the results are unscaled (y2_backward_input's contract)
//
//   dy      : fp32 [M][Cout], row stride Cout exactly (what the tree loss writes): rows are 4-byte aligned only, so every
//             read is one dword per lane under a mask (m < M, c < Cout); times s and to f16 in registers, as the forward
//             kernel converts x
//   packed2 : f16 [Kp2][Cp2], Kp2 = K rounded up to the 128-column tile of dx, Cp2 = Cout rounded up to the 64-element
//             reduction step, padding zero (y2_wide_head_pack2; kept current by y2_wide_head_sgd_step): a filter row's Cout
//             range is contiguous -- the forward image [Cp][Kp] has K contiguous, the wrong way round for dx.  With it the
//             data gradient IS the forward kernel with the roles of K and Cout exchanged: global_load_lds rows of 128 bytes
//   x       : fp32 [M][K], 16-byte aligned (the head stack's training output): float4 reads
//
// One tile geometry for both products: 256 threads = 2 x 2 waves, each 64 x 64 (2 x 2 MFMA tiles of 32x32x16 f16, 64
// accumulator registers); tile 128 x 128; 64 reduction elements per step; LDS two stages of (128 + 128) rows x 128 bytes =
// 64 KiB, XOR-swizzled in 16-byte chunks exactly as wide_head.hip (wt_swz), so two workgroups share a CU.  One barrier per
// step: the loads of step k + 1 are issued behind it, the MFMAs of step k run under them, the converted rows are written
// after the MFMAs.
// Data gradient: rows m, columns k, reduction c.  K = 1024 gives 8 column tiles and M = 289 three row tiles: 24 workgroups
// for 442 reduction steps, so the reduction is SPLIT across workgroups (y2_wide_head_train_plan): split sp takes steps
// [sp per, (sp + 1) per), writes raw fp32 partials [split][M][K] into the workspace, and wide_head_sum_kernel adds them in
// the order of sp and divides by s.  No atomics: the same bits every run.  split = 1 stores dx itself.
// Filter gradient: rows k, columns c, reduction m -- the slow index of BOTH operands.  A thread loads EIGHT consecutive
// rows m of four k (float4) or four c (dwords 32 apart: a wave's read is 128 contiguous bytes of a dy row) and writes, per
// k or c, ONE 16-byte chunk of eight m: the transposition happens in registers on the way into LDS, and the fragment reads
// are the forward kernel's.  Rows m >= M are ZERO (not a copy of row M - 1: they are summed here).  The accumulator keeps c
// on the lane, so a store instruction writes two runs of 32 consecutive floats of two dW rows.  Its split is over M.
// Bias gradient: a launch of its own (wide_head_db_kernel).  Folded into the filter gradient it would either run in every
// one of the K / 128 row tiles of a column panel or make one of them the slow tile of its panel, and under a split over M
// it would need partials of its own; alone it reads dy once more (32 MB at the real width and M = 289, about 7 us).
#include <stdio.h>
#include <stdarg.h>
#include "common.h"
#include "optim_math.h"
#include "../../include/yolo2_hip.h"

namespace y2 {
int set_error(int code, const char* msg);   // net.hip (y2_last_error)

namespace {

constexpr int kWtBM = 128, kWtBN = 128, kWtBK = 64;          // tile rows, tile columns, reduction elements per step
constexpr int kWtNT = 256;                                   // threads: 2 (rows) x 2 (columns) waves
constexpr int kWtRowB = kWtBK * 2;                           // bytes of a staged row: 128
constexpr int kWtStage = (kWtBM + kWtBN) * kWtRowB;          // 32 KiB
constexpr int kWtLds = 2 * kWtStage;
constexpr int kWtPasses = kWtBM * kWtBK / 4 / kWtNT;         // 4-float groups per thread and step: 8
constexpr int kWtWInstr = kWtBN * kWtRowB / 1024 / (kWtNT / 64);   // global_load_lds instructions per wave and step: 4
constexpr int kWtTM = 2, kWtTN = 2;                          // MFMA tiles of a wave
constexpr int kWtMaxSplit = 64;                              // bounds the workspace: split x the product's size

// 16-byte chunk `c` of staged row `r` stands at chunk position c ^ swz(r) (wide_head.hip wh_swz)
Y2_DEV int wt_swz(int r) { return (r >> 1) & 7; }

struct WtFrag {
    int foff[4], abase, bbase, r32, hh, wm, wc;
};
Y2_DEV WtFrag wt_frag(int lane, int w) {
    WtFrag f;
    f.r32 = lane & 31;
    f.hh = lane >> 5;
    f.wm = w >> 1;
    f.wc = w & 1;
#pragma unroll
    for (int g = 0; g < 4; ++g) f.foff[g] = f.r32 * kWtRowB + (((2 * g + f.hh) ^ wt_swz(f.r32)) << 4);
    f.abase = f.wm * kWtTM * 32 * kWtRowB;
    f.bbase = kWtBM * kWtRowB + f.wc * kWtTN * 32 * kWtRowB;
    return f;
}
// the 64 reduction elements of one staged step: acc[i][j] += A rows (registers) x B rows (lanes)
Y2_DEV void wt_mma_step(f32x16 (&acc)[kWtTM][kWtTN], const char* lb, const WtFrag& f) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f16x8 fa[kWtTM], fb[kWtTN];
#pragma unroll
        for (int j = 0; j < kWtTN; ++j) fb[j] = *(const f16x8*)(lb + f.bbase + j * 32 * kWtRowB + f.foff[g]);
#pragma unroll
        for (int i = 0; i < kWtTM; ++i) fa[i] = *(const f16x8*)(lb + f.abase + i * 32 * kWtRowB + f.foff[g]);
#pragma unroll
        for (int i = 0; i < kWtTM; ++i)
#pragma unroll
            for (int j = 0; j < kWtTN; ++j) mma32(acc[i][j], fa[i], fb[j]);
    }
}
Y2_DEV void wt_zero(f32x16 (&acc)[kWtTM][kWtTN]) {
#pragma unroll
    for (int i = 0; i < kWtTM; ++i)
#pragma unroll
        for (int j = 0; j < kWtTN; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
}

// ---- data gradient: D[m][k] = sum_c f16(s dy[m][c]) P2[k][c]; dst = dx (nsplit == 1: divided by s) or the partials
__global__ __launch_bounds__(kWtNT) void wide_head_dgrad_kernel(const float* __restrict__ dy, const char* __restrict__ packed2,
                                                                float* __restrict__ dst, int M, int K, int Cout, int Cp2,
                                                                int nMT, int per, int nsplit, float s) {
    __shared__ __attribute__((aligned(16))) char smem[kWtLds];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = xcd_block(blockIdx.x, gridDim.x, 1);
    // the row tiles of one (column tile, split) read the same filter rows: neighbours in the logical grid
    const int mt = bx % nMT, rest = bx / nMT;
    const int sp = rest % nsplit, kt = rest / nsplit;
    const int m0 = mt * kWtBM, n0 = kt * kWtBN;
    const int nC = Cp2 / kWtBK;
    const int kk0 = sp * per, kk1 = kk0 + per < nC ? kk0 + per : nC;      // kk0 < nC: nsplit = ceil(nC / per)

    // ---- dy: pass p loads dwords [4 xj, 4 xj + 4) of the step of tile row p * 16 + xr; behind M and behind Cout: zero
    const int xr = tid >> 4, xj = tid & 15;
    int xdst[kWtPasses];
#pragma unroll
    for (int p = 0; p < kWtPasses; ++p) {
        const int r = p * 16 + xr;
        xdst[p] = r * kWtRowB + (((xj >> 1) ^ wt_swz(r)) << 4) + ((xj & 1) << 3);
    }
    float xv[kWtPasses][4];
    auto load_a = [&](int kk) {
        const int c = kk * kWtBK + 4 * xj;
#pragma unroll
        for (int p = 0; p < kWtPasses; ++p) {
            const int m = m0 + p * 16 + xr;
            const float* row = dy + (size_t)m * Cout + c;
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[p][e] = (m < M && c + e < Cout) ? row[e] : 0.f;
        }
    };
    auto store_a = [&](int buf) {
        char* lbase = smem + buf * kWtStage;
#pragma unroll
        for (int p = 0; p < kWtPasses; ++p)
            *(u32x2*)(lbase + xdst[p]) = u32x2{pack2<half_t>(xv[p][0] * s, xv[p][1] * s), pack2<half_t>(xv[p][2] * s, xv[p][3] * s)};
    };
    // ---- filters: instruction i of wave w stages rows (w * 4 + i) * 8 + lane / 8, lane % 8 the chunk position
    const char* wbase_g = packed2 + (size_t)n0 * ((size_t)Cp2 * 2);
    int woff[kWtWInstr];
#pragma unroll
    for (int i = 0; i < kWtWInstr; ++i) {
        const int r = (w * kWtWInstr + i) * 8 + (lane >> 3);
        woff[i] = r * Cp2 * 2 + (((lane & 7) ^ wt_swz(r)) << 4);          // at most 127 * 2^21 + 127 bytes
    }
    auto stage_b = [&](int kk, int buf) {
        char* lbase = smem + buf * kWtStage + kWtBM * kWtRowB;
#pragma unroll
        for (int i = 0; i < kWtWInstr; ++i) glds16(wbase_g + woff[i] + (size_t)kk * kWtRowB, lbase + (w * kWtWInstr + i) * 1024);
    };

    const WtFrag f = wt_frag(lane, w);
    f32x16 acc[kWtTM][kWtTN];
    wt_zero(acc);

    stage_b(kk0, 0);
    load_a(kk0);
    store_a(0);
    for (int kk = kk0; kk < kk1; ++kk) {
        const int cur = (kk - kk0) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's filter rows of step kk have landed
        __syncthreads();                                      // everyone's have, and everyone's dy rows; step kk - 1 is read
        const bool more = kk + 1 < kk1;
        if (more) {
            stage_b(kk + 1, cur ^ 1);
            load_a(kk + 1);
        }
        wt_mma_step(acc, smem + cur * kWtStage, f);
        if (more) store_a(cur ^ 1);
    }

    float* out = dst + (nsplit > 1 ? (size_t)sp * M * K : 0);
    const bool fin = nsplit == 1;
#pragma unroll
    for (int j = 0; j < kWtTN; ++j) {
        const int k = n0 + (f.wc * kWtTN + j) * 32 + f.r32;
        if (k >= K) continue;
#pragma unroll
        for (int i = 0; i < kWtTM; ++i) {
            const int mb = m0 + (f.wm * kWtTM + i) * 32;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int m = mb + acc_row(q, f.hh);
                if (m < M) out[(size_t)m * K + k] = fin ? acc[i][j][q] / s : acc[i][j][q];
            }
        }
    }
}

// ---- filter gradient: D[k][c] = sum_m f16(x[m][k]) f16(s dy[m][c]); dst = dW (nsplit == 1: divided by s) or the partials
__global__ __launch_bounds__(kWtNT) void wide_head_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                float* __restrict__ dst, int M, int K, int Cout, int nKT,
                                                                int per, int nsplit, float s) {
    __shared__ __attribute__((aligned(16))) char smem[kWtLds];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = xcd_block(blockIdx.x, gridDim.x, 1);
    // the row tiles (k) of one (column panel, split) read the same dy rows, the larger operand: neighbours
    const int kt = bx % nKT, rest = bx / nKT;
    const int sp = rest % nsplit, ct = rest / nsplit;
    const int k0 = kt * kWtBM, n0 = ct * kWtBN;
    const int nM = (M + kWtBK - 1) / kWtBK;
    const int ms0 = sp * per, ms1 = ms0 + per < nM ? ms0 + per : nM;

    // ---- both operands: thread (mg, q) holds rows mg * 8 .. mg * 8 + 7 of the step; of x the floats 4 q .. 4 q + 3 of the
    // tile's k range, of dy the dwords q, q + 32, q + 64, q + 96 of its c range.  Value e of the eight rows is chunk mg of
    // staged row 4 q + e (x) or q + 32 e (dy)
    const int mg = tid >> 5, q = tid & 31;
    int adst[4], bdst[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ra = 4 * q + e, rb = q + 32 * e;
        adst[e] = ra * kWtRowB + ((mg ^ wt_swz(ra)) << 4);
        bdst[e] = kWtBM * kWtRowB + rb * kWtRowB + ((mg ^ wt_swz(rb)) << 4);
    }
    const bool k_ok = k0 + 4 * q < K;                        // K is a multiple of 32: a quad is whole or absent
    f32x4 xv[kWtPasses];
    float dv[kWtPasses][4];
    auto load_ab = [&](int ms) {
#pragma unroll
        for (int p = 0; p < kWtPasses; ++p) {
            const int m = ms * kWtBK + mg * 8 + p;
            const bool row_ok = m < M;
            xv[p] = (row_ok && k_ok) ? *(const f32x4*)(x + (size_t)m * K + k0 + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
            const float* row = dy + (size_t)m * Cout + n0 + q;
#pragma unroll
            for (int e = 0; e < 4; ++e) dv[p][e] = (row_ok && n0 + q + 32 * e < Cout) ? row[32 * e] : 0.f;
        }
    };
    auto store_ab = [&](int buf) {
        char* lbase = smem + buf * kWtStage;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            *(u32x4*)(lbase + adst[e]) = u32x4{pack2<half_t>(xv[0][e], xv[1][e]), pack2<half_t>(xv[2][e], xv[3][e]),
                                               pack2<half_t>(xv[4][e], xv[5][e]), pack2<half_t>(xv[6][e], xv[7][e])};
            *(u32x4*)(lbase + bdst[e]) =
                u32x4{pack2<half_t>(dv[0][e] * s, dv[1][e] * s), pack2<half_t>(dv[2][e] * s, dv[3][e] * s),
                      pack2<half_t>(dv[4][e] * s, dv[5][e] * s), pack2<half_t>(dv[6][e] * s, dv[7][e] * s)};
        }
    };

    const WtFrag f = wt_frag(lane, w);
    f32x16 acc[kWtTM][kWtTN];
    wt_zero(acc);

    load_ab(ms0);
    store_ab(0);
    for (int ms = ms0; ms < ms1; ++ms) {
        const int cur = (ms - ms0) & 1;
        __syncthreads();                                      // everyone's rows of step ms are written; step ms - 1 is read
        const bool more = ms + 1 < ms1;
        if (more) load_ab(ms + 1);
        wt_mma_step(acc, smem + cur * kWtStage, f);
        if (more) store_ab(cur ^ 1);
    }

    float* out = dst + (nsplit > 1 ? (size_t)sp * K * Cout : 0);
    const bool fin = nsplit == 1;
#pragma unroll
    for (int j = 0; j < kWtTN; ++j) {
        const int c = n0 + (f.wc * kWtTN + j) * 32 + f.r32;
        if (c >= Cout) continue;
#pragma unroll
        for (int i = 0; i < kWtTM; ++i) {
            const int kb = k0 + (f.wm * kWtTM + i) * 32;
#pragma unroll
            for (int qq = 0; qq < 16; ++qq) {
                const int k = kb + acc_row(qq, f.hh);
                if (k < K) out[(size_t)k * Cout + c] = fin ? acc[i][j][qq] / s : acc[i][j][qq];
            }
        }
    }
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
        packed2[i] = (k < (size_t)K && c < (size_t)Cout) ? (half_t)W[k * Cout + c] : (half_t)0.f;
    }
}

struct WtCtrlView { int found_inf, step, skipped, reserved; float lr_t; };

// Darknet's SGD on W (decayed) and b (not) + both operand images from the new W, per 32 x 32 tile of [K][Cout]: reads and
// the packed2 writes run along Cout, the forward image's writes along K through the LDS tile (wide_head_pack_kernel's way).
// The grid covers [Kp2][Cp]: the padding of both images is rewritten as zero.  ctrl (nullable): found_inf set -> return at
// once (the images are current already); else lr_t from the control block
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
        if (c < Cp2) packed2[(size_t)k * Cp2 + c] = (half_t)p;             // k < Kp2: the grid's height
    }
    __syncthreads();
    if (k0 + tx < Kp) {
#pragma unroll
        for (int r = ty; r < 32; r += 8) packed[(size_t)(c0 + r) * Kp + k0 + tx] = (half_t)tile[tx][r];   // c0 + r < Cp: the width
    }
    if (blockIdx.y == 0 && ty == 0 && c0 + tx < Cout) {
        const int c = c0 + tx;
        float p = b[c], a = accum[(size_t)K * Cout + c];
        sgd_update(p, a, db[c] * gscale, lr_t, mom, decay, false);
        accum[(size_t)K * Cout + c] = a;
        b[c] = p;
    }
}

int wt_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return set_error(code, buf);
}

bool wt_shape_ok(int K, int Cout) {
    return !(K < 32 || K % 32 || K > Y2_WIDE_HEAD_MAX_K || Cout < 1 || Cout > Y2_WIDE_HEAD_MAX_COUT);
}
int wt_check(const char* me, int K, int Cout) {
    if (K < 32 || K % 32 || K > Y2_WIDE_HEAD_MAX_K)
        return wt_fail(Y2_ERR_ARG, "%s: K = %d: a multiple of 32, at most %d", me, K, Y2_WIDE_HEAD_MAX_K);
    if (Cout < 1 || Cout > Y2_WIDE_HEAD_MAX_COUT)
        return wt_fail(Y2_ERR_ARG, "%s: Cout = %d outside 1..%d", me, Cout, Y2_WIDE_HEAD_MAX_COUT);
    return Y2_OK;
}
int wt_check_ms(const char* me, int M, float s) {
    if (M < 1) return wt_fail(Y2_ERR_ARG, "%s: M = %d: at least 1", me, M);
    if (!(s > 0.f && s < __builtin_huge_valf())) return wt_fail(Y2_ERR_ARG, "%s: grad_scale = %g: finite and above 0", me, (double)s);
    return Y2_OK;
}

long long wt_up(long long a, long long b) { return (a + b - 1) / b; }
size_t wt_kp(int K) { return (size_t)wt_up(K, 64) * 64; }            // the forward image's (wide_head.hip)
size_t wt_cp(int Cout) { return (size_t)wt_up(Cout, 256) * 256; }
size_t wt_kp2(int K) { return (size_t)wt_up(K, kWtBN) * kWtBN; }
size_t wt_cp2(int Cout) { return (size_t)wt_up(Cout, kWtBK) * kWtBK; }

// `want` workgroups' worth of splits over `steps` reduction steps -> (steps per split, splits): every split holds a step
void wt_normalise(long long want, long long steps, int* per, int* nsplit) {
    if (want > kWtMaxSplit) want = kWtMaxSplit;
    if (want > steps) want = steps;
    if (want < 1) want = 1;
    *per = (int)wt_up(steps, want);
    *nsplit = (int)wt_up(steps, *per);
}
long long wt_dx_tiles(int M, int K) { return wt_up(M, kWtBM) * wt_up(K, kWtBN); }
long long wt_dw_tiles(int K, int Cout) { return wt_up(K, kWtBM) * wt_up(Cout, kWtBN); }
long long wt_dx_steps(int Cout) { return wt_up(Cout, kWtBK); }
long long wt_dw_steps(int M) { return wt_up(M, kWtBK); }

int wt_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            n < 1)
            return 256;                                      // no device to ask: an MI355X's
        cus = n;
    }
    return cus;
}

// the caller's split (0: the plan's for this device) -> (steps per split, splits)
void wt_split(int split, long long tiles, long long steps, int* per, int* nsplit) {
    wt_normalise(split > 0 ? split : wt_up(wt_cus(), tiles), steps, per, nsplit);
}

}  // namespace
}  // namespace y2

using namespace y2;

#define WTCHK(expr)                                                                            \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return wt_fail(Y2_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

extern "C" {

int y2_wide_head_train_plan(int M, int K, int Cout, int cus, int* dx_split, int* dw_split) {
    const char* me = "y2_wide_head_train_plan";
    if (!dx_split || !dw_split) return wt_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wt_check(me, K, Cout)) return e;
    if (M < 1) return wt_fail(Y2_ERR_ARG, "%s: M = %d: at least 1", me, M);
    if (cus < 1) return wt_fail(Y2_ERR_ARG, "%s: cus = %d: at least 1", me, cus);
    int per;
    wt_normalise(wt_up(cus, wt_dx_tiles(M, K)), wt_dx_steps(Cout), &per, dx_split);
    wt_normalise(wt_up(cus, wt_dw_tiles(K, Cout)), wt_dw_steps(M), &per, dw_split);
    return Y2_OK;
}

size_t y2_wide_head_packed2_bytes(int K, int Cout) {
    if (!wt_shape_ok(K, Cout)) return 0;
    return wt_kp2(K) * wt_cp2(Cout) * sizeof(half_t);
}

int y2_wide_head_pack2(const float* W, int K, int Cout, void* packed2, size_t packed2_bytes, void* stream) {
    const char* me = "y2_wide_head_pack2";
    if (!W || !packed2) return wt_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wt_check(me, K, Cout)) return e;
    const size_t need = y2_wide_head_packed2_bytes(K, Cout);
    if (packed2_bytes < need)
        return wt_fail(Y2_ERR_ARG, "%s: packed2_bytes = %zu, K = %d and Cout = %d need %zu", me, packed2_bytes, K, Cout, need);
    if ((uintptr_t)packed2 % 16) return wt_fail(Y2_ERR_ARG, "%s: packed2 is not 16-byte aligned", me);
    const size_t total = need / sizeof(half_t);
    size_t nb = (total + 1023) / 1024;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(wide_head_pack2_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, W, (half_t*)packed2, K, Cout,
                       (int)wt_cp2(Cout), total);
    WTCHK(hipGetLastError());
    return Y2_OK;
}

size_t y2_wide_head_backward_input_workspace_bytes(int M, int K, int Cout, int split) {
    if (!wt_shape_ok(K, Cout) || M < 1 || split < 0) return 0;
    int per, ns;
    wt_split(split, wt_dx_tiles(M, K), wt_dx_steps(Cout), &per, &ns);
    return ns > 1 ? (size_t)ns * M * K * sizeof(float) : 0;
}

size_t y2_wide_head_backward_filter_workspace_bytes(int M, int K, int Cout, int split) {
    if (!wt_shape_ok(K, Cout) || M < 1 || split < 0) return 0;
    int per, ns;
    wt_split(split, wt_dw_tiles(K, Cout), wt_dw_steps(M), &per, &ns);
    return ns > 1 ? (size_t)ns * K * Cout * sizeof(float) : 0;
}

int y2_wide_head_backward_input(const float* dy, const void* packed2, int M, int K, int Cout, float grad_scale, float* dx,
                                void* workspace, size_t workspace_bytes, int split, void* stream) {
    const char* me = "y2_wide_head_backward_input";
    if (!dy || !packed2 || !dx) return wt_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wt_check(me, K, Cout)) return e;
    if (int e = wt_check_ms(me, M, grad_scale)) return e;
    if (split < 0) return wt_fail(Y2_ERR_ARG, "%s: split = %d: 0 for the plan's, or at least 1", me, split);
    if ((uintptr_t)packed2 % 16) return wt_fail(Y2_ERR_ARG, "%s: packed2 must be 16-byte aligned", me);
    if ((uintptr_t)dy % 4 || (uintptr_t)dx % 4) return wt_fail(Y2_ERR_ARG, "%s: dy and dx must be 4-byte aligned", me);
    int per, ns;
    const long long tiles = wt_dx_tiles(M, K);
    wt_split(split, tiles, wt_dx_steps(Cout), &per, &ns);
    const size_t need = ns > 1 ? (size_t)ns * M * K * sizeof(float) : 0;
    if (need && (!workspace || workspace_bytes < need))
        return wt_fail(Y2_ERR_ARG, "%s: workspace_bytes = %zu, %d splits of M = %d and K = %d need %zu", me,
                       workspace ? workspace_bytes : (size_t)0, ns, M, K, need);
    if (need && (uintptr_t)workspace % 16) return wt_fail(Y2_ERR_ARG, "%s: workspace is not 16-byte aligned", me);
    if (tiles * ns > 0x7fffffffLL)
        return wt_fail(Y2_ERR_ARG, "%s: M = %d, K = %d: %lld workgroups are beyond one grid", me, M, K, tiles * ns);
    hipLaunchKernelGGL(wide_head_dgrad_kernel, dim3((unsigned)(tiles * ns)), dim3(kWtNT), 0, (hipStream_t)stream, dy,
                       (const char*)packed2, ns > 1 ? (float*)workspace : dx, M, K, Cout, (int)wt_cp2(Cout),
                       (int)wt_up(M, kWtBM), per, ns, grad_scale);
    WTCHK(hipGetLastError());
    if (ns > 1) {
        const size_t n = (size_t)M * K;
        size_t nb = (n + 255) / 256;
        if (nb > 4096) nb = 4096;
        hipLaunchKernelGGL(wide_head_sum_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dx,
                           n, ns, grad_scale);
        WTCHK(hipGetLastError());
    }
    return Y2_OK;
}

int y2_wide_head_backward_filter(const float* x, const float* dy, int M, int K, int Cout, float grad_scale, float* dW, float* db,
                                 void* workspace, size_t workspace_bytes, int split, void* stream) {
    const char* me = "y2_wide_head_backward_filter";
    if (!x || !dy || !dW || !db) return wt_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wt_check(me, K, Cout)) return e;
    if (int e = wt_check_ms(me, M, grad_scale)) return e;
    if (split < 0) return wt_fail(Y2_ERR_ARG, "%s: split = %d: 0 for the plan's, or at least 1", me, split);
    if ((uintptr_t)x % 16) return wt_fail(Y2_ERR_ARG, "%s: x must be 16-byte aligned", me);
    if ((uintptr_t)dy % 4 || (uintptr_t)dW % 4 || (uintptr_t)db % 4)
        return wt_fail(Y2_ERR_ARG, "%s: dy, dW and db must be 4-byte aligned", me);
    int per, ns;
    const long long tiles = wt_dw_tiles(K, Cout);
    wt_split(split, tiles, wt_dw_steps(M), &per, &ns);
    const size_t need = ns > 1 ? (size_t)ns * K * Cout * sizeof(float) : 0;
    if (need && (!workspace || workspace_bytes < need))
        return wt_fail(Y2_ERR_ARG, "%s: workspace_bytes = %zu, %d splits of K = %d and Cout = %d need %zu", me,
                       workspace ? workspace_bytes : (size_t)0, ns, K, Cout, need);
    if (need && (uintptr_t)workspace % 16) return wt_fail(Y2_ERR_ARG, "%s: workspace is not 16-byte aligned", me);
    if (tiles * ns > 0x7fffffffLL)
        return wt_fail(Y2_ERR_ARG, "%s: K = %d, Cout = %d: %lld workgroups are beyond one grid", me, K, Cout, tiles * ns);
    hipLaunchKernelGGL(wide_head_wgrad_kernel, dim3((unsigned)(tiles * ns)), dim3(kWtNT), 0, (hipStream_t)stream, x, dy,
                       ns > 1 ? (float*)workspace : dW, M, K, Cout, (int)wt_up(K, kWtBM), per, ns, grad_scale);
    WTCHK(hipGetLastError());
    if (ns > 1) {
        const size_t n = (size_t)K * Cout;
        size_t nb = (n + 255) / 256;
        if (nb > 4096) nb = 4096;
        hipLaunchKernelGGL(wide_head_sum_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dW,
                           n, ns, grad_scale);
        WTCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(wide_head_db_kernel, dim3((unsigned)wt_up(Cout, 32)), dim3(256), 0, (hipStream_t)stream, dy, db, M, Cout);
    WTCHK(hipGetLastError());
    return Y2_OK;
}

int y2_wide_head_sgd_step(float* W, float* b, float* accum, const float* dW, const float* db, int K, int Cout, void* packed,
                          size_t packed_bytes, void* packed2, size_t packed2_bytes, const void* ctrl, float lr, float momentum,
                          float decay, float grad_mult, void* stream) {
    const char* me = "y2_wide_head_sgd_step";
    if (!W || !b || !accum || !dW || !db || !packed || !packed2) return wt_fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wt_check(me, K, Cout)) return e;
    const float inf = __builtin_huge_valf();
    if (!ctrl && !(lr >= 0.f && lr < inf)) return wt_fail(Y2_ERR_ARG, "%s: lr = %g: finite and >= 0", me, (double)lr);
    if (!(momentum >= 0.f && momentum < 1.f)) return wt_fail(Y2_ERR_ARG, "%s: momentum = %g outside [0, 1)", me, (double)momentum);
    if (!(decay >= 0.f && decay < inf)) return wt_fail(Y2_ERR_ARG, "%s: decay = %g: finite and >= 0", me, (double)decay);
    const size_t need = wt_cp(Cout) * wt_kp(K) * sizeof(half_t), need2 = y2_wide_head_packed2_bytes(K, Cout);
    if (packed_bytes < need)
        return wt_fail(Y2_ERR_ARG, "%s: packed_bytes = %zu, K = %d and Cout = %d need %zu", me, packed_bytes, K, Cout, need);
    if (packed2_bytes < need2)
        return wt_fail(Y2_ERR_ARG, "%s: packed2_bytes = %zu, K = %d and Cout = %d need %zu", me, packed2_bytes, K, Cout, need2);
    if ((uintptr_t)packed % 16 || (uintptr_t)packed2 % 16)
        return wt_fail(Y2_ERR_ARG, "%s: packed and packed2 must be 16-byte aligned", me);
    hipLaunchKernelGGL(wide_head_sgd_kernel, dim3((unsigned)(wt_cp(Cout) / 32), (unsigned)(wt_kp2(K) / 32)), dim3(256), 0,
                       (hipStream_t)stream, W, b, accum, dW, db, (half_t*)packed, (half_t*)packed2, K, Cout, (int)wt_kp(K),
                       (int)wt_cp2(Cout), (const WtCtrlView*)ctrl, lr, momentum, decay, grad_mult);
    WTCHK(hipGetLastError());
    return Y2_OK;
}

}  // extern "C"
