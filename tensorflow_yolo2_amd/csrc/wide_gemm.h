// The GEMM core of the wide head: what wide_head.hip (forward, pack) and wide_head_train.hip (dx, dW, update) share.
//
//   D[r][c] (+)= sum_k A[r][k] B[c][k]     f16 operands, fp32 accumulate on v_mfma_f32_32x32x16_f16
//
// One workgroup owns a BM x BN tile of D and walks the reduction in steps of 64 elements.  Both operands of a step stand in
// LDS as ROWS of 64 f16 = 128 bytes, the A rows first, then the B rows; two such stages, one barrier per step: the loads of
// step k + 1 are issued behind the barrier, the MFMAs of step k run under them, and what arrived in registers is converted
// and written to the other stage after the MFMAs (wide_main_loop).
//   - 16-byte chunk c of staged row r stands at chunk position c ^ wide_swz(r): two 128-byte rows share a 256-byte bank row,
//     and with the XOR the ds_read_b128 fragment reads are conflict-free as in conv_igemm.hip.
//   - An operand that lies in memory as f16 [rows][pitch] with the reduction contiguous is staged by global_load_lds, the
//     swizzle on the per-lane SOURCE address (WideRows).  An operand that lies there as fp32 goes global -> registers ->
//     v_cvt_pk -> ds_write, the swizzle on the ds_write address (WideQuads, wide_store_quad): no convert pass, no f16 copy.
//   - The accumulator tile keeps the COLUMN on the lane (C/D layout of common.h: col = lane & 31) and the row in the
//     register, so one accumulator register of a wave is two runs of 32 consecutive floats of two rows of D: 128-byte store
//     segments without an LDS round trip, one dword per lane (wide_epilogue; the rows of D are 4-byte aligned only).
// The tile is a template parameter (WideTile); the two instances and which kernel is which stand below it.
// The host half: the one error path, the shape check, the padded sizes of both operand images, the split of a reduction
// across workgroups and the entry both split products go through.  Everything is inline, so each of the two translation
// units (and a stand-alone program linked against one of them) carries what it uses.
#pragma once
#include <stdio.h>
#include <stdarg.h>
#include "common.h"
#include "../../include/yolo2_hip.h"

namespace y2 {
int set_error(int code, const char* msg);   // net.hip (y2_last_error)

// WM x WN waves, each TM x TN MFMA tiles of 32 x 32; everything else follows
template <int WM, int WN, int TM, int TN> struct WideTile {
    static constexpr int kWM = WM, kWN = WN, kTM = TM, kTN = TN;
    static constexpr int kBM = WM * TM * 32, kBN = WN * TN * 32, kBK = 64;   // tile rows, tile columns, reduction step
    static constexpr int kNT = WM * WN * 64;                                 // threads
    static constexpr int kRowB = kBK * 2;                                    // bytes of a staged row: 128
    static constexpr int kStage = (kBM + kBN) * kRowB;
    static constexpr int kLds = 2 * kStage;
    static constexpr int kQuadRows = kNT / 16;                               // A rows one pass of 4-float groups covers
    static constexpr int kPasses = kBM / kQuadRows;                          // 4-float groups per thread and step
    static constexpr int kBInstr = kBN * kRowB / 1024 / (kNT / 64);          // global_load_lds instructions per wave and step
};
// The forward: 256 x 256, 512 threads, 128 KiB.  x is read as fp32, so per step a workgroup loads 64 KiB of x and 32 KiB of
// filters for 2 * 256 * 256 * 64 FLOP; at 128 x 128 the same bytes feed a quarter of the FLOP and the loads, not the matrix
// pipe, bound the launch ("The wide head").
typedef WideTile<2, 4, 4, 2> WideFwdTile;
// Both backward products: 128 x 128, 256 threads, 64 KiB, so two workgroups share a CU ("Training the wide head").
typedef WideTile<2, 2, 2, 2> WideBwdTile;

Y2_DEV int wide_swz(int r) { return (r >> 1) & 7; }

// fragment reads: lane (r32, hh) reads chunk 2 g + hh of row r32 (+ 32 per MFMA tile: the swizzle term of rows 32 apart is
// the same); abase / bbase: the wave's first A and B row in a stage
struct WideFrag {
    int foff[4], abase, bbase, r32, hh, wm, wc;
};
template <class T> Y2_DEV WideFrag wide_frag(int lane, int w) {
    WideFrag f;
    f.r32 = lane & 31;
    f.hh = lane >> 5;
    f.wm = w / T::kWN;
    f.wc = w % T::kWN;
#pragma unroll
    for (int g = 0; g < 4; ++g) f.foff[g] = f.r32 * T::kRowB + (((2 * g + f.hh) ^ wide_swz(f.r32)) << 4);
    f.abase = f.wm * T::kTM * 32 * T::kRowB;
    f.bbase = T::kBM * T::kRowB + f.wc * T::kTN * 32 * T::kRowB;
    return f;
}
// the 64 reduction elements of one stage: acc[i][j] += A rows (registers) x B rows (lanes), for the wave's first `live` row
// tiles (wave-uniform; T::kTM as a constant costs no branch)
template <class T> Y2_DEV void wide_mma_step(f32x16 (&acc)[T::kTM][T::kTN], const char* lb, const WideFrag& f, int live) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f16x8 fa[T::kTM], fb[T::kTN];
#pragma unroll
        for (int j = 0; j < T::kTN; ++j) fb[j] = *(const f16x8*)(lb + f.bbase + j * 32 * T::kRowB + f.foff[g]);
#pragma unroll
        for (int i = 0; i < T::kTM; ++i)
            if (i < live) fa[i] = *(const f16x8*)(lb + f.abase + i * 32 * T::kRowB + f.foff[g]);
#pragma unroll
        for (int i = 0; i < T::kTM; ++i)
            if (i < live) {
#pragma unroll
                for (int j = 0; j < T::kTN; ++j) mma32(acc[i][j], fa[i], fb[j]);
            }
    }
}
template <class T> Y2_DEV void wide_zero(f32x16 (&acc)[T::kTM][T::kTN]) {
#pragma unroll
    for (int i = 0; i < T::kTM; ++i)
#pragma unroll
        for (int j = 0; j < T::kTN; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
}

// The B rows of a tile from an f16 image [rows][pitch bytes] (padded: no mask): instruction i of wave w stages rows
// (w * kBInstr + i) * 8 + lane / 8, lane % 8 the chunk position.  off fits an int in both uses: at most
// 255 rows * 8,192 bytes + 127 (the forward image) and 127 rows * 2^21 bytes + 127 (the second image)
template <class T> struct WideRows {
    const char* base;
    int off[T::kBInstr];
};
template <class T> Y2_DEV WideRows<T> wide_rows(const char* first_row, int pitch, int lane, int w) {
    WideRows<T> b;
    b.base = first_row;
#pragma unroll
    for (int i = 0; i < T::kBInstr; ++i) {
        const int r = (w * T::kBInstr + i) * 8 + (lane >> 3);
        b.off[i] = r * pitch + (((lane & 7) ^ wide_swz(r)) << 4);
    }
    return b;
}
// Step: the integer type the step's byte offset is formed in -- int in the forward, size_t in the data gradient: each keeps
// the address arithmetic it was measured with (profiles/wide_head_refactor.txt section 6)
template <class T, class Step> Y2_DEV void wide_stage_rows(const WideRows<T>& b, int kk, char* stage, int w) {
    char* lbase = stage + T::kBM * T::kRowB;
#pragma unroll
    for (int i = 0; i < T::kBInstr; ++i) glds16(b.base + b.off[i] + (Step)kk * T::kRowB, lbase + (w * T::kBInstr + i) * 1024);
}

// The A rows of a tile from fp32: pass p of a step gives thread (xr, xj) the floats [4 xj, 4 xj + 4) of the step of tile row
// p * kQuadRows + xr; dst[p] is where their four halves stand in a stage
template <class T> struct WideQuads {
    int xr, xj, dst[T::kPasses];
};
template <class T> Y2_DEV WideQuads<T> wide_quads(int tid) {
    WideQuads<T> a;
    a.xr = tid >> 4;
    a.xj = tid & 15;
#pragma unroll
    for (int p = 0; p < T::kPasses; ++p) {
        const int r = p * T::kQuadRows + a.xr;
        a.dst[p] = r * T::kRowB + (((a.xj >> 1) ^ wide_swz(r)) << 4) + ((a.xj & 1) << 3);
    }
    return a;
}
Y2_DEV void wide_store_quad(char* at, float a, float b, float c, float d) {
    *(u32x2*)at = u32x2{pack2<half_t>(a, b), pack2<half_t>(c, d)};
}

// Steps [k0, k1) of the reduction.  issue(k, buf) starts the loads of step k (global_load_lds into stage buf, the rest into
// registers), store(buf) writes the registers' part into stage buf.  kStaged: an operand comes by global_load_lds, so a
// wave waits for its own before the barrier
template <class T, bool kStaged, class Issue, class Store>
Y2_DEV void wide_main_loop(f32x16 (&acc)[T::kTM][T::kTN], const char* smem, const WideFrag& f, int k0, int k1, int live,
                           Issue issue, Store store) {
    issue(k0, 0);
    store(0);
    for (int kk = k0; kk < k1; ++kk) {
        const int cur = (kk - k0) & 1;
        if (kStaged) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's staged rows of step kk have landed
        __syncthreads();                                                // everyone's have, and everyone's written rows; step kk - 1 is read
        const bool more = kk + 1 < k1;
        if (more) issue(kk + 1, cur ^ 1);
        wide_mma_step<T>(acc, smem + cur * T::kStage, f, live);
        if (more) store(cur ^ 1);
    }
}

// The tile's elements inside R x C, one dword per lane: register q of tile (i, j) is row acc_row(q, hh), column r32.
// column(c) is called once per live column and returns what stores (row, value) in it
template <class T, class Column>
Y2_DEV void wide_epilogue(const f32x16 (&acc)[T::kTM][T::kTN], const WideFrag& f, int r0, int c0, int R, int C, Column column) {
#pragma unroll
    for (int j = 0; j < T::kTN; ++j) {
        const int c = c0 + (f.wc * T::kTN + j) * 32 + f.r32;
        if (c >= C) continue;
        auto put = column(c);
#pragma unroll
        for (int i = 0; i < T::kTM; ++i) {
            const int rb = r0 + (f.wm * T::kTM + i) * 32;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int r = rb + acc_row(q, f.hh);
                if (r < R) put(r, acc[i][j][q]);
            }
        }
    }
}

// W [K][Cout] into its two f16 images, 256 threads (tx, ty) = (32, 8) per 32 x 32 tile of W at (k0, c0).  The forward image
// [Cp][Kp] has K contiguous: the tile goes through LDS, tile[k][c] with a 33rd column, reads along Cout, writes along K.
// The second image [Kp2][Cp2] has Cout contiguous, as W has: element by element
Y2_DEV void wide_put_image(const float (&tile)[32][33], half_t* packed, int Kp, int c0, int k0, int tx, int ty) {
#pragma unroll
    for (int r = ty; r < 32; r += 8) packed[(size_t)(c0 + r) * Kp + k0 + tx] = (half_t)tile[tx][r];
}
Y2_DEV void wide_put_image2(half_t* packed2, int Cp2, size_t k, size_t c, float v) { packed2[k * Cp2 + c] = (half_t)v; }

// ---- host

inline int wide_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return set_error(code, buf);
}
#define WIDE_CHK(expr)                                                                           \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) return wide_fail(Y2_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// me == nullptr: no message (the *_bytes entries answer 0)
inline int wide_check(const char* me, int K, int Cout) {
    if (K < 32 || K % 32 || K > Y2_WIDE_HEAD_MAX_K)
        return me ? wide_fail(Y2_ERR_ARG, "%s: K = %d: a multiple of 32, at most %d", me, K, Y2_WIDE_HEAD_MAX_K) : Y2_ERR_ARG;
    if (Cout < 1 || Cout > Y2_WIDE_HEAD_MAX_COUT)
        return me ? wide_fail(Y2_ERR_ARG, "%s: Cout = %d outside 1..%d", me, Cout, Y2_WIDE_HEAD_MAX_COUT) : Y2_ERR_ARG;
    return Y2_OK;
}

inline long long wide_up(long long a, long long b) { return (a + b - 1) / b; }
// the forward image [Cp][Kp]: the forward's B rows; the second image [Kp2][Cp2]: the data gradient's
inline size_t wide_kp(int K) { return (size_t)wide_up(K, WideFwdTile::kBK) * WideFwdTile::kBK; }
inline size_t wide_cp(int Cout) { return (size_t)wide_up(Cout, WideFwdTile::kBN) * WideFwdTile::kBN; }
inline size_t wide_kp2(int K) { return (size_t)wide_up(K, WideBwdTile::kBN) * WideBwdTile::kBN; }
inline size_t wide_cp2(int Cout) { return (size_t)wide_up(Cout, WideBwdTile::kBK) * WideBwdTile::kBK; }

// A backward product: its result [R][C] (with the names the messages use), its tiles and its reduction steps
struct WideProduct {
    const char *rn, *cn;
    int R, C;
    long long tiles, steps;
};
inline WideProduct wide_dx_product(int M, int K, int Cout) {
    typedef WideBwdTile T;
    return {"M", "K", M, K, wide_up(M, T::kBM) * wide_up(K, T::kBN), wide_up(Cout, T::kBK)};
}
inline WideProduct wide_dw_product(int M, int K, int Cout) {
    typedef WideBwdTile T;
    return {"K", "Cout", K, Cout, wide_up(K, T::kBM) * wide_up(Cout, T::kBN), wide_up(M, T::kBK)};
}

constexpr int kWideMaxSplit = 64;                            // bounds the workspace: split x the product's size
// `want` workgroups' worth of splits over `steps` reduction steps -> (steps per split, splits): every split holds a step
inline void wide_normalise(long long want, long long steps, int* per, int* nsplit) {
    if (want > kWideMaxSplit) want = kWideMaxSplit;
    if (want > steps) want = steps;
    if (want < 1) want = 1;
    *per = (int)wide_up(steps, want);
    *nsplit = (int)wide_up(steps, *per);
}
inline int wide_cus() {
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
// the caller's split (0: the plan's for this device) -> (steps per split, splits) and the workspace's bytes
inline size_t wide_split(const WideProduct& p, int split, int* per, int* ns) {
    wide_normalise(split > 0 ? split : wide_up(wide_cus(), p.tiles), p.steps, per, ns);
    return *ns > 1 ? (size_t)*ns * p.R * p.C * sizeof(float) : 0;
}
// A split product: split sp takes steps [sp per, (sp + 1) per) and writes raw fp32 partials [split][R][C] into the
// workspace, then sum(partials, dst, R C, splits) adds them in the order of sp.  No atomics: the same bits every run.  One
// split stores dst itself.  product(workgroups, dst or workspace, per, splits) and sum launch the kernels
template <class Product, class Sum>
int wide_split_product(const char* me, const WideProduct& p, int split, float* dst, void* workspace, size_t workspace_bytes,
                       Product product, Sum sum) {
    int per, ns;
    const size_t need = wide_split(p, split, &per, &ns);
    if (need && (!workspace || workspace_bytes < need))
        return wide_fail(Y2_ERR_ARG, "%s: workspace_bytes = %zu, %d splits of %s = %d and %s = %d need %zu", me,
                         workspace ? workspace_bytes : (size_t)0, ns, p.rn, p.R, p.cn, p.C, need);
    if (need && (uintptr_t)workspace % 16) return wide_fail(Y2_ERR_ARG, "%s: workspace is not 16-byte aligned", me);
    if (p.tiles * ns > 0x7fffffffLL)
        return wide_fail(Y2_ERR_ARG, "%s: %s = %d, %s = %d: %lld workgroups are beyond one grid", me, p.rn, p.R, p.cn, p.C,
                         p.tiles * ns);
    product((unsigned)(p.tiles * ns), ns > 1 ? (float*)workspace : dst, per, ns);
    WIDE_CHK(hipGetLastError());
    if (ns > 1) {
        sum((const float*)workspace, dst, (size_t)p.R * p.C, ns);
        WIDE_CHK(hipGetLastError());
    }
    return Y2_OK;
}

}  // namespace y2
