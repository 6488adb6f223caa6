// Weight-gradient GEMM (TF Conv2DBackpropFilter of darknet.py:20-21):
//     dW[t][ci][co] = sum_p X[p (+) t][ci] * dY[p][co]
// Both operands are pixel-major in HBM (NHWC) and the reduction runs over
// pixels, so the MFMA k index is the slow memory index of BOTH operands.
// gfx950 answer: stage [pixels][channels] tiles with global_load_lds and read
// the fragments with ds_read_b64_tr_b16 (hardware transpose) -- no transposed
// copies of the activations are ever written to HBM.
//
// K runs LINEARLY over the zero-bordered pixel space [0, N*(H+2)*(W+2)):
// dY's border is zero, so border positions contribute nothing and no
// per-pixel index arithmetic is needed (row addresses are affine in k).  The
// tap shift is a constant offset on X; guard bands around the tensors keep the
// shifted reads in finite memory.
// Split-K over blocks; the partial tiles go to a slab and a fixed-order sum (wgrad_reduce_kernel), or are added into
// the fp32 HWIO gradient with float atomics (plan_wgrad, at the end of this file, decides).
#include <stdlib.h>
#include "common.h"
#include "conv_epilogue.h"
#include "kernels.h"

namespace y2 {

// NS = LDS stages: NS - 1 K steps of LDS-DMA stay in flight across the raw barrier (counted vmcnt).  The 1x1
// layers run one workgroup per CU (split-K atomics cost as much as the reads): there a step's 16 MFMAs per wave
// cannot cover the latency of the next step's fetch, and two stages leave the kernel latency-bound.
template <typename T, int WI, int WO, int TI, int TO, int NS = 2>
struct WgCfg {
    static constexpr int NW = WI * WO, NT = NW * 64;
    static constexpr int SZ = sizeof(T);
    static constexpr int BI = WI * TI * 32, BO = WO * TO * 32;
    static constexpr int BKP = (SZ == 2) ? 64 : 32;  // pixels per K step
    static constexpr int ROWX = BI * SZ, ROWY = BO * SZ;
    static constexpr int LPRX = ROWX / 16, LPRY = ROWY / 16;
    static constexpr int RPIX = 64 / LPRX, RPIY = 64 / LPRY;
    static constexpr int NIX = BKP / RPIX, NIY = BKP / RPIY;
    static constexpr int IPWX = NIX / NW, IPWY = NIY / NW;
    static constexpr int XS = BKP * ROWX, YS = BKP * ROWY;
    static constexpr int STAGE = XS + YS;
    static_assert(NIX % NW == 0 && NIY % NW == 0, "staging must split evenly over waves");
};

// swizzle: rows q = row&3 of a transposed 4x16 read must land in distinct
// 64-byte bank segments of the 256-byte LDS bank row
template <int ROWB, int SZ>
Y2_DEV int wg_swz(int row) {
    if (SZ != 2) return 0;
    if (ROWB >= 256) return (row & 3) << 2;
    if (ROWB == 128) return ((row & 3) >> 1) << 2;
    return 0;
}

// PL2 (f16x2 mode): both planes of x and dy staged per K step, the three plane products in one block (wgrad9.hip wg9_body)
template <typename T, int WI, int WO, int TI, int TO, int NS, bool PL2 = false>
__global__ __launch_bounds__(WI* WO * 64) void wgrad_kernel(WgradArgs a) {
    typedef WgCfg<T, WI, WO, TI, TO, NS> Cfg;
    constexpr int NW = Cfg::NW, SZ = Cfg::SZ, BI = Cfg::BI, BO = Cfg::BO, BKP = Cfg::BKP;
    constexpr int ROWX = Cfg::ROWX, ROWY = Cfg::ROWY;
    constexpr int NPL = PL2 ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wi = w / WO, wo = w % WO;

    const int nIT = (a.Cin + BI - 1) / BI, nOT = (a.Cout + BO - 1) / BO;
    int b = xcd_block(blockIdx.x, gridDim.x, a.xcd);
    const int ot = b % nOT; b /= nOT;
    const int it = b % nIT; b /= nIT;
    const int tap = b % a.taps;
    const int split = b / a.taps;
    const int ci0 = it * BI, co0 = ot * BO;

    const long Mp = (long)bbody_pixels(a.N, a.H, a.W);
    const long ksteps = (Mp + BKP - 1) / BKP;
    const long spb = (ksteps + a.splitk - 1) / a.splitk;
    const long s_begin = (long)split * spb;
    long s_end = s_begin + spb;
    if (s_end > ksteps) s_end = ksteps;
    const int nsteps = (int)(s_end > s_begin ? s_end - s_begin : 0);

    int toff;  // tap shift in pixels relative to the centre
    if (a.taps == 9) {
        const int kh = tap / 3, kw = tap - kh * 3;
        toff = (kh - 1) * (a.W + 1) + (kw - 1);
    } else {
        toff = 0;
    }
    const long kb = s_begin * BKP;
    const char* xg = (const char*)a.x + ((kb + toff) * a.xpitch + ci0) * SZ;
    const char* yg = (const char*)a.dy + (kb * a.ypitch + co0) * SZ;
    const long xstep = (long)BKP * a.xpitch * SZ, ystep = (long)BKP * a.ypitch * SZ;

    uint32_t voffx[Cfg::IPWX], voffy[Cfg::IPWY];
#pragma unroll
    for (int i = 0; i < Cfg::IPWX; ++i) {
        const int row = (i * NW + w) * Cfg::RPIX + lane / Cfg::LPRX;
        const int sl = (lane % Cfg::LPRX) ^ wg_swz<ROWX, SZ>(row);
        voffx[i] = (uint32_t)row * (uint32_t)(a.xpitch * SZ) + sl * 16;
    }
#pragma unroll
    for (int i = 0; i < Cfg::IPWY; ++i) {
        const int row = (i * NW + w) * Cfg::RPIY + lane / Cfg::LPRY;
        const int sl = (lane % Cfg::LPRY) ^ wg_swz<ROWY, SZ>(row);
        voffy[i] = (uint32_t)row * (uint32_t)(a.ypitch * SZ) + sl * 16;
    }
    const int xplaneB = a.Cin * SZ, yplaneB = a.Cdy * SZ;      // PL2: byte distance of the lo plane inside a cell
    auto stage = [&](int st, int buf) {
        const char* xs = xg + (long)st * xstep;
        const char* ys = yg + (long)st * ystep;
        char* lb = smem + buf * NPL * Cfg::STAGE;         // [X hi][X lo][dY hi][dY lo]
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
            for (int i = 0; i < Cfg::IPWX; ++i) glds16(xs + pl * xplaneB + voffx[i], lb + pl * Cfg::XS + (i * NW + w) * 1024);
#pragma unroll
            for (int i = 0; i < Cfg::IPWY; ++i)
                glds16(ys + pl * yplaneB + voffy[i], lb + NPL * Cfg::XS + pl * Cfg::YS + (i * NW + w) * 1024);
        }
    };

    f32x16 acc[TI][TO];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TO; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    const int r32 = lane & 31, hh = lane >> 5;
    // transposed-read lane constants (f16/bf16)
    const int qq = (lane & 15) >> 2, pp = lane & 3, g1 = (lane >> 4) & 1;

    constexpr int lps = NPL * (Cfg::IPWX + Cfg::IPWY);     // LDS-DMA pieces per wave and stage
#pragma unroll
    for (int s0 = 0; s0 < NS - 1; ++s0)
        if (s0 < nsteps) stage(s0, s0);
    int cbuf = 0, ibuf = NS - 1;
    for (int st = 0; st < nsteps; ++st) {
        if (st + NS - 2 < nsteps) wait_vmcnt_dyn((NS - 2) * lps);
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();      // step st has landed for every wave; everyone is done with step st - 1's buffer
        asm volatile("" ::: "memory");
        if (st + NS - 1 < nsteps) stage(st + NS - 1, ibuf);
        const int buf = cbuf;
        cbuf = (cbuf + 1 == NS) ? 0 : cbuf + 1;
        ibuf = (ibuf + 1 == NS) ? 0 : ibuf + 1;
        const char* xs = smem + buf * NPL * Cfg::STAGE;
        const char* ys = xs + NPL * Cfg::XS;
        if constexpr (SZ == 2) {
            const int fx = wg_swz<ROWX, SZ>(qq), fy = wg_swz<ROWY, SZ>(qq);
#pragma unroll
            for (int kg = 0; kg < BKP / 16; ++kg) {
                typename Elem<T>::frag fa[NPL][TI], fb[NPL][TO];
                const int row0 = kg * 16 + 8 * hh + qq;
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
                    for (int i = 0; i < TI; ++i) {
                        const int slot = (((wi * TI + i) * 4 + 2 * g1 + (pp >> 1)) ^ fx);
                        const char* p = xs + pl * Cfg::XS + row0 * ROWX + slot * 16 + (pp & 1) * 8;
                        fa[pl][i] = tr_frag<T>(p, p + 4 * ROWX);
                    }
#pragma unroll
                    for (int j = 0; j < TO; ++j) {
                        const int slot = (((wo * TO + j) * 4 + 2 * g1 + (pp >> 1)) ^ fy);
                        const char* p = ys + pl * Cfg::YS + row0 * ROWY + slot * 16 + (pp & 1) * 8;
                        fb[pl][j] = tr_frag<T>(p, p + 4 * ROWY);
                    }
                }
#pragma unroll
                for (int i = 0; i < TI; ++i)
#pragma unroll
                    for (int j = 0; j < TO; ++j) {
                        mma32(acc[i][j], fa[0][i], fb[0][j]);
                        if constexpr (PL2) {
                            mma32(acc[i][j], fa[1][i], fb[0][j]);      // x lo * dy hi
                            mma32(acc[i][j], fa[0][i], fb[1][j]);      // x hi * dy lo
                        }
                    }
            }
        } else {
#pragma unroll
            for (int s2 = 0; s2 < BKP / 2; ++s2) {
                const int row = 2 * s2 + hh;
                float fa[TI], fb[TO];
#pragma unroll
                for (int i = 0; i < TI; ++i) fa[i] = *(const float*)(xs + row * ROWX + ((wi * TI + i) * 32 + r32) * 4);
#pragma unroll
                for (int j = 0; j < TO; ++j) fb[j] = *(const float*)(ys + row * ROWY + ((wo * TO + j) * 32 + r32) * 4);
#pragma unroll
                for (int i = 0; i < TI; ++i)
#pragma unroll
                    for (int j = 0; j < TO; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    // ---- accumulate into fp32 HWIO gradient
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TO; ++j) {
            const int co = co0 + (wo * TO + j) * 32 + r32;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int ci = ci0 + (wi * TI + i) * 32 + acc_row(q, hh);
                if (ci < a.Cin && co < a.Cout) {
                    const size_t o = ((size_t)tap * a.Cin + ci) * a.Cout + co;
                    if (a.splitk == 1 && a.quads == 1) a.dW[o] = acc[i][j][q] * a.scale;
                    else if (a.slab) a.slab[(size_t)(a.part0 + split) * a.taps * a.Cin * a.Cout + o] = acc[i][j][q];
                    else atomicAdd(a.dW + o, acc[i][j][q] * a.scale);
                }
            }
        }
}

// the per-tap family: one tile of the plan
template <typename T, int WI, int WO, int TI, int TO, int NS, bool PL2>
static hipError_t wg_run(const WgradPlan& p, const WgradArgs& a, hipStream_t s) {
    if constexpr (PL2 && sizeof(T) != 2) {
        return hipErrorInvalidValue;      // two planes: 16-bit operands
    } else {
        typedef WgCfg<T, WI, WO, TI, TO, NS> Cfg;
        static_assert(wg_lds(sizeof(T), WgTile(wgrad_tile(WI, WO, TI, TO, 1, 1, 1, NS, PL2))) == (PL2 ? 2 : 1) * NS * Cfg::STAGE,
                      "wg_lds is the kernel's staging");
        static int attr = 0;
        return wgrad_run(wgrad_kernel<T, WI, WO, TI, TO, NS, PL2>, attr, p, a, Cfg::NT, s);
    }
}

template <typename T>
static hipError_t wg_T(const WgradPlan& p, const WgradArgs& a, hipStream_t s) {
#define WT(WI, WO, TI, TO, NS, PL2) \
    case wgrad_tile(WI, WO, TI, TO, 1, 1, 1, NS, PL2): return wg_run<T, WI, WO, TI, TO, NS, PL2>(p, a, s);
#define WT2(WI, WO, TI, TO) WT(WI, WO, TI, TO, 2, 0) WT(WI, WO, TI, TO, 2, 1)
    switch (p.tile) {
        WT2(2, 2, 2, 2)
        WT2(2, 2, 2, 1)
        WT2(4, 1, 1, 1)
        WT2(2, 2, 1, 2)
        WT2(2, 2, 1, 1)
        WT2(2, 1, 1, 1)
        WT2(1, 4, 1, 1)
        WT2(1, 2, 1, 1)
        WT2(1, 1, 1, 1)
#ifdef Y2_DEVBUILD
        WT(2, 2, 2, 2, 3, 0)
        WT(2, 2, 2, 2, 4, 0)
        WT(2, 2, 2, 2, 5, 0)
#endif
    }
#undef WT2
#undef WT
    return hipErrorInvalidValue;
}

hipError_t launch_wgrad(int dtype, const WgradPlan& p, const WgradArgs& a0, hipStream_t s) {
    if (p.kind != WK_TAP) return hipErrorInvalidValue;
    WgradArgs a = a0;
    switch (wgrad_split_args(dtype, a)) {
        case 0: return wg_T<float>(p, a, s);
        case 1: return wg_T<half_t>(p, a, s);
        case 2: return wg_T<bf16_t>(p, a, s);
    }
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------
// Split-K partials: slab[split][taps*Cin*Cout] -> dW = scale * sum over the splits, in split order (deterministic).
// SL = 1: a thread owns four consecutive elements and walks the splits (few splits, large dW);
// SL = 16: 16 lanes share a column group and take every 16th split (hundreds of splits of a tiny dW), LDS add.
// ---------------------------------------------------------------------------
template <int SL>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dW, size_t n4,
                                                           int sk, size_t stride4, float scale) {
    constexpr int COLS = 256 / SL;
    __shared__ f32x4 red[SL > 1 ? 256 : 1];
    const int col = threadIdx.x % COLS, sl = threadIdx.x / COLS;
    const size_t i = (size_t)blockIdx.x * COLS + col;
    const f32x4* p = (const f32x4*)slab;
    f32x4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i < n4) {
        int s = sl;
        // eight splits' loads up front (the kernel runs beside the dgrads: memory latency under that load is what it
        // waits for); every accumulator adds in the order of the four-split loop it replaces: the same bits
        for (; s + 7 * SL < sk; s += 8 * SL) {
            f32x4 r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) r[u] = p[(size_t)(s + u * SL) * stride4 + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u & 3] += r[u];
        }
        for (; s + 3 * SL < sk; s += 4 * SL) {
            f32x4 r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = p[(size_t)(s + u * SL) * stride4 + i];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += r[u];
        }
        for (; s < sk; s += SL) acc[0] += p[(size_t)s * stride4 + i];
    }
    f32x4 t = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    if (SL > 1) {
        red[threadIdx.x] = t;
        __syncthreads();
        if (sl == 0) {
#pragma unroll
            for (int k = 1; k < SL; ++k) t += red[k * COLS + col];
        }
    }
    if (sl == 0 && i < n4) ((f32x4*)dW)[i] = t * scale;
}

hipError_t wgrad_reduce(const WgradPlan& p, const WgradArgs& a, hipStream_t s) {
    const int parts = p.splitk * p.launches;      // f16x2: the three operand-plane pairs are summed like splits
    const size_t n4 = (size_t)a.taps * a.Cin * a.Cout / 4;
    if (p.sum == WS_REDUCE1) {
        hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a.slab, a.dW, n4,
                           parts, n4, a.scale);
    } else if (p.sum == WS_REDUCE16) {
        hipLaunchKernelGGL(wgrad_reduce_kernel<16>, dim3((unsigned)((n4 + 15) / 16)), dim3(256), 0, s, a.slab, a.dW, n4,
                           parts, n4, a.scale);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Kernel policy of the weight gradients: plan_wgrad (below) decides the kernel family, its tile, the operand-plane-pair
// launches, the split-K depth, the route of the partial sums and the dynamic LDS -- host arithmetic only, every LDS fit
// computed here.  launch_wgrad_auto runs its answer.
//
// Measured per shape (scripts/bench_wgrad.py):
//   3x3, rows of 52 and more (16-bit)  : wgrad9r_kernel (ring: 64 new X rows staged per K step instead of the window)
//   3x3, the other rows                : wgrad9_kernel  (nine taps per block on one staged X window)
//   1x1, and 3x3 windows LDS cannot hold : wgrad_kernel (one tap per block)
// ---------------------------------------------------------------------------
constexpr int kWgLdsMax = 160 * 1024;

static long k_steps(const WgradArgs& a, int bkp) { return ((long)bbody_pixels(a.N, a.H, a.W) + bkp - 1) / bkp; }
static int dw_tiles(const WgradArgs& a, const WgTile& t, int taps) {
    return taps * ((a.Cin + t.bi() - 1) / t.bi()) * ((a.Cout + t.bo() - 1) / t.bo());
}
static int clamp_split(long sk, long maxsk) {
    if (sk > maxsk) sk = maxsk;
    return sk < 1 ? 1 : (int)sk;
}
// blocks per CU that LDS allows, at most 3
static int blocks_per_cu(long lds) {
    const long bpc = kWgLdsMax / lds;
    return bpc > 3 ? 3 : (bpc < 1 ? 1 : (int)bpc);
}

// the route of the partial sums, once the split is fixed
static void plan_sum(WgradPlan& p, const WgradArgs& a) {
    static const bool no_slab = getenv("Y2_NO_WGRAD_SLAB") != nullptr;      // A/B switch: float atomics instead
    const int parts = p.splitk * p.launches;
    const size_t n = (size_t)a.taps * a.Cin * a.Cout;
    if (parts <= 1) p.sum = WS_DIRECT;
    else if (!no_slab && a.slab && (n & 3) == 0 && (size_t)parts * n <= a.slab_floats) p.sum = parts <= 8 ? WS_REDUCE1 : WS_REDUCE16;
    else p.sum = WS_ATOMIC;
}

// per-tap kernel.  Split-K target: 1x1 with float atomics -- the partial tiles cost as much as the streaming reads -- one
// block per CU was the optimum, through the slab two per CU are (38 -> 33.5 us at 26x26 / 13x13): 512 blocks where the
// caller lends a slab (read before the slab's size is checked: such a split can still end on atomics), target1 (256)
// otherwise and for the two-plane tiles; 3x3: ~6 per CU
static WgradPlan plan_tap(const WgradArgs& a, int sz, int tile, int launches, int target1) {
    const WgTile t(tile);
    WgradPlan p{};
    if (wg_lds(sz, t) > kWgLdsMax) return p;
    p.kind = WK_TAP;
    p.tile = tile;
    p.launches = launches;
    p.lds = wg_lds(sz, t);
    const int tiles = dw_tiles(a, t, a.taps);
    p.splitk = a.splitk;
    if (p.splitk <= 0) {
        const int target = a.taps == 1 ? (a.slab && target1 == 256 && !t.pl2 ? 512 : target1) : 1536;
        p.splitk = clamp_split((target + tiles - 1) / tiles, (k_steps(a, t.bkp(sz)) + 7) / 8);      // >= 8 K steps per block
    }
    p.blocks = tiles * p.splitk;
    plan_sum(p, a);
    return p;
}

// nine-tap kernel.  Split-K: short image rows (big dW, K = a few thousand steps): two blocks per CU measured best; long rows
// (tiny dW, K = 10^5 steps): ~3 blocks per CU to cover the HBM stream -- but never more blocks than LDS lets a CU hold at
// once (round 4: 28x28 128 -> 256 at batch 128 asked for 768 blocks of 64 KB, 1.5 rounds of the chip: 91 us against 82
// with 512).  blocks_target > 0: that many blocks instead
static WgradPlan plan_nine(const WgradArgs& a, int sz, int tile, int launches, int blocks_target) {
    const WgTile t(tile);
    WgradPlan p{};
    const int wrows = wg9_wrows(sz, t, a.W);
    const int lds = wg9_lds(sz, t, wrows);
    if (lds > kWgLdsMax) return p;
    p.kind = WK_NINE;
    p.tile = tile;
    p.launches = launches;
    p.wrows = wrows;
    const int tiles = dw_tiles(a, t, 1);
    p.splitk = a.splitk;
    if (p.splitk <= 0) {
        long sk = a.W <= 26 ? (512 + tiles / 2) / tiles : (256L * blocks_per_cu(lds) + tiles - 1) / tiles;
        if (blocks_target > 0) sk = (blocks_target + tiles / 2) / tiles;
        p.splitk = clamp_split(sk, (k_steps(a, t.bkp(sz)) + 7) / 8);
    }
    p.blocks = tiles * p.splitk;
    // With no more blocks than CUs, ask for > half of a CU's LDS: the dispatcher then cannot
    // co-locate two blocks on one CU while another CU idles (measured: it does otherwise).
    p.lds = p.blocks <= 256 && lds < 84 * 1024 ? 84 * 1024 : lds;
    plan_sum(p, a);
    return p;
}

// ring kernel.  Split-K: one full wave of resident blocks (256 CUs x blocks per CU by LDS, at most 3: measured best on every
// long-row shape -- 1.5 waves of blocks cost 30 % at 104x104), or blocks_target > 0
static WgradPlan plan_ring(const WgradArgs& a, int sz, int tile, int launches, int blocks_target) {
    const WgTile t(tile);
    WgradPlan p{};
    const int lg = wg9r_lg(sz, t, a.W);
    const long lds = wg9r_lds(sz, t, lg);
    if (lds > kWgLdsMax) return p;
    p.kind = WK_RING;
    p.tile = tile;
    p.launches = launches;
    p.lds = (int)lds;
    p.ring_lg = lg;
    p.ring_g = wg9r_groups(sz, t, a.W);
    const int tiles = dw_tiles(a, t, 1);
    p.splitk = a.splitk;
    if (p.splitk <= 0) {
        const long target = blocks_target > 0 ? blocks_target : 256L * blocks_per_cu(lds);
        // the G-group prologue must stay a small part of a block
        p.splitk = clamp_split(target / tiles, (k_steps(a, t.bkp(sz)) + 4 * p.ring_g - 1) / (4 * p.ring_g));
    }
    p.blocks = tiles * p.splitk;
    plan_sum(p, a);
    return p;
}

static constexpr int nine_tile(int wi, int wo, int ns, int tg, int ks = 1, int cw = 1, int pl2 = 0) {
    return wgrad_tile(wi, wo, 1, 1, tg, ks, cw, ns, pl2);
}
static constexpr int ring_tile(int wi, int wo, int ks, int pl2 = 0) { return wgrad_tile(wi, wo, 1, 1, 2, ks, 1, 2, pl2); }

// 3x3: the nine-tap families; WK_NONE where no tile fits LDS.  launches = 3 (f16x2): the two-plane tiles first.
// Measured (scripts/bench_wgrad.py): narrow co tiles with the taps split over two waves -- many small blocks, two waves per
// SIMD -- beat 64x64 tiles on every Darknet-19 shape
static WgradPlan plan_nine_taps(const WgradArgs& a, int sz, int launches) {
    WgradPlan p{};
#ifdef Y2_DEVBUILD
    static const int minw = getenv("Y2DEV_WG9R_MINW") ? atoi(getenv("Y2DEV_WG9R_MINW")) : 52;
#else
    constexpr int minw = 52;
#endif
    const int wi = a.Cin >= 64 ? 2 : 1, wo = a.Cin < 64 && a.Cdy >= 64 ? 2 : 1;    // 64 x 32, 32 x 64 or 32 x 32 tiles
    if (sz == 2 && a.W >= minw) {
        // long rows.  f16x2: both planes in the ring, 64-pixel K steps (the two rings of the 128-pixel form leave no room
        // at 104 / 208)
        if (launches == 3 && (p = plan_ring(a, sz, ring_tile(wi, wo, 1, 1), 1, 0)).kind) return p;
        // 64 ci x 32 co tiles with 128-pixel K steps measured best at 52 and 104 (3-7 % over 64-pixel steps); 32-channel
        // inputs (208x208): 32 ci x 64 co tiles with 128-pixel K steps where that ring still leaves two blocks per CU
        // (112x112 at batch 128: 90 us against 129; at 208x208 its 96 KB allow one block and the 64-pixel form wins,
        // 160 against 184)
        int ks = wi == 2 ? 2 : 1;
        if (wo == 2 && wg9r_lds(sz, WgTile(ring_tile(1, 2, 2)), wg9r_lg(sz, WgTile(ring_tile(1, 2, 2)), a.W)) <= 80 * 1024) ks = 2;
        if ((p = plan_ring(a, sz, ring_tile(wi, wo, ks), launches, 0)).kind) return p;
    }
    // f16x2: both operand planes staged per K step, 64-pixel K steps so that two blocks still share a CU's LDS
    if (sz == 2 && launches == 3 && a.Cin >= 64 && (p = plan_nine(a, sz, nine_tile(2, 1, 2, 2, 1, 1, 1), 1, 0)).kind) return p;
    // split-K shapes (fewer than 512 dW tiles): K steps of 128 pixels -- half the barriers and a 1.2x instead of 1.4x window at
    // 13x13 (6-8 % faster at 26x26 and on the 512-channel 13x13 layers; the 1024 x 1024 layers, one block per tile, are 2 %
    // faster with 64)
    if (a.Cin >= 64 && sz == 2 && dw_tiles(a, WgTile(nine_tile(2, 1, 2, 2)), 1) < 512 &&
        (p = plan_nine(a, sz, nine_tile(2, 1, 2, 2, 2), launches, 0)).kind)
        return p;
    return plan_nine(a, sz, nine_tile(wi, wo, 2, 2), launches, 0);
}

// 1x1, and the 3x3 windows no nine-tap tile holds: Cin is 32, 64 or a multiple of 128
static WgradPlan plan_per_tap(const WgradArgs& a, int sz, int launches) {
    if (a.Cin % 32 != 0 || (a.Cin > 128 && a.Cin % 128 != 0)) return WgradPlan{};
    const int bi = a.Cin >= 128 ? 128 : a.Cin;
    const int bo = a.Cdy >= 128 ? 128 : (a.Cdy >= 64 ? 64 : 32);
    int wi = 1, wo = 1, ti = 1, to = 1;        // 32 x 32
    if (bi == 128 && bo == 128) wi = 2, wo = 2, ti = 2, to = 2;
    else if (bi == 128 && bo == 64) wi = 2, wo = 2, ti = 2;
    else if (bi == 128) wi = 4;
    else if (bi == 64 && bo == 128) wi = 2, wo = 2, to = 2;
    else if (bi == 64 && bo == 64) wi = 2, wo = 2;
    else if (bi == 64) wi = 2;
    else if (bi == 32 && bo == 128) wo = 4;
    else if (bi == 32 && bo == 64) wo = 2;
    else if (bi != 32) return WgradPlan{};
    // f16x2: both planes staged, the three plane products in one block (one partial per split instead of three) where
    // twice the LDS fits: one block per CU
    if (sz == 2 && launches == 3) {
        const WgradPlan p = plan_tap(a, sz, wgrad_tile(wi, wo, ti, to, 1, 1, 1, 2, 1), 1, 256);
        if (p.kind) return p;
    }
    return plan_tap(a, sz, wgrad_tile(wi, wo, ti, to, 1, 1, 1, 2, 0), launches, 256);
}

WgradPlan plan_wgrad(int dtype, const WgradArgs& a) {
    const int sz = dtype_kbytes(dtype);
    const int launches = dtype == 3 ? 3 : 1;      // f16x2 (not f16x2f: the hi planes alone) -- unless a PL2 tile fits
    if (a.Cin % 32 != 0) return WgradPlan{};
    if (a.taps == 9) {
        const WgradPlan p = plan_nine_taps(a, sz, launches);
        if (p.kind) return p;
    }
    return plan_per_tap(a, sz, launches);
}

hipError_t launch_wgrad_auto(int dtype, const WgradArgs& a0, hipStream_t s) {
    static const int xcd_mode = getenv("Y2_XCD_WGRAD") ? atoi(getenv("Y2_XCD_WGRAD")) : 1;
    WgradArgs a = a0;
    a.xcd = xcd_mode;
    const WgradPlan p = plan_wgrad(dtype, a);
    if (g_launch_log_on.load(std::memory_order_relaxed))
        launch_log_append(1, dtype, (int)p.kind, p.tile, p.splitk > 1, (int)p.sum, 0);
    if (p.kind == WK_TAP) return launch_wgrad(dtype, p, a, s);
    return launch_wgrad9(dtype, p, a, s);
}

#ifdef Y2_DEVBUILD
// development variants (f16) for scripts/bench_wgrad.py: forced plans run by the family launchers.
// 0 / 1: the product policy within the per-tap / nine-tap families; >= 100: per-tap 128 x 128 tiles, stages x the blocks
// target of the 1x1 form
struct WgVariant {
    int id;
    WgradKind kind;
    int tile;
    int target;     // WK_TAP: target1 of plan_tap; the nine-tap families: blocks_target
};
static constexpr int tap_tile(int ns) { return wgrad_tile(2, 2, 2, 2, 1, 1, 1, ns, 0); }
static const WgVariant kWgVariants[] = {
    {100, WK_TAP, tap_tile(2), 256}, {101, WK_TAP, tap_tile(3), 256}, {102, WK_TAP, tap_tile(4), 256},
    {103, WK_TAP, tap_tile(2), 512}, {104, WK_TAP, tap_tile(3), 512}, {105, WK_TAP, tap_tile(5), 256},
    {106, WK_TAP, tap_tile(4), 128}, {107, WK_TAP, tap_tile(2), 768},
    // explicit block shapes: nine_tile(WI, WO, NS, TG, KS, CW)
    {2, WK_NINE, nine_tile(2, 1, 2, 1), 0},
    {3, WK_NINE, nine_tile(1, 2, 2, 1), 0},
    {4, WK_NINE, nine_tile(1, 1, 2, 1), 0},
    {5, WK_NINE, nine_tile(2, 2, 2, 1), 0},
    {6, WK_NINE, nine_tile(2, 2, 2, 1), 0},
    {7, WK_NINE, nine_tile(2, 2, 3, 1), 0},
    {8, WK_NINE, nine_tile(2, 2, 4, 1), 0},
    {9, WK_NINE, nine_tile(2, 2, 2, 2), 0},       // two tap groups, 8 waves
    {10, WK_NINE, nine_tile(2, 2, 3, 2), 0},
    {11, WK_NINE, nine_tile(2, 1, 2, 2), 0},      // 64 x 32 tiles, 4 waves
    {12, WK_NINE, nine_tile(1, 1, 2, 2), 0},      // 32 x 32 tiles, 2 waves
    {13, WK_NINE, nine_tile(1, 2, 2, 2), 0},      // 32 x 64 tiles, 4 waves
    {14, WK_NINE, nine_tile(2, 1, 3, 2), 0},      // 64 x 32, 3 stages
    {16, WK_NINE, nine_tile(2, 1, 2, 1), 0},      // 64 x 32 tiles, 2 waves (no tap split)
    {50, WK_NINE, nine_tile(2, 1, 2, 2, 2), 0},   // 64 x 32, K step of 128 pixels
    {51, WK_NINE, nine_tile(2, 2, 2, 2, 2), 0},   // 64 x 64, 8 waves, K step 128
    {52, WK_NINE, nine_tile(1, 2, 2, 2, 2), 0},
    // two co sub-tiles per wave
    {60, WK_NINE, nine_tile(2, 2, 2, 2, 1, 2), 256},   // 64 ci x 128 co, 8 waves, one block per CU
    {61, WK_NINE, nine_tile(2, 2, 2, 2, 2, 2), 256},   // same, K step 128
    {62, WK_NINE, nine_tile(2, 1, 2, 2, 1, 2), 512},   // 64 ci x 64 co, 4 waves, two blocks per CU
    {63, WK_NINE, nine_tile(2, 1, 2, 2, 2, 2), 512},
    {64, WK_NINE, nine_tile(4, 1, 2, 2, 1, 2), 256},   // 128 ci x 64 co, 8 waves
    {65, WK_NINE, nine_tile(4, 1, 2, 2, 2, 2), 256},
    {66, WK_NINE, nine_tile(2, 2, 3, 2, 1, 2), 256},   // 3 stages
    {67, WK_NINE, nine_tile(4, 2, 2, 2, 1, 2), 256},   // 128 ci x 128 co, 16 waves
    {68, WK_NINE, nine_tile(2, 1, 3, 2, 1, 2), 512},
    {69, WK_NINE, nine_tile(2, 2, 2, 2, 1, 2), 512},   // 64 x 128, two blocks per CU
    // ring form (long rows): ring_tile(WI, WO, KS)
    {30, WK_RING, ring_tile(2, 1, 1), 768},       // 64 x 32, 4 waves
    {31, WK_RING, ring_tile(1, 2, 1), 768},       // 32 x 64, 4 waves
    {32, WK_RING, ring_tile(1, 1, 1), 768},       // 32 x 32, 2 waves
    {33, WK_RING, ring_tile(2, 2, 1), 768},       // 64 x 64, 8 waves
    {34, WK_RING, ring_tile(2, 1, 1), 512},
    {35, WK_RING, ring_tile(1, 2, 1), 512},
    {36, WK_RING, ring_tile(2, 2, 1), 512},
    {37, WK_RING, ring_tile(2, 1, 1), 1024},
    {38, WK_RING, ring_tile(1, 2, 1), 1024},
    {39, WK_RING, ring_tile(2, 2, 1), 1024},
    {40, WK_RING, ring_tile(1, 2, 1), 384},
    {41, WK_RING, ring_tile(1, 2, 1), 256},
    {42, WK_RING, ring_tile(2, 1, 1), 384},
    {43, WK_RING, ring_tile(2, 1, 1), 256},
    {44, WK_RING, ring_tile(1, 2, 2), 0},         // ring, K step 128
    {45, WK_RING, ring_tile(2, 1, 2), 0},
    {46, WK_RING, ring_tile(1, 2, 2), 512},
    {47, WK_RING, ring_tile(2, 1, 2), 512},
};
static hipError_t run_variant(int variant, const WgradArgs& a, hipStream_t s) {
    WgradPlan p{};
    if (variant == 0) p = plan_per_tap(a, 2, 1);
    else if (variant == 1 && a.taps == 9 && a.Cin % 32 == 0) p = plan_nine_taps(a, 2, 1);
    for (const WgVariant& v : kWgVariants) {
        if (v.id != variant) continue;
        if (v.kind == WK_TAP) p = plan_tap(a, 2, v.tile, 1, v.target);
        else if (a.taps == 9) p = v.kind == WK_NINE ? plan_nine(a, 2, v.tile, 1, v.target) : plan_ring(a, 2, v.tile, 1, v.target);
    }
    return p.kind == WK_TAP ? launch_wgrad(1, p, a, s) : launch_wgrad9(1, p, a, s);
}
hipError_t launch_wgrad_variant(int variant, const WgradArgs& a, hipStream_t s) {
    return variant < 2 || variant >= 100 ? run_variant(variant, a, s) : hipErrorInvalidValue;
}
hipError_t launch_wgrad9_variant(int variant, const WgradArgs& a, hipStream_t s) {
    return variant >= 2 && variant < 100 ? run_variant(variant, a, s) : hipErrorInvalidValue;
}
#endif  // Y2_DEVBUILD

}  // namespace y2
