// Weight gradient of a 3x3 convolution with ALL NINE TAPS in one block
// (TF Conv2DBackpropFilter, reference darknet.py:20-21):
//     dW[t][ci][co] = sum_p X[p (+) t][ci] * dY[p][co],   t = (kh, kw)
// The per-tap kernel (wgrad.hip) re-stages X and dY for every tap and is bound by the
// global->LDS fill rate (65 FLOP per staged byte).  Here a block owns a (BI x BO) slice
// of ci x co for all nine taps: per K step it stages ONE dY tile [64 px][BO] and ONE
// X window [64 + 2*pitch + 2 px][BI] of the bordered pixel space; the nine taps read
// row-shifted views of that window.  ~235 FLOP per staged byte at 13x13, 36 MFMAs per
// wave between barriers, and the dY fragment is shared by the nine MFMAs of a k-group.
// K runs linearly over the bordered pixel space (dY border = 0); fragments come out of
// the [pixel][channel] images through ds_read_b64_tr_b16.
#include <stdlib.h>
#include "common.h"
#include "conv_epilogue.h"
#include "kernels.h"

namespace y2 {

// TG = tap groups: with TG = 2 two waves share one (ci, co) tile, taps 0-4 and 5-8 -- twice the
// waves per SIMD at the same accumulator footprint per wave (LDS reads and latency bubbles of
// one wave hide behind the other's MFMAs) and no cross-wave reduction.
// CW = 32-wide co sub-tiles per wave: with CW = 2 every X fragment feeds two MFMAs (1.4 instead of 2.4
// transposed LDS reads per MFMA) and the block stages a dY tile twice as wide per X window (337 instead of
// 144 FLOP per staged byte at 13x13 with 64 ci).
template <typename T, int WI, int WO, int TG = 1, int KS = 1, int CW = 1>
struct Wg9Cfg {
    static constexpr int NW = WI * WO * TG, NT = NW * 64;
    static constexpr int SZ = sizeof(T);
    static constexpr int BI = 32 * WI, BO = 32 * WO * CW;
    static constexpr int BKP = ((SZ == 2) ? 64 : 32) * KS;   // pixels per K step
    static constexpr int ROWX = BI * SZ, ROWY = BO * SZ;
    static constexpr int LPRX = ROWX / 16, LPRY = ROWY / 16;
    static constexpr int RPIX = 64 / LPRX, RPIY = 64 / LPRY;
    static constexpr int NIY = BKP / RPIY;
    static constexpr int IPWY = (NIY + NW - 1) / NW;
    static constexpr int YS = BKP * ROWY;
};

// bank swizzle of the [pixel][channel] images for the transposed 4x16 reads (see wgrad.hip)
template <int ROWB, int SZ>
Y2_DEV int wg9_swz(int row) {
    if (SZ != 2) return 0;
    if (ROWB >= 256) return (row & 3) << 2;
    if (ROWB == 128) return ((row & 3) >> 1) << 2;
    return 0;
}

// NS LDS stages; NS-1 K steps of LDS-DMA stay in flight across the raw barrier (counted vmcnt):
// with one wave per SIMD (as many waves as the dW tiling yields) this is what hides HBM latency.
// PL2 (f16x2 mode, round 5): x and dy are SPLIT tensors -- a cell is [C halves hi][C halves lo] -- and the block forms all
// three plane products itself: both planes of the X window and of the dY tile are staged per K step (2x the LDS of the
// one-plane form) and every fragment pair feeds three MFMAs, hi hi + lo hi + hi lo, into ONE accumulator.  Against
// three launches on plane pairs (WgradArgs::quads; where no two-plane tile fits): 2/3 of the staging and of the LDS
// fragment reads per MFMA, one partial tile per split instead of three.
template <typename T, int WI, int WO, int NS, int TG, int T0, int NTAP, int KS = 1, int CW = 1, bool PL2 = false>
Y2_DEV void wg9_body(const WgradArgs& a, int wrows, char* smem) {
    typedef Wg9Cfg<T, WI, WO, TG, KS, CW> Cfg;
    constexpr int NW = Cfg::NW, SZ = Cfg::SZ, BI = Cfg::BI, BO = Cfg::BO, BKP = Cfg::BKP;
    constexpr int ROWX = Cfg::ROWX, ROWY = Cfg::ROWY;
    constexpr int NPL = PL2 ? 2 : 1;
    static_assert(!PL2 || SZ == 2, "two planes: 16-bit operands");
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = w % (WI * WO);
    const int wi = wq / WO, wo = wq % WO;
    const int pitch = a.W + 1;

    const int nIT = (a.Cin + BI - 1) / BI, nOT = (a.Cout + BO - 1) / BO;
    // split-K launches: the slices of one K range meet in one XCD's L2 (measured +2..7 %); without a split the plain
    // order already gives every XCD a fixed set of co tiles
    int b = xcd_block(blockIdx.x, gridDim.x, a.xcd && a.splitk > 1);
    const int ot = b % nOT; b /= nOT;
    const int it = b % nIT;
    const int split = b / nIT;
    const int ci0 = it * BI, co0 = ot * BO;

    const long Mp = (long)bbody_pixels(a.N, a.H, a.W);
    const long ksteps = (Mp + BKP - 1) / BKP;
    const long spb = (ksteps + a.splitk - 1) / a.splitk;
    const long s_begin = (long)split * spb;
    long s_end = s_begin + spb;
    if (s_end > ksteps) s_end = ksteps;
    const int nsteps = (int)(s_end > s_begin ? s_end - s_begin : 0);

    const int xs_bytes = wrows * ROWX;              // one X window (of one plane)
    const int stage_bytes = NPL * (xs_bytes + Cfg::YS);      // [X hi][X lo][dY hi][dY lo]
    const int xpieces = wrows / Cfg::RPIX;
    const int xplaneB = a.Cin * SZ, yplaneB = a.Cdy * SZ;    // PL2: byte distance of the lo plane inside a cell
    const long kb = s_begin * BKP;
    // window of step s starts at bordered position kb + s*BKP - pitch - 1 (top-left tap)
    const char* xg = (const char*)a.x + ((kb - pitch - 1) * a.xpitch + ci0) * SZ;
    const char* yg = (const char*)a.dy + (kb * a.ypitch + co0) * SZ;
    const long xstep = (long)BKP * a.xpitch * SZ, ystep = (long)BKP * a.ypitch * SZ;

    const int lrx = lane / Cfg::LPRX, lsx = lane % Cfg::LPRX;
    uint32_t voffy[Cfg::IPWY];
#pragma unroll
    for (int i = 0; i < Cfg::IPWY; ++i) {
        const int row = (i * NW + w) * Cfg::RPIY + lane / Cfg::LPRY;
        const int sl = (lane % Cfg::LPRY) ^ wg9_swz<ROWY, SZ>(row);
        voffy[i] = (uint32_t)row * (uint32_t)(a.ypitch * SZ) + sl * 16;
    }
    auto stage = [&](int st, int buf) {
        const char* xs = xg + (long)st * xstep;
        const char* ys = yg + (long)st * ystep;
        char* lb = smem + buf * stage_bytes;
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
            for (int i = w; i < xpieces; i += NW) {
                const int row = i * Cfg::RPIX + lrx;
                const uint32_t off = (uint32_t)row * (uint32_t)(a.xpitch * SZ) + ((lsx ^ wg9_swz<ROWX, SZ>(row)) * 16);
                glds16(xs + pl * xplaneB + off, lb + pl * xs_bytes + i * 1024);
            }
#pragma unroll
            for (int i = 0; i < Cfg::IPWY; ++i) {
                const int ii = i * NW + w;
                if ((i + 1) * NW <= Cfg::NIY || ii < Cfg::NIY)
                    glds16(ys + pl * yplaneB + voffy[i], lb + NPL * xs_bytes + pl * Cfg::YS + ii * 1024);
            }
        }
    };

    f32x16 acc[NTAP][CW];
#pragma unroll
    for (int t = 0; t < NTAP; ++t)
#pragma unroll
        for (int j = 0; j < CW; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[t][j][q] = 0.f;

    const int r32 = lane & 31, hh = lane >> 5;
    const int qq = (lane & 15) >> 2, pp = lane & 3, g1 = (lane >> 4) & 1;
    int shift[NTAP];
#pragma unroll
    for (int t = 0; t < NTAP; ++t) shift[t] = ((T0 + t) / 3) * pitch + ((T0 + t) % 3);

    // loads per wave per stage (the plan makes the X window a multiple of RPIX*NW rows: wg9_wrows)
    const int lps = NPL * (xpieces / NW + Cfg::NIY / NW);
#pragma unroll
    for (int s0 = 0; s0 < NS - 1; ++s0)
        if (s0 < nsteps) stage(s0, s0);
    int cbuf = 0, ibuf = NS - 1;
    for (int st = 0; st < nsteps; ++st) {
        if (st + NS - 2 < nsteps) wait_vmcnt_dyn((NS - 2) * lps);
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (st + NS - 1 < nsteps) stage(st + NS - 1, ibuf);
        const int buf = cbuf;
        cbuf = (cbuf + 1 == NS) ? 0 : cbuf + 1;
        ibuf = (ibuf + 1 == NS) ? 0 : ibuf + 1;
        const char* xs = smem + buf * stage_bytes;
        const char* ys = xs + NPL * xs_bytes;
        if constexpr (SZ == 2) {
            // dY fragment address (no tap shift): rows kg*16 + 8*hh + qq (+4)
            const int fy = wg9_swz<ROWY, SZ>(qq);
            const char* pyb[CW];
#pragma unroll
            for (int j = 0; j < CW; ++j)
                pyb[j] = ys + (8 * hh + qq) * ROWY + ((((wo * CW + j) * 4 + 2 * g1 + (pp >> 1)) ^ fy) * 16) + (pp & 1) * 8;
            // X fragment per tap: row = 8*hh + qq + shift[t]; the swizzle follows the LDS row
            const char* pxb[NTAP];
#pragma unroll
            for (int t = 0; t < NTAP; ++t) {
                const int row = 8 * hh + qq + shift[t];
                const int fx = wg9_swz<ROWX, SZ>(row);
                pxb[t] = xs + row * ROWX + (((wi * 4 + 2 * g1 + (pp >> 1)) ^ fx) * 16) + (pp & 1) * 8;
            }
            // Software pipeline over the k-groups: the fragments of group kg+1 are requested
            // while the nine MFMAs of group kg issue (one wave per SIMD: nothing else hides the
            // ~100-cycle LDS latency; the compiler's own schedule keeps only one fragment ahead).
            typedef typename Elem<T>::frag frag_t;
            frag_t fa0[NPL][NTAP], fa1[NPL][NTAP], fb0[NPL][CW], fb1[NPL][CW];
            auto load_group = [&](int kg, frag_t (&fa)[NPL][NTAP], frag_t (&fb)[NPL][CW]) {
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
                    for (int j = 0; j < CW; ++j) {
                        const char* py = pyb[j] + pl * Cfg::YS + kg * 16 * ROWY;
                        fb[pl][j] = tr_frag<T>(py, py + 4 * ROWY);
                    }
#pragma unroll
                    for (int t = 0; t < NTAP; ++t) {
                        const char* px = pxb[t] + pl * xs_bytes + kg * 16 * ROWX;
                        fa[pl][t] = tr_frag<T>(px, px + 4 * ROWX);
                    }
                }
            };
            auto mma_group = [&](frag_t (&fa)[NPL][NTAP], frag_t (&fb)[NPL][CW]) {
#pragma unroll
                for (int t = 0; t < NTAP; ++t)
#pragma unroll
                    for (int j = 0; j < CW; ++j) {
                        mma32(acc[t][j], fa[0][t], fb[0][j]);
                        if constexpr (PL2) {
                            mma32(acc[t][j], fa[1][t], fb[0][j]);      // x lo * dy hi
                            mma32(acc[t][j], fa[0][t], fb[1][j]);      // x hi * dy lo
                        }
                    }
            };
            load_group(0, fa0, fb0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kg = 0; kg < BKP / 16; kg += 2) {
                load_group(kg + 1, fa1, fb1);
                mma_group(fa0, fb0);
                __builtin_amdgcn_sched_barrier(0);
                if (kg + 2 < BKP / 16) load_group(kg + 2, fa0, fb0);
                mma_group(fa1, fb1);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll 4
            for (int s2 = 0; s2 < BKP / 2; ++s2) {
                const int row = 2 * s2 + hh;
                float fb[CW];
#pragma unroll
                for (int j = 0; j < CW; ++j) fb[j] = *(const float*)(ys + row * ROWY + ((wo * CW + j) * 32 + r32) * 4);
#pragma unroll
                for (int t = 0; t < NTAP; ++t) {
                    const float fa = *(const float*)(xs + (row + shift[t]) * ROWX + (wi * 32 + r32) * 4);
#pragma unroll
                    for (int j = 0; j < CW; ++j) acc[t][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb[j], acc[t][j], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CW; ++j) {
        const int co = co0 + (wo * CW + j) * 32 + r32;
        if (co >= a.Cout) continue;
#pragma unroll
        for (int t = 0; t < NTAP; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int ci = ci0 + wi * 32 + acc_row(q, hh);
                if (ci < a.Cin) {
                    const size_t o = ((size_t)(T0 + t) * a.Cin + ci) * a.Cout + co;
                    if (a.splitk == 1 && a.quads == 1) a.dW[o] = acc[t][j][q] * a.scale;
                    else if (a.slab) a.slab[(size_t)(a.part0 + split) * 9 * a.Cin * a.Cout + o] = acc[t][j][q];
                    else atomicAdd(a.dW + o, acc[t][j][q] * a.scale);
                }
            }
    }
}

template <typename T, int WI, int WO, int NS, int TG, int KS = 1, int CW = 1, bool PL2 = false>
__global__ __launch_bounds__(WI* WO* TG * 64) void wgrad9_kernel(WgradArgs a, int wrows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if constexpr (TG == 1) {
        wg9_body<T, WI, WO, NS, 1, 0, 9, KS, CW, PL2>(a, wrows, smem);
    } else {
        const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if (w < WI * WO) wg9_body<T, WI, WO, NS, 2, 0, 5, KS, CW, PL2>(a, wrows, smem);   // same barrier count in both arms
        else wg9_body<T, WI, WO, NS, 2, 5, 4, KS, CW, PL2>(a, wrows, smem);
    }
}


// ---------------------------------------------------------------------------
// RING form for long image rows (f16/bf16).  The X window of a K step is
// 64 + 2*pitch + 2 bordered pixels; consecutive steps overlap in all but 64 of them, and
// at W = 104 / 208 re-staging the whole window per step costs 4.3x / 7.6x the traffic of the
// step itself (measured: those layers were bound by the global->LDS fill).  Here the X rows
// live in an LDS ring of R = 2^k rows: every step stages only its 64 NEW rows (one aligned
// group), the nine taps read row-shifted views of the ring, and the wrap is one AND on the
// byte offset (v_add + v_and_or per address, hidden in the MFMA shadow).
//   group g = window rows [BKP*g, BKP*(g+1)) (BKP = 64 or 128 pixels per K step); step st reads groups
//   st .. st+G-1, G = ceil(wrows/BKP); group st+G is in flight during step st, so R >= BKP*(G+1).
// ---------------------------------------------------------------------------
template <typename T>
Y2_DEV typename Elem<T>::frag tr_frag_off(uint32_t o0, uint32_t o1) {
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)o0);
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)o1);
    s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(typename Elem<T>::frag, both);
}

template <typename T, int WI, int WO, int TG, int T0, int NTAP, int KS = 1, bool PL2 = false>
Y2_DEV void wg9r_body(const WgradArgs& a, int lgR, int G, char* smem) {
    typedef Wg9Cfg<T, WI, WO, TG, KS> Cfg;
    constexpr int NW = Cfg::NW, SZ = Cfg::SZ, BI = Cfg::BI, BO = Cfg::BO, BKP = Cfg::BKP;
    constexpr int ROWX = Cfg::ROWX, ROWY = Cfg::ROWY;
    constexpr int NPL = PL2 ? 2 : 1;          // PL2: both operand planes of the split-operand mode (see wg9_body)
    static_assert(SZ == 2, "ring form: 16-bit elements");
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = w % (WI * WO);
    const int wi = wq / WO, wo = wq % WO;
    const int pitch = a.W + 1;
    const uint32_t R = 1u << lgR;
    const uint32_t ringB = R * ROWX, maskB = ringB - 1;
    const uint32_t lbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    if (lbase & maskB) __builtin_trap();   // the wrap ORs the column bits into the masked row offset

    const int nIT = (a.Cin + BI - 1) / BI, nOT = (a.Cout + BO - 1) / BO;
    // split-K launches: the slices of one K range meet in one XCD's L2 (measured +2..7 %); without a split the plain
    // order already gives every XCD a fixed set of co tiles
    int b = xcd_block(blockIdx.x, gridDim.x, a.xcd && a.splitk > 1);
    const int ot = b % nOT; b /= nOT;
    const int it = b % nIT;
    const int split = b / nIT;
    const int ci0 = it * BI, co0 = ot * BO;

    const long Mp = (long)bbody_pixels(a.N, a.H, a.W);
    const long ksteps = (Mp + BKP - 1) / BKP;
    const long spb = (ksteps + a.splitk - 1) / a.splitk;
    const long s_begin = (long)split * spb;
    long s_end = s_begin + spb;
    if (s_end > ksteps) s_end = ksteps;
    const int nsteps = (int)(s_end > s_begin ? s_end - s_begin : 0);

    const long kb = s_begin * BKP;
    const char* xg = (const char*)a.x + ((kb - pitch - 1) * a.xpitch + ci0) * SZ;   // window row 0 of step 0
    const char* yg = (const char*)a.dy + (kb * a.ypitch + co0) * SZ;
    const long xstep = (long)BKP * a.xpitch * SZ, ystep = (long)BKP * a.ypitch * SZ;
    char* const ybase = smem + NPL * ringB;      // [ring hi][ring lo][dY: buffer x plane]
    const int xplaneB = a.Cin * SZ, yplaneB = a.Cdy * SZ;

    const int lrx = lane / Cfg::LPRX, lsx = lane % Cfg::LPRX;
    uint32_t voffy[Cfg::IPWY];
#pragma unroll
    for (int i = 0; i < Cfg::IPWY; ++i) {
        const int row = (i * NW + w) * Cfg::RPIY + lane / Cfg::LPRY;
        const int sl = (lane % Cfg::LPRY) ^ wg9_swz<ROWY, SZ>(row);
        voffy[i] = (uint32_t)row * (uint32_t)(a.ypitch * SZ) + sl * 16;
    }
    auto stage_x = [&](int g) {   // BKP rows: BKP / RPIX pieces of 1 KiB (aligned: a piece never wraps)
        const char* xs = xg + (long)g * xstep;
        char* dst = smem + (((uint32_t)g * (uint32_t)BKP * ROWX) & maskB);
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
            for (int i = w; i < BKP / Cfg::RPIX; i += NW) {
                const int row = i * Cfg::RPIX + lrx;   // row & 3 == LDS row & 3 (groups are 64-row aligned)
                const uint32_t off = (uint32_t)row * (uint32_t)(a.xpitch * SZ) + ((lsx ^ wg9_swz<ROWX, SZ>(row)) * 16);
                glds16(xs + pl * xplaneB + off, dst + pl * ringB + i * 1024);
            }
    };
    auto stage_y = [&](int st, int buf) {
        const char* ys = yg + (long)st * ystep;
        char* lb = ybase + buf * NPL * Cfg::YS;
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
            for (int i = 0; i < Cfg::IPWY; ++i) {
                const int ii = i * NW + w;
                if ((i + 1) * NW <= Cfg::NIY || ii < Cfg::NIY) glds16(ys + pl * yplaneB + voffy[i], lb + pl * Cfg::YS + ii * 1024);
            }
    };

    f32x16 acc[NTAP];
#pragma unroll
    for (int t = 0; t < NTAP; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;

    const int r32 = lane & 31, hh = lane >> 5;
    const int qq = (lane & 15) >> 2, pp = lane & 3, g1 = (lane >> 4) & 1;
    // per tap: byte offset of this lane's first row in the ring (advances 64 rows per step) and the
    // constant column part (swizzle follows row & 3, which neither the step nor the wrap changes)
    uint32_t rbB[NTAP], cb[NTAP];
#pragma unroll
    for (int t = 0; t < NTAP; ++t) {
        const int row = 8 * hh + qq + ((T0 + t) / 3) * pitch + ((T0 + t) % 3);
        const int fx = wg9_swz<ROWX, SZ>(row);
        rbB[t] = ((uint32_t)row * ROWX) & maskB;
        cb[t] = lbase | (uint32_t)((((wi * 4 + 2 * g1 + (pp >> 1)) ^ fx) * 16) + (pp & 1) * 8);
    }

    if (nsteps > 0) {
        for (int g = 0; g < G; ++g) stage_x(g);
        stage_y(0, 0);
    }
    for (int st = 0; st < nsteps; ++st) {
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (st + 1 < nsteps) {
            stage_x(st + G);
            stage_y(st + 1, (st + 1) & 1);
        }
        const char* ys = ybase + (st & 1) * NPL * Cfg::YS;
        const int fy = wg9_swz<ROWY, SZ>(qq);
        const char* pyb = ys + (8 * hh + qq) * ROWY + (((wo * 4 + 2 * g1 + (pp >> 1)) ^ fy) * 16) + (pp & 1) * 8;
        typedef typename Elem<T>::frag frag_t;
        frag_t fa0[NPL][NTAP], fa1[NPL][NTAP], fb0[NPL], fb1[NPL];
        auto load_group = [&](int kg, frag_t (&fa)[NPL][NTAP], frag_t (&fb)[NPL]) {
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) {
                const char* py = pyb + pl * Cfg::YS + kg * 16 * ROWY;
                fb[pl] = tr_frag<T>(py, py + 4 * ROWY);
#pragma unroll
                for (int t = 0; t < NTAP; ++t) {
                    // (the second ring starts ringB further: a multiple of the ring size, so the OR of the column bits holds)
                    const uint32_t o0 = (((rbB[t] + (uint32_t)(kg * 16 * ROWX)) & maskB) | cb[t]) + (uint32_t)pl * ringB;
                    const uint32_t o1 = (((rbB[t] + (uint32_t)((kg * 16 + 4) * ROWX)) & maskB) | cb[t]) + (uint32_t)pl * ringB;
                    fa[pl][t] = tr_frag_off<T>(o0, o1);
                }
            }
        };
        auto mma_group = [&](frag_t (&fa)[NPL][NTAP], frag_t (&fb)[NPL]) {
#pragma unroll
            for (int t = 0; t < NTAP; ++t) {
                mma32(acc[t], fa[0][t], fb[0]);
                if constexpr (PL2) {
                    mma32(acc[t], fa[1][t], fb[0]);      // x lo * dy hi
                    mma32(acc[t], fa[0][t], fb[1]);      // x hi * dy lo
                }
            }
        };
        load_group(0, fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kg = 0; kg < BKP / 16; kg += 2) {
            load_group(kg + 1, fa1, fb1);
            mma_group(fa0, fb0);
            __builtin_amdgcn_sched_barrier(0);
            if (kg + 2 < BKP / 16) load_group(kg + 2, fa0, fb0);
            mma_group(fa1, fb1);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int t = 0; t < NTAP; ++t) rbB[t] = (rbB[t] + (uint32_t)BKP * ROWX) & maskB;
    }
    const int co = co0 + wo * 32 + r32;
    if (co < a.Cout) {
#pragma unroll
        for (int t = 0; t < NTAP; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int ci = ci0 + wi * 32 + acc_row(q, hh);
                if (ci < a.Cin) {
                    const size_t o = ((size_t)(T0 + t) * a.Cin + ci) * a.Cout + co;
                    if (a.splitk == 1 && a.quads == 1) a.dW[o] = acc[t][q] * a.scale;
                    else if (a.slab) a.slab[(size_t)(a.part0 + split) * 9 * a.Cin * a.Cout + o] = acc[t][q];
                    else atomicAdd(a.dW + o, acc[t][q] * a.scale);
                }
            }
    }
}

template <typename T, int WI, int WO, int TG, int KS = 1, bool PL2 = false>
__global__ __launch_bounds__(WI* WO* TG * 64) void wgrad9r_kernel(WgradArgs a, int lgR, int G) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if constexpr (TG == 1) {
        wg9r_body<T, WI, WO, 1, 0, 9, KS, PL2>(a, lgR, G, smem);
    } else {
        const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if (w < WI * WO) wg9r_body<T, WI, WO, 2, 0, 5, KS, PL2>(a, lgR, G, smem);
        else wg9r_body<T, WI, WO, 2, 5, 4, KS, PL2>(a, lgR, G, smem);
    }
}


// ---------------------------------------------------------------------------
// The launchers of the two nine-tap families: one tile of the plan (plan_wgrad, wgrad.hip) each
// ---------------------------------------------------------------------------
template <typename T, int WI, int WO, int NS, int TG, int KS, int CW, bool PL2>
static hipError_t wg9_run(const WgradPlan& p, const WgradArgs& a, hipStream_t s) {
    typedef Wg9Cfg<T, WI, WO, TG, KS, CW> Cfg;
    constexpr WgTile t(wgrad_tile(WI, WO, 1, 1, TG, KS, CW, NS, PL2));
    static_assert(Cfg::NIY % Cfg::NW == 0, "dY pieces must split evenly over waves");
    static_assert(wg9_lds(sizeof(T), t, 1) == NS * (PL2 ? 2 : 1) * (Cfg::ROWX + Cfg::YS), "wg9_lds is the kernel's staging");
    static_assert(wg9_wrows(sizeof(T), t, 0) % (NS > 2 ? Cfg::RPIX * Cfg::NW : Cfg::RPIX) == 0, "whole pieces per wave");
    static int attr = 0;
    return wgrad_run(wgrad9_kernel<T, WI, WO, NS, TG, KS, CW, PL2>, attr, p, a, Cfg::NT, s, p.wrows);
}
template <typename T, int WI, int WO, int KS, bool PL2>
static hipError_t wg9r_run(const WgradPlan& p, const WgradArgs& a, hipStream_t s) {
    typedef Wg9Cfg<T, WI, WO, 2, KS> Cfg;
    constexpr WgTile t(wgrad_tile(WI, WO, 1, 1, 2, KS, 1, 2, PL2));
    static_assert(Cfg::NIY % Cfg::NW == 0, "dY pieces must split evenly over waves");
    static_assert(wg9r_lds(sizeof(T), t, 7) == (PL2 ? 2 : 1) * ((Cfg::ROWX << 7) + 2 * Cfg::YS), "wg9r_lds is the kernel's staging");
    static int attr = 0;
    return wgrad_run(wgrad9r_kernel<T, WI, WO, 2, KS, PL2>, attr, p, a, Cfg::NT, s, p.ring_lg, p.ring_g);
}

template <typename T>
static hipError_t wg9_T(const WgradPlan& p, const WgradArgs& a, hipStream_t s) {
#define W9(WI, WO, NS, TG, KS, CW, PL2) \
    case wgrad_tile(WI, WO, 1, 1, TG, KS, CW, NS, PL2): return wg9_run<T, WI, WO, NS, TG, KS, CW, PL2>(p, a, s);
#define WR(WI, WO, KS, PL2) \
    case wgrad_tile(WI, WO, 1, 1, 2, KS, 1, 2, PL2): return wg9r_run<T, WI, WO, KS, PL2>(p, a, s);
    if (p.kind == WK_NINE) {
        switch (p.tile) {
            W9(2, 1, 2, 2, 1, 1, 0)
            W9(2, 1, 2, 2, 2, 1, 0)
            W9(1, 2, 2, 2, 1, 1, 0)
            W9(1, 1, 2, 2, 1, 1, 0)
        }
        if constexpr (sizeof(T) == 2) {
            switch (p.tile) { W9(2, 1, 2, 2, 1, 1, 1) }
        }
#ifdef Y2_DEVBUILD
        if constexpr (std::is_same<T, half_t>::value) {
            switch (p.tile) {
                W9(2, 1, 2, 1, 1, 1, 0)
                W9(1, 2, 2, 1, 1, 1, 0)
                W9(1, 1, 2, 1, 1, 1, 0)
                W9(2, 2, 2, 1, 1, 1, 0)
                W9(2, 2, 3, 1, 1, 1, 0)
                W9(2, 2, 4, 1, 1, 1, 0)
                W9(2, 2, 2, 2, 1, 1, 0)
                W9(2, 2, 3, 2, 1, 1, 0)
                W9(2, 1, 3, 2, 1, 1, 0)
                W9(2, 2, 2, 2, 2, 1, 0)
                W9(1, 2, 2, 2, 2, 1, 0)
                W9(2, 2, 2, 2, 1, 2, 0)
                W9(2, 2, 2, 2, 2, 2, 0)
                W9(2, 1, 2, 2, 1, 2, 0)
                W9(2, 1, 2, 2, 2, 2, 0)
                W9(4, 1, 2, 2, 1, 2, 0)
                W9(4, 1, 2, 2, 2, 2, 0)
                W9(2, 2, 3, 2, 1, 2, 0)
                W9(4, 2, 2, 2, 1, 2, 0)
                W9(2, 1, 3, 2, 1, 2, 0)
            }
        }
#endif
    } else if (p.kind == WK_RING) {
        if constexpr (sizeof(T) == 2) {      // the ring form: 16-bit elements
            switch (p.tile) {
                WR(2, 1, 1, 1)
                WR(1, 2, 1, 1)
                WR(1, 1, 1, 1)
                WR(2, 1, 2, 0)
                WR(1, 2, 2, 0)
                WR(1, 2, 1, 0)
                WR(1, 1, 1, 0)
            }
#ifdef Y2_DEVBUILD
            if constexpr (std::is_same<T, half_t>::value) {
                switch (p.tile) {
                    WR(2, 1, 1, 0)
                    WR(2, 2, 1, 0)
                }
            }
#endif
        }
    }
#undef WR
#undef W9
    return hipErrorInvalidValue;
}

hipError_t launch_wgrad9(int dtype, const WgradPlan& p, const WgradArgs& a0, hipStream_t s) {
    if ((p.kind != WK_NINE && p.kind != WK_RING) || a0.taps != 9) return hipErrorInvalidValue;
    WgradArgs a = a0;
    switch (wgrad_split_args(dtype, a)) {
        case 0: return wg9_T<float>(p, a, s);
        case 1: return wg9_T<half_t>(p, a, s);
        case 2: return wg9_T<bf16_t>(p, a, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace y2
