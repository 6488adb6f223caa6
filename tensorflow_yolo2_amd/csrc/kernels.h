// Internal launcher interface between the network executor (net.hip) and the
// gfx950 kernels.  dtype: 0 = f32 (parity mode, exact-f32 MFMA), 1 = f16, 2 = bf16,
// 3 = f16x2 (round 5: split-operand mode -- every MFMA operand is a (hi, lo) pair of halves in two planes of its
// channel row, three f16 MFMAs per product, fp32-width storage everywhere: common.h hsplit_t).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <atomic>
#include "../../include/yolo2_hip.h"

namespace y2 {

//   4 = f16x2f (round 6): LAUNCH dtype of the backward contractions of a split-mode context created with Y2_F16X2F -- the
//       same split tensors, hi planes only, one f16 MFMA per product (common.h hsplith_t).  A context's own dtype is 3.
//   5 = the same contraction (dgrad launches only) with its output dA stored in f16 instead of fp32 (common.h hsplithh_t)
inline size_t dtype_size(int dtype) { return (dtype == 0 || dtype >= 3) ? 4 : 2; }   // bytes per stored element
inline int dtype_kbytes(int dtype) { return dtype == 0 ? 4 : 2; }                  // bytes per element of ONE K plane (MFMA operand)
inline bool dtype_split(int dtype) { return dtype >= 3; }
// dtype of the kernels whose arithmetic is elementwise fp32 in the split mode (first layer, casts): f32
inline int dtype_plain(int dtype) { return dtype >= 3 ? 0 : dtype; }

struct ConvArgs {
    const void* x;      // zero-bordered NHWC [N][H+2][W+2][C]
    const void* w;      // packed [Cout_pad][taps][C]
    void* y;            // [M][ldy]
    const float* bias;  // [Cout] or null
    float* part_cnt;    // [P]            BN partials (null: no statistics)
    float* part_mean;   // [P][ldy]
    float* part_m2;     // [P][ldy]
    int N, H, W, C;
    int M;              // N*H*W
    int Cout;
    int ldy;
    int taps;           // 9 (3x3) or 1 (1x1)
    // dgrad launches only: the batch-norm backward REDUCE pass of the layer below, fused into this epilogue.
    // y (this launch's output) is dA of that layer; with bw_y = its conv output at the same pixels (a pooled
    // layer: at the window's arg-max, BnActArgs::ysel) and its scale / shift the epilogue accumulates
    // S1 = sum g and S2 = sum g * y, g = dA * leaky'(y * scale + shift), per pixel tile:
    // bw_psum[tile][2][ldy] -- what bn_bwd_kernel<.., APPLY = false> would write.
    const void* bw_y = nullptr;       // [M][ldy]
    const float* bw_scale = nullptr;
    const float* bw_shift = nullptr;
    float* bw_psum = nullptr;
    float bw_slope = 0.1f;            // activation slope of that layer (leaky_slope_s)
    // non-null (plain-store launches): set to 1 when a stored value is inf / NaN -- the early overflow guard of
    // y2_backward_adam / _momentum watches the dgrad that feeds the first layer this way
    unsigned* nonfinite = nullptr;
    int xcd = 0;            // XCD-aware workgroup order (common.h xcd_block)
    int is_dgrad = 0;       // the launch computes an input gradient (filters from the dgrad copy): kernel policy only
    // Inference-mode batch norm FOLDED into the epilogue (forward launches of un-pooled layers whose statistics are
    // the moving ones: tf.layers.batch_normalization(training=False) is a fixed per-channel affine,
    // src/yolo2_nets/darknet.py:39-46): the stored value is leaky(T(conv + bias) * scale + shift) -- the same
    // arithmetic on the same rounded conv output as the two-pass form (bn_act_kernel), bit for bit -- written straight
    // into the consumer's bordered tensor aff_out [N][H+2][W+2][ldy]; y is NOT written.  Set with conv_set_affine().
    const float* aff_scale = nullptr;
    const float* aff_shift = nullptr;
    void* aff_out = nullptr;
    float aff_slope = 0.1f;           // activation slope of this layer
    uint32_t aff_magW = 0, aff_magH = 0;   // m / W = (m * magW) >> shW for m < 2^31 (Granlund-Montgomery), same for H
    int aff_shW = 0, aff_shH = 0;
    // POOLED layers in the fold (round 5; conv_haloq kernels, even H and W): the tile's pixels run in WINDOW-MAJOR order
    // q = ((n Ho + ho) Wo + wo) 4 + 2 dh + dw (common.h pool_order_pixel), so a tile holds whole 2x2 windows -- four
    // consecutive rows of the epilogue patch -- and the stored value is leaky(max over the window of T(conv + b) * scale
    // + shift) at the pooled position of aff_out [N][H/2+2][W/2+2][ldy]: bn_act_kernel's pool_window arithmetic
    int aff_pool = 0;
    // K split over workgroups for launches of a few hundred to a few thousand pixels (conv_haloq.hip: haloq_ks): the
    // caller lends ks_floats floats of scratch; plan_conv decides whether and how deep to split (ks_splits: the launcher's)
    float* ks_scratch = nullptr;
    size_t ks_floats = 0;
    int ks_splits = 0;
};
// scratch floats a launch of M pixels x ldy couts may ask for (0: the K split never applies)
size_t conv_ks_scratch_floats(int taps, int M, int ldy, int row_bytes);
inline void conv_div_magic(uint32_t d, uint32_t* mag, int* sh) {
    int l = 0;
    while ((1u << l) < d) ++l;                    // ceil(log2 d)
    *sh = 31 + l;
    *mag = (uint32_t)((((uint64_t)1 << (31 + l)) + d - 1) / d);
}
inline void conv_set_affine(ConvArgs& a, const float* scale, const float* shift, void* out_bordered) {
    a.aff_scale = scale; a.aff_shift = shift; a.aff_out = out_bordered;
    conv_div_magic((uint32_t)a.W, &a.aff_magW, &a.aff_shW);
    conv_div_magic((uint32_t)a.H, &a.aff_magH, &a.aff_shH);
}

// ---- conv kernel policy (conv_halo.hip): plan_conv decides every forward / dgrad launch, the launchers execute its answer
enum ConvKind {
    CK_RF,          // conv_rf.hip: filters resident in registers, 208-wide 32 <-> 64 layers (cfg 1, 2)
    CK_RFN,         //   ... the 128-cout form (cfg 3; development build: cfg 4, Y2DEV_RF_ALT=1)
    CK_HALOQ,       // conv_haloq.hip: halo image in LDS, filter fragments straight to registers
    CK_HALOQ_KS,    //   ... K split over workgroups + conv_ks_finish (launches of a few hundred pixels)
    CK_HALO,        // conv_halo.hip: halo image + LDS filter ring
    CK_IGEMM,       // conv_igemm.hip: per-tap staging (every 1x1, the 208-wide 3x3 forwards)
    CK_IGEMM_KS,    //   ... K split of the small 1x1 launches
};
struct ConvPlan {
    ConvKind kind;
    int cfg;            // rf: config 1-3; the other kinds: a conv_tile() (development build: a conv_halo variant number)
    int filter_layout;  // what the filter pack must hold: 0 K-contiguous rows, 1 32-row / 2 16-row MFMA fragments
    int block_pixels;   // pixels per tile (the BN partial records of the non-rf kinds cover one tile each)
    int ks_depth;       // K splits of the *_KS kinds (after the scratch-size clamp), else 1
    int records;        // BN partial records a launch with statistics writes (rf kinds: one per workgroup)
    int rf_tiles;       // rf kinds: tiles per workgroup of the persistent grid (records = workgroups over the pixels)
    int lds;            // rf kinds: dynamic LDS bytes of a workgroup (rf_lds / rfn_lds)
};
// LDS of the register-filter kernels (conv_rf.hip; sz = bytes of an element, C = input channels).  plan_conv sizes the
// persistent grid with them; the launchers check them against their kernel's layout at compile time.
//   rf: a ring of 4 groups of bp rows, per wave an epilogue patch of pr rows + doubles S1, S2 and a count, the bias slice
constexpr int rf_lds(int sz, int C, int nct, int wp, int tp, int pr) {
    return 4 * wp * tp * 32 * C * sz + wp * pr * (nct * 32 * sz + 16) + wp * (2 * nct * 32 + 2) * 8 + nct * 32 * 4;
}
//   rfn: a ring of nslot groups, one [bp][bc] patch, the waves' statistics, row table and bias slice; bw (the fused
//   BN-backward reduce of the layer below): + that layer's conv output tile and its scale / shift
constexpr int rfn_lds(int sz, int C, int wp, int wn, int tp, int nslot, bool bw) {
    const int bp = wp * tp * 32, bc = wn * 32, nw = wp * wn;
    return nslot * bp * C * sz + bp * (bc * sz + 16) + 2 * (nw * 2 * bc + nw) * 4 + bp * 4 + bc * 4 +
           (bw ? bp * bc * sz + 2 * bc * 4 : 0);
}
// a kernel tile as one int: waves over pixels x couts, 32-wide MFMA units per wave, K-chunk bytes (64 / 128) and one
// family field (haloq: 16x16 MFMA tiles; halo, igemm: stages of the ring)
constexpr int conv_tile(int wp, int wc, int tp, int tc, int bkb, int aux) {
    return wp | wc << 4 | tp << 8 | tc << 12 | (bkb / 64) << 16 | aux << 20;
}
struct ConvTile {
    int wp, wc, tp, tc, bkb, aux;
    explicit ConvTile(int t)
        : wp(t & 15), wc((t >> 4) & 15), tp((t >> 8) & 15), tc((t >> 12) & 15), bkb(((t >> 16) & 15) * 64), aux(t >> 20) {}
    int bp() const { return wp * tp * 32; }
    int bc() const { return wc * tc * 32; }
};
// no HIP calls, no side effects
ConvPlan plan_conv(int dtype, const ConvArgs& a);
// plan_conv + the launch; filter_layout = the layout the filters were packed in (hipErrorInvalidValue unless the plan's)
hipError_t launch_conv(int dtype, const ConvArgs& a, hipStream_t s, int filter_layout);
// ---- launch log (conv_halo.hip; host memory only, y2_launch_log_* in yolo2_hip.h): while it is on, launch_conv and
// launch_wgrad_auto -- the only two doors to these kernels -- append the form key of each launch: what selects a kernel
// instantiation or a distinct code path inside one.  Off (the default) it costs the launchers one branch.
//   conv : {0, launch dtype, is_dgrad, ConvPlan.kind, ConvPlan.cfg, K split, epilogue (0 plain, 1 BN statistics, 2 fused
//           BN-backward reduce)}
//   wgrad: {1, launch dtype, WgradPlan.kind, WgradPlan.tile, splitk > 1, WgradPlan.sum, 0}
// (the folded-inference epilogue, aff_*, is not part of the key: DESIGN section 4)
extern std::atomic<bool> g_launch_log_on;
void launch_log_append(int op, int dtype, int f2, int f3, int f4, int f5, int f6);
void launch_log_enable(bool on);                        // on: clears the log first
int launch_log_read(int* out, int max_records);         // -> records logged; copies min(that, max_records) of them
// the family launchers (launch_conv's switch): hipErrorInvalidValue for a plan they cannot run
hipError_t launch_conv_rf(int dtype, const ConvPlan& p, const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_haloq(int dtype, const ConvPlan& p, const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_halo(int dtype, const ConvPlan& p, const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_igemm(int dtype, const ConvPlan& p, const ConvArgs& a, hipStream_t s);
// rows of the LDS image of the halo kernels over all tiles of a launch (pool: window-major tiles, ConvArgs::aff_pool)
int halo_image_rows(int H, int W, int BP, int RPI, int pool = 0);
int conv_block_couts(int Cout);
// MXFP8 inference forms (conv_mx8.hip, public Y2_FP8): e4m3fn elements + one E8M0 scale byte per 32 values
int mx8_block_couts();                 // output channels per workgroup: the filter pack pads Cout to a multiple of it
int mx8_channels(int C);               // channel stride of the e4m3 tensors and filters (a multiple of the K step)
// the MXFP8 epilogue's destination: the consumer's bordered e4m3 input q [cell][ldq] and scales sc [cell][ldq / 32]
// (cell-0 pointers)
struct Mx8Out {
    uint8_t* q = nullptr;
    uint8_t* sc = nullptr;
    int ldq = 0;
};
// a: the forward launch (x = e4m3 bordered tensor at cell 0, C = its channel stride, w = packed e4m3 filters); xsc = the
// scale plane [bordered pixel][C / 32] at cell 0, wsc = [Cout_pad][taps][C / 32]; out_f32: y is fp32, else f16 (y or aff_out);
// qo (non-null, with the folded batch norm set): the output is quantised into the consumer's e4m3 input instead
hipError_t launch_conv_mx8(int out_f32, const ConvArgs& a, const uint8_t* xsc, const uint8_t* wsc, const Mx8Out* qo,
                           hipStream_t s);
hipError_t launch_mx_unpack(const uint8_t* q, const uint8_t* sc, float* out, int N, int H, int W, int C, int Cs,
                            hipStream_t s);
// [rows][ldin] fp32 or f16 -> e4m3 [rows][ldq] + scales [rows][ldq / 32] (blocks beyond ldin: zero)
hipError_t launch_mx_quantize(int in_f16, const void* x, size_t rows, int ldin, int ldq, uint8_t* q, uint8_t* sc,
                              hipStream_t s);
// fp32 HWIO -> e4m3 [Cout_pad][taps][C8] + scales [Cout_pad][taps][C8 / 32]
hipError_t launch_mx_pack_filter(const float* w, int taps, int Cin, int Cout, int Cout_pad, int C8, uint8_t* q,
                                 uint8_t* sc, hipStream_t s);

// ---- first layer (Cin = 3, stored as 4 channels)
// plan_conv1 (conv1_wgrad.hip) decides every pass of the layer; the launchers run the planned form and return
// hipErrorInvalidValue for one the plan never produces
enum Conv1Fwd {
    C1F_PLAIN,      // conv1_fwd_kernel stores y (+ statistics), then the generic batch-norm passes
    C1F_POOLED,     // statistics (Conv1Stats), then conv1_pool_kernel: conv again + BN + leaky + 2x2 max pool
};
enum Conv1Stats {
    C1S_NONE,       // inference moments (or the plain route: conv1_fwd_kernel's own partials)
    C1S_CONV,       // conv1_stats_kernel: a statistics-only conv pass + bn_finalize
    C1S_GRAM,       // launch_conv1_gram_stats: from the Gram matrix of the input patches, kept for the backward pass
};
enum Conv1Keep {    // what the forward pass keeps for the backward pass
    C1K_NONE,
    C1K_Y,          // the conv output y [M][32]
    C1K_YSEL,       // conv output at the window's arg-max + 2 index bits (Conv1PoolArgs::ysel / idx)
    C1K_IDX3,       // 3 index bits per element (Conv1PoolArgs::idx3)
};
enum Conv1Bwd {
    C1B_GENERIC,    // bn_bwd reduce + apply -> dy, conv1_wgrad_kernel
    C1B_RECOMPUTE,  // conv1_bnbwd_reduce_kernel (conv output recomputed), generic apply, conv1_wgrad_kernel
    C1B_FUSED,      // generic reduce, apply fused into conv1_wgrad_fused_kernel
    C1B_LINEAR,     // conv1_wgrad_lin_kernel (+ the reduce) and conv1_dw_finalize: no conv output read
};
struct Conv1Plan {
    int T;              // element type of the kernels: dtype_plain (the split mode's are fp32)
    Conv1Fwd fwd;
    Conv1Stats stats;
    Conv1Keep keep;
    Conv1Bwd bwd;
    int xs_fwd;         // split-operand products of the statistics and pool passes (f16x2 mode): 0 / 1
    int xs_bwd;         // ... of the linear backward: 0, 1 (three products), 2 (f16x2f: hi planes only)
    int lin_gram;       // C1B_LINEAR: 1 the kernel builds G, 0 it reads the forward pass's Gram totals
    int lin_nseg, lin_ws;       // C1B_LINEAR: column segments of a row pair and their width (Conv1WgradLinArgs)
    int lin_records;    // C1B_LINEAR: BN-backward partial records written (the blocks, + the S2 record of C1K_IDX3)
    int fwd_blocks;     // conv1_fwd_kernel / conv1_stats_kernel (= statistics records)
    int pool_blocks;    // conv1_pool_kernel, conv1_bnbwd_reduce_kernel
    int gram_rt, gram_blocks, gram_lds;     // conv1_gram_kernel: output rows per tile, grid, LDS
    int bwd_blocks, bwd_lds;    // the weight-gradient kernel of the route
    size_t ysel_bytes, idx_bytes, lin_bytes, gram_bytes;    // workspace of a training binding (0: not used)
    bool y_stored, dy_stored;   // the conv output / its gradient exist in memory after the pass
};
// no HIP calls, no side effects.  trains: the binding trains; has_next: a layer follows; training: BN mode of the forward
// being planned (the backward pass plans with the last forward's)
Conv1Plan plan_conv1(int dtype, int bwd_dtype, int N, int H, int W, int pool, int cout, int ldy, bool trains, bool has_next,
                     bool training);
// LDS of the row-image kernels: dy_rows rows of wp pixels x 32 channels and x_rows rows of wp + 4 pixels x 4 channels
// (isz bytes per element); the closing reductions of the waves reuse it
constexpr int kC1LdsMax = 160 * 1024;
constexpr int c1_images(int dy_rows, int x_rows, int wp, int isz) {
    return dy_rows * wp * 32 * isz + x_rows * (((wp + 4) * 4 * isz + 15) & ~15);
}
constexpr int c1_atleast(int lds, int red) { return lds > red ? lds : red; }
//   conv1_wgrad_kernel: one dy row + three x rows; [4 waves][48][32] floats
constexpr int c1wg_lds(int sz, int W) { return c1_atleast(c1_images(1, 3, (W + 15) & ~15, sz), 4 * 48 * 32 * 4); }
//   conv1_wgrad_fused_kernel: two dy rows + four x rows
constexpr int c1wgf_lds(int sz, int W) { return c1_atleast(c1_images(2, 4, (W + 15) & ~15, sz), 4 * 48 * 32 * 4); }
//   conv1_wgrad_lin_kernel: two dz rows + four x rows of a wp-pixel unit (isz 2 where the images hold halves);
//   [4 waves][48*32 + 48*48] floats
constexpr int c1lin_lds(int isz, int wp) { return c1_atleast(c1_images(2, 4, wp, isz), 4 * (48 * 32 + 48 * 48) * 4); }
//   conv1_gram_kernel: two buffers of rt + 2 x rows (32-pixel groups, halves); [4 waves][48][48] floats
constexpr int c1gram_lds(int rt, int W) { return c1_atleast(2 * c1_images(0, rt + 2, (W + 31) & ~31, 2), 4 * 48 * 48 * 4); }

struct Conv1Args {
    const void* x4;     // [N][H+2][W+2][4]
    const void* w;      // packed [32][3][16] (kh, then kw*4+c, 12 real + 4 zero)
    void* y;            // [M][32]
    const float* bias;
    float* part_cnt;    // [Conv1Plan::fwd_blocks] statistics partials
    float* part_mean;
    float* part_m2;
    int N, H, W, M;
};
// C1F_PLAIN: conv1_fwd_kernel; C1F_POOLED + C1S_CONV: the statistics-only pass (y is not written; Conv1Plan::xs_fwd: the
// fp32 operands are split into half planes in registers and a filter row is three f16 matrix instructions)
hipError_t launch_conv1_fwd(const Conv1Plan& p, const Conv1Args& a, hipStream_t s);
// pooled first layer, second pass: conv again + BN + leaky + 2x2 max pool -> the pooled output and what Conv1Plan::keep says
struct Conv1PoolArgs {
    const void* x4;
    const void* w;
    void* y;            // [M][32] (C1K_Y)
    const float* bias;
    const float *scale, *shift;
    void* out;          // zero-bordered [N][Ho+2][Wo+2][32] of T
    int N, H, W;
    // C1K_YSEL: instead of the conv output (64 B/pixel) keep, per pooled pixel, the conv output at the window's first
    // arg-max (ysel [Mout][32] of T) and WHICH of the four positions it was (idx [Mout][chunks] u16: 2 bits per channel
    // of a 16-byte chunk)
    void* ysel = nullptr;
    unsigned short* idx = nullptr;
    // C1K_IDX3 (round 4): NO conv output at all is kept.  idx3 [Mout][chunks] u32 holds 3 bits per channel of a chunk:
    // the window position (2) and whether the activation there took the leaky branch (1: 0.1 * z >= z).  That is all the
    // backward pass needs per element (g = dA * slope, scattered to that position); its sum of g * y follows from the
    // linearity of y in the filter: sum_p dz y = sum_k W[k] X(dz)[k] + b sum dz, with X(dz) the matrix the weight
    // gradient forms anyway (conv1_wgrad.hip conv1_lin_s2_kernel)
    unsigned* idx3 = nullptr;
    int out_split = 0;  // f16x2 mode (T = float kernels): `out` is a split tensor ([32 halves hi][32 halves lo] per cell)
};
hipError_t launch_conv1_pool(const Conv1Plan& p, const Conv1PoolArgs& a, hipStream_t s);
// C1B_RECOMPUTE: backward reduce pass of the same layer with the conv output recomputed (x4 + dA in, psum out)
struct Conv1BnBwdArgs {
    const void* x4;
    const void* w;
    const float* bias;
    const float *scale, *shift;
    const void* dA;     // grad wrt the pooled output [N*Ho*Wo][32] of T
    float* psum;        // [Conv1Plan::pool_blocks][2][32]
    int N, H, W;
};
hipError_t launch_conv1_bnbwd_reduce(const Conv1Plan& p, const Conv1BnBwdArgs& a, hipStream_t s);
// C1B_GENERIC, C1B_RECOMPUTE
struct Conv1WgradArgs {
    const void* x4;     // [N][H+2][W+2][4]
    const void* dy;     // zero-bordered [N][H+2][W+2][32]
    float* dW;          // [3][3][3][32] fp32, accumulated with atomics (pre-zeroed)
    int N, H, W, M;
    float scale;        // 1 / grad_scale
};
hipError_t launch_conv1_wgrad(const Conv1Plan& p, const Conv1WgradArgs& a, hipStream_t s);
// C1B_FUSED: BN-backward apply fused into the weight gradient (dy never reaches HBM)
struct Conv1WgradFusedArgs {
    const void* x4;       // [N][H+2][W+2][4]
    const void* y;        // conv output [M][32]
    const void* dA;       // grad wrt the pooled layer output [N*Ho*Wo][32]
    const float *scale, *shift;
    const float* coef;    // [2][32]: ka, kb (bn_bwd_finalize)
    float* dW;            // [3][3][3][32] fp32, atomics (pre-zeroed)
    int N, H, W;
    float inv_grad_scale;
};
hipError_t launch_conv1_wgrad_fused(const Conv1Plan& p, const Conv1WgradFusedArgs& a, hipStream_t s);
// C1B_LINEAR (no conv output of the first layer in HBM at all).  With dy = scale dz - (ka + kb y):
//     dW = scale * X(dz) - ka * X(1) - kb * X(y),   X(v)[t][c][co] = sum_p x[p + t][c] v[p][co]
// and y = conv(x, W) + b:  X(y) = G W + b X(1),  G = the Gram matrix of the 27-element input patches
// (weights-independent).  The kernel accumulates X(dz) [48][32] and G [48][48] (rows kh*16 + kw*4 + c; channel 3
// of the stored input is 1 inside the image, so G's row of the centre tap's channel 3 IS X(1)); a one-block
// finalize combines them with the BN-backward constants.
struct Conv1WgradLinArgs {
    const void* x4;             // [N][H+2][W+2][4], channel 3 = 1 inside the image
    const void* dA;             // [Mout][32] of T
    const void* ysel;           // [Mout][32] of T (C1K_YSEL)
    const unsigned short* idx;  // [Mout][chunks]
    const float *scale, *shift;
    // C1K_IDX3: Wf (fp32 HWIO [3][3][3][32]) and bias for sum g * y = W . X(dz) + b sum dz, written as one more psum record
    // (S1 = 0) behind the blocks' records
    const unsigned* idx3 = nullptr;
    const float* Wf = nullptr;
    const float* bias = nullptr;
    float* acc;                 // 16 slice sums of [48*32 + 48*48], followed by the per-block partials (Conv1Plan::lin_bytes)
    float* psum;                // out: BN-backward partial sums [blocks][2][32] (S1, S2) -- the reduce pass rides here
    int N, H, W;
    // set by the launcher (Conv1Plan::lin_nseg / lin_ws): a row pair is worked in nseg column segments of ws pixels (a
    // multiple of 16) so that the LDS row images of the fp32-wide form leave room for two workgroups per CU (8-byte
    // aligned: one scalar load for the pair)
    alignas(8) int nseg = 1;
    int ws = 0;
};
struct Conv1DwFinalizeArgs {
    const float* acc;           // the 16 slice sums (added here)
    const float* W;             // fp32 HWIO [3][3][3][32]
    const float* bias;
    const float* scale;
    const float* coef;          // [2][32] ka, kb
    float* dW;                  // out [3][3][3][32]
    float inv_grad_scale;
    const float* gram = nullptr; // [48][48] Gram totals of the forward pass (Conv1Plan::lin_gram 0; else: the G part of acc)
};
// C1S_GRAM: Gram matrix of the input patches -> batch-norm statistics of the layer (conv1_wgrad.hip: replaces the
// statistics-only convolution pass + bn_finalize) and the totals the backward pass reuses.
// mid: Conv1Plan::gram_bytes = [1 + 16 + 768][48*48] floats: gram totals, slices, block partials.
struct Conv1GramStatsArgs {
    const void* x4;             // [N][H+2][W+2][4], channel 3 = 1 inside the image
    int N, H, Wd;
    const float* W;             // fp32 HWIO [3][3][3][32]
    const float* bias;
    const float *gamma, *beta;
    float *moving_mean, *moving_var;
    float *scale, *shift, *mean, *invstd, *var;
    float eps, momentum;
    int update_moving, bessel;
    float* mid;                 // slices + partials (scratch)
    float* gram;                // out: [48][48] totals
};
hipError_t launch_conv1_gram_stats(const Conv1Plan& p, const Conv1GramStatsArgs& a, hipStream_t s);
hipError_t launch_conv1_wgrad_lin(const Conv1Plan& p, const Conv1WgradLinArgs& a, hipStream_t s);
hipError_t launch_conv1_dw_finalize(const Conv1DwFinalizeArgs& a, hipStream_t s);

// ---- weight-gradient GEMM  dW[t][ci][co] = scale * sum_p X[p+t][ci] * dY[p][co]
struct WgradArgs {
    const void* x;      // zero-bordered [N][H+2][W+2][Cin]
    const void* dy;     // zero-bordered [N][H+2][W+2][Cdy]
    float* dW;          // [taps][Cin][Cout] fp32 (HWIO)
    int N, H, W, M;
    int Cin, Cdy, Cout; // Cdy = channel stride of dy (>= Cout)
    int taps;
    int splitk;         // 0: plan_wgrad decides (the launchers pass the plan's)
    float scale;
    int xcd = 0;        // XCD-aware workgroup order (common.h xcd_block)
    // split-K partial tiles: with a slab of at least splitk * taps*Cin*Cout floats per launch the splits store their
    // partials there (plain stores) and wgrad_reduce_kernel sums them in a fixed order into dW -- deterministic, and no
    // zero-fill of dW; without one they are added into a zeroed dW with float atomics (≈1.3 TB/s chip-wide)
    float* slab = nullptr;
    size_t slab_floats = 0;
    // f16x2 mode: x / dy are split tensors, read by the 16-bit kernels with xpitch / ypitch = elements of the operand
    // type per pixel (2 Cin / 2 Cdy).  Where no two-plane tile fits, one launch per operand-plane pair (hi hi, lo hi,
    // hi lo -- `quads` = 3), every launch's partial tiles in its own range of the slab; ONE fixed-order sum over
    // quads * splitk partials
    int xpitch = 0, ypitch = 0;     // 0: Cin / Cdy
    int quads = 1;          // plane-pair launches (WgradPlan::launches); set by the launchers
    int part0 = 0;          // slab slot of this launch's split 0 (q * splitk); set by wgrad_run
};
// f16x2: the split form of a (x, dy) pair for the 16-bit kernels (dtype 3, 4 -> 1)
inline int wgrad_split_args(int dtype, WgradArgs& a) {
    if (!a.xpitch) a.xpitch = a.Cin;
    if (!a.ypitch) a.ypitch = a.Cdy;
    if (!dtype_split(dtype)) return dtype;
    a.xpitch = 2 * a.Cin; a.ypitch = 2 * a.Cdy;
    return 1;
}

// ---- weight-gradient policy (wgrad.hip): plan_wgrad decides every launch, the family launchers execute its answer
enum WgradKind {
    WK_NONE,        // no kernel takes the shape: the launch returns hipErrorInvalidValue
    WK_TAP,         // wgrad.hip wgrad_kernel: one tap per block
    WK_NINE,        // wgrad9.hip wgrad9_kernel: all nine taps per block, the X window staged per K step
    WK_RING,        // wgrad9.hip wgrad9r_kernel: all nine taps per block, the X rows in an LDS ring (16-bit, long rows)
};
enum WgradSum {
    WS_DIRECT,      // one partial per dW element: the kernel stores it
    WS_REDUCE1,     // partials in the slab, slot q * splitk + split; wgrad_reduce_kernel<1> (up to 8 partials)
    WS_REDUCE16,    //   ... wgrad_reduce_kernel<16> (more)
    WS_ATOMIC,      // float atomics into a zeroed dW (no slab lent, too small, or Y2_NO_WGRAD_SLAB)
};
// a kernel tile as one int: WI x WO waves over ci x co; per wave TI x TO 32-wide MFMA units (per-tap kernel) or one ci unit
// and CW co units for its TG-th share of the taps (nine-tap kernels); K steps of KS x 64 pixels (f32: 32); NS LDS stages
// (the ring: its two dY buffers); PL2: both operand planes of the f16x2 mode staged, the three plane products in one block
constexpr int wgrad_tile(int wi, int wo, int ti, int to, int tg, int ks, int cw, int ns, int pl2) {
    return wi | wo << 3 | ti << 6 | to << 9 | tg << 12 | ks << 15 | cw << 18 | ns << 21 | pl2 << 24;
}
struct WgTile {
    int wi, wo, ti, to, tg, ks, cw, ns, pl2;
    constexpr explicit WgTile(int t)
        : wi(t & 7), wo((t >> 3) & 7), ti((t >> 6) & 7), to((t >> 9) & 7), tg((t >> 12) & 7), ks((t >> 15) & 7),
          cw((t >> 18) & 7), ns((t >> 21) & 7), pl2(t >> 24) {}
    constexpr int bi() const { return 32 * wi * ti; }
    constexpr int bo() const { return 32 * wo * to * cw; }
    constexpr int nw() const { return wi * wo * tg; }
    constexpr int npl() const { return pl2 ? 2 : 1; }
    constexpr int bkp(int sz) const { return (sz == 2 ? 64 : 32) * ks; }     // pixels per K step
};
// LDS of a block, one formula per family (sz = bytes of an operand element).  plan_wgrad sizes the launch with them; the
// launchers check them against their kernel's staging layout at compile time.
//   per-tap: NS stages of [X: BKP x BI][dY: BKP x BO] per plane
constexpr int wg_lds(int sz, WgTile t) { return t.npl() * t.ns * t.bkp(sz) * (t.bi() + t.bo()) * sz; }
//   nine-tap: NS stages of [X window: wrows x BI][dY: BKP x BO] per plane.  The window is the K step plus the 3x3 reach,
//   in whole 1-KiB pieces (deeper rings count the loads in flight, so there every wave issues the same number of pieces)
constexpr int wg9_wrows(int sz, WgTile t, int W) {
    const int gran = (1024 / (t.bi() * sz)) * (t.ns > 2 ? t.nw() : 1);
    return (t.bkp(sz) + 2 * (W + 1) + 2 + gran - 1) / gran * gran;
}
constexpr int wg9_lds(int sz, WgTile t, int wrows) { return t.ns * t.npl() * (wrows * t.bi() * sz + t.bkp(sz) * t.bo() * sz); }
//   ring: a ring of 2^lg X rows and NS dY buffers per plane; the window spans G groups of BKP rows, and group st + G is in
//   flight during step st, so the ring holds at least BKP * (G + 1) rows
constexpr int wg9r_groups(int sz, WgTile t, int W) { return (t.bkp(sz) + 2 * (W + 1) + 2 + t.bkp(sz) - 1) / t.bkp(sz); }
constexpr int wg9r_lg(int sz, WgTile t, int W) {
    int lg = 7;
    while ((1 << lg) < t.bkp(sz) * (wg9r_groups(sz, t, W) + 1)) ++lg;
    return lg;
}
constexpr long wg9r_lds(int sz, WgTile t, int lg) {
    return (long)t.npl() * (((long)t.bi() * sz << lg) + (long)t.ns * t.bkp(sz) * t.bo() * sz);
}
struct WgradPlan {
    WgradKind kind;
    int tile;           // wgrad_tile
    int launches;       // 1, or 3 on operand-plane pairs (f16x2 where no PL2 tile fits)
    int splitk;
    WgradSum sum;
    int blocks;         // workgroups of one launch: dW tiles x splitk
    int lds;            // dynamic LDS bytes of a block
    int wrows;          // WK_NINE: X window rows per K step
    int ring_lg, ring_g;    // WK_RING: log2 of the ring's rows, groups of BKP rows per window
};
// no HIP calls, no side effects
WgradPlan plan_wgrad(int dtype, const WgradArgs& a);
// plan_wgrad + the launch (xcd order from Y2_XCD_WGRAD)
hipError_t launch_wgrad_auto(int dtype, const WgradArgs& a, hipStream_t s);
// the family launchers: hipErrorInvalidValue for a plan they cannot run
hipError_t launch_wgrad(int dtype, const WgradPlan& p, const WgradArgs& a, hipStream_t s);      // WK_TAP
hipError_t launch_wgrad9(int dtype, const WgradPlan& p, const WgradArgs& a, hipStream_t s);     // WK_NINE, WK_RING
// the slab's fixed-order sum into dW (WS_REDUCE1 / WS_REDUCE16)
hipError_t wgrad_reduce(const WgradPlan& p, const WgradArgs& a, hipStream_t s);
// what every family launcher does with its kernel: the LDS attribute (lds_attr: the largest size set so far for this
// kernel), the zero-filled dW of the atomics route, one launch per operand-plane pair with its own slab slots, the sum
template <typename K, typename... Extra>
inline hipError_t wgrad_run(K kern, int& lds_attr, const WgradPlan& p, const WgradArgs& a0, int threads, hipStream_t s,
                            Extra... extra) {
    if (p.lds > 160 * 1024 || p.blocks <= 0) return hipErrorInvalidValue;
    if (p.lds > lds_attr) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds);
        if (e != hipSuccess) return e;
        lds_attr = p.lds;
    }
    WgradArgs a = a0;
    a.splitk = p.splitk;
    a.quads = p.launches;
    const bool slab = p.sum == WS_REDUCE1 || p.sum == WS_REDUCE16;
    if (!slab) a.slab = nullptr;
    if (p.sum == WS_ATOMIC) {
        hipError_t e = hipMemsetAsync(a.dW, 0, (size_t)a.taps * a.Cin * a.Cout * sizeof(float), s);
        if (e != hipSuccess) return e;
    }
    for (int q = 0; q < p.launches; ++q) {
        WgradArgs b = a;
        if (q == 1) b.x = (const char*)a.x + (size_t)a.Cin * 2;
        if (q == 2) b.dy = (const char*)a.dy + (size_t)a.Cdy * 2;
        b.part0 = q * p.splitk;
        hipLaunchKernelGGL(kern, dim3(p.blocks), dim3(threads), p.lds, s, b, extra...);
    }
    hipError_t e = hipGetLastError();
    return e != hipSuccess || !slab ? e : wgrad_reduce(p, a, s);
}

// ---- packing
hipError_t launch_pack_input(int dtype, const float* img, void* x4, int N, int H, int W, hipStream_t s);
// same from uint8 pixels, with image_read's conversion x / 255 * 2 - 1 (src/img_dataset/pascal_voc.py:63-64) fused
hipError_t launch_pack_input_u8(int dtype, const uint8_t* img, void* x4, int N, int H, int W, hipStream_t s);
// fwd:  wf[co][t][ci] = W[t][ci][co]           rows co >= Cout zero (Cout_pad rows)
// dgrad: wd[ci][t'][co] = W[8-t'][ci][co]       rows ci >= Cin zero, cols co >= Cout zero (Cdy cols)
//   Kc = row length per tap of wf (>= Cin, zero beyond Cin)
hipError_t launch_pack_weights(int dtype, const float* W, void* wf, void* wd, int taps, int Cin, int Cout,
                               int Cout_pad, int Kc, int Cin_pad, int Cdy, int frag, hipStream_t s);
hipError_t launch_pack_conv1_weights(int dtype, const float* W, void* wp, hipStream_t s);
// all layers in one launch: table entry per layer (device copy lives in the workspace)
struct PackLayer {
    const float* W;
    size_t w_off;       // offset of W in the flat parameter buffer (adam_pack: the same offset into m, v, grads)
    void* wf;
    void* wd;           // null: no dgrad copy
    int taps, Cin, Cout, Cout_pad, Kc, Cin_pad, Cdy;
    int wf_bx, wf_by, wf_blocks, wd_blocks, first_block;
    int opt_first;      // first tile block of this layer in launch_opt_pack's grid (tiles only)
    int wf_frag, wd_frag;   // ConvPlan::filter_layout: 0 K-contiguous rows, 1 / 2 MFMA-fragment order (32 / 16 rows)
};
void pack_layer_plan(PackLayer& L, int first_block, int elem_size);
hipError_t launch_pack_all(int dtype, const PackLayer* tab_dev, int nlayers, int total_blocks, hipStream_t s);
// Optimizer step + filter re-pack in ONE pass over the parameters (the update reads and writes every filter
// anyway: the packed f16 / bf16 copies leave from the same registers instead of a second 193 MB read).
// kind 0: Adam (slot0 = m, slot1 = v), 1: Momentum (slot0 = accum), 2: Darknet's SGD (slot0 = accum, b1 = momentum,
// b2 = decay; the tiles are filters and always decay).  ctrl != null: guarded (optim.hip), lr_t from ctrl for kinds 0
// and 2; else lr_t = hyper[0].  hyper = {lr_t or lr, b1 or momentum, b2, eps, grad_mult}.
// small: [offset, count, decayed] ranges of the parameters that are not filter tiles (b, gamma, beta: not decayed; a
// 3-channel first filter: decayed -- kind 2 alone reads the flag)
struct OptPackArgs {
    float* p; float* slot0; float* slot1; const float* g;
    const void* ctrl;
    float lr_t, b1, b2, eps, gmult;
    int kind;
    const PackLayer* tab; int nlayers; int tile_blocks;
    const unsigned* small; int nsmall;
};
hipError_t launch_opt_pack(int dtype, const OptPackArgs& a, hipStream_t s);
hipError_t launch_convert_grad(int dtype, const float* src, void* dst, int M, int C, int ldd, float scale,
                               hipStream_t s);
hipError_t launch_unpack_act(int dtype, const void* xp, float* out, int N, int H, int W, int C, int Cs,
                             hipStream_t s);
// whole allocation of a bordered tensor (guards, borders, body, padding channels) in one pass; hipErrorNotSupported
// where the 16-byte form does not apply (the caller then zeroes the allocation and uses launch_pack_act)
hipError_t launch_pack_act_region(int dtype, const float* in, void* region, size_t region_bytes, size_t front_px, int N,
                                  int H, int W, int C, int Cs, hipStream_t s);
hipError_t launch_pack_act(int dtype, const float* in, void* xp, int N, int H, int W, int C, int Cs,
                           hipStream_t s);
hipError_t launch_cast_to_f32(int dtype, const void* src, float* dst, size_t rows, int C, int lds, hipStream_t s,
                              float scale = 1.0f);

// ---- batch norm
struct BnFinalizeArgs {
    const float* part_cnt;
    const float* part_mean;
    const float* part_m2;
    int P, C, ldp;
    const float* gamma;
    const float* beta;
    float* moving_mean;   // updated in place when update_moving
    float* moving_var;
    float* scale;         // out: gamma * rsqrt(var + eps)
    float* shift;         // out: beta - mean * scale
    float* mean;          // out (saved for backward)
    float* invstd;        // out
    float* var;           // out: biased (or Bessel) batch variance as the moving update uses it
    float eps, momentum;
    int update_moving;
    int bessel;
    float* scratch = nullptr;   // >= 64 * (1 + 2 * ldp) floats: long partial lists are compressed to 64 records first
};
hipError_t launch_bn_finalize(const BnFinalizeArgs& a, hipStream_t s);
// per layer: moving statistics + gamma / beta -> scale, shift, mean, invstd of the apply pass
struct BnInferLayer {
    const float *gamma, *beta, *mm, *mv;
    float *scale, *shift, *mean, *invstd;
    int C, is_core;
};
hipError_t launch_bn_infer_prepare_all(const BnInferLayer* tab, int nlayers, int max_c, int train_core, int train_head,
                                       float eps, hipStream_t s);
hipError_t launch_bn_update_moving(const float* mean, const float* var, float* mm, float* mv, int C, float momentum,
                                   hipStream_t s);
struct BnActArgs {
    const void* y;        // [M][ldy]
    const float* scale;
    const float* shift;
    void* out;            // zero-bordered [N][Ho+2][Wo+2][C] of T, or (out_f32) float [M][C] compact
    int N, H, W, C, ldy;
    int pool;             // 1: 2x2/2 SAME max pool after the activation.  2 (round 5, the ResNet swap's stride-2 3x3
                          // convolutions, slim conv2d_same: resnet_utils.py:77-122): SUBSAMPLE -- the layer keeps window
                          // position 0 (the stride-1 output at even rows / columns) and its batch norm runs over the kept
                          // positions only; even H and W
    int out_f32;
    float slope = 0.1f;   // activation: max(slope * z, z)
    void* ysel = nullptr; // pooled layers, training: the conv output at the window's (first) arg-max, [Mout][ldy] of T --
                          // what the BN-backward reduce needs of y (fused into the dgrad epilogue above this layer)
    const float* join = nullptr;   // out_f32 only, [M][C] like out: the stored value is max(act + join, 0) -- the join of a
                                   // ResNet bottleneck unit (y2_forward_join)
    const void* join_t = nullptr;  // the same join read from a BORDERED tensor of T with the output's geometry (round 5,
                                   // y2_link: bottleneck units chained without an fp32 hand-over); either output form
};
hipError_t launch_bn_act(int dtype, const BnActArgs& a, hipStream_t s);
// merge of a short partial list (P <= kBnFinPmax) + apply in one launch (kBnSlab-channel slabs: C = ldy = ldp, a multiple)
constexpr int kBnSlab = 64, kBnFinPmax = 128;
hipError_t launch_bn_fin_act(int dtype, const BnActArgs& a, const BnFinalizeArgs& f, hipStream_t s);
// subsampling layers (BnActArgs::pool == 2): (count, mean, M2) records of the conv output y [N*H*W][ldy] over the KEPT
// positions (even rows and columns), one record per kBnSubRec kept pixels
constexpr int kBnSubRec = 256;
constexpr int bn_stats_sub_records(int N, int H, int W) { return (N * (H / 2) * (W / 2) + kBnSubRec - 1) / kBnSubRec; }
hipError_t launch_bn_stats_sub(int dtype, const void* y, int N, int H, int W, int ldy, float* part_cnt, float* part_mean,
                               float* part_m2, hipStream_t s);

struct BnBwdArgs {
    const void* dA;       // grad wrt layer output [M_out][ldd] of T (scaled by grad_scale)
    const void* y;        // conv output [M][ldy]
    const float* scale;   // gamma*invstd
    const float* shift;
    const float* mean;
    const float* invstd;
    float* psum;          // [P][2][C] partial sums (dz, dz*y)
    float* dgamma;        // out (unscaled)
    float* dbeta;
    float* dbias;         // out: sum(dy), analytic (see bn.hip)
    float* coef;          // [2][ldy]: ka, kb of dy = scale*dz - (ka + kb*y)   (scaled domain)
    void* dyp;            // out: zero-bordered [N][H+2][W+2][ldy] of T
    int N, H, W, C, ldy, ldd;
    int pool;
    int training;         // batch statistics (1) or moving statistics (0)
    float inv_grad_scale;
    int P;                // number of partial records (the reduce: bn_bwd_reduce_records)
    float slope = 0.1f;   // activation slope of the forward pass
    int hi_only = 0;      // f16x2f (split dyp): the consumers read the hi plane of dY alone -- the lo plane is not written
    int dA_half = 0;      // f16x2f (T = float kernels): dA [M_out][ldd] is f16 (written by a launch-dtype-5 dgrad, common.h hsplithh_t)
};
// records of the standalone reduce (its grid)
int bn_bwd_reduce_records(int dtype, const BnBwdArgs& a);
hipError_t launch_bn_bwd_reduce(int dtype, const BnBwdArgs& a, hipStream_t s);
hipError_t launch_bn_bwd_finalize(const BnBwdArgs& a, hipStream_t s);
hipError_t launch_bn_bwd_apply(int dtype, const BnBwdArgs& a, hipStream_t s);
// finalize of a short partial list (P <= kBnFinPmax) + apply in one launch (kBnSlab-channel slabs: C = ldy, a multiple)
hipError_t launch_bn_bwd_fin_apply(int dtype, const BnBwdArgs& a, hipStream_t s);

// ---- loss / heads
struct LossArgs {
    const float* net;     // [N][S][S][C + 5B]
    const float* labels;  // [N][S][S][5 + C]
    float* loss;          // [5]: class, object, noobject, coord, total
    float* ious;          // [N][S][S][B]
    float* mask;          // [N][S][S][B]
    float* dnet;          // [N][S][S][C+5B] or null
    float* partial;       // [nblocks][4]
    int N, S, B, C;
    float image_size;
    float lambda_coord, lambda_noobj;
};
int loss_blocks(int N, int S);
hipError_t launch_yolo_loss(const LossArgs& a, hipStream_t s);
hipError_t launch_get_iou(const float* b1, const float* b2, float* out, int n, hipStream_t s);
hipError_t launch_decode(const float* pred, int S, int B, int C, int im_w, int im_h, float thresh, int* out,
                         float* out_conf, hipStream_t s);
hipError_t launch_avgpool_fwd(const float* h, float* out, int N, int H, int W, int C, int k, hipStream_t s);
hipError_t launch_avgpool_bwd(const float* dout, float* dh, int N, int H, int W, int C, int k, hipStream_t s);
hipError_t launch_softmax_ce(const float* logits, const int* labels, float* loss, float* dlogits, int N, int C,
                             hipStream_t s);

hipError_t launch_accuracy(const float* logits, const int* labels, float* acc, int N, int C, hipStream_t s);

// ---- optimizers (flat buffers)
hipError_t launch_adam(float* p, float* m, float* v, const float* g, size_t n, float lr_t, float b1, float b2,
                       float eps, float gscale, hipStream_t s);
hipError_t launch_momentum(float* p, float* acc, const float* g, size_t n, float lr, float mom, float gscale,
                           hipStream_t s);
// dynamic loss scaling: ctrl = {int found_inf, int step, int skipped, float lr_t}
hipError_t launch_grad_check(const float* g, size_t n, void* ctrl, hipStream_t s);
hipError_t launch_grad_check_ranges(const float* g, const void* ranges_dev, int nranges, void* ctrl, hipStream_t s,
                                    unsigned* flag = nullptr, bool keep = false);   // keep: do not clear found_inf first
hipError_t launch_range_check(const float* x, size_t n, float limit, void* ctrl, hipStream_t s);   // found_inf |= !(|x| <= limit)
hipError_t launch_opt_ctrl_advance(void* ctrl, float lr, float b1, float b2, hipStream_t s);
hipError_t launch_adam_guarded(float* p, float* m, float* v, const float* g, size_t n, const void* ctrl, float b1,
                               float b2, float eps, float gscale, hipStream_t s);
hipError_t launch_momentum_guarded(float* p, float* acc, const float* g, size_t n, const void* ctrl, float lr, float mom,
                                   float gscale, hipStream_t s);
// Darknet's SGD on a flat buffer (optim.hip): the buffer as segments that decay (filters) or not (b / gamma / beta),
// in buffer order; first_block: the segment's first block of launch_sgd's grid, sgd_seg_blocks() blocks each
struct SgdSeg { unsigned off, cnt, first_block, decayed; };
int sgd_seg_blocks(size_t off, size_t cnt);
hipError_t launch_sgd(float* p, float* acc, const float* g, const SgdSeg* segs_dev, int nsegs, int blocks,
                      const void* ctrl, float lr_t, float mom, float decay, float gscale, hipStream_t s);
hipError_t launch_sgd_ctrl_advance(void* ctrl, const y2_sgd_solver& sv, hipStream_t s);
hipError_t launch_init_trunc_normal(float* p, size_t n, float stddev, uint64_t seed, uint64_t stream_id,
                                    hipStream_t s);
hipError_t launch_fill(float* p, size_t n, float v, hipStream_t s);

// ---- evaluation of the grid detector (detect.hip): the limits its LDS arrays and bit masks are sized for
constexpr int kDetectMaxCand = Y2_DETECT_MAX_CANDIDATES;   // candidates of one image in y2_detect_grid_batch
constexpr int kDetectAnchorMaxCand = Y2_DETECT_ANCHOR_MAX_CANDIDATES;   // ... in y2_detect_anchor_batch
constexpr int kMatchMaxObj = Y2_MATCH_MAX_OBJECTS;         // objects of one image in y2_voc_match_batch (16 per lane)

// per-(device, stream) scratch of the graph-level operators (split partial sums); grows on demand, never shrinks
void* op_scratch(hipStream_t s, size_t bytes);
int op_scratch_error();      // code of the last null return of op_scratch on this thread (its message is already in y2_last_error)

}  // namespace y2
