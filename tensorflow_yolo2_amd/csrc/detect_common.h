// What the detect kernels of detect.hip (integer pixel rows) and darknet_io.hip (Darknet's float rows) share: the 64-bit
// sort word, the devkit's IoU, the wave-wide first maximum and the matching kernel, whose only difference between the two
// is how words 0..3 of a row are read, and (host code) the argument checks of the per-anchor detect entries and the
// matchers' entry.  One definition of each; both files are compiled with -ffp-contract=off.
#pragma once
#include "common.h"
#include "data_common.h"
#include "kernels.h"

namespace y2 {

// (score, candidate) as one 64-bit word whose unsigned order is "score descending, then index ascending" read from the
// top: the float's bits made monotonic in the high half, ~index in the low half.  The words of a workgroup are distinct
// (the indices are), so the sort needs one compare.  A valid score is sigmoid * softmax >= +0 or it is not kept at all,
// so -0.0 and +0.0, equal as floats but not as bits, never meet.
Y2_DEV uint64_t sort_word(float key, int idx) {
    const uint32_t u = __float_as_uint(key);
    const uint32_t m = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
    return ((uint64_t)m << 32) | (uint32_t)(0xffffffffu - (uint32_t)idx);
}
Y2_DEV int word_index(uint64_t w) { return (int)(0xffffffffu - (uint32_t)w); }
Y2_DEV float word_key(uint64_t w) {
    const uint32_t m = (uint32_t)(w >> 32);
    return __uint_as_float(m ^ ((m >> 31) ? 0x80000000u : 0xffffffffu));
}

// IoU of two inclusive pixel boxes with the devkit's +1 extents (utils/voc_eval.box_iou_voc): `a` is its `box`
Y2_DEV double iou_voc(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3) {
    const double ixmin = fmax(b0, a0), iymin = fmax(b1, a1);
    const double ixmax = fmin(b2, a2), iymax = fmin(b3, a3);
    const double iw = fmax(ixmax - ixmin + 1.0, 0.0), ih = fmax(iymax - iymin + 1.0, 0.0);
    const double inter = iw * ih;
    const double uni = ((a2 - a0 + 1.0) * (a3 - a1 + 1.0) + (b2 - b0 + 1.0) * (b3 - b1 + 1.0)) - inter;
    return inter / uni;
}

// first maximum over the wave of (iou, object index): the larger iou, ties to the lower index
Y2_DEV void wave_first_max(double& best, int& arg) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off, kWave);
        const int oa = __shfl_xor(arg, off, kWave);
        if (ob > best || (ob == best && oa < arg)) {
            best = ob;
            arg = oa;
        }
    }
}

// a corner (word 0..3 of a det row) as the double the matching works on: the integer pixel, or the float32 whose bit
// pattern the word holds (y2_detect_anchor_classes_batch_dk)
template <bool FLOAT_ROWS>
Y2_DEV double row_corner(int word) {
    return FLOAT_ROWS ? (double)__int_as_float(word) : (double)word;
}

// grid (n), ONE 64-lane wave per image.  Lane l holds objects l, l + 64, ... of the image (the first one in registers,
// the others re-read through the cache: VOC images have at most 42 objects) with their `difficult` and `taken` bits in
// two 16-bit masks (max_obj <= 1024).  The detections are walked in row order; each step is a wave-wide first maximum
// of the float64 IoU over the objects of the detection's class, and the lane that owns the winner settles the flag.
// FLOAT_ROWS: row_corner.
template <bool FLOAT_ROWS>
__global__ __launch_bounds__(kWave) void voc_match_kernel(const int* __restrict__ det, const int* __restrict__ count,
                                                          const double* __restrict__ boxes,
                                                          const int32_t* __restrict__ counts,
                                                          const uint8_t* __restrict__ difficult,
                                                          const int32_t* __restrict__ index, int max_obj, int max_out,
                                                          float iou_thresh, int* __restrict__ flags) {
    const int img = blockIdx.x, lane = threadIdx.x;
    const size_t e = index ? (size_t)index[img] : (size_t)img;
    const int cnt = min(max(counts[e], 0), max_obj);
    const int ndet = min(max(count[img], 0), max_out);
    const double* bx = boxes + e * (size_t)max_obj * 5;
    const uint8_t* df = difficult + e * (size_t)max_obj;
    const int strides = (cnt + kWave - 1) / kWave;
    unsigned hard = 0, taken = 0;
    for (int k = 0; k < strides; ++k) {
        const int j = lane + kWave * k;
        if (j < cnt && df[j]) hard |= 1u << k;
    }
    double g0 = 0, g1 = 0, g2 = 0, g3 = 0, gc = -1.0;
    if (lane < cnt) {
        g0 = bx[lane * 5 + 0]; g1 = bx[lane * 5 + 1]; g2 = bx[lane * 5 + 2]; g3 = bx[lane * 5 + 3]; gc = bx[lane * 5 + 4];
    }
    const double thr = (double)iou_thresh;
    const int* drow = det + (size_t)img * max_out * 6;
    int* frow = flags + (size_t)img * max_out;
    for (int d = 0; d < ndet; ++d) {
        const double d0 = row_corner<FLOAT_ROWS>(drow[d * 6 + 0]), d1 = row_corner<FLOAT_ROWS>(drow[d * 6 + 1]);
        const double d2 = row_corner<FLOAT_ROWS>(drow[d * 6 + 2]), d3 = row_corner<FLOAT_ROWS>(drow[d * 6 + 3]);
        const double dc = drow[d * 6 + 4];
        double best = -1.0;
        int arg = 0x7fffffff;
        if (lane < cnt && gc == dc) {
            best = iou_voc(d0, d1, d2, d3, g0, g1, g2, g3);
            arg = lane;
        }
        for (int k = 1; k < strides; ++k) {
            const int j = lane + kWave * k;
            if (j < cnt && bx[j * 5 + 4] == dc) {
                const double v = iou_voc(d0, d1, d2, d3, bx[j * 5 + 0], bx[j * 5 + 1], bx[j * 5 + 2], bx[j * 5 + 3]);
                if (v > best || arg == 0x7fffffff) {           // (ascending j: the strict > keeps the lane's first maximum)
                    best = v;
                    arg = j;
                }
            }
        }
        wave_first_max(best, arg);
        int flag = 0;
        if (arg != 0x7fffffff && best >= thr) {                // uniform: every lane holds the winner
            const int owner = arg & (kWave - 1);
            const unsigned bit = 1u << (arg / kWave);
            int mine = 0;
            if (lane == owner) {
                if (hard & bit) mine = 2;
                else if (!(taken & bit)) {
                    mine = 1;
                    taken |= bit;
                }
            }
            flag = __shfl(mine, owner, kWave);
        }
        if (lane == 0) frow[d] = flag;
    }
    for (int d = ndet + lane; d < max_out; d += kWave) frow[d] = -1;
}

// ---- host code: the entry points' argument checks ----------------------------------------------------------------
// The checks of a per-anchor detect entry `name`, in the order every one of them reports: null pointers, n (the
// per-class entries launch n as the grid's y and cap it with n_cap; 0: no cap), the rows per image or per class
// (`rows_name` is max_out or max_per_class), the head's shape, the candidate limit and, for a letterboxed batch,
// net_size = 32 S.  Leaves KP, the next power of two of S * S * B (at least one wave), for the launch.
static int detect_anchor_args(const char* name, bool pointers, int n, int n_cap, const char* rows_name, int rows, int S,
                              int B, int num_class, bool letterbox, int net_size, int* KP) {
    if (!pointers) return fail(Y2_ERR_ARG, "%s: null pointer", name);
    if (n < 1 || (n_cap && n > n_cap))
        return n_cap ? fail(Y2_ERR_ARG, "%s: n = %d outside 1..%d", name, n, n_cap)
                     : fail(Y2_ERR_ARG, "%s: n = %d", name, n);
    if (rows < 1) return fail(Y2_ERR_ARG, "%s: %s = %d", name, rows_name, rows);
    if (S < 1 || B < 1 || num_class < 1 || S > kDetectAnchorMaxCand || B > 16)
        return fail(Y2_ERR_ARG, "%s: S = %d, B = %d (at most 16), num_class = %d", name, S, B, num_class);
    if (S * S * B > kDetectAnchorMaxCand)
        return fail(Y2_ERR_ARG, "%s: S * S * B = %d candidates beyond Y2_DETECT_ANCHOR_MAX_CANDIDATES = %d", name,
                    S * S * B, kDetectAnchorMaxCand);
    if (letterbox && (net_size < 32 || net_size % 32 || net_size != 32 * S))
        return fail(Y2_ERR_ARG, "%s: net_size = %d is not the positive multiple of 32 that S = %d makes (32 S = %d)",
                    name, net_size, S, 32 * S);
    *KP = kWave;
    while (*KP < S * S * B) *KP <<= 1;
    return Y2_OK;
}

// y2_voc_match_batch (integer rows) and y2_voc_match_batch_f (float rows).  `score` is not read: the rows arrive in
// descending score (y2_detect_grid_batch, y2_nms), and the order is all that is used.
template <bool FLOAT_ROWS>
static int voc_match_any(const char* name, const int* det, const int* count, const double* boxes, const int32_t* counts,
                         const uint8_t* difficult, const int32_t* index, int n, int max_obj, int max_out,
                         float iou_thresh, int* flags, void* stream) {
    if (!det || !count || !boxes || !counts || !difficult || !flags) return fail(Y2_ERR_ARG, "%s: null pointer", name);
    if (n < 1) return fail(Y2_ERR_ARG, "%s: n = %d", name, n);
    if (max_out < 1) return fail(Y2_ERR_ARG, "%s: max_out = %d", name, max_out);
    if (max_obj < 1 || max_obj > kMatchMaxObj)
        return fail(Y2_ERR_ARG, "%s: max_obj = %d outside 1..Y2_MATCH_MAX_OBJECTS = %d", name, max_obj, kMatchMaxObj);
    hipLaunchKernelGGL(voc_match_kernel<FLOAT_ROWS>, dim3(n), dim3(kWave), 0, (hipStream_t)stream, det, count, boxes,
                       counts, difficult, index, max_obj, max_out, iou_thresh, flags);
    return launched(name);
}

}  // namespace y2
