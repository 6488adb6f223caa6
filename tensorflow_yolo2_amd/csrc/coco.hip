// COCO's bounding-box matching on the device ("COCO evaluation"): y2_coco_match_batch walks the detection
// rows of every (image, class) segment against the image's annotations under all (area range, IoU threshold) pairs at
// once and leaves one packed word per row and area range.  The specification is utils/coco_eval.match_segment (numpy
// float64, a restatement of COCOeval.evaluateImg and bbIou) and the kernel equals it bit for bit: every IoU is formed
// in double in the specification's operation order, and the file is compiled with -ffp-contract=off.
#include "data_common.h"
#include "kernels.h"
#include "detect_common.h"
using namespace y2;

namespace {

constexpr int kCocoMaxObj = Y2_COCO_MAX_OBJECTS;
// LDS of one segment, per object of the box table: x, y, w, h, class (float64 each, structure of arrays), the IoU and the
// index of the compacted same-class list, and one state byte per lane
constexpr int kCocoObjBytes = 5 * 8 + 8 + 4 + kWave;
constexpr unsigned kTaken = 1, kIgnored = 2, kCrowd = 4;

// utils/coco_eval.bbox_iou
Y2_DEV double coco_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh,
                       bool crowd) {
    const double da = dw * dh;
    const double ga = gw * gh;
    const double ow = fmin(dx + dw, gx + gw) - fmax(dx, gx);
    if (ow <= 0) return 0.0;
    const double oh = fmin(dy + dh, gy + gh) - fmax(dy, gy);
    if (oh <= 0) return 0.0;
    const double i = ow * oh;
    const double u = crowd ? da : (da + ga) - i;
    return i / u;
}

// grid (n), ONE 64-lane wave per segment; lane = a * T + t is one (area range, threshold) pair, T * A <= 64.
// Start: the entry's objects go to LDS once, and every lane writes its own state byte per object: ignored under its
// area range (crowd, or the annotation's area outside the range), crowd, and later taken.
// Per row, two phases with a barrier between them:
//   (1) the lanes share the objects: lane l forms the IoU of objects l, l + 64, ... of the row's class, and a ballot
//       compacts them, in annotation order, into the list (iou, object) -- every IoU is computed once, not T * A times;
//   (2) every lane walks that list on its own.  All lanes read the same list element (a broadcast); only the state byte
//       is the lane's.  The specification's two passes are one walk with two running bests: the second pass counts only
//       where the first found nothing, and then the first has left `best` at its initial value.
// The values of the T lanes of an area range are gathered with two ballots and stored as one word by lane a.
__global__ __launch_bounds__(kWave) void coco_match_kernel(const int* __restrict__ det, const int* __restrict__ count,
                                                           const double* __restrict__ boxes,
                                                           const double* __restrict__ area,
                                                           const uint8_t* __restrict__ crowd,
                                                           const int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ index, int max_obj, int max_out,
                                                           const double* __restrict__ thresholds, int T,
                                                           const double* __restrict__ area_ranges, int A, int row_form,
                                                           int* __restrict__ match) {
    extern __shared__ __attribute__((aligned(16))) unsigned char coco_lds[];
    double* gx = (double*)coco_lds;                          // [max_obj] each
    double* gy = gx + max_obj;
    double* gw = gy + max_obj;
    double* gh = gw + max_obj;
    double* gc = gh + max_obj;
    double* liou = gc + max_obj;                             // [max_obj]: the row's compacted list
    int* lobj = (int*)(liou + max_obj);                      // [max_obj]
    unsigned char* state = (unsigned char*)(lobj + max_obj);   // [max_obj][kWave]

    const int seg = blockIdx.x, lane = threadIdx.x;
    const int ndet = min(max(count[seg], 0), max_out);
    int* mrow = match + (size_t)seg * max_out * A;
    for (int i = ndet * A + lane; i < max_out * A; i += kWave) mrow[i] = -1;
    if (ndet == 0) return;                                   // uniform

    const size_t e = index ? (size_t)index[seg] : (size_t)seg;
    const int cnt = min(max(counts[e], 0), max_obj);
    const double* bx = boxes + e * (size_t)max_obj * 5;
    const double* ar = area + e * (size_t)max_obj;
    const uint8_t* cr = crowd + e * (size_t)max_obj;
    const bool live = lane < T * A;
    const int a = live ? lane / T : 0, t = live ? lane - a * T : 0;
    const double lo = area_ranges[2 * a], hi = area_ranges[2 * a + 1];
    const double first = fmin(thresholds[t], 1 - 1e-10);
    for (int j = lane; j < cnt; j += kWave) {
        gx[j] = bx[j * 5 + 0]; gy[j] = bx[j * 5 + 1]; gw[j] = bx[j * 5 + 2]; gh[j] = bx[j * 5 + 3]; gc[j] = bx[j * 5 + 4];
    }
    for (int j = 0; j < cnt; ++j) {                          // uniform loads, the lane's own range
        const double s = ar[j];
        const bool c = cr[j] != 0;
        state[j * kWave + lane] = (unsigned char)((c || s < lo || s > hi ? kIgnored : 0u) | (c ? kCrowd : 0u));
    }
    __syncthreads();

    const int* drow = det + (size_t)seg * max_out * 6;
    for (int d = 0; d < ndet; ++d) {
        const int w0 = drow[d * 6 + 0], w1 = drow[d * 6 + 1], w2 = drow[d * 6 + 2], w3 = drow[d * 6 + 3];
        const double dc = (double)drow[d * 6 + 4];
        double dx, dy, dw, dh;
        if (row_form) {
            const double x0 = (double)__int_as_float(w0), y0 = (double)__int_as_float(w1);
            dx = x0 - 1.0; dy = y0 - 1.0;
            dw = (double)__int_as_float(w2) - x0; dh = (double)__int_as_float(w3) - y0;
        } else {
            const double x0 = (double)w0, y0 = (double)w1;
            dx = x0 - 1.0; dy = y0 - 1.0;
            dw = (double)w2 - x0 + 1.0; dh = (double)w3 - y0 + 1.0;
        }
        // (1) the objects of the row's class, compacted in annotation order
        int nlist = 0;
        for (int base = 0; base < cnt; base += kWave) {      // uniform trip count
            const int j = base + lane;
            const bool mine = j < cnt && gc[j] == dc;
            const unsigned long long mask = __ballot(mine);
            if (mine) {
                const int pos = nlist + __popcll(mask & ((1ull << lane) - 1ull));
                liou[pos] = coco_iou(dx, dy, dw, dh, gx[j], gy[j], gw[j], gh[j],
                                      (state[j * kWave + lane] & kCrowd) != 0);
                lobj[pos] = j;
            }
            nlist += __popcll(mask);
        }
        __syncthreads();
        // (2) the lane's walk
        double best1 = first, best2 = first;
        int m1 = -1, m2 = -1;
        for (int k = 0; k < nlist; ++k) {
            const double v = liou[k];
            const int j = lobj[k];
            const unsigned st = state[j * kWave + lane];
            if ((st & kTaken) && !(st & kCrowd)) continue;
            if (st & kIgnored) {
                if (!(v < best2)) { best2 = v; m2 = j; }
            } else {
                if (!(v < best1)) { best1 = v; m1 = j; }
            }
        }
        const int m = m1 >= 0 ? m1 : m2;
        int value;
        if (m >= 0) {
            const unsigned st = state[m * kWave + lane];
            state[m * kWave + lane] = (unsigned char)(st | kTaken);
            value = (st & kIgnored) ? 2 : 1;
        } else {
            const double own = dw * dh;
            value = (own < lo || own > hi) ? 2 : 0;
        }
        if (!live) value = 0;
        const unsigned long long b0 = __ballot(value & 1), b1 = __ballot(value & 2);
        if (lane < A) {
            const unsigned v0 = (unsigned)(b0 >> (lane * T)), v1 = (unsigned)(b1 >> (lane * T));
            unsigned word = 0;
            for (int k = 0; k < T; ++k) word |= (((v0 >> k) & 1u) << (2 * k)) | (((v1 >> k) & 1u) << (2 * k + 1));
            mrow[d * A + lane] = (int)word;
        }
        __syncthreads();                                     // the list is rewritten by the next row
    }
}

}  // namespace

extern "C" {

int y2_coco_match_batch(const int* det, const int* count, const double* boxes, const double* area, const uint8_t* crowd,
                        const int32_t* counts, const int32_t* index, int n, int max_obj, int max_out,
                        const double* thresholds, int T, const double* area_ranges, int A, int row_form, int* match,
                        void* stream) {
    const char* name = "y2_coco_match_batch";
    if (!det || !count || !boxes || !area || !crowd || !counts || !thresholds || !area_ranges || !match)
        return fail(Y2_ERR_ARG, "%s: null pointer", name);
    if (n < 1 || n > Y2_COCO_MAX_SEGMENTS)
        return fail(Y2_ERR_ARG, "%s: n = %d outside 1..Y2_COCO_MAX_SEGMENTS = %d", name, n, Y2_COCO_MAX_SEGMENTS);
    if (max_obj < 1 || max_obj > kCocoMaxObj)
        return fail(Y2_ERR_ARG, "%s: max_obj = %d outside 1..Y2_COCO_MAX_OBJECTS = %d", name, max_obj, kCocoMaxObj);
    if (max_out < 1 || max_out > Y2_COCO_MAX_ROWS)
        return fail(Y2_ERR_ARG, "%s: max_out = %d outside 1..Y2_COCO_MAX_ROWS = %d", name, max_out, Y2_COCO_MAX_ROWS);
    if (T < 1 || T > Y2_COCO_MAX_THRESHOLDS || A < 1 || A > Y2_COCO_MAX_AREAS || T * A > kWave)
        return fail(Y2_ERR_ARG, "%s: T = %d (1..%d), A = %d (1..%d), T * A at most %d", name, T, Y2_COCO_MAX_THRESHOLDS, A,
                    Y2_COCO_MAX_AREAS, kWave);
    if (row_form != 0 && row_form != 1) return fail(Y2_ERR_ARG, "%s: row_form = %d is neither 0 nor 1", name, row_form);
    hipLaunchKernelGGL(coco_match_kernel, dim3(n), dim3(kWave), (size_t)max_obj * kCocoObjBytes, (hipStream_t)stream, det,
                       count, boxes, area, crowd, counts, index, max_obj, max_out, thresholds, T, area_ranges, A, row_form,
                       match);
    return launched(name);
}

}  // extern "C"
