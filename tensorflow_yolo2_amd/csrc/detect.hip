// Evaluation of the detectors on the device (pascal/pascal_eval_darknet.py, pascal/pascal_eval_yolov2.py): per image, the
// head's output (the grid head's, or the raw anchor head's: detect_anchor_kernel, specified by anchor_detect; with one
// row per class instead of the best class: detect_anchor_classes_kernel, specified by anchor_detect_classes) decoded
// into boxes in the pixels of the ORIGINAL image, a score-ordered class-aware greedy NMS, and the VOC devkit's matching
// of the surviving rows against the image's ground truth.  The specification is this repository's host code
// (utils/detect_batch.py: grid_detect, match_image) and both kernels are bit-equal to it: the decoded products and every
// IoU are float64 in the specification's operation order, and the file is compiled with -ffp-contract=off.  What stays
// on the host is the per-class precision / recall curve, which needs one sort across all images (map_from_flags).
#include "data_common.h"
#include "kernels.h"
#include "anchor_decode.h"
#include "letterbox.h"
#include "detect_common.h"
using namespace y2;

namespace {

constexpr int kMaxCand = kDetectMaxCand;   // candidates (S * S * B) of one image; LDS below is sized for it: 29 KB
// (the sort word, the devkit's IoU and the matching kernel are detect_common.h's, shared with darknet_io.hip)

// grid (n), one workgroup per image, KP = the next power of two of K = S * S * B (at least 64) lanes.
//   1. lane i decodes candidate i (cell i / B: row cell / S, column cell % S) into LDS: the clipped 1-based box, the
//      class, and the sort key = confidence, or -inf for a candidate that is not valid (and for i >= K);
//   2. bitonic sort of (key, index), descending key, ties by ascending index: the valid candidates come first;
//   3. the order is walked: a row that is not suppressed is kept (lane 0 writes it) and suppresses, in parallel, every
//      later row of its class with IoU > iou_thresh.  `kept` and sup[i] are uniform over the workgroup, so the barrier
//      inside the branch is met by every lane.
__global__ __launch_bounds__(kMaxCand) void detect_grid_kernel(const float* __restrict__ predict,
                                                               const int64_t* __restrict__ table,
                                                               const int32_t* __restrict__ index, int S, int B, int C,
                                                               float object_thresh, float iou_thresh, int max_out,
                                                               int KP, int* __restrict__ det, float* __restrict__ score,
                                                               int* __restrict__ count) {
    __shared__ float skey[kMaxCand];
    __shared__ int sidx[kMaxCand];
    __shared__ int bx0[kMaxCand], by0[kMaxCand], bx1[kMaxCand], by1[kMaxCand];
    __shared__ int bcls[kMaxCand];
    __shared__ unsigned char sup[kMaxCand];
    __shared__ int s_valid;
    const int img = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int K = S * S * B, D = C + 5 * B;
    const int64_t* t = table + (size_t)kTable * (index ? index[img] : img);
    const int64_t h64 = t[1], w64 = t[2];
    const bool sized = h64 >= 1 && w64 >= 1 && h64 <= 0x7fffffff && w64 <= 0x7fffffff;
    const int im_h = sized ? (int)h64 : 1, im_w = sized ? (int)w64 : 1;
    const float* pred = predict + (size_t)img * S * S * D;
    if (tid == 0) s_valid = 0;
    __syncthreads();
    for (int i = tid; i < KP; i += nt) {
        bool valid = false;
        float conf = -INFINITY;
        if (i < K && sized) {
            const int cell = i / B, b = i - cell * B;
            const int c = cell / S, r = cell - c * S;
            const float* p = pred + (size_t)cell * D;
            conf = p[C + b];
            const float* pb = p + C + B + 4 * b;
            const double xs = ((double)pb[0] + (double)r) / (double)S;   // decode_kernel's products (loss.hip)
            const double ys = ((double)pb[1] + (double)c) / (double)S;
            const float ws = pb[2] * pb[2], hs = pb[3] * pb[3];          // np.square on float32
            const double dx = xs * (double)im_w, dy = ys * (double)im_h;
            const double dw = (double)ws * (double)im_w, dh = (double)hs * (double)im_h;
            const double lim = 1073741824.0;                             // 2^30: checked BEFORE any conversion to int
            valid = conf > object_thresh && fabs(dx) < lim && fabs(dy) < lim && fabs(dw) < lim && fabs(dh) < lim;
            if (valid) {
                const int x = (int)dx, y = (int)dy, w = (int)dw, h = (int)dh;   // w, h >= 0: floor(w / 2) = w >> 1
                const int ulx = x - (w >> 1), uly = y - (h >> 1);
                const int xmin = max(ulx, 0), ymin = max(uly, 0);
                const int xmax = min(ulx + w - 1, im_w - 1), ymax = min(uly + h - 1, im_h - 1);
                valid = xmax >= xmin && ymax >= ymin;
                int cls = 0;
                float best = p[0];
                for (int k = 1; k < C; ++k)
                    if (p[k] > best) {
                        best = p[k];
                        cls = k;
                    }
                bx0[i] = xmin + 1; by0[i] = ymin + 1; bx1[i] = xmax + 1; by1[i] = ymax + 1;
                bcls[i] = cls;
            }
        }
        skey[i] = valid ? conf : -INFINITY;
        sidx[i] = i;
        sup[i] = 0;
        if (valid) atomicAdd(&s_valid, 1);
    }
    __syncthreads();
    for (int k = 2; k <= KP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < KP; i += nt) {
                const int l = i ^ j;
                if (l > i) {
                    const float a = skey[i], b = skey[l];
                    const int ia = sidx[i], ib = sidx[l];
                    const bool a_first = (a > b) || (a == b && ia < ib);   // a precedes b in the final order
                    const bool desc = (i & k) == 0;
                    if (desc ? !a_first : a_first) {
                        skey[i] = b; skey[l] = a;
                        sidx[i] = ib; sidx[l] = ia;
                    }
                }
            }
            __syncthreads();
        }
    // a valid key is > object_thresh >= -inf, so the valid candidates are exactly the first s_valid of the order
    const int nvalid = s_valid;
    const double thr = (double)iou_thresh;
    int* drow = det + (size_t)img * max_out * 6;
    float* srow = score + (size_t)img * max_out;
    int kept = 0;
    for (int i = 0; i < nvalid && kept < max_out; ++i) {
        if (sup[i]) continue;
        const int o = sidx[i];
        const int ac = bcls[o];
        const double a0 = bx0[o], a1 = by0[o], a2 = bx1[o], a3 = by1[o];
        if (tid == 0) {
            int* d = drow + (size_t)kept * 6;
            d[0] = bx0[o]; d[1] = by0[o]; d[2] = bx1[o]; d[3] = by1[o]; d[4] = ac; d[5] = o;
            srow[kept] = skey[i];
        }
        for (int j = i + 1 + tid; j < nvalid; j += nt) {
            if (sup[j]) continue;
            const int q = sidx[j];
            if (bcls[q] != ac) continue;
            if (iou_voc(a0, a1, a2, a3, bx0[q], by0[q], bx1[q], by1[q]) > thr) sup[j] = 1;
        }
        ++kept;
        __syncthreads();
    }
    if (tid == 0) count[img] = kept;
    for (int i = kept * 6 + tid; i < max_out * 6; i += nt) drow[i] = -1;
    for (int i = kept + tid; i < max_out; i += nt) srow[i] = 0.0f;
}

// ---- the anchor (YOLOv2) head: y2_detect_anchor_batch --------------------------------------------------------------
constexpr int kAnchorLanes = 1024;                     // the workgroup; above it a lane owns two decode and sort slots
constexpr int kAnchorSlotBytes = 8 + 5 * 4 + 1;        // sort word, four corners, class, suppressed flag

// grid (n), one workgroup per image of min(KP, 1024) lanes, KP = the next power of two of K = S * S * B (64 .. 2048).
//   1. slot i = lane + 1024 r is decoded from the raw head (anchor_decode.h: the values of y2_decode_anchors +
//      y2_class_argmax), taken to the pixels of the original image in float64 and cut, as detect_grid_kernel does;
//   2. bitonic sort of the 64-bit words, one compare-exchange PAIR per lane and pass (KP / 2 pairs: at 2048 slots every
//      lane of the 1024 works in every pass).  LDS is one array per field, and a lane's slots are 1024 apart, so the lanes
//      of a wave touch consecutive words: a pass reads and writes whole 256-byte bank rows for j >= 32 and meets at most
//      2 lanes per bank below that (pair p -> slot 2 (p - p % j) + p % j), against 2 everywhere for adjacent slots per lane;
//   3. detect_grid_kernel's walk: `kept` and sup[] are uniform, one barrier per kept row, none per suppressed row.
// LETTERBOX: the four products go through letterbox_map instead of the plain stretch; nothing else differs, and the
// `false` instantiation does not read net_size.
template <bool LETTERBOX>
__global__ __launch_bounds__(kAnchorLanes) void detect_anchor_kernel(const float* __restrict__ net,
                                                                     const float* __restrict__ anchors,
                                                                     const int64_t* __restrict__ table,
                                                                     const int32_t* __restrict__ index, int S, int B, int C,
                                                                     float score_thresh, float iou_thresh, int max_out,
                                                                     int KP, int net_size, int* __restrict__ det,
                                                                     float* __restrict__ score, int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // kAnchorSlotBytes per slot: 58 KB at 2048
    uint64_t* sword = (uint64_t*)smem;
    int* bx0 = (int*)(sword + KP);
    int *by0 = bx0 + KP, *bx1 = by0 + KP, *by1 = bx1 + KP, *bcls = by1 + KP;
    unsigned char* sup = (unsigned char*)(bcls + KP);
    __shared__ int s_valid;
    const int img = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int K = S * S * B, D = 5 + C;
    const int64_t* t = table + (size_t)kTable * (index ? index[img] : img);
    const int64_t h64 = t[1], w64 = t[2];
    const bool sized = h64 >= 1 && w64 >= 1 && h64 <= 0x7fffffff && w64 <= 0x7fffffff;
    const int im_h = sized ? (int)h64 : 1, im_w = sized ? (int)w64 : 1;
    const float* rows = net + (size_t)img * K * D;
    LetterboxMap lb = {};
    if (LETTERBOX) lb = letterbox_map(im_w, im_h, net_size);
    if (tid == 0) s_valid = 0;
    __syncthreads();
    for (int i = tid; i < KP; i += nt) {
        bool valid = false;
        float best = -INFINITY;
        if (i < K && sized) {
            const int cell = i / B, b = i - cell * B;
            const int row = cell / S, col = cell - row * S;
            const float* p = rows + (size_t)i * D;
            const AnchorBox bx = anchor_decode_box(p, anchors, b, row, col, S);
            float mx, sum;
            anchor_softmax_norm(p, C, mx, sum);
            int cls = 0;
            best = anchor_class_score(p, 0, bx.so, mx, sum);              // class_argmax_kernel: the first maximum
            for (int c = 1; c < C; ++c) {
                const float v = anchor_class_score(p, c, bx.so, mx, sum);
                if (v > best) {
                    best = v;
                    cls = c;
                }
            }
            double dx, dy, dw, dh;
            if (LETTERBOX) {
                dx = ((double)bx.cx * lb.n - lb.ox) * lb.sx; dy = ((double)bx.cy * lb.n - lb.oy) * lb.sy;
                dw = ((double)bx.w * lb.n) * lb.sx; dh = ((double)bx.h * lb.n) * lb.sy;
            } else {
                dx = (double)bx.cx * (double)im_w; dy = (double)bx.cy * (double)im_h;
                dw = (double)bx.w * (double)im_w; dh = (double)bx.h * (double)im_h;
            }
            const double lim = 1073741824.0;                              // 2^30: checked BEFORE any conversion to int
            valid = best > score_thresh && fabs(dx) < lim && fabs(dy) < lim && fabs(dw) < lim && fabs(dh) < lim;
            if (valid) {
                const int x = (int)dx, y = (int)dy, w = (int)dw, h = (int)dh;   // >> 1 on an int is floor(. / 2)
                const int ulx = x - (w >> 1), uly = y - (h >> 1);
                const int xmin = max(ulx, 0), ymin = max(uly, 0);
                const int xmax = min(ulx + w - 1, im_w - 1), ymax = min(uly + h - 1, im_h - 1);
                valid = xmax >= xmin && ymax >= ymin;
                bx0[i] = xmin + 1; by0[i] = ymin + 1; bx1[i] = xmax + 1; by1[i] = ymax + 1;
                bcls[i] = cls;
            }
        }
        sword[i] = sort_word(valid ? best : -INFINITY, i);
        sup[i] = 0;
        if (valid) atomicAdd(&s_valid, 1);
    }
    __syncthreads();
    for (int k = 2; k <= KP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int pr = tid; pr < (KP >> 1); pr += nt) {
                const int lo = pr & (j - 1);
                const int i = ((pr - lo) << 1) | lo, l = i | j;
                const uint64_t a = sword[i], b = sword[l];
                const bool desc = (i & k) == 0;
                if (desc ? a < b : a > b) {
                    sword[i] = b;
                    sword[l] = a;
                }
            }
            __syncthreads();
        }
    // a valid score is > score_thresh >= -inf, so the valid candidates are exactly the first s_valid of the order
    const int nvalid = s_valid;
    const double thr = (double)iou_thresh;
    int* drow = det + (size_t)img * max_out * 6;
    float* srow = score + (size_t)img * max_out;
    int kept = 0;
    for (int i = 0; i < nvalid && kept < max_out; ++i) {
        if (sup[i]) continue;
        const uint64_t wd = sword[i];
        const int o = word_index(wd);
        const int ac = bcls[o];
        const double a0 = bx0[o], a1 = by0[o], a2 = bx1[o], a3 = by1[o];
        if (tid == 0) {
            int* d = drow + (size_t)kept * 6;
            d[0] = bx0[o]; d[1] = by0[o]; d[2] = bx1[o]; d[3] = by1[o]; d[4] = ac; d[5] = o;
            srow[kept] = word_key(wd);
        }
        for (int j = i + 1 + tid; j < nvalid; j += nt) {
            if (sup[j]) continue;
            const int q = word_index(sword[j]);
            if (bcls[q] != ac) continue;
            if (iou_voc(a0, a1, a2, a3, bx0[q], by0[q], bx1[q], by1[q]) > thr) sup[j] = 1;
        }
        ++kept;
        __syncthreads();
    }
    if (tid == 0) count[img] = kept;
    for (int i = kept * 6 + tid; i < max_out * 6; i += nt) drow[i] = -1;
    for (int i = kept + tid; i < max_out; i += nt) srow[i] = 0.0f;
}

// ---- one row per (candidate, class), as Darknet's `valid` writes: y2_detect_anchor_classes_batch ----------------------
constexpr int kClassLanes = 512;                       // the workgroup: n * C of them, up to three resident on a CU
constexpr int kClassSlotBytes = 8 + 4 * 4 + 1;         // sort word, four corners, suppressed flag: 50 KB at 2048

// grid (C, n), one workgroup per (class, image) of min(KP, 512) lanes, KP = the next power of two of K (64 .. 2048).
//   1. every lane decodes candidates lane, lane + lanes, ... from the raw head as detect_anchor_kernel does (the C
//      workgroups of an image repeat the box, and the softmax's normaliser where the objectness passes the threshold by
//      itself) but scores ONE class.  A valid candidate
//      writes its corners at its own index and its sort word at the next free COMPACT slot: per wave and round one
//      ballot, one LDS atomicAdd of the wave's count by its first lane, each lane's slot from the prefix of the ballot.
//      Which slot a word lands in cannot show: the words are distinct and the sort is total.
//   2. nvalid is uniform after the barrier; the bitonic sort runs over NP = the next power of two of nvalid (at least
//      64) and not over KP: the slots nvalid .. NP are filled with words below every valid one (-inf).
//   3. detect_anchor_kernel's walk without the class test: the segment holds one class.
// LETTERBOX as in detect_anchor_kernel.
template <bool LETTERBOX>
__global__ __launch_bounds__(kClassLanes) void detect_anchor_classes_kernel(
    const float* __restrict__ net, const float* __restrict__ anchors, const int64_t* __restrict__ table,
    const int32_t* __restrict__ index, int S, int B, int C, float score_thresh, float iou_thresh, int max_out, int KP,
    int net_size, int* __restrict__ det, float* __restrict__ score, int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // kClassSlotBytes per slot
    uint64_t* sword = (uint64_t*)smem;
    int* bx0 = (int*)(sword + KP);
    int *by0 = bx0 + KP, *bx1 = by0 + KP, *by1 = bx1 + KP;
    unsigned char* sup = (unsigned char*)(by1 + KP);
    __shared__ int s_valid;
    const int cls = blockIdx.x, img = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & (kWave - 1);
    const int K = S * S * B, D = 5 + C;
    const int64_t* t = table + (size_t)kTable * (index ? index[img] : img);
    const int64_t h64 = t[1], w64 = t[2];
    const bool sized = h64 >= 1 && w64 >= 1 && h64 <= 0x7fffffff && w64 <= 0x7fffffff;
    const int im_h = sized ? (int)h64 : 1, im_w = sized ? (int)w64 : 1;
    const float* rows = net + (size_t)img * K * D;
    LetterboxMap lb = {};
    if (LETTERBOX) lb = letterbox_map(im_w, im_h, net_size);
    if (tid == 0) s_valid = 0;
    __syncthreads();
    for (int base = 0; base < K; base += nt) {                    // uniform trips: every lane of a wave meets the ballot
        const int i = base + tid;
        bool valid = false;
        float v = -INFINITY;
        if (i < K && sized) {
            const int cell = i / B, b = i - cell * B;
            const int row = cell / S, col = cell - row * S;
            const float* p = rows + (size_t)i * D;
            const AnchorBox bx = anchor_decode_box(p, anchors, b, row, col, S);
            // score = so * (expf(<= 0) / sum) and sum holds the term expf(0) = 1, so score <= so in float32 (or it is
            // NaN): a candidate whose objectness alone does not pass is not valid in ANY class, and on a trained head
            // that is nearly all of them -- the class logits are not even read
            if (bx.so > score_thresh) {
                float mx, sum;
                anchor_softmax_norm(p, C, mx, sum);
                v = anchor_class_score(p, cls, bx.so, mx, sum);
            }
            double dx, dy, dw, dh;
            if (LETTERBOX) {
                dx = ((double)bx.cx * lb.n - lb.ox) * lb.sx; dy = ((double)bx.cy * lb.n - lb.oy) * lb.sy;
                dw = ((double)bx.w * lb.n) * lb.sx; dh = ((double)bx.h * lb.n) * lb.sy;
            } else {
                dx = (double)bx.cx * (double)im_w; dy = (double)bx.cy * (double)im_h;
                dw = (double)bx.w * (double)im_w; dh = (double)bx.h * (double)im_h;
            }
            const double lim = 1073741824.0;                              // 2^30: checked BEFORE any conversion to int
            valid = v > score_thresh && fabs(dx) < lim && fabs(dy) < lim && fabs(dw) < lim && fabs(dh) < lim;
            if (valid) {
                const int x = (int)dx, y = (int)dy, w = (int)dw, h = (int)dh;   // >> 1 on an int is floor(. / 2)
                const int ulx = x - (w >> 1), uly = y - (h >> 1);
                const int xmin = max(ulx, 0), ymin = max(uly, 0);
                const int xmax = min(ulx + w - 1, im_w - 1), ymax = min(uly + h - 1, im_h - 1);
                valid = xmax >= xmin && ymax >= ymin;
                bx0[i] = xmin + 1; by0[i] = ymin + 1; bx1[i] = xmax + 1; by1[i] = ymax + 1;
            }
        }
        const unsigned long long mask = __ballot(valid);
        int first = 0;
        if (lane == 0 && mask) first = atomicAdd(&s_valid, __popcll(mask));
        first = __shfl(first, 0, kWave);
        if (valid) sword[first + __popcll(mask & ((1ull << lane) - 1ull))] = sort_word(v, i);
    }
    __syncthreads();
    const int nvalid = s_valid;                                   // <= K <= KP
    int NP = kWave;
    while (NP < nvalid) NP <<= 1;
    for (int i = tid; i < NP; i += nt) {
        if (i >= nvalid) sword[i] = sort_word(-INFINITY, i);      // a valid score is > score_thresh >= -inf
        sup[i] = 0;
    }
    __syncthreads();
    for (int k = 2; k <= NP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int pr = tid; pr < (NP >> 1); pr += nt) {
                const int lo = pr & (j - 1);
                const int i = ((pr - lo) << 1) | lo, l = i | j;
                const uint64_t a = sword[i], b = sword[l];
                const bool desc = (i & k) == 0;
                if (desc ? a < b : a > b) {
                    sword[i] = b;
                    sword[l] = a;
                }
            }
            __syncthreads();
        }
    const double thr = (double)iou_thresh;
    const size_t seg = (size_t)img * C + cls;
    int* drow = det + seg * max_out * 6;
    float* srow = score + seg * max_out;
    int kept = 0;
    for (int i = 0; i < nvalid && kept < max_out; ++i) {
        if (sup[i]) continue;
        const uint64_t wd = sword[i];
        const int o = word_index(wd);
        const double a0 = bx0[o], a1 = by0[o], a2 = bx1[o], a3 = by1[o];
        if (tid == 0) {
            int* d = drow + (size_t)kept * 6;
            d[0] = bx0[o]; d[1] = by0[o]; d[2] = bx1[o]; d[3] = by1[o]; d[4] = cls; d[5] = o;
            srow[kept] = word_key(wd);
        }
        for (int j = i + 1 + tid; j < nvalid; j += nt) {
            if (sup[j]) continue;
            const int q = word_index(sword[j]);
            if (iou_voc(a0, a1, a2, a3, bx0[q], by0[q], bx1[q], by1[q]) > thr) sup[j] = 1;
        }
        ++kept;
        __syncthreads();
    }
    if (tid == 0) count[seg] = kept;
    for (int i = kept * 6 + tid; i < max_out * 6; i += nt) drow[i] = -1;
    for (int i = kept + tid; i < max_out; i += nt) srow[i] = 0.0f;
}

}  // namespace

extern "C" {

int y2_detect_grid_batch(const float* predict, const int64_t* table, const int32_t* index, int n, int S, int B,
                         int num_class, float object_thresh, float iou_thresh, int max_out, int* det, float* score,
                         int* count, void* stream) {
    if (!predict || !table || !det || !score || !count) return fail(Y2_ERR_ARG, "y2_detect_grid_batch: null pointer");
    if (n < 1) return fail(Y2_ERR_ARG, "y2_detect_grid_batch: n = %d", n);
    if (max_out < 1) return fail(Y2_ERR_ARG, "y2_detect_grid_batch: max_out = %d", max_out);
    if (S < 1 || B < 1 || num_class < 1 || S > kMaxCand || B > kMaxCand)
        return fail(Y2_ERR_ARG, "y2_detect_grid_batch: S = %d, B = %d, num_class = %d", S, B, num_class);
    if (S * S * B > kMaxCand)
        return fail(Y2_ERR_ARG, "y2_detect_grid_batch: S * S * B = %d candidates beyond Y2_DETECT_MAX_CANDIDATES = %d",
                    S * S * B, kMaxCand);
    int KP = kWave;
    while (KP < S * S * B) KP <<= 1;
    hipLaunchKernelGGL(detect_grid_kernel, dim3(n), dim3(KP), 0, (hipStream_t)stream, predict, table, index, S, B,
                       num_class, object_thresh, iou_thresh, max_out, KP, det, score, count);
    return launched("y2_detect_grid_batch");
}

// y2_detect_anchor_batch (net_size 0: the plain stretch) and y2_detect_anchor_batch_lb: detect_anchor_args' checks
// (detect_common.h) with this family's bounds, and the launch
static int detect_anchor_any(const char* name, const float* net, const float* anchors, const int64_t* table,
                             const int32_t* index, int n, int S, int B, int num_class, float score_thresh,
                             float iou_thresh, int max_out, int net_size, bool letterbox, int* det, float* score,
                             int* count, void* stream) {
    int KP;
    if (const int rc = detect_anchor_args(name, net && anchors && table && det && score && count, n, 0, "max_out",
                                          max_out, S, B, num_class, letterbox, net_size, &KP))
        return rc;
    const int lanes = KP < kAnchorLanes ? KP : kAnchorLanes;
    if (letterbox)
        hipLaunchKernelGGL(detect_anchor_kernel<true>, dim3(n), dim3(lanes), (size_t)KP * kAnchorSlotBytes,
                           (hipStream_t)stream, net, anchors, table, index, S, B, num_class, score_thresh, iou_thresh,
                           max_out, KP, net_size, det, score, count);
    else
        hipLaunchKernelGGL(detect_anchor_kernel<false>, dim3(n), dim3(lanes), (size_t)KP * kAnchorSlotBytes,
                           (hipStream_t)stream, net, anchors, table, index, S, B, num_class, score_thresh, iou_thresh,
                           max_out, KP, 0, det, score, count);
    return launched(name);
}

int y2_detect_anchor_batch(const float* net, const float* anchors, const int64_t* table, const int32_t* index, int n,
                           int S, int B, int num_class, float score_thresh, float iou_thresh, int max_out, int* det,
                           float* score, int* count, void* stream) {
    return detect_anchor_any("y2_detect_anchor_batch", net, anchors, table, index, n, S, B, num_class, score_thresh,
                             iou_thresh, max_out, 0, false, det, score, count, stream);
}

int y2_detect_anchor_batch_lb(const float* net, const float* anchors, const int64_t* table, const int32_t* index, int n,
                              int S, int B, int num_class, float score_thresh, float iou_thresh, int max_out,
                              int net_size, int* det, float* score, int* count, void* stream) {
    return detect_anchor_any("y2_detect_anchor_batch_lb", net, anchors, table, index, n, S, B, num_class, score_thresh,
                             iou_thresh, max_out, net_size, true, det, score, count, stream);
}

// the same for y2_detect_anchor_classes_batch and y2_detect_anchor_classes_batch_lb
static int detect_anchor_classes_any(const char* name, const float* net, const float* anchors, const int64_t* table,
                                     const int32_t* index, int n, int S, int B, int num_class, float score_thresh,
                                     float iou_thresh, int max_per_class, int net_size, bool letterbox, int* det,
                                     float* score, int* count, void* stream) {
    int KP;
    if (const int rc = detect_anchor_args(name, net && anchors && table && det && score && count, n, 65535,
                                          "max_per_class", max_per_class, S, B, num_class, letterbox, net_size, &KP))
        return rc;
    const int lanes = KP < kClassLanes ? KP : kClassLanes;
    if (letterbox)
        hipLaunchKernelGGL(detect_anchor_classes_kernel<true>, dim3(num_class, n), dim3(lanes),
                           (size_t)KP * kClassSlotBytes, (hipStream_t)stream, net, anchors, table, index, S, B, num_class,
                           score_thresh, iou_thresh, max_per_class, KP, net_size, det, score, count);
    else
        hipLaunchKernelGGL(detect_anchor_classes_kernel<false>, dim3(num_class, n), dim3(lanes),
                           (size_t)KP * kClassSlotBytes, (hipStream_t)stream, net, anchors, table, index, S, B, num_class,
                           score_thresh, iou_thresh, max_per_class, KP, 0, det, score, count);
    return launched(name);
}

int y2_detect_anchor_classes_batch(const float* net, const float* anchors, const int64_t* table, const int32_t* index,
                                   int n, int S, int B, int num_class, float score_thresh, float iou_thresh,
                                   int max_per_class, int* det, float* score, int* count, void* stream) {
    return detect_anchor_classes_any("y2_detect_anchor_classes_batch", net, anchors, table, index, n, S, B, num_class,
                                     score_thresh, iou_thresh, max_per_class, 0, false, det, score, count, stream);
}

int y2_detect_anchor_classes_batch_lb(const float* net, const float* anchors, const int64_t* table, const int32_t* index,
                                      int n, int S, int B, int num_class, float score_thresh, float iou_thresh,
                                      int max_per_class, int net_size, int* det, float* score, int* count,
                                      void* stream) {
    return detect_anchor_classes_any("y2_detect_anchor_classes_batch_lb", net, anchors, table, index, n, S, B, num_class,
                                     score_thresh, iou_thresh, max_per_class, net_size, true, det, score, count, stream);
}

int y2_voc_match_batch(const int* det, const float* score, const int* count, const double* boxes,
                       const int32_t* counts, const uint8_t* difficult, const int32_t* index, int n, int max_obj,
                       int max_out, float iou_thresh, int* flags, void* stream) {
    (void)score;
    return voc_match_any<false>("y2_voc_match_batch", det, count, boxes, counts, difficult, index, n, max_obj, max_out,
                                iou_thresh, flags, stream);
}

}  // extern "C"
