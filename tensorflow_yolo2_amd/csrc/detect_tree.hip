// Detection on a word-tree head from the tree's node instead of the class row ("Detection from the node").
// A tree model has exactly one class per candidate -- the node where the walk down the tree stops -- and its score is
// the objectness, so the rows need the walk's answer and elements 0..4 of a head row, never the class logits again:
//   y2_word_tree_top                 the walk of word_tree_head_kernel (word_tree.hip) without the row rewrite
//   y2_detect_anchor_tree_batch      detect_anchor_kernel (detect.hip) with class = top[candidate], score = sigmoid(to)
//   y2_detect_anchor_tree_batch_dk   the boxes of detect_anchor_classes_dk_kernel (darknet_io.hip), flat rows
// The sort and walk loops restate those kernels', as darknet_io.hip restates detect.hip's; the arithmetic they share is
// the headers'.  Bit-equal to the old two-launch path on the rewritten rows, and to the host specification
// (utils/detect_batch: anchor_detect, anchor_detect_tree_darknet).  Compiled with -ffp-contract=off.
#include <cmath>
#include "data_common.h"
#include "kernels.h"
#include "anchor_decode.h"
#include "letterbox.h"
#include "detect_common.h"
#include "darknet_box.h"
#include "word_tree_walk.h"
using namespace y2;

namespace {

// ---- the walk: y2_word_tree_top -------------------------------------------------------------------------------------
constexpr int kTopRows = 4;                            // a wave per row, four rows per workgroup

// word_tree_head_kernel's walk, statement for statement: the lanes stride over one group per level, a butterfly gives
// its first maximum (value, then lowest index) and its sum, cond of the maximum is 1 / sum.  Nothing is written but top
// / prob. obj_thresh >= 0: a row whose objectness sigmoid(to) -- anchor_decode_box's expression -- is not > obj_thresh
// (NaN included) answers top = -1, prob = 0 before any class logit is read; the test is uniform over the wave.  No LDS.
__global__ __launch_bounds__(256) void word_tree_top_kernel(const float* __restrict__ net, int* __restrict__ top_out,
                                                            float* __restrict__ prob_out, WtTables tb, int rows,
                                                            float thresh, float obj_thresh) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * kTopRows + (threadIdx.x >> 6);
    if (row >= rows) return;                                 // a whole wave leaves: no barrier follows
    const int D = 5 + tb.C;
    const float* t = net + (size_t)row * D;
    if (obj_thresh >= 0.0f) {
        const float so = 1.f / (1.f + expf(-t[4]));
        if (!(so > obj_thresh)) {
            if (lane == 0) {
                top_out[row] = -1;
                if (prob_out) prob_out[row] = 0.0f;
            }
            return;
        }
    }
    float p = 1.0f;
    int g = 0, top = 0;
    for (int level = 0; level <= tb.max_depth; ++level) {
        int off, size;
        wt_span(tb, g, off, size);
        if (size <= 0) break;
        float m = -INFINITY;
        int arg = 0x7fffffff;
        for (int j = lane; j < size; j += 64) {
            const float v = t[5 + off + j];
            if (v > m) { m = v; arg = off + j; }             // ascending j: the first maximum of the lane's share
        }
        for (int s = 32; s > 0; s >>= 1) {
            const float om = __shfl_xor(m, s, 64);
            const int oa = __shfl_xor(arg, s, 64);
            if (om > m || (om == m && oa < arg)) { m = om; arg = oa; }
        }
        const int j = (arg >= off && arg < off + size) ? arg : off;   // (a group of NaN or -inf alone: its first node)
        float se = 0.f;
        for (int i = lane; i < size; i += 64) se += expf(t[5 + off + i] - m);
        se = wt_wave_sum(se);
        const float pc = p * (1.0f / se);
        if (pc > thresh) {
            p = pc;
            top = j;
            const int ch = __builtin_amdgcn_readfirstlane(tb.child[j]);
            if (ch < 0 || ch >= tb.G) break;                 // a leaf
            g = ch;
        } else {
            if (level == 0) { top = j; p = pc; }             // the root group always answers
            break;                                           // else: the node whose children were not convincing
        }
    }
    if (lane == 0) {
        top_out[row] = top;
        if (prob_out) prob_out[row] = p;
    }
}

// ---- the integer rows: y2_detect_anchor_tree_batch -------------------------------------------------------------------
constexpr int kTreeLanes = 1024;                       // the workgroup, as detect_anchor_kernel's
constexpr int kTreeSlotBytes = 8 + 5 * 4 + 1;          // sort word, four values of the box, class, suppressed flag

// grid (n), one workgroup per image of min(KP, 1024) lanes: detect_anchor_kernel (detect.hip) where the class of
// candidate i is top[i] and its score sigmoid(to).  A candidate whose top lies outside [0, C) -- the -1 of a row the
// walk skipped -- is not valid; top is compared and stored, never an index.  A lane reads elements 0..4 of its row and
// nothing behind them: at a row stride of 5 + C floats that is one cache line per candidate.  The decode-cut, the sort
// and the walk are that kernel's, statement for statement.
template <bool LETTERBOX>
__global__ __launch_bounds__(kTreeLanes) void detect_anchor_tree_kernel(
    const float* __restrict__ net, const int* __restrict__ top, const float* __restrict__ anchors,
    const int64_t* __restrict__ table, const int32_t* __restrict__ index, int S, int B, int C, float score_thresh,
    float iou_thresh, int max_out, int KP, int net_size, int* __restrict__ det, float* __restrict__ score,
    int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // kTreeSlotBytes per slot: 58 KB at 2048
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
    const int* tops = top + (size_t)img * K;
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
            const int cls = tops[i];
            best = bx.so;
            double dx, dy, dw, dh;
            if (LETTERBOX) {
                dx = ((double)bx.cx * lb.n - lb.ox) * lb.sx; dy = ((double)bx.cy * lb.n - lb.oy) * lb.sy;
                dw = ((double)bx.w * lb.n) * lb.sx; dh = ((double)bx.h * lb.n) * lb.sy;
            } else {
                dx = (double)bx.cx * (double)im_w; dy = (double)bx.cy * (double)im_h;
                dw = (double)bx.w * (double)im_w; dh = (double)bx.h * (double)im_h;
            }
            const double lim = 1073741824.0;                              // 2^30: checked BEFORE any conversion to int
            valid = cls >= 0 && cls < C && best > score_thresh && fabs(dx) < lim && fabs(dy) < lim && fabs(dw) < lim &&
                    fabs(dh) < lim;
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

// ---- Darknet's rows: y2_detect_anchor_tree_batch_dk -------------------------------------------------------------------
// grid (n), the same workgroup and LDS per slot.  The box, the validity (score > score_thresh, the four un-mapped values
// finite; nothing else but top in [0, C)), the IoU and the row are detect_anchor_classes_dk_kernel's (darknet_io.hip),
// and so are its ballot compaction and the sort over the next power of two of the valid candidates; the rows are FLAT,
// one descending order per image, under the class-aware walk: a kept box suppresses later boxes of its own node.
__global__ __launch_bounds__(kTreeLanes) void detect_anchor_tree_dk_kernel(
    const float* __restrict__ net, const int* __restrict__ top, const float* __restrict__ anchors,
    const int64_t* __restrict__ table, const int32_t* __restrict__ index, int S, int B, int C, float score_thresh,
    float iou_thresh, int max_out, int KP, int net_size, int* __restrict__ det, float* __restrict__ score,
    int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // kTreeSlotBytes per slot
    uint64_t* sword = (uint64_t*)smem;
    float* fx = (float*)(sword + KP);
    float *fy = fx + KP, *fw = fy + KP, *fh = fw + KP;
    int* bcls = (int*)(fh + KP);
    unsigned char* sup = (unsigned char*)(bcls + KP);
    __shared__ int s_valid;
    const int img = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & (kWave - 1);
    const int K = S * S * B, D = 5 + C;
    const int64_t* t = table + (size_t)kTable * (index ? index[img] : img);
    const int64_t h64 = t[1], w64 = t[2];
    const bool sized = h64 >= 1 && w64 >= 1 && h64 <= 0x7fffffff && w64 <= 0x7fffffff;
    const int im_h = sized ? (int)h64 : 1, im_w = sized ? (int)w64 : 1;
    const float* rows = net + (size_t)img * K * D;
    const int* tops = top + (size_t)img * K;
    const DarknetMap m = darknet_map(im_w, im_h, net_size);
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
            const int cls = tops[i];
            if (cls >= 0 && cls < C) v = bx.so;
            if (v > score_thresh) {                               // the two double divisions only where the score passes
                float x = (float)(((double)bx.cx - m.offx) / m.scx), y = (float)(((double)bx.cy - m.offy) / m.scy);
                float w = bx.w * m.rw, h = bx.h * m.rh;
                x = x * m.fw; w = w * m.fw; y = y * m.fh; h = h * m.fh;
                valid = isfinite(x) && isfinite(y) && isfinite(w) && isfinite(h);
                if (valid) {
                    fx[i] = x; fy[i] = y; fw[i] = w; fh[i] = h;
                    bcls[i] = cls;
                }
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
        if (i >= nvalid) sword[i] = sort_word(-INFINITY, i);      // a valid score is > score_thresh, so not -inf
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
    int* drow = det + (size_t)img * max_out * 6;
    float* srow = score + (size_t)img * max_out;
    int kept = 0;
    for (int i = 0; i < nvalid && kept < max_out; ++i) {
        if (sup[i]) continue;
        const uint64_t wd = sword[i];
        const int o = word_index(wd);
        const int ac = bcls[o];
        const float ax = fx[o], ay = fy[o], aw = fw[o], ah = fh[o];
        if (tid == 0) {
            int* d = drow + (size_t)kept * 6;
            float xmin = dk_corner(ax, aw, -1.0), ymin = dk_corner(ay, ah, -1.0);
            float xmax = dk_corner(ax, aw, 1.0), ymax = dk_corner(ay, ah, 1.0);
            if (xmin < 1.0f) xmin = 1.0f;
            if (ymin < 1.0f) ymin = 1.0f;
            if (xmax > m.fw) xmax = m.fw;
            if (ymax > m.fh) ymax = m.fh;
            d[0] = __float_as_int(xmin); d[1] = __float_as_int(ymin);
            d[2] = __float_as_int(xmax); d[3] = __float_as_int(ymax);
            d[4] = ac; d[5] = o;
            srow[kept] = word_key(wd);
        }
        for (int j = i + 1 + tid; j < nvalid; j += nt) {
            if (sup[j]) continue;
            const int q = word_index(sword[j]);
            if (bcls[q] != ac) continue;
            if (iou_darknet(ax, ay, aw, ah, fx[q], fy[q], fw[q], fh[q]) > iou_thresh) sup[j] = 1;
        }
        ++kept;
        __syncthreads();
    }
    if (tid == 0) count[img] = kept;
    for (int i = kept * 6 + tid; i < max_out * 6; i += nt) drow[i] = -1;
    for (int i = kept + tid; i < max_out; i += nt) srow[i] = 0.0f;
}

}  // namespace

extern "C" {

int y2_word_tree_top(const float* net, const int* tables, int rows, int num_class, int G, int max_depth,
                     float tree_thresh, float obj_thresh, int* top, float* prob, void* stream) {
    const char* me = "y2_word_tree_top";
    if (!net || !top) return fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wt_tree_check(me, tables, num_class, G, max_depth)) return e;
    if (rows < 1) return fail(Y2_ERR_ARG, "%s: rows = %d: at least 1", me, rows);
    if (!(tree_thresh >= 0.0f && tree_thresh < 1.0f))
        return fail(Y2_ERR_ARG, "%s: tree_thresh = %g outside [0, 1)", me, (double)tree_thresh);
    if (!std::isfinite(obj_thresh))
        return fail(Y2_ERR_ARG, "%s: obj_thresh = %g is not finite", me, (double)obj_thresh);
    const unsigned blocks = ((unsigned)rows + kTopRows - 1) / kTopRows;
    hipLaunchKernelGGL(word_tree_top_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, net, top, prob,
                       wt_tables(tables, num_class, G, max_depth), rows, tree_thresh, obj_thresh);
    return launched(me);
}

int y2_detect_anchor_tree_batch(const float* net, const int* top, const float* anchors, const int64_t* table,
                                const int32_t* index, int n, int S, int B, int num_class, float score_thresh,
                                float iou_thresh, int max_out, int net_size, int* det, float* score, int* count,
                                void* stream) {
    const char* name = "y2_detect_anchor_tree_batch";
    const bool letterbox = net_size != 0;                 // 0: the plain stretch; else it must be 32 S
    int KP;
    const bool pointers = net && top && anchors && table && det && score && count;
    if (const int rc = detect_anchor_args(name, pointers, n, 0, "max_out", max_out, S, B, num_class, letterbox, net_size,
                                          &KP))
        return rc;
    const int lanes = KP < kTreeLanes ? KP : kTreeLanes;
    if (letterbox)
        hipLaunchKernelGGL(detect_anchor_tree_kernel<true>, dim3(n), dim3(lanes), (size_t)KP * kTreeSlotBytes,
                           (hipStream_t)stream, net, top, anchors, table, index, S, B, num_class, score_thresh, iou_thresh,
                           max_out, KP, net_size, det, score, count);
    else
        hipLaunchKernelGGL(detect_anchor_tree_kernel<false>, dim3(n), dim3(lanes), (size_t)KP * kTreeSlotBytes,
                           (hipStream_t)stream, net, top, anchors, table, index, S, B, num_class, score_thresh, iou_thresh,
                           max_out, KP, 0, det, score, count);
    return launched(name);
}

int y2_detect_anchor_tree_batch_dk(const float* net, const int* top, const float* anchors, const int64_t* table,
                                   const int32_t* index, int n, int S, int B, int num_class, float score_thresh,
                                   float iou_thresh, int max_out, int net_size, int* det, float* score, int* count,
                                   void* stream) {
    const char* name = "y2_detect_anchor_tree_batch_dk";
    int KP;
    const bool pointers = net && top && anchors && table && det && score && count;
    if (const int rc = detect_anchor_args(name, pointers, n, 0, "max_out", max_out, S, B, num_class, true, net_size, &KP))
        return rc;
    const int lanes = KP < kTreeLanes ? KP : kTreeLanes;
    hipLaunchKernelGGL(detect_anchor_tree_dk_kernel, dim3(n), dim3(lanes), (size_t)KP * kTreeSlotBytes,
                       (hipStream_t)stream, net, top, anchors, table, index, S, B, num_class, score_thresh, iou_thresh,
                       max_out, KP, net_size, det, score, count);
    return launched(name);
}

}  // extern "C"
