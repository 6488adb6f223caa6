// The word tree of the region layer (YOLO9000's softmax_tree; specification: utils/word_tree.py): the box-list loss with
// the hierarchical class term, its statistics, and the head rewrite every detect entry reads unchanged.  Compiled with
// -ffp-contract=off like ext.hip, whose ownership / coord / object / noobject arithmetic the loss repeats.
//
// Tables (utils/word_tree.py pack(); device memory, int32 [3 C + 2 G]): parent[C], group[C], child[C], group_offset[G],
// group_size[G].  The host cannot see their content, so every value read from them is cut into its range before it
// becomes an index (wt_span, the node checks of the walks) and every walk is a loop of at most max_depth + 1 levels:
// whatever the tables or the truth lists hold, no kernel here reads or writes outside a head row or a table, or spins.
#include <stdio.h>
#include <stdarg.h>
#include "common.h"
#include "kernels.h"
#include "region_math.h"
#include "word_tree_walk.h"
#include "../../include/yolo2_hip.h"

namespace y2 {
int set_error(int code, const char* msg);   // net.hip (y2_last_error)
}
using namespace y2;
static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return set_error(code, buf);
}

#define WTCHK(expr)                                                                         \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) return fail(Y2_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

Y2_DEV float wt_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---------------------------------------------------------------------------
// Loss (specification: utils/word_tree.py yolov2_loss_boxes_tree).  Grid (ceil(S*S*B / 256), N) and the ownership rule
// of yolov2_loss_boxes_kernel (ext.hip): a workgroup owns 256 consecutive (cell, anchor) slots of one image.
//   A  one thread per slot: the coord / object / noobject terms, bit for bit that kernel's arithmetic; the five box
//      gradients of the slot go to LDS, the truth's node (or -1: un-owned, or a class outside [0, C)) too
//   B  the workgroup writes its 256 rows -- one contiguous span of 256 (5 + C) floats -- with consecutive lanes on
//      consecutive floats: the box gradients from LDS, zero in every class entry
//   C  each wave takes the owned rows among its 64 slots in ascending order (a ballot, so the order is fixed) and walks
//      the truth's path to the root, at most max_depth + 1 levels: per level the lanes stride over the node's group,
//      form its maximum and its sum through a butterfly, add class_scale (lse - logit[node]) and overwrite the group's
//      gradients.  A barrier stands between B and C: both write the same words
// One partial [4] per workgroup, the finalize of the flat loss: two runs give the same bits.
// ---------------------------------------------------------------------------
struct WtLossArgs {
    const float* net;      // [N][S][S][B][5+C]
    const float* truth;    // [N][T][5]
    const int* ntruth;     // [N]
    const float* anchors;  // [B][2] cell units
    float* dnet;           // same shape as net (nullable)
    float* partial;        // [N][gridDim.x][4]
    WtTables tb;
    int N, S, B, C, T;
    float image_size, coord, obj, noobj, cls, thresh, prior;
    int area_weight;
};
constexpr int kWtNoOwner = 0x7fffffff;

__global__ __launch_bounds__(256) void yolov2_loss_boxes_tree_kernel(WtLossArgs a) {
    __shared__ float tr[Y2_MAX_BOXES][4];
    __shared__ int tcls[Y2_MAX_BOXES];
    __shared__ int own[256];
    __shared__ int node[256];
    __shared__ float g5[256][5];
    __shared__ float red[4][256];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int cells = a.S * a.S, D = 5 + a.C, slots = cells * a.B;
    const int slot0 = blockIdx.x * 256;
    const float fs = (float)a.S;
    const int nt = min(max(a.ntruth[n], 0), a.T);
    own[tid] = kWtNoOwner;
    node[tid] = -1;
    __syncthreads();
    for (int k = tid; k < nt; k += 256) {
        const float* tk = a.truth + ((size_t)n * a.T + k) * 5;
        const float gx = tk[0] / a.image_size * fs, gy = tk[1] / a.image_size * fs;
        const float gw = tk[2] / a.image_size * fs, gh = tk[3] / a.image_size * fs;
        tr[k][0] = gx; tr[k][1] = gy; tr[k][2] = gw; tr[k][3] = gh;
        tcls[k] = (int)tk[4];
        // the cell of the truth (cut into the grid: every index below is in range whatever the list holds)
        const int q = (int)fminf(fmaxf(gx, 0.0f), fs - 1.0f), r = (int)fminf(fmaxf(gy, 0.0f), fs - 1.0f);
        int bs = 0;
        float bi = -1.0f;
        for (int j = 0; j < a.B; ++j) {   // the anchor whose shape fits best, first one on ties
            const float kw = a.anchors[2 * j], kh = a.anchors[2 * j + 1];
            const float inter = fminf(gw, kw) * fminf(gh, kh);
            const float si = inter / (gw * gh + kw * kh - inter);
            if (si > bi) { bi = si; bs = j; }
        }
        const int slot = (r * a.S + q) * a.B + bs - slot0;
        if (slot >= 0 && slot < 256) atomicMin(&own[slot], k);
    }
    __syncthreads();
    // ---- A
    float t_coord = 0.f, t_obj = 0.f, t_noobj = 0.f;
    const float invN = 1.0f / (float)a.N;
    const int p = slot0 + tid;
    if (p < slots) {
        const int cell = p / a.B, b = p - cell * a.B;
        const int row = cell / a.S, col = cell - row * a.S;
        const float* t = a.net + ((size_t)n * slots + p) * D;
        const float aw = a.anchors[2 * b], ah = a.anchors[2 * b + 1];
        const float sx = v2_sigmoid(t[0]), sy = v2_sigmoid(t[1]), so = v2_sigmoid(t[4]);
        const float px = sx + (float)col, py = sy + (float)row, pw = aw * expf(t[2]), ph = ah * expf(t[3]);
        const int owner = own[tid];
        float* g = g5[tid];
        if (owner != kWtNoOwner) {
            const float gx = tr[owner][0], gy = tr[owner][1], gw = tr[owner][2], gh = tr[owner][3];
            const float wgt = a.area_weight ? a.coord * (2.0f - (gw / fs) * (gh / fs)) : a.coord;
            const float ex = sx - (gx - (float)col), ey = sy - (gy - (float)row);
            const float ew = t[2] - logf(gw / aw), eh = t[3] - logf(gh / ah);
            t_coord += wgt * (ex * ex + ey * ey + ew * ew + eh * eh);
            const float iou = v2_iou(px, py, pw, ph, gx, gy, gw, gh);
            const float eo = so - iou;
            t_obj += a.obj * eo * eo;
            const int k = tcls[owner];
            node[tid] = (k >= 0 && k < a.C) ? k : -1;   // a class index outside [0, C): no class term
            g[0] = wgt * 2.0f * ex * sx * (1.0f - sx) * invN;
            g[1] = wgt * 2.0f * ey * sy * (1.0f - sy) * invN;
            g[2] = wgt * 2.0f * ew * invN;
            g[3] = wgt * 2.0f * eh * invN;
            g[4] = a.obj * 2.0f * eo * so * (1.0f - so) * invN;
        } else {
            float best = 0.f;
            for (int k = 0; k < nt; ++k) best = fmaxf(best, v2_iou(px, py, pw, ph, tr[k][0], tr[k][1], tr[k][2], tr[k][3]));
            const bool pen = best <= a.thresh;
            if (pen) t_noobj += a.noobj * so * so;
            const bool prior = a.prior > 0.0f;
            const float dx = sx - 0.5f, dy = sy - 0.5f;
            if (prior) t_coord += a.prior * (dx * dx + dy * dy + t[2] * t[2] + t[3] * t[3]);
            g[0] = prior ? a.prior * 2.0f * dx * sx * (1.0f - sx) * invN : 0.f;
            g[1] = prior ? a.prior * 2.0f * dy * sy * (1.0f - sy) * invN : 0.f;
            g[2] = prior ? a.prior * 2.0f * t[2] * invN : 0.f;
            g[3] = prior ? a.prior * 2.0f * t[3] * invN : 0.f;
            g[4] = pen ? a.noobj * 2.0f * so * so * (1.0f - so) * invN : 0.f;
        }
    }
    __syncthreads();
    // ---- B
    const size_t base = ((size_t)n * slots + slot0) * D;
    if (a.dnet) {
        float* gb = a.dnet + base;
        const int total = min(256, slots - slot0) * D;       // at most 256 (5 + Y2_WORD_TREE_MAX_NODES): an int
        const int dr = 256 / D, de = 256 - dr * D;           // idx += 256 as (row, element)
        int r = tid / D, e = tid - r * D;
        for (int idx = tid; idx < total; idx += 256) {
            gb[idx] = e < 5 ? g5[r][e] : 0.f;
            r += dr; e += de;
            if (e >= D) { e -= D; r += 1; }
        }
    }
    __syncthreads();
    // ---- C
    const int lane = tid & 63, wave = tid >> 6;
    float t_cls = 0.f;
    unsigned long long todo = __ballot(node[tid] >= 0);
    while (todo) {
        const int s = wave * 64 + __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const float* t = a.net + base + (size_t)s * D + 5;
        float* g = a.dnet ? a.dnet + base + (size_t)s * D + 5 : nullptr;
        int at = __builtin_amdgcn_readfirstlane(node[s]);
        for (int level = 0; level <= a.tb.max_depth; ++level) {
            if (at < 0 || at >= a.C) break;
            int off, size;
            wt_span(a.tb, __builtin_amdgcn_readfirstlane(a.tb.group[at]), off, size);
            if (size <= 0) break;
            float m = -INFINITY;
            for (int j = lane; j < size; j += 64) m = fmaxf(m, t[off + j]);
            m = wt_wave_max(m);
            float se = 0.f;
            for (int j = lane; j < size; j += 64) se += expf(t[off + j] - m);
            se = wt_wave_sum(se);
            const float lse = m + logf(se);
            t_cls += a.cls * (lse - t[at]);
            if (g)
                for (int j = lane; j < size; j += 64)
                    g[off + j] = a.cls * (expf(t[off + j] - lse) - (off + j == at ? 1.0f : 0.0f)) * invN;
            at = __builtin_amdgcn_readfirstlane(a.tb.parent[at]);
        }
    }
    red[0][tid] = t_coord; red[1][tid] = t_obj; red[2][tid] = t_noobj; red[3][tid] = lane == 0 ? t_cls : 0.f;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + s];
        __syncthreads();
    }
    if (tid < 4) a.partial[((size_t)n * gridDim.x + blockIdx.x) * 4 + tid] = red[tid][0];
}
// one workgroup of 256: lane (j, k) adds component k of the partials j, j + 64, ... in ascending order, then a tree
__global__ __launch_bounds__(256) void yolov2_loss_boxes_tree_finalize_kernel(const float* partial, float* loss, int count,
                                                                              int N) {
    __shared__ float red[256];
    const int tid = threadIdx.x, k = tid & 3;
    float p = 0.f;
    for (int j = tid >> 2; j < count; j += 64) p += partial[(size_t)j * 4 + k];
    red[tid] = p;
    __syncthreads();
    for (int s = 128; s >= 4; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        float tot = 0.f;
        for (int c = 0; c < 4; ++c) { loss[c] = red[c] / (float)N; tot += loss[c]; }
        loss[4] = tot;
    }
}

// ---------------------------------------------------------------------------
// Statistics (specification: utils/word_tree.py region_stats_boxes_tree): yolov2_region_stats_kernel (ext.hip) with the
// class statistic of a truth = abs[node], the product of the conditionals on its path to the root (Darknet's avg_cat).
// A thread per truth walks the path, one group's softmax per level; the product runs leaf first.
// ---------------------------------------------------------------------------
struct WtStatsArgs {
    const float* net;      // [N][S][S][B][5+C]
    const float* truth;    // [N][T][5]
    const int* ntruth;     // [N]
    const float* anchors;  // [B][2] cell units
    int* partial;          // [N][8]: float bits of sum iou, sum class, sum obj, sum sig(to); int recall, count, classed; 0
    WtTables tb;
    int N, S, B, C, T;
    float image_size;
};

__global__ __launch_bounds__(256) void yolov2_region_stats_tree_kernel(WtStatsArgs a) {
    __shared__ int red[8][256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int cells = a.S * a.S, D = 5 + a.C, slots = cells * a.B;
    const float fs = (float)a.S;
    const int nt = min(max(a.ntruth[n], 0), a.T);
    const float* base = a.net + (size_t)n * slots * D;
    float s_all = 0.f;
    for (int p = tid; p < slots; p += 256) s_all += v2_sigmoid(base[(size_t)p * D + 4]);
    float s_iou = 0.f, s_cls = 0.f, s_obj = 0.f;
    int recall = 0, count = 0, classed = 0;
    for (int k = tid; k < nt; k += 256) {
        const float* tk = a.truth + ((size_t)n * a.T + k) * 5;
        const float gx = tk[0] / a.image_size * fs, gy = tk[1] / a.image_size * fs;
        const float gw = tk[2] / a.image_size * fs, gh = tk[3] / a.image_size * fs;
        // the cell of the truth, cut into the grid as the loss cuts it: every index below is in range
        const int q = (int)fminf(fmaxf(gx, 0.0f), fs - 1.0f), r = (int)fminf(fmaxf(gy, 0.0f), fs - 1.0f);
        int bs = 0;
        float bi = -1.0f;
        for (int j = 0; j < a.B; ++j) {   // the anchor whose shape fits best, first one on ties
            const float kw = a.anchors[2 * j], kh = a.anchors[2 * j + 1];
            const float inter = fminf(gw, kw) * fminf(gh, kh);
            const float si = inter / (gw * gh + kw * kh - inter);
            if (si > bi) { bi = si; bs = j; }
        }
        const float* t = base + ((size_t)(r * a.S + q) * a.B + bs) * D;
        const float px = v2_sigmoid(t[0]) + (float)q, py = v2_sigmoid(t[1]) + (float)r;
        const float pw = a.anchors[2 * bs] * expf(t[2]), ph = a.anchors[2 * bs + 1] * expf(t[3]);
        const float iou = v2_iou(px, py, pw, ph, gx, gy, gw, gh);
        s_iou += iou;
        s_obj += v2_sigmoid(t[4]);
        recall += iou > 0.5f ? 1 : 0;
        count += 1;
        const int c = (int)tk[4];
        if (c >= 0 && c < a.C) {
            float prob = 1.0f;
            int at = c;
            for (int level = 0; level <= a.tb.max_depth; ++level) {
                if (at < 0 || at >= a.C) break;
                int off, size;
                wt_span(a.tb, a.tb.group[at], off, size);
                if (size <= 0) break;
                float m = t[5 + off];
                for (int j = 1; j < size; ++j) m = fmaxf(m, t[5 + off + j]);
                float se = 0.f;
                for (int j = 0; j < size; ++j) se += expf(t[5 + off + j] - m);
                prob *= expf(t[5 + at] - m) / se;
                at = a.tb.parent[at];
            }
            s_cls += prob;
            classed += 1;
        }
    }
    red[0][tid] = __float_as_int(s_iou); red[1][tid] = __float_as_int(s_cls); red[2][tid] = __float_as_int(s_obj);
    red[3][tid] = __float_as_int(s_all); red[4][tid] = recall; red[5][tid] = count; red[6][tid] = classed; red[7][tid] = 0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 8; ++k) red[k][tid] = v2_stats_add(k, red[k][tid], red[k][tid + s]);
        __syncthreads();
    }
    if (tid < 8) a.partial[(size_t)n * 8 + tid] = red[tid][0];
}

// the finalize of the flat statistics (ext.hip): lane (j, k) adds component k of images j, j + 32, ..., then a tree
__global__ __launch_bounds__(256) void yolov2_region_stats_tree_finalize_kernel(const int* partial, float* stats, int N,
                                                                                float slots) {
    __shared__ int red[256];
    const int tid = threadIdx.x, k = tid & 7;
    int p = 0;                                           // the bit pattern of 0.0f too
    for (int j = tid >> 3; j < N; j += 32) p = v2_stats_add(k, p, partial[(size_t)j * 8 + k]);
    red[tid] = p;
    __syncthreads();
    for (int s = 128; s >= 8; s >>= 1) {
        if (tid < s) red[tid] = v2_stats_add(k, red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) {
        const float count = (float)red[5], classed = (float)red[6];
        stats[0] = red[5] > 0 ? __int_as_float(red[0]) / count : 0.f;
        stats[1] = red[6] > 0 ? __int_as_float(red[1]) / classed : 0.f;
        stats[2] = red[5] > 0 ? __int_as_float(red[2]) / count : 0.f;
        stats[3] = __int_as_float(red[3]) / slots;
        stats[4] = red[5] > 0 ? (float)red[4] / count : 0.f;
        stats[5] = count;
    }
}

// ---------------------------------------------------------------------------
// Head rewrite (specification: utils/word_tree.py word_tree_head).  One wave per row, four rows per workgroup.  The walk
// needs one group per level, never the whole row: the lanes stride over the group, a butterfly gives its first maximum
// (value, then lowest index) and its sum, and cond of the maximum is 1 / sum exactly as the specification's exp(0) / sum.
// The wave has read every logit it needs before it knows `top`, and it writes only behind that, so out == net is safe;
// rows are disjoint between waves.  No LDS: the node limit is the index arithmetic's.
// ---------------------------------------------------------------------------
constexpr int kWtHeadRows = 4;

__global__ __launch_bounds__(256) void word_tree_head_kernel(const float* net, float* out, int* top_out, float* prob_out,
                                                             WtTables tb, int rows, float thresh) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * kWtHeadRows + (threadIdx.x >> 6);
    if (row >= rows) return;                                 // a whole wave leaves: no barrier follows
    const int D = 5 + tb.C;
    const float* t = net + (size_t)row * D;
    float* o = out + (size_t)row * D;
    const float box = lane < 5 ? t[lane] : 0.f;
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
    if (lane < 5) o[lane] = box;
    for (int e = lane; e < tb.C; e += 64) o[5 + e] = e == top ? 0.0f : -INFINITY;
    if (lane == 0) {
        if (top_out) top_out[row] = top;
        if (prob_out) prob_out[row] = p;
    }
}

extern "C" {

static int wt_box_blocks(int S, int B) { return (S * S * B + 255) / 256; }

size_t y2_yolov2_loss_boxes_tree_workspace_bytes(int batch, int S, int B) {
    if (batch < 1 || S < 1 || B < 1 || (long long)S * S * B > Y2_LOSS_BOXES_MAX_SLOTS) return 0;
    return (size_t)batch * wt_box_blocks(S, B) * 4 * sizeof(float) + 256;
}

int y2_yolov2_loss_boxes_tree(const float* net, const float* truth, const int* ntruth, const float* anchors,
                              const int* tables, int batch, int S, int B, int num_class, int G, int max_depth,
                              int max_boxes, float image_size, const float* scales, float* loss, float* dnet,
                              void* workspace, void* stream) {
    const char* me = "y2_yolov2_loss_boxes_tree";
    if (!net || !truth || !ntruth || !anchors || !loss || !workspace) return fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wt_tree_check(me, tables, num_class, G, max_depth)) return e;
    if (batch < 1 || batch > 65535 || S < 1 || B < 1 || !(image_size > 0.0f))
        return fail(Y2_ERR_ARG, "%s: batch = %d, S = %d, B = %d, image_size = %g", me, batch, S, B, (double)image_size);
    if ((long long)S * S * B > Y2_LOSS_BOXES_MAX_SLOTS)
        return fail(Y2_ERR_ARG, "%s: S * S * B = %lld beyond Y2_LOSS_BOXES_MAX_SLOTS = %d", me, (long long)S * S * B,
                    Y2_LOSS_BOXES_MAX_SLOTS);
    if (max_boxes < 1 || max_boxes > Y2_MAX_BOXES)
        return fail(Y2_ERR_ARG, "%s: max_boxes = %d outside 1..%d", me, max_boxes, Y2_MAX_BOXES);
    WtLossArgs a{};
    a.net = net; a.truth = truth; a.ntruth = ntruth; a.anchors = anchors; a.dnet = dnet; a.partial = (float*)workspace;
    a.tb = wt_tables(tables, num_class, G, max_depth);
    a.N = batch; a.S = S; a.B = B; a.C = num_class; a.T = max_boxes; a.image_size = image_size;
    a.coord = scales ? scales[0] : 1.0f; a.obj = scales ? scales[1] : 5.0f; a.noobj = scales ? scales[2] : 1.0f;
    a.cls = scales ? scales[3] : 1.0f; a.thresh = scales ? scales[4] : 0.6f;
    a.area_weight = scales ? (scales[5] != 0.0f) : 0; a.prior = scales ? scales[6] : 0.0f;
    const int blocks = wt_box_blocks(S, B);
    hipLaunchKernelGGL(yolov2_loss_boxes_tree_kernel, dim3(blocks, batch), dim3(256), 0, (hipStream_t)stream, a);
    WTCHK(hipGetLastError());
    hipLaunchKernelGGL(yolov2_loss_boxes_tree_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a.partial, loss,
                       blocks * batch, batch);
    WTCHK(hipGetLastError());
    return Y2_OK;
}

int y2_yolov2_region_stats_tree(const float* net, const float* truth, const int* ntruth, const float* anchors,
                                const int* tables, int batch, int S, int B, int num_class, int G, int max_depth,
                                int max_boxes, float image_size, float* stats, void* workspace, void* stream) {
    const char* me = "y2_yolov2_region_stats_tree";
    if (!net || !truth || !ntruth || !anchors || !stats || !workspace) return fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wt_tree_check(me, tables, num_class, G, max_depth)) return e;
    if (batch < 1 || batch > 65535 || S < 1 || B < 1 || B > 8 || !(image_size > 0.0f))
        return fail(Y2_ERR_ARG, "%s: batch = %d, S = %d, B = %d (1..8), image_size = %g", me, batch, S, B,
                    (double)image_size);
    if ((long long)S * S * B > Y2_LOSS_BOXES_MAX_SLOTS)
        return fail(Y2_ERR_ARG, "%s: S * S * B = %lld beyond Y2_LOSS_BOXES_MAX_SLOTS = %d", me, (long long)S * S * B,
                    Y2_LOSS_BOXES_MAX_SLOTS);
    if (max_boxes < 1 || max_boxes > Y2_MAX_BOXES)
        return fail(Y2_ERR_ARG, "%s: max_boxes = %d outside 1..%d", me, max_boxes, Y2_MAX_BOXES);
    WtStatsArgs a{};
    a.net = net; a.truth = truth; a.ntruth = ntruth; a.anchors = anchors; a.partial = (int*)workspace;
    a.tb = wt_tables(tables, num_class, G, max_depth);
    a.N = batch; a.S = S; a.B = B; a.C = num_class; a.T = max_boxes; a.image_size = image_size;
    hipLaunchKernelGGL(yolov2_region_stats_tree_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, a);
    WTCHK(hipGetLastError());
    hipLaunchKernelGGL(yolov2_region_stats_tree_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a.partial,
                       stats, batch, (float)batch * (float)S * (float)S * (float)B);
    WTCHK(hipGetLastError());
    return Y2_OK;
}

int y2_word_tree_head(const float* net, const int* tables, int rows, int num_class, int G, int max_depth,
                      float tree_thresh, float* out, int* top, float* prob, void* stream) {
    const char* me = "y2_word_tree_head";
    if (!net || !out) return fail(Y2_ERR_ARG, "%s: null pointer", me);
    if (int e = wt_tree_check(me, tables, num_class, G, max_depth)) return e;
    if (rows < 1) return fail(Y2_ERR_ARG, "%s: rows = %d: at least 1", me, rows);
    if (!(tree_thresh >= 0.0f && tree_thresh < 1.0f))
        return fail(Y2_ERR_ARG, "%s: tree_thresh = %g outside [0, 1)", me, (double)tree_thresh);
    const unsigned blocks = ((unsigned)rows + kWtHeadRows - 1) / kWtHeadRows;
    hipLaunchKernelGGL(word_tree_head_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, net, out, top, prob,
                       wt_tables(tables, num_class, G, max_depth), rows, tree_thresh);
    WTCHK(hipGetLastError());
    return Y2_OK;
}

}  // extern "C"
