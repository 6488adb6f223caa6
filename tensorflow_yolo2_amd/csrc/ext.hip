// YOLOv2 pieces that north_star names but the reference does NOT contain (SURVEY §8 rows a-x1,
// a-x2): stride-2 reorg / passthrough concat, anchor-box decode, per-image greedy NMS.
// There is no reference code to follow; the specification is oracle/ext_ref.py (this repo),
// and parity is bit-exact for the index work (reorg, NMS keep lists) -- the file is compiled
// with -ffp-contract=off and the IoU uses the spec's fp32 operation order.
#include <stdio.h>
#include "common.h"
#include "kernels.h"
#include "anchor_decode.h"
#include "region_math.h"
#include "../../include/yolo2_hip.h"

#include <stdarg.h>
#include <float.h>
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

#define EXTCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) return fail(Y2_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// ---------------------------------------------------------------------------
// reorg (space-to-depth, block s): y[n, h/s, w/s, ((h%s)*s + w%s)*C + c] = x[n, h, w, c]
// forward = 0 runs the inverse permutation (its gradient).  16-byte moves when C % 4 == 0.
// ---------------------------------------------------------------------------
template <int VEC>
__global__ void reorg_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C, int s,
                             int forward, int ldy, int coff) {
    const int Cv = C / VEC;
    const size_t total = (size_t)N * H * W * Cv;
    const int Ho = H / s, Wo = W / s;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int cv = (int)(i % Cv);
        size_t p = i / Cv;
        const int w = (int)(p % W); p /= W;
        const int h = (int)(p % H);
        const int n = (int)(p / H);
        const size_t fine = (((size_t)n * H + h) * W + w) * C + (size_t)cv * VEC;
        const size_t coarse = (((size_t)n * Ho + h / s) * Wo + w / s) * ldy + coff +
                              (size_t)((h % s) * s + (w % s)) * C + (size_t)cv * VEC;
        if (VEC == 4) {
            if (forward) *(f32x4*)(y + coarse) = *(const f32x4*)(x + fine);
            else *(f32x4*)(y + fine) = *(const f32x4*)(x + coarse);
        } else {
            if (forward) y[coarse] = x[fine];
            else y[fine] = x[coarse];
        }
    }
}

static int reorg_launch(const float* x, float* y, int N, int H, int W, int C, int s, int forward, int ldy, int coff,
                        hipStream_t st) {
    const bool vec = (C % 4) == 0 && (ldy % 4) == 0 && (coff % 4) == 0;
    const size_t total = (size_t)N * H * W * (vec ? C / 4 : C);
    size_t nb = (total + 255) / 256;
    if (nb > 65536) nb = 65536;
    if (nb < 1) nb = 1;
    if (vec) hipLaunchKernelGGL(reorg_kernel<4>, dim3((unsigned)nb), dim3(256), 0, st, x, y, N, H, W, C, s, forward, ldy, coff);
    else hipLaunchKernelGGL(reorg_kernel<1>, dim3((unsigned)nb), dim3(256), 0, st, x, y, N, H, W, C, s, forward, ldy, coff);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

// copy channels [0, C) of src [M][lds] (offset soff) into dst [M][ldd] (offset doff)
__global__ void chan_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t M, int C, int lds,
                                 int soff, int ldd, int doff) {
    const size_t total = M * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t m = i / C;
        dst[m * ldd + doff + c] = src[m * lds + soff + c];
    }
}
static int chan_copy(const float* src, float* dst, size_t M, int C, int lds, int soff, int ldd, int doff, hipStream_t st) {
    size_t nb = (M * C + 255) / 256;
    if (nb > 65536) nb = 65536;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(chan_copy_kernel, dim3((unsigned)nb), dim3(256), 0, st, src, dst, M, C, lds, soff, ldd, doff);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

// dst += src (the 26x26x512 activation of the YOLOv2 graph has two consumers -- the pool and the passthrough --
// so its gradient is the sum of two paths)
__global__ void accumulate_kernel(float4* __restrict__ dst, const float4* __restrict__ src, size_t n4, float* dt,
                                  const float* st, size_t tail0, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 a = dst[i];
        const float4 b = src[i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        dst[i] = a;
    }
    if (blockIdx.x == 0)
        for (size_t i = tail0 + threadIdx.x; i < n; i += blockDim.x) dt[i] += st[i];
}

// ---------------------------------------------------------------------------
// anchor decode: net [N,S,S,B,5+C] = (tx, ty, tw, th, to, class logits)
//   bx = (sigmoid(tx) + col)/S, by = (sigmoid(ty) + row)/S, bw = pw*exp(tw)/S, bh = ph*exp(th)/S
//   score[c] = sigmoid(to) * softmax(class logits)[c]
// ---------------------------------------------------------------------------
__global__ void decode_anchors_kernel(const float* __restrict__ net, const float* __restrict__ anchors,
                                      float* __restrict__ boxes, float* __restrict__ scores, int N, int S, int B, int C) {
    const int total = N * S * S * B;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int b = i % B;
    const int cell = (i / B) % (S * S);
    const int row = cell / S, col = cell % S;
    const float* p = net + (size_t)i * (5 + C);
    const AnchorBox bx = anchor_decode_box(p, anchors, b, row, col, S);    // anchor_decode.h: shared with detect.hip
    boxes[(size_t)i * 4 + 0] = bx.cx;
    boxes[(size_t)i * 4 + 1] = bx.cy;
    boxes[(size_t)i * 4 + 2] = bx.w;
    boxes[(size_t)i * 4 + 3] = bx.h;
    float mx, sum;
    anchor_softmax_norm(p, C, mx, sum);
    for (int c = 0; c < C; ++c) scores[(size_t)i * C + c] = anchor_class_score(p, c, bx.so, mx, sum);
}

// ---------------------------------------------------------------------------
// per-image greedy NMS.  One block per image, K <= 4096 candidates.
//   order: score descending, ties by ascending index (bitonic sort of (score, index) in LDS);
//   candidates with score < score_thresh are dropped;
//   walk the order; a kept box suppresses every later box with IoU > iou_thresh
//   (and, if class_aware, the same class id).  keep[n][0..count) = original indices.
// IoU (fp32, this exact operation order -- oracle/ext_ref.py: nms_iou):
//   x1 = cx - w*0.5, x2 = cx + w*0.5 (same for y); iw = max(0, min(x2a,x2b) - max(x1a,x1b));
//   inter = iw*ih; union = (wa*ha + wb*hb) - inter; iou = union > 0 ? inter/union : 0
// ---------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(1024) void nms_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                    const int* __restrict__ classes, int K, float iou_thresh,
                                                    float score_thresh, int max_out, int class_aware,
                                                    int* __restrict__ keep, int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 33 bytes per candidate (132 KB at 4096)
    float* skey = (float*)smem;
    int* sidx = (int*)(skey + KP);
    float *bx1 = (float*)(sidx + KP), *by1 = bx1 + KP, *bx2 = by1 + KP, *by2 = bx2 + KP, *barea = by2 + KP;
    int* bcls = (int*)(barea + KP);
    unsigned char* sup = (unsigned char*)(bcls + KP);
    __shared__ int s_cnt, s_valid;
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* bb = boxes + (size_t)n * K * 4;
    const float* sc = scores + (size_t)n * K;
    for (int i = tid; i < KP; i += 1024) {
        const bool v = i < K && sc[i] >= score_thresh;
        skey[i] = v ? sc[i] : -INFINITY;
        sidx[i] = i;
    }
    __syncthreads();
    // bitonic sort, descending by (score, -index)
    for (int k = 2; k <= KP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < KP; i += 1024) {
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
    if (tid == 0) { s_cnt = 0; s_valid = 0; }
    __syncthreads();
    for (int i = tid; i < KP; i += 1024) {
        const bool v = skey[i] > -INFINITY;
        if (v) {
            const int o = sidx[i];
            const float cx = bb[o * 4 + 0], cy = bb[o * 4 + 1], w = bb[o * 4 + 2], h = bb[o * 4 + 3];
            const float hw = w * 0.5f, hh = h * 0.5f;
            bx1[i] = cx - hw; bx2[i] = cx + hw; by1[i] = cy - hh; by2[i] = cy + hh;
            barea[i] = w * h;
            bcls[i] = classes ? classes[(size_t)n * K + o] : 0;
            atomicAdd(&s_valid, 1);
        }
        sup[i] = 0;
    }
    __syncthreads();
    const int nvalid = s_valid;   // valid entries are the first nvalid of the sorted order
    for (int i = 0; i < nvalid; ++i) {
        if (s_cnt >= max_out) break;
        if (!sup[i]) {
            if (tid == 0) keep[(size_t)n * max_out + s_cnt] = sidx[i];
            const float ax1 = bx1[i], ay1 = by1[i], ax2 = bx2[i], ay2 = by2[i], aa = barea[i];
            const int ac = bcls[i];
            for (int j = i + 1 + tid; j < nvalid; j += 1024) {
                if (sup[j]) continue;
                const float iw = fmaxf(0.f, fminf(ax2, bx2[j]) - fmaxf(ax1, bx1[j]));
                const float ih = fmaxf(0.f, fminf(ay2, by2[j]) - fmaxf(ay1, by1[j]));
                const float inter = iw * ih;
                const float uni = (aa + barea[j]) - inter;
                const float iou = uni > 0.f ? inter / uni : 0.f;
                if (iou > iou_thresh && (!class_aware || bcls[j] == ac)) sup[j] = 1;
            }
            __syncthreads();
            if (tid == 0) s_cnt = s_cnt + 1;
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) count[n] = s_cnt;
    for (int i = s_cnt + tid; i < max_out; i += 1024) keep[(size_t)n * max_out + i] = -1;
}

// ---------------------------------------------------------------------------
// standalone 2x2/2 SAME max pool on fp32 NHWC (tf.nn.max_pool, reference darknet.py:24-25) and its gradient
// (first maximum in row-major window order, like MaxPoolGrad and like the fused pooling of bn.hip).  The
// network executor pools inside its BN pass; this op exists for composed graphs (the YOLOv2 passthrough
// needs the UN-pooled 26x26 activation as well as the pooled one).
// ---------------------------------------------------------------------------
__global__ void maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ dy,
                               float* __restrict__ dx, int N, int H, int W, int C) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const size_t total = (size_t)N * Ho * Wo * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t p = i / C;
        const int wo = (int)(p % Wo); p /= Wo;
        const int ho = (int)(p % Ho);
        const int n = (int)(p / Ho);
        float best = -INFINITY;
        int arg = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int h = 2 * ho + (d >> 1), w = 2 * wo + (d & 1);
            if (h < H && w < W) {
                const float v = x[(((size_t)n * H + h) * W + w) * C + c];
                if (v > best) { best = v; arg = d; }
            }
        }
        if (y) y[i] = best;
        if (dx) {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int h = 2 * ho + (d >> 1), w = 2 * wo + (d & 1);
                if (h < H && w < W) dx[(((size_t)n * H + h) * W + w) * C + c] = (d == arg) ? dy[i] : 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// YOLOv2 anchor-box loss, forward + gradient in one kernel (specification: oracle/ext_ref.py yolov2_loss; the
// reference has no anchor model).  One block per image: the image's ground-truth boxes (one per responsible
// cell of the reference's label grid) go to LDS, then one thread per (cell, anchor) pair decodes its
// prediction, finds its best IoU over those boxes and writes its whole gradient row.
// ---------------------------------------------------------------------------
struct V2LossArgs {
    const float* net;      // [N][S][S][B][5+C]
    const float* labels;   // [N][S][S][5+C]
    const float* anchors;  // [B][2] cell units
    float* dnet;           // same shape as net (nullable)
    float* partial;        // [N][4] coord, object, noobject, class of one image
    int N, S, B, C;
    float image_size, coord, obj, noobj, cls, thresh;
};
constexpr int kV2MaxTruth = 1024;

// v2_sigmoid, v2_iou: region_math.h

__global__ __launch_bounds__(256) void yolov2_loss_kernel(V2LossArgs a) {
    __shared__ float tr[kV2MaxTruth][4];
    __shared__ int ntr;
    __shared__ float red[4][256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int cells = a.S * a.S, D = 5 + a.C, LD = 5 + a.C;
    const float fs = (float)a.S;
    if (tid == 0) ntr = 0;
    __syncthreads();
    for (int cell = tid; cell < cells; cell += 256) {
        const float* lab = a.labels + ((size_t)n * cells + cell) * LD;
        if (lab[0] > 0.0f) {
            const int k = atomicAdd(&ntr, 1);
            tr[k][0] = lab[1] / a.image_size * fs; tr[k][1] = lab[2] / a.image_size * fs;
            tr[k][2] = lab[3] / a.image_size * fs; tr[k][3] = lab[4] / a.image_size * fs;
        }
    }
    __syncthreads();
    const int nt = ntr;
    float t_coord = 0.f, t_obj = 0.f, t_noobj = 0.f, t_cls = 0.f;
    const float invN = 1.0f / (float)a.N;
    for (int p = tid; p < cells * a.B; p += 256) {
        const int cell = p / a.B, b = p - cell * a.B;
        const int row = cell / a.S, col = cell - row * a.S;
        const float* t = a.net + (((size_t)n * cells + cell) * a.B + b) * D;
        float* g = a.dnet ? a.dnet + (((size_t)n * cells + cell) * a.B + b) * D : nullptr;
        const float* lab = a.labels + ((size_t)n * cells + cell) * LD;
        const float aw = a.anchors[2 * b], ah = a.anchors[2 * b + 1];
        const float sx = v2_sigmoid(t[0]), sy = v2_sigmoid(t[1]), so = v2_sigmoid(t[4]);
        const float px = sx + (float)col, py = sy + (float)row, pw = aw * expf(t[2]), ph = ah * expf(t[3]);
        bool responsible = false;
        float gx = 0.f, gy = 0.f, gw = 1.f, gh = 1.f;
        if (lab[0] > 0.0f) {
            gx = lab[1] / a.image_size * fs; gy = lab[2] / a.image_size * fs;
            gw = lab[3] / a.image_size * fs; gh = lab[4] / a.image_size * fs;
            int bs = 0;
            float bi = -1.0f;
            for (int k = 0; k < a.B; ++k) {   // the anchor whose shape fits best, first one on ties
                const float kw = a.anchors[2 * k], kh = a.anchors[2 * k + 1];
                const float inter = fminf(gw, kw) * fminf(gh, kh);
                const float si = inter / (gw * gh + kw * kh - inter);
                if (si > bi) { bi = si; bs = k; }
            }
            responsible = (bs == b);
        }
        if (responsible) {
            const float ex = sx - (gx - (float)col), ey = sy - (gy - (float)row);
            const float ew = t[2] - logf(gw / aw), eh = t[3] - logf(gh / ah);
            t_coord += a.coord * (ex * ex + ey * ey + ew * ew + eh * eh);
            const float iou = v2_iou(px, py, pw, ph, gx, gy, gw, gh);
            const float eo = so - iou;
            t_obj += a.obj * eo * eo;
            int k = 0;
            float bestl = lab[5], m = t[5];
            for (int c = 1; c < a.C; ++c) {
                if (lab[5 + c] > bestl) { bestl = lab[5 + c]; k = c; }     // class = argmax of the one-hot
                m = fmaxf(m, t[5 + c]);
            }
            float se = 0.f;
            for (int c = 0; c < a.C; ++c) se += expf(t[5 + c] - m);
            const float lse = m + logf(se);
            t_cls += a.cls * (lse - t[5 + k]);
            if (g) {
                g[0] = a.coord * 2.0f * ex * sx * (1.0f - sx) * invN;
                g[1] = a.coord * 2.0f * ey * sy * (1.0f - sy) * invN;
                g[2] = a.coord * 2.0f * ew * invN;
                g[3] = a.coord * 2.0f * eh * invN;
                g[4] = a.obj * 2.0f * eo * so * (1.0f - so) * invN;
                for (int c = 0; c < a.C; ++c)
                    g[5 + c] = a.cls * (expf(t[5 + c] - lse) - (c == k ? 1.0f : 0.0f)) * invN;
            }
        } else {
            float best = 0.f;
            for (int k = 0; k < nt; ++k) best = fmaxf(best, v2_iou(px, py, pw, ph, tr[k][0], tr[k][1], tr[k][2], tr[k][3]));
            const bool pen = best <= a.thresh;
            if (pen) t_noobj += a.noobj * so * so;
            if (g) {
                g[0] = g[1] = g[2] = g[3] = 0.f;
                g[4] = pen ? a.noobj * 2.0f * so * so * (1.0f - so) * invN : 0.f;
                for (int c = 0; c < a.C; ++c) g[5 + c] = 0.f;
            }
        }
    }
    red[0][tid] = t_coord; red[1][tid] = t_obj; red[2][tid] = t_noobj; red[3][tid] = t_cls;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + s];
        __syncthreads();
    }
    if (tid < 4) a.partial[n * 4 + tid] = red[tid][0];
}
__global__ void yolov2_loss_finalize_kernel(const float* partial, float* loss, int N) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < 4; ++k) p[k] += partial[n * 4 + k];
    float tot = 0.f;
    for (int k = 0; k < 4; ++k) { loss[k] = p[k] / (float)N; tot += loss[k]; }
    loss[4] = tot;
}

// ---------------------------------------------------------------------------
// The same loss on BOX LISTS (specification: utils/region_loss.py yolov2_loss_boxes): every ground-truth box of an
// image is kept, truth [N][T][5] = cx, cy, w, h in pixels and the class index, ntruth [N].  Grid (ceil(S*S*B / 256), N):
// a workgroup owns 256 consecutive (cell, anchor) slots of one image.  It stages ALL truths of the image in LDS with
// the slot each one claims (its cell and its best-fitting anchor), settles the ownership of its own slots with
// atomicMin on the truth index (the lowest index wins whatever the order of arrival), then one thread per slot writes
// the slot's terms and its whole gradient row: an owned slot the coord / object / class terms of its owner, any other
// slot the noobject term under the best IoU over all truths and, while the prior is on, the pull toward its anchor.
// One partial [4] per workgroup; the finalize adds them in a fixed order, so two runs give the same bits.
// ---------------------------------------------------------------------------
struct V2BoxLossArgs {
    const float* net;      // [N][S][S][B][5+C]
    const float* truth;    // [N][T][5]
    const int* ntruth;     // [N]
    const float* anchors;  // [B][2] cell units
    float* dnet;           // same shape as net (nullable)
    float* partial;        // [N][gridDim.x][4]
    int N, S, B, C, T;
    float image_size, coord, obj, noobj, cls, thresh, prior;
    int area_weight;
};
constexpr int kV2NoOwner = 0x7fffffff;

__global__ __launch_bounds__(256) void yolov2_loss_boxes_kernel(V2BoxLossArgs a) {
    __shared__ float tr[Y2_MAX_BOXES][4];
    __shared__ int tcls[Y2_MAX_BOXES];
    __shared__ int own[256];
    __shared__ float red[4][256];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int cells = a.S * a.S, D = 5 + a.C, slots = cells * a.B;
    const int slot0 = blockIdx.x * 256;
    const float fs = (float)a.S;
    const int nt = min(max(a.ntruth[n], 0), a.T);
    own[tid] = kV2NoOwner;
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
    float t_coord = 0.f, t_obj = 0.f, t_noobj = 0.f, t_cls = 0.f;
    const float invN = 1.0f / (float)a.N;
    const int p = slot0 + tid;
    if (p < slots) {
        const int cell = p / a.B, b = p - cell * a.B;
        const int row = cell / a.S, col = cell - row * a.S;
        const float* t = a.net + ((size_t)n * slots + p) * D;
        float* g = a.dnet ? a.dnet + ((size_t)n * slots + p) * D : nullptr;
        const float aw = a.anchors[2 * b], ah = a.anchors[2 * b + 1];
        const float sx = v2_sigmoid(t[0]), sy = v2_sigmoid(t[1]), so = v2_sigmoid(t[4]);
        const float px = sx + (float)col, py = sy + (float)row, pw = aw * expf(t[2]), ph = ah * expf(t[3]);
        const int owner = own[tid];
        if (owner != kV2NoOwner) {
            const float gx = tr[owner][0], gy = tr[owner][1], gw = tr[owner][2], gh = tr[owner][3];
            const float wgt = a.area_weight ? a.coord * (2.0f - (gw / fs) * (gh / fs)) : a.coord;
            const float ex = sx - (gx - (float)col), ey = sy - (gy - (float)row);
            const float ew = t[2] - logf(gw / aw), eh = t[3] - logf(gh / ah);
            t_coord += wgt * (ex * ex + ey * ey + ew * ew + eh * eh);
            const float iou = v2_iou(px, py, pw, ph, gx, gy, gw, gh);
            const float eo = so - iou;
            t_obj += a.obj * eo * eo;
            const int k = tcls[owner];
            const bool has_class = k >= 0 && k < a.C;   // a class index outside [0, C): no class term (caller's contract)
            float lse = 0.f;
            if (has_class) {
                float m = t[5];
                for (int c = 1; c < a.C; ++c) m = fmaxf(m, t[5 + c]);
                float se = 0.f;
                for (int c = 0; c < a.C; ++c) se += expf(t[5 + c] - m);
                lse = m + logf(se);
                t_cls += a.cls * (lse - t[5 + k]);
            }
            if (g) {
                g[0] = wgt * 2.0f * ex * sx * (1.0f - sx) * invN;
                g[1] = wgt * 2.0f * ey * sy * (1.0f - sy) * invN;
                g[2] = wgt * 2.0f * ew * invN;
                g[3] = wgt * 2.0f * eh * invN;
                g[4] = a.obj * 2.0f * eo * so * (1.0f - so) * invN;
                for (int c = 0; c < a.C; ++c)
                    g[5 + c] = has_class ? a.cls * (expf(t[5 + c] - lse) - (c == k ? 1.0f : 0.0f)) * invN : 0.f;
            }
        } else {
            float best = 0.f;
            for (int k = 0; k < nt; ++k) best = fmaxf(best, v2_iou(px, py, pw, ph, tr[k][0], tr[k][1], tr[k][2], tr[k][3]));
            const bool pen = best <= a.thresh;
            if (pen) t_noobj += a.noobj * so * so;
            const bool prior = a.prior > 0.0f;
            const float dx = sx - 0.5f, dy = sy - 0.5f;
            if (prior) t_coord += a.prior * (dx * dx + dy * dy + t[2] * t[2] + t[3] * t[3]);
            if (g) {
                g[0] = prior ? a.prior * 2.0f * dx * sx * (1.0f - sx) * invN : 0.f;
                g[1] = prior ? a.prior * 2.0f * dy * sy * (1.0f - sy) * invN : 0.f;
                g[2] = prior ? a.prior * 2.0f * t[2] * invN : 0.f;
                g[3] = prior ? a.prior * 2.0f * t[3] * invN : 0.f;
                g[4] = pen ? a.noobj * 2.0f * so * so * (1.0f - so) * invN : 0.f;
                for (int c = 0; c < a.C; ++c) g[5 + c] = 0.f;
            }
        }
    }
    red[0][tid] = t_coord; red[1][tid] = t_obj; red[2][tid] = t_noobj; red[3][tid] = t_cls;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + s];
        __syncthreads();
    }
    if (tid < 4) a.partial[((size_t)n * gridDim.x + blockIdx.x) * 4 + tid] = red[tid][0];
}
// one workgroup of 256: lane (j, k) adds component k of the partials j, j + 64, ... in ascending order, then a tree
__global__ __launch_bounds__(256) void yolov2_loss_boxes_finalize_kernel(const float* partial, float* loss, int count, int N) {
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
// Region statistics (specification: utils/region_loss.py region_stats_boxes): the numbers of Darknet's region-layer log
// line, from the tensors the box-list loss reads.  One workgroup of 256 per image.  Pass 1: the lanes walk the image's
// S*S*B slots and add sig(to).  Pass 2: the lanes walk the image's truths; each derives its truth's cell and
// best-fitting anchor exactly as the loss does, decodes the prediction there and adds the IoU, the objectness, the class
// probability (valid class only) and the counts.  EVERY listed truth counts, owner of its slot or not.  The four float
// sums and three counts go through one LDS tree per image into partial[n][8]; the finalize adds the images in a fixed
// order (lane (j, k): component k of images j, j + 32, ... ascending, then a tree), so two runs give the same bits.
// ---------------------------------------------------------------------------
struct V2RegionStatsArgs {
    const float* net;      // [N][S][S][B][5+C]
    const float* truth;    // [N][T][5]
    const int* ntruth;     // [N]
    const float* anchors;  // [B][2] cell units
    int* partial;          // [N][8]: float bits of sum iou, sum class, sum obj, sum sig(to); int recall, count, classed; 0
    int N, S, B, C, T;
    float image_size;
};

// v2_stats_add (components 0..3 are float bit patterns, 4..7 integers): region_math.h

__global__ __launch_bounds__(256) void yolov2_region_stats_kernel(V2RegionStatsArgs a) {
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
            float m = t[5];
            for (int j = 1; j < a.C; ++j) m = fmaxf(m, t[5 + j]);
            float se = 0.f;
            for (int j = 0; j < a.C; ++j) se += expf(t[5 + j] - m);
            s_cls += expf(t[5 + c] - m) / se;
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

// stats[6] = mean IoU, mean class probability, mean objectness at the truths, mean sig(to) over every slot, recall at
// IoU 0.5, the truth count.  A mean over nothing is 0 (Darknet prints NaN there)
__global__ __launch_bounds__(256) void yolov2_region_stats_finalize_kernel(const int* partial, float* stats, int N,
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

extern "C" {

int y2_maxpool2x2(const float* x, float* y, int N, int H, int W, int C, void* stream) {
    if (!x || !y) return fail(Y2_ERR_ARG, "null tensor");
    const size_t total = (size_t)N * ((H + 1) / 2) * ((W + 1) / 2) * C;
    size_t nb = (total + 255) / 256;
    if (nb > 65536) nb = 65536;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, y, nullptr, nullptr, N, H,
                       W, C);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

int y2_maxpool2x2_backward(const float* x, const float* dy, float* dx, int N, int H, int W, int C, void* stream) {
    if (!x || !dy || !dx) return fail(Y2_ERR_ARG, "null tensor");
    const size_t total = (size_t)N * ((H + 1) / 2) * ((W + 1) / 2) * C;
    size_t nb = (total + 255) / 256;
    if (nb > 65536) nb = 65536;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, nullptr, dy, dx, N, H,
                       W, C);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

int y2_reorg(const float* x, float* y, int N, int H, int W, int C, int stride, int forward, void* stream) {
    if (!x || !y) return fail(Y2_ERR_ARG, "null tensor");
    if (stride < 1 || H % stride || W % stride) return fail(Y2_ERR_ARG, "H and W must be multiples of the stride");
    // forward: x fine [N,H,W,C] -> y coarse; inverse: x coarse -> y fine [N,H,W,C]
    return reorg_launch(x, y, N, H, W, C, stride, forward ? 1 : 0, stride * stride * C, 0, (hipStream_t)stream);
}

int y2_passthrough_concat(const float* fine, const float* coarse, float* out, int N, int H, int W, int Cf, int Cc,
                          void* stream) {
    if (!fine || !coarse || !out) return fail(Y2_ERR_ARG, "null tensor");
    const int ld = 4 * Cf + Cc;
    int rc = reorg_launch(fine, out, N, 2 * H, 2 * W, Cf, 2, 1, ld, 0, (hipStream_t)stream);
    if (rc) return rc;
    return chan_copy(coarse, out, (size_t)N * H * W, Cc, Cc, 0, ld, 4 * Cf, (hipStream_t)stream);
}

int y2_passthrough_concat_backward(const float* dout, float* dfine, float* dcoarse, int N, int H, int W, int Cf, int Cc,
                                   void* stream) {
    if (!dout || !dfine || !dcoarse) return fail(Y2_ERR_ARG, "null tensor");
    const int ld = 4 * Cf + Cc;
    int rc = reorg_launch(dout, dfine, N, 2 * H, 2 * W, Cf, 2, 0, ld, 0, (hipStream_t)stream);
    if (rc) return rc;
    return chan_copy(dout, dcoarse, (size_t)N * H * W, Cc, ld, 4 * Cf, Cc, 0, (hipStream_t)stream);
}

int y2_decode_anchors(const float* net, const float* anchors, float* boxes, float* scores, int N, int S, int B, int C,
                      void* stream) {
    if (!net || !anchors || !boxes || !scores) return fail(Y2_ERR_ARG, "null tensor");
    if (N < 1 || S < 1 || B < 1 || C < 1) return fail(Y2_ERR_ARG, "bad shape");
    const int total = N * S * S * B;
    hipLaunchKernelGGL(decode_anchors_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, net, anchors,
                       boxes, scores, N, S, B, C);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

int y2_nms(const float* boxes, const float* scores, const int* classes, int N, int K, float iou_thresh,
           float score_thresh, int max_out, int class_aware, int* keep, int* count, void* stream) {
    if (!boxes || !scores || !keep || !count) return fail(Y2_ERR_ARG, "null tensor");
    if (N < 1 || K < 1 || K > 4096 || max_out < 1) return fail(Y2_ERR_ARG, "need 1 <= K <= 4096 candidates per image");
    if (class_aware && !classes) return fail(Y2_ERR_ARG, "class-aware NMS needs class ids");
    hipStream_t st = (hipStream_t)stream;
#define NMS_LAUNCH(KP)                                                                                          \
    do {                                                                                                        \
        const int lds = KP * 33 + 64;                                                                           \
        EXTCHK(hipFuncSetAttribute((const void*)nms_kernel<KP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds)); \
        hipLaunchKernelGGL(nms_kernel<KP>, dim3(N), dim3(1024), lds, st, boxes, scores, classes, K, iou_thresh, \
                           score_thresh, max_out, class_aware, keep, count);                                    \
    } while (0)
    if (K <= 1024) NMS_LAUNCH(1024);
    else if (K <= 2048) NMS_LAUNCH(2048);
    else NMS_LAUNCH(4096);
#undef NMS_LAUNCH
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

int y2_accumulate(float* dst, const float* src, size_t n, void* stream) {
    if (!dst || !src) return fail(Y2_ERR_ARG, "null tensor");
    const size_t n4 = n / 4;
    size_t nb = (n4 + 255) / 256;
    if (nb > 16384) nb = 16384;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (float4*)dst,
                       (const float4*)src, n4, dst, src, n4 * 4, n);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

// best class score and its index per box: scores [R][C] -> best [R], cls [R] (ties: the smallest index, as argmax)
__global__ void class_argmax_kernel(const float* __restrict__ scores, float* __restrict__ best, int* __restrict__ cls,
                                    int R, int C) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const float* p = scores + (size_t)r * C;
    float m = p[0];
    int k = 0;
    for (int c = 1; c < C; ++c) {
        const float v = p[c];
        if (v > m) { m = v; k = c; }
    }
    best[r] = m;
    cls[r] = k;
}
int y2_class_argmax(const float* scores, float* best, int* cls, int rows, int classes, void* stream) {
    if (!scores || !best || !cls || rows < 0 || classes < 1) return fail(Y2_ERR_ARG, "bad arguments");
    if (rows == 0) return Y2_OK;
    hipLaunchKernelGGL(class_argmax_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, scores, best, cls,
                       rows, classes);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

// x *= s (loss scaling of an output gradient in front of a half-precision backward pass)
__global__ void scale_kernel(float* __restrict__ x, size_t n, float s) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] *= s;
}
int y2_scale(float* x, size_t n, float s, void* stream) {
    if (!x) return fail(Y2_ERR_ARG, "null tensor");
    if (n == 0) return Y2_OK;
    size_t nb = (n + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, n, s);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

size_t y2_yolov2_loss_workspace_bytes(int batch) { return (size_t)batch * 4 * sizeof(float) + 256; }

int y2_yolov2_loss(const float* net, const float* labels, const float* anchors, int batch, int S, int B, int num_class,
                   float image_size, const float* scales, float* loss, float* dnet, void* workspace, void* stream) {
    if (!net || !labels || !anchors || !loss || !workspace) return fail(Y2_ERR_ARG, "null tensor");
    if (batch < 1 || S < 1 || S * S > kV2MaxTruth || B < 1 || num_class < 1) return fail(Y2_ERR_ARG, "bad loss geometry");
    V2LossArgs a{};
    a.net = net; a.labels = labels; a.anchors = anchors; a.dnet = dnet; a.partial = (float*)workspace;
    a.N = batch; a.S = S; a.B = B; a.C = num_class; a.image_size = image_size;
    a.coord = scales ? scales[0] : 1.0f; a.obj = scales ? scales[1] : 5.0f; a.noobj = scales ? scales[2] : 1.0f;
    a.cls = scales ? scales[3] : 1.0f; a.thresh = scales ? scales[4] : 0.6f;
    hipLaunchKernelGGL(yolov2_loss_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, a);
    EXTCHK(hipGetLastError());
    hipLaunchKernelGGL(yolov2_loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a.partial, loss, batch);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

static int v2_box_blocks(int S, int B) { return (S * S * B + 255) / 256; }

size_t y2_yolov2_loss_boxes_workspace_bytes(int batch, int S, int B) {
    if (batch < 1 || S < 1 || B < 1 || (long long)S * S * B > Y2_LOSS_BOXES_MAX_SLOTS) return 0;
    return (size_t)batch * v2_box_blocks(S, B) * 4 * sizeof(float) + 256;
}

int y2_yolov2_loss_boxes(const float* net, const float* truth, const int* ntruth, const float* anchors, int batch, int S,
                         int B, int num_class, int max_boxes, float image_size, const float* scales, float* loss,
                         float* dnet, void* workspace, void* stream) {
    if (!net || !truth || !ntruth || !anchors || !loss || !workspace)
        return fail(Y2_ERR_ARG, "y2_yolov2_loss_boxes: null pointer");
    if (batch < 1 || batch > 65535 || S < 1 || B < 1 || num_class < 1 || !(image_size > 0.0f))
        return fail(Y2_ERR_ARG, "y2_yolov2_loss_boxes: batch = %d, S = %d, B = %d, num_class = %d, image_size = %g", batch,
                    S, B, num_class, (double)image_size);
    if ((long long)S * S * B > Y2_LOSS_BOXES_MAX_SLOTS)
        return fail(Y2_ERR_ARG, "y2_yolov2_loss_boxes: S * S * B = %lld beyond Y2_LOSS_BOXES_MAX_SLOTS = %d",
                    (long long)S * S * B, Y2_LOSS_BOXES_MAX_SLOTS);
    if (max_boxes < 1 || max_boxes > Y2_MAX_BOXES)
        return fail(Y2_ERR_ARG, "y2_yolov2_loss_boxes: max_boxes = %d outside 1..%d", max_boxes, Y2_MAX_BOXES);
    V2BoxLossArgs a{};
    a.net = net; a.truth = truth; a.ntruth = ntruth; a.anchors = anchors; a.dnet = dnet; a.partial = (float*)workspace;
    a.N = batch; a.S = S; a.B = B; a.C = num_class; a.T = max_boxes; a.image_size = image_size;
    a.coord = scales ? scales[0] : 1.0f; a.obj = scales ? scales[1] : 5.0f; a.noobj = scales ? scales[2] : 1.0f;
    a.cls = scales ? scales[3] : 1.0f; a.thresh = scales ? scales[4] : 0.6f;
    a.area_weight = scales ? (scales[5] != 0.0f) : 0; a.prior = scales ? scales[6] : 0.0f;
    const int blocks = v2_box_blocks(S, B);
    hipLaunchKernelGGL(yolov2_loss_boxes_kernel, dim3(blocks, batch), dim3(256), 0, (hipStream_t)stream, a);
    EXTCHK(hipGetLastError());
    hipLaunchKernelGGL(yolov2_loss_boxes_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a.partial, loss,
                       blocks * batch, batch);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

size_t y2_yolov2_region_stats_workspace_bytes(int batch) {
    if (batch < 1 || batch > 65535) return 0;
    return (size_t)batch * 8 * sizeof(int) + 256;
}

int y2_yolov2_region_stats(const float* net, const float* truth, const int* ntruth, const float* anchors, int batch, int S,
                           int B, int num_class, int max_boxes, float image_size, float* stats, void* workspace,
                           void* stream) {
    if (!net || !truth || !ntruth || !anchors || !stats || !workspace)
        return fail(Y2_ERR_ARG, "y2_yolov2_region_stats: null pointer");
    if (batch < 1 || batch > 65535 || S < 1 || B < 1 || B > 8 || num_class < 1 || !(image_size > 0.0f))
        return fail(Y2_ERR_ARG, "y2_yolov2_region_stats: batch = %d, S = %d, B = %d (1..8), num_class = %d, image_size = %g",
                    batch, S, B, num_class, (double)image_size);
    if ((long long)S * S * B > Y2_LOSS_BOXES_MAX_SLOTS)
        return fail(Y2_ERR_ARG, "y2_yolov2_region_stats: S * S * B = %lld beyond Y2_LOSS_BOXES_MAX_SLOTS = %d",
                    (long long)S * S * B, Y2_LOSS_BOXES_MAX_SLOTS);
    if (max_boxes < 1 || max_boxes > Y2_MAX_BOXES)
        return fail(Y2_ERR_ARG, "y2_yolov2_region_stats: max_boxes = %d outside 1..%d", max_boxes, Y2_MAX_BOXES);
    V2RegionStatsArgs a{};
    a.net = net; a.truth = truth; a.ntruth = ntruth; a.anchors = anchors; a.partial = (int*)workspace;
    a.N = batch; a.S = S; a.B = B; a.C = num_class; a.T = max_boxes; a.image_size = image_size;
    hipLaunchKernelGGL(yolov2_region_stats_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, a);
    EXTCHK(hipGetLastError());
    hipLaunchKernelGGL(yolov2_region_stats_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a.partial, stats,
                       batch, (float)batch * (float)S * (float)S * (float)B);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Darknet's passthrough (specification: utils/darknet_reorg.py): out [N,Ho,Wo,4*C+Cc] = concat(Darknet's reorg of
// fine [N,H,W,C], coarse [N,Ho,Wo,Cc]), H = 2 Ho, W = 2 Wo -- the order of `route layers=-1,-4`.  Darknet's reorg is a
// scramble of each image's C*H*W values over channels and positions, not a space-to-depth, so the reorganised part is
// an element gather; ONE launch writes both parts.  The OUTPUT side is the coalesced one: a lane owns VEC consecutive
// output channels of one output pixel (VEC = 4: one 16-byte store; the coarse part is a 16-byte load too).  The four
// values of a reorganised slot are four 4-byte loads: output channels 4k .. 4k+3 come from four different input
// pixels, while the neighbouring lane (k + 1) reads 16 bytes further in the same four pixel rows -- a wave's load
// covers whole 256-byte rows of `fine` in 16-byte steps, and the steps in between belong to lanes of the same
// workgroup, so the rows are fetched once and re-read from the vector cache.  `fine` is a seventh of the bytes moved
// (N*H*W*C against the 4*C + Cc written and Cc read per output pixel), which is why no LDS tile is staged for it.
// ---------------------------------------------------------------------------
// the input element (offset into one image of fine [H][W][C]) of output channel co < 4 C at output pixel s = jo * Wo + io
Y2_DEV int darknet_reorg_source(int s, int co, int H, int W, int C) {
    const int HW = H * W;
    const int k = co >> 2;
    const int rem = s + (HW >> 2) * (co & 3);        // q = s + Ho Wo co, unravelled over [C][H][W]: (k, rem)
    const int j = rem / W, i = rem - j * W;
    const int out_c = C >> 2;
    const int off = k / out_c, c2 = k - off * out_c;
    const int m = (2 * i + (off & 1)) + 2 * W * (2 * j + (off >> 1));      // p = m + 4 H W c2, m < 4 H W
    const int t = m / HW, mm = m - t * HW;
    const int js = mm / W, is = mm - js * W;
    return (js * W + is) * C + 4 * c2 + t;
}

// The gradient of Darknet's passthrough (specification: utils/darknet_reorg.passthrough_concat_darknet_backward).  The
// reorg is a permutation of each image, so its gradient is the inverse permutation: dfine[darknet_reorg_source(s, co)] =
// dout[s][co], every element of dfine named exactly once.  ONE launch writes both outputs, every element exactly once,
// with no zero fill and no atomics.  This is the SCATTER form, the forward walk with loads and stores exchanged: a lane
// owns VEC consecutive channels of one dout pixel (VEC = 4: one 16-byte load), then makes one 16-byte store into dcoarse
// or four 4-byte stores into dfine -- the lane beside it (k + 1) writes 16 bytes further in the same four pixel rows, so a
// wave's stores fill whole 256-byte rows of dfine between them.  The gather form (a lane owns four channels of a dfine
// pixel, one 16-byte store, four 4-byte loads through the closed-form inverse of darknet_reorg_source) is the same
// function and measured 7 % slower at S = 13 and 19 (scripts/probes/darknet_route_backward_ab.hip holds both forms and
// the inverse with its derivation), so it is not in the library.  VEC = 1: Cc % 4 != 0 or a pointer off 16 bytes.
//
// Both directions are ONE walk over the concatenated tensor `cat` [N,Ho,Wo,4*C+Cc]: BACKWARD = false reads fine and
// coarse and writes cat (cat = out), BACKWARD = true reads cat (= dout) and writes fine (= dfine) and coarse (= dcoarse).
// The direction is a template argument, so each of the two kernels below holds its own loads and stores only.  first /
// stride: the grid-stride loop's start and step, (size_t)blockIdx.x * blockDim.x + threadIdx.x and (size_t)gridDim.x *
// blockDim.x -- read in the kernels, where the compiler knows the workgroup size to be uniform (read here, every
// instantiation gains 8 to 11 instructions that pick the size of a partial last workgroup).
template <int VEC, bool BACKWARD>
Y2_DEV void darknet_passthrough_walk(float* __restrict__ fine, float* __restrict__ coarse, float* __restrict__ cat, int N,
                                     int Ho, int Wo, int C, int Cc, size_t first, size_t stride) {
    const int H = 2 * Ho, W = 2 * Wo, ld = 4 * C + Cc;
    const int ldv = ld / VEC;
    const size_t image = (size_t)H * W * C;
    const size_t total = (size_t)N * Ho * Wo * ldv;
    for (size_t e = first; e < total; e += stride) {
        const int co = (int)(e % ldv) * VEC;
        const size_t pix = e / ldv;                  // n * Ho * Wo + s
        const int s = (int)(pix % ((size_t)Ho * Wo));
        const size_t n = pix / ((size_t)Ho * Wo);
        float* slot = cat + pix * ld + co;
        if (co >= 4 * C) {
            float* part = coarse + pix * Cc + (co - 4 * C);
            float* dst = BACKWARD ? part : slot;
            const float* src = BACKWARD ? slot : part;
            if (VEC == 4) *(f32x4*)dst = *(const f32x4*)src;
            else *dst = *src;
        } else {
            float* img = fine + n * image;
            if (VEC == 4) {
                f32x4 v;
                if (BACKWARD) v = *(const f32x4*)slot;
                for (int q = 0; q < 4; ++q) {
                    float* p = img + darknet_reorg_source(s, co + q, H, W, C);
                    if (BACKWARD) *p = v[q];
                    else v[q] = *p;
                }
                if (!BACKWARD) *(f32x4*)slot = v;
            } else {
                float* p = img + darknet_reorg_source(s, co, H, W, C);
                if (BACKWARD) *p = *slot;
                else *slot = *p;
            }
        }
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void passthrough_concat_darknet_kernel(const float* __restrict__ fine,
                                                                         const float* __restrict__ coarse,
                                                                         float* __restrict__ out, int N, int Ho, int Wo,
                                                                         int C, int Cc) {
    darknet_passthrough_walk<VEC, false>(const_cast<float*>(fine), const_cast<float*>(coarse), out, N, Ho, Wo, C, Cc,
                                         (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

template <int VEC>
__global__ __launch_bounds__(256) void darknet_route_backward_kernel(const float* __restrict__ dout,
                                                                     float* __restrict__ dfine,
                                                                     float* __restrict__ dcoarse, int N, int Ho, int Wo,
                                                                     int C, int Cc) {
    darknet_passthrough_walk<VEC, true>(dfine, dcoarse, const_cast<float*>(dout), N, Ho, Wo, C, Cc,
                                        (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// Darknet's network input from this repository's uint8 BGR batches: dst[p][c] = float(src[p][2 - c]) / 255.0f, a true
// division (bit-equal to numpy's float32 quotient).  VEC4: a lane converts four pixels, three dwords in, three 16-byte
// stores out; the entry point sends the pixels behind the last whole group of four to the scalar form.
template <bool VEC4>
__global__ __launch_bounds__(256) void u8_bgr_to_f32_rgb_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                                 size_t first, size_t count) {
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += (size_t)gridDim.x * blockDim.x) {
        if (VEC4) {
            const uint32_t* s = (const uint32_t*)src + g * 3;
            const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];      // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
            float* d = dst + g * 12;
            f32x4 a, b, c;
            a[0] = (float)((w0 >> 16) & 255u) / 255.0f; a[1] = (float)((w0 >> 8) & 255u) / 255.0f;
            a[2] = (float)(w0 & 255u) / 255.0f;         a[3] = (float)((w1 >> 8) & 255u) / 255.0f;
            b[0] = (float)(w1 & 255u) / 255.0f;         b[1] = (float)(w0 >> 24) / 255.0f;
            b[2] = (float)(w2 & 255u) / 255.0f;         b[3] = (float)(w1 >> 24) / 255.0f;
            c[0] = (float)((w1 >> 16) & 255u) / 255.0f; c[1] = (float)(w2 >> 24) / 255.0f;
            c[2] = (float)((w2 >> 16) & 255u) / 255.0f; c[3] = (float)((w2 >> 8) & 255u) / 255.0f;
            *(f32x4*)(d + 0) = a; *(f32x4*)(d + 4) = b; *(f32x4*)(d + 8) = c;
        } else {
            const size_t p = first + g;
            dst[p * 3 + 0] = (float)src[p * 3 + 2] / 255.0f;
            dst[p * 3 + 1] = (float)src[p * 3 + 1] / 255.0f;
            dst[p * 3 + 2] = (float)src[p * 3 + 0] / 255.0f;
        }
    }
}

// The one launcher of the two Darknet passthrough entry points (`what`: the entry point's name, for its messages).  a, b, c
// are the kernel's three tensors in its own order; wide_a and wide_b the two that move 16 bytes at a time: the coarse part
// and the concatenated tensor.  The bounds: the index arithmetic of one image of the fine map is 32-bit -- 16 H W Cf
// values, (4 Cf + Cc) channels.
template <typename A, typename B, typename C>
static int darknet_passthrough_launch(const char* what, void (*vec4)(A*, B*, C*, int, int, int, int, int),
                                      void (*vec1)(A*, B*, C*, int, int, int, int, int), A* a, B* b, C* c,
                                      const float* wide_a, const float* wide_b, int N, int H, int W, int Cf, int Cc,
                                      void* stream) {
    if (!a || !b || !c) return fail(Y2_ERR_ARG, "%s: null tensor", what);
    if (N < 1 || H < 1 || W < 1 || Cf < 1 || Cc < 1)
        return fail(Y2_ERR_ARG, "%s: N = %d, H = %d, W = %d, Cf = %d, Cc = %d must be positive", what, N, H, W, Cf, Cc);
    if (Cf % 4) return fail(Y2_ERR_ARG, "%s: Cf = %d is no multiple of 4 (Darknet's reorg reads the fine map as "
                            "[Cf / 4][4 H][4 W])", what, Cf);
    if ((long long)16 * H * W * Cf > 0x7fffffffLL || (long long)4 * Cf + Cc > 0x7fffffffLL)
        return fail(Y2_ERR_ARG, "%s: an image of %d x %d x %d is beyond 32-bit indices", what, 2 * H, 2 * W, Cf);
    const bool vec = (Cc % 4) == 0 && ((uintptr_t)wide_a % 16) == 0 && ((uintptr_t)wide_b % 16) == 0;
    const size_t total = (size_t)N * H * W * ((size_t)(4 * Cf + Cc) / (vec ? 4 : 1));
    size_t nb = (total + 255) / 256;
    if (nb > 65536) nb = 65536;
    hipLaunchKernelGGL(vec ? vec4 : vec1, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, a, b, c, N, H, W, Cf, Cc);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

// Darknet's `[maxpool] size=2 stride=1` (maxpool_layer.c with padding = size - 1 = 1, offset -padding / 2 = 0) on fp32
// NHWC; specification: utils/darknet_maxpool.py.  Output (i, j) is the maximum over input (i + dy, j + dx), dy, dx in
// {0, 1}, of the taps inside the map: the window is anchored top-left and clipped at the bottom and right edges.  The
// running maximum starts at -FLT_MAX and is replaced on a strict >, taps in the order (0,0), (0,1), (1,0), (1,1): the
// first maximum wins a tie (-0.0 does not displace +0.0 nor the reverse) and a NaN is never chosen.  A window of NaNs
// alone keeps -FLT_MAX and has no arg-max, so it routes no gradient -- where Darknet would index out of bounds.
//
// Both kernels walk the tensor's channel groups with one grid-stride loop: a lane owns VEC consecutive channels of one
// pixel and consecutive lanes hold consecutive channel groups, so a wave reads and writes whole stretches of a row of C
// floats.  VEC = 4: 16-byte loads and stores; VEC = 1: C % 4 != 0 or a pointer off 16 bytes.  Every index fits 31 bits
// (the entry points check), so the index arithmetic is 32-bit.  No LDS, no scratch.
template <int VEC>
Y2_DEV void s1_load(float (&v)[VEC], const float* __restrict__ p) {
    if (VEC == 4) { const f32x4 w = *(const f32x4*)p; for (int q = 0; q < 4; ++q) v[q] = w[q]; }
    else v[0] = *p;
}

template <int VEC>
Y2_DEV void s1_store(float* __restrict__ p, const float (&v)[VEC]) {
    if (VEC == 4) { f32x4 w; for (int q = 0; q < 4; ++q) w[q] = v[q]; *(f32x4*)p = w; }
    else *p = v[0];
}

// forward: a lane owns VEC consecutive channels of one OUTPUT pixel: up to four loads, one store
template <int VEC>
__global__ __launch_bounds__(256) void maxpool2x2s1_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H,
                                                           int W, int C) {
    const uint32_t cv = C / VEC, total = (uint32_t)N * H * W * cv;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t pix = e / cv;                 // (n * H + i) * W + j; e * VEC = pix * C + c
        const int j = (int)(pix % W), i = (int)((pix / W) % H);
        const bool right = j + 1 < W, below = i + 1 < H;
        const float* p = x + (size_t)e * VEC;        // tap (0,0)
        float best[VEC], v[VEC];
        for (int q = 0; q < VEC; ++q) best[q] = -FLT_MAX;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (((t & 1) && !right) || ((t >> 1) && !below)) continue;
            s1_load<VEC>(v, p + ((t >> 1) * W + (t & 1)) * C);
            for (int q = 0; q < VEC; ++q)
                if (v[q] > best[q]) best[q] = v[q];
        }
        s1_store<VEC>(y + (size_t)e * VEC, best);
    }
}

// backward, the GATHER form: a lane owns VEC channels of one INPUT pixel (i, j), decides which of the up to four windows
// that hold it -- anchors (i-1,j-1), (i-1,j), (i,j-1), (i,j), in which it is tap 3, 2, 1, 0 -- it won, and adds the dy
// of those in that (ascending row-major) order, starting from +0.0f; then ONE store of dx.  No atomics, no zero fill,
// every dx element written exactly once, the same bits every run.
//
// The four windows lie in the 3 x 3 neighbourhood of the pixel, which the lane loads once (nine loads where the
// forward rule, window by window, asks sixteen times); a position outside the map holds NaN, which loses every
// comparison below just as a clipped tap takes no part.  The pixel's value m wins a window under the running-maximum
// rule exactly when
//     m > -FLT_MAX,   no EARLIER tap u has u >= m   and   no LATER tap u has u > m:
// an earlier tap with u >= m leaves a running maximum that m does not exceed, and otherwise the running maximum in front
// of m is below it (or still -FLT_MAX); m then stays unless a later tap exceeds it.  A NaN m fails the first test, a NaN
// u fails both of its tests, as in the running rule.
template <int VEC>
__global__ __launch_bounds__(256) void maxpool2x2s1_backward_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                    float* __restrict__ dx, int N, int H, int W, int C) {
    const uint32_t cv = C / VEC, total = (uint32_t)N * H * W * cv;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t pix = e / cv;
        const int j = (int)(pix % W), i = (int)((pix / W) % H);
        const bool rows_in[3] = {i > 0, true, i + 1 < H}, cols_in[3] = {j > 0, true, j + 1 < W};
        const size_t at = (size_t)e * VEC;           // this pixel's channels
        float v[3][3][VEC];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                if (rows_in[r] && cols_in[s]) s1_load<VEC>(v[r][s], x + at + ((r - 1) * W + (s - 1)) * C);
                else for (int q = 0; q < VEC; ++q) v[r][s][q] = __builtin_nanf("");
            }
        float acc[VEC], g[VEC];
        for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {                // the anchor (i - 1 + ar, j - 1 + as); this pixel is its tap 3 - a
            const int ar = a >> 1, as = a & 1;
            if (!rows_in[ar] || !cols_in[as]) continue;
            s1_load<VEC>(g, dy + at + ((ar - 1) * W + (as - 1)) * C);
            for (int q = 0; q < VEC; ++q) {
                const float m = v[1][1][q];
                bool wins = m > -FLT_MAX;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (t == 3 - a) continue;
                    const float u = v[ar + (t >> 1)][as + (t & 1)][q];
                    wins = wins && (t < 3 - a ? !(u >= m) : !(u > m));
                }
                if (wins) acc[q] += g[q];
            }
        }
        s1_store<VEC>(dx + at, acc);
    }
}

// the checks and the grid the two stride-1 pool entry points share (`what`: the entry point's name, for its messages)
static int maxpool2x2s1_check(const char* what, bool null, int N, int H, int W, int C) {
    if (null) return fail(Y2_ERR_ARG, "%s: null tensor", what);
    if (N < 1 || H < 1 || W < 1 || C < 1)
        return fail(Y2_ERR_ARG, "%s: N = %d, H = %d, W = %d, C = %d must be positive", what, N, H, W, C);
    const long long rows = (long long)N * H;         // below 2^62; the next factors go in only while the count fits 31 bits
    if (rows > 0x7fffffffLL || rows * W > 0x7fffffffLL || rows * W * C > 0x7fffffffLL)
        return fail(Y2_ERR_ARG, "%s: %d x %d x %d x %d elements are beyond 32-bit indices", what, N, H, W, C);
    return Y2_OK;
}

static unsigned maxpool2x2s1_blocks(int N, int H, int W, int C, bool vec) {
    const size_t total = (size_t)N * H * W * (size_t)(C / (vec ? 4 : 1));
    const size_t nb = (total + 255) / 256;
    return (unsigned)(nb > 65536 ? 65536 : nb);
}

extern "C" {

int y2_maxpool2x2s1(const float* x, float* y, int N, int H, int W, int C, void* stream) {
    const int rc = maxpool2x2s1_check("y2_maxpool2x2s1", !x || !y, N, H, W, C);
    if (rc) return rc;
    const bool vec = (C % 4) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0;
    hipLaunchKernelGGL(vec ? maxpool2x2s1_kernel<4> : maxpool2x2s1_kernel<1>, dim3(maxpool2x2s1_blocks(N, H, W, C, vec)),
                       dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, C);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

int y2_maxpool2x2s1_backward(const float* x, const float* dy, float* dx, int N, int H, int W, int C, void* stream) {
    const int rc = maxpool2x2s1_check("y2_maxpool2x2s1_backward", !x || !dy || !dx, N, H, W, C);
    if (rc) return rc;
    const bool vec = (C % 4) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)dy % 16) == 0 && ((uintptr_t)dx % 16) == 0;
    hipLaunchKernelGGL(vec ? maxpool2x2s1_backward_kernel<4> : maxpool2x2s1_backward_kernel<1>,
                       dim3(maxpool2x2s1_blocks(N, H, W, C, vec)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, N, H, W, C);
    EXTCHK(hipGetLastError());
    return Y2_OK;
}

int y2_passthrough_concat_darknet(const float* fine, const float* coarse, float* out, int N, int H, int W, int Cf, int Cc,
                                  void* stream) {
    return darknet_passthrough_launch("y2_passthrough_concat_darknet", passthrough_concat_darknet_kernel<4>,
                                      passthrough_concat_darknet_kernel<1>, fine, coarse, out, coarse, out, N, H, W, Cf, Cc,
                                      stream);
}

int y2_passthrough_concat_darknet_backward(const float* dout, float* dfine, float* dcoarse, int N, int H, int W, int Cf,
                                           int Cc, void* stream) {
    return darknet_passthrough_launch("y2_passthrough_concat_darknet_backward", darknet_route_backward_kernel<4>,
                                      darknet_route_backward_kernel<1>, dout, dfine, dcoarse, dout, dcoarse, N, H, W, Cf, Cc,
                                      stream);
}

int y2_zero(float* x, size_t n, void* stream) {
    if (!x) return fail(Y2_ERR_ARG, "y2_zero: null tensor");
    if (n == 0) return Y2_OK;
    EXTCHK(hipMemsetAsync(x, 0, n * sizeof(float), (hipStream_t)stream));
    return Y2_OK;
}

int y2_u8_bgr_to_f32_rgb(const uint8_t* src, float* dst, size_t n_pixels, void* stream) {
    if (!src || !dst) return fail(Y2_ERR_ARG, "y2_u8_bgr_to_f32_rgb: null tensor");
    if (n_pixels < 1) return fail(Y2_ERR_ARG, "y2_u8_bgr_to_f32_rgb: no pixels");
    const bool vec = ((uintptr_t)src % 4) == 0 && ((uintptr_t)dst % 16) == 0;
    const size_t groups = vec ? n_pixels / 4 : 0, rest = n_pixels - groups * 4;
    if (groups) {
        size_t nb = (groups + 255) / 256;
        if (nb > 65536) nb = 65536;
        hipLaunchKernelGGL(u8_bgr_to_f32_rgb_kernel<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, src, dst,
                           (size_t)0, groups);
        EXTCHK(hipGetLastError());
    }
    if (rest) {
        size_t nb = (rest + 255) / 256;
        if (nb > 65536) nb = 65536;
        hipLaunchKernelGGL(u8_bgr_to_f32_rgb_kernel<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, src, dst,
                           groups * 4, rest);
        EXTCHK(hipGetLastError());
    }
    return Y2_OK;
}

}  // extern "C"
