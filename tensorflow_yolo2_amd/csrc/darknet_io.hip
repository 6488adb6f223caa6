// Darknet's test-time protocol on the device ("Darknet's test-time protocol"): the float letterbox of its
// `letterbox_image` straight from the uint8 pool to the network's RGB input in [0, 1], and the boxes as its `valid`
// forms them -- the float un-map of `correct_region_boxes`, a float centre-box IoU in the NMS, float corners in the rows
// -- with the matching of those float rows.  The specification is this repository's host code
// (img_dataset/pascal_voc.letterbox_darknet; utils/detect_batch: darknet_unmap, box_iou_darknet,
// anchor_detect_classes_darknet, match_image_f) and every kernel is bit-equal to it: float32 in the specification's
// operation order, double where it says double, and the file is compiled with -ffp-contract=off.
#include "data_common.h"
#include "kernels.h"
#include "anchor_decode.h"
#include "letterbox.h"
#include "detect_common.h"
#include "darknet_box.h"
using namespace y2;

namespace {

// ---- the image: y2_letterbox_darknet_batch ------------------------------------------------------------------------
constexpr int kDkBand = 8;                      // canvas rows of one workgroup
constexpr int kDkPix = 4;                       // consecutive canvas pixels of one lane: twelve floats, three 16-byte stores

// Darknet's pixel: channel k of RGB from the pool's BGR bytes, float(b) / 255.0f.  The quotient is formed without the
// division's expansion (scale, reciprocal, refinement, fix-up: the kernel's time went there, profiles/darknet_protocol.txt):
// q0 = b * r with r = float(1 / 255.), then one correction by the remainder, which the fused multiply-add forms exactly.
// For all 256 bytes the result is the correctly rounded quotient, bit for bit what u8_bgr_to_f32_rgb_kernel's division
// gives (tests/test_darknet_protocol_host.py proves the identity in exact rational arithmetic).  These two fmaf are
// explicit, not contractions: the file is still built with -ffp-contract=off.
Y2_DEV float dk_src(const uint8_t* row, int xbyte, int k) {
    const float b = (float)row[xbyte + 2 - k];
    const float r = 1.0f / 255.0f;              // a constant: 0x3b808081
    const float q0 = b * r;
    return fmaf(fmaf(-255.0f, q0, b), r, q0);
}

// the horizontal pass at one source row: part = (1 - dx) * src(ix) + dx * src(ix + 1), two products and one sum.  The
// copied last column (and a source one pixel wide) arrives here as ix = ix + 1 = W - 1 with dx = 0, which is that pixel
// exactly: 1 * a + 0 * a = a for every finite a >= 0.
Y2_DEV float dk_part(const uint8_t* row, int xa, int xb, float dx, int k) {
    return (1.0f - dx) * dk_src(row, xa, k) + dx * dk_src(row, xb, k);
}

// grid (ceil(size / kDkBand), n), size / 4 lanes rounded up to whole waves (size is a multiple of 32 up to 1024, so a
// canvas row is whole groups of four pixels and at most 256 of them).  Lane t owns canvas columns 4 t .. 4 t + 3 of the
// band's rows: its x coefficients (byte offsets of the two source columns, dx) are formed once, the y coefficients are
// uniform per row, and both passes are recomputed per output value from byte loads of the pool -- `part` is a pure
// function of its indices, so no intermediate image exists and the bits are the specification's.  Rows and columns of
// the bars are 0.5; a band that lies wholly in a bar (or whose table row is empty) returns before any coefficient.  The
// + 1 neighbours are clamped to the last row / column (their weight is zero there), and so are ix and iy themselves: no
// read leaves the image.  No LDS, no barrier.  The flip column is not read.
__global__ __launch_bounds__(256) void letterbox_darknet_kernel(const uint8_t* __restrict__ pool,
                                                                const int64_t* __restrict__ table,
                                                                const int32_t* __restrict__ index, int size,
                                                                float* __restrict__ out) {
    const int tid = threadIdx.x, img = blockIdx.y;
    if (tid >= size / kDkPix) return;
    const int64_t* t = table + (size_t)kTable * (index ? index[img] : img);
    const int64_t off = t[0], h64 = t[1], w64 = t[2], pitch64 = t[3];
    const int band0 = blockIdx.x * kDkBand, nrows = min(kDkBand, size - band0);
    const int rowvec = 3 * (size / kDkPix);     // 16-byte words of a canvas row
    f32x4* obase = (f32x4*)(out + ((size_t)img * size + band0) * size * 3) + 3 * tid;
    const f32x4 bar = {0.5f, 0.5f, 0.5f, 0.5f};
    const bool sized = h64 >= 1 && w64 >= 1 && h64 <= 0x7fffffff && w64 <= 0x7fffffff;
    const int H = sized ? (int)h64 : 1, W = sized ? (int)w64 : 1;
    const LetterboxGeom g = letterbox_geometry(W, H, size);
    // the picture's rows of this band, relative to band0: [p0, p1)
    const int p0 = sized ? min(max(g.oy - band0, 0), nrows) : nrows;
    const int p1 = sized ? min(max(g.oy + g.new_h - band0, p0), nrows) : nrows;
    for (int j = 0; j < nrows; ++j) {
        if (j >= p0 && j < p1) continue;
        f32x4* o = obase + j * rowvec;
        o[0] = bar; o[1] = bar; o[2] = bar;
    }
    if (p0 >= p1) return;                       // uniform: a pure fill
    const float w_scale = g.new_w > 1 ? (float)(W - 1) / (float)(g.new_w - 1) : 0.0f;
    const float h_scale = g.new_h > 1 ? (float)(H - 1) / (float)(g.new_h - 1) : 0.0f;
    int xa[kDkPix], xb[kDkPix];
    float dx[kDkPix];
    bool in[kDkPix];
#pragma unroll
    for (int e = 0; e < kDkPix; ++e) {
        const int c = kDkPix * tid + e - g.ox;
        in[e] = c >= 0 && c < g.new_w;
        int ix = W - 1;
        dx[e] = 0.0f;
        if (in[e] && c != g.new_w - 1 && W != 1) {
            const float sx = (float)c * w_scale;
            ix = (int)sx;
            dx[e] = sx - (float)ix;
        }
        xa[e] = 3 * min(ix, W - 1);
        xb[e] = 3 * min(ix + 1, W - 1);
    }
    const uint8_t* src = pool + off;
    for (int j = p0; j < p1; ++j) {
        const int r = band0 + j - g.oy;         // the picture's row: uniform
        const float sy = (float)r * h_scale;
        const int iy = (int)sy;
        const float dy = sy - (float)iy;
        const bool second = !(r == g.new_h - 1 || H == 1);   // Darknet's last row never receives the second term
        const uint8_t* r0 = src + (size_t)min(iy, H - 1) * pitch64;
        const uint8_t* r1 = src + (size_t)min(iy + 1, H - 1) * pitch64;
        float v[3 * kDkPix];
#pragma unroll
        for (int e = 0; e < kDkPix; ++e)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float val = 0.5f;
                if (in[e]) {
                    val = (1.0f - dy) * dk_part(r0, xa[e], xb[e], dx[e], k);
                    if (second) val = val + dy * dk_part(r1, xa[e], xb[e], dx[e], k);
                }
                v[3 * e + k] = val;
            }
        f32x4* o = obase + j * rowvec;
        o[0] = f32x4{v[0], v[1], v[2], v[3]};
        o[1] = f32x4{v[4], v[5], v[6], v[7]};
        o[2] = f32x4{v[8], v[9], v[10], v[11]};
    }
}

// ---- the boxes: y2_detect_anchor_classes_batch_dk -------------------------------------------------------------------
constexpr int kClassLanes = 512;                       // the workgroup, as detect_anchor_classes_kernel's
constexpr int kClassSlotBytes = 8 + 4 * 4 + 1;         // sort word, the float centre box, suppressed flag: 50 KB at 2048

// grid (C, n): detect_anchor_classes_kernel's workgroup per (class, image), objectness shortcut, ballot compaction and
// bitonic sort over the next power of two of the valid candidates (detect.hip).  What differs is the box: a valid
// candidate (score > score_thresh, the four un-mapped values finite; nothing else) keeps its float centre box
// (bx, by, bw, bh) in pixels of the original image at its own index, the walk suppresses with Darknet's float IoU on
// those, and a kept row's words 0..3 are the bit patterns of the float corners, the minima raised to 1 and the maxima
// lowered to the image size.  A box that is empty after that cut is kept, as Darknet keeps it.
__global__ __launch_bounds__(kClassLanes) void detect_anchor_classes_dk_kernel(
    const float* __restrict__ net, const float* __restrict__ anchors, const int64_t* __restrict__ table,
    const int32_t* __restrict__ index, int S, int B, int C, float score_thresh, float iou_thresh, int max_out, int KP,
    int net_size, int* __restrict__ det, float* __restrict__ score, int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // kClassSlotBytes per slot
    uint64_t* sword = (uint64_t*)smem;
    float* fx = (float*)(sword + KP);
    float *fy = fx + KP, *fw = fy + KP, *fh = fw + KP;
    unsigned char* sup = (unsigned char*)(fh + KP);
    __shared__ int s_valid;
    const int cls = blockIdx.x, img = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & (kWave - 1);
    const int K = S * S * B, D = 5 + C;
    const int64_t* t = table + (size_t)kTable * (index ? index[img] : img);
    const int64_t h64 = t[1], w64 = t[2];
    const bool sized = h64 >= 1 && w64 >= 1 && h64 <= 0x7fffffff && w64 <= 0x7fffffff;
    const int im_h = sized ? (int)h64 : 1, im_w = sized ? (int)w64 : 1;
    const float* rows = net + (size_t)img * K * D;
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
            if (bx.so > score_thresh) {                           // score <= so in float32: detect_anchor_classes_kernel
                float mx, sum;
                anchor_softmax_norm(p, C, mx, sum);
                v = anchor_class_score(p, cls, bx.so, mx, sum);
            }
            if (v > score_thresh) {                               // the two double divisions only where the score passes
                float x = (float)(((double)bx.cx - m.offx) / m.scx), y = (float)(((double)bx.cy - m.offy) / m.scy);
                float w = bx.w * m.rw, h = bx.h * m.rh;
                x = x * m.fw; w = w * m.fw; y = y * m.fh; h = h * m.fh;
                valid = isfinite(x) && isfinite(y) && isfinite(w) && isfinite(h);
                if (valid) {
                    fx[i] = x; fy[i] = y; fw[i] = w; fh[i] = h;
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
    const size_t seg = (size_t)img * C + cls;
    int* drow = det + seg * max_out * 6;
    float* srow = score + seg * max_out;
    int kept = 0;
    for (int i = 0; i < nvalid && kept < max_out; ++i) {
        if (sup[i]) continue;
        const uint64_t wd = sword[i];
        const int o = word_index(wd);
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
            d[4] = cls; d[5] = o;
            srow[kept] = word_key(wd);
        }
        for (int j = i + 1 + tid; j < nvalid; j += nt) {
            if (sup[j]) continue;
            const int q = word_index(sword[j]);
            if (iou_darknet(ax, ay, aw, ah, fx[q], fy[q], fw[q], fh[q]) > iou_thresh) sup[j] = 1;
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

int y2_letterbox_darknet_batch(const uint8_t* pool, const int64_t* table, const int32_t* index, int n, int size,
                               float* out, void* stream) {
    if (!pool || !table || !out) return fail(Y2_ERR_ARG, "y2_letterbox_darknet_batch: null pointer");
    if (n < 1 || n > 65535) return fail(Y2_ERR_ARG, "y2_letterbox_darknet_batch: n = %d outside 1..65535", n);
    if (size < 32 || size % 32 || size > kMaxOutW)
        return fail(Y2_ERR_ARG, "y2_letterbox_darknet_batch: size = %d is not a multiple of 32 in 32..Y2_RESIZE_MAX_OUT_W = %d",
                    size, kMaxOutW);
    if ((uintptr_t)out & 15) return fail(Y2_ERR_ARG, "y2_letterbox_darknet_batch: out is not 16-byte aligned");
    const int lanes = (size / kDkPix + kWave - 1) / kWave * kWave;   // <= 256
    hipLaunchKernelGGL(letterbox_darknet_kernel, dim3((size + kDkBand - 1) / kDkBand, n), dim3(lanes), 0,
                       (hipStream_t)stream, pool, table, index, size, out);
    return launched("y2_letterbox_darknet_batch");
}

int y2_detect_anchor_classes_batch_dk(const float* net, const float* anchors, const int64_t* table, const int32_t* index,
                                      int n, int S, int B, int num_class, float score_thresh, float iou_thresh,
                                      int max_per_class, int net_size, int* det, float* score, int* count,
                                      void* stream) {
    const char* name = "y2_detect_anchor_classes_batch_dk";
    int KP;
    if (const int rc = detect_anchor_args(name, net && anchors && table && det && score && count, n, 65535,
                                          "max_per_class", max_per_class, S, B, num_class, true, net_size, &KP))
        return rc;
    const int lanes = KP < kClassLanes ? KP : kClassLanes;
    hipLaunchKernelGGL(detect_anchor_classes_dk_kernel, dim3(num_class, n), dim3(lanes), (size_t)KP * kClassSlotBytes,
                       (hipStream_t)stream, net, anchors, table, index, S, B, num_class, score_thresh, iou_thresh,
                       max_per_class, KP, net_size, det, score, count);
    return launched(name);
}

int y2_voc_match_batch_f(const int* det, const float* score, const int* count, const double* boxes,
                         const int32_t* counts, const uint8_t* difficult, const int32_t* index, int n, int max_obj,
                         int max_out, float iou_thresh, int* flags, void* stream) {
    (void)score;
    return voc_match_any<true>("y2_voc_match_batch_f", det, count, boxes, counts, difficult, index, n, max_obj, max_out,
                               iou_thresh, flags, stream);
}

}  // extern "C"
