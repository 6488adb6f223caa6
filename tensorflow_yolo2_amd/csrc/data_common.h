// What the bit-equal input paths share (data.hip: plain resize, letterbox, label grid; augment.hip: window + colour,
// classifier warp, box list): the launch geometry, the x-coefficient record and table, the coefficient arithmetic, the
// fixed-point blend, the staging of whole source rows in LDS, the three-dword store, the window arithmetic of the boxes
// with the label-grid kernel body, and the tail of an entry point.  One definition of each, so that the identity window
// cannot drift from the plain resize, nor one label format from another.  What differs between kernels stays with the
// kernel.
#pragma once
#include <stdio.h>
#include <stdarg.h>
#include "common.h"
#include "../../include/yolo2_hip.h"

namespace y2 {
int set_error(int code, const char* msg);   // net.hip (y2_last_error)
}
static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return y2::set_error(code, buf);
}
// the tail of an entry point `who` after its launch
static int launched(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(Y2_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return Y2_OK;
}

namespace {

constexpr int kThreads = 256;
constexpr int kMaxOutW = Y2_RESIZE_MAX_OUT_W;   // columns of the x-coefficient table in LDS
constexpr int kBand = 16;                       // output rows of one workgroup
constexpr int kRows = 4;                        // output rows produced from one staging of source rows
constexpr int kMaxPitch = 4096;                 // widest source row (bytes) that is staged in LDS; wider rows are read in place
constexpr int kTable = 5;                       // int64 per image: byte offset, height, width, row pitch, flip
constexpr int kParams = 8;                      // double per batch slot with a window: x0, y0, cw, ch, flip, hue, sat, exp

struct XCoef { int x0; short dx; short w1; };   // byte offset of the left pixel, byte distance to the right one, weight

// one axis of cv2.resize INTER_LINEAR on uint8: output index o of n_out -> clamped source indices and the 11-bit
// weight of the second one.  float64, the specification's operation order.
Y2_DEV void lin_coef(int o, int n_in, int n_out, int& i0c, int& i1c, int& w1) {
    const double scale = (double)n_in / (double)n_out;
    const double f = ((double)o + 0.5) * scale - 0.5;
    const double fl = floor(f);
    const int i0 = (int)fl;
    const double frac = i0 < 0 ? 0.0 : f - fl;
    w1 = (int)rint(frac * 2048.0);
    i0c = min(max(i0, 0), n_in - 1);
    i1c = min(max(i0 + 1, 0), n_in - 1);
}

// the x table of W source columns resized to n_out output columns (mirrored: `flip`), by the whole workgroup
Y2_DEV void build_xtable(XCoef* xt, int W, int n_out, int flip, int tid) {
    for (int x = tid; x < n_out; x += kThreads) {
        int x0, x1, w1;
        lin_coef(flip ? n_out - 1 - x : x, W, n_out, x0, x1, w1);
        xt[x] = XCoef{3 * x0, (short)(3 * (x1 - x0)), (short)w1};
    }
}

// the four taps of one output byte blended with the 11-bit weights of the right column and the lower row
Y2_DEV int blend4(int v00, int v01, int v10, int v11, int wx1, int wy1) {
    const int wx0 = 2048 - wx1, wy0 = 2048 - wy1;
    const int top = v00 * wx0 + v01 * wx1;
    const int bot = v10 * wx0 + v11 * wx1;
    return (top * wy0 + bot * wy1 + (1 << 21)) >> 22;   // <= 255 * 2^22 + 2^21 < 2^31
}

// four pixels b | g << 8 | r << 16 as 12 bytes at a multiple of 12 of a 4-byte aligned batch
Y2_DEV void store_px4(uint32_t* o32, const uint32_t pix[4]) {
    o32[0] = pix[0] | pix[1] << 24;
    o32[1] = pix[1] >> 8 | pix[2] << 16;
    o32[2] = pix[2] >> 16 | pix[3] << 8;
}

// rows of `pitch` bytes that start at byte `off` of the pool can be copied with 16-byte loads of whole rows of W pixels;
// beside it every kernel tests its own LDS budget
Y2_DEV bool stageable(int64_t off, int64_t pitch, int W) { return ((off | pitch) & 15) == 0 && pitch >= 3 * (int64_t)W; }

// the 2 * gr source rows of gr output rows into LDS slots of `pitch` bytes, with 16-byte loads: slot 2j + s is row
// yc[j][s] of the image.  (The plain resize and the letterbox; the augment kernel's loop stages a row outside the image
// as fill, and stays with it: taken from here with a flag it compiled to other scalar code and measured 0.1 % slower.)
Y2_DEV void stage_rows(uint8_t* rows, const uint8_t* src, int64_t pitch64, const int (*yc)[3], int gr, int tid) {
    const int pitch = (int)pitch64, chunks = pitch >> 4;
    for (int i = tid; i < 2 * gr * chunks; i += kThreads) {
        const int slot = i / chunks, c = i - slot * chunks;
        const int y = yc[slot >> 1][slot & 1];
        *(y2::u32x4*)(rows + slot * pitch + 16 * c) = *(const y2::u32x4*)(src + (size_t)y * pitch64 + 16 * c);
    }
}

// a window coordinate of the parameter row as an integer of [lo, hi] (not a number -> lo)
Y2_DEV int win_int(double v, int lo, int hi) { return (int)fmin(fmax(v, (double)lo), (double)hi); }

// the window of a parameter row as the image kernel reads it -- integers, a fraction is cut off in both -- and the
// mirror: the entry's flip XOR the row's
Y2_DEV bool read_window(const double* prm, bool entry_flip, double& wx0, double& wy0, double& cw, double& ch) {
    wx0 = win_int(prm[0], -(1 << 30), 1 << 30); wy0 = win_int(prm[1], -(1 << 30), 1 << 30);
    cw = win_int(prm[2], 0, 1 << 30); ch = win_int(prm[3], 0, 1 << 30);
    return entry_flip != (prm[4] != 0.0);
}

// an object's box in pixels of the input: clamped corners, and whether the UNCLAMPED centre lies in [0, size)
struct WindowBox {
    bool keep;
    double x1, y1, x2, y2;
    Y2_DEV double cx() const { return (x2 + x1) / 2.0; }
    Y2_DEV double cy() const { return (y2 + y1) / 2.0; }
    Y2_DEV double w() const { return x2 - x1; }
    Y2_DEV double h() const { return y2 - y1; }
};

Y2_DEV double clamp_px(double v, double hi) { v = hi < v ? hi : v; return 0.0 > v ? 0.0 : v; }

// box bx = xmin, ymin, xmax, ymax (1-based source pixels) through the window: x = (bx - 1 - wx0) * w_ratio, y likewise,
// in double in the specification's order (augment.py: _window_boxes); hi = size - 1.  keep is false for not a number.
Y2_DEV WindowBox window_box(const double* bx, double wx0, double wy0, double w_ratio, double h_ratio, double hi,
                            double size) {
    const double x1 = (bx[0] - 1 - wx0) * w_ratio, y1 = (bx[1] - 1 - wy0) * h_ratio;
    const double x2 = (bx[2] - 1 - wx0) * w_ratio, y2 = (bx[3] - 1 - wy0) * h_ratio;
    const double ux = (x2 + x1) / 2.0, uy = (y2 + y1) / 2.0;
    return WindowBox{ux >= 0.0 && ux < size && uy >= 0.0 && uy < size, clamp_px(x1, hi), clamp_px(y1, hi),
                     clamp_px(x2, hi), clamp_px(y2, hi)};
}

// The body of the two label-grid kernels, grid (n).  The workgroup zero-fills the image's grid; then ONE lane walks the
// image's objects in annotation order (the first object of a cell wins, which is sequential).  double arithmetic in the
// specification's order, one cast to float at each store.  A flipped image writes the mirrored column and
// image_size - 1 - x directly: the mirror is a bijection of the cells, so "first wins" picks the same objects as flipping
// the finished grid.  WINDOW: the boxes follow the window of the slot's parameter row, and an object whose unclamped centre
// leaves it is dropped.  Else the window is the image of the table row (x - 1 - 0.0 is x - 1 bit for bit, both zeros
// included) and every object is clamped and kept: pascal_voc.encode_boxes.
template <bool WINDOW>
Y2_DEV void encode_labels(const double* __restrict__ boxes, const int32_t* __restrict__ counts,
                          const int64_t* __restrict__ table, const int32_t* __restrict__ index,
                          const double* __restrict__ params, int max_obj, int image_size, int S, int num_class,
                          float* __restrict__ labels) {
    const int img = blockIdx.x, D = 5 + num_class;
    const size_t e = index ? (size_t)index[img] : (size_t)img;
    float* g = labels + (size_t)img * S * S * D;
    for (int i = threadIdx.x; i < S * S * D; i += kThreads) g[i] = 0.0f;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int64_t* t = table + kTable * e;
    double wx0 = 0.0, wy0 = 0.0, cw = (double)(int)t[2], ch = (double)(int)t[1];
    bool flip = (int)t[4] != 0;
    if (WINDOW) {
        flip = read_window(params + (size_t)kParams * img, t[4] != 0, wx0, wy0, cw, ch);
        if (!(cw >= 1.0 && ch >= 1.0)) return;
    }
    const double w_ratio = (double)image_size / cw, h_ratio = (double)image_size / ch;
    const double hi = (double)(image_size - 1);
    const int cnt = min(max(counts[e], 0), max_obj);
    const double* bx = boxes + e * (size_t)max_obj * 5;
    for (int o = 0; o < cnt; ++o, bx += 5) {
        const WindowBox b = window_box(bx, wx0, wy0, w_ratio, h_ratio, hi, (double)image_size);
        if (WINDOW && !b.keep) continue;        // the centre left the window
        const double cx = b.cx(), cy = b.cy();
        int x_ind = (int)(cx * S / image_size), y_ind = (int)(cy * S / image_size);
        if (!(x_ind >= 0 && x_ind < S && y_ind >= 0 && y_ind < S)) continue;   // (not a number in the box table)
        if (flip) x_ind = S - 1 - x_ind;
        float* cell = g + ((size_t)y_ind * S + x_ind) * D;
        if (cell[0] == 1.0f) continue;
        cell[0] = 1.0f;
        cell[1] = (float)(flip ? hi - cx : cx);
        cell[2] = (float)cy;
        cell[3] = (float)b.w();
        cell[4] = (float)b.h();
        const int cls = (int)bx[4];
        if (cls >= 0 && cls < num_class) cell[5 + cls] = 1.0f;
    }
}

}  // namespace
