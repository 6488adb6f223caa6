// Training augmentation on the device-resident image pool (img_dataset/device_voc.py with an Augment): one launch makes
// the finished uint8 BGR batch -- crop / pad window of the source, bilinear resize, mirror, hue / saturation / exposure
// distortion -- and a second one the label grids whose boxes follow the window.  The specification is the host code of
// img_dataset/augment.py (crop_resize_u8, distort_hsv_u8, encode_boxes_window) and both kernels are bit-equal to it:
// resize coefficients in double in the specification's operation order (as data.hip), the colour stage in float32
// with one correctly rounded operation per specification operation.  The file is compiled with -ffp-contract=off: a
// fused multiply-add in x * 255 + 0.5 or 1 - s * f rounds once where the specification rounds twice.
// Here: what the window, the colour stage and the warp need of their own (the x table with fill flags, tap_pixel,
// distort_pixel, the band loop with its staging of rows outside the image, the box-list compaction, the warp's tiles).
// Coefficients, blend, three-dword store, the window arithmetic of the boxes and the body of the label-grid kernel are
// data_common.h's: one definition with data.hip.
#include "data_common.h"
using namespace y2;

namespace {

// XCoef here: offsets CLAMPED into the source row (every address is readable whatever the window is), and above the
// 11-bit weight (0 .. 2048) of w1 a flag where that pixel of the window lies outside the image and reads as the fill
constexpr int kFillLeft = 1 << 12, kFillRight = 1 << 13;

// window index i -> source index x0 + i clamped into [0, n), and whether it was outside
Y2_DEV int src_index(int x0, int i, int n, bool& outside) {
    const long long s = (long long)x0 + i;
    outside = s < 0 || s >= n;
    return (int)min(max(s, 0LL), (long long)n - 1);
}

// one output pixel, b | g << 8 | r << 16, from the taps at bytes ca (left) and cb (right) of the source rows r0 / r1 (LDS
// or global): fl / fr / f0 / f1 say that the left / right column, the upper / lower row lies outside the image -- such a
// tap reads `fill`, whatever its (readable) address holds
template <typename Off>
Y2_DEV uint32_t tap_pixel(const uint8_t* r0, const uint8_t* r1, Off ca, Off cb, bool fl, bool fr, bool f0, bool f1,
                          int wx1, int wy1, int fill) {
    uint32_t packed = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v00 = (fl || f0) ? fill : (int)r0[ca + c], v01 = (fr || f0) ? fill : (int)r0[cb + c];
        const int v10 = (fl || f1) ? fill : (int)r1[ca + c], v11 = (fr || f1) ? fill : (int)r1[cb + c];
        packed |= (uint32_t)(blend4(v00, v01, v10, v11, wx1, wy1) & 255) << (8 * c);
    }
    return packed;
}

// one pixel of the row-staged resize: f0 / f1 say that the whole source row lies outside the image
Y2_DEV uint32_t resize_pixel(const uint8_t* r0, const uint8_t* r1, const XCoef q, int wy1, bool f0, bool f1, int fill) {
    return tap_pixel(r0, r1, q.x0, q.x0 + q.dx, q.w1 & kFillLeft, q.w1 & kFillRight, f0, f1, q.w1 & 4095, wy1, fill);
}

Y2_DEV uint32_t to_u8(float x) { return (uint32_t)min(max((int)(x * 255.0f + 0.5f), 0), 255); }

// distort_hsv_u8 of one pixel (b | g << 8 | r << 16); unit[c] = c / 255 in float32
Y2_DEV uint32_t distort_pixel(uint32_t bgr, const float* unit, float hue6, float sat, float exp) {
    const float b = unit[bgr & 255], g = unit[(bgr >> 8) & 255], r = unit[(bgr >> 16) & 255];
    float v = fmaxf(fmaxf(r, g), b);
    const float d = v - fminf(fminf(r, g), b);
    float s = v == 0.0f ? 0.0f : d / (v == 0.0f ? 1.0f : v);
    const float num = v == r ? g - b : (v == g ? b - r : r - g);
    const float qd = num / (d == 0.0f ? 1.0f : d);
    float h = v == r ? qd : (v == g ? 2.0f + qd : 4.0f + qd);
    h = d == 0.0f ? 0.0f : h;
    h = h + hue6;
    h = h < 0.0f ? h + 6.0f : h;
    h = h >= 6.0f ? h - 6.0f : h;
    s = fminf(s * sat, 1.0f);
    v = fminf(v * exp, 1.0f);
    const float i = floorf(h), f = h - i;
    const float p = v * (1.0f - s);
    const float q = v * (1.0f - s * f);
    const float t = v * (1.0f - s * (1.0f - f));
    const float r2 = (i == 0.0f || i >= 5.0f) ? v : (i == 1.0f ? q : (i == 4.0f ? t : p));
    const float g2 = i == 0.0f ? t : ((i == 1.0f || i == 2.0f) ? v : (i == 3.0f ? q : p));
    const float b2 = i == 2.0f ? t : ((i == 3.0f || i == 4.0f) ? v : (i >= 5.0f ? q : p));
    return to_u8(b2) | to_u8(g2) << 8 | to_u8(r2) << 16;
}

// `gr` output rows of `groups` * VEC pixels each.  STAGED: row j blends slots 2j and 2j + 1 of the LDS staging, `pitch`
// bytes apart (rows outside the image were staged as fill); else it reads rows y[0] and y[1] of the image in place and
// the row flags of y[3] select the fill.  Two instantiations, so that the staged one reads LDS with LDS instructions.
template <int VEC, bool STAGED>
Y2_DEV void produce_rows(const uint8_t* base, int64_t pitch, const XCoef* xt, const int (*yc)[4], const float* unit, int gr,
                         int groups, bool colour, float hue6, float sat, float exp, int fill, uint8_t* obase,
                         int rowbytes) {
    const int total = gr * groups;
    for (int k = threadIdx.x; k < total; k += kThreads) {
        const int j = k / groups, px = (k - j * groups) * VEC;
        const int* y = yc[j];
        const uint8_t* r0 = STAGED ? base + (2 * j) * (int)pitch : base + (size_t)y[0] * pitch;
        const uint8_t* r1 = STAGED ? base + (2 * j + 1) * (int)pitch : base + (size_t)y[1] * pitch;
        const bool f0 = !STAGED && (y[3] & 1), f1 = !STAGED && (y[3] & 2);
        uint32_t pix[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) pix[e] = resize_pixel(r0, r1, xt[px + e], y[2], f0, f1, fill);
        if (colour) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) pix[e] = distort_pixel(pix[e], unit, hue6, sat, exp);
        }
        uint8_t* o = obase + (size_t)j * rowbytes + 3 * px;
        if (VEC == 4) {
            store_px4((uint32_t*)o, pix);
        } else {
            o[0] = (uint8_t)pix[0];
            o[1] = (uint8_t)(pix[0] >> 8);
            o[2] = (uint8_t)(pix[0] >> 16);
        }
    }
}

// grid (ceil(out_h / kBand), n), the geometry of data.hip's resize kernel.  A workgroup owns kBand output rows of one
// batch slot: the x coefficients of its window (mirrored when exactly one of the entry's and the row's flips is set)
// and the c / 255 table are computed once into LDS; for every kRows output rows the 2 * kRows source rows they blend are
// staged into LDS with 16-byte loads (a row outside the image is staged as fill bytes, without a load), and each lane
// produces VEC whole pixels -- the colour stage needs the triple -- stored as 3 * VEC bytes (VEC = 4: three dwords).
template <int VEC>
__global__ __launch_bounds__(kThreads) void augment_u8_kernel(const uint8_t* __restrict__ pool,
                                                              const int64_t* __restrict__ table,
                                                              const int32_t* __restrict__ index,
                                                              const double* __restrict__ params, int out_h, int out_w,
                                                              int fill, uint8_t* __restrict__ out) {
    __shared__ XCoef xt[kMaxOutW];
    __shared__ int yc[kBand][4];                // source rows (clamped), weight, bit 0 / 1: row 0 / 1 is outside
    __shared__ float unit[256];
    __shared__ __attribute__((aligned(16))) uint8_t rows[2 * kRows * kMaxPitch];
    const int tid = threadIdx.x, img = blockIdx.y;
    const int64_t* t = table + (size_t)kTable * (index ? index[img] : img);
    const double* prm = params + (size_t)kParams * img;
    const int64_t off = t[0], pitch64 = t[3];
    const int H = (int)t[1], W = (int)t[2];
    const int wx0 = win_int(prm[0], -(1 << 30), 1 << 30), wy0 = win_int(prm[1], -(1 << 30), 1 << 30);
    const int cw = win_int(prm[2], 0, 1 << 30), ch = win_int(prm[3], 0, 1 << 30);
    const bool flip = (t[4] != 0) != (prm[4] != 0.0);
    const float hue = (float)prm[5], sat = (float)prm[6], exp = (float)prm[7];
    const bool colour = !(hue == 0.0f && sat == 1.0f && exp == 1.0f);
    const float hue6 = 6.0f * hue;
    const int band0 = blockIdx.x * kBand, nrows = min(kBand, out_h - band0);
    if (H < 1 || W < 1) return;                 // (an empty table row: nothing to read, as data.hip)
    if (cw < 1 || ch < 1) {                     // no window (or not a number): the slot is all fill, its grid empty
        uint8_t* o = out + ((size_t)img * out_h + band0) * 3 * out_w;
        for (int i = tid; i < nrows * 3 * out_w; i += kThreads) o[i] = (uint8_t)fill;
        return;
    }
    for (int x = tid; x < out_w; x += kThreads) {
        int i0, i1, w1;
        bool o0, o1;
        lin_coef(flip ? out_w - 1 - x : x, cw, out_w, i0, i1, w1);
        const int c0 = src_index(wx0, i0, W, o0), c1 = src_index(wx0, i1, W, o1);
        xt[x] = XCoef{3 * c0, (short)(3 * (c1 - c0)), (short)(w1 | (o0 ? kFillLeft : 0) | (o1 ? kFillRight : 0))};
    }
    if (tid < nrows) {
        int i0, i1, w1;
        bool o0, o1;
        lin_coef(band0 + tid, ch, out_h, i0, i1, w1);
        yc[tid][0] = src_index(wy0, i0, H, o0);
        yc[tid][1] = src_index(wy0, i1, H, o1);
        yc[tid][2] = w1;
        yc[tid][3] = (o0 ? 1 : 0) | (o1 ? 2 : 0);
    }
    unit[tid] = (float)tid / 255.0f;            // kThreads == 256
    __syncthreads();
    const bool staged = pitch64 <= kMaxPitch && stageable(off, pitch64, W);
    const int pitch = (int)pitch64;
    const uint8_t* src = pool + off;
    const int rowbytes = 3 * out_w, groups = out_w / VEC;   // (VEC = 4 is launched for out_w % 4 == 0 only)
    const uint32_t fill4 = 0x01010101u * (uint32_t)fill;
    uint8_t* obase = out + ((size_t)img * out_h + band0) * rowbytes;
    for (int g0 = 0; g0 < nrows; g0 += kRows) {
        const int gr = min(kRows, nrows - g0);
        if (staged) {
            const int chunks = pitch >> 4;          // data_common.h's stage_rows with the fill: see there
            for (int i = tid; i < 2 * gr * chunks; i += kThreads) {
                const int slot = i / chunks, c = i - slot * chunks;
                const int* y = yc[g0 + (slot >> 1)];
                u32x4 v = {fill4, fill4, fill4, fill4};
                if (!((y[3] >> (slot & 1)) & 1)) v = *(const u32x4*)(src + (size_t)y[slot & 1] * pitch64 + 16 * c);
                *(u32x4*)(rows + slot * pitch + 16 * c) = v;
            }
            __syncthreads();
        }
        if (staged)
            produce_rows<VEC, true>(rows, pitch, xt, yc + g0, unit, gr, groups, colour, hue6, sat, exp, fill,
                                    obase + (size_t)g0 * rowbytes, rowbytes);
        else
            produce_rows<VEC, false>(src, pitch64, xt, yc + g0, unit, gr, groups, colour, hue6, sat, exp, fill,
                                     obase + (size_t)g0 * rowbytes, rowbytes);
        if (staged) __syncthreads();
    }
}

// the label grid with the boxes following the window (data_common.h: encode_labels): x = (bx - 1 - x0) * (image_size /
// cw), an object whose unclamped centre leaves [0, image_size) is dropped, and the mirror is the entry's flip XOR the row's
__global__ __launch_bounds__(kThreads) void encode_labels_window_kernel(const double* __restrict__ boxes,
                                                                        const int32_t* __restrict__ counts,
                                                                        const int64_t* __restrict__ table,
                                                                        const int32_t* __restrict__ index,
                                                                        const double* __restrict__ params, int max_obj,
                                                                        int image_size, int S, int num_class,
                                                                        float* __restrict__ labels) {
    encode_labels<true>(boxes, counts, table, index, params, max_obj, image_size, S, num_class, labels);
}

// The label of the anchor model that keeps every object (augment.encode_box_list): grid (n), ONE 64-lane wave per image.
// Lane l owns objects l, l + 64, ...: the window arithmetic of the kernel above in double, keep or drop.  The kept
// objects of a round of 64 are compacted in annotation order with a ballot and the count of kept lanes below (no
// atomics: order and the max_boxes cut do not depend on timing), then the rows beyond the count are zero-filled.
// params == nullptr: the identity row {0, 0, width, height, 0} of every entry, the plain path.
__global__ __launch_bounds__(64) void encode_box_list_kernel(const double* __restrict__ boxes,
                                                             const int32_t* __restrict__ counts,
                                                             const int64_t* __restrict__ table,
                                                             const int32_t* __restrict__ index,
                                                             const double* __restrict__ params, int max_obj,
                                                             int image_size, int max_boxes, float* __restrict__ truth,
                                                             int32_t* __restrict__ ntruth) {
    const int img = blockIdx.x, lane = threadIdx.x;
    const size_t e = index ? (size_t)index[img] : (size_t)img;
    const int64_t* t = table + kTable * e;
    double wx0 = 0.0, wy0 = 0.0, cw = (double)t[2], ch = (double)t[1];
    bool flip = t[4] != 0;
    if (params) flip = read_window(params + (size_t)kParams * img, flip, wx0, wy0, cw, ch);
    const bool window = cw >= 1.0 && ch >= 1.0;           // a row without a window: an empty list
    const double w_ratio = (double)image_size / cw, h_ratio = (double)image_size / ch;
    const double hi = (double)(image_size - 1), size = (double)image_size;
    const int cnt = window ? min(max(counts[e], 0), max_obj) : 0;
    const double* bx0 = boxes + e * (size_t)max_obj * 5;
    float* out = truth + (size_t)img * max_boxes * 5;
    int base = 0;                                         // rows written by the rounds before (wave-uniform)
    for (int o0 = 0; o0 < cnt && base < max_boxes; o0 += 64) {
        const int o = o0 + lane;
        bool keep = false;
        double cx = 0.0, cy = 0.0, bw = 0.0, bh = 0.0;
        int cls = 0;
        if (o < cnt) {
            const double* bx = bx0 + (size_t)o * 5;
            const WindowBox b = window_box(bx, wx0, wy0, w_ratio, h_ratio, hi, size);
            keep = b.keep;                                // else the centre left the window (or not a number)
            cx = b.cx(); cy = b.cy();
            bw = b.w(); bh = b.h();
            cls = (int)bx[4];
        }
        const unsigned long long kept = __ballot(keep);
        const int pos = base + __popcll(kept & ((1ull << lane) - 1ull));
        if (keep && pos < max_boxes) {
            float* r = out + (size_t)pos * 5;
            r[0] = (float)(flip ? hi - cx : cx);
            r[1] = (float)cy;
            r[2] = (float)bw;
            r[3] = (float)bh;
            r[4] = (float)cls;
        }
        base += __popcll(kept);
    }
    const int rows = min(base, max_boxes);
    for (int i = rows * 5 + lane; i < max_boxes * 5; i += 64) out[i] = 0.0f;
    if (lane == 0) ntruth[img] = rows;
}

// augment.box_rank: the 32-bit hash of (key, annotation index) that orders an image's objects for the draw.  32-bit
// integer operations only -- xor, shift, multiply modulo 2^32 -- so that numpy and this function agree on every bit.
Y2_DEV uint32_t box_rank(uint32_t key, uint32_t j) {
    uint32_t x = key ^ (j * 0x9E3779B9u);
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

constexpr int kDrawMaxObj = 1024;               // Y2_DRAW_MAX_OBJ: objects per entry the draw kernel holds ballots for
constexpr int kDrawRounds = kDrawMaxObj / 64;

// The box list with Darknet's shuffle-then-cut (augment.encode_box_list_draw): grid (n), ONE 64-lane wave per image, the
// arithmetic and the layout of the kernel above.  Where an image has more surviving objects than max_boxes, the ones
// kept are the max_boxes with the smallest (box_rank(key, j), j), written in annotation order:
//   round one   window_box per object, keep or drop; the ballot of every round of 64 goes to LDS (kDrawRounds words)
//   round two   a surviving lane counts the survivors that rank before it: the ballot words are wave-uniform, so the walk
//               over their set bits is a scalar loop, and every lane recomputes the other object's hash -- no sort, no
//               atomics, nothing depends on timing.  It is selected when fewer than max_boxes rank before it
//   compaction  the selected lanes of a round, with the ballot and the count of selected lanes below
// With at most max_boxes survivors, or keys == nullptr, every survivor is selected and the pos < max_boxes guard is the
// kernel above's cut: the same rows bit for bit.  The box is formed again in round two rather than held: the rounds of
// an image are few, and a per-round register array would be indexed at run time (scratch).
__global__ __launch_bounds__(64) void encode_box_list_draw_kernel(const double* __restrict__ boxes,
                                                                  const int32_t* __restrict__ counts,
                                                                  const int64_t* __restrict__ table,
                                                                  const int32_t* __restrict__ index,
                                                                  const double* __restrict__ params,
                                                                  const uint32_t* __restrict__ keys, int max_obj,
                                                                  int image_size, int max_boxes,
                                                                  float* __restrict__ truth,
                                                                  int32_t* __restrict__ ntruth) {
    __shared__ unsigned long long kept[kDrawRounds];
    const int img = blockIdx.x, lane = threadIdx.x;
    const size_t e = index ? (size_t)index[img] : (size_t)img;
    const int64_t* t = table + kTable * e;
    double wx0 = 0.0, wy0 = 0.0, cw = (double)t[2], ch = (double)t[1];
    bool flip = t[4] != 0;
    if (params) flip = read_window(params + (size_t)kParams * img, flip, wx0, wy0, cw, ch);
    const bool window = cw >= 1.0 && ch >= 1.0;           // a row without a window: an empty list
    const double w_ratio = (double)image_size / cw, h_ratio = (double)image_size / ch;
    const double hi = (double)(image_size - 1), size = (double)image_size;
    const int cnt = window ? min(max(counts[e], 0), min(max_obj, kDrawMaxObj)) : 0;
    const int rounds = (cnt + 63) >> 6;                   // <= kDrawRounds
    const double* bx0 = boxes + e * (size_t)max_obj * 5;
    float* out = truth + (size_t)img * max_boxes * 5;
    const unsigned long long below = (1ull << lane) - 1ull;
    int survivors = 0;
    for (int r = 0; r < rounds; ++r) {
        const int o = r * 64 + lane;
        const bool keep = o < cnt && window_box(bx0 + (size_t)o * 5, wx0, wy0, w_ratio, h_ratio, hi, size).keep;
        const unsigned long long b = __ballot(keep);
        if (lane == 0) kept[r] = b;
        survivors += __popcll(b);
    }
    __syncthreads();
    const bool draw = keys != nullptr && survivors > max_boxes;          // (wave-uniform)
    const uint32_t key = keys ? keys[img] : 0u;
    int base = 0;                                         // rows written by the rounds before (wave-uniform)
    for (int r = 0; r < rounds; ++r) {
        const int o = r * 64 + lane;
        bool sel = (kept[r] >> lane) & 1ull;
        if (draw) {
            const uint32_t mine = box_rank(key, (uint32_t)o);
            int before = 0;
            for (int r2 = 0; r2 < rounds; ++r2) {
                for (unsigned long long m = kept[r2]; m; m &= m - 1ull) {
                    const int j = r2 * 64 + __builtin_ctzll(m);
                    const uint32_t other = box_rank(key, (uint32_t)j);
                    before += (other < mine || (other == mine && j < o)) ? 1 : 0;
                }
            }
            sel = sel && before < max_boxes;
        }
        const unsigned long long chosen = __ballot(sel);
        const int pos = base + __popcll(chosen & below);
        if (sel && pos < max_boxes) {
            const double* bx = bx0 + (size_t)o * 5;
            const WindowBox b = window_box(bx, wx0, wy0, w_ratio, h_ratio, hi, size);
            float* row = out + (size_t)pos * 5;
            row[0] = (float)(flip ? hi - b.cx() : b.cx());
            row[1] = (float)b.cy();
            row[2] = (float)b.w();
            row[3] = (float)b.h();
            row[4] = (float)(int)bx[4];
        }
        base += __popcll(chosen);
    }
    const int rows = min(base, max_boxes);
    for (int i = rows * 5 + lane; i < max_boxes * 5; i += 64) out[i] = 0.0f;
    if (lane == 0) ntruth[img] = rows;
}

// ---- The classifier's augmentation (img_dataset/augment_cls.py): mirror, rotation, scale and crop are ONE affine map from
// an output pixel index to a source coordinate, so the kernel is a gather of four taps per pixel through that map -- not
// the row-staged resize above, whose window is axis-aligned.  Bit-equal to augment_cls.warp_affine_u8 + distort_hsv_u8:
// the coordinates in double with every product and sum rounded on its own (-ffp-contract=off), the validity test before
// any conversion to integer, the blend in int32, the colour stage through distort_pixel.
constexpr int kWarpParams = 9;                  // double per batch slot: m00 m01 m02 m10 m11 m12, hue, sat, exp
constexpr int kWarpTile = 32;                   // a workgroup owns kWarpTile x kWarpTile output pixels: 4 per lane
constexpr int kWarpLds = 32768;                 // bytes of source staged per tile (augment_cls.LDS_BUDGET)
constexpr double kWarpLimit = 1073741824.0;     // a coordinate of this magnitude, or not finite, reads as fill

struct WarpMap { double m00, m01, m02, m10, m11, m12; };

// source coordinate of output pixel (u, v); false: not a coordinate (not finite, or |c| >= 2^30) -> the pixel is fill
Y2_DEV bool warp_coord(const WarpMap& m, int u, int v, double& sx, double& sy) {
    const double du = (double)u, dv = (double)v;
    sx = (m.m00 * du + m.m01 * dv) + m.m02;
    sy = (m.m10 * du + m.m11 * dv) + m.m12;
    return fabs(sx) < kWarpLimit && fabs(sy) < kWarpLimit;
}

// one output pixel, b | g << 8 | r << 16.  STAGED: `base` is the LDS copy of source rows ly0 .. ly1, `pitch` bytes each,
// whose byte 0 is byte `a0` of the source row; else `base` is the image in the pool (a0 = 0, ly0 = 0).  A tap inside the
// image lies inside [lx0, lx1] x [ly0, ly1] (the tile's box, or the image); one outside reads `fill` and its address
// is clamped into that rectangle, so that every address formed is readable.
template <bool STAGED>
Y2_DEV uint32_t warp_pixel(const uint8_t* base, int64_t pitch, int64_t a0, int lx0, int lx1, int ly0, int ly1, int H,
                           int W, const WarpMap& m, int u, int v, int fill) {
    double sx, sy;
    if (!warp_coord(m, u, v, sx, sy)) return 0x010101u * (uint32_t)fill;
    const double fx = floor(sx), fy = floor(sy);
    const int x0 = (int)fx, y0 = (int)fy;       // |c| < 2^30
    const int wx1 = (int)((sx - fx) * 2048.0 + 0.5), wy1 = (int)((sy - fy) * 2048.0 + 0.5);
    const bool ol = x0 < 0 || x0 >= W, orr = x0 + 1 < 0 || x0 + 1 >= W;
    const bool ot = y0 < 0 || y0 >= H, ob = y0 + 1 < 0 || y0 + 1 >= H;
    const int xa = min(max(x0, lx0), lx1), xb = min(max(x0 + 1, lx0), lx1);
    const int ya = min(max(y0, ly0), ly1), yb = min(max(y0 + 1, ly0), ly1);
    if (STAGED)                                 // its own row pointers and 32-bit offsets: LDS read with LDS instructions
        return tap_pixel(base + (ya - ly0) * (int)pitch, base + (yb - ly0) * (int)pitch, 3 * xa - (int)a0,
                         3 * xb - (int)a0, ol, orr, ot, ob, wx1, wy1, fill);
    return tap_pixel(base + (size_t)ya * pitch, base + (size_t)yb * pitch, 3 * (size_t)xa, 3 * (size_t)xb, ol, orr, ot,
                     ob, wx1, wy1, fill);
}

// the lane's 4 pixels (u .. u + 3, v) of one tile: gather, colour, three dwords
template <bool STAGED>
Y2_DEV void warp_produce(const uint8_t* base, int64_t pitch, int64_t a0, int lx0, int lx1, int ly0, int ly1, int H, int W,
                         const WarpMap& m, int u, int v, int fill, bool colour, const float* unit, float hue6, float sat,
                         float exp, uint32_t* o32) {
    uint32_t pix[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) pix[e] = warp_pixel<STAGED>(base, pitch, a0, lx0, lx1, ly0, ly1, H, W, m, u + e, v, fill);
    if (colour) {
#pragma unroll
        for (int e = 0; e < 4; ++e) pix[e] = distort_pixel(pix[e], unit, hue6, sat, exp);
    }
    store_px4(o32, pix);
}

// grid (tiles of kWarpTile x kWarpTile output pixels, n), 256 lanes; lane l produces the 4 pixels 4 (l % 8) .. + 3 of tile
// row l / 8 and stores them as three dwords (out_w % 4 == 0, `out` 4-byte aligned).  The source box of the tile is
// spanned by its four corners through the map -- the map is monotone in u and in v, rounding included -- plus one pixel
// for the second tap, cut to the image:
//   a corner that is no coordinate   every pixel decides for itself, the taps read the pool in place
//   the box is empty                 the tile is fill (through the colour stage), nothing is read
//   the 16-byte aligned row segments of the box fit kWarpLds bytes: staged with 16-byte loads (pool rows start on 16-byte
//                                    boundaries and the pitch is a multiple of 16: an aligned superset of a segment lies
//                                    inside the row), and the taps read LDS
//   else (strong down-scaling)       the taps read the pool in place
// The choice depends on the table row, the parameter row and the tile alone (augment_cls.tile_path restates it).
// PARAMS = false: no parameter rows; the map is augment_cls.identity_row of the table row, formed here in the same
// float64 operations, and there is no colour stage.  One lane per batch slot copies the slot's class label.
template <bool PARAMS>
__global__ __launch_bounds__(kThreads) void warp_u8_kernel(const uint8_t* __restrict__ pool,
                                                           const int64_t* __restrict__ table,
                                                           const int32_t* __restrict__ index,
                                                           const double* __restrict__ params,
                                                           const int32_t* __restrict__ labels, int out_h, int out_w,
                                                           int fill, uint8_t* __restrict__ out,
                                                           int32_t* __restrict__ labels_out) {
    __shared__ float unit[256];
    __shared__ __attribute__((aligned(16))) uint8_t rows[kWarpLds];
    const int tid = threadIdx.x, img = blockIdx.y;
    const size_t e = index ? (size_t)index[img] : (size_t)img;
    if (labels_out && blockIdx.x == 0 && tid == 0) labels_out[img] = labels[e];
    const int64_t* t = table + (size_t)kTable * e;
    const int64_t off = t[0], pitch64 = t[3];
    const int H = (int)t[1], W = (int)t[2];
    if (H < 1 || W < 1) return;                 // (an empty table row: nothing to read, as data.hip)
    WarpMap m;
    float hue = 0.0f, sat = 1.0f, exp = 1.0f;
    if (PARAMS) {
        const double* prm = params + (size_t)kWarpParams * img;
        m = WarpMap{prm[0], prm[1], prm[2], prm[3], prm[4], prm[5]};
        hue = (float)prm[6]; sat = (float)prm[7]; exp = (float)prm[8];
    } else {                                    // compose(H, W, out_w, out_h, 0, 0, angle 0, no mirror): alpha 1, beta 0
        const double ax = (double)W / (double)out_w, ay = (double)H / (double)out_h;
        const double bx = 0.5 * ax - 0.5, by = 0.5 * ay - 0.5;
        const double cx = (double)(W / 2), cy = (double)(H / 2);
        m = WarpMap{ax, 0.0, (bx - cx) + cx, 0.0, ay, (by - cy) + cy};
    }
    const bool colour = PARAMS && !(hue == 0.0f && sat == 1.0f && exp == 1.0f);
    const float hue6 = 6.0f * hue;
    if (colour) {                               // (uniform in the workgroup)
        unit[tid] = (float)tid / 255.0f;        // kThreads == 256
        __syncthreads();
    }
    const int tiles_x = (out_w + kWarpTile - 1) / kWarpTile;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int u0 = tx * kWarpTile, v0 = ty * kWarpTile;
    const int u1 = min(u0 + kWarpTile - 1, out_w - 1), v1 = min(v0 + kWarpTile - 1, out_h - 1);
    const int u = u0 + 4 * (tid & 7), v = v0 + (tid >> 3);
    const bool active = u < out_w && v < out_h;             // out_w % 4 == 0: the 4 pixels are inside together
    uint32_t* o32 = (uint32_t*)(out + (((size_t)img * out_h + (active ? v : 0)) * out_w + (active ? u : 0)) * 3);
    const uint8_t* src = pool + off;
    double x00, y00, x10, y10, x01, y01, x11, y11;
    bool box = warp_coord(m, u0, v0, x00, y00);
    box = warp_coord(m, u1, v0, x10, y10) && box;
    box = warp_coord(m, u0, v1, x01, y01) && box;
    box = warp_coord(m, u1, v1, x11, y11) && box;
    if (box) {
        const int bx0 = max((int)floor(fmin(fmin(x00, x10), fmin(x01, x11))), 0);
        const int bx1 = min((int)floor(fmax(fmax(x00, x10), fmax(x01, x11))) + 1, W - 1);
        const int by0 = max((int)floor(fmin(fmin(y00, y10), fmin(y01, y11))), 0);
        const int by1 = min((int)floor(fmax(fmax(y00, y10), fmax(y01, y11))) + 1, H - 1);
        if (bx0 > bx1 || by0 > by1) {           // every tap of every pixel lies outside the image
            if (!active) return;
            uint32_t p = 0x010101u * (uint32_t)fill;
            if (colour) p = distort_pixel(p, unit, hue6, sat, exp);
            const uint32_t pix[4] = {p, p, p, p};
            store_px4(o32, pix);
            return;
        }
        const int64_t a0 = (3 * (int64_t)bx0) & ~(int64_t)15, a1 = (3 * (int64_t)bx1 + 3 + 15) & ~(int64_t)15;
        const int64_t seg = a1 - a0, nrow = (int64_t)by1 - by0 + 1;
        if (stageable(off, pitch64, W) && seg * nrow <= kWarpLds) {
            const int chunks = (int)(seg >> 4), total = chunks * (int)nrow;
            for (int i = tid; i < total; i += kThreads) {
                const int r = i / chunks, c = i - r * chunks;
                *(u32x4*)(rows + r * (int)seg + 16 * c) =
                    *(const u32x4*)(src + (size_t)(by0 + r) * pitch64 + a0 + 16 * c);
            }
            __syncthreads();
            if (active)
                warp_produce<true>(rows, seg, a0, bx0, bx1, by0, by1, H, W, m, u, v, fill, colour, unit, hue6, sat, exp,
                                   o32);
            return;
        }
    }
    if (active)
        warp_produce<false>(src, pitch64, 0, 0, W - 1, 0, H - 1, H, W, m, u, v, fill, colour, unit, hue6, sat, exp, o32);
}

}  // namespace

extern "C" {

int y2_warp_u8_batch(const uint8_t* pool, const int64_t* table, const int32_t* index, const double* params,
                     const int32_t* labels, int n, int out_h, int out_w, int fill, uint8_t* out, int32_t* labels_out,
                     void* stream) {
    if (!pool || !table || !out) return fail(Y2_ERR_ARG, "y2_warp_u8_batch: null pointer");
    if (n < 1 || n > 65535) return fail(Y2_ERR_ARG, "y2_warp_u8_batch: n = %d outside 1..65535", n);
    if (out_h < 1 || out_w < 4 || out_w % 4)
        return fail(Y2_ERR_ARG, "y2_warp_u8_batch: output %d x %d (out_w must be a positive multiple of 4)", out_h, out_w);
    if (fill < 0 || fill > 255) return fail(Y2_ERR_ARG, "y2_warp_u8_batch: fill = %d outside 0..255", fill);
    if ((uintptr_t)out & 3) return fail(Y2_ERR_ARG, "y2_warp_u8_batch: out is not 4-byte aligned");
    if ((labels == nullptr) != (labels_out == nullptr))
        return fail(Y2_ERR_ARG, "y2_warp_u8_batch: labels and labels_out come together or not at all");
    const int64_t tiles = (int64_t)((out_w + kWarpTile - 1) / kWarpTile) * ((out_h + kWarpTile - 1) / kWarpTile);
    if (tiles > 0x7fffffff) return fail(Y2_ERR_ARG, "y2_warp_u8_batch: output %d x %d has too many tiles", out_h, out_w);
    const dim3 grid((unsigned)tiles, n);
    if (params)
        hipLaunchKernelGGL(warp_u8_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, pool, table, index, params,
                           labels, out_h, out_w, fill, out, labels_out);
    else
        hipLaunchKernelGGL(warp_u8_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, pool, table, index, params,
                           labels, out_h, out_w, fill, out, labels_out);
    return launched("y2_warp_u8_batch");
}

int y2_encode_box_list(const double* boxes, const int32_t* counts, const int64_t* table, const int32_t* index,
                       const double* params, int n, int max_obj, int image_size, int max_boxes, float* truth,
                       int32_t* ntruth, void* stream) {
    if (!boxes || !counts || !table || !truth || !ntruth) return fail(Y2_ERR_ARG, "y2_encode_box_list: null pointer");
    if (n < 1) return fail(Y2_ERR_ARG, "y2_encode_box_list: n = %d", n);
    if (max_obj < 1 || image_size < 1)
        return fail(Y2_ERR_ARG, "y2_encode_box_list: max_obj = %d, image_size = %d", max_obj, image_size);
    if (max_boxes < 1 || max_boxes > Y2_MAX_BOXES)
        return fail(Y2_ERR_ARG, "y2_encode_box_list: max_boxes = %d outside 1..%d", max_boxes, Y2_MAX_BOXES);
    hipLaunchKernelGGL(encode_box_list_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, boxes, counts, table, index,
                       params, max_obj, image_size, max_boxes, truth, ntruth);
    return launched("y2_encode_box_list");
}

int y2_encode_box_list_draw(const double* boxes, const int32_t* counts, const int64_t* table, const int32_t* index,
                            const double* params, const uint32_t* keys, int n, int max_obj, int image_size,
                            int max_boxes, float* truth, int32_t* ntruth, void* stream) {
    if (!boxes || !counts || !table || !truth || !ntruth)
        return fail(Y2_ERR_ARG, "y2_encode_box_list_draw: null pointer");
    if (n < 1) return fail(Y2_ERR_ARG, "y2_encode_box_list_draw: n = %d", n);
    if (max_obj < 1 || image_size < 1)
        return fail(Y2_ERR_ARG, "y2_encode_box_list_draw: max_obj = %d, image_size = %d", max_obj, image_size);
    if (max_obj > kDrawMaxObj)
        return fail(Y2_ERR_ARG, "y2_encode_box_list_draw: max_obj = %d beyond Y2_DRAW_MAX_OBJ = %d", max_obj, kDrawMaxObj);
    if (max_boxes < 1 || max_boxes > Y2_MAX_BOXES)
        return fail(Y2_ERR_ARG, "y2_encode_box_list_draw: max_boxes = %d outside 1..%d", max_boxes, Y2_MAX_BOXES);
    hipLaunchKernelGGL(encode_box_list_draw_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, boxes, counts, table,
                       index, params, keys, max_obj, image_size, max_boxes, truth, ntruth);
    return launched("y2_encode_box_list_draw");
}

int y2_augment_u8_batch(const uint8_t* pool, const int64_t* table, const int32_t* index, const double* params, int n,
                        int out_h, int out_w, int fill, uint8_t* out, void* stream) {
    if (!pool || !table || !params || !out) return fail(Y2_ERR_ARG, "y2_augment_u8_batch: null pointer");
    if (n < 1 || n > 65535) return fail(Y2_ERR_ARG, "y2_augment_u8_batch: n = %d outside 1..65535", n);
    if (out_h < 1 || out_w < 1) return fail(Y2_ERR_ARG, "y2_augment_u8_batch: output %d x %d", out_h, out_w);
    if (out_w > kMaxOutW)
        return fail(Y2_ERR_ARG, "y2_augment_u8_batch: out_w = %d beyond Y2_RESIZE_MAX_OUT_W = %d", out_w, kMaxOutW);
    if (fill < 0 || fill > 255) return fail(Y2_ERR_ARG, "y2_augment_u8_batch: fill = %d outside 0..255", fill);
    const dim3 grid((out_h + kBand - 1) / kBand, n);
    if (out_w % 4 == 0 && ((uintptr_t)out & 3) == 0)
        hipLaunchKernelGGL(augment_u8_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, pool, table, index, params,
                           out_h, out_w, fill, out);
    else
        hipLaunchKernelGGL(augment_u8_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, pool, table, index, params,
                           out_h, out_w, fill, out);
    return launched("y2_augment_u8_batch");
}

int y2_encode_labels_window(const double* boxes, const int32_t* counts, const int64_t* table, const int32_t* index,
                            const double* params, int n, int max_obj, int image_size, int S, int num_class,
                            float* labels, void* stream) {
    if (!boxes || !counts || !table || !params || !labels)
        return fail(Y2_ERR_ARG, "y2_encode_labels_window: null pointer");
    if (n < 1) return fail(Y2_ERR_ARG, "y2_encode_labels_window: n = %d", n);
    if (max_obj < 1 || image_size < 1 || S < 1 || num_class < 0 || S > 1024)
        return fail(Y2_ERR_ARG, "y2_encode_labels_window: max_obj = %d, image_size = %d, S = %d, num_class = %d", max_obj,
                    image_size, S, num_class);
    hipLaunchKernelGGL(encode_labels_window_kernel, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, boxes, counts,
                       table, index, params, max_obj, image_size, S, num_class, labels);
    return launched("y2_encode_labels_window");
}

}  // extern "C"
