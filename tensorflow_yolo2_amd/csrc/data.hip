// The input side of the detector on the device: a batch of uint8 BGR images resized from a pool of images kept at their
// native resolution, and the [S,S,5+C] label grids of the same batch from per-image object lists.  The specification is
// this repository's host code (img_dataset/pascal_voc.py: resize_bilinear_u8, encode_boxes, flip_label; restated in
// oracle/data_ref.py), and both kernels are bit-equal to it: the coefficients are computed in double in the
// specification's operation order, and the file is compiled with -ffp-contract=off (a fused multiply-add in
// (i + 0.5) * scale - 0.5 or in frac * 2048 can move a rounding tie).
// Here: the band loops of the plain resize and of the letterbox and what only they need (resize_bytes, fill_dwords,
// canvas_dword).  The coefficient and x-table arithmetic, the blend, the staging of source rows and the body of the label
// kernel are data_common.h's, shared with augment.hip.
#include "data_common.h"
#include "letterbox.h"
using namespace y2;

namespace {

// VEC consecutive output bytes starting at byte b of an output row: r0 / r1 are the two source rows (LDS or global)
template <int VEC>
Y2_DEV uint32_t resize_bytes(const uint8_t* r0, const uint8_t* r1, const XCoef* xt, int b, int wy1) {
    int x = b / 3, c = b - 3 * x;
    uint32_t packed = 0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const XCoef q = xt[x];
        const int a0 = q.x0 + c, a1 = a0 + q.dx;
        const int wx1 = q.w1;                   // read before the taps, not after them as an argument would be: measured,
        const int v = blend4(r0[a0], r0[a1], r1[a0], r1[a1], wx1, wy1);   // 1 % of the kernel at 320 and 416
        packed |= (uint32_t)(v & 255) << (8 * e);
        if (++c == 3) { c = 0; ++x; }
    }
    return packed;
}

// grid (ceil(out_h / kBand), n).  A workgroup owns kBand output rows of one image: the x coefficients of the image
// (mirrored when it is flipped) are computed once into LDS; for every kRows output rows the 2 * kRows source rows they
// blend are staged into LDS with 16-byte loads, and each lane produces VEC consecutive output bytes per store.
template <int VEC>
__global__ __launch_bounds__(kThreads) void resize_u8_kernel(const uint8_t* __restrict__ pool,
                                                             const int64_t* __restrict__ table,
                                                             const int32_t* __restrict__ index, int out_h, int out_w,
                                                             uint8_t* __restrict__ out) {
    __shared__ XCoef xt[kMaxOutW];
    __shared__ int yc[kBand][3];
    __shared__ __attribute__((aligned(16))) uint8_t rows[2 * kRows * kMaxPitch];
    const int tid = threadIdx.x, img = blockIdx.y;
    const int64_t* t = table + (size_t)kTable * (index ? index[img] : img);
    const int64_t off = t[0], pitch64 = t[3];
    const int H = (int)t[1], W = (int)t[2], flip = (int)t[4];
    const int band0 = blockIdx.x * kBand, nrows = min(kBand, out_h - band0);
    if (H < 1 || W < 1) return;                 // (an empty table row: nothing to read)
    build_xtable(xt, W, out_w, flip, tid);
    if (tid < nrows) lin_coef(band0 + tid, H, out_h, yc[tid][0], yc[tid][1], yc[tid][2]);
    __syncthreads();
    const bool staged = pitch64 <= kMaxPitch && stageable(off, pitch64, W);
    const int pitch = (int)pitch64;
    const uint8_t* src = pool + off;
    const int rowbytes = 3 * out_w;
    uint8_t* obase = out + ((size_t)img * out_h + band0) * rowbytes;
    for (int g0 = 0; g0 < nrows; g0 += kRows) {
        const int gr = min(kRows, nrows - g0);
        if (staged) {
            stage_rows(rows, src, pitch64, yc + g0, gr, tid);
            __syncthreads();
        }
        const int total = gr * rowbytes;
        for (int k = tid * VEC; k < total; k += kThreads * VEC) {
            const int j = k / rowbytes, b = k - j * rowbytes;
            const int* y = yc[g0 + j];
            uint32_t v;
            if (staged)
                v = resize_bytes<VEC>(rows + (2 * j) * pitch, rows + (2 * j + 1) * pitch, xt, b, y[2]);
            else
                v = resize_bytes<VEC>(src + (size_t)y[0] * pitch64, src + (size_t)y[1] * pitch64, xt, b, y[2]);
            uint8_t* o = obase + (size_t)g0 * rowbytes + k;
            if (VEC == 4) *(uint32_t*)o = v;
            else *o = (uint8_t)v;
        }
        if (staged) __syncthreads();
    }
}

// n4 dwords of `v` from the 4-byte aligned p by the whole workgroup: 16-byte stores between the unaligned ends
Y2_DEV void fill_dwords(uint8_t* p, int n4, uint32_t v, int tid) {
    const int head = min(n4, (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2));
    const int body = (n4 - head) >> 2;
    uint32_t* q = (uint32_t*)p;
    if (tid < head) q[tid] = v;
    u32x4* b = (u32x4*)(q + head);
    const u32x4 v4 = {v, v, v, v};
    for (int i = tid; i < body; i += kThreads) b[i] = v4;
    const int done = head + 4 * body;
    if (tid < n4 - done) q[done + tid] = v;     // fewer than 4 left
}

// the aligned dword at byte cb of a canvas row whose picture bytes are [lo, hi): r0 / r1 are the two source rows
Y2_DEV uint32_t canvas_dword(const uint8_t* r0, const uint8_t* r1, const XCoef* xt, int cb, int lo, int hi, int wy1,
                             uint32_t fill4) {
    if (cb >= lo && cb + 4 <= hi) return resize_bytes<4>(r0, r1, xt, cb - lo, wy1);
    uint32_t v = fill4;
    if (cb + 4 > lo && cb < hi) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int b = cb + e - lo;
            if (b >= 0 && b < hi - lo) v = (v & ~(255u << (8 * e))) | (resize_bytes<1>(r0, r1, xt, b, wy1) << (8 * e));
        }
    }
    return v;
}

// The letterboxed batch (img_dataset/pascal_voc.letterbox_u8): grid (ceil(size / kBand), n), resize_u8_kernel's band of
// kBand canvas rows per workgroup.  The geometry comes from letterbox.h; a band that lies wholly in the top or bottom
// bar (or whose table row is empty) is `fill` and nothing else: no coefficient, no source row.  Otherwise the band's bar
// rows are filled, and its picture rows go the way of the plain resize with new_w x new_h for the output size: the x
// table is built for new_w columns, the two source rows of an output row are staged, and a lane produces one aligned
// dword of the CANVAS row -- resize_bytes<4> where the dword lies in the picture, the fill where it lies in a side bar,
// byte by byte (resize_bytes<1>) for the at most two dwords of a row that straddle the picture's edge.  The flip column
// of the table is not read: evaluation uses unmirrored entries.
__global__ __launch_bounds__(kThreads) void letterbox_u8_kernel(const uint8_t* __restrict__ pool,
                                                                const int64_t* __restrict__ table,
                                                                const int32_t* __restrict__ index, int size, int fill,
                                                                uint8_t* __restrict__ out) {
    __shared__ XCoef xt[kMaxOutW];
    __shared__ int yc[kBand][3];
    __shared__ __attribute__((aligned(16))) uint8_t rows[2 * kRows * kMaxPitch];
    const int tid = threadIdx.x, img = blockIdx.y;
    const int64_t* t = table + (size_t)kTable * (index ? index[img] : img);
    const int64_t off = t[0], h64 = t[1], w64 = t[2], pitch64 = t[3];
    const int band0 = blockIdx.x * kBand, nrows = min(kBand, size - band0);
    const int rowbytes = 3 * size;
    const uint32_t fill4 = 0x01010101u * (uint32_t)fill;
    uint8_t* obase = out + ((size_t)img * size + band0) * rowbytes;
    const bool sized = h64 >= 1 && w64 >= 1 && h64 <= 0x7fffffff && w64 <= 0x7fffffff;
    const int H = sized ? (int)h64 : 1, W = sized ? (int)w64 : 1;
    const LetterboxGeom g = letterbox_geometry(W, H, size);
    // the picture's rows of this band, relative to band0: [p0, p1)
    const int p0 = sized ? min(max(g.oy - band0, 0), nrows) : nrows;
    const int p1 = sized ? min(max(g.oy + g.new_h - band0, p0), nrows) : nrows;
    fill_dwords(obase, p0 * (rowbytes >> 2), fill4, tid);
    fill_dwords(obase + (size_t)p1 * rowbytes, (nrows - p1) * (rowbytes >> 2), fill4, tid);
    if (p0 >= p1) return;                       // uniform: a pure fill
    build_xtable(xt, W, g.new_w, 0, tid);
    if (tid >= p0 && tid < p1) lin_coef(band0 + tid - g.oy, H, g.new_h, yc[tid][0], yc[tid][1], yc[tid][2]);
    __syncthreads();
    const bool staged = pitch64 <= kMaxPitch && stageable(off, pitch64, W);
    const int pitch = (int)pitch64;
    const uint8_t* src = pool + off;
    const int lo = 3 * g.ox, hi = lo + 3 * g.new_w;         // the picture's bytes of a canvas row: [lo, hi)
    for (int g0 = p0; g0 < p1; g0 += kRows) {
        const int gr = min(kRows, p1 - g0);
        if (staged) {
            stage_rows(rows, src, pitch64, yc + g0, gr, tid);
            __syncthreads();
        }
        const int total = gr * rowbytes;
        for (int k = tid * 4; k < total; k += kThreads * 4) {
            const int j = k / rowbytes, cb = k - j * rowbytes;
            const int* y = yc[g0 + j];
            uint32_t v;                            // two calls, so that the staged one reads LDS with LDS instructions
            if (staged) v = canvas_dword(rows + (2 * j) * pitch, rows + (2 * j + 1) * pitch, xt, cb, lo, hi, y[2], fill4);
            else v = canvas_dword(src + (size_t)y[0] * pitch64, src + (size_t)y[1] * pitch64, xt, cb, lo, hi, y[2], fill4);
            *(uint32_t*)(obase + (size_t)g0 * rowbytes + k) = v;
        }
        if (staged) __syncthreads();
    }
}

// pascal_voc.encode_boxes: the label grid of the plain path (data_common.h: encode_labels without a window)
__global__ __launch_bounds__(kThreads) void encode_labels_kernel(const double* __restrict__ boxes,
                                                                 const int32_t* __restrict__ counts,
                                                                 const int64_t* __restrict__ table,
                                                                 const int32_t* __restrict__ index, int max_obj,
                                                                 int image_size, int S, int num_class,
                                                                 float* __restrict__ labels) {
    encode_labels<false>(boxes, counts, table, index, nullptr, max_obj, image_size, S, num_class, labels);
}

}  // namespace

extern "C" {

int y2_resize_bilinear_u8_batch(const uint8_t* pool, const int64_t* table, const int32_t* index, int n, int out_h,
                                int out_w, uint8_t* out, void* stream) {
    if (!pool || !table || !out) return fail(Y2_ERR_ARG, "y2_resize_bilinear_u8_batch: null pointer");
    if (n < 1 || n > 65535) return fail(Y2_ERR_ARG, "y2_resize_bilinear_u8_batch: n = %d outside 1..65535", n);
    if (out_h < 1 || out_w < 1) return fail(Y2_ERR_ARG, "y2_resize_bilinear_u8_batch: output %d x %d", out_h, out_w);
    if (out_w > kMaxOutW)
        return fail(Y2_ERR_ARG, "y2_resize_bilinear_u8_batch: out_w = %d beyond Y2_RESIZE_MAX_OUT_W = %d", out_w, kMaxOutW);
    const dim3 grid((out_h + kBand - 1) / kBand, n);
    if (out_w % 4 == 0 && ((uintptr_t)out & 3) == 0)
        hipLaunchKernelGGL(resize_u8_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, pool, table, index, out_h,
                           out_w, out);
    else
        hipLaunchKernelGGL(resize_u8_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, pool, table, index, out_h,
                           out_w, out);
    return launched("y2_resize_bilinear_u8_batch");
}

int y2_letterbox_u8_batch(const uint8_t* pool, const int64_t* table, const int32_t* index, int n, int size, int fill,
                          uint8_t* out, void* stream) {
    if (!pool || !table || !out) return fail(Y2_ERR_ARG, "y2_letterbox_u8_batch: null pointer");
    if (n < 1 || n > 65535) return fail(Y2_ERR_ARG, "y2_letterbox_u8_batch: n = %d outside 1..65535", n);
    if (size < 4 || size % 4 || size > kMaxOutW)
        return fail(Y2_ERR_ARG, "y2_letterbox_u8_batch: size = %d is not a multiple of 4 in 4..Y2_RESIZE_MAX_OUT_W = %d",
                    size, kMaxOutW);
    if (fill < 0 || fill > 255) return fail(Y2_ERR_ARG, "y2_letterbox_u8_batch: fill = %d outside 0..255", fill);
    if ((uintptr_t)out & 3) return fail(Y2_ERR_ARG, "y2_letterbox_u8_batch: out is not 4-byte aligned");
    hipLaunchKernelGGL(letterbox_u8_kernel, dim3((size + kBand - 1) / kBand, n), dim3(kThreads), 0, (hipStream_t)stream,
                       pool, table, index, size, fill, out);
    return launched("y2_letterbox_u8_batch");
}

int y2_letterbox_geometry(int im_h, int im_w, int size, int* geometry) {
    if (!geometry) return fail(Y2_ERR_ARG, "y2_letterbox_geometry: null pointer");
    if (im_h < 1 || im_w < 1 || size < 1)
        return fail(Y2_ERR_ARG, "y2_letterbox_geometry: image %d x %d, size = %d", im_w, im_h, size);
    const LetterboxGeom g = letterbox_geometry(im_w, im_h, size);
    geometry[0] = g.new_w; geometry[1] = g.new_h; geometry[2] = g.ox; geometry[3] = g.oy;
    return Y2_OK;
}

int y2_encode_labels(const double* boxes, const int32_t* counts, const int64_t* table, const int32_t* index, int n,
                     int max_obj, int image_size, int S, int num_class, float* labels, void* stream) {
    if (!boxes || !counts || !table || !labels) return fail(Y2_ERR_ARG, "y2_encode_labels: null pointer");
    if (n < 1) return fail(Y2_ERR_ARG, "y2_encode_labels: n = %d", n);
    if (max_obj < 1 || image_size < 1 || S < 1 || num_class < 0 || S > 1024)
        return fail(Y2_ERR_ARG, "y2_encode_labels: max_obj = %d, image_size = %d, S = %d, num_class = %d", max_obj,
                    image_size, S, num_class);
    hipLaunchKernelGGL(encode_labels_kernel, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, boxes, counts, table,
                       index, max_obj, image_size, S, num_class, labels);
    return launched("y2_encode_labels");
}

}  // extern "C"
