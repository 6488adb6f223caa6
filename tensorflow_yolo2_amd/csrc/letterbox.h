// The geometry of a letterboxed input, ONE definition: the image kernel (data.hip: letterbox_u8_kernel), the inverse map
// of the two anchor detect kernels (detect.hip) and the host entry y2_letterbox_geometry all call it, so the boxes are
// un-mapped from exactly the rectangle the picture was embedded in.  Integer arithmetic only, as Darknet's
// letterbox_image; the Python restatement is img_dataset/pascal_voc.letterbox_geometry.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "common.h"

namespace y2 {

struct LetterboxGeom { int new_w, new_h, ox, oy; };   // the picture's rectangle in the n x n canvas: size, left / top bar

// im_w x im_h >= 1 x 1 pixels into a square of n >= 1: the longer side becomes n, the other keeps the aspect ratio
// (C integer division, at least 1), and the rectangle is centred with the odd pixel in the right / bottom bar.  The
// products are 64-bit: a table row may hold any height or width up to 2^31 - 1.
__host__ __device__ inline LetterboxGeom letterbox_geometry(int im_w, int im_h, int n) {
    LetterboxGeom g;
    if ((int64_t)n * im_h <= (int64_t)n * im_w) {
        const int64_t v = (int64_t)im_h * n / im_w;
        g.new_w = n;
        g.new_h = v < 1 ? 1 : (int)v;
    } else {
        const int64_t v = (int64_t)im_w * n / im_h;
        g.new_h = n;
        g.new_w = v < 1 ? 1 : (int)v;
    }
    g.ox = (n - g.new_w) / 2;
    g.oy = (n - g.new_h) / 2;
    return g;
}

// Where the input was letterboxed (net_size = 32 S; the anchor detect kernels of detect.hip and detect_tree.hip): the
// map from a box relative to the net_size canvas to the pixels of the original image, the exact inverse of the
// embedding, in the specification's operation order (utils/detect_batch.anchor_candidates with net_size).  Uniform over
// the workgroup: made once from the table row.
struct LetterboxMap { double n, ox, oy, sx, sy; };
Y2_DEV LetterboxMap letterbox_map(int im_w, int im_h, int net_size) {
    const LetterboxGeom g = letterbox_geometry(im_w, im_h, net_size);
    return LetterboxMap{(double)net_size, (double)g.ox, (double)g.oy, (double)im_w / (double)g.new_w,
                        (double)im_h / (double)g.new_h};
}

}  // namespace y2
