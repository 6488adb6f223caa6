// The arithmetic of the YOLOv2 anchor decode, shared by decode_anchors_kernel (ext.hip) and detect_anchor_kernel
// (detect.hip).  One definition: both files are compiled with -ffp-contract=off, so the fused detect kernel forms the
// same float32 values as y2_decode_anchors followed by y2_class_argmax, bit for bit.
//   p = one (cell, anchor) row of the head: tx, ty, tw, th, to, class logits [C]
//   bx = (sigmoid(tx) + col) / S, by = (sigmoid(ty) + row) / S, bw = pw * exp(tw) / S, bh = ph * exp(th) / S
//   score[c] = sigmoid(to) * softmax(class logits)[c]
#pragma once
#include "common.h"

namespace y2 {

struct AnchorBox {
    float cx, cy, w, h;   // relative to the image
    float so;             // sigmoid(to)
};

Y2_DEV AnchorBox anchor_decode_box(const float* __restrict__ p, const float* __restrict__ anchors, int b, int row,
                                   int col, int S) {
    const float sx = 1.f / (1.f + expf(-p[0])), sy = 1.f / (1.f + expf(-p[1]));
    const float so = 1.f / (1.f + expf(-p[4]));
    const float fs = (float)S;
    AnchorBox r;
    r.cx = (sx + (float)col) / fs;
    r.cy = (sy + (float)row) / fs;
    r.w = anchors[2 * b] * expf(p[2]) / fs;
    r.h = anchors[2 * b + 1] * expf(p[3]) / fs;
    r.so = so;
    return r;
}

// the softmax's shift and denominator over the C class logits at p[5 ..]
Y2_DEV void anchor_softmax_norm(const float* __restrict__ p, int C, float& mx, float& sum) {
    mx = p[5];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[5 + c]);
    sum = 0.f;
    for (int c = 0; c < C; ++c) sum += expf(p[5 + c] - mx);
}

Y2_DEV float anchor_class_score(const float* __restrict__ p, int c, float so, float mx, float sum) {
    return so * (expf(p[5 + c] - mx) / sum);
}

}  // namespace y2
