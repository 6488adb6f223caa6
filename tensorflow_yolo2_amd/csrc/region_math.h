// The scalar arithmetic the region-layer kernels share (ext.hip: the flat losses and statistics; word_tree.hip: the
// word-tree ones).  Both files are compiled with -ffp-contract=off, so one expression gives one result in either.
#pragma once
#include "common.h"

namespace y2 {

Y2_DEV float v2_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
Y2_DEV float v2_iou(float ax, float ay, float aw, float ah, float bx, float by, float bw, float bh) {
    const float iw = fmaxf(0.0f, fminf(ax + aw / 2, bx + bw / 2) - fmaxf(ax - aw / 2, bx - bw / 2));
    const float ih = fmaxf(0.0f, fminf(ay + ah / 2, by + bh / 2) - fmaxf(ay - ah / 2, by - bh / 2));
    const float inter = iw * ih;
    const float uni = aw * ah + bw * bh - inter;
    return uni > 0.0f ? inter / uni : 0.0f;
}

// the region statistics' partial sums: components 0..3 are float bit patterns, 4..7 integers
__device__ __forceinline__ int v2_stats_add(int k, int a, int b) {
    return k < 4 ? __float_as_int(__int_as_float(a) + __int_as_float(b)) : a + b;
}

}  // namespace y2
