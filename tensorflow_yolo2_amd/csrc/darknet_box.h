// Darknet's boxes at test time, shared by the two kernels that form its rows (darknet_io.hip: one segment per class;
// detect_tree.hip: one class per candidate): the float un-map of correct_region_boxes, the float centre-box IoU of its
// NMS and the float corners of a row.  One definition of each, moved here verbatim from darknet_io.hip; both files are
// compiled with -ffp-contract=off.  The specification is utils/detect_batch: darknet_unmap, box_iou_darknet,
// darknet_corners.
#pragma once
#include "common.h"
#include "letterbox.h"

namespace y2 {

// Darknet's correct_region_boxes for a letterboxed input of n x n: uniform over the workgroup, made once from the table
// row.  off = (n - new) / 2. / n and sc = (double)((float)new / (float)n) act on the centre in double; r = (float)n /
// (float)new on the extent in float; then everything is taken to pixels by the float image size.
struct DarknetMap { double offx, offy, scx, scy; float rw, rh, fw, fh; };
Y2_DEV DarknetMap darknet_map(int im_w, int im_h, int n) {
    const LetterboxGeom g = letterbox_geometry(im_w, im_h, n);
    DarknetMap m;
    m.offx = (double)(n - g.new_w) / 2.0 / (double)n;
    m.offy = (double)(n - g.new_h) / 2.0 / (double)n;
    m.scx = (double)((float)g.new_w / (float)n);
    m.scy = (double)((float)g.new_h / (float)n);
    m.rw = (float)n / (float)g.new_w;
    m.rh = (float)n / (float)g.new_h;
    m.fw = (float)im_w;
    m.fh = (float)im_h;
    return m;
}

// Darknet's box_iou on centre boxes, all float32; NaN (a zero union, an overflow) compares false where it is used
Y2_DEV float dk_overlap(float x1, float w1, float x2, float w2) {
    return fminf(x1 + w1 / 2.0f, x2 + w2 / 2.0f) - fmaxf(x1 - w1 / 2.0f, x2 - w2 / 2.0f);
}
Y2_DEV float iou_darknet(float ax, float ay, float aw, float ah, float bx, float by, float bw, float bh) {
    const float ow = dk_overlap(ax, aw, bx, bw), oh = dk_overlap(ay, ah, by, bh);
    const float inter = (ow < 0.0f || oh < 0.0f) ? 0.0f : ow * oh;
    const float uni = (aw * ah + bw * bh) - inter;
    return inter / uni;
}

// one corner of a row: float(double(centre) -/+ double(extent) / 2.0 + 1.0)
Y2_DEV float dk_corner(float c, float ext, double sign) {
    return (float)((double)c + sign * ((double)ext / 2.0) + 1.0);
}

}  // namespace y2
