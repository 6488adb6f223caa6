// What the two bit-equal input paths share (data.hip: plain resize; augment.hip: window + colour): the launch geometry,
// the x-coefficient record and the coefficient arithmetic.  One definition, so that the identity window cannot drift
// from the plain resize.
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

namespace {

constexpr int kThreads = 256;
constexpr int kMaxOutW = Y2_RESIZE_MAX_OUT_W;   // columns of the x-coefficient table in LDS
constexpr int kBand = 16;                       // output rows of one workgroup
constexpr int kRows = 4;                        // output rows produced from one staging of source rows
constexpr int kMaxPitch = 4096;                 // widest source row (bytes) that is staged in LDS; wider rows are read in place
constexpr int kTable = 5;                       // int64 per image: byte offset, height, width, row pitch, flip

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

}  // namespace
