// Classifier scoring on the device (utils/score_views.py is the float64 specification): per image the softmax of every
// view, the mean over the views, the k best classes, the rank of the label and the running counters -- one launch, no
// host read.  Darknet's validate_classifier_single / _10 (average the predictions of the views, then top-1 / top-k).
//
// One workgroup of 256 lanes per image.  Every reduction is a wave butterfly plus one LDS step over the four waves in a
// fixed order, so the result of a reduction depends on (classes, lane) alone: two calls on the same logits return the
// same bits.  There is no floating-point atomic; the counters are integer atomics, at most one per field and workgroup.
// The file is compiled with -ffp-contract=off: p[c] is the same chain of float32 operations for the label (formed first,
// in every lane) and in the sweep, and depends on c only through the logits read.
#include "data_common.h"
using namespace y2;

namespace {

constexpr int kScoreThreads = 256;
constexpr int kScoreWaves = kScoreThreads / 64;
constexpr int kMaxViews = 16;
constexpr int kMaxK = 8;
constexpr int kNone = 0x7fffffff;               // the class index of an empty slot: after every class in the order
constexpr size_t kScoreLds = 48 * 1024;         // an image's logits (views * classes * 4 bytes) that may be staged

// the order of the scores: larger first, equal scores by the lower class index
Y2_DEV bool before(float s, int i, float t, int j) { return s > t || (s == t && i < j); }

// p[c] = (1 / V) sum_v exp(x_v[c] - max_v) / sum_v, the views added in order
Y2_DEV float mean_prob(const float* x, int classes, int views, const float* vmax, const float* vsum, float inv_views,
                       int c) {
    float acc = 0.0f;
    for (int v = 0; v < views; ++v) acc += expf(x[(size_t)v * classes + c] - vmax[v]) / vsum[v];
    return acc * inv_views;
}

// grid (n), 256 lanes.  STAGED (the image's logits fit kScoreLds): the pass that takes the maxima copies them to LDS and the
// two later passes read them there; else every pass reads them from global memory (L2 after the first).
template <bool STAGED>
__global__ __launch_bounds__(kScoreThreads) void score_views_kernel(const float* __restrict__ logits,
                                                                    const int32_t* __restrict__ labels, int views,
                                                                    int classes, int k, int n_valid,
                                                                    float* __restrict__ prob,
                                                                    int32_t* __restrict__ top_idx,
                                                                    float* __restrict__ top_val,
                                                                    int32_t* __restrict__ rank,
                                                                    int32_t* __restrict__ hits) {
    extern __shared__ float staged[];
    __shared__ float red[kMaxViews][kScoreWaves];
    __shared__ float vmax[kMaxViews], vsum[kMaxViews];
    __shared__ float wscore[2][kScoreWaves];
    __shared__ int widx[2][kScoreWaves];
    __shared__ int wcount[kScoreWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const float* g = logits + b * (size_t)views * classes;

    // ---- the maximum of every view
    for (int v = 0; v < views; ++v) {
        float m = -INFINITY;
        for (int c = tid; c < classes; c += kScoreThreads) {
            const float xv = g[(size_t)v * classes + c];
            if (STAGED) staged[v * classes + c] = xv;
            m = fmaxf(m, xv);
        }
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        if (lane == 0) red[v][wave] = m;
    }
    __syncthreads();
    if (tid < views) vmax[tid] = fmaxf(fmaxf(red[tid][0], red[tid][1]), fmaxf(red[tid][2], red[tid][3]));
    __syncthreads();
    const float* x = STAGED ? staged : g;

    // ---- the sum of every view: a lane adds its classes in ascending order, then the butterfly, then wave 0 .. 3
    for (int v = 0; v < views; ++v) {
        const float m = vmax[v];
        float s = 0.0f;
        for (int c = tid; c < classes; c += kScoreThreads) s += expf(x[(size_t)v * classes + c] - m);
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) red[v][wave] = s;
    }
    __syncthreads();
    if (tid < views) vsum[tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
    __syncthreads();

    // ---- the label's score, in every lane; a label outside the classes forms no address
    const float inv_views = 1.0f / (float)views;
    const int lab = labels ? labels[b] : -1;
    const bool lab_ok = labels && (unsigned)lab < (unsigned)classes;
    float lab_score = 0.0f;
    if (lab_ok) lab_score = views == 1 ? x[lab] : mean_prob(x, classes, views, vmax, vsum, inv_views, lab);

    // ---- one sweep: p[c], the classes ordered before the label, the lane's own best kMaxK (score, p, class)
    float bs[kMaxK], bp[kMaxK];
    int bi[kMaxK];
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) { bs[j] = -INFINITY; bp[j] = 0.0f; bi[j] = kNone; }
    int ahead = 0;
    for (int c = tid; c < classes; c += kScoreThreads) {
        float cp = mean_prob(x, classes, views, vmax, vsum, inv_views, c);
        float cs = views == 1 ? x[c] : cp;
        int ci = c;
        if (prob) prob[b * (size_t)classes + c] = cp;
        if (lab_ok && before(cs, ci, lab_score, lab)) ++ahead;
#pragma unroll
        for (int j = 0; j < kMaxK; ++j) {       // the displaced entry moves on down the list
            if (before(cs, ci, bs[j], bi[j])) {
                const float ts = bs[j], tp = bp[j];
                const int ti = bi[j];
                bs[j] = cs; bp[j] = cp; bi[j] = ci;
                cs = ts; cp = tp; ci = ti;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) ahead += __shfl_xor(ahead, off, 64);
    if (lane == 0) wcount[wave] = ahead;

    // ---- k rounds of a block-wide arg-max over the lanes' heads; the lane that owns the winner writes it and moves up
    for (int j = 0; j < k; ++j) {
        float hs = bs[0];
        int hi = bi[0];
        for (int off = 32; off > 0; off >>= 1) {
            const float os = __shfl_xor(hs, off, 64);
            const int oi = __shfl_xor(hi, off, 64);
            if (before(os, oi, hs, hi)) { hs = os; hi = oi; }
        }
        if (lane == 0) { wscore[j & 1][wave] = hs; widx[j & 1][wave] = hi; }
        __syncthreads();
        float ws = wscore[j & 1][0];
        int wi = widx[j & 1][0];
#pragma unroll
        for (int w = 1; w < kScoreWaves; ++w)
            if (before(wscore[j & 1][w], widx[j & 1][w], ws, wi)) { ws = wscore[j & 1][w]; wi = widx[j & 1][w]; }
        if (wi == kNone) {                      // fewer classes than k (or scores that are no numbers): the padding
            if (tid == 0) { top_idx[b * (size_t)k + j] = -1; top_val[b * (size_t)k + j] = 0.0f; }
        } else if (bi[0] == wi) {
            top_idx[b * (size_t)k + j] = wi;
            top_val[b * (size_t)k + j] = bp[0];
#pragma unroll
            for (int q = 0; q + 1 < kMaxK; ++q) { bs[q] = bs[q + 1]; bp[q] = bp[q + 1]; bi[q] = bi[q + 1]; }
            bs[kMaxK - 1] = -INFINITY; bp[kMaxK - 1] = 0.0f; bi[kMaxK - 1] = kNone;
        }
    }

    // ---- rank and counters (wcount was written before the first round's barrier; k >= 1)
    if (tid == 0 && labels) {
        const int r = lab_ok ? ((wcount[0] + wcount[1]) + wcount[2]) + wcount[3] : classes;
        if (rank) rank[b] = r;
        if (hits && b < (size_t)n_valid) {
            atomicAdd(hits + 0, 1);
            if (r == 0) atomicAdd(hits + 1, 1);
            if (lab_ok && r < k) atomicAdd(hits + 2, 1);       // (classes < k: a label outside them is still a miss)
            if (!lab_ok) atomicAdd(hits + 3, 1);
        }
    }
}

}  // namespace

extern "C" {

int y2_score_views(const float* logits, const int32_t* labels, int n, int views, int classes, int k, int n_valid,
                   float* prob, int32_t* top_idx, float* top_val, int32_t* rank, int32_t* hits, void* stream) {
    if (!logits || !top_idx || !top_val) return fail(Y2_ERR_ARG, "y2_score_views: null pointer");
    if (n < 1) return fail(Y2_ERR_ARG, "y2_score_views: n = %d", n);
    if (views < 1 || views > kMaxViews) return fail(Y2_ERR_ARG, "y2_score_views: views = %d outside 1..%d", views, kMaxViews);
    if (classes < 1) return fail(Y2_ERR_ARG, "y2_score_views: classes = %d", classes);
    if (k < 1 || k > kMaxK) return fail(Y2_ERR_ARG, "y2_score_views: k = %d outside 1..%d", k, kMaxK);
    if (n_valid < 0 || n_valid > n) return fail(Y2_ERR_ARG, "y2_score_views: n_valid = %d outside 0..%d", n_valid, n);
    if (!labels && (rank || hits)) return fail(Y2_ERR_ARG, "y2_score_views: rank and hits need labels");
    // measured (scripts/bench_score_views.py, profiles/score_views.txt): staging an image's logits in LDS beats re-reading
    // them from L2 in the two later passes, so they are staged wherever they fit; Y2_SCORE_NO_STAGE=1 is the A/B switch
    const size_t bytes = (size_t)views * classes * sizeof(float);
    if (bytes <= kScoreLds && !getenv("Y2_SCORE_NO_STAGE"))
        hipLaunchKernelGGL(score_views_kernel<true>, dim3(n), dim3(kScoreThreads), bytes, (hipStream_t)stream, logits,
                           labels, views, classes, k, n_valid, prob, top_idx, top_val, rank, hits);
    else
        hipLaunchKernelGGL(score_views_kernel<false>, dim3(n), dim3(kScoreThreads), 0, (hipStream_t)stream, logits, labels,
                           views, classes, k, n_valid, prob, top_idx, top_val, rank, hits);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(Y2_ERR_HIP, "y2_score_views: %s", hipGetErrorString(e));
    return Y2_OK;
}

}  // extern "C"
