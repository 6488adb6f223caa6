// The two optimizer updates as ONE piece of device code shared by the flat kernels (optim.hip) and the fused
// update + re-pack kernel (pack.hip): with contraction pinned, both produce the same bits.
//   tf.train.AdamOptimizer (epsilon-hat form, src/pascal/pascal_train_darknet.py:51):
//       m <- b1 m + (1 - b1) g ;  v <- b2 v + (1 - b2) g g ;  var <- var - lr_t m / (sqrt(v) + eps)
//   tf.train.MomentumOptimizer (src/imagenet/imagenet_train_darknet.py:58):
//       accum <- momentum accum + g ;  var <- var - lr accum
//   Darknet's SGD (update_convolutional_layer; specification utils/solver.py sgd_step):
//       gd <- g + decay p  (convolution filters only) ;  accum <- momentum accum + gd ;  var <- var - lr_t accum
//   and its rate schedule (get_current_rate; utils/solver.py current_rate), shared by the host routine and the
//   one-thread schedule kernel: double arithmetic, powers as repeated products, so both give the same bits
#pragma once
#include "common.h"
#include "../../include/yolo2_hip.h"

namespace y2 {

Y2_DEV void adam_update(float& p, float& m, float& v, float g, float lr_t, float b1, float b2, float eps) {
#pragma clang fp contract(off)
    const float gm = (1.0f - b1) * g;
    const float gv = ((1.0f - b2) * g) * g;
    m = __builtin_fmaf(b1, m, gm);
    v = __builtin_fmaf(b2, v, gv);
    const float step = (lr_t * m) / (sqrtf(v) + eps);
    p = p - step;
}

Y2_DEV void momentum_update(float& p, float& acc, float g, float lr, float mom) {
#pragma clang fp contract(off)
    acc = __builtin_fmaf(mom, acc, g);
    const float step = lr * acc;
    p = p - step;
}

// decayed: per tensor (a wave-uniform branch), never a product with zero -- gd is g itself where it is false
Y2_DEV void sgd_update(float& p, float& acc, float g, float lr_t, float mom, float decay, bool decayed) {
#pragma clang fp contract(off)
    float gd = g;
    if (decayed) {
        const float d = decay * p;
        gd = gd + d;
    }
    acc = __builtin_fmaf(mom, acc, gd);
    const float step = lr_t * acc;
    p = p - step;
}

// null, or what is wrong with the record
__host__ __device__ inline const char* solver_invalid(const y2_sgd_solver& s) {
    const float inf = __builtin_huge_valf();
    if (!(s.learning_rate >= 0.f && s.learning_rate < inf)) return "learning_rate must be finite and >= 0";
    if (!(s.momentum >= 0.f && s.momentum < 1.f)) return "momentum must lie in [0, 1)";
    if (!(s.decay >= 0.f && s.decay < inf)) return "decay must be finite and >= 0";
    if (s.policy < Y2_POLICY_CONSTANT || s.policy > Y2_POLICY_POLY) return "policy must be constant, steps or poly";
    if (s.burn_in < 0) return "burn_in must be >= 0";
    if (s.power < 1 || s.power > 8) return "power must lie in 1..8";
    if (s.nsteps < 0 || s.nsteps > Y2_SOLVER_MAX_STEPS) return "at most 8 steps";
    for (int i = 0; i < s.nsteps; ++i) {
        if (s.steps[i] < 1 || (i > 0 && s.steps[i] <= s.steps[i - 1])) return "steps must be >= 1 and strictly ascending";
        if (!(s.scales[i] > 0.f && s.scales[i] < inf)) return "scales must be finite and > 0";
    }
    if (s.policy == Y2_POLICY_POLY && s.max_batches < 1) return "the poly policy needs max_batches >= 1";
    return nullptr;
}

// rate of applied step t >= 1 of a valid record
__host__ __device__ inline float solver_rate(const y2_sgd_solver& s, int t) {
#pragma clang fp contract(off)
    const double lr = (double)s.learning_rate;
    double x, r;
    if (t < s.burn_in) {
        x = (double)t / (double)s.burn_in;
    } else if (s.policy == Y2_POLICY_POLY) {
        x = 1.0 - (double)t / (double)s.max_batches;
        if (!(x > 0.0)) x = 0.0;
    } else {
        r = lr;
        if (s.policy == Y2_POLICY_STEPS)
            for (int i = 0; i < s.nsteps && s.steps[i] <= t; ++i) r = r * (double)s.scales[i];
        return (float)r;
    }
    r = x;
    for (int k = 1; k < s.power; ++k) r = r * x;
    return (float)(lr * r);
}

}  // namespace y2
