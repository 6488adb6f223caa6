"""Darknet's SGD solver for the YOLOv2 anchor model -- the specification (numpy, host only) that the device code
(csrc/optim_math.h sgd_update / solver_rate, the flat kernel of csrc/optim.hip, KIND 2 of csrc/pack.hip's fused update +
re-pack) is held to.  This is the project's own restatement of Darknet's `get_current_rate` and
`update_convolutional_layer`; the reference repository trains its grid model with Adam and has no counterpart.

    Solver          the record: Darknet's cfg keys learning_rate, momentum, decay, policy, burn_in, power, steps, scales,
                    max_batches, with yolov2-voc.cfg's values as defaults
    current_rate    the rate of applied step t >= 1 (Darknet's batch_num is 1 at the first update)
    sgd_step        the float32 update of one element (or of arrays, elementwise)

Stated departures from Darknet: the schedule is computed in float64 on the float32 record with powers as repeated
products (Darknet: float and powf), so that host and device agree bit for bit by IEEE rules alone -- the difference is
a few float32 ulps of the rate; and under the overflow guard of the half-precision modes a skipped step does not count
(Darknet has no skipped steps)."""
import numpy as np

POLICIES = ("constant", "steps", "poly")
MAX_STEPS = 8
FIELDS = ("learning_rate", "momentum", "decay", "policy", "burn_in", "power", "steps", "scales", "max_batches")


class Solver:
    """A plain record.  validate() raises ValueError naming the field."""

    def __init__(self, learning_rate=0.001, momentum=0.9, decay=0.0005, policy="steps", burn_in=1000, power=4,
                 steps=(40000, 60000), scales=(0.1, 0.1), max_batches=0):
        self.learning_rate, self.momentum, self.decay = learning_rate, momentum, decay
        self.policy, self.burn_in, self.power = policy, burn_in, power
        self.steps, self.scales, self.max_batches = tuple(steps), tuple(scales), max_batches
        self.validate()

    def validate(self):
        def whole(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if not (np.isfinite(self.learning_rate) and self.learning_rate >= 0):
            raise ValueError("learning_rate %r: must be finite and >= 0" % (self.learning_rate,))
        if not 0 <= self.momentum < 1:
            raise ValueError("momentum %r: must lie in [0, 1)" % (self.momentum,))
        if not (np.isfinite(self.decay) and self.decay >= 0):
            raise ValueError("decay %r: must be finite and >= 0" % (self.decay,))
        if self.policy not in POLICIES:
            raise ValueError("policy %r: one of %s" % (self.policy, ", ".join(POLICIES)))
        if not whole(self.burn_in) or self.burn_in < 0:
            raise ValueError("burn_in %r: must be an integer >= 0" % (self.burn_in,))
        if not whole(self.power) or not 1 <= self.power <= 8:
            raise ValueError("power %r: must be an integer in 1..8" % (self.power,))
        if len(self.steps) > MAX_STEPS:
            raise ValueError("steps %r: at most %d" % (self.steps, MAX_STEPS))
        if any(not whole(s) or s < 1 for s in self.steps) or any(b <= a for a, b in zip(self.steps, self.steps[1:])):
            raise ValueError("steps %r: integers >= 1, strictly ascending" % (self.steps,))
        if len(self.scales) != len(self.steps):
            raise ValueError("scales %r: one per step (%d steps)" % (self.scales, len(self.steps)))
        if any(not (np.isfinite(s) and s > 0) for s in self.scales):
            raise ValueError("scales %r: each finite and > 0" % (self.scales,))
        if not whole(self.max_batches) or self.max_batches < 0:
            raise ValueError("max_batches %r: must be an integer >= 0" % (self.max_batches,))
        if self.policy == "poly" and self.max_batches < 1:
            raise ValueError("max_batches %r: the poly policy needs max_batches >= 1" % (self.max_batches,))
        return self

    def as_dict(self):
        """every field as the C ABI carries it: float32 rates, integers, the policy's name"""
        return {"learning_rate": np.float32(self.learning_rate), "momentum": np.float32(self.momentum),
                "decay": np.float32(self.decay), "policy": str(self.policy), "burn_in": int(self.burn_in),
                "power": int(self.power), "steps": tuple(int(s) for s in self.steps),
                "scales": tuple(np.float32(s) for s in self.scales), "max_batches": int(self.max_batches)}

    def __eq__(self, other):
        return isinstance(other, Solver) and self.as_dict() == other.as_dict()

    def __repr__(self):
        return "Solver(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in FIELDS)


def _ipow(x, power):
    """x^power as power - 1 products, left to right (not pow: IEEE fixes every bit)"""
    r = x
    for _ in range(power - 1):
        r = r * x
    return r


def current_rate(solver, t):
    """float32 rate of applied step t >= 1.  float64 arithmetic on the float32 values of learning_rate and scales
    widened (as the C ABI passes them), one cast at the end.
        t < burn_in:  lr (t / burn_in)^power
        constant:     lr
        steps:        lr times scales[i] of every steps[i] <= t (in order; stops at the first steps[i] > t)
        poly:         lr max(0, 1 - t / max_batches)^power"""
    t = int(t)
    if t < 1:
        raise ValueError("current_rate: t %d, the first applied step is 1" % t)
    lr = np.float64(np.float32(solver.learning_rate))
    if t < solver.burn_in:
        return np.float32(lr * _ipow(np.float64(t) / np.float64(solver.burn_in), solver.power))
    if solver.policy == "constant":
        return np.float32(lr)
    if solver.policy == "steps":
        r = lr
        for step, scale in zip(solver.steps, solver.scales):
            if step > t:
                break
            r = r * np.float64(np.float32(scale))
        return np.float32(r)
    x = max(np.float64(0.0), np.float64(1.0) - np.float64(t) / np.float64(solver.max_batches))
    return np.float32(lr * _ipow(x, solver.power))


def sgd_step(p, acc, g, lr_t, momentum, decay, decayed, dtype=np.float32):
    """One float32 update -> (p, acc).  Scalars or arrays; `decayed` a bool or a bool array of p's shape.

        gd  = g                    g already times grad_mult (1 / world), as the other optimizers take it
        gd  = gd + decay * p       only where `decayed`: two roundings (the product, then the sum); elsewhere gd is g
        acc = fma(momentum, acc, gd)
        p   = p - lr_t * acc       the product rounded, then the difference

    `decayed` is true for every convolution filter W (the 3-channel first one and the 1x1 output convolution
    included) and for nothing else: not b, gamma or beta.  In exact arithmetic this is Darknet's three calls
    (wu -= decay batch w; w += lr / batch wu; wu *= momentum) with acc = -wu / batch before the scal.  This
    repository's losses are already means over the batch: lr_t times the mean gradient here is Darknet's
    learning_rate / batch times its summed gradient, so the cfg's learning_rate is the rate to give.  grad_mult
    multiplies g only, never the decay term.
    numpy has no fused multiply-add: the fma is the float64 product (exact for float32 factors) and sum rounded to
    float64, then to float32, which may double-round -- at most 1 float32 ulp from the device's single rounding.
    dtype=np.float64 runs the same formula in float64 (the algebra, without the float32 roundings)."""
    f = dtype
    p, acc, g = np.asarray(p, f), np.asarray(acc, f), np.asarray(g, f)
    d = (f(decay) * p).astype(f)
    gd = np.where(decayed, (g + d).astype(f), g).astype(f)
    acc = (np.float64(f(momentum)) * acc.astype(np.float64) + gd.astype(np.float64)).astype(f)
    step = (f(lr_t) * acc).astype(f)
    return (p - step).astype(f), acc


def network_decayed(network):
    """bool mask over a Network's flat parameter buffer: True on every filter W"""
    mask = np.zeros(network.n_params, bool)
    for l in range(network.num_layers):
        o = network._offsets[l]
        mask[o[0]:o[1]] = True
    return mask
