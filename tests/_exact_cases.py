"""Exact-arithmetic cases of the 16-bit convolution and weight-gradient kernel forms (test_gpu_exact_forms.py on the
device, test_exact_cases_host.py on the host).

Data: x, W, bias and dy are integers from fixed seeds, entries in {-1, 0, +1}, with a nonzero density of
min(0.5, sqrt(1000 / K)) per operand (bias: the three values equally likely), K = the contraction length (taps * Cin
forward, taps * Cout dgrad; the filter sits in both contractions and takes the longer one).  Every product and every partial sum is then an exact fp32 integer
whatever the order of the sum -- K chunks, split-K slabs, float atomics and K-split scratch included -- and every
stored result is representable in f16 (integers to 2048) and bf16 (integers to 256) as long as the magnitudes stay
below those bounds: check_magnitudes() asserts that from the float64 reference alone, before any device value is read.

Reference: float64 torch (one matmul per tap on zero-padded tensors), on whatever device its inputs live -- never a
project kernel.  Integers: the float64 sums are exact too, so device and reference must agree in every bit.

Form keys: what the library's launch log records (include/yolo2_hip.h y2_launch_log_*, csrc/kernels.h).  Each case pins
the keys of its three launches, so a policy change that moves a case off its form fails instead of silently
uncovering the form.  The table is a greedy cover of the keys plan_conv / plan_wgrad return for 16-bit launches through
engine.conv2d / conv2d_backward, each case at about the smallest shape that selects its forms."""
import numpy as np
import torch

# csrc/kernels.h: ConvKind, WgradKind, WgradSum
CK_RF, CK_RFN, CK_HALOQ, CK_HALOQ_KS, CK_HALO, CK_IGEMM, CK_IGEMM_KS = range(7)
WK_NONE, WK_TAP, WK_NINE, WK_RING = range(4)
WS_DIRECT, WS_REDUCE1, WS_REDUCE16, WS_ATOMIC = range(4)
EPI_PLAIN, EPI_STATS, EPI_BNBWD = range(3)
CK_NAMES = ("rf", "rfn", "haloq", "haloq_ks", "halo", "igemm", "igemm_ks")
WK_NAMES = ("none", "tap", "nine", "ring")
WS_NAMES = ("direct", "reduce1", "reduce16", "atomic")
EPI_NAMES = ("plain", "stats", "bnbwd")
LAUNCH_DTYPE = {"f16": 1, "bf16": 2}
# largest integer magnitude up to which EVERY integer is representable in the storage type
STORE_MAX = {"f16": 2048, "bf16": 256}

# (name, N, H, W, Cin, Cout, k, seed,
#  forward (kind, cfg, K split), dgrad (kind, cfg, K split), wgrad (kind, tile, splitk > 1, sum route))
# Channel counts that the op-level entries pad (96 -> 128, Cout 30 / 125 / 425 -> 32 / 128 / 448) also take the
# non-direct dW copy.  The comments give the split depths the plan chose (not part of the key).
CASES = [
    ("1x1_32to30_n1_5x5", 1, 5, 5, 32, 30, 1, 1000,
     (CK_IGEMM, 0x211214, 0), (CK_IGEMM, 0x211214, 0), (WK_TAP, 0x449249, 0, WS_DIRECT)),   # splitk 1
    ("1x1_32to64_n1_5x5", 1, 5, 5, 32, 64, 1, 1001,
     (CK_IGEMM, 0x212214, 0), (CK_IGEMM, 0x221214, 0), (WK_TAP, 0x449251, 0, WS_DIRECT)),   # splitk 1
    ("1x1_32to125_n1_5x5", 1, 5, 5, 32, 125, 1, 1002,
     (CK_IGEMM, 0x211242, 0), (CK_IGEMM, 0x221214, 0), (WK_TAP, 0x449261, 0, WS_DIRECT)),   # splitk 1
    ("1x1_64to30_n1_5x5", 1, 5, 5, 64, 30, 1, 1003,
     (CK_IGEMM, 0x221214, 0), (CK_IGEMM, 0x212214, 0), (WK_TAP, 0x44924a, 0, WS_DIRECT)),   # splitk 1
    ("1x1_64to64_n1_5x5", 1, 5, 5, 64, 64, 1, 1004,
     (CK_IGEMM, 0x222214, 0), (CK_IGEMM, 0x222214, 0), (WK_TAP, 0x449252, 0, WS_DIRECT)),   # splitk 1
    ("1x1_64to125_n1_5x5", 1, 5, 5, 64, 125, 1, 1005,
     (CK_IGEMM, 0x321242, 0), (CK_IGEMM, 0x222214, 0), (WK_TAP, 0x449452, 0, WS_DIRECT)),   # splitk 1
    ("1x1_96to30_n1_5x5", 1, 5, 5, 96, 30, 1, 1006,
     (CK_IGEMM, 0x221214, 0), (CK_IGEMM, 0x211242, 0), (WK_TAP, 0x44924c, 0, WS_DIRECT)),   # splitk 1
    ("1x1_96to64_n1_5x5", 1, 5, 5, 96, 64, 1, 1007,
     (CK_IGEMM, 0x222214, 0), (CK_IGEMM, 0x321242, 0), (WK_TAP, 0x449292, 0, WS_DIRECT)),   # splitk 1
    ("1x1_96to256_n1_5x5", 1, 5, 5, 96, 256, 1, 1008,
     (CK_IGEMM, 0x321242, 0), (CK_IGEMM_KS, 0x221242, 1), (WK_TAP, 0x449492, 0, WS_DIRECT)),   # dgrad K split 2 deep, splitk 1
    ("1x1_1024to425_n1_5x5", 1, 5, 5, 1024, 425, 1, 1009,
     (CK_IGEMM_KS, 0x221242, 1), (CK_IGEMM_KS, 0x221242, 1), (WK_TAP, 0x449492, 0, WS_DIRECT)),   # forward K split 8 deep, dgrad 3 deep (of 7 chunks), splitk 1
    ("1x1_32to30_n8_7x7", 8, 7, 7, 32, 30, 1, 1010,
     (CK_IGEMM, 0x211214, 0), (CK_IGEMM, 0x211214, 0), (WK_TAP, 0x449249, 1, WS_REDUCE1)),   # splitk 2
    ("1x1_32to64_n8_7x7", 8, 7, 7, 32, 64, 1, 1011,
     (CK_IGEMM, 0x212214, 0), (CK_IGEMM, 0x221214, 0), (WK_TAP, 0x449251, 1, WS_REDUCE1)),   # splitk 2
    ("1x1_32to125_n8_7x7", 8, 7, 7, 32, 125, 1, 1012,
     (CK_IGEMM, 0x211242, 0), (CK_IGEMM, 0x221214, 0), (WK_TAP, 0x449261, 1, WS_REDUCE1)),   # splitk 2
    ("1x1_64to30_n8_7x7", 8, 7, 7, 64, 30, 1, 1013,
     (CK_IGEMM, 0x221214, 0), (CK_IGEMM, 0x212214, 0), (WK_TAP, 0x44924a, 1, WS_REDUCE1)),   # splitk 2
    ("1x1_64to64_n8_7x7", 8, 7, 7, 64, 64, 1, 1014,
     (CK_IGEMM, 0x222214, 0), (CK_IGEMM, 0x222214, 0), (WK_TAP, 0x449252, 1, WS_REDUCE1)),   # splitk 2
    ("1x1_64to125_n8_7x7", 8, 7, 7, 64, 125, 1, 1015,
     (CK_IGEMM, 0x321242, 0), (CK_IGEMM, 0x222214, 0), (WK_TAP, 0x449452, 1, WS_REDUCE1)),   # splitk 2
    ("1x1_96to30_n8_7x7", 8, 7, 7, 96, 30, 1, 1016,
     (CK_IGEMM, 0x221214, 0), (CK_IGEMM, 0x211242, 0), (WK_TAP, 0x44924c, 1, WS_REDUCE1)),   # splitk 2
    ("1x1_96to64_n8_7x7", 8, 7, 7, 96, 64, 1, 1017,
     (CK_IGEMM, 0x222214, 0), (CK_IGEMM, 0x321242, 0), (WK_TAP, 0x449292, 1, WS_REDUCE1)),   # splitk 2
    ("1x1_512to125_n8_7x7", 8, 7, 7, 512, 125, 1, 1018,
     (CK_IGEMM_KS, 0x221242, 1), (CK_IGEMM, 0x321242, 0), (WK_TAP, 0x449492, 1, WS_REDUCE1)),   # forward K split 4 deep, splitk 2
    ("1x1_32to30_n64_7x7", 64, 7, 7, 32, 30, 1, 1019,
     (CK_IGEMM, 0x211214, 0), (CK_IGEMM, 0x211214, 0), (WK_TAP, 0x449249, 1, WS_REDUCE16)),   # splitk 9
    ("1x1_32to64_n64_7x7", 64, 7, 7, 32, 64, 1, 1020,
     (CK_IGEMM, 0x212214, 0), (CK_IGEMM, 0x221214, 0), (WK_TAP, 0x449251, 1, WS_REDUCE16)),   # splitk 9
    ("1x1_32to125_n64_7x7", 64, 7, 7, 32, 125, 1, 1021,
     (CK_IGEMM, 0x211242, 0), (CK_IGEMM, 0x221214, 0), (WK_TAP, 0x449261, 1, WS_REDUCE16)),   # splitk 9
    ("1x1_64to30_n64_7x7", 64, 7, 7, 64, 30, 1, 1022,
     (CK_IGEMM, 0x221214, 0), (CK_IGEMM, 0x212214, 0), (WK_TAP, 0x44924a, 1, WS_REDUCE16)),   # splitk 9
    ("1x1_64to64_n64_7x7", 64, 7, 7, 64, 64, 1, 1023,
     (CK_IGEMM, 0x222214, 0), (CK_IGEMM, 0x222214, 0), (WK_TAP, 0x449252, 1, WS_REDUCE16)),   # splitk 9
    ("1x1_64to125_n64_7x7", 64, 7, 7, 64, 125, 1, 1024,
     (CK_IGEMM, 0x321242, 0), (CK_IGEMM, 0x222214, 0), (WK_TAP, 0x449452, 1, WS_REDUCE16)),   # splitk 9
    ("1x1_96to30_n64_7x7", 64, 7, 7, 96, 30, 1, 1025,
     (CK_IGEMM, 0x221214, 0), (CK_IGEMM, 0x211242, 0), (WK_TAP, 0x44924c, 1, WS_REDUCE16)),   # splitk 9
    ("1x1_96to64_n64_7x7", 64, 7, 7, 96, 64, 1, 1026,
     (CK_IGEMM, 0x222214, 0), (CK_IGEMM, 0x321242, 0), (WK_TAP, 0x449292, 1, WS_REDUCE16)),   # splitk 9
    ("1x1_96to125_n64_7x7", 64, 7, 7, 96, 125, 1, 1027,
     (CK_IGEMM, 0x321242, 0), (CK_IGEMM, 0x321242, 0), (WK_TAP, 0x449492, 1, WS_REDUCE16)),   # splitk 9
    ("1x1_96to125_n8_40x104", 8, 40, 104, 96, 125, 1, 1028,
     (CK_IGEMM, 0x221242, 0), (CK_IGEMM, 0x221242, 0), (WK_TAP, 0x449492, 1, WS_REDUCE16)),   # two-stage 128-cout tile (more than 256 workgroups), splitk 68
    ("3x3_32to30_n1_5x5", 1, 5, 5, 32, 30, 3, 1029,
     (CK_HALOQ, 0x11214, 0), (CK_HALOQ, 0x11214, 0), (WK_NINE, 0x44a249, 0, WS_DIRECT)),   # splitk 1
    ("3x3_32to64_n1_5x5", 1, 5, 5, 32, 64, 3, 1030,
     (CK_HALOQ, 0x12214, 0), (CK_HALOQ, 0x21214, 0), (WK_NINE, 0x44a251, 0, WS_DIRECT)),   # splitk 1
    ("3x3_96to30_n1_5x5", 1, 5, 5, 96, 30, 3, 1031,
     (CK_HALOQ, 0x21214, 0), (CK_HALOQ, 0x12222, 0), (WK_NINE, 0x45224a, 0, WS_DIRECT)),   # splitk 1
    ("3x3_96to64_n1_5x5", 1, 5, 5, 96, 64, 3, 1032,
     (CK_HALOQ, 0x22214, 0), (CK_HALOQ, 0x21224, 0), (WK_NINE, 0x45224a, 0, WS_DIRECT)),   # splitk 1
    ("3x3_96to256_n1_5x5", 1, 5, 5, 96, 256, 3, 1033,
     (CK_HALOQ, 0x21224, 0), (CK_HALOQ_KS, 0x21224, 1), (WK_NINE, 0x45224a, 0, WS_DIRECT)),   # dgrad K split 2 deep, splitk 1
    ("3x3_96to425_n1_5x5", 1, 5, 5, 96, 425, 3, 1034,
     (CK_HALOQ, 0x21224, 0), (CK_HALOQ_KS, 0x21224, 1), (WK_NINE, 0x45224a, 0, WS_DIRECT)),   # dgrad K split 3 deep (of 7 chunks), splitk 1
    ("3x3_2048to512_n1_5x5", 1, 5, 5, 2048, 512, 3, 1035,
     (CK_HALOQ_KS, 0x21224, 1), (CK_HALOQ_KS, 0x21224, 1), (WK_NINE, 0x44a24a, 0, WS_DIRECT)),   # forward K split 8 deep, dgrad 4 deep, splitk 1
    ("3x3_32to30_n8_7x7", 8, 7, 7, 32, 30, 3, 1036,
     (CK_HALOQ, 0x11214, 0), (CK_HALOQ, 0x11214, 0), (WK_NINE, 0x44a249, 1, WS_REDUCE1)),   # splitk 2
    ("3x3_32to125_n8_7x7", 8, 7, 7, 32, 125, 3, 1037,
     (CK_HALOQ, 0x12222, 0), (CK_HALOQ, 0x21214, 0), (WK_NINE, 0x44a251, 1, WS_REDUCE1)),   # splitk 2
    ("3x3_64to30_n16_7x7", 16, 7, 7, 64, 30, 3, 1038,
     (CK_HALOQ, 0x21214, 0), (CK_HALOQ, 0x12214, 0), (WK_NINE, 0x45224a, 1, WS_REDUCE1)),   # splitk 2
    ("3x3_1024to1024_n1_28x28", 1, 28, 28, 1024, 1024, 3, 1039,
     (CK_HALOQ_KS, 0x21224, 1), (CK_HALOQ_KS, 0x21224, 1), (WK_NINE, 0x44a24a, 1, WS_REDUCE1)),   # both K splits 4 deep, splitk 2
    ("3x3_64to64_n1_19x52", 1, 19, 52, 64, 64, 3, 1040,
     (CK_HALOQ, 0x22214, 0), (CK_HALOQ, 0x22214, 0), (WK_RING, 0x45224a, 1, WS_REDUCE1)),   # splitk 2
    ("3x3_32to64_n1_30x53", 1, 30, 53, 32, 64, 3, 1041,
     (CK_HALOQ, 0x11424, 0), (CK_HALOQ, 0x21218, 0), (WK_RING, 0x452251, 1, WS_REDUCE1)),   # splitk 2
    ("3x3_64to64_n1_30x53", 1, 30, 53, 64, 64, 3, 1042,
     (CK_HALOQ, 0x21424, 0), (CK_HALOQ, 0x21424, 0), (WK_RING, 0x45224a, 1, WS_REDUCE1)),   # splitk 2
    ("3x3_96to125_n1_30x53", 1, 30, 53, 96, 125, 3, 1043,
     (CK_HALOQ, 0x12224, 0), (CK_HALOQ, 0x12224, 0), (WK_RING, 0x45224a, 1, WS_REDUCE1)),   # splitk 2
    ("3x3_32to30_n2_19x52", 2, 19, 52, 32, 30, 3, 1044,
     (CK_HALOQ, 0x11214, 0), (CK_HALOQ, 0x11214, 0), (WK_RING, 0x44a249, 1, WS_REDUCE1)),   # ring over two images, W + 1 = 53, splitk 3
    ("3x3_32to30_n64_7x7", 64, 7, 7, 32, 30, 3, 1045,
     (CK_HALOQ, 0x11214, 0), (CK_HALOQ, 0x11214, 0), (WK_NINE, 0x44a249, 1, WS_REDUCE16)),   # splitk 9
    ("3x3_32to125_n64_7x7", 64, 7, 7, 32, 125, 3, 1046,
     (CK_HALOQ, 0x12324, 0), (CK_HALOQ, 0x21214, 0), (WK_NINE, 0x44a251, 1, WS_REDUCE16)),   # splitk 9
    ("3x3_32to64_n1_12x300", 1, 12, 300, 32, 64, 3, 1047,
     (CK_IGEMM, 0x212214, 0), (CK_HALOQ, 0x21214, 0), (WK_RING, 0x44a251, 1, WS_REDUCE1)),   # 3x3 igemm outside the register-filter window, splitk 2
    ("3x3_1024to1024_n4_19x52", 4, 19, 52, 1024, 1024, 3, 1048,
     (CK_HALOQ, 0x21324, 0), (CK_HALOQ, 0x21324, 0), (WK_RING, 0x45224a, 0, WS_DIRECT)),   # ring over four images, splitk 1
    ("3x3_32to30_n2_56x56", 2, 56, 56, 32, 30, 3, 1049,
     (CK_HALOQ, 0x11218, 0), (CK_HALOQ, 0x11218, 0), (WK_RING, 0x44a249, 1, WS_REDUCE16)),   # splitk 9
    ("3x3_96to30_n128_7x7", 128, 7, 7, 96, 30, 3, 1050,
     (CK_HALOQ, 0x21214, 0), (CK_HALOQ, 0x12324, 0), (WK_NINE, 0x45224a, 1, WS_REDUCE16)),   # splitk 9
    ("3x3_32to64_n8_19x52", 8, 19, 52, 32, 64, 3, 1051,
     (CK_HALOQ, 0x12214, 0), (CK_HALOQ, 0x21214, 0), (WK_RING, 0x452251, 1, WS_REDUCE16)),   # splitk 9
    ("3x3_64to30_n3_56x56", 3, 56, 56, 64, 30, 3, 1052,
     (CK_HALOQ, 0x21218, 0), (CK_HALOQ, 0x11424, 0), (WK_RING, 0x45224a, 1, WS_REDUCE16)),   # splitk 10
    ("3x3_32to64_n2_64x127", 2, 64, 127, 32, 64, 3, 1053,
     (CK_IGEMM, 0x212214, 0), (CK_HALOQ, 0x21218, 0), (WK_RING, 0x44a251, 1, WS_REDUCE16)),   # splitk 11
    ("3x3_96to125_n256_14x14", 256, 14, 14, 96, 125, 3, 1054,
     (CK_HALOQ, 0x22224, 0), (CK_HALOQ, 0x22224, 0), (WK_NINE, 0x45224a, 1, WS_REDUCE16)),   # cost model: 256 x 128, splitk 57
    ("3x3_96to125_n64_19x52", 64, 19, 52, 96, 125, 3, 1055,
     (CK_HALOQ, 0x122324, 0), (CK_HALOQ, 0x122324, 0), (WK_RING, 0x45224a, 1, WS_REDUCE16)),   # 384 x 128 on 16x16 tiles, splitk 64
    ("3x3_96to125_n512_14x14", 512, 14, 14, 96, 125, 3, 1056,
     (CK_HALOQ, 0x22424, 0), (CK_HALOQ, 0x22424, 0), (WK_NINE, 0x45224a, 1, WS_REDUCE16)),   # cost model: 512 x 128, splitk 64
    ("3x3_64to125_n32_40x104", 32, 40, 104, 64, 125, 3, 1057,
     (CK_RFN, 0x3, 0), (CK_HALOQ, 0x21424, 0), (WK_RING, 0x45224a, 1, WS_REDUCE16)),   # register filters, 128-cout form (M >= 131072), splitk 90
    ("3x3_96to64_n32_40x104", 32, 40, 104, 96, 64, 3, 1058,
     (CK_HALOQ, 0x21424, 0), (CK_RFN, 0x3, 0), (WK_RING, 0x45224a, 1, WS_REDUCE16)),   # its dgrad, splitk 90
    ("3x3_32to64_n64_20x208", 64, 20, 208, 32, 64, 3, 1059,
     (CK_RF, 0x1, 0), (CK_RF, 0x2, 0), (WK_RING, 0x44a251, 1, WS_REDUCE16)),   # register filters 32 <-> 64 (M >= 262144), splitk 138
    ("3x3_64to30_n64_20x208", 64, 20, 208, 64, 30, 3, 1060,
     (CK_RF, 0x2, 0), (CK_RF, 0x1, 0), (WK_RING, 0x45224a, 1, WS_REDUCE16)),   # the same two configs with the directions swapped, splitk 110
    ("3x3_1152to1024_n1_28x28", 1, 28, 28, 1152, 1024, 3, 1061,
     (CK_HALOQ_KS, 0x21224, 1), (CK_HALOQ_KS, 0x21224, 1), (WK_NINE, 0x44a24a, 1, WS_ATOMIC)),   # 576 dW tiles, splitk 2: 2 x 9 x 1152 x 1024 floats outgrow the slab
    ("3x3_64to64_n1_4x400", 1, 4, 400, 64, 64, 3, 1062,
     (CK_IGEMM, 0x222214, 0), (CK_IGEMM, 0x222214, 0), (WK_TAP, 0x449252, 1, WS_REDUCE1)),   # 400-wide rows: no nine-tap window fits LDS, the per-tap kernel runs nine taps; splitk 5
]
CASE_IDS = [c[0] for c in CASES]
# Cases whose three keys all occur in earlier cases too, kept for a stated reason (test_exact_cases_host.py)
DUPLICATE_REASONS = {
    "3x3_96to425_n1_5x5": "the conv_haloq K split at a depth (3) that does not divide its 7 K chunks: the depth is not "
                          "part of the key",
    "3x3_64to64_n1_4x400": "the per-tap weight-gradient kernel with NINE taps (rows too long for a nine-tap window or ring "
                           "in LDS): the key has no taps field, so it shares the 1x1 cases' key",
}
# cases run once more in a child process with Y2_NO_WGRAD_SLAB=1: the float-atomics route (WS_ATOMIC) of each family.
# Without the switch the route is taken where the partial tiles outgrow the 1024 x 18432 floats of the slab: 3x3 layers
# 27 to 51 wide whose 64 x 32 dW tiles number 513 to 767 take splitk 2 (3x3_1152to1024_n1_28x28 above; 1024 -> 1024 sits
# exactly on the boundary).  The other condition of plan_sum, taps * Cin * Cout not a multiple of 4, cannot occur: every
# accepted Cin is a multiple of 32.
ATOMIC_CASES = ("1x1_64to125_n8_7x7", "3x3_32to125_n8_7x7", "3x3_32to30_n2_19x52")


# ---- forms only a Network launches: the forward epilogue that writes batch-norm records (layer 0 of a two-layer
# network in training mode) and the dgrad whose epilogue carries the batch-norm-backward reduce of the layer below
# (layer 1's dgrad: a layer's dgrad reduces for the layer UNDER it, so a 3x3 second layer is what reaches the conv_haloq
# and register-filter forms).
# (name, N, H, W, layer 0 (k, cin, cout, pool), layer 1 (k, cout), seed, layer 0 forward form, layer 1 dgrad form, note)
NET_CASES = [
    ("rf_32to64_pool", 64, 20, 208, (3, 32, 64, 1), (1, 32), 2000, (CK_RF, 0x1, 0), (CK_IGEMM, 0x212214, 0),
     "register-filter kernel's own records; pooled"),
    ("rfn_64to128", 32, 40, 104, (3, 64, 128, 0), (3, 64), 2001, (CK_RFN, 0x3, 0), (CK_RFN, 0x3, 0),
     "128-cout register-filter form: its records, and its dgrad with the fused reduce"),
    ("haloq_32to32_56", 2, 56, 56, (3, 32, 32, 0), (3, 64), 2002, (CK_HALOQ, 0x11218, 0), (CK_HALOQ, 0x21218, 0),
     "whole tiles and a tail tile (M = 6272, 512-pixel tiles)"),
    ("haloq_32to64_53", 1, 30, 53, (3, 32, 64, 0), (1, 32), 2003, (CK_HALOQ, 0x11424, 0), (CK_IGEMM, 0x212214, 0),
     "odd row length, whole tiles and a tail"),
    ("haloq_64to64_53", 1, 30, 53, (3, 64, 64, 0), (3, 64), 2004, (CK_HALOQ, 0x21424, 0), (CK_HALOQ, 0x21424, 0), ""),
    ("haloq_128to128_53", 1, 30, 53, (3, 128, 128, 0), (3, 32), 2005, (CK_HALOQ, 0x12224, 0), (CK_HALOQ, 0x12224, 0), ""),
    ("haloq_128to128_5", 1, 5, 5, (3, 128, 128, 0), (3, 128), 2006, (CK_HALOQ, 0x21224, 0), (CK_HALOQ, 0x21224, 0),
     "one tail tile only: the VALU record path"),
    ("haloq_512to512_n64_13", 64, 13, 13, (3, 512, 512, 0), (3, 512), 2007, (CK_HALOQ, 0x21324, 0), (CK_HALOQ, 0x21324, 0),
     "384 x 64 tiles: the cost model keeps them from 512 channels at 10816 pixels on"),
    ("haloq_64to64_pool_10", 1, 10, 10, (3, 64, 64, 1), (3, 64), 2008, (CK_HALOQ, 0x22214, 0), (CK_HALOQ, 0x22214, 0),
     "pooled: bn_stats_sub_kernel"),
    ("haloq_128to128_n256_14", 256, 14, 14, (3, 128, 128, 0), (3, 128), 2009, (CK_HALOQ, 0x22224, 0), (CK_HALOQ, 0x22224, 0),
     "whole tiles only (M = 196 x 256)"),
    ("haloq_128to128_n512_14", 512, 14, 14, (3, 128, 128, 0), (3, 128), 2010, (CK_HALOQ, 0x22424, 0), (CK_HALOQ, 0x22424, 0), ""),
    ("haloq_128to128_n64_19x52", 64, 19, 52, (3, 128, 128, 0), (3, 128), 2011, (CK_HALOQ, 0x122324, 0),
     (CK_HALOQ, 0x122324, 0), "16x16-tile kernel"),
    ("haloq_ks_256to256_5", 1, 5, 5, (3, 256, 256, 0), (1, 32), 2012, (CK_HALOQ_KS, 0x21224, 1), (CK_IGEMM, 0x211242, 0),
     "conv_ks_stats_kernel after the conv_haloq K split"),
    ("igemm_32to64_5", 1, 5, 5, (1, 32, 64, 0), (1, 64), 2013, (CK_IGEMM, 0x212214, 0), (CK_IGEMM, 0x222214, 0), ""),
    ("igemm_64to32_5", 1, 5, 5, (1, 64, 32, 0), (1, 32), 2014, (CK_IGEMM, 0x221214, 0), (CK_IGEMM, 0x211214, 0), ""),
    ("igemm_128to128_40x104", 8, 40, 104, (1, 128, 128, 0), (1, 128), 2015, (CK_IGEMM, 0x221242, 0),
     (CK_IGEMM, 0x221242, 0), "two-stage 128-cout tile"),
    ("igemm_64to64_5", 1, 5, 5, (1, 64, 64, 0), (1, 32), 2016, (CK_IGEMM, 0x222214, 0), (CK_IGEMM, 0x212214, 0), ""),
    ("igemm_64to128_5", 1, 5, 5, (1, 64, 128, 0), (1, 64), 2017, (CK_IGEMM, 0x321242, 0), (CK_IGEMM, 0x321242, 0), ""),
    ("igemm_ks_512to128_7", 8, 7, 7, (1, 512, 128, 0), (1, 32), 2018, (CK_IGEMM_KS, 0x221242, 1), (CK_IGEMM, 0x211242, 0),
     "conv_ks_stats_kernel after the 1x1 K split"),
    ("igemm_32to128_long_list", 8, 257, 256, (1, 32, 128, 0), (1, 32), 2019, (CK_IGEMM, 0x211242, 0), (CK_IGEMM, 0x211242, 0),
     "4112 records of 128 pixels: bn_compress_kernel (P > 4096); the narrowest layer with 128-pixel records"),
]
NET_CASE_IDS = [c[0] for c in NET_CASES]


def net_case_keys(case, dtype):
    """the two records a net case pins: layer 0's forward with statistics, layer 1's dgrad with the fused reduce"""
    return conv_key(dtype, 0, case[7], EPI_STATS), conv_key(dtype, 1, case[8], EPI_BNBWD)


def net_case_data(case):
    """integer x [N,H,W,cin], W0 [k,k,cin,cout], b0 [cout] of layer 0: the op-level recipe, plus an integer offset of
    two to three standard deviations of the response on every fifth channel (alternating sign), so that the statistics
    are formed around an offset on some channels and around zero on the others"""
    _, N, H, W, (k, cin, cout, _pool), _l1, seed = case[:7]
    rng = np.random.default_rng(seed)
    K = k * k * cin
    p = density(K)
    x = _sparse_signs(rng, (N, H, W, cin), p)
    w = _sparse_signs(rng, (k, k, cin, cout), p)
    b = rng.integers(-1, 2, cout).astype(np.float32)
    # (three of them where the response leaves room below bf16's 256: the extremes of the sum reach about 5.5 of them)
    std = float(np.sqrt(K * p * p))
    off = float(np.round(min(3.0 * std, 252.0 - 6.0 * std)))
    b[::5] += off * np.where(np.arange(0, cout, 5) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return x, w, b


def conv_key(dtype, is_dgrad, form, epi=EPI_PLAIN):
    """the launch-log record of a convolution: form = (kind, cfg, K split)"""
    return (0, LAUNCH_DTYPE[dtype], int(is_dgrad), form[0], form[1], form[2], epi)


def wgrad_key(dtype, form, sum_route=None):
    """the launch-log record of a weight gradient: form = (kind, tile, splitk > 1, sum route)"""
    return (1, LAUNCH_DTYPE[dtype], form[0], form[1], form[2], form[3] if sum_route is None else sum_route, 0)


def case_keys(case, dtype):
    return [conv_key(dtype, 0, case[8]), conv_key(dtype, 1, case[9]), wgrad_key(dtype, case[10])]


def key_name(rec):
    """a record of the launch log as text, dtype-free (f16 and bf16 take identical plans)"""
    if rec[0] == 0:
        return "conv %-5s %-8s 0x%06x %-6s %s" % ("dgrad" if rec[2] else "fwd", CK_NAMES[rec[3]], rec[4],
                                                  "ksplit" if rec[5] else "-", EPI_NAMES[rec[6]])
    return "wgrad      %-8s 0x%06x %-6s %s" % (WK_NAMES[rec[2]], rec[3], "splitk" if rec[4] else "-", WS_NAMES[rec[5]])


def _sparse_signs(rng, shape, density):
    """integers in {-1, 0, +1} as float32, nonzero with probability `density`"""
    u = rng.random(shape, dtype=np.float32)
    s = np.where(rng.random(shape, dtype=np.float32) < 0.5, np.float32(-1), np.float32(1))
    return np.where(u < np.float32(density), s, np.float32(0)).astype(np.float32)


def density(K):
    return min(0.5, float(np.sqrt(1000.0 / K)))


def case_data(case):
    """-> x [N,H,W,Cin], w [k,k,Cin,Cout] (HWIO), bias [Cout], dy [N,H,W,Cout]: float32 numpy holding small integers"""
    _, N, H, W, cin, cout, k, seed = case[:8]
    rng = np.random.default_rng(seed)
    Kf, Kd = k * k * cin, k * k * cout
    x = _sparse_signs(rng, (N, H, W, cin), density(Kf))
    w = _sparse_signs(rng, (k, k, cin, cout), density(max(Kf, Kd)))
    b = rng.integers(-1, 2, cout).astype(np.float32)
    dy = _sparse_signs(rng, (N, H, W, cout), density(Kd))
    return x, w, b, dy


def dgrad_reference(dy, w):
    """float64: dx[p] = sum over taps of dy[p - tap] W[tap]^T for dy [N,H,W,Cout], W [k,k,Cin,Cout] -> [N,H,W,Cin]"""
    dy, w = dy.double(), w.double()
    N, H, W, cout = dy.shape
    k, cin = w.shape[0], w.shape[2]
    r = k // 2
    dyp = torch.nn.functional.pad(dy, (0, 0, r, r, r, r))
    dx = torch.zeros((N * H * W, cin), dtype=torch.float64, device=dy.device)
    for dh in range(k):
        for dv in range(k):
            ds = dyp[:, 2 * r - dh:2 * r - dh + H, 2 * r - dv:2 * r - dv + W, :].reshape(-1, cout)
            dx += ds @ w[dh, dv].t()
    return dx.reshape(N, H, W, cin)


def reference(x, w, b, dy):
    """float64 torch on the device of its inputs: y = conv(x, W) 'SAME' + b [N,H,W,Cout], dx [N,H,W,Cin],
    dW [k,k,Cin,Cout] = sum over all pixels of x[p + tap] (x) dy[p].  One matmul per tap on zero-padded tensors."""
    x, w, dy = x.double(), w.double(), dy.double()
    N, H, W, cin = x.shape
    k, cout = w.shape[0], w.shape[3]
    r = k // 2
    xp = torch.nn.functional.pad(x, (0, 0, r, r, r, r))
    dyp = torch.nn.functional.pad(dy, (0, 0, r, r, r, r))
    M = N * H * W
    y = torch.zeros((M, cout), dtype=torch.float64, device=x.device)
    dx = torch.zeros((M, cin), dtype=torch.float64, device=x.device)
    dw = torch.empty((k, k, cin, cout), dtype=torch.float64, device=x.device)
    dyf = dy.reshape(M, cout)
    for dh in range(k):
        for dv in range(k):
            xs = xp[:, dh:dh + H, dv:dv + W, :].reshape(M, cin)
            y += xs @ w[dh, dv]
            dw[dh, dv] = xs.t() @ dyf
            # dx[p] = sum over taps of dy[p - tap] W[tap]^T
            ds = dyp[:, 2 * r - dh:2 * r - dh + H, 2 * r - dv:2 * r - dv + W, :].reshape(M, cout)
            dx += ds @ w[dh, dv].t()
    if b is not None:
        y += b.double()
    return y.reshape(N, H, W, cout), dx.reshape(N, H, W, cin), dw


def check_magnitudes(name, y, dx, dw):
    """the conditions under which every stored value is exact in f16 AND bf16, from the reference alone"""
    my, mdx, mdw = float(y.abs().max()), float(dx.abs().max()), float(dw.abs().max())
    assert my <= STORE_MAX["bf16"] and mdx <= STORE_MAX["bf16"], (name, "max |y|, |dx| beyond bf16's integers", my, mdx)
    assert mdw < 2 ** 24, (name, "max |dW| beyond fp32's integers", mdw)
    return my, mdx, mdw


def mismatch_report(what, got, ref, axes):
    """'' when got == ref in every element, else the count and the first few wrong indices named by `axes`"""
    bad = got != ref
    n = int(bad.sum())
    if n == 0:
        return ""
    idx = bad.nonzero()[:8].cpu().tolist()
    first = ", ".join("(%s) got %g want %g" % (", ".join("%s %d" % (a, i) for a, i in zip(axes, ix)),
                                                float(got[tuple(ix)]), float(ref[tuple(ix)])) for ix in idx)
    return "%s: %d of %d elements wrong; first: %s" % (what, n, bad.numel(), first)
