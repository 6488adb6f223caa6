// probe: the two forms of y2_passthrough_concat_darknet_backward (csrc/ext.hip) side by side in one process, batch 32,
// Cf = 64, Cc = 1024, S = 13 and 19; HIP events, median of 9 alternating blocks of 200 launches; the outputs are compared
// bit for bit first.  The library ships the scatter form ("Training Darknet's graph"): it measured 7 % faster.
//     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o darknet_route_backward_ab darknet_route_backward_ab.hip
//
// gather   a lane owns four channels of one dfine pixel: four 4-byte loads of dout through darknet_reorg_dest, the
//          closed-form inverse of darknet_reorg_source, one 16-byte store
// scatter  a lane owns four channels of one dout pixel: one 16-byte load, four 4-byte stores through
//          darknet_reorg_source (or one 16-byte store into dcoarse)
//
// The inverse.  An element of fine [H][W][C] is (pixel r = js W + is, channel cs).  darknet_reorg_source returns
// (js W + is) C + 4 c2 + t, so c2 = cs >> 2 and t = cs & 3, and its m = mm + t H W = r + t H W (mm < H W is the pixel).
// m was built as (2 i + (off & 1)) + 2 W (2 j + (off >> 1)) with 2 i + (off & 1) < 2 W, so h2 = m / 2W, w2 = m mod 2W,
// off = 2 (h2 & 1) + (w2 & 1), j = h2 >> 1, i = w2 >> 1.  Then k = off (C / 4) + c2 and rem = j W + i, which the
// forward split as rem = s + (H W / 4) (co & 3) with s < H W / 4 and co = 4 k + (co & 3): u = rem / (H W / 4),
// s = rem mod (H W / 4), co = 4 k + u.  The result is the offset s ld + co into one image of dout [Ho Wo][ld].
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <cstring>
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define Y2_DEV static __device__ __forceinline__
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 2; } } while (0)

Y2_DEV int darknet_reorg_source(int s, int co, int H, int W, int C) {
    const int HW = H * W;
    const int k = co >> 2;
    const int rem = s + (HW >> 2) * (co & 3);
    const int j = rem / W, i = rem - j * W;
    const int out_c = C >> 2;
    const int off = k / out_c, c2 = k - off * out_c;
    const int m = (2 * i + (off & 1)) + 2 * W * (2 * j + (off >> 1));
    const int t = m / HW, mm = m - t * HW;
    const int js = mm / W, is = mm - js * W;
    return (js * W + is) * C + 4 * c2 + t;
}
Y2_DEV size_t darknet_reorg_dest(int r, int cs, int H, int W, int C, int ld) {
    const int HW = H * W, quarter = HW >> 2;
    const int c2 = cs >> 2, t = cs & 3;
    const int m = r + HW * t;
    const int h2 = m / (2 * W), w2 = m - h2 * 2 * W;
    const int off = 2 * (h2 & 1) + (w2 & 1);
    const int k = off * (C >> 2) + c2;
    const int rem = (h2 >> 1) * W + (w2 >> 1);
    const int u = rem / quarter, s = rem - u * quarter;
    return (size_t)s * ld + (size_t)(4 * k + u);
}
__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ dout, float* __restrict__ dfine,
                                                     float* __restrict__ dcoarse, int N, int Ho, int Wo, int C, int Cc) {
    const int H = 2 * Ho, W = 2 * Wo, ld = 4 * C + Cc;
    const int cv = C / 4, ccv = Cc / 4;
    const size_t image = (size_t)Ho * Wo * ld, HW = (size_t)H * W;
    const size_t fine_total = (size_t)N * HW * cv;
    const size_t total = fine_total + (size_t)N * Ho * Wo * ccv;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        if (e < fine_total) {
            const int cs = (int)(e % cv) * 4;
            const size_t pix = e / cv;
            const int r = (int)(pix % HW);
            const float* img = dout + (pix / HW) * image;
            float* dst = dfine + pix * C + cs;
            f32x4 v;
            v[0] = img[darknet_reorg_dest(r, cs + 0, H, W, C, ld)];
            v[1] = img[darknet_reorg_dest(r, cs + 1, H, W, C, ld)];
            v[2] = img[darknet_reorg_dest(r, cs + 2, H, W, C, ld)];
            v[3] = img[darknet_reorg_dest(r, cs + 3, H, W, C, ld)];
            *(f32x4*)dst = v;
        } else {
            const size_t g = e - fine_total;
            const int cc = (int)(g % ccv) * 4;
            const size_t pix = g / ccv;
            *(f32x4*)(dcoarse + pix * Cc + cc) = *(const f32x4*)(dout + pix * ld + 4 * C + cc);
        }
    }
}
// scatter: a lane owns four consecutive channels of one dout pixel: one 16-byte load, then a 16-byte store (coarse) or
// four scattered 4-byte stores (reorganised part)
__global__ __launch_bounds__(256) void scatter_kernel(const float* __restrict__ dout, float* __restrict__ dfine,
                                                      float* __restrict__ dcoarse, int N, int Ho, int Wo, int C, int Cc) {
    const int H = 2 * Ho, W = 2 * Wo, ld = 4 * C + Cc;
    const int ldv = ld / 4;
    const size_t image = (size_t)H * W * C;
    const size_t total = (size_t)N * Ho * Wo * ldv;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int co = (int)(e % ldv) * 4;
        const size_t pix = e / ldv;
        const int s = (int)(pix % ((size_t)Ho * Wo));
        const size_t n = pix / ((size_t)Ho * Wo);
        const f32x4 v = *(const f32x4*)(dout + pix * ld + co);
        if (co >= 4 * C) {
            *(f32x4*)(dcoarse + pix * Cc + (co - 4 * C)) = v;
        } else {
            float* img = dfine + n * image;
            img[darknet_reorg_source(s, co + 0, H, W, C)] = v[0];
            img[darknet_reorg_source(s, co + 1, H, W, C)] = v[1];
            img[darknet_reorg_source(s, co + 2, H, W, C)] = v[2];
            img[darknet_reorg_source(s, co + 3, H, W, C)] = v[3];
        }
    }
}
int main() {
    const int N = 32, C = 64, Cc = 1024;
    for (int S : {13, 19}) {
        const size_t nd = (size_t)N * S * S * (4 * C + Cc), nf = (size_t)N * 4 * S * S * C, nc = (size_t)N * S * S * Cc;
        if (nf + nc != nd) { printf("size mismatch\n"); return 2; }
        std::vector<float> h(nd);
        for (size_t i = 0; i < nd; ++i) h[i] = (float)(i % 1000003) * 0.5f;
        float *dout, *dfA, *dcA, *dfB, *dcB;
        CK(hipMalloc(&dout, nd * 4)); CK(hipMalloc(&dfA, nf * 4)); CK(hipMalloc(&dcA, nc * 4));
        CK(hipMalloc(&dfB, nf * 4)); CK(hipMalloc(&dcB, nc * 4));
        CK(hipMemcpy(dout, h.data(), nd * 4, hipMemcpyHostToDevice));
        CK(hipMemset(dfA, 0xff, nf * 4)); CK(hipMemset(dfB, 0xff, nf * 4));
        CK(hipMemset(dcA, 0xff, nc * 4)); CK(hipMemset(dcB, 0xff, nc * 4));
        const size_t total = nd / 4;
        unsigned nb = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
        auto ga = [&]() { hipLaunchKernelGGL(gather_kernel, dim3(nb), dim3(256), 0, 0, dout, dfA, dcA, N, S, S, C, Cc); };
        auto sc = [&]() { hipLaunchKernelGGL(scatter_kernel, dim3(nb), dim3(256), 0, 0, dout, dfB, dcB, N, S, S, C, Cc); };
        ga(); sc();
        CK(hipDeviceSynchronize());
        std::vector<float> a(nf), b(nf), ca(nc), cb(nc);
        CK(hipMemcpy(a.data(), dfA, nf * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(b.data(), dfB, nf * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(ca.data(), dcA, nc * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(cb.data(), dcB, nc * 4, hipMemcpyDeviceToHost));
        const bool same = !memcmp(a.data(), b.data(), nf * 4) && !memcmp(ca.data(), cb.data(), nc * 4);
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        std::vector<float> tg, ts;
        for (int rep = 0; rep < 9; ++rep) {
            for (int leg = 0; leg < 2; ++leg) {
                CK(hipEventRecord(e0, 0));
                for (int i = 0; i < 200; ++i) { if (leg == 0) ga(); else sc(); }
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                (leg == 0 ? tg : ts).push_back(ms / 200);
            }
        }
        std::sort(tg.begin(), tg.end()); std::sort(ts.begin(), ts.end());
        const double moved = 2.0 * nd * 4;
        printf("S %d  outputs equal %d  gather %.4f ms %.0f GB/s  scatter %.4f ms %.0f GB/s  scatter/gather %.3f\n", S, (int)same,
               tg[4], moved / tg[4] / 1e6, ts[4], moved / ts[4] / 1e6, ts[4] / tg[4]);
        CK(hipFree(dout)); CK(hipFree(dfA)); CK(hipFree(dcA)); CK(hipFree(dfB)); CK(hipFree(dcB));
    }
    return 0;
}
