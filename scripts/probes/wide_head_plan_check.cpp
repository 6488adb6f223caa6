// The plan and byte functions of csrc/wide_head_train.hip under the host sanitizers: a stand-alone program (its own main,
// nothing loaded into Python, no GPU work -- only the host-only entries are called).  Their arithmetic stands in
// csrc/wide_gemm.h, header-inline, so wide_head_train.hip alone links.  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tensorflow_yolo2_amd/csrc/wide_head_train.hip \
//         scripts/probes/wide_head_plan_check.cpp -o scripts/probes/wide_head_plan_check && scripts/probes/wide_head_plan_check
// It walks 8 x 8 x 8 (M, K, Cout) triples, the limits and INT_MAX among them, 8 CU counts and 6 forced split counts each.
#include <stdio.h>
#include <stddef.h>
extern "C" {
int y2_wide_head_train_plan(int M, int K, int Cout, int cus, int* dx_split, int* dw_split);
size_t y2_wide_head_packed2_bytes(int K, int Cout);
size_t y2_wide_head_backward_input_workspace_bytes(int M, int K, int Cout, int split);
size_t y2_wide_head_backward_filter_workspace_bytes(int M, int K, int Cout, int split);
}
namespace y2 {
int set_error(int code, const char* msg) { (void)msg; return code; }
}
int main() {
    const int Ms[] = {1, 25, 256, 257, 513, 9248, 100000, 2147483647};
    const int Ks[] = {32, 64, 96, 1024, 4096, 48, 0, 4128};
    const int Cs[] = {1, 225, 257, 2115, 28269, 65536 * 16, 0, 65536 * 16 + 1};
    const int cus[] = {1, 8, 104, 256, 304, 1024, 2147483647, 0};
    long checked = 0;
    unsigned long long sum = 0;
    for (int M : Ms) for (int K : Ks) for (int C : Cs) {
        for (int cu : cus) {
            int a = -1, b = -1;
            if (y2_wide_head_train_plan(M, K, C, cu, &a, &b) == 0) {
                if (a < 1 || a > 64 || b < 1 || b > 64) { printf("bad plan %d %d %d %d -> %d %d\n", M, K, C, cu, a, b); return 1; }
                ++checked;
            }
        }
        for (int split : {1, 2, 64, 1000, 2147483647, -1}) {
            sum += y2_wide_head_backward_input_workspace_bytes(M, K, C, split);
            sum += y2_wide_head_backward_filter_workspace_bytes(M, K, C, split);
        }
        sum += y2_wide_head_packed2_bytes(K, C);
    }
    printf("plans checked: %ld, byte sum %llu\n", checked, sum);
    return 0;
}
