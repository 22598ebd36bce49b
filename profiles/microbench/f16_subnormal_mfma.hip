// Does v_mfma_f32_32x32x16_f16 keep fp16 SUBNORMAL inputs (A side and B side) on gfx950 under this library's compile flags?
// One wave: the only non-zero product of output (0, 0) is 2^-15 (a subnormal half) x 1.0; prints what the MFMA returns.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 profiles/microbench/f16_subnormal_mfma.hip -o profiles/microbench/f16_subnormal_mfma
#include <hip/hip_runtime.h>
#include <cstdio>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ void probe(float* out) {
    const int lane = threadIdx.x;
    for (int side = 0; side < 2; side++) {
        f16x8 a, b;
        for (int j = 0; j < 8; j++) { a[j] = (_Float16)0.0f; b[j] = (_Float16)0.0f; }
        if (lane == 0) {
            const _Float16 tiny = (_Float16)0x1p-15f, one = (_Float16)1.0f;
            a[0] = side == 0 ? tiny : one;
            b[0] = side == 0 ? one : tiny;
        }
        f32x16 acc;
        for (int r = 0; r < 16; r++) acc[r] = 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
        if (lane == 0) out[side] = acc[0];
    }
}

int main() {
    float* d = nullptr;
    float h[2] = {-1.0f, -1.0f};
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 1;
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    printf("{\"expected\": %.9g, \"subnormal_A_times_1\": %.9g, \"one_times_subnormal_B\": %.9g, \"A_kept\": %s, \"B_kept\": %s}\n",
           0x1p-15, h[0], h[1], h[0] == 0x1p-15f ? "true" : "false", h[1] == 0x1p-15f ? "true" : "false");
    (void)hipFree(d);
    return 0;
}
