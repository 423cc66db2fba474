// l2_channel_probe.hip -- which address bits select an L2 (TCC) channel?
//
// One kernel per probed bit K: every workgroup reads 128-byte lines of a 256 MiB buffer whose byte addresses have bit K
// CLEAR and all other bits free (a running line index with a zero inserted at bit K).  Kernel <0> reads every line.  Under
//   rocprofv3 --pmc TCC_REQ --output-format json -- scripts/ubench/l2_channel_probe
// the per-instance values of TCC_REQ (scripts/pmc_channels.py prints them) show whether a kernel left channels idle: a bit
// that alone selects a channel halves the loaded channels, a bit that is hashed with others leaves all of them loaded.
// <100 + K>: bits K and K + 1 both clear, <200>: bits 7..9 all clear (one head of the dense [N, S, 8, 32] fp32 layout).
//   hipcc --offload-arch=gfx950 -O3 scripts/ubench/l2_channel_probe.hip -o scripts/ubench/l2_channel_probe
#include <hip/hip_runtime.h>
#include <cstdio>

constexpr size_t kBytes = 256ull << 20;
constexpr unsigned kLines = 1u << 19;       // lines each kernel reads (64 MiB)

__device__ __forceinline__ unsigned long long insert_zero(unsigned long long a, int bit)
{
    const unsigned long long low = a & ((1ull << bit) - 1ull);
    return ((a >> bit) << (bit + 1)) | low;
}

template <int MODE>
__global__ void __launch_bounds__(256) probe(const float4 *buf, float *sink)
{
    float s = 0.f;
    const unsigned part = threadIdx.x & 7u;                  // 8 lanes x 16 bytes = one 128-byte line
    for (unsigned line = blockIdx.x * 32u + threadIdx.x / 8u; line < kLines; line += gridDim.x * 32u) {
        unsigned long long a = (unsigned long long)line << 7;
        if (MODE >= 7 && MODE < 100) a = insert_zero(a, MODE);
        if (MODE >= 100 && MODE < 200) a = insert_zero(insert_zero(a, MODE - 100), MODE - 100 + 1);
        if (MODE == 200) a = insert_zero(insert_zero(insert_zero(a, 7), 8), 9);
        a &= kBytes - 1;
        const float4 v = buf[a / 16 + part];
        s += v.x + v.y + v.z + v.w;
    }
    if (s == 12345.678f) *sink = s;
}

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main()
{
    float4 *buf; float *sink;
    CHECK(hipMalloc(&buf, kBytes));
    CHECK(hipMalloc(&sink, 4));
    CHECK(hipMemset(buf, 0, kBytes));
    const dim3 grid(2048), block(256);
    hipLaunchKernelGGL(probe<0>, grid, block, 0, 0, buf, sink);
    hipLaunchKernelGGL(probe<7>, grid, block, 0, 0, buf, sink);
    hipLaunchKernelGGL(probe<8>, grid, block, 0, 0, buf, sink);
    hipLaunchKernelGGL(probe<9>, grid, block, 0, 0, buf, sink);
    hipLaunchKernelGGL(probe<10>, grid, block, 0, 0, buf, sink);
    hipLaunchKernelGGL(probe<11>, grid, block, 0, 0, buf, sink);
    hipLaunchKernelGGL(probe<12>, grid, block, 0, 0, buf, sink);
    hipLaunchKernelGGL(probe<107>, grid, block, 0, 0, buf, sink);
    hipLaunchKernelGGL(probe<108>, grid, block, 0, 0, buf, sink);
    hipLaunchKernelGGL(probe<109>, grid, block, 0, 0, buf, sink);
    hipLaunchKernelGGL(probe<200>, grid, block, 0, 0, buf, sink);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    printf("done\n");
    return 0;
}
