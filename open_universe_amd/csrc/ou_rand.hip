// ou_rand.hip -- the sampler's noise for hosts without torch: ou_randn
// (include/ouhip.h) fills a buffer with standard normals from Philox4x32-10
// counters through Box-Muller.  One counter gives four outputs, so a lane
// stores 16 bytes per counter; the grid is capped and strides over the rest.
// The kernel is far from any roof that matters (4 MB per 8 s clip): logf,
// sqrtf and sincospif are the accurate library functions, so the stream can be
// restated on a host to a few ulp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ouhip.h"
#include "ou_common.h"
#include "ou_normal.h"

namespace {

// kVec: out is 16-byte aligned (one float4 store per counter)
template <bool kVec>
__global__ void __launch_bounds__(256) randn_kernel(float* __restrict__ out, long long n, uint32_t k0, uint32_t k1,
                                                    unsigned long long offset)
{
    const long long nq = (n + 3) / 4;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += stride) {
        float z[4];
        ouhip_detail::normal4(k0, k1, offset + (unsigned long long)q, z);
        const long long i = 4 * q;
        if (kVec && i + 4 <= n) {
            *reinterpret_cast<float4*>(out + i) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
            for (int j = 0; j < 4; ++j)
                if (i + j < n) out[i + j] = z[j];
        }
    }
}

}  // namespace

extern "C" {

int ou_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    if (!ctr || !key || !out) return ou_fail(-1, "philox4x32: null");
    ouhip_detail::philox4x32(ctr, key, out);
    return 0;
}

int ou_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream)
{
    if (n < 0 || (n > 0 && !out)) return ou_fail(-1, "randn: bad arguments");
    if (n == 0) return 0;
    if ((uintptr_t)out % 4) return ou_fail(-1, "randn: out is not aligned to a float");
    const long long nq = ((long long)n + 3) / 4;
    const long long want = (nq + 255) / 256;
    const unsigned grid = (unsigned)(want < 2048 ? want : 2048);   // 256 CUs x 8 blocks, grid-stride beyond
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    hipStream_t s = (hipStream_t)stream;
    if ((uintptr_t)out % 16 == 0)
        hipLaunchKernelGGL(randn_kernel<true>, dim3(grid), dim3(256), 0, s, out, (long long)n, k0, k1,
                           (unsigned long long)offset);
    else
        hipLaunchKernelGGL(randn_kernel<false>, dim3(grid), dim3(256), 0, s, out, (long long)n, k0, k1,
                           (unsigned long long)offset);
    return ou_check_launch("randn");
}

}  // extern "C"
