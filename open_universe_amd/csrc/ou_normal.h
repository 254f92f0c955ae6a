// ou_normal.h -- the sampler's noise stream as a function of position: counter
// c of (seed, offset) gives the four standard normals ou_randn stores at
// elements 4 (c - offset) .. 4 (c - offset) + 3 (include/ouhip.h: ou_randn).
// One definition for ou_rand.hip, which fills a buffer with the stream, and
// ou_stream.hip, which generates a window's slice of it in place: the two must
// agree bit for bit.  Contraction is off inside box_muller, so no caller can
// fuse its final products into an addition of its own (__fmul_rn would not do:
// hipcc defines it as a plain product, which -ffp-contract=fast may fuse);
// nothing else in the chain is a multiply feeding an add (the scalings by 2^-24
// and by 2 are exact).
#pragma once
#include <cstdint>

#include "ou_philox.h"

namespace ouhip_detail {

__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float& za, float& zb)
{
#pragma clang fp contract(off)
    const float u1 = (float)((xa >> 8) + 1u) * 0x1p-24f;   // (0, 1], exact
    const float u2 = (float)(xb >> 8) * 0x1p-24f;          // [0, 1), exact
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    za = r * c;
    zb = r * s;
}

// the four normals of the 64-bit counter cq under the key (k0, k1)
__device__ __forceinline__ void normal4(uint32_t k0, uint32_t k1, unsigned long long cq, float z[4])
{
    const uint32_t ctr[4] = {(uint32_t)cq, (uint32_t)(cq >> 32), 0u, 0u};
    const uint32_t key[2] = {k0, k1};
    uint32_t x[4];
    philox4x32(ctr, key, x);
    box_muller(x[0], x[1], z[0], z[1]);
    box_muller(x[2], x[3], z[2], z[3]);
}

}  // namespace ouhip_detail
