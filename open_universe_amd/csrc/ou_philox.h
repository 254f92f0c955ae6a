// ou_philox.h -- Philox4x32-10 (Salmon et al., "Parallel random numbers: as
// easy as 1, 2, 3", SC'11), the block function of the sampler's noise stream
// (include/ouhip.h: ou_randn).  One definition for the kernel and for the
// host export ou_philox4x32, which the known-answer tests call.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OU_HD __host__ __device__
#else
#define OU_HD
#endif

namespace ouhip_detail {

OU_HD inline void philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    uint32_t k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0, c1 = (uint32_t)p1, c2 = n2, c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;   // the key schedule (the bump after round 10 is unused)
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

}  // namespace ouhip_detail
