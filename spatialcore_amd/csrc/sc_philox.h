// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): the counter-based generator of sc_perm_counter.hip (permutations)
// and sc_umap.hip (negative samples).  c <- ten rounds on the counter c under the key (k0, k1).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ static inline void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
