// svdq_philox.h -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011),
// the counter-based generator of the DARE merge (svdq_dare.hip; include/svdq.h at svdq_plan_dare_merge says which counter
// and key a (row, task) pair uses).  Plain C++: two 32 x 32 -> 64-bit products per round as __umulhi and a 32-bit
// multiply, ten rounds, the key bumped by the Weyl constants between rounds.  A function of its arguments alone -- no
// state, no memory -- so any kernel may call it; the known answers are in tests/test_dare_model_cpu.py.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define SVDQ_PHILOX_M0 0xD2511F53u
#define SVDQ_PHILOX_M1 0xCD9E8D57u
#define SVDQ_PHILOX_W0 0x9E3779B9u
#define SVDQ_PHILOX_W1 0xBB67AE85u

// out0 .. out3 = Philox4x32-10 of the counter (c0, c1, c2, c3) under the key (k0, k1).  With a wave-uniform key the
// round keys are scalar.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t &out0, uint32_t &out1, uint32_t &out2, uint32_t &out3) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(SVDQ_PHILOX_M0, c0), lo0 = SVDQ_PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(SVDQ_PHILOX_M1, c2), lo1 = SVDQ_PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += SVDQ_PHILOX_W0;
        k1 += SVDQ_PHILOX_W1;
    }
    out0 = c0, out1 = c1, out2 = c2, out3 = c3;
}
