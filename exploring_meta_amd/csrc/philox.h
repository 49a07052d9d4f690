// Philox4x32-10 as a counter-based stream: key = the 64-bit seed's halves, counter = (id_lo, id_hi, stream, block).  Shared by the task
// draw (sampler.hip) and the rollout noise (rollout.hip, section 14); exploring_meta_amd/utils/task_sampler.py
// (philox4x32) restates it in numpy, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct Philox {           // one stream of one id: word w = output w % 4 of block w / 4
  uint32_t k0, k1, c0, c1, c2, block;
  uint32_t o0, o1, o2, o3;
  int pos;
  __device__ Philox(uint64_t seed, uint64_t id, uint32_t stream)
      : k0((uint32_t)seed), k1((uint32_t)(seed >> 32)), c0((uint32_t)id), c1((uint32_t)(id >> 32)), c2(stream), block(0), pos(4) {}
  __device__ void refill() {
    uint32_t a = c0, b = c1, c = c2, d = block, ka = k0, kb = k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      const uint32_t h0 = __umulhi(0xD2511F53u, a), l0 = 0xD2511F53u * a;
      const uint32_t h1 = __umulhi(0xCD9E8D57u, c), l1 = 0xCD9E8D57u * c;
      a = h1 ^ b ^ ka; b = l1; c = h0 ^ d ^ kb; d = l0;
      ka += 0x9E3779B9u; kb += 0xBB67AE85u;
    }
    o0 = a; o1 = b; o2 = c; o3 = d;
    ++block; pos = 0;
  }
  __device__ void seek(uint32_t b) { block = b; pos = 4; }   // the next word is word 0 of block b
  __device__ uint32_t next() {
    if (pos == 4) refill();
    const uint32_t v = pos == 0 ? o0 : pos == 1 ? o1 : pos == 2 ? o2 : o3;
    ++pos;
    return v;
  }
  // exactly uniform in [0, b), b >= 1 (Lemire's multiply-and-reject)
  __device__ uint32_t bounded(uint32_t b) {
    uint64_t m = (uint64_t)next() * b;
    uint32_t l = (uint32_t)m;
    if (l < b) {
      const uint32_t t = (0u - b) % b;            // (2^32 - b) % b
      while (l < t) { m = (uint64_t)next() * b; l = (uint32_t)m; }
    }
    return (uint32_t)(m >> 32);
  }
};
