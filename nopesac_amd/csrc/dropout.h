// Counter-based dropout (not a public header): the keep decision of one element is a pure function of (seed, dropout site, element index),
// so no kernel stores a mask - the forward, the backward and nopesac_dropout_keep_mask all call dropout_keep and agree bit for bit.
//
//   mix64(z): the finaliser of SplitMix64 (Steele, Lea, Flood 2014; Stafford's "Mix13" constants), a bijection of 64-bit words
//       z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
//   key  = mix64(stream + mix64(seed))                 one word per (seed, site): dropout_key, wave-uniform, hoisted out of every loop
//   keep = (mix64(index + key) >> 32) >= threshold     threshold = floor(p 2^32) (host, double arithmetic): P(keep) = 1 - threshold / 2^32
//
// `stream` names the dropout site (the decoder trainer uses step * 64 + layer * 8 + site >= 0, the encoder trainer
// -(step * 32 + layer * 4 + site) - 1 < 0: disjoint under one seed, and dropout_key works modulo 2^64), `index` is the row-major index of
// the element in the logical tensor.  All arithmetic is modulo 2^64.  threshold == 0 (p == 0) keeps everything; callers test it first and skip the hash.
#pragma once
#include <stdint.h>

namespace nps {

__host__ __device__ __forceinline__ uint64_t dropout_mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__host__ __device__ __forceinline__ uint64_t dropout_key(int64_t seed, int64_t stream) {
    return dropout_mix64((uint64_t)stream + dropout_mix64((uint64_t)seed));
}

__host__ __device__ __forceinline__ bool dropout_keep_keyed(uint64_t key, int64_t index, uint32_t threshold) {
    return (uint32_t)(dropout_mix64((uint64_t)index + key) >> 32) >= threshold;
}

// THE decision: element `index` of site `stream` under `seed` is kept.
__host__ __device__ __forceinline__ bool dropout_keep(int64_t seed, int64_t stream, int64_t index, uint32_t threshold) {
    return dropout_keep_keyed(dropout_key(seed, stream), index, threshold);
}

}  // namespace nps
