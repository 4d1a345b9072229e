// device_rng.h - the native random stream: Philox2x32-10, the seed and key mixing, one block per (block index, id, step).
// Part of libmarlnav.so: included by device_math.h (the step kernels' re-init
// draws) and by marlnav_policy.hip (the policy's action noise), inside each
// translation unit's anonymous namespace.
#pragma once

// ----------------------------------------------------------- native RNG
// The native stream (rng='native'; a distributional match of the reference's
// torch.rand draws, utils.py:381-398, checked by tests/test_native_rng_dist.py):
// Philox2x32-10 (Salmon et al., SC'11: Random123's philox2x32 at its default
// 10 rounds; its published known-answer vectors are checked in
// tests/test_oracle_golden.py). Uniform #idx of env gid at step s is word
// idx & 1 of block idx >> 1: counter (lo32(gid), lo32(s) ^ hi32(gid) *
// 0x85EBCA77) under the key native_key(seed, idx >> 1, s), on torch.rand's
// 24-bit grid. The key holds no per-env term, so where the block index is
// wave-uniform (the env-block kernel's draws) it and its round increments
// live in SGPRs. Obstacle j is block j (x = word 0, y = word 1): one block per
// obstacle, so an A3/O3 env block draws exactly one block per thread
// (Philox4x32-10, rounds 1-4, drew two 4-word blocks per env on two of the
// three waves: 20 v_mad_u64_u32 per drawing lane against 10 here).
// oracle/marlnav_oracle.c restates it.
constexpr uint32_t kPhiloxM2 = 0xD256D193u, kPhiloxW = 0x9E3779B9u;

__device__ __forceinline__ void philox2x32_10(uint32_t &c0, uint32_t &c1, uint32_t k)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // one v_mad_u64_u32 per round for the 64-bit product
        const uint64_t p = (uint64_t)c0 * kPhiloxM2;
        const uint32_t hi = (uint32_t)(p >> 32), lo = (uint32_t)p;
        c0 = __builtin_amdgcn_bitop3_b32(hi, k, c1, 0x96);  // hi ^ k ^ c1 in one VALU
        c1 = lo;
        k += kPhiloxW;
    }
}

// The caller's 64-bit seed enters the stream only through its splitmix64
// finalisation (Steele, Lea, Flood, OOPSLA'14: a bijection of the 64-bit
// words), done once per launch on the host (marlnav_step, marlnav_reinit_all
// store it in the kernel's MarlnavParams.seed): seeds that differ in either
// word give unrelated mixed seeds.
__host__ __device__ constexpr uint64_t native_seed_mix(uint64_t seed)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// murmur3's 32-bit finaliser (a bijection)
__host__ __device__ constexpr uint32_t fmix32(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

// the 32-bit Philox key of block `blk` at step s from the MIXED seed m
// (native_seed_mix): its low word XOR fmix32 of the block index, the high
// word of s (zero below 2^32 steps) and m's high word. No linear relation
// ties (seed, blk) to (seed', blk'): a key shared by two of them is a
// 2^-32 coincidence of the hashes, not a shift of the block index. The
// counter carries the env id and the low word of s. Where blk is
// wave-uniform (the env-block kernel's draws) the key is SALU work.
__host__ __device__ constexpr uint32_t native_key(uint64_t m, uint32_t blk, uint64_t s)
{
    return (uint32_t)m ^
           fmix32(blk * 0x9E3779B1u + (uint32_t)(s >> 32) * 0x85EBCA77u + (uint32_t)(m >> 32));
}

// block `blk` of env gid at step s: two 32-bit words
__device__ __forceinline__ void native_block(uint64_t seed, uint32_t blk, uint64_t gid, uint64_t s,
                                             uint32_t &r0, uint32_t &r1)
{
    r0 = (uint32_t)gid;
    r1 = (uint32_t)s ^ ((uint32_t)(gid >> 32) * 0x85EBCA77u);
    philox2x32_10(r0, r1, native_key(seed, blk, s));
}

// a 32-bit word -> [0, 1) on a 24-bit grid (torch.rand's fp32 values)
__device__ __forceinline__ float native_u24(uint32_t r) { return (float)(r >> 8) * 0x1.0p-24f; }
