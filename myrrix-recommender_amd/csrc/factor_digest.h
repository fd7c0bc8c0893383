// factor_digest.h -- the digest of a range of a factor replica (mals_factor_digest, mals_group_replica_digest,
// mals_factor_digest_host; defined in include/myrrix_als.h): the sum modulo 2^64 over the elements of the range of
// factor_digest_term(j, bits), j = the element's global flat index row * features + f, bits = its 32 bits.  A sum: any
// grid, any reduction tree and any split into ranges give the same number.  The arithmetic lives here once, for the host
// (mals_group.cpp) and for the device kernel below (mals_serving.hip).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MALS_DIGEST_HD __host__ __device__
#else
#define MALS_DIGEST_HD
#endif

namespace mals {

constexpr uint64_t DIGEST_MUL_INDEX = 0x9E3779B97F4A7C15ull;
constexpr uint64_t DIGEST_MUL_MIX = 0xD6E8FEB86659FD93ull;

// the second half of the mix, from z = j * DIGEST_MUL_INDEX + bits (modulo 2^64)
MALS_DIGEST_HD inline uint64_t factor_digest_finish(uint64_t z) {
  z ^= z >> 32;
  z *= DIGEST_MUL_MIX;
  z ^= z >> 32;
  return z;
}

MALS_DIGEST_HD inline uint64_t factor_digest_term(uint64_t j, uint32_t bits) { return factor_digest_finish(j * DIGEST_MUL_INDEX + bits); }

#if defined(MALS_FACTOR_DIGEST_KERNEL)   // (mals_serving.hip: every kernel lives in one translation unit)
// One streaming pass over the elements [e0, e1) of F (flat indices; F = the replica's first element).  The range is cut at
// the 16-byte boundaries of the ADDRESS: block 0 takes the elements before the first and after the last whole float4 one by
// one, every block strides over the float4s in between.  j * DIGEST_MUL_INDEX is carried along by additions (exact modulo
// 2^64), so an element costs one 64-bit multiply.  Per lane a 64-bit sum, folded per wave (shuffles), per workgroup (LDS),
// then one 64-bit vector atomic add per workgroup into *out, which the caller zeroed.
__global__ __launch_bounds__(256) void factor_digest_kernel(const float* __restrict__ F, int64_t e0, int64_t e1,
                                                            unsigned long long* __restrict__ out) {
  const int64_t n = e1 - e0;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(F + e0);
  int64_t head = (int64_t)(((16 - (addr & 15)) & 15) / sizeof(float));
  if (head > n) head = n;
  const int64_t n_vec = (n - head) / 4;
  const int64_t tail0 = e0 + head + 4 * n_vec;   // first element behind the float4s
  uint64_t acc = 0;
  if (blockIdx.x == 0) {
    if ((int64_t)threadIdx.x < head) {
      const int64_t j = e0 + threadIdx.x;
      acc += factor_digest_term((uint64_t)j, __float_as_uint(F[j]));
    }
    if (tail0 + (int64_t)threadIdx.x < e1) {   // (at most 3 elements)
      const int64_t j = tail0 + threadIdx.x;
      acc += factor_digest_term((uint64_t)j, __float_as_uint(F[j]));
    }
  }
  const float4* __restrict__ V = reinterpret_cast<const float4*>(F + e0 + head);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t zj = (uint64_t)(e0 + head + 4 * v) * DIGEST_MUL_INDEX;   // (j of the float4's first element) * DIGEST_MUL_INDEX
  const uint64_t zstep = (uint64_t)(4 * stride) * DIGEST_MUL_INDEX;
  for (; v < n_vec; v += stride, zj += zstep) {
    const float4 x = V[v];
    acc += factor_digest_finish(zj + __float_as_uint(x.x));
    acc += factor_digest_finish(zj + DIGEST_MUL_INDEX + __float_as_uint(x.y));
    acc += factor_digest_finish(zj + 2 * DIGEST_MUL_INDEX + __float_as_uint(x.z));
    acc += factor_digest_finish(zj + 3 * DIGEST_MUL_INDEX + __float_as_uint(x.w));
  }
  for (int d = 32; d > 0; d >>= 1) acc += (uint64_t)__shfl_down((unsigned long long)acc, d, 64);
  __shared__ unsigned long long part[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long s = part[0] + part[1] + part[2] + part[3];
    if (s) atomicAdd(out, s);
  }
}
#endif

}  // namespace mals
