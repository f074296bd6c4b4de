// rk_csv_scan.h -- the scans the device CSV ingress (rk_csv.hip) and egress
// (rk_csv_out.hip) share: a block's exclusive scan, and the one-block scan of
// per-block counts to offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rk {

// exclusive scan of v over the block's N threads; *total = the block's sum
template <uint32_t N>
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t *lds, uint32_t *total) {
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < N; d <<= 1) {
    const uint32_t a = t >= d ? lds[t - d] : 0u;
    __syncthreads();
    lds[t] += a;
    __syncthreads();
  }
  const uint32_t incl = lds[t];
  *total = lds[N - 1];
  __syncthreads();
  return incl - v;
}

// out[i] = in[0] + ... + in[i-1] for i in [0, n]; one block
template <class Out>
__global__ __launch_bounds__(1024) void k_csv_scan(const uint32_t *in, uint64_t n, Out *out) {
  __shared__ Out s[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t chunk = (n + 1023) / 1024;
  const uint64_t lo = min(n, (uint64_t)t * chunk), hi = min(n, lo + chunk);
  Out sum = 0;
  for (uint64_t i = lo; i < hi; ++i) sum += in[i];
  s[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const Out a = t >= d ? s[t - d] : (Out)0;
    __syncthreads();
    s[t] += a;
    __syncthreads();
  }
  Out run = s[t] - sum;
  for (uint64_t i = lo; i < hi; ++i) {
    out[i] = run;
    run += in[i];
  }
  if (t == 1023) out[n] = s[1023];
}

}  // namespace rk
