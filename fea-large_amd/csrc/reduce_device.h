// reduce_device.h -- the block reductions of every kernel in the library: the one place a block sum is written.
//
// All of them sum in one fixed order -- a shuffle-down tree inside each of the four waves of a 256-thread block,
// then wave 0 + wave 1 + wave 2 + wave 3 --, which is what the bit-identical repeats the tests pin rest on.
// (k_norm2_* of amg.hip sum over an LDS tree instead and stay there: the smoother weights depend on that order.)
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// the same sum in every lane (butterfly: a fixed order as well)
__device__ __forceinline__ double wave_sum_all(double v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// sum over the 256 threads of a block; result valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *scratch /*[4]*/)
{
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0;
  if (threadIdx.x == 0) r = scratch[0] + scratch[1] + scratch[2] + scratch[3];
  __syncthreads();
  return r;
}

// NV sums over the 256 threads of a block, each in the order of block_sum; sum k valid in thread k < NV
template <int NV>
__device__ __forceinline__ double block_sums(double (&v)[NV], double (*scratch)[NV] /*[4][NV]*/)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const double s = wave_sum(v[k]);
    if (lane == 0) scratch[wave][k] = s;
  }
  __syncthreads();
  double r = 0;
  if (threadIdx.x < NV) r = ((scratch[0][threadIdx.x] + scratch[1][threadIdx.x]) + scratch[2][threadIdx.x]) + scratch[3][threadIdx.x];
  __syncthreads();
  return r;
}

// every block re-reduces the producer kernel's partial sums, in fixed order;
// result broadcast to all threads
__device__ __forceinline__ double reduce_partials(const double *part, int n, double *scratch /*[5]*/)
{
  double v = 0;
  for (int i = threadIdx.x; i < n; i += 256) v += part[i];
  v = block_sum(v, scratch);
  if (threadIdx.x == 0) scratch[4] = v;
  __syncthreads();
  v = scratch[4];
  __syncthreads();
  return v;
}

// The two generic kernels, defined once in kernels_solve.hip; other files launch the second through
// enq_reduce_final (feahip_internal.h).
// part[block] = sum of a[i] * b[i] over the block's share of [i0, i1)
__global__ __launch_bounds__(256) void k_dot_partial(int i0, int i1, const double *a, const double *b, double *part);
// out[k] = sum of part[k*stride .. k*stride+n)  for k < nsums  (one block)
__global__ __launch_bounds__(256) void k_reduce_final(int n, int nsums, int stride, const double *part, double *out);
