// Host and launch helpers shared by the kernel files: the grid clamp of the grid-stride kernels, argument checks, and the 256-thread
// workgroup sum of the loss reductions.
#pragma once
#include "common.h"

// workgroups of 256 threads for `work` items of a grid-stride kernel: ceil(work / 256) clamped to [1, cap]
inline int grid_256(int64_t work, int64_t cap = 8192) {
  const int64_t b = (work + 255) / 256;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

inline bool finite_f(float v) { return v == v && v - v == 0.f; }

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// sum over a 256-thread workgroup, the same value in every thread; `red` = 4 floats of LDS.  The leading barrier lets a kernel call it
// twice in a row on the same `red`.
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
