// Workgroup building blocks of the codec and metric kernels (png.hip, jpeg.hip, jpegdec.hip, sflow.hip, metrics.hip); device
// only.  The order of every operation is part of what these helpers promise: the f64 sums and the segmented joins built on
// them are compared bit for bit with CPU models that add in the same order.
#pragma once
#include <hip/hip_runtime.h>

namespace dvd {

// Sum over the 64 lanes of a wave, valid in lane 0: v += the value 32, 16, .. 1 lanes further down, in that order.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// Maximum over the 64 lanes of a wave, valid in lane 0, in the same order; for values that hold no NaN.
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const T o = __shfl_down(v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

// Inclusive Hillis-Steele scan of one value per thread of a 256-thread workgroup in lds[256]: returns the thread's
// join(v_0, .., v_tid) and *total = that of thread 255.  join(earlier, later) need not commute; join(identity, x) stands for
// "nothing in front of x".  Two barriers per step; the caller puts a barrier between the return and the next write of lds.
template <typename T, typename Join>
__device__ __forceinline__ T block_scan_256(T* lds, T v, T identity, Join join, T* total) {
  const int tid = threadIdx.x;
  lds[tid] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const T before = tid >= d ? lds[tid - d] : identity;
    const T me = lds[tid];
    __syncthreads();
    lds[tid] = join(before, me);
    __syncthreads();
  }
  *total = lds[255];
  return lds[tid];
}

// One 256-thread workgroup scans n elements: thread t owns the contiguous run [t per, (t + 1) per) cut to n, per = ceil(n / 256).
// It joins load(i) over its run in index order, the runs are scanned, then it walks the run again and calls
// store(i, exclusive prefix of element i).  Returns the join of all n elements to every thread.
template <typename T, typename Index, typename Load, typename Join, typename Store>
__device__ __forceinline__ T chunked_scan_256(T* lds, Index n, T identity, Load load, Join join, Store store) {
  const int tid = threadIdx.x;
  const Index per = (n + 255) / 256;
  const Index lo = (Index)tid * per < n ? (Index)tid * per : n, hi = lo + per < n ? lo + per : n;
  T acc = identity;
  for (Index i = lo; i < hi; ++i) acc = join(acc, load(i));
  T total;
  block_scan_256(lds, acc, identity, join, &total);
  acc = tid ? lds[tid - 1] : identity;
  for (Index i = lo; i < hi; ++i) {
    const T v = load(i);                       // before the store: store may overwrite what load reads
    store(i, acc);
    acc = join(acc, v);
  }
  return total;
}

}  // namespace dvd
