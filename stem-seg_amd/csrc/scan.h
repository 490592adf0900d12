// Exact int64 exclusive scan on the device, shared by the writers (writers.hip) and the JPEG encoder (vis.hip).
#pragma once
#include "common.h"

#include <algorithm>

namespace stemseg {
namespace {

constexpr int kScanThreads = 256;
constexpr int kScanTile = 4096;          // elements per workgroup in the scan (256 threads x 16)

__device__ __forceinline__ long long dev_n(const long long* n_dev, long long n_max) { return n_dev ? min(*n_dev, n_max) : n_max; }

// ------------------------------------------------------------------------------------------------ exclusive scan (int64)
// out[i] = sum(in[0..i)), out[n] = total, for n = min(*n_dev, n_max) (n_dev may be null).  Phase 1: tile sums.  Phase 2: one
// workgroup scans the tile sums.  Phase 3: each tile rescans itself from its offset.  Sequential per thread, so exact.
__device__ long long block_exclusive_scan(long long v, long long* sh, long long* total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const long long a = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const long long incl = sh[t];
    *total = sh[kScanThreads - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kScanThreads) void scan_tiles_kernel(const long long* __restrict__ in, const long long* n_dev, long long n_max,
                                                              long long* __restrict__ tile_sums) {
    __shared__ long long sh[kScanThreads];
    const long long n = dev_n(n_dev, n_max);
    const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * (kScanTile / kScanThreads);
    long long s = 0;
    for (int j = 0; j < kScanTile / kScanThreads; ++j)
        if (base + j < n) s += in[base + j];
    long long total;
    block_exclusive_scan(s, sh, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanThreads) void scan_tile_sums_kernel(long long* __restrict__ tile_sums, int n_tiles) {
    __shared__ long long sh[kScanThreads];
    long long carry = 0;
    for (int b = 0; b < n_tiles; b += kScanThreads) {
        const int i = b + (int)threadIdx.x;
        const long long v = i < n_tiles ? tile_sums[i] : 0;
        long long total;
        const long long ex = block_exclusive_scan(v, sh, &total);
        if (i < n_tiles) tile_sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tile_sums[n_tiles] = carry;
}

__global__ __launch_bounds__(kScanThreads) void scan_apply_kernel(const long long* __restrict__ in, const long long* n_dev, long long n_max,
                                                              const long long* __restrict__ tile_sums, int n_tiles, long long* __restrict__ out) {
    __shared__ long long sh[kScanThreads];
    const long long n = dev_n(n_dev, n_max);
    const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * (kScanTile / kScanThreads);
    long long s = 0;
    for (int j = 0; j < kScanTile / kScanThreads; ++j)
        if (base + j < n) s += in[base + j];
    long long total;
    long long run = tile_sums[blockIdx.x] + block_exclusive_scan(s, sh, &total);
    for (int j = 0; j < kScanTile / kScanThreads; ++j)
        if (base + j < n) {
            out[base + j] = run;
            run += in[base + j];
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = tile_sums[n_tiles];
}

int scan_tiles(long long n_max) { return (int)std::max<long long>(1, ceil_div(n_max, kScanTile)); }

// tile_sums: scan_tiles(n_max) + 1 entries; out: n_max + 1 entries
void launch_scan(const long long* in, const long long* n_dev, long long n_max, long long* tile_sums, long long* out, hipStream_t s) {
    const int nt = scan_tiles(n_max);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(nt), dim3(kScanThreads), 0, s, in, n_dev, n_max, tile_sums);
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3(1), dim3(kScanThreads), 0, s, tile_sums, nt);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nt), dim3(kScanThreads), 0, s, in, n_dev, n_max, tile_sums, nt, out);
}

}  // namespace
}  // namespace stemseg
