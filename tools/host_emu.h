// What the tools/*_host_emu.cpp programs share: enough of HIP for the kernels of phasm_amd/csrc/*.hip.h to compile as plain
// C++ with ONE lane per wave -- the qualifiers as nothing, the thread coordinates as globals that LAUNCH walks (threads run
// one after another, barriers are no-ops), the atomics as the plain read-modify-write they are without a second thread,
// and the wave helpers of kernels.hip.h for a wave of one.  A program includes this first, defines in namespace po what
// its kernels expect from kernels.hip.h beyond that (Edge, Row, NODE_NO_RANK, EDGE_EMPTY / edge_slot), then includes them.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <algorithm>
#define __global__
#define __device__
#define __shared__ static
#define __restrict__
#define __launch_bounds__(x)
struct D3 { uint32_t x; };
static D3 threadIdx, blockIdx, blockDim, gridDim;
static inline void __syncthreads() {}
template <class T, class V> T atomicAdd(T* p, V v) { T o = *p; *p = (T)(*p + (T)v); return o; }
template <class T, class V> T atomicSub(T* p, V v) { T o = *p; *p = (T)(*p - (T)v); return o; }
template <class T> T atomicMin(T* p, T v) { T o = *p; if (v < o) *p = v; return o; }
template <class T> T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
template <class T> T atomicOr(T* p, T v) { T o = *p; *p = o | v; return o; }
template <class T> T atomicCAS(T* p, T cmp, T v) { T o = *p; if (o == cmp) *p = v; return o; }
template <class T> T __shfl_xor(T v, int, int = 1) { return v; }
using std::max;
namespace po {
constexpr int WAVE = 1;
static inline uint32_t lane_id() { return 0; }
static inline uint64_t wave_sum64(uint64_t v) { return v; }
template <int N> void block_add(const uint64_t (&v)[N], unsigned long long* c) { for (int k = 0; k < N; ++k) c[k] += v[k]; }
}
#define LAUNCH(grid, block, ...) do { gridDim.x = (grid); blockDim.x = (block); for (uint32_t b_ = 0; b_ < (grid); ++b_) for (uint32_t t_ = 0; t_ < (block); ++t_) { blockIdx.x = b_; threadIdx.x = t_; __VA_ARGS__; } } while (0)
