// Host stand-in for csrc/pa_device.h, for tools/tokenise_host/check.py ONLY: csrc/tokenise.hip compiled by the host compiler, one OS
// thread per GPU thread (pthread barrier = __syncthreads, statics = LDS), the blocks of a launch one after another.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <pthread.h>
#include <atomic>
#include <thread>
#include <vector>
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static thread_local dim3 threadIdx, blockIdx;
typedef void* hipStream_t;
static pthread_barrier_t g_bar;
static std::atomic<int> g_cnt{0};
inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
inline int __syncthreads_count(int p) {
    g_cnt.fetch_add(p ? 1 : 0); pthread_barrier_wait(&g_bar);
    int r = g_cnt.load(); pthread_barrier_wait(&g_bar);
    if (threadIdx.x == 0) g_cnt.store(0);
    pthread_barrier_wait(&g_bar);
    return r;
}
inline uint32_t mix32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline int atomicOr(int* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) {
    unsigned long long o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return o;
}
inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
    unsigned long long o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (v > o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return o;
}
template <typename K, typename A> void emu_launch(K kernel, dim3 grid, dim3 block, A a) {
    pthread_barrier_init(&g_bar, nullptr, block.x);
    for (unsigned b = 0; b < grid.x; ++b) {
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < block.x; ++t) ts.emplace_back([=] { threadIdx = dim3(t); blockIdx = dim3(b); kernel(a); });
        for (auto& t : ts) t.join();
    }
    pthread_barrier_destroy(&g_bar);
}
#define PA_LAUNCH(kernel, grid, block, shm, stream, a) emu_launch(kernel, grid, block, a)
