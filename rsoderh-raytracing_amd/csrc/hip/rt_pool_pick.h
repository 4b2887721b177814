// rt_pool_pick.h — which stage a wave of the pool kernel (rt_wavepool.h) runs next, from how many of its slots wait in each stage.
// Plain C++17: no HIP header, no runtime call — the kernel and a CPU test (tests/cpp/pool_pick_host.cpp) read the same lines.
//
// The rule: the fullest stage; among equally full stages the later one, which drains paths; no stage if every count is zero; and
// never GEN (stage 0) once the frame's work is handed out — FREE slots are then nothing to run.  Written as a scan it is
//     for s = 0 .. 4:  if (count[s] >= best_n && count[s] > 0) { best = s; best_n = count[s]; }
// a chain of compares and selects, each waiting for the one before.  Here every stage gets the key (count << 3) | stage and the largest
// key wins: the larger count does, and of two equal counts the larger stage — the scan's `>=`.  A key below 8 has a count of zero, so a
// maximum below 8 means that nothing waits anywhere.  The counts are wave-uniform, at most a pool's 192 slots: four scalar maxima.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_PICK_FN __host__ __device__ inline
#else
#define RT_PICK_FN inline
#endif
// On the device every maximum is pinned to a scalar register (an empty asm statement, no instruction): left alone, the compiler fuses
// two maxima into a three-operand one, which only the vector unit has, moves the keys to vector registers for it and reads the
// result back — and forms the scheduler's exit test there too.  The counts are wave-uniform: this is scalar work.
#if defined(__HIP_DEVICE_COMPILE__)
#define RT_PICK_SCALAR(x) asm volatile("" : "+s"(x))
#else
#define RT_PICK_SCALAR(x) (void)(x)
#endif

constexpr uint32_t kPoolPickStages = 5u; // rt_wavepool.h PoolStage: GEN, TRACE, MISS, SHADE, FINISH; kPoolPickStages itself says "none"

struct PoolPick {
    uint32_t best;   // the stage to run, or kPoolPickStages
    uint32_t best_n; // how many slots wait in it
};

RT_PICK_FN uint32_t pool_pick_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// (counts below 2^29: the key is a 32-bit word)
RT_PICK_FN PoolPick pool_pick(uint32_t n_gen, uint32_t n_trace, uint32_t n_miss, uint32_t n_shade, uint32_t n_finish, bool exhausted)
{
    uint32_t key = exhausted ? 0u : (n_gen << 3);
    key = pool_pick_max(key, (n_trace << 3) | 1u);
    RT_PICK_SCALAR(key);
    key = pool_pick_max(key, (n_miss << 3) | 2u);
    RT_PICK_SCALAR(key);
    key = pool_pick_max(key, (n_shade << 3) | 3u);
    RT_PICK_SCALAR(key);
    key = pool_pick_max(key, (n_finish << 3) | 4u);
    RT_PICK_SCALAR(key);
    PoolPick p;
    p.best = key < 8u ? kPoolPickStages : (key & 7u);
    p.best_n = key >> 3;
    return p;
}
