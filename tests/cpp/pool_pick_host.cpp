// pool_pick_host.cpp — the stage pick of rt_pool_pick.h against the scan it replaces, on the host (tests/test_pool_pick.py builds and
// runs this with g++, once more under -fsanitize=address,undefined; no HIP header, no GPU).  The scan is the pool kernel's former
// loop, transcribed: GEN's count is dropped once the work is exhausted, then the stages are scanned upwards and a stage wins with
// `>=`, so the fullest stage is picked and of equally full stages the later one.  Compared for every count vector in
// {0, 1, 2, 63, 64, 65, 191, 192}^5, for both values of `exhausted`, and for 10^6 random vectors whose sum is at most a pool's 192 slots.
#include <cstdio>
#include <cstdint>

#include "rt_pool_pick.h"

static int failures = 0;
static unsigned long long checked = 0;

static PoolPick scan_pick(const uint32_t in[5], bool exhausted)
{
    uint32_t count[5];
    for (int s = 0; s < 5; s++) count[s] = in[s];
    if (exhausted) count[0] = 0;
    uint32_t best = 5, best_n = 0;
    for (uint32_t s = 0; s < 5; s++)
        if (count[s] >= best_n && count[s] > 0) { best = s; best_n = count[s]; }
    PoolPick p;
    p.best = best;
    p.best_n = best_n;
    return p;
}

static void check(const uint32_t c[5], bool exhausted)
{
    const PoolPick want = scan_pick(c, exhausted), got = pool_pick(c[0], c[1], c[2], c[3], c[4], exhausted);
    checked++;
    if (want.best != got.best || want.best_n != got.best_n) {
        if (failures++ < 20)
            std::fprintf(stderr, "FAILED counts %u %u %u %u %u exhausted %d: scan picks stage %u (%u slots), keys pick stage %u (%u slots)\n",
                         c[0], c[1], c[2], c[3], c[4], (int)exhausted, want.best, want.best_n, got.best, got.best_n);
    }
}

// (a generator of its own: the same vectors on every host)
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t next_u32()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}

int main()
{
    static_assert(kPoolPickStages == 5u, "five stages");
    const uint32_t edge[8] = {0u, 1u, 2u, 63u, 64u, 65u, 191u, 192u};
    for (uint32_t i = 0; i < 8u * 8u * 8u * 8u * 8u; i++) {
        uint32_t c[5], r = i;
        for (int s = 0; s < 5; s++) { c[s] = edge[r & 7u]; r >>= 3; }
        check(c, false);
        check(c, true);
    }
    for (uint32_t i = 0; i < 1000000u; i++) {
        // a pool of 192 slots dealt over the five stages and "waiting nowhere": cut points in [0, 192], sorted
        uint32_t cut[5];
        for (int k = 0; k < 5; k++) cut[k] = next_u32() % 193u;
        for (int a = 1; a < 5; a++)
            for (int b = a; b > 0 && cut[b - 1] > cut[b]; b--) { const uint32_t t = cut[b]; cut[b] = cut[b - 1]; cut[b - 1] = t; }
        // (every third vector with few distinct values, so that ties are common)
        uint32_t c[5] = {cut[0], cut[1] - cut[0], cut[2] - cut[1], cut[3] - cut[2], cut[4] - cut[3]};
        if (i % 3u == 0u)
            for (int s = 0; s < 5; s++) c[s] = (c[s] % 3u) * 8u;
        check(c, (next_u32() & 1u) != 0u);
    }
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("pool pick ok: %llu vectors\n", checked);
    return 0;
}
