// cold_layout_host.cpp — the arena layout of rt_cold_layout.h, checked on the host (tests/test_cold_layout.py builds and runs this
// with g++; no HIP header, no GPU).  For every traversal 0-6 and pools of 128, 160 and 192 slots: cold_index is injective over
// fields x slots and stays inside the wave's block; the walks keep field * pool + slot; the flat kernel keeps a slot's fields inside
// its own 64-byte record, each of the four groups in one 16-byte cell, and its block is a whole number of 64-byte records.
#include <cstdio>
#include <vector>

#include "rt_cold_layout.h"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures++ < 20) {                        \
                std::fprintf(stderr, "FAILED %s: ", #cond); \
                std::fprintf(stderr, __VA_ARGS__);        \
                std::fprintf(stderr, "\n");               \
            }                                             \
        }                                                 \
    } while (0)

int main()
{
    const uint32_t pools[] = {128u, 160u, 192u};
    unsigned long long checked = 0;
    for (int trav = 0; trav <= 6; trav++) {
        for (uint32_t pool : pools) {
            const uint32_t fields = pool_cold_columns(trav), block = pool_wave_cold_dwords(trav, pool);
            std::vector<unsigned char> taken(block, 0);
            for (uint32_t f = 0; f < fields; f++) {
                for (uint32_t s = 0; s < pool; s++) {
                    const uint32_t i = cold_index(trav, pool, f, s);
                    checked++;
                    CHECK(i < block, "trav %d pool %u field %u slot %u: index %u, block %u", trav, pool, f, s, i, block);
                    if (i >= block) continue;
                    CHECK(!taken[i], "trav %d pool %u field %u slot %u: index %u is taken", trav, pool, f, s, i);
                    taken[i] = 1;
                    if (trav != 2) CHECK(i == f * pool + s, "trav %d pool %u field %u slot %u: index %u is not field * pool + slot", trav, pool, f, s, i);
                    else CHECK(i >= 16u * s && i < 16u * s + 16u, "pool %u field %u slot %u: index %u is outside the slot's record", pool, f, s, i);
                }
            }
            if (trav != 2) continue;
            CHECK(fields == 13u, "the flat kernel has %u fields", fields);
            CHECK(block * 4u % 64u == 0u && block == 16u * pool, "pool %u: block of %u dwords", pool, block);
            const uint32_t groups[4][4] = {{C_TX, C_TY, C_TZ, C_LASTPDF}, {C_LX, C_LY, C_LZ, C_OUT}, {C_NEEX, C_NEEY, C_NEEZ, C_NEEZ}, {C_REM_LO, C_REM_HI, C_REM_HI, C_REM_HI}};
            for (uint32_t s = 0; s < pool; s++)
                for (uint32_t g = 0; g < 4u; g++)
                    for (uint32_t k = 0; k < 4u; k++) {
                        const uint32_t i = cold_index(2, pool, groups[g][k], s);
                        CHECK(i / 4u == 4u * s + g, "pool %u slot %u: field %u at %u is not in 16-byte cell %u of the record", pool, s, groups[g][k], i, g);
                    }
        }
    }
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("cold layout ok: %llu indices\n", checked);
    return 0;
}
