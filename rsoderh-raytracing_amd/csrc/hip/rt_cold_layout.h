// rt_cold_layout.h — where a pool slot's cold path state lies in a wave's block of the arena (rt_wavepool.h): the fields, how many
// dwords a wave's block holds, and the one function that turns (traversal, pool size, field, slot) into a dword index.
// Plain C++17: no HIP header, no runtime call — the kernel, the host code that sizes the arena (rsrt_api.hip) and a CPU test
// (tests/cpp/cold_layout_host.cpp) read the same lines.
//
// Two layouts.
//   The walks (TRAV 0, 1, 3, 4, 5, 6): one contiguous column per field and wave, field * pool + slot.  Their per-ray columns (the hit
//   record, the wide walk's parked stack) are touched by single rays at single times; nothing groups them.
//   The flat kernel (TRAV 2): one 64-byte-aligned record of sixteen dwords per slot, at slot * 16.  A stage trip runs 64 of a pool's
//   192 slots in ascending slot order — about one slot in three — so a column store of 256 payload bytes dirtied all twelve 64-byte
//   segments of a 768-byte column, and SHADE's ten columns about 120 segments (7.7 KB) for 2.5 KB of payload; the arena does not fit
//   the L2, and what is dirtied goes out over the fabric (profiles/lazy_nee_ab.txt: 1.8 and 2.4 times the payload).  With a record a
//   slot the same trip dirties 64 segments and fills most of each, the stage reads and writes the same lines, and every field of a
//   slot is within 64 bytes of one address.  The fields are grouped into 16-byte quads by who touches them together:
//     quad 0   T.x T.y T.z last_pdf      read by SHADE, MISS            written by SHADE when the path continues
//     quad 1   L.x L.y L.z out_slot      read by SHADE, MISS, FINISH    written whole by SHADE: L, and out_slot as loaded — or, at a
//                                                                       path's first vertex, from the hot cell GEN left it in
//     quad 2   NEE.x NEE.y NEE.z -       read by SHADE, MISS, FINISH    written by SHADE when the term counts
//     quad 3   REM_LO REM_HI - -         read by a resumed TRACE        written for a ray the triangle-loop vote cut short
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_LAYOUT_FN __host__ __device__ constexpr
#else
#define RT_LAYOUT_FN constexpr
#endif

enum ColdField {
    C_TX, C_TY, C_TZ, C_LX, C_LY, C_LZ, C_NEEX, C_NEEY, C_NEEZ, C_LASTPDF, C_OUT,
    C_RNG, // (the flat traversal keeps it in a hot cell)
    C_BOUNCE,
    C_REF, // tree-walk traversals only: best hit of the extension ray, record | source << 30
    C_COUNT,
    // the flat traversal stops early: its bounce count and hit record ride in the idle cursor bits of H_CT; two words
    // hold the untested triangles of a ray whose triangle loop was cut short (only such rays touch them)
    C_REM_LO = C_RNG, C_REM_HI = C_BOUNCE,
    C_COUNT_FLAT = C_REF
};

// What sizes the walks' extra columns and the cooperative walk's overflow block.  rt_wavepool.h asserts that these are the walks' own
// constants (rt_device.h: RT_WSTACK, RT_WSTATE_WORDS; rt_coop.h: RT_COOP_GCAP).
constexpr uint32_t kColdWideStack = 8u;        // the wide walk's register stack
constexpr uint32_t kColdWideStateWords = 27u;  // next node, pending group, the register stack, overflow count, 16 overflow words
constexpr uint32_t kColdCoopOverflow = 4096u;  // node items a wave of the cooperative walk may spill to its arena block
constexpr uint32_t kColdRecordDwords = 16u;    // TRAV 2: a slot's record, 64 bytes

// the wide walk parks an unfinished ray's stack in columns of its own, and a deep tree's walk keeps the bottom of its stack there
// (kColdWideStateWords columns, rt_device.h WalkState); only such rays touch them
#define C_WIDE_STATE ((uint32_t)C_COUNT)
#define C_COUNT_WIDE ((uint32_t)C_COUNT + 2u + kColdWideStack)   /* TRAV 4: next node, pending group, the register stack */
#define C_COUNT_WIDE_DEEP ((uint32_t)C_COUNT + kColdWideStateWords) /* TRAV 5: + overflow count and overflow words */

// how many fields a slot has (the walks: as many columns)
RT_LAYOUT_FN uint32_t pool_cold_columns(int trav)
{
    // (6, the cooperative walk: no C_REF — the hit's record waits in the slot's hot result cell — and nothing parked)
    return trav == 2 ? (uint32_t)C_COUNT_FLAT : (trav == 4 ? C_COUNT_WIDE : (trav == 5 ? C_COUNT_WIDE_DEEP : (trav == 6 ? (uint32_t)C_REF : (uint32_t)C_COUNT)));
}

// a wave's block of the arena, in dwords
RT_LAYOUT_FN uint32_t pool_wave_cold_dwords(int trav, uint32_t pool)
{
    return trav == 2 ? kColdRecordDwords * pool : pool_cold_columns(trav) * pool + (trav == 6 ? kColdCoopOverflow : 0u);
}

// TRAV 2: the dword of a slot's record that holds `field` (field < C_COUNT_FLAT)
RT_LAYOUT_FN uint32_t cold_record_dword(uint32_t field)
{
    return field <= (uint32_t)C_TZ     ? field                          // quad 0: T
           : field <= (uint32_t)C_LZ   ? field + 1u                     // quad 1: L
           : field <= (uint32_t)C_NEEZ ? field + 2u                     // quad 2: NEE
           : field == (uint32_t)C_LASTPDF ? 3u                          // quad 0, with T
           : field == (uint32_t)C_OUT  ? 7u                             // quad 1, with L
                                       : field + 1u;                    // quad 3: REM_LO, REM_HI
}

// the dword index of `field` of `slot` in a wave's block
RT_LAYOUT_FN uint32_t cold_index(int trav, uint32_t pool, uint32_t field, uint32_t slot)
{
    return trav == 2 ? slot * kColdRecordDwords + cold_record_dword(field) : field * pool + slot;
}

namespace cold_layout_checks {
constexpr bool same_quad(uint32_t a, uint32_t b) { return cold_record_dword(a) / 4u == cold_record_dword(b) / 4u; }
constexpr bool record_is_injective()
{
    uint32_t seen = 0u;
    for (uint32_t f = 0; f < (uint32_t)C_COUNT_FLAT; f++) {
        const uint32_t d = cold_record_dword(f);
        if (d >= kColdRecordDwords || (seen >> d & 1u)) return false;
        seen |= 1u << d;
    }
    return true;
}
static_assert(record_is_injective(), "every field of the flat kernel has a dword of its own inside the 16-dword record");
static_assert(same_quad(C_TX, C_TY) && same_quad(C_TX, C_TZ) && same_quad(C_TX, C_LASTPDF) && cold_record_dword(C_TX) / 4u == 0u, "quad 0: T and last_pdf");
static_assert(same_quad(C_LX, C_LY) && same_quad(C_LX, C_LZ) && same_quad(C_LX, C_OUT) && cold_record_dword(C_LX) / 4u == 1u, "quad 1: L and out_slot");
static_assert(same_quad(C_NEEX, C_NEEY) && same_quad(C_NEEX, C_NEEZ) && cold_record_dword(C_NEEX) / 4u == 2u, "quad 2: the pending NEE term");
static_assert(same_quad(C_REM_LO, C_REM_HI) && cold_record_dword(C_REM_LO) / 4u == 3u, "quad 3: the triangles a cut-short ray has left");
static_assert(cold_record_dword(C_TX) % 4u == 0u && cold_record_dword(C_LX) % 4u == 0u && cold_record_dword(C_NEEX) % 4u == 0u && cold_record_dword(C_REM_LO) % 4u == 0u,
              "a quad's first field is 16-byte aligned");
static_assert(pool_wave_cold_dwords(2, 192u) % 16u == 0u && pool_wave_cold_dwords(2, 160u) % 16u == 0u && pool_wave_cold_dwords(2, 128u) % 16u == 0u,
              "a wave's block is a whole number of 64-byte records: every record is 64-byte aligned in a 64-byte-aligned arena");
static_assert(cold_index(2, 192u, C_REM_HI, 191u) < pool_wave_cold_dwords(2, 192u) && cold_index(2, 160u, C_REM_HI, 159u) < pool_wave_cold_dwords(2, 160u), "inside the block");
static_assert(cold_index(0, 192u, C_REF, 5u) == (uint32_t)C_REF * 192u + 5u && cold_index(5, 128u, C_COUNT_WIDE_DEEP - 1u, 127u) == pool_wave_cold_dwords(5, 128u) - 1u,
              "the walks keep one column per field");
} // namespace cold_layout_checks
