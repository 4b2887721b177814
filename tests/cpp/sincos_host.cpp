// sincos_host.cpp — rsrt_sincosf against the two functions it fuses (include/rsrt_detmath.h), as uint32, on the CPU.
// Built by tests/test_sincos.py with g++ -O2 -ffp-contract=off.  Prints one line per set of inputs:
//   <set> checked <n> mismatches <m> first <hex pattern of the first failing input, 0 if none>
// and returns 1 if any input failed.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "rsrt_detmath.h"

static inline uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float flt(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

struct Tally {
    uint64_t checked = 0, bad = 0;
    uint32_t first = 0;
    void one(uint32_t pattern)
    {
        // (volatile: the compiler must not fold the three calls into one evaluation)
        volatile float x = flt(pattern);
        float s, c;
        rsrt_sincosf(x, &s, &c);
        const uint32_t ws = bits(rsrt_sinf(x)), wc = bits(rsrt_cosf(x));
        checked++;
        if (bits(s) != ws || bits(c) != wc) {
            if (bad == 0) first = pattern;
            bad++;
        }
    }
    bool report(const char *name) const
    {
        printf("%s checked %llu mismatches %llu first %08x\n", name, (unsigned long long)checked, (unsigned long long)bad, first);
        return bad == 0;
    }
};

// every pattern within +-ulps of the pattern of v, both signs of v
static void around(Tally &t, float v, uint32_t ulps)
{
    for (int sign = 0; sign < 2; sign++) {
        const uint32_t centre = bits(v) | (sign ? 0x80000000u : 0u);
        const uint32_t mag = centre & 0x7fffffffu;
        const uint32_t lo = mag > ulps ? mag - ulps : 0u;
        for (uint32_t m = lo; m <= mag + ulps; m++) t.one((centre & 0x80000000u) | m);
    }
}

int main()
{
    bool ok = true;
    {
        Tally t; // every 37th of all 2^32 bit patterns
        for (uint64_t p = 0; p < (1ull << 32); p += 37) t.one((uint32_t)p);
        ok &= t.report("stride37");
    }
    {
        Tally t; // +-4096 ulps of k pi / 4, k = 0 .. 64, either sign (the octant borders)
        for (int k = 0; k <= 64; k++) around(t, (float)((double)k * 0.78539816339744830962), 4096u);
        ok &= t.report("octants");
    }
    {
        Tally t; // +-4096 ulps of +-8192 (the range check)
        around(t, 8192.0f, 4096u);
        ok &= t.report("range");
    }
    {
        Tally t; // +-0, the smallest subnormals, the largest, the smallest normal, +-inf, NaNs of either sign, quiet and signalling
        const uint32_t s[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x00000002u, 0x80000002u, 0x007fffffu, 0x807fffffu,
                              0x00800000u, 0x80800000u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u,
                              0x7f800001u, 0xff800001u, 0x7fffffffu, 0xffffffffu};
        for (uint32_t p : s) t.one(p);
        ok &= t.report("special");
    }
    return ok ? 0 : 1;
}
