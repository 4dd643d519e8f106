// tungsten_amd/csrc/hip/pt_libm.h's sinhfCore -- the device's restatement of glibc's sinhf, compiled here for the host as oracle/libm_host.cpp
// compiles the header -- against the host libm's sinhf on EVERY float32 of its restated domain (0, 10]: bit patterns 1 .. 0x41200000.
// Prints the number of arguments and the number whose results differ in any bit (which must be 0), the first few of them, and what the
// function returns outside the domain; exits 1 when anything differs.
//   g++ -std=c++17 -O2 -ffp-contract=off tools/libm_sinhf_sweep.cpp -o build/libm_sinhf_sweep -lm && build/libm_sinhf_sweep
// (once with -fsanitize=address,undefined as well: profiles/fibre_libm_sinhf_sweep.txt holds both runs)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#define PT_LIBM_FN static inline
#define PT_LIBM_TABLE static const
#include "../tungsten_amd/csrc/hip/pt_libm.h"

int main()
{
    const uint32_t first = 1u, last = 0x41200000u;       // the smallest subnormal .. 10.0f
    unsigned long long tested = 0, bad = 0;
    for (uint32_t u = first; u <= last; ++u) {
        float x, got, want;
        memcpy(&x, &u, 4);
        got = ptlibm::sinhfCore(x);
        want = sinhf(x);
        ++tested;
        if (memcmp(&got, &want, 4) != 0) {
            if (bad < 8) printf("  differs: x = %a (0x%08x): restated %a, libm %a\n", x, u, got, want);
            ++bad;
        }
    }
    // outside the domain: NaN, never a wrong number
    const float outside[] = {0.0f, -0.0f, -1.0f, 0x1.400002p+3f, 22.0f, 100.0f, __builtin_huge_valf(), -__builtin_huge_valf(), __builtin_nanf("")};
    unsigned long long outsideBad = 0;
    for (float x : outside) {
        const float got = ptlibm::sinhfCore(x);
        if (got == got) { printf("  outside the domain: x = %a gives %a, not NaN\n", x, got); ++outsideBad; }
    }
    printf("sinhf on (0, 10]: %llu floats tested, %llu differences from the host libm; %llu of %zu arguments outside the domain not NaN\n",
           tested, bad, outsideBad, sizeof(outside)/sizeof(outside[0]));
    return bad || outsideBad ? 1 : 0;
}
