// high_base.h - where a checker that owns its words buffer puts its first base.  The checkers lay their sequences out from base 0; with a first-base argument
// the buffer really is that large and every position the cores receive is shifted, so an int, a u32 or a 2 * g in 32 bits between a job and load32 shows:
//   a number    that base
//   straddle    base 2^31 falls in the middle of the checker's `total` bases, and the first base is 13 modulo 32
//   top         the last base is 2^32 - 2: the bases end where the largest volume ends (2^32 - 1 bases)
// No argument (nullptr): 0, as before.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace high_base {

inline uint64_t first_base(const char* arg, uint64_t total)
{
    if (!arg || !*arg) return 0;
    if (!strcmp(arg, "top")) return (1ULL << 32) - 1 - total;
    if (!strcmp(arg, "straddle")) {
        uint64_t f = (1ULL << 31) - total / 2;
        f -= (f + 32 - 13) % 32;          // 13 modulo 32, at most 31 bases earlier
        if (!(f < (1ULL << 31) && (1ULL << 31) < f + total)) { fprintf(stderr, "high_base: %llu bases cannot straddle 2^31\n", (unsigned long long)total); exit(2); }
        return f;
    }
    char* end = nullptr;
    const uint64_t f = strtoull(arg, &end, 10);
    if (!end || *end) { fprintf(stderr, "high_base: first base '%s' is neither a number, straddle nor top\n", arg); exit(2); }
    return f;
}

}  // namespace high_base
