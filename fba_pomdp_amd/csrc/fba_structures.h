// fba_structures.h -- what fba_belief_structures (fba_structures.hip) decides about a word list, callable on the host as well: the 64-bit
// hash that keys the table of distinct structures, equality of two word lists, and the order of the top list.  Nothing here knows a record
// format: a word list arrives as a functor m -> uint32.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FBA_HD __host__ __device__ inline
#else
#define FBA_HD inline
#endif

namespace fba {

constexpr uint64_t STRUCT_HASH_FREE = 0;   // the table's mark of a free entry: no word list hashes to it (struct_hash)

// splitmix64's finaliser over the running value and each word in turn; never STRUCT_HASH_FREE.  `keep` is the test hook of the equal-hash
// path: the bits of the hash that count (all of them outside the tests)
template <class Words>
FBA_HD uint64_t struct_hash(const Words& word, int n, uint64_t keep = ~0ull)
{
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
    for (int m = 0; m < n; ++m) {
        h += (uint64_t)word(m) + 0x9E3779B97F4A7C15ull;
        h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
        h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
        h ^= h >> 31;
    }
    h &= keep;
    return h == STRUCT_HASH_FREE ? 1ull : h;
}

// -1 / 0 / +1: word list a before / equal to / behind word list b, word 0 most significant
template <class WordsA, class WordsB>
FBA_HD int struct_compare(const WordsA& a, const WordsB& b, int n)
{
    for (int m = 0; m < n; ++m) {
        const uint32_t x = a(m), y = b(m);
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

// the order of the top list: the larger mass first, among equal masses the smaller word list
template <class WordsA, class WordsB>
FBA_HD bool struct_before(double mass_a, const WordsA& a, double mass_b, const WordsB& b, int n)
{
    if (mass_a != mass_b) return mass_a > mass_b;
    return struct_compare(a, b, n) < 0;
}

}  // namespace fba
