// fba_structures_table.h -- what structures_kernel (fba_structures.hip) and struct_stats_slot_kernel (fba_structure_stats.hip) must agree
// on, defined once: the key word of a record (what identifies its structure, whatever the record format) and the claim-or-find rounds of
// the per-slot table of distinct structures in LDS.  Device code only.
#pragma once

#include "fba_kernels_common.h"
#include "fba_structures.h"

namespace fba {

// word m of what identifies a record's structure: the words themselves, or -- history records -- the bits of rec[1] that stand for them
// (one key word; record_mask_word expands bit m to the word 3 or 7 on output)
__device__ __forceinline__ uint32_t record_key_word(const Problem& P, int n_words, int ncounts, const float* rec, int m)
{
    if (P.hist) return __float_as_uint(rec[1]) & ((1u << n_words) - 1u);
    if (P.ft_packed) return __float_as_uint(rec[ncounts / 2]);
    return __float_as_uint(rec[ncounts + m]);
}

// One trip of a workgroup through the table, every thread with one particle (`live`: the thread has one; i its index, w its weight, h the
// hash of its key words key(0..nk)).  Claim a free entry with the hash, or find the entry of that hash whose representative holds the same
// words; two structures of one hash are two entries.  A thread never waits for another: where an entry's owner has not named the
// representative yet, the thread leaves the round, and the barrier between rounds makes the name visible.  rep_key(p, m): key word m of
// particle p.  s_mass (the mass per entry) and s_unplaced (the weight that found no place) may be null where the caller wants neither;
// *s_overflow is set where every entry holds another structure.  EVERY thread of the workgroup makes the call: the rounds hold barriers.
template <int TABLE, class Key, class RepKey>
__device__ __forceinline__ void struct_table_rounds(unsigned long long* s_hash, double* s_mass, int* s_rep, double* s_unplaced, int* s_overflow,
                                                    bool live, int i, double w, unsigned long long h, const Key& key, const RepKey& rep_key, int nk)
{
    static_assert((TABLE & (TABLE - 1)) == 0, "a probe wraps with a mask");
    uint32_t pos = (uint32_t)(h >> 20) & (TABLE - 1);
    int probes   = 0;
    bool pending = live;
    for (;;) {
        while (pending) {
            if (probes == TABLE) {   // every entry holds another structure
                if (s_unplaced) unsafeAtomicAdd(s_unplaced, w);
                *s_overflow = 1;
                pending     = false;
                break;
            }
            const unsigned long long old = atomicCAS(&s_hash[pos], (unsigned long long)STRUCT_HASH_FREE, h);
            if (old == STRUCT_HASH_FREE) {
                reinterpret_cast<volatile int*>(s_rep)[pos] = i;
                if (s_mass) unsafeAtomicAdd(&s_mass[pos], w);
                pending = false;
                break;
            }
            if (old == h) {
                const int rp = reinterpret_cast<volatile int*>(s_rep)[pos];
                if (rp < 0) break;   // (next round)
                bool same = true;
                for (int m = 0; m < nk && same; ++m) same = key(m) == rep_key(rp, m);
                if (same) {
                    if (s_mass) unsafeAtomicAdd(&s_mass[pos], w);
                    pending = false;
                    break;
                }
            }
            pos = (pos + 1) & (TABLE - 1);
            ++probes;
        }
        if (!__syncthreads_or(pending ? 1 : 0)) break;
    }
}

}  // namespace fba
