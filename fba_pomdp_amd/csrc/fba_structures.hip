// fba_structures.hip -- fba_belief_structures: the posterior over whole model graphs of a range of slots, reduced on the device from
// whatever record format the context stores (dense fp32, packed factored tiger, gridworld history records).
//
//   structures_kernel   one workgroup per slot: weight total, mass per (word, parent set), mass per query, the table of distinct
//                       structures and its top list
//
// A translation unit of its own, as fba_summary.hip is: nothing here is on the parity path (the order of the fp64 additions is the
// hardware's), and the code generation of the search and belief kernels stays what it was.  Read-only on every buffer of the context.
//
// LDS of a workgroup: the table (STRUCT_TABLE entries of hash, mass, representative: 40 KB), STRUCT_HIST_CELLS histogram cells (8 KB)
// and STRUCT_QUERY_LDS query masses (8 KB) -- 56 KB and a little, so that two workgroups share a CU's 160 KB.
#include "fba_structures_table.h"

namespace fba {

constexpr int STRUCT_BLOCK = 256;
static_assert((STRUCT_TABLE & (STRUCT_TABLE - 1)) == 0, "a probe wraps with a mask");

// Dynamic LDS: [STRUCT_TABLE] hashes, [STRUCT_TABLE] masses, [STRUCT_HIST_CELLS] histogram, [STRUCT_QUERY_LDS] query masses (doubles and
// 64-bit words), then [STRUCT_TABLE] representatives (int).
__global__ void __launch_bounds__(STRUCT_BLOCK) structures_kernel(Problem P, DeviceState D, BeliefStructuresArgs a)
{
    extern __shared__ double s_dyn[];
    __shared__ double s_tot[2];          // weight total, unplaced mass
    __shared__ int s_flag[2];            // overflow, distinct
    __shared__ int s_best[STRUCT_BLOCK];
    unsigned long long* s_hash = reinterpret_cast<unsigned long long*>(s_dyn);
    double* s_mass = s_dyn + STRUCT_TABLE;
    double* s_hist = s_mass + STRUCT_TABLE;
    double* s_qm   = s_hist + STRUCT_HIST_CELLS;
    int* s_rep     = reinterpret_cast<int*>(s_qm + STRUCT_QUERY_LDS);   // >= 0: the particle whose words the entry stands for; -1: none yet; < -1: taken by the top list

    const int b = blockIdx.x, e = a.first + b, tid = threadIdx.x;
    const int nw = a.n_words, ns = a.n_sets, nk = a.n_keys;
    const int tile  = min(nw, STRUCT_HIST_CELLS / ns);   // words whose histograms one pass keeps (n_sets <= 256: four at least)
    const int q_lds = min(a.nq, STRUCT_QUERY_LDS);
    for (int k = tid; k < STRUCT_TABLE; k += STRUCT_BLOCK) { s_hash[k] = STRUCT_HASH_FREE; s_mass[k] = 0.0; s_rep[k] = -1; }
    for (int k = tid; k < STRUCT_HIST_CELLS; k += STRUCT_BLOCK) s_hist[k] = 0.0;
    for (int k = tid; k < STRUCT_QUERY_LDS; k += STRUCT_BLOCK) s_qm[k] = 0.0;
    if (tid < 2) { s_tot[tid] = 0.0; s_flag[tid] = 0; }
    __syncthreads();

    const SlotRecs r = slot_recs(P, D, e);
    BeliefSummaryArgs sa{};   // (record_mask_word asks it where the words stand)
    sa.ncounts = a.ncounts;

    // ---- first pass over the slot: weight total, the histograms of the first `tile` words, the queries, the table
    double lw = 0.0;
    for (int base = 0; base < P.N; base += STRUCT_BLOCK) {   // (every thread makes every trip: the table's rounds hold barriers)
        const int i     = base + tid;
        const bool live = i < P.N;
        const float* rec = r.rec + (size_t)(live ? i : 0) * r.stride;
        const double w   = live ? particle_weight(P, D, r, i) : 0.0;
        const auto key   = [&](int m) { return record_key_word(P, nw, a.ncounts, rec, m); };
        lw += w;
        if (live) {
            if (a.set_mass)
                for (int m = 0; m < tile; ++m) {
                    const uint32_t v = record_mask_word(P, sa, rec, m);
                    if (v < (uint32_t)ns) unsafeAtomicAdd(&s_hist[m * ns + (int)v], w);
                }
            if (a.query_mass)
                for (int q = 0; q < a.nq; ++q) {
                    const uint32_t* qw = a.query + (size_t)q * nk;
                    bool same = true;
                    for (int m = 0; m < nk && same; ++m) same = key(m) == qw[m];
                    if (same) {
                        if (q < q_lds) unsafeAtomicAdd(&s_qm[q], w);
                        else unsafeAtomicAdd(&a.query_mass[(size_t)b * a.nq + q], w);
                    }
                }
        }
        // The table (struct_table_rounds, fba_structures_table.h): claim a free entry with the hash, or find the entry of that hash whose
        // representative holds the same words
        const unsigned long long h = live ? struct_hash(key, nk, a.hash_keep) : 0ull;
        struct_table_rounds<STRUCT_TABLE>(s_hash, s_mass, s_rep, &s_tot[1], &s_flag[0], live, i, w, h, key,
                                          [&](int rp, int m) { return record_key_word(P, nw, a.ncounts, r.rec + (size_t)rp * r.stride, m); }, nk);
    }
    unsafeAtomicAdd(&s_tot[0], lw);
    __syncthreads();
    if (a.query_mass)
        for (int q = tid; q < q_lds; q += STRUCT_BLOCK) a.query_mass[(size_t)b * a.nq + q] = s_qm[q];

    // ---- the histograms: the first tile is there, each further one is a pass of its own
    if (a.set_mass) {
        double* out = a.set_mass + (size_t)b * nw * ns;
        for (int m0 = 0; m0 < nw; m0 += tile) {
            const int mw = min(tile, nw - m0);
            if (m0 > 0) {
                __syncthreads();
                for (int k = tid; k < mw * ns; k += STRUCT_BLOCK) s_hist[k] = 0.0;
                __syncthreads();
                for (int i = tid; i < P.N; i += STRUCT_BLOCK) {
                    const float* rec = r.rec + (size_t)i * r.stride;
                    const double w   = particle_weight(P, D, r, i);
                    for (int m = 0; m < mw; ++m) {
                        const uint32_t v = record_mask_word(P, sa, rec, m0 + m);
                        if (v < (uint32_t)ns) unsafeAtomicAdd(&s_hist[m * ns + (int)v], w);
                    }
                }
                __syncthreads();
            }
            for (int k = tid; k < mw * ns; k += STRUCT_BLOCK) out[(size_t)m0 * ns + k] = s_hist[k];
        }
    }

    // ---- the table: how many structures, and the top list by repeated arg-max (the order needs the representatives' words: read again)
    int mine = 0;
    for (int k = tid; k < STRUCT_TABLE; k += STRUCT_BLOCK) mine += s_hash[k] != STRUCT_HASH_FREE ? 1 : 0;
    if (mine) atomicAdd(&s_flag[1], mine);
    __syncthreads();
    const int distinct = s_flag[1], stored = min(a.top_k, distinct);
    if (tid == 0) {
        fba_structure_head hd;
        hd.weight_total = s_tot[0]; hd.unplaced_mass = s_tot[1];
        hd.distinct = distinct; hd.overflow = s_flag[0]; hd.stored = stored; hd.reserved = 0;
        a.head[b] = hd;
    }
    if (!a.top_words && !a.top_mass) return;
    const auto before = [&](int x, int y) {   // entry x stands before entry y in the top list
        const float* rx = r.rec + (size_t)s_rep[x] * r.stride;
        const float* ry = r.rec + (size_t)s_rep[y] * r.stride;
        return struct_before(s_mass[x], [&](int m) { return record_mask_word(P, sa, rx, m); }, s_mass[y], [&](int m) { return record_mask_word(P, sa, ry, m); }, nw);
    };
    for (int k = 0; k < a.top_k; ++k) {
        uint32_t* tw = a.top_words ? a.top_words + ((size_t)b * a.top_k + k) * nw : nullptr;
        if (k >= stored) {   // rows behind `stored` are zero
            if (tw) for (int m = tid; m < nw; m += STRUCT_BLOCK) tw[m] = 0u;
            if (a.top_mass && tid == 0) a.top_mass[(size_t)b * a.top_k + k] = 0.0;
            continue;
        }
        int best = -1;
        for (int j = tid; j < STRUCT_TABLE; j += STRUCT_BLOCK)
            if (s_rep[j] >= 0 && (best < 0 || before(j, best))) best = j;
        s_best[tid] = best;
        __syncthreads();
        for (int s = STRUCT_BLOCK / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const int x = s_best[tid + s], y = s_best[tid];
                if (x >= 0 && (y < 0 || before(x, y))) s_best[tid] = x;
            }
            __syncthreads();
        }
        const int win = s_best[0];   // (k < stored: an entry is left)
        if (win < 0) break;
        const int rep     = s_rep[win];
        const double mass = s_mass[win];
        __syncthreads();
        if (tw) {
            const float* rw = r.rec + (size_t)rep * r.stride;
            for (int m = tid; m < nw; m += STRUCT_BLOCK) tw[m] = record_mask_word(P, sa, rw, m);
        }
        if (tid == 0) {
            if (a.top_mass) a.top_mass[(size_t)b * a.top_k + k] = mass;
            s_rep[win] = -2 - rep;
        }
        __syncthreads();
    }
}

void launch_belief_structures(const Problem& P, const DeviceState& D, const BeliefStructuresArgs& a, hipStream_t st)
{
    const size_t lds = ((size_t)2 * STRUCT_TABLE + STRUCT_HIST_CELLS + STRUCT_QUERY_LDS) * sizeof(double) + (size_t)STRUCT_TABLE * sizeof(int);
    hipLaunchKernelGGL(structures_kernel, dim3(a.count), dim3(STRUCT_BLOCK), lds, st, P, D, a);
}

}  // namespace fba
