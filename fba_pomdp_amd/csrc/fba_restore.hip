// fba_restore.hip -- the device side of a resumed span (fba_run_bapomdp_span, include/fba_hip.h): while DeviceState::restore_store is set,
// a slot that starts a run takes its run's snapshot block as its filter instead of drawing one from the prior.
//
//   restore_kernel          in init_kernel's place (start_experiment and tick, the FBA_K_BELIEF_INIT bucket): for every slot with need_init,
//                           the records of block (run - run_offset) % restore_nblocks into the slot's live buffer at the block's stride, the
//                           weights beside them.  Moved as snapshot_replicate_kernel moves a filter: 16-byte loads and stores, a wave moves
//                           1 KB of whole lines per instruction, several workgroups per slot; one block (a few MB at most) serves many
//                           slots from L2.  The store places every block so that its record part starts at a multiple of 16 bytes
//                           (snapshot_store_pad, fba_kernels.h): the weights of an odd particle count would leave it at 8
//   restore_post_kernel     what post_init_kernel does behind init_kernel, with the commit of an import: hist_cnt from the header, the slot
//                           no longer compact, no lazy reset pending, need_init cleared
//   span_increments_kernel  validation, before anything runs: no 16-bit increment of a packed record exceeds head.updates
//
// Works under a search budget (slots start their runs in different launches: each launch serves the slots whose flag is up) and with
// compact tiger filters on (the live buffer is written as whole records and the slot says so, as after init_kernel).
#include <algorithm>

#include "fba_kernels_common.h"

namespace fba {

namespace {

// the block of the store that is the filter of slot e's run
__device__ __forceinline__ const uint8_t* restore_block(const Problem& P, const DeviceState& D, int e, int weighted)
{
    const int b = (int)(((long long)D.run[e] - D.run_offset) % D.restore_nblocks);
    return D.restore_store + (size_t)b * (size_t)D.restore_pitch + (size_t)snapshot_store_pad(weighted, P.N);
}

}  // namespace

__global__ void __launch_bounds__(256) restore_kernel(Problem P, DeviceState D)
{
    const int e = D.slot_base + blockIdx.y, tid = threadIdx.x;   // (slot_base: launch_restore's own, a grid's rows at a time)
    if (!D.need_init[e]) return;
    const int weighted = P.belief == FBA_BELIEF_IMPORTANCE ? 1 : 0;
    const uint8_t* blk = restore_block(P, D, e, weighted);
    const fba_snapshot_head* head = reinterpret_cast<const fba_snapshot_head*>(blk);
    const uint8_t* pay = blk + sizeof(fba_snapshot_head);
    const int sel      = D.bufsel[e];
    const uint4* s4    = reinterpret_cast<const uint4*>(pay + (weighted ? (size_t)P.N * 8 : 0));
    uint4* d4          = reinterpret_cast<uint4*>(D.p_rec + rec_base(P, D, e, sel) * (size_t)P.Cs);
    // (the host pass: the stride is a multiple of 16 bytes and at most a whole record, so the pieces stay inside the slot's buffer)
    const size_t n16 = (size_t)P.N * (size_t)(head->stride / 16u), step = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + tid;
    for (; i + 3 * step < n16; i += 4 * step) {   // four loads in flight per lane, then four stores
        const uint4 v0 = s4[i], v1 = s4[i + step], v2 = s4[i + 2 * step], v3 = s4[i + 3 * step];
        d4[i] = v0; d4[i + step] = v1; d4[i + 2 * step] = v2; d4[i + 3 * step] = v3;
    }
    for (; i < n16; i += step) d4[i] = s4[i];
    if (weighted) {   // (8-byte pieces: with an odd particle count neither the store's weights nor the slot's need stand at 16)
        const double* sw = reinterpret_cast<const double*>(pay);
        double* dw       = D.p_weight + pbase(P, e, sel);
        for (size_t k = (size_t)blockIdx.x * 256 + tid; k < (size_t)P.N; k += step) dw[k] = sw[k];
    }
}

__global__ void restore_post_kernel(Problem P, DeviceState D)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P.E || !D.need_init[e]) return;
    if (P.hist) D.hist_cnt[e] = reinterpret_cast<const fba_snapshot_head*>(restore_block(P, D, e, P.belief == FBA_BELIEF_IMPORTANCE ? 1 : 0))->hist_cnt;
    D.compact[e]    = 0;   // restore_kernel has written the live buffer as whole records
    D.lazy_reset[e] = 0;   // (the reset of the span's first episode follows in the same tick)
    D.need_init[e]  = 0;
}

__global__ void __launch_bounds__(256) span_increments_kernel(Problem P, BeliefSnapshotArgs a, int inc_words)
{
    const int b = blockIdx.y;
    const uint32_t* blk = reinterpret_cast<const uint32_t*>(a.stage + (size_t)b * (size_t)a.per_slot);
    const uint32_t most = reinterpret_cast<const fba_snapshot_head*>(blk)->updates;
    const uint32_t* rec = blk + sizeof(fba_snapshot_head) / 4 + (a.weighted ? (size_t)2 * P.N : 0);
    const size_t words  = (size_t)P.N * (size_t)inc_words;
    unsigned long long bad = ~0ull;
    for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (size_t)gridDim.x * 256) {
        const size_t particle = w / (size_t)inc_words;
        const uint32_t v      = rec[particle * (size_t)P.Cs + w % (size_t)inc_words];
        if ((v & 0xffffu) > most || (v >> 16) > most) bad = min(bad, ((unsigned long long)b << 40) | ((unsigned long long)particle << 8) | (unsigned long long)SNAP_BAD_INCREMENT);
    }
    if (bad != ~0ull) atomicMin(a.bad, bad);
}

void launch_restore(const Problem& P, const DeviceState& D, hipStream_t st)
{
    for (int done = 0; done < P.E; done += SNAPSHOT_MAX_SLOTS) {   // (a grid has 65 535 rows at most)
        const int n = std::min(SNAPSHOT_MAX_SLOTS, P.E - done);
        DeviceState Dc = D;
        Dc.slot_base = done;
        // workgroups per slot: 1 024 pieces each, enough to fill the chip at few slots, no more than 8 192 in all at many (as a replicate)
        const size_t want = ((size_t)P.N * (size_t)P.Cs / 4 + 1023) / 1024, cap = (size_t)std::max(1, ceil_div(8192, n));
        const dim3 grid((unsigned)std::max<size_t>(1, std::min(want, cap)), n);
        hipLaunchKernelGGL(restore_kernel, grid, dim3(256), 0, st, P, Dc);
    }
    hipLaunchKernelGGL(restore_post_kernel, dim3(ceil_div(P.E, 256)), dim3(256), 0, st, P, D);
}

void launch_span_increments(const Problem& P, const BeliefSnapshotArgs& a, int inc_words, hipStream_t st)
{
    if (inc_words <= 0 || a.count <= 0) return;
    const size_t want = ((size_t)P.N * (size_t)inc_words + 2047) / 2048, cap = (size_t)std::max(1, ceil_div(8192, a.count));
    const dim3 grid((unsigned)std::max<size_t>(1, std::min(want, cap)), a.count);
    hipLaunchKernelGGL(span_increments_kernel, grid, dim3(256), 0, st, P, a, inc_words);
}

}  // namespace fba
