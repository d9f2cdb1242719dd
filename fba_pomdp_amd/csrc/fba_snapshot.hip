// fba_snapshot.hip -- belief snapshots (fba_belief_export / _import / _replicate): the main filter of a slot moved as the records the
// context stores, between the layout only the kernels know (the live buffer behind bufsel or rec_buf, records at the stride hist_cnt
// implies) and the flat block of include/fba_hip.h: fba_snapshot_head | weights | records at the slot's current stride | zeros.
//
//   snapshot_pack_kernel       export: the live weights and records of a slot into its block of the staging buffer, dead words as zeros,
//                              and the block's checksum -- a sum modulo 2^64, reduced per wave, per workgroup, then one atomic
//   snapshot_validate_kernel   import, first pass over the staged blocks: the checksum again, and every word of every record judged by what
//                              it is (weight, state, structure word, count, history entry); the first offender leaves through an error word
//                              of the call's own (atomicMin), never through DeviceState::fault.  Writes nothing of the context
//   snapshot_commit_kernel     import, second pass: weights and records into the slot's live buffers at the block's stride, hist_cnt set,
//                              lazy_reset cleared
//   snapshot_replicate_kernel  one slot's filter into many, device to device: 16-byte loads and stores, a wave moves 1 KB of whole lines
//                              per instruction, the source (a few MB at most) stays in L2; several workgroups per destination slot
//
// Word-wise on the staging side: a block's record part is only 8-byte aligned when the particle count is odd.  A translation unit of its
// own: nothing here is on the path of a tick.
#include <algorithm>

#include "fba_kernels_common.h"

namespace fba {

namespace {

constexpr int SNAP_HEAD_WORDS = (int)(sizeof(fba_snapshot_head) / 4);
static_assert(sizeof(fba_snapshot_head) == 64, "a snapshot block starts with 64 bytes of header");

// the live buffers of slot e (what slot_recs finds for a reader, writable)
__device__ __forceinline__ float* live_records(const Problem& P, const DeviceState& D, int e) { return D.p_rec + rec_base(P, D, e, D.bufsel[e]) * (size_t)P.Cs; }
__device__ __forceinline__ double* live_weights(const Problem& P, const DeviceState& D, int e) { return D.p_weight + pbase(P, e, D.bufsel[e]); }

}  // namespace

__global__ void __launch_bounds__(256) snapshot_pack_kernel(Problem P, DeviceState D, BeliefSnapshotArgs a)
{
    const int b = blockIdx.y, e = a.first + b, tid = threadIdx.x;
    const SlotRecs r = slot_recs(P, D, e);
    uint32_t* out       = reinterpret_cast<uint32_t*>(a.stage + (size_t)b * (size_t)a.per_slot) + SNAP_HEAD_WORDS;
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(r.rec);
    const uint32_t* wts = reinterpret_cast<const uint32_t*>(D.p_weight + r.wb);
    const size_t ww = a.weighted ? (size_t)2 * P.N : 0, live = (size_t)P.N * (size_t)r.stride, words = ww + (size_t)P.N * (size_t)P.Cs;
    const int alive = P.hist ? 2 + hist_total(r.cnt) : P.C + 1;   // words of a record that say something: the rest leaves as zeros
    unsigned long long sum = 0;
    for (size_t w = (size_t)blockIdx.x * 256 + tid; w < words; w += (size_t)gridDim.x * 256) {
        uint32_t v = 0;
        if (w < ww) v = wts[w];
        else {
            const size_t q = w - ww;
            if (q < live && (int)(q % (size_t)r.stride) < alive) v = rec[q];
        }
        out[w] = v;
        sum += check_term(v, w);
    }
    block_check_add(sum, a.check + b);
}

// x, y and goal of a packed gridworld state inside the grid
__device__ __forceinline__ bool gw_fields_ok(uint32_t sp, int N, int G) { return sp < 1024u && hist_x(sp) < N && hist_y(sp) < N && hist_g(sp) < G; }

// FMT: the record format as with_record_format numbers it; the packed formats (1..4) are judged alike and run as 1
template <int FMT>
__global__ void __launch_bounds__(256) snapshot_validate_kernel(Problem P, DeviceState D, BeliefSnapshotArgs a)
{
    constexpr int HIST = FMT > 4 ? FMT - 4 : 0;
    const int b = blockIdx.y, tid = threadIdx.x;
    const uint32_t* blk = reinterpret_cast<const uint32_t*>(a.stage + (size_t)b * (size_t)a.per_slot);
    const fba_snapshot_head* head = reinterpret_cast<const fba_snapshot_head*>(blk);
    const uint32_t* in = blk + SNAP_HEAD_WORDS;
    // (the host pass has checked both against the context: the stride is that of the total, the total fits a record)
    const uint32_t cnt = head->hist_cnt;
    const int stride = (int)(head->stride / 4u), total = HIST ? hist_total(cnt) : 0;
    const size_t ww = a.weighted ? (size_t)2 * P.N : 0, live = (size_t)P.N * (size_t)stride, words = ww + (size_t)P.N * (size_t)P.Cs;
    HistDims dims{};
    if (HIST) dims = hist_dims<(HIST ? HIST : 1)>(P, P.ca);
    unsigned long long sum = 0, bad = ~0ull;
    for (size_t w = (size_t)blockIdx.x * 256 + tid; w < words; w += (size_t)gridDim.x * 256) {
        const uint32_t v = in[w];
        sum += check_term(v, w);
        int what = 0;
        size_t particle = 0;
        if (w < ww) {
            particle = w >> 1;
            if (!(w & 1)) {
                const double x = __hiloint2double((int)in[w + 1], (int)v);
                if (!(x >= 0.0 && x < (double)INFINITY)) what = SNAP_BAD_WEIGHT;
            }
        } else if (w - ww < live) {
            const size_t q = w - ww;
            particle    = q / (size_t)stride;
            const int k = (int)(q % (size_t)stride);
            if (k == P.C) {
                if (v >= (uint32_t)P.S) what = SNAP_BAD_STATE;
            } else if (HIST) {
                if (k == 1) {
                    if (HIST == 1) {   // structure bits of the x / y nodes, the state once more as hist_pack: the search and the update step from it
                        const uint32_t s = in[w - 1];
                        if ((v & 0xffffu) >> (2 * P.A)) what = SNAP_BAD_STRUCTURE;
                        else if (s < (uint32_t)P.S && (v >> 16) != gridworld_pack_state(P, (int)s)) what = SNAP_BAD_STATE;
                    }
                } else if (k < 2 + total) {
                    const int j = k - 2;
                    int act = 0;
                    for (int c = 1; c < 4; ++c) act += j >= hist_offset(cnt, c) ? 1 : 0;   // (groups in action order; the host pass: none beyond A)
                    bool ok;
                    if (HIST == 1) ok = v < (1u << 30) && gw_fields_ok(v & 0x3ffu, dims.N, dims.G) && gw_fields_ok((v >> 10) & 0x3ffu, dims.N, dims.G) &&
                                        gw_fields_ok(v >> 20, dims.N, dims.G);
                    else if (HIST == 2) ok = (v & 0x3ffu) < (uint32_t)P.S && ((v >> 10) & 0x3ffu) < (uint32_t)P.S && (v >> 20) < (uint32_t)P.O;
                    else {
                        ok = (int)(v & 7u) < dims.W && (int)((v >> 3) & 7u) < dims.W && (int)((v >> 6) & 7u) < dims.H && (int)((v >> 9) & 7u) < dims.H;
                        for (int c = 0; c < 2; ++c) {
                            const uint32_t f = v >> (12 + 9 * c);
                            if (c < dims.n) ok = ok && (int)(f & 7u) < dims.H && (int)((f >> 3) & 7u) < dims.H && (int)((f >> 6) & 7u) < dims.H;
                        }
                    }
                    if (ok) {   // ... and through the engine's own decoding: every cell the entry raises lies inside the table
                        int cells[HIST_ENTRY_CELLS];
                        hist_entry_cells<(HIST ? HIST : 1)>(dims, in[w - (size_t)k + 1], act, v, cells);
#pragma unroll
                        for (int c = 0; c < HIST_ENTRY_CELLS; ++c) ok = ok && cells[c] >= -1 && cells[c] < a.ncells;
                    }
                    if (!ok) what = SNAP_BAD_ENTRY;
                }
            } else if (FMT == 0 && k < a.ncounts) {
                const float x = __uint_as_float(v);
                if (!(x >= 0.f && x < INFINITY)) what = SNAP_BAD_COUNT;
            } else if (a.nvar > 0 && k >= a.mask_at && k < a.mask_at + a.nvar && k < P.C) {
                if (v >= a.mask_limit[k - a.mask_at]) what = SNAP_BAD_STRUCTURE;
            }
        }
        if (what) bad = min(bad, ((unsigned long long)b << 40) | ((unsigned long long)particle << 8) | (unsigned long long)what);
    }
    if (bad != ~0ull) atomicMin(a.bad, bad);
    block_check_add(sum, a.check + b);
}

__global__ void __launch_bounds__(256) snapshot_commit_kernel(Problem P, DeviceState D, BeliefSnapshotArgs a)
{
    const int b = blockIdx.y, e = a.first + b, tid = threadIdx.x;
    const uint32_t* blk = reinterpret_cast<const uint32_t*>(a.stage + (size_t)b * (size_t)a.per_slot);
    const fba_snapshot_head* head = reinterpret_cast<const fba_snapshot_head*>(blk);
    const uint32_t* in = blk + SNAP_HEAD_WORDS;
    const size_t ww = a.weighted ? (size_t)2 * P.N : 0, live = (size_t)P.N * (size_t)(head->stride / 4u);   // live <= N * Cs: the host pass
    uint32_t* rec = reinterpret_cast<uint32_t*>(live_records(P, D, e));
    uint32_t* wts = reinterpret_cast<uint32_t*>(live_weights(P, D, e));
    for (size_t w = (size_t)blockIdx.x * 256 + tid; w < ww + live; w += (size_t)gridDim.x * 256) {
        if (w < ww) wts[w] = in[w];
        else rec[w - ww] = in[w];
    }
    if (blockIdx.x == 0 && tid == 0) {
        if (P.hist) D.hist_cnt[e] = head->hist_cnt;
        D.lazy_reset[e] = 0;
    }
}

__global__ void __launch_bounds__(256) snapshot_replicate_kernel(Problem P, DeviceState D, int src, int first)
{
    const int e = first + blockIdx.y, tid = threadIdx.x;
    if (e == src) return;
    const SlotRecs r = slot_recs(P, D, src);
    // (a record buffer starts at a multiple of N * Cs * 4 bytes and every stride is a multiple of four words: 16-byte pieces throughout)
    const uint4* s4 = reinterpret_cast<const uint4*>(r.rec);
    uint4* d4       = reinterpret_cast<uint4*>(live_records(P, D, e));
    const size_t n16 = (size_t)P.N * (size_t)r.stride / 4, step = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + tid;
    for (; i + 3 * step < n16; i += 4 * step) {   // four loads in flight per lane, then four stores
        const uint4 v0 = s4[i], v1 = s4[i + step], v2 = s4[i + 2 * step], v3 = s4[i + 3 * step];
        d4[i] = v0; d4[i + step] = v1; d4[i + 2 * step] = v2; d4[i + 3 * step] = v3;
    }
    for (; i < n16; i += step) d4[i] = s4[i];
    if (P.belief == FBA_BELIEF_IMPORTANCE) {
        const double* sw = D.p_weight + r.wb;
        double* dw       = live_weights(P, D, e);
        for (size_t k = (size_t)blockIdx.x * 256 + tid; k < (size_t)P.N; k += step) dw[k] = sw[k];
    }
    if (blockIdx.x == 0 && tid == 0) {
        if (P.hist) D.hist_cnt[e] = r.cnt;
        D.lazy_reset[e] = 0;
    }
}

static size_t payload_words(const Problem& P, const BeliefSnapshotArgs& a) { return (a.weighted ? (size_t)2 * P.N : 0) + (size_t)P.N * (size_t)P.Cs; }

void launch_snapshot_pack(const Problem& P, const DeviceState& D, const BeliefSnapshotArgs& a, hipStream_t st)
{
    const dim3 grid(blocks_per_slot(payload_words(P, a), 256 * 8, a.count), a.count);
    hipLaunchKernelGGL(snapshot_pack_kernel, grid, dim3(256), 0, st, P, D, a);
}
void launch_snapshot_validate(const Problem& P, const DeviceState& D, const BeliefSnapshotArgs& a, hipStream_t st)
{
    const dim3 grid(blocks_per_slot(payload_words(P, a), 256 * 8, a.count), a.count);
    if (P.hist == 3) hipLaunchKernelGGL(snapshot_validate_kernel<7>, grid, dim3(256), 0, st, P, D, a);
    else if (P.hist == 2) hipLaunchKernelGGL(snapshot_validate_kernel<6>, grid, dim3(256), 0, st, P, D, a);
    else if (P.hist) hipLaunchKernelGGL(snapshot_validate_kernel<5>, grid, dim3(256), 0, st, P, D, a);
    else if (P.packed || P.ft_packed) hipLaunchKernelGGL(snapshot_validate_kernel<1>, grid, dim3(256), 0, st, P, D, a);
    else hipLaunchKernelGGL(snapshot_validate_kernel<0>, grid, dim3(256), 0, st, P, D, a);
}
void launch_snapshot_commit(const Problem& P, const DeviceState& D, const BeliefSnapshotArgs& a, hipStream_t st)
{
    const dim3 grid(blocks_per_slot(payload_words(P, a), 256 * 8, a.count), a.count);
    hipLaunchKernelGGL(snapshot_commit_kernel, grid, dim3(256), 0, st, P, D, a);
}
void launch_snapshot_replicate(const Problem& P, const DeviceState& D, int src, int first, int count, hipStream_t st)
{
    for (int done = 0; done < count; done += SNAPSHOT_MAX_SLOTS) {   // (a grid has 65 535 rows at most)
        const int n = std::min(SNAPSHOT_MAX_SLOTS, count - done);
        const dim3 grid(blocks_per_slot((size_t)P.N * (size_t)P.Cs / 4, 256 * 4, n), n);
        hipLaunchKernelGGL(snapshot_replicate_kernel, grid, dim3(256), 0, st, P, D, src, first + done);
    }
}

}  // namespace fba
