// fba_convert.hip -- fba_belief_convert: snapshot blocks of one context refitted to another that differs from it in the particle count
// and, for history records, in the room of a record.  Staging buffer to staging buffer; nothing of a context is read or written, and
// nothing here is on the path of a tick.  The staged source blocks are judged by snapshot_validate_kernel (fba_snapshot.hip), launched
// with a Problem shaped like the source.
//
//   snapshot_convert_scan_kernel   weighted blocks whose particle count changes: the device-order inclusive prefix sums of the source
//                                  weights (block_device_scan), one workgroup per block, into scratch of the call's; a total that is
//                                  zero or not finite leaves through the call's error word (atomicMin), never through DeviceState::fault
//   snapshot_convert_kernel        several workgroups per destination block, a tile of 256 output particles at a time: a thread finds the
//                                  source of its particle -- itself, uniform_int(N') or the guided pick on the prefix sums, first draw of
//                                  stream (first_run + block, 0, 0, CONVERT, particle) -- and writes its weight; then the tile's records
//                                  move as 16-byte pieces, consecutive lanes on consecutive pieces of the destination: the live words of
//                                  the source record (read at the source stride), zeros behind them.  Every word written enters the
//                                  block's checksum in the same pass
//
// Both sides are staged as a span's store is (snapshot_store_pad / _pitch, fba_kernels.h): the record part of every block starts at a
// multiple of 16 bytes, every stride is a multiple of 16 bytes, so whole pieces move; W4 = false is the word-wise form for a stride pair
// that is not (no context of this engine makes one).
#include "fba_kernels_common.h"

namespace fba {

__global__ void __launch_bounds__(256) snapshot_convert_scan_kernel(BeliefConvertArgs a)
{
    __shared__ double s_carry[IS_MAX_CHUNKS + 2];   // (n_src <= 256 * IS_MAX_CHUNKS: the host)
    const int b = blockIdx.x;
    const double* w = reinterpret_cast<const double*>(a.src + (size_t)b * (size_t)a.src_pitch + sizeof(fba_snapshot_head));
    double* incl = a.incl + (size_t)b * (size_t)a.n_src;
    (void)block_device_scan(w, a.n_src, incl, s_carry);
    if (threadIdx.x == 0) {
        const double total = incl[a.n_src - 1];   // (written by this workgroup, before the barrier block_device_scan ends with)
        if (!(total > 0.0 && total < (double)INFINITY)) atomicMin(a.bad, ((unsigned long long)b << 40) | (unsigned long long)SNAP_BAD_TOTAL);
    }
}

template <bool W4>
__global__ void __launch_bounds__(256) snapshot_convert_kernel(Problem P, BeliefConvertArgs a)
{
    __shared__ int s_src[256];
    const int b = blockIdx.y, tid = threadIdx.x, N = P.N, n_src = a.n_src;
    const uint8_t* sblk = a.src + (size_t)b * (size_t)a.src_pitch;
    const fba_snapshot_head* head = reinterpret_cast<const fba_snapshot_head*>(sblk);
    // (the host pass: the total fits a record on both sides, the source stride is that of the total in the source's room)
    const int total = P.hist ? hist_total(head->hist_cnt) : 0;
    const int live = P.hist ? 2 + total : P.C + 1;   // words of a record that say something
    const int sstride = (int)(head->stride / 4u), dstride = P.hist ? hist_stride(P, total) : P.Cs;
    const size_t sww = a.weighted ? (size_t)2 * n_src : 0, dww = a.weighted ? (size_t)2 * N : 0;
    const uint32_t* swts = reinterpret_cast<const uint32_t*>(sblk + sizeof(fba_snapshot_head));
    const uint32_t* srec = swts + sww;
    uint32_t* dwts = reinterpret_cast<uint32_t*>(a.dst + (size_t)b * (size_t)a.dst_pitch + sizeof(fba_snapshot_head));
    uint32_t* drec = dwts + dww;
    const double* incl = a.mode == CONVERT_WEIGHTED ? a.incl + (size_t)b * (size_t)n_src : nullptr;
    const double wtot = incl ? incl[n_src - 1] : 0.0;
    if (incl && !(wtot > 0.0 && wtot < (double)INFINITY)) return;   // (the scan has reported the block; uniform over the workgroup)
    Rng g;
    g.seed(a.seed_lo, a.seed_hi);
    g.position(a.first_run + (uint32_t)b, 0, 0);
    g.draw = 0; g.c1 = 0; g.keep_lo = 0; g.keep_hi = 0;
    const double wnew = 1.0 / (double)N;   // what importance_sampling::resample leaves (ImportanceSampler.hpp:73)
    unsigned long long sum = 0;
    for (int j0 = (int)blockIdx.x * 256; j0 < N; j0 += (int)gridDim.x * 256) {
        const int j = j0 + tid;
        __syncthreads();   // (the pieces of the tile before have read s_src)
        if (j < N) {
            int src = j;
            if (a.mode != CONVERT_SAME) {
                g.stream(FBA_PHASE_CONVERT, (uint32_t)j);
                src = a.mode == CONVERT_FLAT ? g.uniform_int(n_src) : weighted_pick_guided(incl, n_src, g.u01() * wtot, wtot);
            }
            s_src[tid] = src;
            if (a.weighted) {
                uint2 wv;
                if (a.mode == CONVERT_SAME) wv = make_uint2(swts[2 * (size_t)src], swts[2 * (size_t)src + 1]);
                else wv = make_uint2((uint32_t)__double2loint(wnew), (uint32_t)__double2hiint(wnew));
                *reinterpret_cast<uint2*>(dwts + 2 * (size_t)j) = wv;   // (the weights start at a multiple of 8 bytes)
                sum += check_term(wv.x, 2 * (size_t)j) + check_term(wv.y, 2 * (size_t)j + 1);
            }
        }
        __syncthreads();
        const int np = min(256, N - j0);
        if (W4) {
            const int d4 = dstride >> 2, pieces = np * d4;
            for (int q = tid; q < pieces; q += 256) {
                const int p = q / d4, k = (q - p * d4) * 4;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (k < live) {   // (live <= sstride, a multiple of four words: the piece lies inside the source record)
                    v = *reinterpret_cast<const uint4*>(srec + (size_t)s_src[p] * (size_t)sstride + k);
                    if (k + 1 >= live) v.y = 0u;
                    if (k + 2 >= live) v.z = 0u;
                    if (k + 3 >= live) v.w = 0u;
                }
                const size_t w = (size_t)(j0 + p) * (size_t)dstride + (size_t)k;
                *reinterpret_cast<uint4*>(drec + w) = v;
                sum += (check_term(v.x, dww + w) + check_term(v.y, dww + w + 1)) + (check_term(v.z, dww + w + 2) + check_term(v.w, dww + w + 3));
            }
        } else {
            const int words = np * dstride;
            for (int q = tid; q < words; q += 256) {
                const int p = q / dstride, k = q - p * dstride;
                const uint32_t v = k < live ? srec[(size_t)s_src[p] * (size_t)sstride + k] : 0u;
                const size_t w = (size_t)(j0 + p) * (size_t)dstride + (size_t)k;
                drec[w] = v;
                sum += check_term(v, dww + w);
            }
        }
    }
    // behind the last record: zeros up to N * Cs words (they add nothing to the checksum)
    const size_t used = (size_t)N * (size_t)dstride, all = (size_t)N * (size_t)P.Cs;
    if (W4) {
        uint4* z = reinterpret_cast<uint4*>(drec);
        for (size_t i = used / 4 + (size_t)blockIdx.x * 256 + tid; i < all / 4; i += (size_t)gridDim.x * 256) z[i] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        for (size_t i = used + (size_t)blockIdx.x * 256 + tid; i < all; i += (size_t)gridDim.x * 256) drec[i] = 0u;
    }
    block_check_add(sum, a.check + b);
}

void launch_convert_scan(const BeliefConvertArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(snapshot_convert_scan_kernel, dim3(a.count), dim3(256), 0, st, a);
}
void launch_snapshot_convert(const Problem& P, const BeliefConvertArgs& a, hipStream_t st)
{
    const dim3 grid(blocks_per_slot((size_t)P.N, 256, a.count), a.count);
    if ((P.Cs & 3) == 0 && (a.src_cs & 3) == 0) hipLaunchKernelGGL(snapshot_convert_kernel<true>, grid, dim3(256), 0, st, P, a);
    else hipLaunchKernelGGL(snapshot_convert_kernel<false>, grid, dim3(256), 0, st, P, a);
}

}  // namespace fba
