// fba_forecast.hip -- fba_belief_forecast: the one-step predictive of a range of slots after the action the caller names, evaluated on
// the device from whatever record format the context stores, without building a particle's table.  Per particle its OWN domain state s_i
// and its OWN model: p_i(s') = the product over the transition nodes of the expected Dirichlet row of (s_i, a) at the features of s',
// l_i(s') = the product over the observation nodes of the row the features of s' choose, at the features of the observation.
//
//   forecast_chunk_kernel   a workgroup takes a chunk of a slot's particles:
//                             factors     each particle's transition rows (TL entries) and, per observation node and row, theta[row][o_g],
//                                         as fp64 tables in LDS: belief_factors (fba_belief_factors.h), which fba_probe.hip calls as well
//                                         -- the only phase that knows the record format
//                             accumulate  thread k owns s' = k, k + 256, ...: sum_i w_i p_i(s') and sum_i w_i p_i(s') l_i(s') in registers
//                             combine     one global fp64 atomic per non-zero entry into the slot's zeroed accumulators
//   forecast_finish_kernel  weight total, / W, evidence = the sum of post_mass                       one workgroup per slot
//
// A translation unit of its own, outside the parity path: the order of the fp64 additions is the engine's.  Read-only on the context.
#include "fba_belief_factors.h"

namespace fba {

// FMT: the record format (with_record_format).  Dynamic LDS: forecast_lds_bytes (fba_kernels.h).
template <int FMT>
__global__ void __launch_bounds__(256) forecast_chunk_kernel(Problem P, DeviceState D, BeliefForecastArgs a)
{
    const int tid = threadIdx.x, b = blockIdx.y;
    const int nT = a.lay.nT, nO = a.lay.nO, nn = nT + nO, TL = a.lay.TL, RL = a.lay.RL, S = P.S;
    const bool want_l = a.obs != nullptr;
    // (more entries than a record has room for: the host refuses such a slot before the launch; the phase checks, for s_w and its walk)
    const auto [s_P, s_L, s_w, s_mask, s_nd, s_seg, s_out, nloc] =
        belief_factors<FMT>(P, D, a.lay, a.first + b, a.action[b], want_l ? a.obs[b] : 0, want_l, true);

    // ---- accumulate, combine ----
    double* acc = a.acc + (size_t)b * 2 * S;
    for (int sp = tid; sp < S; sp += 256) {
        const uint64_t fv = P.fd ? pack_features(sp, P.fd->Sstep, nT) : (uint64_t)sp;
        int tix[MAXF], oix[MAXF];
#pragma unroll
        for (int f = 0; f < MAXF; ++f) {
            tix[f] = f < nT ? s_seg[f] + (P.fd ? feat(fv, f) : sp) : 0;
            oix[f] = f < nO && want_l ? s_seg[nT + f] + (P.fd ? node_row(nullptr, s_nd[nT + f], s_nd[nT + f].fixed_mask, fv) : sp) : 0;
        }
        double sn = 0.0, sq = 0.0;
        for (int i = 0; i < nloc; ++i) {
            const double w = s_w[i];
            if (w == 0.0) continue;
            double p = 1.0;
#pragma unroll
            for (int f = 0; f < MAXF; ++f)
                if (f < nT) p *= s_P[(size_t)i * TL + tix[f]];
            p *= w;
            sn += p;
            if (want_l) {
#pragma unroll
                for (int g = 0; g < MAXF; ++g)
                    if (g < nO) {
                        int ix = oix[g];
                        if (s_nd[nT + g].var >= 0) ix = s_seg[nT + g] + node_row(nullptr, s_nd[nT + g], s_mask[i * nn + nT + g], fv);
                        p *= s_L[(size_t)i * RL + ix];
                    }
                sq += p;
            }
        }
        if (sn != 0.0) unsafeAtomicAdd(&acc[sp], sn);
        if (sq != 0.0) unsafeAtomicAdd(&acc[S + sp], sq);
    }
}

__global__ void __launch_bounds__(256) forecast_finish_kernel(Problem P, DeviceState D, BeliefForecastArgs a)
{
    __shared__ double s_part[256];
    const int b = blockIdx.x, e = a.first + b, tid = threadIdx.x, S = P.S;
    const double W = slot_weight_total(P, D, slot_recs(P, D, e), s_part);
    __syncthreads();
    const double* acc = a.acc + (size_t)b * 2 * S;
    double ev = 0.0;
    for (int sp = tid; sp < S; sp += 256) {
        // (a filter whose weights are all 0 has no predictive: every output is 0.0, as every term is)
        if (a.next_mass) a.next_mass[(size_t)b * S + sp] = W > 0.0 ? acc[sp] / W : 0.0;
        const double pm = W > 0.0 ? acc[S + sp] / W : 0.0;
        if (a.post_mass) a.post_mass[(size_t)b * S + sp] = pm;
        ev += pm;
    }
    s_part[tid] = ev;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) s_part[tid] += s_part[tid + st];
        __syncthreads();
    }
    if (tid == 0 && a.evidence) a.evidence[b] = s_part[0];
}

void launch_belief_forecast(const Problem& P, const DeviceState& D, const BeliefForecastArgs& a, hipStream_t st)
{
    const size_t lds = forecast_lds_bytes(a.lay.TL, a.lay.RL, a.lay.nT + a.lay.nO, a.lay.chunk, P.hist != 0);
    const dim3 grid(ceil_div(P.N, a.lay.chunk), a.count), block(256);
    with_record_format(P, a.lay.ft_FS, [&](auto fmt) { hipLaunchKernelGGL(forecast_chunk_kernel<decltype(fmt)::value>, grid, block, lds, st, P, D, a); });
    hipLaunchKernelGGL(forecast_finish_kernel, dim3(a.count), block, 0, st, P, D, a);
}

}  // namespace fba
