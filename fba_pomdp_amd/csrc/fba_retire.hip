// fba_retire.hip -- fba_giveup_policy(FBA_GIVEUP_RETIRE): the run of a slot whose rejection update gave up is taken out of the experiment,
// reported, and the slot moved on to its next run (include/fba_hip.h).  Launched by tick() between the belief update and flush_kernel, only
// under that policy.
//
//   retire_kernel   one thread per slot.  A slot is served iff its flag DeviceState::gave_up is set: reject_give_up (fba_kernels.hip) set it
//                   in this launch's belief update, cleared the slot's request for an update and left everything else as it was -- the
//                   filter the slot held, its position (run, episode, t still address the step that was taken), and what env_kernel
//                   decided for the step in DeviceState::adv:
//                     adv == 2   the step was the last of the horizon: env_kernel has recorded the episode's return and length and added it
//                                to the slot's sums.  They stay: the episode is counted.
//                     adv == 1   the episode would have gone on: nothing of it has been recorded, and nothing will be (void).
//                   The kernel appends one fba_retired_rec, marks the step's record (update_count = FBA_UPDATE_GAVE_UP: flush_kernel hands
//                   it over as it does every other, step_stats_kernel counts the step but no update) and sets adv = 3, on which
//                   advance_kernel takes the way out of a run's last episode: the slot's next run with need_init and need_reset, or
//                   inactive and one off n_active.  Budgeted searches: a slot that gives up has taken its step in this launch, so its
//                   search is finished and nothing is parked.  Compact tiger filters: the slot keeps its flag with its filter, as at the
//                   end of any run; post_init_kernel clears it with the next run's Belief::initiate.
//
// A translation unit of its own, outside the parity path: a run that is not retired never meets it.
#include "fba_kernels_common.h"

namespace fba {

__global__ void __launch_bounds__(256) retire_kernel(Problem P, DeviceState D, RetireArgs a)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P.E || !D.gave_up[e]) return;
    D.gave_up[e] = 0;
    if (!D.active[e]) return;   // (a flag without a run: nothing to retire)
    const int adv = D.adv[e];
    const unsigned long long idx = atomicAdd(a.seen, 1ull);
    if (idx < (unsigned long long)a.capacity) {
        fba_retired_rec r;
        r.run = D.run[e]; r.episode = D.episode[e]; r.t = D.t[e]; r.slot = e;
        r.reason = FBA_RETIRED_REJECTION;
        r.counted = adv == 2 ? 1 : 0;
        r.max_attempts = P.reject_max; r.reserved = 0;
        a.recs[idx] = r;
    }
    D.cur[e].update_count = FBA_UPDATE_GAVE_UP;
    D.adv[e] = 3;
}

void launch_retire(const Problem& P, const DeviceState& D, const RetireArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(retire_kernel, dim3(ceil_div(P.E, 256)), dim3(256), 0, st, P, D, a);
}

}  // namespace fba
