// run_candidate.h -- which runs of a batch an iterate call left worth asking about: the half of a run's eligibility that does
// not need the collision verdict.  multistart_kernels.hip (select_key, respawn_rank_kernel) adds the verdict or the margin to it;
// verdict_kernels.hip decides with it which runs the verdict is taken of at all (DevVerdictPlan::cand_status), so the two
// cannot disagree about a run.  or_cdchomp_amd/module.py `candidates` is its specification.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// status: the run's status of the last iterate call (-1 left its limits, 0 ran, 1 stopped converged); total_cost: costs[run][0]
__host__ __device__ __forceinline__ bool orc_run_candidate(int status, double total_cost)
{
   return (status == 0 || status == 1) && isfinite(total_cost);
}
