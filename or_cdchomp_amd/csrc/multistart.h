// multistart.h -- host side of the multi-start calls (multistart.cpp; the kernels are multistart_kernels.hip): orc_batch_perturb,
// _select_best[_by], _select_clear, _respawn and _gettraj_runs.  The members of BatchShard, Batch and Module that make them are
// declared in batch.h and module.h; here is what they pass each other.  Nothing in this file needs HIP or the module.
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>
#include "cost_key.h"

namespace orc {

constexpr size_t ORC_PERTURB_MAX_MN = 20136;     // m n of a run that perturb_kernel stages in LDS: 8 m n + 2496 (the mt19937 state) <= 160 KB - 256
constexpr int ORC_RESPAWN_MAX_GROUP = 4096;      // the largest group respawn_rank_kernel takes (14 bytes of LDS per member: 56 KB)

// Which runs a selection takes, always among the candidates (run_candidate.h).  collision_free: the verdict made just before
// found no contact; by_margin: the clearance made just before walked the run and the smaller of its two minima is at least
// `margin`.  column 0 total, 1 obs, 2 smooth: the cost that is minimised and reported; 3 (by_margin only): minus the clearance
struct SelectCriterion { bool collision_free = false, by_margin = false; double margin = 0.0; int column = 0; };

// Per group: the lowest key (cost_key.h) among the eligible runs, the lowest run that has it (a shard's: its LOCAL run; -1 once
// merged: no eligible run), the winner's clearance (NaN: none, or no margin) and the number of eligible runs
struct SelectResult
{
   std::vector<unsigned long long> key; std::vector<double> clear; std::vector<int> run, count;
   explicit SelectResult(size_t n_groups = 0) : key(n_groups), clear(n_groups), run(n_groups), count(n_groups) {}
   double cost(size_t g) const { return run[g] >= 0 ? cost_of_key(key[g]) : HUGE_VAL; }      // +inf for an empty group
};

// the merge of n_shards x n_groups winners: the lower key, then the lower run (shard k holds the runs from offs[k]), the counts added
inline SelectResult merge_winners(const std::vector<SelectResult> & shard, const std::vector<int> & offs, int n_groups)
{
   SelectResult out(n_groups);
   for (int g=0; g<n_groups; g++)
   {
      unsigned long long bk = ~0ull; int br = -1, cnt = 0; double bc = std::nan("");
      for (size_t k=0; k<shard.size(); k++)
      {
         const SelectResult & s = shard[k];
         cnt += s.count[g];
         if (s.count[g] > 0 && s.key[g] < bk) { bk = s.key[g]; br = offs[k] + s.run[g]; bc = s.clear[g]; }
      }
      out.key[g] = bk; out.run[g] = br; out.count[g] = cnt; out.clear[g] = bc;
   }
   return out;
}

// a shard's groups (the caller's numbers) and their CSR over its local runs: group_offs [groups.size() + 1], members ascending per group
struct GroupCsr { std::vector<int> groups, group_offs, members; };

// group [n_runs] (entries in [0, n_groups)) as one GroupCsr per shard (offs: the first run of every shard, then n_runs); throws
// for a group over ORC_RESPAWN_MAX_GROUP and for one whose runs lie on two shards
inline std::vector<GroupCsr> group_csr_by_shard(const std::vector<int> & group, int n_groups, const std::vector<int> & offs)
{
   const int n_runs = (int) group.size();
   // a counting sort of the runs by group: the members of a group ascending
   std::vector<int> first(n_groups + 1, 0);
   for (int r=0; r<n_runs; r++) first[group[r] + 1]++;
   for (int g=0; g<n_groups; g++)
   {
      if (first[g+1] > ORC_RESPAWN_MAX_GROUP)
         throw std::runtime_error("respawn: group " + std::to_string(g) + " has " + std::to_string(first[g+1]) + " runs, more than the ranking kernel takes (" + std::to_string(ORC_RESPAWN_MAX_GROUP) + ")!");
      first[g+1] += first[g];
   }
   std::vector<int> sorted(n_runs), fill(first.begin(), first.end() - 1);
   for (int r=0; r<n_runs; r++) sorted[fill[group[r]]++] = r;
   // every group to the shard that holds its runs
   std::vector<GroupCsr> shards(offs.size() - 1);
   for (auto & sh : shards) sh.group_offs.assign(1, 0);
   for (int g=0; g<n_groups; g++)
   {
      if (first[g+1] == first[g]) continue;      // (a group without runs: no survivor, nothing to do)
      size_t k = 0;
      while (sorted[first[g]] >= offs[k+1]) k++;
      if (sorted[first[g+1] - 1] >= offs[k+1])
         throw std::runtime_error("respawn: the runs of group " + std::to_string(g) + " lie on more than one shard of the module's devices (a copy does not cross devices)!");
      GroupCsr & sh = shards[k];
      sh.groups.push_back(g);
      for (int q=first[g]; q<first[g+1]; q++) sh.members.push_back(sorted[q] - offs[k]);
      sh.group_offs.push_back((int) sh.members.size());
   }
   return shards;
}

// what a perturbation of a batch needs: the generators of A^-1 (U [D][m], then V [D][m]) and sigma c; sigma == 0: scale 0 and no generators
struct PerturbPlan { std::vector<double> gen; int D = 0; double scale = 0.0; };

// what Batch::respawn_plan leaves of a checked orc_batch_respawn: no device work went into it
struct RespawnPlan
{
   int column = 0, mode = 0, keep = 1, n_groups = 0;
   PerturbPlan perturb;
   std::vector<GroupCsr> shards;
};

} // namespace orc
