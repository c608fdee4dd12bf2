// deal.h -- the queries of a single-row call dealt to the shard that owns their run, and the shard's answers put back in the
// caller's order (Batch::deal_by_run, batch.cpp).  Plain C++ without HIP: the arrays are the caller's host arrays.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace orc {

// a column of a call: per query `width` elements of `elem` bytes; data NULL: the caller does not pass it, and it stays NULL
struct DealColumn
{
   void * data;
   size_t width, elem;
   size_t bytes() const { return width * elem; }
};
template <typename T> DealColumn deal_in(const T * data, size_t width) { return DealColumn{ const_cast<T *>(data), width, sizeof(T) }; }      // (read only)
template <typename T> DealColumn deal_out(T * data, size_t width) { return DealColumn{ data, width, sizeof(T) }; }

// a shard's share: the queries whose run lies in [r0, r1), in their order, with the run rebased to the shard, the input
// columns gathered and room for the output columns
struct Deal
{
   std::vector<int> at, run;
   std::vector<std::vector<unsigned char>> in, out;      // (a NULL column: empty)
   std::vector<void *> in_ptr, out_ptr;                  // their data, NULL for a NULL column
};

// run_of_q NULL: every query names run 0
inline Deal deal_gather(int n_q, const int * run_of_q, int r0, int r1, const std::vector<DealColumn> & ins, const std::vector<DealColumn> & outs)
{
   Deal d;
   for (int q=0; q<n_q; q++)
   {
      const int r = run_of_q ? run_of_q[q] : 0;
      if (r < r0 || r >= r1) continue;
      d.at.push_back(q); d.run.push_back(r - r0);
   }
   const size_t cnt = d.at.size();
   d.in.resize(ins.size()); d.out.resize(outs.size());
   for (size_t j=0; j<ins.size(); j++)
   {
      if (ins[j].data) d.in[j].resize(cnt * ins[j].bytes());
      for (size_t i=0; i<cnt && ins[j].data; i++)
         std::memcpy(d.in[j].data() + i*ins[j].bytes(), (const unsigned char *) ins[j].data + (size_t) d.at[i]*ins[j].bytes(), ins[j].bytes());
      d.in_ptr.push_back(ins[j].data ? d.in[j].data() : nullptr);
   }
   for (size_t j=0; j<outs.size(); j++)
   {
      if (outs[j].data) d.out[j].resize(cnt * outs[j].bytes());
      d.out_ptr.push_back(outs[j].data ? d.out[j].data() : nullptr);
   }
   return d;
}

// (a query belongs to one shard: the shards' threads write disjoint entries)
inline void deal_scatter(const Deal & d, const std::vector<DealColumn> & outs)
{
   for (size_t j=0; j<outs.size(); j++)
      for (size_t i=0; i<d.at.size() && outs[j].data; i++)
         std::memcpy((unsigned char *) outs[j].data + (size_t) d.at[i]*outs[j].bytes(), d.out[j].data() + i*outs[j].bytes(), outs[j].bytes());
}

} // namespace orc
