// config_query.h -- what the kernels that answer questions about single rows share (config_kernels.hip, penetration_kernels.hip):
// a query's two minima with their keys, the staging of a workgroup's queries from the LDS carve-up to the fence behind FK, and
// the launcher.  A query is one row, tested against the scene of the run it names, with the batch's model (config_device.h).
//
// Included inside the including file's namespace after verdict_walk.h and wave.h (wave_min), with the contraction the walk is compiled with in force.
// The minima of the two kernels agree bit for bit because this text is compiled into both: config_tests is one loop, lanes
// striding over the items, whatever else the including kernel does with the same lookups.
#pragma once

// a workgroup's LDS header before the walk's part: two ints per query (its run, its non-finite flag), then `extra` bytes per
// query of the kernel's own
__host__ __device__ inline size_t config_query_header_bytes(int chunk, size_t extra) { return (size_t) chunk * (8 + extra); }
// dynamic LDS of a kernel whose top is config_query_prologue
inline size_t config_query_lds_bytes(int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk, size_t extra)
{
   return config_query_header_bytes(chunk, extra) + verdict_walk_lds_bytes(n, Sa, Sa_real, nj, real_size, chunk);
}

// a lane's running minimum of one leg
template <typename real>
struct ConfigMin
{
   real val;
   unsigned int key;
};

// clearance_offer without the sample and its time.  The items do not reach a lane in key order here, so the lowest key among
// equal gaps is kept explicitly.  (a NaN is ignored; +inf is never below)
template <typename real>
__device__ __forceinline__ void config_offer(ConfigMin<real> & m, real gap, int a, int b)
{
   const unsigned int key = ((unsigned int) a << 16) | (unsigned int) b;
   if (gap < m.val || (gap == m.val && key < m.key && m.key != ORC_CONFIG_NONE))
   {
      m.val = gap;
      m.key = key;
   }
}

// the wavefront's minimum of a leg and the lowest key at it, written by lane 0
template <typename real>
__device__ __forceinline__ void config_report(const ConfigMin<real> & m, int lane, double * clear_out, unsigned int * key_out)
{
   const real lowest = wave_min<real>(m.val);
   unsigned int key = (m.key != ORC_CONFIG_NONE && m.val == lowest) ? m.key : ORC_CONFIG_NONE;
   for (int d=32; d>=1; d>>=1) { const unsigned int o = __shfl_xor(key, d); key = o < key ? o : key; }
   if (lane == 0)
   {
      *clear_out = (key == ORC_CONFIG_NONE) ? (double) M<real>::inf() : (double) lowest;
      *key_out = key;
   }
}

// verdict_tests / clearance_tests for ONE query (sample s of the chunk) by ONE wavefront: the same two subtractions
template <typename real>
__device__ __forceinline__ void config_tests(const DevVerdictWalk<real> & v, const ModelView<real> & mod, const DevSdf<real> * sdfs, int n_fields,
   int s, int lane, const VerdictLds<real> & L, ConfigMin<real> & fld, ConfigMin<real> & slf)
{
   const int Sa = mod.Sa;
   for (int item=lane; item<Sa*n_fields; item+=64)
   {
      const int slot = item / n_fields, i = item - slot*n_fields;
      if (!((mod.live_mask >> slot) & 1ull)) continue;
      const real * p = L.pos_s + s*L.pstr + slot*3;
      const real radius = L.srad_s[slot];
      const DevSdf<real> & F = sdfs[i];
      real gp[3], gg[3], val;
#pragma unroll
      for (int k=0; k<3; k++)
         gp[k] = F.Rgw[k*3+0]*p[0] + F.Rgw[k*3+1]*p[1] + F.Rgw[k*3+2]*p[2] + F.tgw[k];
      if (sdf_lookup(F, gp, val, gg)) continue;                 // outside this field
      config_offer<real>(fld, val - radius, L.xml_s[slot], i);
   }
   for (int pi=lane; pi<v.n_pairs; pi+=64)
   {
      const int ea = v.pairs[pi*4+0], eb = v.pairs[pi*4+1];
      const real * pa = (ea >= 0) ? L.pos_s + s*L.pstr + ea*3 : v.inact_pos + (-1 - ea)*3;
      const real * pb = (eb >= 0) ? L.pos_s + s*L.pstr + eb*3 : v.inact_pos + (-1 - eb)*3;
      const real dx = pa[0]-pb[0], dy = pa[1]-pb[1], dz = pa[2]-pb[2];
      const real dist = M<real>::sqrt_(dx*dx + dy*dy + dz*dz);
      const real rs = v.pair_rsum[pi];
      config_offer<real>(slf, dist - rs, v.pairs[pi*4+2], v.pairs[pi*4+3]);
   }
}

// what config_query_prologue leaves for the per-query loop: the calling wavefront evaluates the queries q0 + s, s in
// [s_begin, s_end), the ones it ran FK for (20 per wavefront, fk.h's triads)
template <typename real>
struct ConfigQuery
{
   VerdictLds<real> L;
   ModelView<real> mod;
   const int * run_s;   // [chunk] the query's run
   const int * bad_s;   // [chunk] nonzero: the row has a non-finite entry
   int q0, count, s_begin, s_end;
};

// The top of a kernel over DevConfigClearance (or what derives from it), run by all ORC_BLOCK threads: the model staged as the
// walk stages it, the workgroup's rows COPIED into the walk's rows_s (from the uploaded configurations, from the named waypoints
// or, in the profile form, from every waypoint in storage order), then verdict_renormalise and verdict_fk, whose text is the
// walk's.  `extra_bytes` per query of the LDS header are the kernel's own, and per_row(s, row, mod) is run for every query by
// the thread that looked at its row, before the row is renormalised (the clearance kernel passes 0 and a callable that does nothing).
template <typename real, bool TREE, typename PerRow>
__device__ __forceinline__ ConfigQuery<real> config_query_prologue(const DevConfigClearance<real> & v, unsigned char * smem_raw, size_t extra_bytes, PerRow && per_row)
{
   const DevModel<real> & gmod = *v.model;
   const int tid = threadIdx.x;
   const int n = v.n, np = v.n_points, chunk = v.chunk;
   const int q0 = blockIdx.x * chunk;
   const int count = (v.n_q - q0 < chunk) ? v.n_q - q0 : chunk;      // (the launcher's grid: count >= 1)
   int * run_s = (int *) smem_raw;                 // [chunk] the query's run
   int * bad_s = run_s + chunk;                    // [chunk] nonzero: the row has a non-finite entry
   const VerdictLds<real> L = verdict_lds(smem_raw + config_query_header_bytes(chunk, extra_bytes), gmod, n, chunk);
   verdict_stage<real, ORC_BLOCK>(gmod, v.slot_xml, L, tid);
   const ModelView<real> mod = verdict_model_view(gmod, n, L);
   const bool profile = !v.configs && !v.point_of_q;
   if (tid < count)
   {
      const int q = q0 + tid;
      run_s[tid] = profile ? q / np : (v.run_of_q ? v.run_of_q[q] : 0);
   }
   // the rows, copied
   for (int e=tid; e<count*n; e+=ORC_BLOCK)
   {
      const int s = e / n, c = e - s*n, q = q0 + s;
      real x;
      if (v.configs) x = v.configs[(size_t) q*n + c];
      else
      {
         const int run = profile ? q / np : v.run_of_q[q];
         const int point = profile ? q - run*np : v.point_of_q[q];
         x = v.traj[((size_t) run*np + point)*n + c];
      }
      L.rows_s[s*n + c] = x;
   }
   __syncthreads();
   // a row with a non-finite entry is not evaluated: decided here, before FK, which then runs on a harmless row in its place
   if (tid < count)
   {
      real * row = L.rows_s + tid*n;
      bool bad = false;
      for (int c=0; c<n; c++) bad = bad || !(M<real>::fabs_(row[c]) < M<real>::inf());
      bad_s[tid] = bad ? 1 : 0;
      if (bad)
      {
         for (int c=0; c<n; c++) row[c] = (real)0;
         if (mod.floating) row[6] = (real)1;
      }
      per_row(tid, row, mod);
   }
   verdict_renormalise(mod, count, tid, L);      // (tid < count: the thread that looked at the row)
   __syncthreads();
   verdict_fk<real, TREE>(mod, count, tid, L);
   // what the wavefront's lanes stored for its 20 queries is read by its other lanes: a wavefront's LDS operations execute in
   // program order, and the compiler keeps them on their side of this point
   __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
   __builtin_amdgcn_wave_barrier();
   __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
   const int s_begin = (tid >> 6) * 20;
   const int s_end = (s_begin + 20 < count) ? s_begin + 20 : count;
   return ConfigQuery<real>{ L, mod, run_s, bad_s, q0, count, s_begin, s_end };
}

// One launcher for a kernel's two instantiations of a precision (host code: the including file has <atomic>), with a grid of
// chunks where launch_verdict_kernels (verdict_planned.h) has one of runs; the dynamic-LDS attribute is per device and per
// kernel, and set for both on a device's first launch.
template <typename Args, void (*KTREE)(Args), void (*KCHAIN)(Args)>
static hipError_t launch_config_query(const Args & v, size_t lds, hipStream_t stream, int tree)
{
   static std::atomic<unsigned long long> attr_set{0ull};
   if (v.chunk < 4 || v.chunk > 64 || (v.chunk & 3)) return hipErrorInvalidValue;
   if (v.n_q < 1 || v.n_q > ORC_CONFIG_MAX_Q || v.n_points < 1) return hipErrorInvalidValue;
   if (!v.configs && ((v.run_of_q == nullptr) != (v.point_of_q == nullptr))) return hipErrorInvalidValue;
   if (!v.configs && !v.point_of_q && v.n_q > v.n_runs * v.n_points) return hipErrorInvalidValue;
   if (lds > ORC_VERDICT_LDS_LIMIT) return hipErrorInvalidValue;
   int dev = 0;
   if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
   if (!((attr_set.load() >> dev) & 1ull))
   {
      hipError_t e = hipFuncSetAttribute((const void *) KTREE, hipFuncAttributeMaxDynamicSharedMemorySize, ORC_VERDICT_LDS_LIMIT);
      if (e == hipSuccess) e = hipFuncSetAttribute((const void *) KCHAIN, hipFuncAttributeMaxDynamicSharedMemorySize, ORC_VERDICT_LDS_LIMIT);
      if (e != hipSuccess) return e;
      attr_set.fetch_or(1ull << dev);
   }
   const int blocks = (v.n_q + v.chunk - 1) / v.chunk;
   if (tree) hipLaunchKernelGGL(KTREE, dim3(blocks), dim3(ORC_BLOCK), lds, stream, v);
   else hipLaunchKernelGGL(KCHAIN, dim3(blocks), dim3(ORC_BLOCK), lds, stream, v);
   return hipGetLastError();
}
