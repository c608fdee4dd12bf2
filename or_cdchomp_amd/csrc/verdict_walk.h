// verdict_walk.h -- the walk over a run's samples that both collision verdicts make (verdict_kernels.hip): rows interpolated
// on their segments -> FK (fk.h, triads of lanes) -> every active sphere against every field of the run's scene -> the pairs
// of spheres that may collide; the first contact in (sample, XML sphere, field) order, then (sample, pair) order, is kept as
// a key, which is where the reference's loop stops (src/orcdchomp_mod.cpp:2958-3006).
//
// Its steps also serve the clearance of a run (clearance_kernels.hip, through verdict_planned.h) and the kernels over single rows
// (config_kernels.hip, penetration_kernels.hip, through config_query.h).  Of the iterate kernel's headers it takes the FK and
// the field lookup, none of the others.
//
// Included inside the including file's namespace after dev_types.h, verdict_device.h, sdf_lookup.h and fk.h, with the
// contraction the walk is compiled with in force.  One kernel walks samples the host planned, the other plans them itself
// with a fifth wavefront; `depth`, `time` and the key of the two agree bit for bit because this text is compiled into both.
// The steps of a chunk hold no barrier and no early return: ORC_BLOCK threads (tid < ORC_BLOCK) run each of them, and the
// kernels put their barriers, and whatever else they do, between them.
#pragma once

// the walk's part of a workgroup's dynamic LDS, behind the kernel's own header
template <typename real>
struct VerdictLds
{
   real * rows_s;   // [chunk][n] the samples' rows
   real * pos_s;    // [chunk][pstr] sphere centres
   real * ax_s;     // [chunk][astr] joint frames
   real * base_s;   // [12] DevModel::base_R, base_t
   real * srad_s;   // [Sa]
   int * slot_s;    // [Sa_real]
   int * xml_s;     // [Sa]
   int * jctl_s;    // [nj][2]
   int pstr, astr;
};

template <typename real>
__device__ __forceinline__ VerdictLds<real> verdict_lds(unsigned char * base, const DevModel<real> & gmod, int n, int chunk)
{
   VerdictLds<real> L;
   const int Sa = gmod.Sa;
   L.pstr = (Sa*3) | 1; L.astr = (gmod.nj*6) | 1;
   L.rows_s = (real *) base;
   L.pos_s = L.rows_s + ((chunk*n + 3) & ~3);
   L.ax_s = L.pos_s + ((chunk*L.pstr + 3) & ~3);
   L.base_s = L.ax_s + ((chunk*L.astr + 3) & ~3);
   L.srad_s = L.base_s + 12;
   L.slot_s = (int *)(L.srad_s + ((Sa + 3) & ~3));
   L.xml_s = L.slot_s + ((gmod.Sa_real + 3) & ~3);
   L.jctl_s = L.xml_s + ((Sa + 3) & ~3);
   return L;
}

// bytes of that carve-up (and 64 to spare)
inline size_t verdict_walk_lds_bytes(int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk)
{
   const int pstr = (Sa*3) | 1, astr = (nj*6) | 1;
   auto r4 = [](int x) { return (x + 3) & ~3; };
   const size_t reals = (size_t) r4(chunk*n) + r4(chunk*pstr) + r4(chunk*astr) + 12 + r4(Sa);
   const size_t ints = (size_t) r4(Sa_real) + r4(Sa);
   return reals * real_size + ints * 4 + (size_t) nj * 8 + 64;
}

// the model into LDS, by all THREADS threads of the workgroup (a barrier of the kernel's follows)
template <typename real, int THREADS>
__device__ __forceinline__ void verdict_stage(const DevModel<real> & gmod, const int * slot_xml, const VerdictLds<real> & L, int tid)
{
   const int Sa = gmod.Sa, nj = gmod.nj;
   for (int e=tid; e<12; e+=THREADS) L.base_s[e] = (e < 9) ? gmod.base_R[e] : gmod.base_t[e-9];
   for (int e=tid; e<Sa; e+=THREADS) { L.srad_s[e] = gmod.sph_radius[e]; L.xml_s[e] = slot_xml[e]; }
   for (int e=tid; e<gmod.Sa_real; e+=THREADS) L.slot_s[e] = gmod.slot_of[e];
   for (int e=tid; e<nj; e+=THREADS) { L.jctl_s[2*e] = gmod.joints[e].packed; L.jctl_s[2*e+1] = 0; }
}

// what fk.h reads of the robot
template <typename real>
__device__ __forceinline__ ModelView<real> verdict_model_view(const DevModel<real> & gmod, int n, const VerdictLds<real> & L)
{
   ModelView<real> mod;
   mod.nj = gmod.nj; mod.n = n; mod.floating = gmod.floating; mod.tree = gmod.tree; mod.Sa = gmod.Sa; mod.S = gmod.S; mod.GS = gmod.GS;
   mod.base_sph_begin = gmod.base_sph_begin; mod.base_sph_end = gmod.base_sph_end; mod.jt_scan = 0;
   mod.Sa_real = gmod.Sa_real; mod.placed = gmod.placed; mod.live_mask = gmod.live_mask; mod.slot_of = L.slot_s;
   mod.base_R = L.base_s; mod.base_t = L.base_s + 9;
   mod.jctl = L.jctl_s; mod.sph_affects = nullptr; mod.n_static = 0; mod.empty_mask = 0u;
   mod.jpk = (const __attribute__((address_space(4))) int *) gmod.jpacked;
   mod.jpk2 = (const __attribute__((address_space(4))) int *) gmod.jpacked2;
   mod.sph_pos_c = (const __attribute__((address_space(4))) real (*)[3]) gmod.sph_pos;
   mod.joints_c = (const __attribute__((address_space(4))) DevJoint<real> *) gmod.joints;
   mod.slot_c = (const __attribute__((address_space(4))) int *) gmod.slot_of;
   mod.fkj = (const __attribute__((address_space(4))) DevFkJoint<real> *) gmod.fkj;
   return mod;
}

// the run's scene: its slice of the descriptors and its field count
template <typename real>
__device__ __forceinline__ void verdict_scene(const DevVerdictWalk<real> & v, int run, const DevSdf<real> * & sdfs, int & n_fields)
{
   const int scene = v.scene_of_run ? v.scene_of_run[run] : 0;
   n_fields = v.scene_nsdf ? v.scene_nsdf[scene] : v.n_sdfs;
   sdfs = v.sdfs + (size_t) scene * v.n_sdfs;
}

// rows of the `count` samples first .. of seg / u: a0 + (a1 - a0) u on their segments (u: the host's reals in global memory,
// or the planner's doubles in LDS, narrowed here as the host narrows them on upload)
template <typename real, typename U>
__device__ __forceinline__ void verdict_rows(const real * traj, const int * seg, const U * u, int first, int count, int n, int tid, const VerdictLds<real> & L)
{
   for (int e=tid; e<count*n; e+=ORC_BLOCK)
   {
      const int s = e / n, c = e - s*n;
      const int sg = seg[first + s];
      const real uu = (real) u[first + s];
      const real a0 = traj[sg*n + c], a1 = traj[(sg+1)*n + c];
      L.rows_s[s*n + c] = a0 + (a1 - a0) * uu;
   }
}

// a floating base's quaternion, renormalised
template <typename real>
__device__ __forceinline__ void verdict_renormalise(const ModelView<real> & mod, int count, int tid, const VerdictLds<real> & L)
{
   if (mod.floating && tid < count)
   {
      real * row = L.rows_s + tid*mod.n;
      const real len = M<real>::sqrt_(row[3]*row[3] + row[4]*row[4] + row[5]*row[5] + row[6]*row[6]);
      const real inv = (real)1 / len;
      row[3] *= inv; row[4] *= inv; row[5] *= inv; row[6] *= inv;
   }
}

// 20 samples per wavefront (fk.h: triads of lanes)
template <typename real, bool TREE>
__device__ __forceinline__ void verdict_fk(const ModelView<real> & mod, int count, int tid, const VerdictLds<real> & L)
{
   const int lane16 = tid & 15, triad = (lane16 * 11) >> 5;
   const int s = (tid >> 6) * 20 + ((tid >> 4) & 3) * 5 + triad;
   const bool valid = (lane16 < 15) && (s < count);
   const int sr = valid ? s : 0;
   fk_waypoint_triad<real, TREE>(mod, L.rows_s + sr*mod.n, 0, 0, mod.nj, true, (lane16 < 15) ? lane16 - 3*triad : 0, valid, L.pos_s + sr*L.pstr, L.ax_s + sr*L.astr);
}

// a contact: kept when it is the thread's first (its depth stays with the thread) and offered as the run's first
__device__ __forceinline__ void verdict_contact(int sample, unsigned long long pair_bit, int sphere, int other, double depth,
   unsigned long long & my_key, double & my_depth, unsigned long long * key_s)
{
   const unsigned long long key = ((unsigned long long) sample << 32) | (pair_bit << 31) | ((unsigned long long) sphere << 16) | (unsigned long long) other;
   if (key < my_key) { my_key = key; my_depth = depth; }
   atomicMin(&key_s[0], key);
}

// the chunk's `count` samples, the run's samples sbase .. : every live sphere against every field, then the pairs
template <typename real>
__device__ __forceinline__ void verdict_tests(const DevVerdictWalk<real> & v, const ModelView<real> & mod, const DevSdf<real> * sdfs, int n_fields,
   int sbase, int count, int tid, const VerdictLds<real> & L, unsigned long long & my_key, double & my_depth, unsigned long long * key_s)
{
   const int Sa = mod.Sa;
   for (int item=tid; item<count*Sa; item+=ORC_BLOCK)
   {
      const int s = item / Sa, slot = item - s*Sa;
      if (!((mod.live_mask >> slot) & 1ull)) continue;
      const real * p = L.pos_s + s*L.pstr + slot*3;
      const real radius = L.srad_s[slot];
      for (int i=0; i<n_fields; i++)
      {
         const DevSdf<real> & F = sdfs[i];
         real gp[3], gg[3], val;
#pragma unroll
         for (int k=0; k<3; k++)
            gp[k] = F.Rgw[k*3+0]*p[0] + F.Rgw[k*3+1]*p[1] + F.Rgw[k*3+2]*p[2] + F.tgw[k];
         if (sdf_lookup(F, gp, val, gg)) continue;                 // outside this field
         if (val - radius < (real)0) verdict_contact(sbase + s, 0ull, L.xml_s[slot], i, (double)(radius - val), my_key, my_depth, key_s);
      }
   }
   // self collision: a pair of spheres on links that may collide overlaps
   for (int item=tid; item<count*v.n_pairs; item+=ORC_BLOCK)
   {
      const int s = item / v.n_pairs, pi = item - s*v.n_pairs;
      const int ea = v.pairs[pi*4+0], eb = v.pairs[pi*4+1];
      const real * pa = (ea >= 0) ? L.pos_s + s*L.pstr + ea*3 : v.inact_pos + (-1 - ea)*3;
      const real * pb = (eb >= 0) ? L.pos_s + s*L.pstr + eb*3 : v.inact_pos + (-1 - eb)*3;
      const real dx = pa[0]-pb[0], dy = pa[1]-pb[1], dz = pa[2]-pb[2];
      const real dist = M<real>::sqrt_(dx*dx + dy*dy + dz*dz);
      const real rs = v.pair_rsum[pi];
      if (dist - rs < (real)0) verdict_contact(sbase + s, 1ull, v.pairs[pi*4+2], v.pairs[pi*4+3], (double)(rs - dist), my_key, my_depth, key_s);
   }
}
