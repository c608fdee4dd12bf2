// verdict_device.h -- the two collision verdicts of a batch (verdict_kernels.hip), as verdict.cpp launches them.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_types.h"

// Collision verdict of the trajectories of a batch (the step after the path: gettraj's re-check,
// src/orcdchomp_mod.cpp:2958-3006, with the optimizer's own sphere / field model): what the walk over a run's samples
// reads and writes (verdict_walk.h), whoever planned the samples.
template <typename real>
struct DevVerdictWalk
{
   const DevModel<real> * model;
   const DevSdf<real> * sdfs;  // [n_scenes][n_sdfs]
   int n_sdfs;                 // fields of the largest scene
   const int * scene_of_run;   // [n_runs] (DevBatch::scene_of_run)
   const int * scene_nsdf;     // [n_scenes]
   int n_runs, n_points, n;
   int chunk;                  // samples walked at a time (<= 64, a multiple of 4: as many as the CU's LDS holds of this robot)
   const real * traj;          // [n_runs][n_points][n]
   const int * slot_xml;       // [Sa lanes] XML index of the sphere in a slot, -1: empty
   // self collision (src/orcdchomp_mod.cpp:2998-2999: `|| CheckSelfCollision`): the pairs of spheres on links that may
   // collide, XML order (a < b); an end of a pair is a slot of the position row, or -1 - k: inactive sphere k of inact_pos
   int n_pairs;
   const int * pairs;          // [n_pairs][4]: end a, end b, XML index of a, XML index of b
   const real * pair_rsum;     // [n_pairs] r_a + r_b
   const real * inact_pos;     // [inactive spheres][3] world positions
   // first contact of a run: ORC_VERDICT_NONE, or sample << 32 | pair bit << 31 | XML sphere (a) << 16 | field, or XML
   // sphere b of a pair.  Within a sample the fields come first (sphere, field order), then the pairs
   unsigned long long * key_out;   // [n_runs]
   double * depth_out;         // [n_runs] penetration depth of that contact (the caller zeroes it)
};

// ... of samples the host planned (Module::batch_collision_verdict)
template <typename real>
struct DevVerdict : DevVerdictWalk<real>
{
   const int * offs;           // [n_runs+1] first sample of every run
   const int * seg;            // [samples] segment of the trajectory the sample lies on
   const real * u;             // [samples] position on the segment, 0..1
};

// ... with the retiming and the sample planning on the device (verdict_planned.h): what DevVerdict takes as offs / seg / u, the
// workgroup derives from the trajectory and vmax.  What the two kernels made of that walk share of their arguments:
template <typename real>
struct DevVerdictPlanned : DevVerdictWalk<real>
{
   int col0;                   // first column the retiming reads (7 with a floating base)
   const double * vmax;        // [n - col0] velocity limits of the retimed columns
   // Which runs are examined (orc_batch_collision_verdict_subset, orc_batch_set_verdict_scope, orc_batch_clearance); all NULL:
   // every run.  A run that is not examined stages and walks nothing and reports n_samples ORC_VERDICT_SKIPPED.
   const unsigned char * examine;   // [n_runs] nonzero: examine the run; NULL: every run, or the candidates below
   const int * cand_status;    // [n_runs] with examine NULL: the runs orc_run_candidate (run_candidate.h) passes on the status ...
   const double * cand_costs;  // [n_runs][3] ... and the costs an iterate call left; both NULL: every run
   int * n_samples_out;        // [n_runs] samples of the run's trajectory; ORC_VERDICT_SKIPPED: not examined; ORC_VERDICT_TOO_LONG
};

// the first contact of every examined run (collision_verdict_planned_kernel).  A run that is not examined or too long has key
// ORC_VERDICT_NONE and time -1, its depth left as the caller zeroed it.
template <typename real>
struct DevVerdictPlan : DevVerdictPlanned<real>
{
   double * time_out;          // [n_runs] the first contact's time on the retimed trajectory, -1 without a contact
   int * too_long;             // [1] set when a run has 2^30 samples or more: nothing of that run is walked (the caller zeroes it)
   int count_rest;             // 1: the samples behind a contact are counted (n_samples_out is exact); 0: n_samples_out is what was
                               // planned when the walk stopped, and "too long" is only what is decided before anything is walked
   int long_marks_run;         // 0: a run that is too long sets *too_long; 1: it reports like a run that is not examined, with
                               // n_samples ORC_VERDICT_TOO_LONG, and *too_long stays
};
#define ORC_VERDICT_SKIPPED  (-1)
#define ORC_VERDICT_TOO_LONG (-2)

hipError_t orc_launch_verdict(const DevVerdict<double> & v, size_t lds, hipStream_t stream, int tree);
hipError_t orc_launch_verdict(const DevVerdict<float> & v, size_t lds, hipStream_t stream, int tree);
hipError_t orc_launch_verdict_planned(const DevVerdictPlan<double> & v, size_t lds, hipStream_t stream, int tree);
hipError_t orc_launch_verdict_planned(const DevVerdictPlan<float> & v, size_t lds, hipStream_t stream, int tree);
// dynamic LDS of collision_verdict_kernel and of collision_verdict_planned_kernel
size_t orc_verdict_lds_bytes(int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk);
size_t orc_verdict_planned_lds_bytes(int n_points, int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk);

// the most dynamic LDS a workgroup of these kernels takes (a CU has 160 KB): `chunk` is chosen under it, the launcher (verdict_planned.h) refuses more
#define ORC_VERDICT_LDS_LIMIT (160*1024 - 256)
