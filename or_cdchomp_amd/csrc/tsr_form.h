// tsr_form.h -- which form of the structured constraint solve a batch takes (tsr.h phase_tsr), for the device and for the host.
//
// One definition of every condition: phase_tsr takes ORC_TSR_FORM_WIDTH and asks the tsr_form_is_* rungs below, and tsr_form puts
// the same rungs together in the same order for the host (orc_batch_get_state "tsr_plan", orc_host_tsr_form), so that a test can
// say which form it ran.  The rungs are inlined before anything else is, as if their text stood in the ladder: the iterate
// kernels' device code is what it was when it did.
// No HIP types: BLOCK threads per workgroup, m moving waypoints, n columns, Nm = n + (most constrained rows on one point), the
// block [S | r] of a point at its largest.
#pragma once

#ifndef ORC_HD
#if defined(__HIPCC__)
#define ORC_HD __host__ __device__
#else
#define ORC_HD
#endif
#endif

struct TsrForm
{
   int width;      // lanes per row of the register form: 16 or 32; 0: the LDS form of one wavefront (tsr_block_thomas)
   int regs;       // registers per lane of tsr_eliminate_regs<real, width, regs>
   int aug;        // the augmented block fits the rows as well (tsr_eliminate_regs<.., true>)
   int meet;       // tsr_meet_regs<meet>; 0: tsr_meet
   int subst_w;    // tsr_substitute<real, dir, subst_w, subst_u>
   int subst_u;
};

#define ORC_FORM ORC_HD inline __attribute__((always_inline))

// the register form's padded width into `shape`, which starts at 0, the LDS form (one wavefront).  A block [S | r] of N = n +
// (constrained rows of the point) rows needs N + 1 columns: rows of 16 lanes up to N = 15 (a 7-dof arm with up to eight
// constrained rows on a point), rows of 32 lanes up to N = 24; the row lists of a point hold 16 entries: more constrained rows on
// one point take the dense path.  (Two statements as text, for phase_tsr: the value of a function, even of one inlined at once,
// leaves the kernel's blocks in another order, and its device code is held to what it was.)
#define ORC_TSR_FORM_WIDTH(shape, BLOCK, m, n, Nm) \
   if ((BLOCK) >= 128 && (m) >= 4 && (n) <= 23) \
      shape = ((Nm) <= 15) ? 16 : (((Nm) <= 24) ? 32 : 0); \
   if ((Nm) - (n) > 16) shape = 0;

inline int tsr_form_width(int BLOCK, int m, int n, int Nm)
{
   int shape = 0;
   ORC_TSR_FORM_WIDTH(shape, BLOCK, m, n, Nm)
   return shape;
}

// the rungs of the elimination's ladder, asked in this order; the last form, 32 lanes and 12 registers, is what is left
ORC_FORM bool tsr_form_is_16_2_aug(int shape, int n, int Nm) { return shape == 16 && Nm <= 8 && Nm + n + 1 <= 16; }      // (the augmented block fits as well: see AUG)
ORC_FORM bool tsr_form_is_16_2(int shape, int Nm) { return shape == 16 && Nm <= 8; }       // (four rows per register)
ORC_FORM bool tsr_form_is_16_3(int shape, int Nm) { return shape == 16 && Nm <= 12; }      // (a WAM point with up to five constrained rows)
ORC_FORM bool tsr_form_is_16_4(int shape) { return shape == 16; }
ORC_FORM bool tsr_form_is_32_8(int Nm) { return Nm <= 16; }                                // (two rows per register)
ORC_FORM bool tsr_form_is_32_10(int Nm) { return Nm <= 20; }
// ... of the meet's and the substitution's, which go by the columns alone: tsr_meet_regs<2> and tsr_substitute<8, 1>, then
// tsr_meet_regs<4> and tsr_substitute<16, 4>; tsr_meet and tsr_substitute<0, 1> are what is left
ORC_FORM bool tsr_form_is_meet_2(int n) { return n <= 7; }
ORC_FORM bool tsr_form_is_meet_4(int n) { return n <= 15; }

// the whole decision, for the host's report
inline TsrForm tsr_form(int BLOCK, int m, int n, int Nm)
{
   TsrForm f = { tsr_form_width(BLOCK, m, n, Nm), 0, 0, 0, 0, 0 };
   const int shape = f.width;
   if (!shape) return f;
   if (tsr_form_is_16_2_aug(shape, n, Nm)) { f.regs = 2; f.aug = 1; }
   else if (tsr_form_is_16_2(shape, Nm)) f.regs = 2;
   else if (tsr_form_is_16_3(shape, Nm)) f.regs = 3;
   else if (tsr_form_is_16_4(shape)) f.regs = 4;
   else if (tsr_form_is_32_8(Nm)) f.regs = 8;
   else if (tsr_form_is_32_10(Nm)) f.regs = 10;
   else f.regs = 12;
   if (tsr_form_is_meet_2(n)) { f.meet = 2; f.subst_w = 8; f.subst_u = 1; }
   else if (tsr_form_is_meet_4(n)) { f.meet = 4; f.subst_w = 16; f.subst_u = 4; }
   else { f.meet = 0; f.subst_w = 0; f.subst_u = 1; }
   return f;
}
