// nls_observe.hpp -- host-visible handles of the observable kernels (nls_observe.hip):
// one radius-1 stencil-and-reduce pass over the field (k_observe) and the single
// workgroup that sums its partials in fixed order and writes one nls_observables
// record (k_observe_finish).  Definitions: include/nls.h, DESIGN.md "Observables".
#pragma once
#include "nls_device.hpp"

namespace nls {

// Summed columns of one observation, as pairs in cplx words (block_store / sum_partials /
// allreduce_sums all move cplx): {mass, kinetic}, {p4, p6}, {vel2, potential}, {nonfinite, -}
constexpr int OBS_NCOL = 4;
// words of the device sums buffer: OBS_NCOL summed columns, then the slab's max |u|^2 in
// [OBS_NCOL].re (never all-reduced: the transports only sum)
constexpr int OBS_NSUM = OBS_NCOL + 1;
constexpr int OBS_NFIELDS = 10;  // == NLS_OBS_NFIELDS

// Equation class of k_observe (template argument EQ).
//   complex fields: OBS_W1 w = 1 (G1 cubic, G1 cubic-quintic), OBS_WM w = m(x) (G2 cubic, G2 cubic-quintic)
//   real fields: the potential density G, 0 1-cos u, 1 (1-cos u) + 2(1-cos(u/2)), 2 cosh u - 1,
//                3 u^2/2 + u^4/4 (0..3 == GautschiForce), 4 u^4/4 (Klein-Gordon)
// Two value spaces, told apart by the field type S: distinct ranges, so a value of one
// can never select a kernel of the other.
enum ObsEqComplex { OBS_W1 = 16, OBS_WM = 17 };
enum ObsEqReal { OBS_G_SIN = 0, OBS_G_SIN_DOUBLE = 1, OBS_G_SINH = 2, OBS_G_PHI4 = 3, OBS_G_KG = 4 };

// Per-cell inputs besides the stencil vector (local plane 0, no ghost planes).
struct ObsArgs {
  const double *mf;   // w = m(x); complex EQ 0: unused
  const double *up;   // real fields: u_past
  const double *vel;  // real fields: stored velocity (KG after a step), else NULL: (u - u_past) / dt
  double dt;
};

// What the finishing kernel needs to form potential and energy.
struct ObsFin {
  double step;     // record field 0
  double c4, c6;   // complex fields: energy = kinetic + c4 p4 + c6 p6
  int32_t real_;   // real fields: energy = vel2 / 2 + kinetic / 2 + potential
  int32_t pad;
};

//   observe        : (const S* V, Geo g, ObsArgs a, cplx* part, double* pmax)
//                    part: OBS_NCOL column-major partial columns of gridDim.x, pmax[gridDim.x]
//   observe_finish : (const cplx* part, const double* pmax, int nb, cplx* sums, int do_sum,
//                     int do_fin, ObsFin f, double* rec)
//                    do_sum 1: partials -> sums[0..OBS_NSUM); 2: the column sums are in sums
//                    already (k_colsum), only the max is reduced; do_fin: sums -> rec[0..10)
const void *kernel_observe(bool complex_, int dim, bool ani, int eq);
const void *kernel_observe_finish();
int observe_rows_per_thread();

}  // namespace nls
