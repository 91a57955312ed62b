// nls_observe.hip -- on-device observables (nls_observe / nls_monitor, include/nls.h).
//
// k_observe marches the field once with the handle's own operator (march, nls_stencil.hpp:
// cur = u_p and lap = (L u)_p per cell, 16 B/cell for a complex field) and reduces, per
// thread, the grid sums of DESIGN.md "Observables" together with the maximum of |u|^2 over
// the finite cells and the count of non-finite ones; block_store writes one partial per
// workgroup and column.  k_observe_finish, one workgroup, sums the partials in fixed order
// (sum_partials), so a record is bitwise reproducible run to run, forms potential and
// energy and writes the record.  No atomics on doubles, nothing in scratch.
#include "nls_observe.hpp"
#include "nls_reduce.hpp"
#include "nls_stencil.hpp"

#include <type_traits>

namespace nls {

constexpr int OBS_RB = 1;  // rows per thread: k_alpha_l2's shape (RB_L2), the same 16 B/cell stream
int observe_rows_per_thread() { return OBS_RB; }

namespace {

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// potential density G(u) of the real equations (include/nls.h); the 1 - cos and cosh - 1
// forms as squares of half-angle values, which do not cancel for small u
template <int EQ> __device__ __forceinline__ double obs_G(double u) {
  if constexpr (EQ == OBS_G_PHI4) {
    const double u2 = u * u;
    return 0.5 * u2 + 0.25 * (u2 * u2);
  } else if constexpr (EQ == OBS_G_KG) {
    const double u2 = u * u;
    return 0.25 * (u2 * u2);
  } else if constexpr (EQ == OBS_G_SINH) {
    // sinh(u/2): Taylor series below 2^-5 (where e^y - e^-y would cancel), else from exp;
    // both evaluated and selected, so the pass keeps one uniform control flow
    const double y = 0.5 * fabs(u), z = y * y;
    const double st = y + y * z * (1.0 / 6.0 + z * (1.0 / 120.0 + z * (1.0 / 5040.0 + z * (1.0 / 362880.0))));
    const double sh = y < 0.03125 ? st : 0.5 * (exp(y) - exp(-y));
    return 2.0 * (sh * sh);
  } else {
    double sn, cs;
    nl_sincos(0.5 * u, sn, cs);
    double G = 2.0 * (sn * sn);  // 1 - cos u
    if constexpr (EQ == OBS_G_SIN_DOUBLE) {
      nl_sincos(0.25 * u, sn, cs);
      G += 4.0 * (sn * sn);  // 2 (1 - cos(u/2))
    }
    return G;
  }
}

template <class S, int DIM, bool ANI, int EQ>
__global__ __launch_bounds__(NTHREADS) void k_observe(const S *__restrict__ V, Geo g, ObsArgs a,
                                                      cplx *__restrict__ part, double *__restrict__ pmax) {
  constexpr bool CX = std::is_same<S, cplx>::value;
  double mass = 0.0, kin = 0.0, p4 = 0.0, p6 = 0.0, vel2 = 0.0, pot = 0.0, nonf = 0.0, mx = 0.0;
  march<S, DIM, OBS_RB, false, ANI>(V, g, [&](int p, const S &c, const S &lap) {
    // |u|^2 with each operation rounded on its own (no contraction into an FMA): max_abs2
    // is then exactly the largest re*re + im*im a host computes from the same field
    // (the empty asm makes each product opaque, so the sum cannot absorb one)
    const cplx cc = to_c(c);
    double sr = cc.re * cc.re, si = cc.im * cc.im;
    asm volatile("" : "+v"(sr), "+v"(si));
    const double a2 = sr + si;
    bool fin;
    mass += a2;
    kin -= to_c(cj_mul(c, lap)).re;
    if constexpr (CX) {
      fin = isfinite(to_c(c).re) && isfinite(to_c(c).im);
      double w = 1.0;
      if constexpr (EQ == OBS_WM) w = a.mf[p];
      const double a4 = a2 * a2;
      p4 += w * a4;
      p6 += w * (a4 * a2);
    } else {
      const double u = to_c(c).re, up = a.up[p];
      fin = isfinite(u) && isfinite(up);
      const double v = a.vel ? a.vel[p] : (u - up) / a.dt;  // nls_get_sg_velocity's choice
      vel2 += v * v;
      pot += a.mf[p] * obs_G<EQ>(u);
    }
    if (fin) mx = fmax(mx, a2);
    else nonf += 1.0;
  });
  cplx v[OBS_NCOL] = {{mass, kin}, {p4, p6}, {vel2, pot}, {nonf, 0.0}};
  block_store<OBS_NCOL>(v, part, gridDim.x, 0);
  __shared__ double smax[NTHREADS / 64];
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = smax[0];
#pragma unroll
    for (int w = 1; w < NTHREADS / 64; ++w) m = fmax(m, smax[w]);
    pmax[blockIdx.x] = m;
  }
}

__global__ __launch_bounds__(NTHREADS) void k_observe_finish(const cplx *__restrict__ part,
                                                             const double *__restrict__ pmax, int nb,
                                                             cplx *__restrict__ sums, int do_sum, int do_fin,
                                                             ObsFin f, double *__restrict__ rec) {
  __shared__ cplx ssum[OBS_NSUM];
  __shared__ double smax[NTHREADS / 64];
  if (do_sum) {
    if (do_sum == 1) sum_partials(part, nb, OBS_NCOL, ssum);  // one wave per column, fixed order
    else if (threadIdx.x < OBS_NCOL) ssum[threadIdx.x] = sums[threadIdx.x];  // 2: k_colsum summed them
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;  // four loads in flight per thread
    int q = threadIdx.x;
    for (; q + 3 * NTHREADS < nb; q += 4 * NTHREADS) {
      m0 = fmax(m0, pmax[q]);
      m1 = fmax(m1, pmax[q + NTHREADS]);
      m2 = fmax(m2, pmax[q + 2 * NTHREADS]);
      m3 = fmax(m3, pmax[q + 3 * NTHREADS]);
    }
    for (; q < nb; q += NTHREADS) m0 = fmax(m0, pmax[q]);
    double m = wave_max(fmax(fmax(m0, m1), fmax(m2, m3)));
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      m = smax[0];
#pragma unroll
      for (int w = 1; w < NTHREADS / 64; ++w) m = fmax(m, smax[w]);
      ssum[OBS_NCOL] = {m, 0.0};
    }
    __syncthreads();
    if (!do_fin) {
      if (threadIdx.x < OBS_NSUM) sums[threadIdx.x] = ssum[threadIdx.x];
      return;
    }
  } else {
    if (threadIdx.x < OBS_NSUM) ssum[threadIdx.x] = sums[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double mass = ssum[0].re, kin = ssum[0].im, p4 = ssum[1].re, p6 = ssum[1].im;
  const double vel2 = ssum[2].re, potr = ssum[2].im;
  double pot, en;
  if (f.real_) {
    pot = potr;
    en = (0.5 * vel2 + 0.5 * kin) + pot;
  } else {
    en = kin + (f.c4 * p4 + f.c6 * p6);
    pot = en - kin;
  }
  rec[0] = f.step;
  rec[1] = mass;
  rec[2] = kin;
  rec[3] = f.real_ ? 0.0 : p4;
  rec[4] = f.real_ ? 0.0 : p6;
  rec[5] = f.real_ ? vel2 : 0.0;
  rec[6] = pot;
  rec[7] = en;
  rec[8] = ssum[OBS_NCOL].re;
  rec[9] = ssum[3].re;
}

template <class S, int EQ> const void *pick_iso(int dim) {
  return dim == 3 ? reinterpret_cast<const void *>(&k_observe<S, 3, false, EQ>)
                  : reinterpret_cast<const void *>(&k_observe<S, 2, false, EQ>);
}
template <class S, int EQ> const void *pick_ani(int dim) {
  return dim == 3 ? reinterpret_cast<const void *>(&k_observe<S, 3, true, EQ>)
                  : reinterpret_cast<const void *>(&k_observe<S, 2, true, EQ>);
}

}  // namespace

// Only what the ten equations need: complex iso {w = 1, w = m}, complex ani {w = m} (G2),
// real iso {the four G1 / G2 Gautschi potentials}, real ani {Klein-Gordon}; each 2D and 3D.
const void *kernel_observe(bool complex_, int dim, bool ani, int eq) {
  if (dim != 2 && dim != 3) return nullptr;
  if (complex_) {
    if (ani) return eq == OBS_WM ? pick_ani<cplx, OBS_WM>(dim) : nullptr;
    return eq == OBS_WM ? pick_iso<cplx, OBS_WM>(dim) : eq == OBS_W1 ? pick_iso<cplx, OBS_W1>(dim) : nullptr;
  }
  if (ani) return eq == OBS_G_KG ? pick_ani<double, OBS_G_KG>(dim) : nullptr;
  switch (eq) {
    case OBS_G_SIN: return pick_iso<double, OBS_G_SIN>(dim);
    case OBS_G_SIN_DOUBLE: return pick_iso<double, OBS_G_SIN_DOUBLE>(dim);
    case OBS_G_SINH: return pick_iso<double, OBS_G_SINH>(dim);
    case OBS_G_PHI4: return pick_iso<double, OBS_G_PHI4>(dim);
    default: return nullptr;
  }
}

const void *kernel_observe_finish() { return reinterpret_cast<const void *>(&k_observe_finish); }

}  // namespace nls
