// TEST-ONLY host build of the hand-written elementary functions that have a host path
// (mhpc_dual.h: sin_cos_short, sin_cos, sin_cos_n; mhpc_model.h: div_const), so their accuracy
// can be held to the 60-digit references of tests/golden/prim_kat.npz on a CPU-only machine.
// Never linked into the product library.  Built twice, without contraction: as it stands
// (real = double) and with -DMHPC_FP32 (real = float; the inputs rounded to float and the
// results widened, as the library's hooks do).  log_pos, reduced_barrier, the fp64 device path
// of pivot_rcp and the sweep's recip are device code only: tests/test_gpu_primitives.py.
#include "../../mhpc_minimal_env_amd/csrc/mhpc_model.h"

using namespace MHPC_NS;

template <int N>
static void sin_cos_groups(int n, const double* a, double* s, double* c) {
  for (int g = 0; (g + 1) * N <= n; ++g) {
    real v[N], sv[N], cv[N];
    for (int i = 0; i < N; ++i) v[i] = real(a[g * N + i]);
    sin_cos_n<N>(v, sv, cv);
    for (int i = 0; i < N; ++i) {
      s[g * N + i] = sv[i];
      c[g * N + i] = cv[i];
    }
  }
}
extern "C" {

void hc_sin_cos(int n, const double* a, double* s, double* c) {
  for (int i = 0; i < n; ++i) {
    real sv, cv;
    sin_cos(real(a[i]), &sv, &cv);
    s[i] = sv;
    c[i] = cv;
  }
}

#ifndef MHPC_FP32
// the short reduction alone, also past the |a| <= 1e5 it is used on
void hc_sin_cos_short(int n, const double* a, double* s, double* c) {
  for (int i = 0; i < n; ++i) sin_cos_short(a[i], &s[i], &c[i]);
}
#endif

// groups of N = 5 or 3 consecutive angles (n a multiple of N)
void hc_sin_cos_n(int N, int n, const double* a, double* s, double* c) {
  if (N == 5) sin_cos_groups<5>(n, a, s, c);
  else sin_cos_groups<3>(n, a, s, c);
}

// a / c by div_const: c the SRB mass (which = 0) or inertia
void hc_div_const(int n, int which, const double* a, double* out) {
  for (int i = 0; i < n; ++i)
    out[i] = which == 0 ? div_const(real(a[i]), kSrbMass, kSrbMassRcp)
                        : div_const(real(a[i]), kSrbInertia, kSrbInertiaRcp);
}
void hc_div_const_c(double* c) {
  c[0] = kSrbMass;
  c[1] = kSrbInertia;
}

}  // extern "C"
