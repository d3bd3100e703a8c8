// Robots on different ground in one batch (the batch axis over cost weights and constraint
// parameters).  In the reference every MHPCLocomotion owns its WBConstraint object, whose
// _friccoeff bounds the ground-reaction-force cone (MHPCConstraints.cpp:14-88): a sweep over
// friction coefficients is one controller per coefficient.  Here one handle holds them all: the
// 2 WB + 2 SRB PRONK controller (config C3), 8 friction coefficients 0.3 ... 1.0 times 8 start
// states, problem b on coefficient b / 8 from start state b % 8, solved once.
// Prints one line per coefficient: "mu m J = <mean cost> viol = <largest violation>", over the
// coefficient's 8 start states.  Exits 1 if a problem's solve status is not MHPC_SOLVE_OK or
// if mhpc_get_problem_params does not read back what was set.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mhpc_locomotion.hpp"

int main() {
  const int n_mu = 8, n_x0 = 8, batch = n_mu * n_x0;
  HSDDP_OPTION<double> option;
  USRCMD usrcmd{1.5f, 0.f, 0.f, 0.f, 0.f};
  Gait pronk(GaitType2D::PRONK);
  MHPCUserParameters params;
  params.n_wbphase = 2; params.n_fbphase = 2; params.usrcmd = &usrcmd;
  MHPCLocomotion<double> fleet(&params, &pronk, option, batch);
  // every start state a little faster than the one before it.  (The friction coefficient acts
  // through the ReB barrier alone, which the reference switches on only in an AL iteration after
  // the first whose touchdown violation is below 0.05, MultiPhaseDDP.cpp:172-190: from these
  // states the second AL iteration gets there; from many others the coefficient changes nothing.)
  const double x0d[14] = {0.09672987, -0.11199392, -0.13969963, 1.11487634, -2.18401471,
                          0.96300834, -1.72134949, 0.92429674,  0.23890571, 0.76015309,
                          0.05130527, 0.03526379,  1.35191486,  2.69109069};
  std::vector<double> x0((size_t)batch * 14);
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < 14; ++i) x0[(size_t)b * 14 + i] = x0d[i] + (i == 7 ? 0.02 * (b % n_x0) : 0.0);
  std::vector<mhpc_constraint_params> ground(n_mu);
  std::vector<int32_t> set_of(batch);
  for (int m = 0; m < n_mu; ++m) {
    mhpc_default_constraint_params(&ground[m]);
    ground[m].friction_coeff = 0.3 + 0.1 * m;
  }
  for (int b = 0; b < batch; ++b) set_of[b] = b / n_x0;
  fleet.set_param_sets({}, ground, set_of);  // weights: the reference's for every robot
  int bad = 0;
  if (fleet.num_param_sets() != n_mu) {
    std::printf("expected %d parameter sets, the handle holds %d\n", n_mu, fleet.num_param_sets());
    bad = 1;
  }
  for (int b = 0; b < batch; ++b) {
    mhpc_constraint_params c;
    fleet.get_problem_params(b, nullptr, &c);
    if (c.friction_coeff != ground[set_of[b]].friction_coeff || c.torque_limit != 33) {
      std::printf("problem %d reads back friction %.17g\n", b, c.friction_coeff);
      bad = 1;
    }
  }
  fleet.set_initial_conditions(x0);
  fleet.initialization();
  fleet.solve_mhpc();
  for (int m = 0; m < n_mu; ++m) {
    double J = 0, viol = 0;
    for (int i = 0; i < n_x0; ++i) {
      const int b = m * n_x0 + i;
      if (fleet.status()[b] != MHPC_SOLVE_OK) {
        std::printf("problem %d solve status %d\n", b, (int)fleet.status()[b]);
        bad = 1;
      }
      fleet.select_problem(b);
      J += fleet._actual_cost / n_x0;
      viol = std::fmax(viol, fleet._tconstr_violation);
    }
    std::printf("mu %.9g J = %.17g viol = %.9g\n", ground[m].friction_coeff, J, viol);
  }
  return bad;
}
