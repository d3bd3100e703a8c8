// Warm-starting a fleet from another controller's plan (mhpc_import_plan).  In the reference a user
// who wants to start a controller from a guess writes into _phases[p]->get_nominal_ms_ptr() and
// get_CTG_info_ptr() between initialization() and solve_mhpc(): the first thing the solve does is
// a real rollout of u = u_nom + K (x - x_nom) from x0.  Here a donor handle solves the 2 WB + 2 SRB
// problem on the PRONK gait with the full budget.  A fleet of 8 robots at perturbed start states
// imports the donor's whole plan -- every phase (MHPC_STEPS_ALL), with the gains and the nominal
// states they refer to -- and solves under a small budget of one AL and one DDP iteration, beside
// a twin fleet at the same states that solves under the same budget from the PD warm start.
// Prints per robot: "robot b J imported = .. J pd = ..".
#include <cstdio>
#include <vector>

#include "mhpc_locomotion.hpp"

int main() {
  const int batch = 8;
  HSDDP_OPTION<double> full, small;
  small.max_AL_iter = 1;
  small.max_DDP_iter = 1;
  USRCMD usrcmd{1.5f, 0.f, 0.f, 0.f, 0.f};
  Gait pronk(GaitType2D::PRONK);
  MHPCUserParameters p;
  p.n_wbphase = 2; p.n_fbphase = 2; p.usrcmd = &usrcmd;

  MHPCLocomotion<double> donor(&p, &pronk, full, 1);
  donor.initialization();
  donor.solve_mhpc();
  const std::vector<double> xd = donor.get_x0();
  const int xw = donor.x0_width();

  // the donor's plan, step by step over all its phases, in rows of the x0 width
  const int W = donor.num_plan_steps(0, MHPC_STEPS_ALL);
  std::vector<double> u1((size_t)W * 4), K1((size_t)W * 4 * xw, 0.0), x1((size_t)W * xw, 0.0);
  donor.select_problem(0);
  size_t w = 0;
  for (auto& ph : donor._phases) {
    const size_t n = ph->_xsize, N = ph->_N_TIMESTEPS;
    for (size_t k = 0; k + 1 < N; ++k, ++w) {  // a phase's last knot has no control
      auto knot = [&](auto* ms, auto* ctg) {
        for (size_t i = 0; i < n; ++i) x1[w * xw + i] = ms[k].x(i);
        for (size_t i = 0; i < 4; ++i) u1[w * 4 + i] = ms[k].u(i);
        for (size_t i = 0; i < 4; ++i)
          for (size_t j = 0; j < n; ++j) K1[(w * 4 + i) * xw + j] = ctg[k].K(i, j);
      };
      if (n == 14)
        knot((ModelState<double, 14, 4, 4>*)ph->get_nominal_ms_ptr(),
             (CostToGoStruct<double, 14, 4>*)ph->get_CTG_info_ptr());
      else
        knot((ModelState<double, 6, 4, 4>*)ph->get_nominal_ms_ptr(),
             (CostToGoStruct<double, 6, 4>*)ph->get_CTG_info_ptr());
    }
  }
  if ((int)w != W) {
    std::printf("step count mismatch: %zu against %d\n", w, W);
    return 1;
  }
  // every robot gets the same guess
  std::vector<double> u, K, x;
  for (int b = 0; b < batch; ++b) {
    u.insert(u.end(), u1.begin(), u1.end());
    K.insert(K.end(), K1.begin(), K1.end());
    x.insert(x.end(), x1.begin(), x1.end());
  }
  // start states around the donor's: a few millimetres and milliradians, a few cm/s
  std::vector<double> x0((size_t)batch * xw);
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < xw; ++i)
      x0[(size_t)b * xw + i] = xd[i] + (i < xw / 2 ? 2e-3 : 2e-2) * (((b * 7 + i * 3) % 11) - 5) / 5.0;

  MHPCLocomotion<double> fleet(&p, &pronk, small, batch), twin(&p, &pronk, small, batch);
  fleet.set_initial_conditions(x0);
  twin.set_initial_conditions(x0);
  fleet.initialization();
  twin.initialization();
  fleet.import_plan({}, {}, W, u, K, x, MHPC_STEPS_ALL);
  fleet.solve_mhpc();
  twin.solve_mhpc();
  for (int b = 0; b < batch; ++b) {
    fleet.select_problem(b);
    twin.select_problem(b);
    std::printf("robot %d J imported = %.9g J pd = %.9g\n", b, (double)fleet._actual_cost,
                (double)twin._actual_cost);
  }
  return 0;
}
