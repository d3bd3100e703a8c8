// A disturbed closed loop on the device (the batch axis over measured start states).  The
// reference closes its loop on the host: set_initial_condition(x) with the measured state, then
// update_problem and solve (MHPCLocomotion.cpp:107-158); running the solved policy from a state
// is set_initial_condition + forward_sweep_dynamics_only(0) (SinglePhase.cpp:117-144).  Here a
// fleet of 8 PRONK controllers (2 WB + 2 SRB, config C3) runs 6 ticks of
//   solve_mhpc, advance_x0(1, push), update_problem
// where advance_x0 runs every problem's policy over its first phase from x0 + push on the
// device and makes the end state the next x0 -- no state crosses to the host in the loop.  The
// push is a pitch-rate kick of 0.5 rad/s on tick 2, zero on every other tick; a second fleet
// runs the same loop without it.
// Prints one line per tick: "tick t J = <cost of problem 0> dev = <largest |x0 - x0 of the
// undisturbed fleet| after the tick's advance>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mhpc_locomotion.hpp"

int main(int argc, char** argv) {
  const int ticks = argc > 1 ? std::atoi(argv[1]) : 6;
  const int batch = 8, kick_tick = 2;
  HSDDP_OPTION<double> option;
  USRCMD usrcmd{1.5f, 0.f, 0.f, 0.f, 0.f};
  Gait pronk(GaitType2D::PRONK);
  MHPCUserParameters params;
  params.n_wbphase = 2; params.n_fbphase = 2; params.usrcmd = &usrcmd;
  MHPCLocomotion<double> fleet(&params, &pronk, option, batch), calm(&params, &pronk, option, batch);
  // every robot of the fleet starts a little faster than the one before it
  const double x0d[14] = {0.0927, -0.1093, -0.1542, 1.0957, -2.2033, 0.9742, -1.7098,
                          0.9011, 0.2756,  0.7333,  0.0446, 0.0009,  1.3219, 2.7346};
  std::vector<double> x0((size_t)batch * 14), push((size_t)batch * 14, 0.0);
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < 14; ++i) x0[(size_t)b * 14 + i] = x0d[i] + (i == 7 ? 0.02 * b : 0.0);
  for (int b = 0; b < batch; ++b) push[(size_t)b * 14 + 9] = 0.5;  // entry 9: pitch rate
  fleet.set_initial_conditions(x0);
  calm.set_initial_conditions(x0);
  fleet.initialization();
  calm.initialization();
  for (int t = 0; t < ticks; ++t) {
    fleet.solve_mhpc();
    calm.solve_mhpc();
    fleet.advance_x0(1, t == kick_tick ? push : std::vector<double>());
    calm.advance_x0(1);
    const std::vector<double> xa = fleet.get_x0(), xb = calm.get_x0();
    double dev = 0;
    for (size_t i = 0; i < xa.size(); ++i) dev = std::fmax(dev, std::fabs(xa[i] - xb[i]));
    std::printf("tick %d J = %.17g dev = %.9g\n", t, fleet._actual_cost, dev);
    fleet.update_problem();
    calm.update_problem();
  }
  return 0;
}
