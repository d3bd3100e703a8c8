// Episodes inside a live fleet (the batch axis over controller lifetimes).  In the reference a
// fleet is a set of MHPCLocomotion objects and restarting one of them is set_initial_condition
// plus initialization() on that object (MHPCLocomotion.cpp:47-53); the others never notice.
// Here a fleet of 8 BOUND controllers (4 WB + 6 SRB, config C5) runs the device-side closed loop
// of mhpc_disturb.cpp,
//   solve_mhpc, advance_x0(1), update_problems
// for 12 ticks.  That loop is not stable for this gait: some robots' costs turn non-finite over
// the ticks (the algorithm's behaviour, the CPU oracle loses the same ones).  After each solve the
// lost robots are reset to their start state with reset_problems -- and robot 0 at tick 3 whatever
// its state, so the example never depends on a robot being lost -- and take no gait step in the
// following update_problems (steps 0: a fresh controller starts at its own first mode), while
// every other robot steps on with its warm start untouched.
// Prints one line per tick: "tick t finite = <robots with a finite cost> reset = <robots reset>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mhpc_locomotion.hpp"

int main(int argc, char** argv) {
  const int ticks = argc > 1 ? std::atoi(argv[1]) : 12;
  const int batch = 8, forced_tick = 3;
  HSDDP_OPTION<double> option;
  USRCMD usrcmd{1.5f, 0.f, 0.f, 0.f, 0.f};
  Gait bound;
  MHPCUserParameters params;
  params.n_wbphase = 4; params.n_fbphase = 6; params.usrcmd = &usrcmd;
  MHPCLocomotion<double> fleet(&params, &bound, option, batch);
  // every robot of the fleet starts a little faster than the one before it
  const double x0d[14] = {0.0927, -0.1093, -0.1542, 1.0957, -2.2033, 0.9742, -1.7098,
                          0.9011, 0.2756,  0.7333,  0.0446, 0.0009,  1.3219, 2.7346};
  std::vector<double> x0((size_t)batch * 14);
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < 14; ++i) x0[(size_t)b * 14 + i] = x0d[i] + (i == 7 ? 0.02 * b : 0.0);
  fleet.set_initial_conditions(x0);
  fleet.initialization();
  for (int t = 0; t < ticks; ++t) {
    fleet.solve_mhpc();
    std::vector<int> reset = fleet.lost_problems();
    const int finite = batch - (int)reset.size();
    if (t == forced_tick && std::find(reset.begin(), reset.end(), 0) == reset.end())
      reset.insert(reset.begin(), 0);
    fleet.advance_x0(1);  // (a lost robot's policy has no state to give: its row is reset below)
    std::vector<int32_t> steps(batch, 1);
    if (!reset.empty()) {
      std::vector<double> rows;
      for (int b : reset) {
        rows.insert(rows.end(), x0.begin() + (size_t)b * 14, x0.begin() + (size_t)(b + 1) * 14);
        steps[b] = 0;
      }
      fleet.reset_problems(reset, rows);
    }
    fleet.update_problems({&bound}, {}, steps);
    std::printf("tick %d finite = %d reset =", t, finite);
    for (int b : reset) std::printf(" %d", b);
    std::printf("\n");
  }
  return 0;
}
