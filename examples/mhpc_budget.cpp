// A ticking fleet with per-robot solver budgets (mhpc_set_option_sets).  In the reference every
// robot is its own MHPCLocomotion with its own MultiPhaseDDP::_option.  A robot that has just been
// put back on its PD warm start (reset_problems) needs the full AL x DDP budget; the warm-started
// robots ticking beside it want the real-time-iteration budget of one AL iteration and two DDP
// iterations.  Here one handle holds a fleet of 2 WB + 2 SRB controllers on the PRONK gait.  Every
// round a few robots "fall" and are reset; they get the full option, everybody else (1, 2).  The
// round then ticks the warm robots and the fresh ones in two calls: the launch schedule of a tick
// runs to the largest budget among the listed robots, so the warm robots' tick is as short as
// their budget.
// Prints per round: "round r  warm n: .. ms  fresh m: .. ms  sets s".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mhpc_locomotion.hpp"

int main(int argc, char** argv) {
  const int batch = argc > 1 ? std::atoi(argv[1]) : 64;
  const int rounds = argc > 2 ? std::atoi(argv[2]) : 6;
  const int falls = argc > 3 ? std::atoi(argv[3]) : 2;  // robots reset per round
  HSDDP_OPTION<double> full, rti;
  full.max_AL_iter = 2;
  full.max_DDP_iter = 3;
  rti.max_AL_iter = 1;
  rti.max_DDP_iter = 2;
  USRCMD usrcmd{1.5f, 0.f, 0.f, 0.f, 0.f};
  Gait pronk(GaitType2D::PRONK);
  MHPCUserParameters p;
  p.n_wbphase = 2; p.n_fbphase = 2; p.usrcmd = &usrcmd;
  MHPCLocomotion<double> fleet(&p, &pronk, full, batch);
  fleet.initialization();
  const std::vector<double> xinit = fleet.get_x0();  // the rows a fallen robot restarts from
  fleet.solve_mhpc();
  const int xw = fleet.x0_width();
  for (int r = 0; r < rounds; ++r) {
    std::vector<char> fell(batch, 0);
    for (int i = 0; i < falls && i < batch; ++i) fell[(r * falls + i) % batch] = 1;
    std::vector<int> warm, fresh;
    std::vector<double> x0_warm, x0_fresh;
    std::vector<int32_t> set_of(batch);
    for (int b = 0; b < batch; ++b) {
      set_of[b] = fell[b] ? 0 : 1;
      if (fell[b]) {
        fresh.push_back(b);
        x0_fresh.insert(x0_fresh.end(), xinit.begin() + (size_t)b * xw, xinit.begin() + (size_t)(b + 1) * xw);
      } else {  // where the plan says the robot is when its mode ends
        warm.push_back(b);
        fleet.select_problem(b);
        const std::vector<double> xe = fleet._phases[0]->get_terminal_state();
        x0_warm.insert(x0_warm.end(), xe.begin(), xe.begin() + xw);
      }
    }
    fleet.set_option_sets({full, rti}, set_of);
    float ms_warm = 0, ms_fresh = 0;
    if (!warm.empty()) fleet.tick_problems(warm, x0_warm, {}, {}, {}, &ms_warm);
    if (!fresh.empty()) {
      // initialization() of the fallen robots, then their first solve with the full budget: a tick
      // without a gait step (their nominal is the warm start, not a rotated plan)
      fleet.reset_problems(fresh, x0_fresh);
      fleet.tick_problems(fresh, {}, {}, {}, std::vector<int32_t>(fresh.size(), 0), &ms_fresh);
    }
    std::printf("round %d  warm %zu: %.3f ms  fresh %zu: %.3f ms  sets %d\n", r, warm.size(), ms_warm,
                fresh.size(), ms_fresh, fleet.num_option_sets());
  }
  double J = 0;
  for (int b = 0; b < batch; ++b) {
    fleet.select_problem(b);
    J += fleet._actual_cost;
  }
  std::printf("mean J = %.9g\n", J / batch);
  return 0;
}
