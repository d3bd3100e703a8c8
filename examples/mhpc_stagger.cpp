// A fleet whose robots tick at their own times (mhpc_tick_problems).  In the reference every
// robot is its own MHPCLocomotion and re-plans when its own gait mode ends: set_initial_condition,
// update_problem (MHPCLocomotion.cpp:107-158), solve_mhpc (:167-195).  Here one handle holds a
// fleet of 2 WB + 2 SRB controllers, the even robots on the default gait (BOUND: modes of 80 and
// 100 ms), the odd ones on the PRONK gait (80 ms each), started at different modes; the mode
// durations differ, so the robots reach their mode boundaries at different simulator steps (1 ms
// each).  At every step the robots whose current mode has ended -- and only they -- take the
// state at the end of phase 0 of their plan, advance one gait step and are solved again; the
// others keep following the plan they have.
// Prints one line per step with a tick: "step s ticked = b ...  J = ...".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mhpc_locomotion.hpp"

int main(int argc, char** argv) {
  const int batch = argc > 1 ? std::atoi(argv[1]) : 6;
  const int sim_steps = argc > 2 ? std::atoi(argv[2]) : 400;
  HSDDP_OPTION<double> option;
  option.max_AL_iter = 2;
  option.max_DDP_iter = 3;
  USRCMD usrcmd{1.5f, 0.f, 0.f, 0.f, 0.f};
  Gait bound, pronk(GaitType2D::PRONK);
  MHPCUserParameters p;
  p.n_wbphase = 2; p.n_fbphase = 2; p.usrcmd = &usrcmd;
  std::vector<mhpc_problem_desc> layouts;  // 2 gaits x 2 start modes
  for (Gait* g : {&bound, &pronk})
    for (int c : {1, 2}) {
      p.cmode = c;
      layouts.push_back(MHPCLocomotion<double>::build_desc(&p, g));
    }
  std::vector<int32_t> layout_of(batch), gait_of(batch);
  for (int b = 0; b < batch; ++b) {
    gait_of[b] = b % 2;
    layout_of[b] = 2 * gait_of[b] + (b / 2) % 2;
  }
  p.cmode = 1;
  MHPCLocomotion<double> fleet(&p, &bound, option, batch);
  fleet.set_layouts(layouts, layout_of);
  fleet.initialization();
  fleet.solve_mhpc();
  // simulator steps until each robot's current mode ends: the controls of phase 0 of its plan
  std::vector<int> left(batch);
  for (int b = 0; b < batch; ++b) {
    fleet.select_problem(b);
    left[b] = fleet.desc().N[0] - 1;
  }
  const int xw = fleet.x0_width();
  for (int s = 1; s <= sim_steps; ++s) {
    std::vector<int> due;
    std::vector<int32_t> g;
    std::vector<double> x0;
    for (int b = 0; b < batch; ++b) {
      if (--left[b] > 0) continue;
      due.push_back(b);
      g.push_back(gait_of[b]);
      fleet.select_problem(b);  // where the plan says the robot is when its mode ends
      const std::vector<double> xe = fleet._phases[0]->get_terminal_state();
      x0.insert(x0.end(), xe.begin(), xe.begin() + xw);
    }
    if (due.empty()) continue;
    fleet.tick_problems(due, x0, {&bound, &pronk}, g);
    std::printf("step %3d ticked =", s);
    for (int b : due) std::printf(" %d", b);
    std::printf("  J =");
    for (int b : due) {
      fleet.select_problem(b);
      std::printf(" %.9g", fleet._actual_cost);
      left[b] = fleet.desc().N[0] - 1;
    }
    std::printf("\n");
  }
  std::printf("layouts in use: %d\n", fleet.num_layouts());
  return 0;
}
