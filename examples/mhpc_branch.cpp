// Branching in one batch (the batch axis over controller copies).  In the reference a controller
// is an object, and trying C speed commands from where a warm-started robot stands is C copies of
// that object, each with its own usrcmd, one update_problem and one solve each.  Here R robots
// (2 WB + 2 SRB PRONK, config C3) live in slots r * C of one batch of R * C and run a few
// receding-horizon ticks; then copy_problems forks each robot into the C - 1 slots behind it,
// warm start and all, the C slots of a robot get C speed commands, and one update_problems
// (steps 0: the candidates stay at the robot's gait point) plus one solve evaluates every
// candidate.  Prints one line per robot: "robot r best vel = v J = ...", the candidate with the
// smallest total cost.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mhpc_locomotion.hpp"

int main(int argc, char** argv) {
  const int R = argc > 1 ? std::atoi(argv[1]) : 2, C = argc > 2 ? std::atoi(argv[2]) : 4;
  const int ticks = 2, batch = R * C;
  HSDDP_OPTION<double> option;
  USRCMD usrcmd{1.5f, 0.f, 0.f, 0.f, 0.f};
  Gait pronk(GaitType2D::PRONK);
  MHPCUserParameters params;
  params.n_wbphase = 2; params.n_fbphase = 2; params.usrcmd = &usrcmd;
  MHPCLocomotion<double> fleet(&params, &pronk, option, batch);
  // robot r starts a little faster than the one before it (the slots behind it idle along)
  const double x0d[14] = {0.0927, -0.1093, -0.1542, 1.0957, -2.2033, 0.9742, -1.7098,
                          0.9011, 0.2756,  0.7333,  0.0446, 0.0009,  1.3219, 2.7346};
  std::vector<double> x0((size_t)batch * 14);
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < 14; ++i) x0[(size_t)b * 14 + i] = x0d[i] + (i == 7 ? 0.02 * (b / C) : 0.0);
  fleet.set_initial_conditions(x0);
  fleet.initialization();
  fleet.solve_mhpc();
  for (int t = 0; t < ticks; ++t) {
    fleet.advance_x0(1);
    fleet.update_problem();
    fleet.solve_mhpc();
  }
  // fork: slot r * C + c becomes robot r, c = 1 .. C - 1, and tries its own speed
  std::vector<int> dst, src;
  std::vector<float> vel(batch);
  for (int b = 0; b < batch; ++b) {
    if (b % C) {
      dst.push_back(b);
      src.push_back(b - b % C);
    }
    vel[b] = C > 1 ? 1.0f + 1.0f * (b % C) / (C - 1) : 1.5f;
  }
  fleet.advance_x0(1);  // where each robot stands now; the clones take their robot's row
  const float ms = dst.empty() ? 0.f : fleet.copy_problems(dst, src);
  fleet.set_commands(vel);
  fleet.update_problems({&pronk}, {}, std::vector<int32_t>(batch, 0));
  fleet.solve_mhpc();
  std::printf("forked %d robots into %d candidates each (copy: %.3f ms on the device)\n", R, C, ms);
  for (int r = 0; r < R; ++r) {
    int best = -1;
    double Jbest = 0;
    for (int c = 0; c < C; ++c) {
      fleet.select_problem(r * C + c);
      const double J = fleet._actual_cost;
      if (J == J && (best < 0 || J < Jbest)) {
        best = c;
        Jbest = J;
      }
    }
    std::printf("robot %d best vel = %.9g J = %.17g\n", r, best < 0 ? 0.0 : (double)vel[r * C + best], Jbest);
  }
  return 0;
}
