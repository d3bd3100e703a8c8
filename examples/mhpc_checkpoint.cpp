// Checkpoint and resume (the batch axis over controller lifetimes across processes).  In the
// reference a controller is an object in one process: when the process ends, its warm starts,
// rotated phase buffers and AL / ReB state are gone, and the only "resume" is initialization()
// again -- a different trajectory from the first tick on.  Here a fleet of R robots (2 WB + 2 SRB
// PRONK, config C3, each with its own speed command) runs receding-horizon ticks in a closed loop
// on the device; --save FILE snapshots the whole fleet after the last tick (save_problems), and a
// second run with --resume FILE builds its fleet from that file (from_snapshot) and goes on where
// the first stopped.  One line per robot per tick, costs with %.17g: a run split in two prints the
// lines of a straight-through run.
//   mhpc_checkpoint --ticks 4
//   mhpc_checkpoint --ticks 2 --save fleet.snap && mhpc_checkpoint --ticks 4 --resume fleet.snap
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "mhpc_locomotion.hpp"

int main(int argc, char** argv) {
  int ticks = 4, R = 3;
  std::string save, resume;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--ticks" && i + 1 < argc) ticks = std::atoi(argv[++i]);
    else if (a == "--robots" && i + 1 < argc) R = std::atoi(argv[++i]);
    else if (a == "--save" && i + 1 < argc) save = argv[++i];
    else if (a == "--resume" && i + 1 < argc) resume = argv[++i];
    else {
      std::fprintf(stderr, "usage: %s [--ticks N] [--robots R] [--save FILE] [--resume FILE]\n", argv[0]);
      return 2;
    }
  }
  Gait pronk(GaitType2D::PRONK);
  std::unique_ptr<MHPCLocomotion<double>> fleet;
  int t0 = 0;  // ticks already run (kept beside the blob: a blob holds controllers, not a clock)
  if (!resume.empty()) {
    fleet = MHPCLocomotion<double>::from_snapshot(MHPCLocomotion<double>::load_snapshot(resume), &pronk);
    std::ifstream(resume + ".tick") >> t0;
    R = (int)fleet->status().size();
  } else {
    HSDDP_OPTION<double> option;
    USRCMD usrcmd{1.5f, 0.f, 0.f, 0.f, 0.f};
    MHPCUserParameters params;
    params.n_wbphase = 2; params.n_fbphase = 2; params.usrcmd = &usrcmd;
    fleet.reset(new MHPCLocomotion<double>(&params, &pronk, option, R));
    const double x0d[14] = {0.0927, -0.1093, -0.1542, 1.0957, -2.2033, 0.9742, -1.7098,
                            0.9011, 0.2756,  0.7333,  0.0446, 0.0009,  1.3219, 2.7346};
    std::vector<double> x0((size_t)R * 14);
    std::vector<float> vel(R);
    for (int b = 0; b < R; ++b) {
      for (int i = 0; i < 14; ++i) x0[(size_t)b * 14 + i] = x0d[i] + (i == 7 ? 0.02 * b : 0.0);
      vel[b] = 1.2f + 0.15f * b;
    }
    fleet->set_commands(vel);
    fleet->set_initial_conditions(x0);
    fleet->initialization();
  }
  for (int t = t0; t < ticks; ++t) {
    if (t > 0) {  // closed loop on the device: x0 <- where phase 0 of the last solution ends
      fleet->advance_x0(1);
      fleet->update_problem();
    }
    fleet->solve_mhpc();
    for (int b = 0; b < R; ++b) {
      fleet->select_problem(b);
      std::printf("tick %d robot %d J = %.17g viol = %.17g\n", t, b, fleet->_actual_cost,
                  fleet->_tconstr_violation);
    }
  }
  if (!save.empty()) {
    fleet->save_problems(save);
    std::ofstream(save + ".tick") << ticks << "\n";
    std::printf("saved %d robots after %d ticks to %s\n", R, ticks, save.c_str());
  }
  return 0;
}
