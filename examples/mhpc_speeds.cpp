// A speed sweep in one batch (the batch axis over user commands).  In the reference every
// controller owns its MHPCUserParameters::usrcmd, which build_problem hands to ReferenceGen
// (MHPCLocomotion.cpp:98-103): a sweep over speed commands is one MHPCLocomotion per speed.
// Here one handle holds them all: the 2 WB + 2 SRB PRONK controller (config C3), problem b
// commanded to 0.5 ... 2.5 m/s, solved once.
// Prints one line per problem: "problem b vel v height z J = ... vx_end = ...", vx_end being
// the forward velocity at the last knot of the horizon.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mhpc_locomotion.hpp"

int main(int argc, char** argv) {
  const int batch = argc > 1 ? std::atoi(argv[1]) : 9;
  HSDDP_OPTION<double> option;
  USRCMD usrcmd{1.5f, 0.f, 0.f, 0.f, 0.f};
  Gait pronk(GaitType2D::PRONK);
  MHPCUserParameters params;
  params.n_wbphase = 2; params.n_fbphase = 2; params.usrcmd = &usrcmd;
  MHPCLocomotion<double> sweep(&params, &pronk, option, batch);
  std::vector<float> vel(batch);
  for (int b = 0; b < batch; ++b) vel[b] = batch > 1 ? 0.5f + 2.0f * b / (batch - 1) : 1.5f;
  sweep.set_commands(vel);
  sweep.initialization();
  sweep.solve_mhpc();
  std::vector<double> v, z;
  sweep.get_commands(v, z);
  for (int b = 0; b < batch; ++b) {
    sweep.select_problem(b);
    // the last phase is single-rigid-body: state (x, z, pitch, vx, vz, pitch rate)
    const std::vector<double> xe = sweep._phases.back()->get_terminal_state();
    std::printf("problem %d vel %.9g height %.9g J = %.17g vx_end = %.9g\n", b, v[b], z[b],
                sweep._actual_cost, xe[3]);
  }
  return 0;
}
