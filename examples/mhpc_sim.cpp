// A fleet whose states and actions live in device buffers, as in a GPU simulator or an RL loop:
// every tick the controller reads the measured states from the simulator's state buffer and writes
// the torques to apply into its action buffer, and neither crosses the host.  The reference closes
// this loop on one CPU: set_initial_condition(x) with the measured state, update_problem, solve
// (MHPCLocomotion.cpp:107-158), then the first knot of the policy, u = u_nom + K (x - x_nom)
// (SinglePhase.cpp:117-144).  Here a fleet of 4 PRONK controllers (2 WB + 2 SRB, config C3) runs
//   set_x0_device, update_problem (initialization on tick 0), solve_mhpc, control_device
// on a state buffer [batch][16] and an action buffer [batch][8] of doubles (rows wider than the
// 14 states / 4 torques, as slices of a simulator's tensors are).
// The stand-in simulator is the solver's own model: advance_x0 runs each robot's policy over its
// first phase from the measured state plus a small disturbance, and the end state is written to
// the state buffer (a real simulator writes that buffer itself, on its own stream).
// Prints one line per tick, "tick t J = <cost of problem 0> u0 = <first torque of robot 0>", and
// at the end "worst |u_device - u_host| = <d>": the controls of the device path against
// mhpc_control on host copies of the same states, over all ticks.  d is 0.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mhpc_locomotion.hpp"

#define HIP_OK(expr)                                                              \
  do {                                                                            \
    const hipError_t e_ = (expr);                                                 \
    if (e_ != hipSuccess) {                                                       \
      std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));             \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

int main(int argc, char** argv) {
  const int ticks = argc > 1 ? std::atoi(argv[1]) : 4;
  const int batch = argc > 2 ? std::atoi(argv[2]) : 4;
  const int ldx = 16, ldu = 8;
  HSDDP_OPTION<double> option;
  USRCMD usrcmd{1.5f, 0.f, 0.f, 0.f, 0.f};
  Gait pronk(GaitType2D::PRONK);
  MHPCUserParameters params;
  params.n_wbphase = 2; params.n_fbphase = 2; params.usrcmd = &usrcmd;
  MHPCLocomotion<double> fleet(&params, &pronk, option, batch);

  // the simulator's buffers: states [batch][16], actions [batch][8]
  double *dX = nullptr, *dU = nullptr;
  HIP_OK(hipMalloc((void**)&dX, sizeof(double) * batch * ldx));
  HIP_OK(hipMalloc((void**)&dU, sizeof(double) * batch * ldu));
  const double x0d[14] = {0.0927, -0.1093, -0.1542, 1.0957, -2.2033, 0.9742, -1.7098,
                          0.9011, 0.2756,  0.7333,  0.0446, 0.0009,  1.3219, 2.7346};
  std::vector<double> X((size_t)batch * ldx, 0.0), U((size_t)batch * ldu, 0.0);
  for (int b = 0; b < batch; ++b)  // every robot starts a little faster than the one before it
    for (int i = 0; i < 14; ++i) X[(size_t)b * ldx + i] = x0d[i] + (i == 7 ? 0.02 * b : 0.0);
  HIP_OK(hipMemcpy(dX, X.data(), sizeof(double) * X.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dU, 0, sizeof(double) * U.size()));

  double worst = 0;
  for (int t = 0; t < ticks; ++t) {
    // measured states in, one solve, controls out: all on the device
    fleet.set_x0_device(dX, ldx);
    if (t == 0) fleet.initialization();
    else fleet.update_problem();
    fleet.solve_mhpc();
    fleet.control_device({}, dX, ldx, dU, ldu);

    // the same controls through the host, from host copies of the same states
    HIP_OK(hipMemcpy(X.data(), dX, sizeof(double) * X.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(U.data(), dU, sizeof(double) * U.size(), hipMemcpyDeviceToHost));
    std::vector<double> x((size_t)batch * 14);
    for (int b = 0; b < batch; ++b)
      for (int i = 0; i < 14; ++i) x[(size_t)b * 14 + i] = X[(size_t)b * ldx + i];
    const auto host = fleet.control({}, x);
    for (int b = 0; b < batch; ++b)
      for (int i = 0; i < 4; ++i) {
        const double d = std::fabs(U[(size_t)b * ldu + i] - host.u[(size_t)b * 4 + i]);
        worst = (d > worst || std::isnan(d)) ? d : worst;
      }
    std::printf("tick %d J = %.17g u0 = %.17g\n", t, fleet._actual_cost, U[0]);

    // the stand-in simulator: each robot's first phase under its policy from the measured state
    // plus a disturbance (a pitch-rate kick that alternates in sign), into the state buffer
    std::vector<double> push((size_t)batch * 14, 0.0);
    for (int b = 0; b < batch; ++b) push[(size_t)b * 14 + 9] = (t % 2 ? -0.05 : 0.05) * (b + 1);
    fleet.advance_x0(1, push);
    const std::vector<double> xn = fleet.get_x0();
    for (int b = 0; b < batch; ++b)
      for (int i = 0; i < 14; ++i) X[(size_t)b * ldx + i] = xn[(size_t)b * 14 + i];
    HIP_OK(hipMemcpy(dX, X.data(), sizeof(double) * X.size(), hipMemcpyHostToDevice));
  }
  std::printf("worst |u_device - u_host| = %.17g\n", worst);
  (void)hipFree(dX);
  (void)hipFree(dU);
  return worst == 0 ? 0 : 1;
}
