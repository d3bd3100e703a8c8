// Learning from the MPC with the dataset on the device: every tick of a receding-horizon loop the
// fleet's plans -- each robot's first-phase policy window (x_nom, u_nom, K, du, Vx, y per control
// step) and the results of its solve (J, dV_exp, viol, V and dV per phase, status) -- go straight
// into slice t of dataset arrays that live in device memory, as an imitation / value learner's
// buffers do; nothing crosses the host.  A fleet of 4 PRONK controllers (2 WB + 2 SRB, config C3)
// runs a few ticks of
//   update_problem (initialization on tick 0), solve_mhpc, export_plan_device, export_results_device
// with the policy arrays laid out [robot][tick][step][c] (the export writes one robot's
// [step][c] block per tick and leaves the rest of the array alone: ld = ticks * steps * c) and the
// results [tick][robot].  The stand-in simulator is the solver's own model, as in mhpc_sim.
// At the end the dataset is copied to the host once and compared with what the host getters
// (mhpc_get_phase_problems, mhpc_get_scalars, the solve's status) reported at the same ticks.
// Prints one line per tick, "tick t J = <cost of robot 0> window = <steps> ms = <device ms>", and
// "worst |device - host| = <d>".  d is 0.
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
#define MHPC_OK_(expr)                                                            \
  do {                                                                            \
    if ((expr) != MHPC_OK) {                                                      \
      std::fprintf(stderr, "%s: %s\n", #expr, mhpc_last_error());                 \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

static double worst = 0;
static void diff(double dev, double host) {
  const double d = std::fabs(dev - host);
  worst = (d > worst || std::isnan(d)) ? d : worst;
}

int main(int argc, char** argv) {
  const int T = argc > 1 ? std::atoi(argv[1]) : 3;
  const int B = argc > 2 ? std::atoi(argv[2]) : 4;
  const int WD = 110;  // steps a slice holds: a phase buffer's knots (N_TIMESTEPS_MAX)
  HSDDP_OPTION<double> option;
  USRCMD usrcmd{1.5f, 0.f, 0.f, 0.f, 0.f};
  Gait pronk(GaitType2D::PRONK);
  MHPCUserParameters params;
  params.n_wbphase = 2; params.n_fbphase = 2; params.usrcmd = &usrcmd;
  MHPCLocomotion<double> fleet(&params, &pronk, option, B);
  const int r = 14;
  int P = 0;
  MHPC_OK_(mhpc_max_phases(fleet.handle(), &P));

  // the dataset: policy arrays [B][T][WD][c], mode [B][T][WD], valid and results [T][B]
  const int cols[6] = {r, 4, 4 * r, 4, r, 4};  // x_nom, u_nom, K, du, Vx, y
  double* dpol[6];
  for (int a = 0; a < 6; ++a) {
    HIP_OK(hipMalloc((void**)&dpol[a], sizeof(double) * B * T * WD * cols[a]));
    HIP_OK(hipMemset(dpol[a], 0, sizeof(double) * B * T * WD * cols[a]));
  }
  int32_t *dmode = nullptr, *dvalid = nullptr, *dstatus = nullptr;
  double* dres[5];  // J, dV_exp, viol [T][B]; V_phase, dV_phase [T][B][P]
  HIP_OK(hipMalloc((void**)&dmode, sizeof(int32_t) * B * T * WD));
  HIP_OK(hipMemset(dmode, 0, sizeof(int32_t) * B * T * WD));
  HIP_OK(hipMalloc((void**)&dvalid, sizeof(int32_t) * T * B));
  HIP_OK(hipMalloc((void**)&dstatus, sizeof(int32_t) * T * B));
  for (int a = 0; a < 5; ++a) HIP_OK(hipMalloc((void**)&dres[a], sizeof(double) * T * B * (a < 3 ? 1 : P)));

  // what the host getters report, tick by tick
  struct Tick {
    int N, mode;
    std::vector<double> x, u, y, K, du, Vx, J, dV_exp, viol, V, dV;
    std::vector<int32_t> status;
  };
  std::vector<Tick> ticks(T);

  for (int t = 0; t < T; ++t) {
    if (t == 0) fleet.initialization();
    else fleet.update_problem();
    fleet.solve_mhpc();
    const int N = fleet.desc().N[0], W = N - 1;  // the first phase's control steps
    if (W > WD) {
      std::fprintf(stderr, "first phase longer than a slice\n");
      return 1;
    }

    // plans and results into slice t of the dataset, on the device
    mhpc_plan_out po = {};
    const size_t at = (size_t)t * WD;
    po.x_nom = dpol[0] + at * cols[0]; po.ld_x_nom = (int64_t)T * WD * cols[0];
    po.u_nom = dpol[1] + at * cols[1]; po.ld_u_nom = (int64_t)T * WD * cols[1];
    po.K = dpol[2] + at * cols[2];     po.ld_K = (int64_t)T * WD * cols[2];
    po.du = dpol[3] + at * cols[3];    po.ld_du = (int64_t)T * WD * cols[3];
    po.Vx = dpol[4] + at * cols[4];    po.ld_Vx = (int64_t)T * WD * cols[4];
    po.y = dpol[5] + at * cols[5];     po.ld_y = (int64_t)T * WD * cols[5];
    po.mode = dmode + at;              po.ld_mode = (int64_t)T * WD;
    po.valid = dvalid + (size_t)t * B;
    const float ms = fleet.export_plan_device({}, {}, W, po);
    mhpc_results_out ro = {};
    ro.J = dres[0] + (size_t)t * B;
    ro.dV_exp = dres[1] + (size_t)t * B;
    ro.viol = dres[2] + (size_t)t * B;
    ro.V_phase = dres[3] + (size_t)t * B * P;
    ro.dV_phase = dres[4] + (size_t)t * B * P;
    ro.status = dstatus + (size_t)t * B;
    fleet.export_results_device({}, ro);

    // the same through the host getters
    Tick& k = ticks[t];
    k.N = N;
    k.mode = fleet.desc().mode_seq[0];
    k.x.resize((size_t)B * N * r); k.u.resize((size_t)B * N * 4); k.y.resize((size_t)B * N * 4);
    k.K.resize((size_t)B * N * 4 * r); k.du.resize((size_t)B * N * 4); k.Vx.resize((size_t)B * N * r);
    MHPC_OK_(mhpc_get_phase_problems(fleet.handle(), 0, 0, B, k.x.data(), k.u.data(), k.y.data(),
                                     k.K.data(), k.du.data(), k.Vx.data()));
    k.J.resize(B); k.dV_exp.resize(B); k.viol.resize(B);
    k.V.resize((size_t)B * P); k.dV.resize((size_t)B * P);
    MHPC_OK_(mhpc_get_scalars(fleet.handle(), k.J.data(), k.dV_exp.data(), k.viol.data(), k.V.data(),
                              k.dV.data(), nullptr));
    k.status = fleet.status();
    std::printf("tick %d J = %.17g window = %d ms = %.4f\n", t, k.J[0], W, ms);

    // the stand-in simulator: each robot's first phase under its policy, with a pitch-rate kick
    std::vector<double> push((size_t)B * 14, 0.0);
    for (int b = 0; b < B; ++b) push[(size_t)b * 14 + 9] = (t % 2 ? -0.05 : 0.05) * (b + 1);
    fleet.advance_x0(1, push);
  }

  // the dataset to the host, once, against the ticks' host copies
  std::vector<double> pol[6], res[5];
  for (int a = 0; a < 6; ++a) {
    pol[a].resize((size_t)B * T * WD * cols[a]);
    HIP_OK(hipMemcpy(pol[a].data(), dpol[a], sizeof(double) * pol[a].size(), hipMemcpyDeviceToHost));
  }
  for (int a = 0; a < 5; ++a) {
    res[a].resize((size_t)T * B * (a < 3 ? 1 : P));
    HIP_OK(hipMemcpy(res[a].data(), dres[a], sizeof(double) * res[a].size(), hipMemcpyDeviceToHost));
  }
  std::vector<int32_t> mode((size_t)B * T * WD), valid((size_t)T * B), status((size_t)T * B);
  HIP_OK(hipMemcpy(mode.data(), dmode, sizeof(int32_t) * mode.size(), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(valid.data(), dvalid, sizeof(int32_t) * valid.size(), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(status.data(), dstatus, sizeof(int32_t) * status.size(), hipMemcpyDeviceToHost));
  double gain = 0;
  for (int t = 0; t < T; ++t) {
    const Tick& k = ticks[t];
    const int N = k.N, W = N - 1;
    for (int b = 0; b < B; ++b) {
      diff(valid[(size_t)t * B + b], W);
      diff(status[(size_t)t * B + b], k.status[b]);
      diff(res[0][(size_t)t * B + b], k.J[b]);
      diff(res[1][(size_t)t * B + b], k.dV_exp[b]);
      diff(res[2][(size_t)t * B + b], k.viol[b]);
      for (int p = 0; p < P; ++p) {
        diff(res[3][((size_t)t * B + b) * P + p], k.V[(size_t)b * P + p]);
        diff(res[4][((size_t)t * B + b) * P + p], k.dV[(size_t)b * P + p]);
      }
      for (int w = 0; w < WD; ++w) {
        const size_t o = ((size_t)b * T + t) * WD + w, h = (size_t)b * N + w;
        const bool in = w < W;  // the rest of the slice keeps its zeros
        diff(mode[o], in ? k.mode : 0);
        for (int c = 0; c < r; ++c) {
          diff(pol[0][o * r + c], in ? k.x[h * r + c] : 0.0);
          diff(pol[4][o * r + c], in ? k.Vx[h * r + c] : 0.0);
        }
        for (int c = 0; c < 4; ++c) {
          diff(pol[1][o * 4 + c], in ? k.u[h * 4 + c] : 0.0);
          diff(pol[3][o * 4 + c], in ? k.du[h * 4 + c] : 0.0);
          diff(pol[5][o * 4 + c], in ? k.y[h * 4 + c] : 0.0);
        }
        for (int c = 0; c < 4 * r; ++c) {
          diff(pol[2][o * 4 * r + c], in ? k.K[h * 4 * r + c] : 0.0);
          if (in) gain = std::fmax(gain, std::fabs(pol[2][o * 4 * r + c]));
        }
      }
    }
  }
  std::printf("largest |K| in the dataset = %.6g\n", gain);
  std::printf("worst |device - host| = %.17g\n", worst);
  for (int a = 0; a < 6; ++a) (void)hipFree(dpol[a]);
  for (int a = 0; a < 5; ++a) (void)hipFree(dres[a]);
  (void)hipFree(dmode);
  (void)hipFree(dvalid);
  (void)hipFree(dstatus);
  return (worst == 0 && gain > 0) ? 0 : 1;
}
