// Per-precision implementation of the C-ABI (mhpc_runtime.cpp compiled once per arithmetic
// type into namespace API_NS); mhpc_capi.cpp exports the extern "C" symbols and dispatches
// on the descriptor's precision.  No include guard: included once per namespace.
namespace API_NS {
struct Handle;
const char* api_kernel_name(int k);
int api_create(const mhpc_problem_desc* desc, const mhpc_hsddp_option* opt, int batch, int device,
               Handle** out);
int api_set_x0(Handle* h, const double* x0);
int api_initialize(Handle* h);
int api_solve(Handle* h, int32_t* status);
int api_get_phase(Handle* h, int phase, int first, int count, double* x, double* u, double* y,
                  double* K, double* du, double* Vx);
int api_batch(Handle* h);
int api_get_scalars(Handle* h, double* J, double* dV_exp, double* viol, double* V_phase,
                    double* dV_phase, int32_t* trace);
int api_rollout_costs(Handle* h, int n_eps, const double* eps, double* J, double* viol, float* ms);
int api_rollout_policy(Handle* h, int n_samples, const double* xs, int n_phases, double* J,
                       double* viol, double* x_end, float* ms);
int api_rollout_policy_phase(Handle* h, int phase, int first, int count, int n_samples,
                             const double* xs, double* x, double* u, double* y);
int api_advance_x0(Handle* h, int n_phases, const double* dx);
int api_get_x0(Handle* h, double* x0);
int api_num_control_steps(Handle* h, int b, int* n);
int api_control(Handle* h, const int32_t* step, const double* x, double* u, double* x_nom,
                double* u_nom, double* K);
int api_control_device(Handle* h, const int32_t* step, const void* x, int64_t ldx, void* u,
                       int64_t ldu, void* x_nom, void* u_nom, void* K, int dtype, void* stream);
int api_set_x0_device(Handle* h, const void* x0, int64_t ld, int dtype, void* stream);
int api_export_plan_device(Handle* h, int n, const int32_t* problems, const int32_t* first_step,
                           int window, const mhpc_plan_out* out, int dtype, void* stream, float* ms);
int api_export_results_device(Handle* h, int n, const int32_t* problems,
                              const mhpc_results_out* out, int dtype, void* stream);
int api_num_plan_steps(Handle* h, int b, int scope, int* n);
int api_import_plan_device(Handle* h, int n, const int32_t* problems, const int32_t* first_step,
                           int window, int scope, const mhpc_plan_in* in, int dtype, void* stream,
                           float* ms);
int api_import_plan(Handle* h, int n, const int32_t* problems, const int32_t* first_step,
                    int window, int scope, const double* u_nom, const double* K,
                    const double* x_nom);
int api_get_cost_gradients(Handle* h, int phase, int first, int count, double* lx, double* Phix);
int api_update_problem(Handle* h, const mhpc_gait* gait);
int api_update_problems(Handle* h, int n_gaits, const mhpc_gait* gaits, const int32_t* gait_of,
                        const int32_t* steps);
int api_tick_problems(Handle* h, int n, const int32_t* problems, const double* x0, int n_gaits,
                      const mhpc_gait* gaits, const int32_t* gait_of, const int32_t* steps,
                      int32_t* status, float* ms);
int api_reserve_knots(Handle* h, int knots);
int api_set_layouts(Handle* h, int n_desc, const mhpc_problem_desc* descs, const int32_t* lop);
int api_reset_problems(Handle* h, int n, const int32_t* problems, const double* x0, int n_desc,
                       const mhpc_problem_desc* descs, const int32_t* desc_of);
int api_copy_problems(Handle* dst, const int32_t* dst_problems, Handle* src,
                      const int32_t* src_problems, int n, float* ms);
int api_snapshot_size(Handle* h, int n, const int32_t* problems, int64_t* bytes);
int api_snapshot_problems(Handle* h, int n, const int32_t* problems, void* blob, int64_t bytes,
                          float* ms);
int api_restore_problems(Handle* dst, int n, const int32_t* dst_problems, const void* blob,
                         int64_t bytes, const int32_t* entries, float* ms);
int api_snapshot_entry(const void* blob, int64_t bytes, int entry, mhpc_problem_desc* desc,
                       mhpc_hsddp_option* option, mhpc_cost_weights* w, mhpc_constraint_params* c);
int api_snapshot_status(const void* blob, int64_t bytes, int first, int count, int32_t* status);
int api_get_problem_desc(Handle* h, int b, mhpc_problem_desc* desc);
int api_set_commands(Handle* h, const double* vel, const double* height);
int api_get_commands(Handle* h, double* vel, double* height);
int api_get_reference(Handle* h, int phase, int first, int count, double* xref);
int api_num_layouts(Handle* h, int* n);
int api_max_phases(Handle* h, int* n);
int api_get_desc(Handle* h, mhpc_problem_desc* desc);
int api_get_counters(Handle* h, mhpc_counters* c);
int api_set_profiling(Handle* h, int on);
int api_get_kernel_stats(Handle* h, double* ms, int64_t* launches, double* alg_bytes);
int api_reset_kernel_stats(Handle* h);
int api_get_kernel_flops(Handle* h, double* flops);
int api_set_kernel_variant(Handle* h, int which, int variant);
int api_set_cost_weights(Handle* h, const mhpc_cost_weights* w);
int api_get_cost_weights(Handle* h, mhpc_cost_weights* w);
int api_set_constraint_params(Handle* h, const mhpc_constraint_params* c);
int api_get_constraint_params(Handle* h, mhpc_constraint_params* c);
int api_set_param_sets(Handle* h, int n_sets, const mhpc_cost_weights* w,
                       const mhpc_constraint_params* c, const int32_t* set_of);
int api_get_problem_params(Handle* h, int b, mhpc_cost_weights* w, mhpc_constraint_params* c);
int api_num_param_sets(Handle* h, int* n);
int api_set_options(Handle* h, const mhpc_hsddp_option* o);
int api_get_options(Handle* h, mhpc_hsddp_option* o);
int api_set_option_sets(Handle* h, int n_sets, const mhpc_hsddp_option* sets, const int32_t* set_of);
int api_get_problem_options(Handle* h, int b, mhpc_hsddp_option* o);
int api_num_option_sets(Handle* h, int* n);
void api_destroy(Handle* h);
}  // namespace API_NS
