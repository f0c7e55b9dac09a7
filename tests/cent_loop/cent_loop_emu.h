// TEST INFRASTRUCTURE: the entries of tests/cent_loop/cent_loop_emu.cpp, for that file and for tests/cent_loop/cent_loop_sanitize.cpp.
#pragma once
#include "../../include/hsqp_cent_loop.h"

extern "C" {
// the model image from the binding's hsqp_model_desc (a centroidal one), with the default joint state hsqp_set_default_joint_state would give it
void* cl_create(const hsqp_model_desc* md, const double* default_joint_state, char* err, int errlen);
void cl_destroy(void* h);
double cl_total_mass(void* h);
// k_command_targets_cent over B instances: v_cmd [B][4], v_filt [B][4] in / out, x0 [B][58], target_times [B][3], target_states [B][3][58], base_vel [B][6] or null
void cl_command_targets(void* h, double alpha, int B, const double* v_cmd, double* v_filt, const double* x0, double t0, double horizon, double* target_times,
                        double* target_states, double* base_vel);
}
