// TEST INFRASTRUCTURE: the entries of tests/perceive/perceive_emu.cpp, for that file and for tests/perceive/perceive_sanitize.cpp.
#pragma once
#include <cstdint>

#include "../../include/hsqp_perceive.h"

// The resident terrain of a call: what hsqp_terrain_set_maps and hsqp_terrain_set_instances take, and hsqp_contact.h's ground height of every instance
struct pc_terrain {
  int32_t n_maps, reserved;
  const int32_t* nx; const int32_t* ny; const double* cell;   // [n_maps]
  const double* heights;                     // the maps concatenated
  const hsqp_terrain_placement* place;       // [B]
  const double* ground_height;               // [B]
};

extern "C" {
void* pc_create(const hsqp_model_desc* md, const double* default_joint_state, char* err, int errlen);
void pc_destroy(void* h);
int pc_node_params(const hsqp_swing_config* cfg, double terrain, int arm_swing, int E, int n_ev, const double* ev, const int* seq, int n_knots, const double* tt,
                   const double* ts, int n_t, const double* times, const double* lift, const double* touch, double* par);
void pc_foot_heights(void* h, const pc_terrain* t, int B, int E, int K, double time, double offset, const double* x, const int* ne, const double* ev, const int* seq,
                     const double* tt, const double* ts, double* lift, double* touch, double* fxy);
void pc_terrain_eval(const pc_terrain* t, int B, int n_pts, const double* xy, double* height);
}

