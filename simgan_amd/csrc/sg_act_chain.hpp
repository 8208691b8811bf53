// sg_act_chain.hpp -- the seam of the chained act (sg_act_chain.hip), shared with the test library (sg_test.hip: sg_test_squash).
#pragma once
#include <hip/hip_runtime.h>

// What the hybrid-sim environments put between the two policies of a step: torch.tanh on the first policy's action before it
// is concatenated behind the state (my_pybullet_envs/hopper_env_combined_policy.py:195-216,298-325,
// laikago_env_combined_policy.py:240-268,420-438).  on == 0: the action passes as it is.
__device__ __forceinline__ float sg_squash(float v, int on) { return on ? tanhf(v) : v; }
