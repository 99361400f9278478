// aqua_qnet.hpp -- what the translation units around the DQN's 5 -> 64 -> 64 -> 3 Q-network (main/impl/dqn.py:301-314)
// share: the Philox streams of the policy and the learner, the random action of the epsilon-greedy pick, and the geometry
// of the network on v_mfma_f32_32x32x2_f32.  The forward passes are not here: the policy's is float32 throughout, the
// learner's has its last layer in double, by design.
#pragma once
#include "aqua_device.hpp"

namespace aqua {
namespace qnet {

// ---- Philox streams (aqua_device.hpp: 0, 1, 3, 4 are the environment's)
constexpr uint32_t STREAM_POLICY = 5;    // epsilon-greedy draws of the policy kernel, and of the exploration pass that reproduces them
constexpr uint32_t STREAM_LEARNER = 6;   // minibatch draws
static_assert(STREAM_POLICY != STREAM_LEARNER && STREAM_POLICY != STREAM_STEP && STREAM_POLICY != STREAM_PLACE &&
              STREAM_POLICY != STREAM_POSE && STREAM_POLICY != STREAM_ACT && STREAM_LEARNER != STREAM_STEP &&
              STREAM_LEARNER != STREAM_PLACE && STREAM_LEARNER != STREAM_POSE && STREAM_LEARNER != STREAM_ACT,
              "the policy and minibatch draws need streams of their own");

// ---- the network
constexpr int IN = 5, HID = 64, ACT = 3;
constexpr int TILE = 32;                 // worlds (samples) per wavefront and pass: the MFMA's column count

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the unit (row of the accumulator tile) that register r of row block M holds on lane half h
__host__ __device__ constexpr int unit_of(int M, int r, int h) { return 32 * M + (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- the random action of an epsilon-greedy pick, from the words r of the world's draw; it is taken when u_01(r[0]) < epsilon
__device__ __forceinline__ uint32_t random_action(const uint32_t (&r)[4]) { return ((r[1] >> 8) * static_cast<uint32_t>(ACT)) >> 24; }

}  // namespace qnet
}  // namespace aqua
