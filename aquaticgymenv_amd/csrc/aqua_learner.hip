// aqua_learner.hip -- libaqua_learner.so (include/aqua_learner.h): one DQN update of the 5 -> 64 -> 64 -> 3 Q-network for a
// minibatch of the device experience ring on gfx950 -- TD target (main/impl/dqn.py:262-292), gradient of the mean squared TD
// error or, with AQUALRN_LOSS_REFERENCE, of the broadcast loss that dqn.py:243-247 executes, Adam as Keras 2.3
// applies it (dqn.py:313), soft target update (dqn.py:294-299) and the re-pack into the acting network's blob -- in two
// launches.  Its own translation unit and library: libaqua_hip.so, libaqua_policy.so and their kernels are not touched.
//
// The device side -- the constants, the argument structs, the forward pass and the bodies of both kernels, the launch shape
// and the workspace layout -- is stated in aqua_lrn.hpp, once for this library and libaqua_lbank.so (DESIGN.md 5.7 and
// 5.12).  Here: the two `__global__` wrappers, aqualrn_update_f32 and its validation.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/aqua_learner.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"
#include "aqua_qnet.hpp"
#include "aqua_lrn.hpp"

namespace {

using namespace aqua::lrn;

template <int STRAT>
__global__ __launch_bounds__(BLOCK) void lrn_grad_kernel(const GradArgs a)
{
    grad_body<STRAT>(a, blockIdx.x);
}

__global__ __launch_bounds__(APPLY_BLOCK) void lrn_apply_kernel(const ApplyArgs a)
{
    apply_body(a, blockIdx.x);
}

}  // namespace

extern "C" {

int aqualrn_version(void) { return AQUALRN_ABI_VERSION; }
const char* aqualrn_last_error(void) { return g_err; }

size_t aqualrn_workspace_bytes(int64_t B)
{
    if (B < 0 || B > AQUALRN_MAX_BATCH) return 0;
    return workspace_region(B);
}

int aqualrn_update_f32(float* theta, float* theta_target, float* m, float* v, uint64_t* t_dev,
                       const float* s, const uint8_t* a, const float* r, const float* s2, const uint8_t* d,
                       const uint8_t* ok, int64_t ld, int64_t size,
                       const int32_t* idx, int64_t B, uint64_t seed,
                       int strategy, double gamma, double tau, double lr, double beta1, double beta2, double eps,
                       float* blob_online, float* blob_target, const int32_t* perm, int64_t blob_floats,
                       void* workspace, size_t workspace_bytes,
                       int32_t* idx_out, float* grad_out, float* loss, void* stream)
{
    if (theta == nullptr || theta_target == nullptr || m == nullptr || v == nullptr || t_dev == nullptr)
        return fail(AQUALRN_E_INVALID, "theta, theta_target, m, v or t is NULL");
    if (theta == theta_target || theta == m || theta == v || theta_target == m || theta_target == v || m == v)
        return fail(AQUALRN_E_INVALID, "theta, theta_target, m and v must be four different buffers");
    if (B < 0 || B > AQUALRN_MAX_BATCH) return fail(AQUALRN_E_INVALID, "B=%lld: must be in [0, %d]", (long long)B, AQUALRN_MAX_BATCH);
    if (ld < 0 || size < 0 || size > ld || ld > INT32_MAX)
        return fail(AQUALRN_E_INVALID, "bad ring sizes: size=%lld ld=%lld", (long long)size, (long long)ld);
    const int loss_ref = (strategy & AQUALRN_LOSS_REFERENCE) != 0 ? 1 : 0;
    if (strategy >= 0) strategy &= ~AQUALRN_LOSS_REFERENCE;          // what is left: the bootstrap strategy, no other bit
    if (strategy < AQUALRN_DOUBLE_REF || strategy > AQUALRN_STANDARD) return fail(AQUALRN_E_INVALID, "strategy=%d: unknown", strategy);
    if (!is_number(gamma) || !(gamma >= 0.0 && gamma <= 1.0)) return fail(AQUALRN_E_INVALID, "gamma=%g: must be in [0, 1]", gamma);
    if (!is_number(tau) || !(tau >= 0.0 && tau <= 1.0)) return fail(AQUALRN_E_INVALID, "tau=%g: must be in [0, 1]", tau);
    if (!is_number(lr) || !(lr >= 0.0)) return fail(AQUALRN_E_INVALID, "lr=%g: must be finite and >= 0", lr);
    if (!is_number(beta1) || !is_number(beta2) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return fail(AQUALRN_E_INVALID, "beta1=%g beta2=%g: must be in [0, 1)", beta1, beta2);
    if (!is_number(eps) || !(eps > 0.0)) return fail(AQUALRN_E_INVALID, "eps=%g: must be finite and > 0", eps);
    if ((blob_online != nullptr || blob_target != nullptr) && perm == nullptr)
        return fail(AQUALRN_E_INVALID, "a blob is given without the permutation table");
    if ((blob_online != nullptr || blob_target != nullptr) && blob_floats < AQUALRN_PARAMS)
        return fail(AQUALRN_E_INVALID, "blob_floats=%lld < %d", (long long)blob_floats, AQUALRN_PARAMS);
    if (blob_online != nullptr && blob_online == blob_target) return fail(AQUALRN_E_INVALID, "blob_online == blob_target");
    if (!aligned(theta, 4) || !aligned(theta_target, 4) || !aligned(m, 4) || !aligned(v, 4))
        return fail(AQUALRN_E_ALIGN, "theta / theta_target / m / v must be 4-byte aligned");
    if (!aligned(t_dev, 8)) return fail(AQUALRN_E_ALIGN, "t must be 8-byte aligned");
    if (!aligned(s, 4) || !aligned(s2, 4) || !aligned(r, 4)) return fail(AQUALRN_E_ALIGN, "s / s2 / r must be 4-byte aligned");
    if (!aligned(idx, 4) || !aligned(idx_out, 4) || !aligned(perm, 4)) return fail(AQUALRN_E_ALIGN, "idx / idx_out / perm must be 4-byte aligned");
    if (!aligned(blob_online, 4) || !aligned(blob_target, 4) || !aligned(grad_out, 4) || !aligned(loss, 4))
        return fail(AQUALRN_E_ALIGN, "blobs / grad_out / loss must be 4-byte aligned");
    if (!aligned(workspace, 16)) return fail(AQUALRN_E_ALIGN, "the workspace must be 16-byte aligned");
    if (B == 0) return 0;
    if (s == nullptr || a == nullptr || r == nullptr || s2 == nullptr || d == nullptr || ok == nullptr)
        return fail(AQUALRN_E_INVALID, "a ring buffer is NULL");
    if (workspace == nullptr) return fail(AQUALRN_E_INVALID, "workspace is NULL");
    if (workspace_bytes < aqualrn_workspace_bytes(B))
        return fail(AQUALRN_E_INVALID, "workspace too small: %zu < %zu bytes", workspace_bytes, aqualrn_workspace_bytes(B));

    const Shape sh = shape_of(B);
    GradArgs g;
    g.theta = theta; g.theta_target = theta_target; g.t_dev = t_dev;
    g.s = s; g.a = a; g.r = r; g.s2 = s2; g.d = d; g.ok = ok;
    g.ld = ld; g.size = size; g.B = B; g.idx = idx; g.seed = seed;
    g.gamma = static_cast<float>(gamma);
    g.tiles_per_wave = sh.tiles_per_wave;
    g.loss_ref = loss_ref;
    g.ws_t = static_cast<uint64_t*>(workspace);
    g.ws = reinterpret_cast<float*>(static_cast<char*>(workspace) + WS_HEADER);
    g.idx_out = idx_out;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(sh.groups)), block(BLOCK);
    switch (strategy) {
    case AQUALRN_DOUBLE_REF: hipLaunchKernelGGL((lrn_grad_kernel<AQUALRN_DOUBLE_REF>), grid, block, 0, st, g); break;
    case AQUALRN_DOUBLE: hipLaunchKernelGGL((lrn_grad_kernel<AQUALRN_DOUBLE>), grid, block, 0, st, g); break;
    case AQUALRN_FIXED: hipLaunchKernelGGL((lrn_grad_kernel<AQUALRN_FIXED>), grid, block, 0, st, g); break;
    default: hipLaunchKernelGGL((lrn_grad_kernel<AQUALRN_STANDARD>), grid, block, 0, st, g); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "lrn_grad_kernel launch");

    ApplyArgs p;
    p.theta = theta; p.theta_target = theta_target; p.m = m; p.v = v; p.t_dev = t_dev;
    p.ws_t = g.ws_t; p.ws = g.ws; p.partials = sh.groups;
    p.tau = tau; p.lr = lr; p.beta1 = beta1; p.beta2 = beta2; p.eps = eps;
    p.blob_online = blob_online; p.blob_target = blob_target; p.perm = perm; p.blob_floats = blob_floats;
    p.grad_out = grad_out; p.loss = loss;
    hipLaunchKernelGGL(lrn_apply_kernel, dim3(APPLY_GROUPS), dim3(APPLY_BLOCK), 0, st, p);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "lrn_apply_kernel launch");
    return 0;
}

}  // extern "C"
