// The Adam step: the C ABI of the kernel of dffw_optim.hip.  dffw_adam_step checks everything before the GPU is touched, computes
// the step's scalars in double as torch.optim.Adam's single-tensor path does, cuts the list into launches of at most ADAM_TENSORS_PER_LAUNCH tensors
// and enqueues them on the caller's stream: the table is the kernel's argument, so nothing is allocated, copied or waited for.
#include <cmath>

#include "dffw_optim.h"
#include "dffw_run.h"

using namespace dffw;

extern "C" {

int dffw_adam_tensors_per_launch(void) { return ADAM_TENSORS_PER_LAUNCH; }

int dffw_adam_step(int device, const dffw_adam_tensor *tensors, int n_tensors, int64_t step, double lr, double beta1, double beta2, double eps,
                   void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (!tensors || n_tensors < 1) return fail(DFFW_EINVAL, "the Adam step needs a list of at least one tensor");
    if (step < 1) return fail(DFFW_EINVAL, "step is the count after the increment and starts at 1, got %lld", (long long)step);
    if (!std::isfinite(lr) || !std::isfinite(eps) || !std::isfinite(beta1) || !std::isfinite(beta2))
        return fail(DFFW_EINVAL, "lr, eps and the betas must be finite (lr %g, eps %g, betas %g %g)", lr, eps, beta1, beta2);
    if (lr < 0) return fail(DFFW_EINVAL, "lr must not be negative, got %g", lr);
    if (eps < 0) return fail(DFFW_EINVAL, "eps must not be negative, got %g", eps);
    if (beta1 < 0 || beta1 >= 1 || beta2 < 0 || beta2 >= 1) return fail(DFFW_EINVAL, "the betas must lie in [0, 1), got %g %g", beta1, beta2);
    int64_t live = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const dffw_adam_tensor &e = tensors[i];
        if (e.numel < 0 || e.numel >= (1ll << 31)) return fail(DFFW_EINVAL, "tensor %d: numel %lld is outside 0 .. 2^31 - 1", i, (long long)e.numel);
        if (e.numel > 0 && (!e.param || !e.grad || !e.exp_avg || !e.exp_avg_sq)) return fail(DFFW_EINVAL, "tensor %d: null pointer", i);
        if (!aligned(e.param, 4) || !aligned(e.grad, 4) || !aligned(e.exp_avg, 4) || !aligned(e.exp_avg_sq, 4))
            return fail(DFFW_EINVAL, "tensor %d: param, grad, exp_avg and exp_avg_sq must be 4-byte aligned", i);
        live += e.numel > 0;
    }
    if (!live) return DFFW_OK;   // nothing to update: no launch, and the GPU is not touched

    // torch/optim/adam.py, _single_tensor_adam with a host step: Python floats, that is doubles
    const double t = (double)step;
    const double bias_correction1 = 1.0 - std::pow(beta1, t), bias_correction2 = 1.0 - std::pow(beta2, t);
    AdamTable tab;
    memset(&tab, 0, sizeof tab);
    tab.beta1 = (float)beta1;
    tab.beta2 = (float)beta2;
    tab.c1 = (float)(1.0 - beta1);
    tab.c2 = (float)(1.0 - beta2);
    tab.bc2_sqrt = (float)std::sqrt(bias_correction2);
    tab.step_size = (float)(lr / bias_correction1);
    tab.eps = (float)eps;

    HIPCHK(hipSetDevice(device));
    std::string names;
    auto flush = [&]() -> hipError_t {
        if (!tab.n_tensors) return hipSuccess;
        const hipError_t h = launch_adam(tab, (hipStream_t)hip_stream);
        names += (names.empty() ? "" : ";") + std::string(adam_kernel_name());
        tab.n_tensors = 0;
        return h;
    };
    for (int i = 0; i < n_tensors; ++i) {
        const dffw_adam_tensor &e = tensors[i];
        if (e.numel == 0) continue;
        const int64_t chunks = (e.numel + ADAM_CHUNK - 1) / ADAM_CHUNK;
        if (tab.n_tensors == ADAM_TENSORS_PER_LAUNCH || (tab.n_tensors && tab.chunk_start[tab.n_tensors] + chunks > ADAM_CHUNKS_PER_LAUNCH)) HIPCHK(flush());
        const int k = tab.n_tensors++;
        tab.param[k] = e.param;
        tab.grad[k] = e.grad;
        tab.exp_avg[k] = e.exp_avg;
        tab.exp_avg_sq[k] = e.exp_avg_sq;
        tab.numel[k] = (int)e.numel;
        if (k == 0) tab.chunk_start[0] = 0;
        tab.chunk_start[k + 1] = tab.chunk_start[k] + (int)chunks;
    }
    HIPCHK(flush());
    dffw_set_last_op_kernels(names.c_str());
    return DFFW_OK;
}

}  // extern "C"
