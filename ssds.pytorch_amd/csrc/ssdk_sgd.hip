// ssdk_sgd.hip -- the optimizer update of the training step: SGD (momentum, weight decay, Nesterov), Adam / AMSGrad and
// RMSprop, every parameter tensor of the model in a handful of launches, with the NaN/Inf skip decided on the DEVICE.
//
// Reference: optimizer.step() of the reference's loop (pipeline_anchor_apex.py:128-130) on the torch.optim object built by
// core/optimizer.py:73-134 (sgd: momentum 0.9, weight decay 1e-4; adam / amsgrad: betas (MOMENTUM, MOMENTUM_2); rmsprop:
// alpha MOMENTUM_2, momentum MOMENTUM), skipped when the loss is not finite (:110-111, 126-127: a host-side `continue` after
// .item() reads).  Rounds 4-5 used torch's fused multi-tensor SGD with its `found_inf` hook.  The update rules, per element, in
// the operation order of torch's own single-tensor / foreach implementations (libssdk is built with -ffp-contract=off):
//
//   SGD      g = grad + wd p;  buf = momentum buf + g;  p -= lr (nesterov ? g + momentum buf : buf)
//            (buffers are created as zeros: the first step then is buf = g, torch's rule)
//   Adam     g = grad + wd p;  m = lerp(m, g, 1 - beta1);  v = beta2 v + (1 - beta2) g g;  AMSGrad: vmax = max(vmax, v)
//            p += -(lr / bc1) (m / (sqrt(v | vmax) / sqrt(bc2) + eps)),  bc_k = 1 - beta_k^s in fp64, s = step + 1
//   RMSprop  g = grad + wd p;  sq = alpha sq + (1 - alpha) g g;  avg = sqrt(sq) + eps   (torch's non-centered rule)
//            momentum: buf = momentum buf + g / avg;  p += -lr buf        otherwise: p += -lr (g / avg)
//
// A launch carries up to 40 tensors as kernel arguments (L pointer lists + element counts + their first 4096-element block); a
// block finds its tensor by a linear walk over <= 40 prefix sums held in SGPRs, and updates 4096 consecutive elements with
// 16-byte accesses when every pointer of the tensor is 16-byte aligned, 4-byte ones otherwise (an HBM stream: SGD 20 bytes per
// element, Adam and RMSprop with momentum 28, AMSGrad 36).  `lr` may live on the device (a float the caller updates in place: a
// captured hipGraph keeps a LIVE learning rate), `found_inf` != 0 makes every block return before it touches anything.
//
// Adam and RMSprop keep torch's per-tensor step counter (state["step"], an fp32 device scalar).  Adam's blocks READ their
// tensor's counter; one small launch after all update launches of a call advances every counter (unless found_inf is set), so
// no block ever sees a counter another block of its tensor has already advanced.
#include "ssdk_common.h"

#include <math.h>

namespace ssdk {

constexpr int kOptTensors = 40;
constexpr unsigned kOptChunk = 4096;  // elements per block
constexpr int kStepTensors = 256;     // counters per step_count_kernel launch

// One launch: up to kOptTensors tensors, L float lists each (0 = params, 1 = grads: read only, 2.. = optimizer state).
template <class Rule, int L>
struct MultiTensorArgs {
  float* t[L][kOptTensors];
  const float* step[kOptTensors];   // per-tensor step counters (Adam; NULL for the rules that do not read them)
  unsigned n[kOptTensors];
  unsigned start[kOptTensors + 1];  // first block of tensor i
  int count;
  const float* lr_dev;
  float lr;
  const float* found_inf;
  Rule rule;
};

struct SgdRule {  // L = 3 (p, grad, momentum buffer) or 2 (momentum 0)
  float momentum, weight_decay;
  int nesterov;
  struct Op {
    float lr, mom, wd;
    int nesterov;
    template <int L>
    __device__ __forceinline__ void operator()(float (&x)[L]) const {
      const float gg = x[1] + wd * x[0];
      float d = gg;
      if constexpr (L == 3) {
        x[2] = mom * x[2] + gg;
        d = nesterov ? gg + mom * x[2] : x[2];
      }
      x[0] = x[0] - lr * d;
    }
  };
  __device__ Op at(const float*, float lr) const { return Op{lr, momentum, weight_decay, nesterov}; }
};

struct AdamRule {  // L = 4 (p, grad, exp_avg, exp_avg_sq) or 5 (+ max_exp_avg_sq: AMSGrad)
  double beta1, beta2;
  float w1;                                // (float)(1 - beta1): lerp weight
  float beta2f, omb2, eps, weight_decay;  // (float)beta2, (float)(1 - beta2)
  struct Op {
    float w1, beta2, omb2, eps, wd, neg_step_size, bc2_sqrt;
    template <int L>
    __device__ __forceinline__ void operator()(float (&x)[L]) const {
      const float g = wd != 0.f ? x[1] + wd * x[0] : x[1];
      // torch's lerp: self + w (end - self) for |w| < 0.5, end - (end - self) (1 - w) otherwise
      x[2] = w1 < 0.5f ? x[2] + w1 * (g - x[2]) : g - (g - x[2]) * (1.f - w1);
      x[3] = x[3] * beta2 + omb2 * (g * g);  // torch's foreach addcmul: self + value * (t1 * t2)
      float v = x[3];
      if constexpr (L == 5) {
        if (v > x[4] || v != v) x[4] = v;  // torch.maximum (NaN propagates)
        v = x[4];
      }
      const float denom = sqrtf(v) / bc2_sqrt + eps;
      x[0] = x[0] + neg_step_size * (x[2] / denom);
    }
  };
  // bias corrections in fp64 from s = step + 1, like torch's default path on the host (step_t += 1; 1 - beta ** step.item())
  __device__ Op at(const float* step, float lr) const {
    const double s = (double)(*step + 1.f);
    const double bc1 = 1.0 - pow(beta1, s), bc2 = 1.0 - pow(beta2, s);
    return Op{w1, beta2f, omb2, eps, weight_decay, -(float)((double)lr / bc1), (float)sqrt(bc2)};
  }
};

struct RmspropRule {  // L = 3 (p, grad, square_avg) or 4 (+ momentum buffer)
  float alpha, oma, eps, weight_decay, momentum;  // (float)alpha, (float)(1 - alpha)
  struct Op {
    float alpha, oma, eps, wd, mom, neg_lr;
    template <int L>
    __device__ __forceinline__ void operator()(float (&x)[L]) const {
      const float g = wd != 0.f ? x[1] + wd * x[0] : x[1];
      x[2] = x[2] * alpha + oma * (g * g);
      const float avg = sqrtf(x[2]) + eps;
      if constexpr (L == 4) {
        x[3] = x[3] * mom + g / avg;
        x[0] = x[0] + neg_lr * x[3];
      } else {
        x[0] = x[0] + neg_lr * (g / avg);
      }
    }
  };
  __device__ Op at(const float*, float lr) const { return Op{alpha, oma, eps, weight_decay, momentum, -lr}; }
};

static_assert(sizeof(MultiTensorArgs<SgdRule, 3>) <= 4096, "kernel arguments are limited to 4 KB");
static_assert(sizeof(MultiTensorArgs<AdamRule, 5>) <= 4096, "kernel arguments are limited to 4 KB");
static_assert(sizeof(MultiTensorArgs<RmspropRule, 4>) <= 4096, "kernel arguments are limited to 4 KB");

typedef float opt_f4 __attribute__((ext_vector_type(4)));

template <class Rule, int L>
__global__ __launch_bounds__(256) void multi_tensor_kernel(const MultiTensorArgs<Rule, L> a) {
  if (a.found_inf && *a.found_inf != 0.f) return;  // the collective skip flag (pipeline_anchor_ddp.train_step)
  int t = 0;
  for (int i = 1; i < a.count; ++i)
    if (blockIdx.x >= a.start[i]) t = i;
  const unsigned base = (blockIdx.x - a.start[t]) * kOptChunk, n = a.n[t];
  float* ptr[L];
  uintptr_t bits = 0;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    ptr[k] = a.t[k][t];
    bits |= (uintptr_t)ptr[k];
  }
  const typename Rule::Op op = a.rule.at(a.step[t], a.lr_dev ? *a.lr_dev : a.lr);
  const bool vec = (bits & 15) == 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned i0 = base + ((unsigned)r * 256u + threadIdx.x) * 4u;
    if (i0 >= n) continue;
    if (vec && i0 + 3u < n) {
      opt_f4 v[L];
#pragma unroll
      for (int k = 0; k < L; ++k) v[k] = *reinterpret_cast<const opt_f4*>(ptr[k] + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x[L];
#pragma unroll
        for (int k = 0; k < L; ++k) x[k] = v[k][e];
        op(x);
#pragma unroll
        for (int k = 0; k < L; ++k) v[k][e] = x[k];
      }
#pragma unroll
      for (int k = 0; k < L; ++k)
        if (k != 1) *reinterpret_cast<opt_f4*>(ptr[k] + i0) = v[k];
    } else {
      for (unsigned i = i0; i < n && i < i0 + 4u; ++i) {
        float x[L];
#pragma unroll
        for (int k = 0; k < L; ++k) x[k] = ptr[k][i];
        op(x);
#pragma unroll
        for (int k = 0; k < L; ++k)
          if (k != 1) ptr[k][i] = x[k];
      }
    }
  }
}

struct StepArgs {
  float* step[kStepTensors];
  int count;
  const float* found_inf;
};
static_assert(sizeof(StepArgs) <= 4096, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(256) void step_count_kernel(const StepArgs a) {
  if (a.found_inf && *a.found_inf != 0.f) return;
  if ((int)threadIdx.x < a.count) *a.step[threadIdx.x] += 1.f;
}

// Validates everything first (a bad argument launches nothing), then packs the tensors into launches of <= kOptTensors.
// lists[k] (k < L) are the caller's host arrays of n device pointers; `steps` (may be NULL: SGD) are advanced by one launch per
// kStepTensors counters after all update launches; `read_steps`: the rule reads its tensor's counter (Adam).
template <class Rule, int L>
static int multi_tensor_step(const char* what, int n, void* const* const (&lists)[L], void* const* steps, bool read_steps,
                             const int64_t* numel, const float* lr_dev, float lr, const Rule& rule, const float* found_inf,
                             void* stream) {
  bool bad = n < 0 || (n > 0 && !numel);
  for (int k = 0; k < L; ++k) bad = bad || (n > 0 && !lists[k]);
  if (bad) {
    set_error("%s: bad argument (n < 0 or a NULL array)", what);
    return SSDK_E_BADARG;
  }
  for (int i = 0; i < n; ++i) {
    if (steps && !steps[i]) {
      set_error("%s: tensor %d: null step counter", what, i);
      return SSDK_E_BADARG;
    }
    if (numel[i] <= 0) continue;
    bool null = false;
    for (int k = 0; k < L; ++k) null = null || !lists[k][i];
    if (null || numel[i] >= ((int64_t)1 << 32)) {
      set_error("%s: tensor %d: null pointer or too large", what, i);
      return SSDK_E_BADARG;
    }
  }
  int i = 0;
  while (i < n) {
    MultiTensorArgs<Rule, L> a;
    a.count = 0;
    a.lr_dev = lr_dev;
    a.lr = lr;
    a.found_inf = found_inf;
    a.rule = rule;
    unsigned blocks = 0;
    for (; i < n && a.count < kOptTensors; ++i) {
      if (numel[i] <= 0) continue;
      for (int k = 0; k < L; ++k) a.t[k][a.count] = (float*)lists[k][i];
      a.step[a.count] = read_steps ? (const float*)steps[i] : nullptr;
      a.n[a.count] = (unsigned)numel[i];
      a.start[a.count] = blocks;
      blocks += ((unsigned)numel[i] + kOptChunk - 1) / kOptChunk;
      ++a.count;
    }
    if (a.count == 0) break;
    a.start[a.count] = blocks;
    hipLaunchKernelGGL((multi_tensor_kernel<Rule, L>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    int rc = check_launch(what);
    if (rc) return rc;
  }
  for (int j = 0; steps && j < n; j += kStepTensors) {  // after every update launch: no block reads an advanced counter
    StepArgs s;
    s.count = n - j < kStepTensors ? n - j : kStepTensors;
    for (int k = 0; k < s.count; ++k) s.step[k] = (float*)steps[j + k];
    s.found_inf = found_inf;
    hipLaunchKernelGGL(step_count_kernel, dim3(1), dim3(kStepTensors), 0, (hipStream_t)stream, s);
    int rc = check_launch("step_count_kernel");
    if (rc) return rc;
  }
  return SSDK_OK;
}

}  // namespace ssdk

using namespace ssdk;

extern "C" int ssdk_sgd_step(int n, void* const* params, const void* const* grads, void* const* momentum_bufs, const int64_t* numel,
                             const float* lr_dev, float lr, float momentum, float weight_decay, int nesterov, const float* found_inf,
                             void* stream) {
  const SgdRule rule{momentum, weight_decay, nesterov};
  if (momentum == 0.f) {
    void* const* const lists[2] = {params, (void* const*)grads};
    return multi_tensor_step("ssdk_sgd_step", n, lists, nullptr, false, numel, lr_dev, lr, rule, found_inf, stream);
  }
  void* const* const lists[3] = {params, (void* const*)grads, momentum_bufs};
  return multi_tensor_step("ssdk_sgd_step", n, lists, nullptr, false, numel, lr_dev, lr, rule, found_inf, stream);
}

extern "C" int ssdk_adam_step(int n, void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                              void* const* max_exp_avg_sq, void* const* steps, const int64_t* numel, const float* lr_dev, float lr,
                              double beta1, double beta2, float eps, float weight_decay, int amsgrad, const float* found_inf,
                              void* stream) {
  if (n > 0 && !steps) {
    set_error("ssdk_adam_step: bad argument (NULL steps)");
    return SSDK_E_BADARG;
  }
  const AdamRule rule{beta1, beta2, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps, weight_decay};
  if (amsgrad) {
    void* const* const lists[5] = {params, (void* const*)grads, exp_avg, exp_avg_sq, max_exp_avg_sq};
    return multi_tensor_step("ssdk_adam_step", n, lists, steps, true, numel, lr_dev, lr, rule, found_inf, stream);
  }
  void* const* const lists[4] = {params, (void* const*)grads, exp_avg, exp_avg_sq};
  return multi_tensor_step("ssdk_adam_step", n, lists, steps, true, numel, lr_dev, lr, rule, found_inf, stream);
}

extern "C" int ssdk_rmsprop_step(int n, void* const* params, const void* const* grads, void* const* square_avg,
                                 void* const* momentum_bufs, void* const* steps, const int64_t* numel, const float* lr_dev, float lr,
                                 double alpha, float eps, float weight_decay, float momentum, const float* found_inf, void* stream) {
  if (n > 0 && !steps) {
    set_error("ssdk_rmsprop_step: bad argument (NULL steps)");
    return SSDK_E_BADARG;
  }
  const RmspropRule rule{(float)alpha, (float)(1.0 - alpha), eps, weight_decay, momentum};
  if (momentum != 0.f) {
    void* const* const lists[4] = {params, (void* const*)grads, square_avg, momentum_bufs};
    return multi_tensor_step("ssdk_rmsprop_step", n, lists, steps, false, numel, lr_dev, lr, rule, found_inf, stream);
  }
  void* const* const lists[3] = {params, (void* const*)grads, square_avg};
  return multi_tensor_step("ssdk_rmsprop_step", n, lists, steps, false, numel, lr_dev, lr, rule, found_inf, stream);
}
