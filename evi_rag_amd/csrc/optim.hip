// Optimiser step of the retriever's training path over FLAT parameter / gradient buffers: the mirror keeps
// all 25 parameters (9.4 M floats at D = H = 1024) in one allocation, so a step is one gradient-norm pass and one fused AdamW
// pass — HBM-bound, 7 floats of traffic per parameter — instead of 25 x (clip, weight decay, two moment updates, update).
//   reference: torch.optim.AdamW built by setup_optimizer (src/utils/optimization.py:20-35; type adamw, lr 1e-3,
//   weight_decay 1e-4: configs/model/retriever_module.yaml:37-40) and Lightning's gradient_clip_val: 1.0
//   (configs/trainer/default.yaml:20 -> torch.nn.utils.clip_grad_norm_, L2 over all parameters).
#include "common.hpp"

namespace evi {

constexpr int kNormChunk = 8192;  // elements per workgroup of the norm's first stage

// stage 1: f64 sum of squares of a chunk (fixed order: a thread's strided elements, then the LDS tree)
__global__ __launch_bounds__(256) void k_sumsq_partial(const float* __restrict__ g, int64_t n, double* __restrict__ part) {
    __shared__ double red[256];
    const int64_t b = (int64_t)blockIdx.x * kNormChunk;
    const int64_t e = b + kNormChunk < n ? b + kNormChunk : n;
    double acc = 0.0;
    for (int64_t i = b + threadIdx.x; i < e; i += 256) {
        const double x = (double)g[i];
        acc += x * x;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// stage 2: the chunks in ascending order; norm_out = |scale| * sqrt(sum)
__global__ __launch_bounds__(256) void k_sumsq_final(const double* __restrict__ part, int64_t nparts, float scale, float* __restrict__ norm_out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < nparts; i += 256) acc += part[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) norm_out[0] = (float)(fabs((double)scale) * sqrt(red[0]));
}

struct AdamWArgs {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    float lr, beta1, beta2, eps, weight_decay;
    float step_size;      // lr / (1 - beta1^t)
    float inv_sqrt_bc2;   // 1 / sqrt(1 - beta2^t)
    float grad_scale;     // e.g. 1 / world_size after a SUM all-reduce
    const float* grad_norm;  // device scalar (norm of grad_scale * g) or null: no clipping
    float max_norm;
};

// torch.optim.AdamW's single-tensor update, in its order of operations (torch/optim/adamw.py -> _single_tensor_adam with
// decoupled weight decay): p *= 1 - lr wd; m = lerp(m, g, 1 - b1); v = b2 v + (1 - b2) g g; p -= step_size m / (sqrt(v) / sqrt(bc2) + eps)
__global__ __launch_bounds__(256) void k_adamw(AdamWArgs a) {
    float clip = 1.0f;
    if (a.grad_norm) {
        const float c = a.max_norm / (a.grad_norm[0] + 1e-6f);  // clip_grad_norm_: clamped to 1
        clip = c < 1.0f ? c : 1.0f;
    }
    const float gs = a.grad_scale * clip;
    const float decay = 1.0f - a.lr * a.weight_decay;
    const int64_t n4 = a.n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 p = reinterpret_cast<float4*>(a.p)[i];
        const float4 g4 = reinterpret_cast<const float4*>(a.g)[i];
        float4 m = reinterpret_cast<float4*>(a.m)[i];
        float4 v = reinterpret_cast<float4*>(a.v)[i];
        float* pp = &p.x;
        const float* gp = &g4.x;
        float* mp = &m.x;
        float* vp = &v.x;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float g = gp[c] * gs;
            pp[c] *= decay;
            mp[c] = mp[c] + (g - mp[c]) * (1.0f - a.beta1);
            vp[c] = vp[c] * a.beta2 + (1.0f - a.beta2) * g * g;
            const float denom = sqrtf(vp[c]) * a.inv_sqrt_bc2 + a.eps;
            pp[c] -= a.step_size * (mp[c] / denom);
        }
        reinterpret_cast<float4*>(a.p)[i] = p;
        reinterpret_cast<float4*>(a.m)[i] = m;
        reinterpret_cast<float4*>(a.v)[i] = v;
    }
    // tail (n not a multiple of 4)
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        const float g = a.g[i] * gs;
        float p = a.p[i] * decay;
        const float m = a.m[i] + (g - a.m[i]) * (1.0f - a.beta1);
        const float v = a.v[i] * a.beta2 + (1.0f - a.beta2) * g * g;
        p -= a.step_size * (m / (sqrtf(v) * a.inv_sqrt_bc2 + a.eps));
        a.p[i] = p;
        a.m[i] = m;
        a.v[i] = v;
    }
}

// ---- grouped, multi-rule step ---------------------------------------------------------------------------------------------
// The reference's setup_optimizer (src/utils/optimization.py:20-35) hands torch.optim any elementwise rule and per-group
// overrides (param_groups: no decay on biases / LayerNorm, another lr for the projectors).  The host lays the parameters out
// group by group, so a group is a contiguous range of the flat buffers and a step stays ONE launch: every workgroup walks the
// groups in turn, grid-striding over each range with the same 16-byte accesses as k_adamw.  The group table (ranges + the
// step's scalars, formed on the host in f64 the way torch's Python forms them) travels by value in the kernel arguments.
// Each rule keeps the order of operations of torch's single-tensor (foreach=False) implementation; the elementwise pieces
// are torch's own: lerp_ (ATen/native/Lerp.h), addcmul_ = a + value * (b * c), addcdiv_ = a + value * (b / c).
struct OptimGroupDev {
    int64_t b4, e4;  // the group's range in float4 units
    int32_t opt;     // the rule's option bits (EVI_OPTIM_OPT_*), already masked to the ones the rule has
    float c[11];     // the rule's scalars for this step (see group_scalars)
};

struct OptimArgs {
    float* p;
    const float* g;
    float* s0;
    float* s1;
    float* s2;
    float grad_scale;
    const float* grad_norm;  // device scalar (norm of grad_scale * g) or null: no clipping
    float max_norm;
    int num_groups;
    OptimGroupDev groups[EVI_OPTIM_MAX_GROUPS];
};

__device__ __forceinline__ float lerp_f(float a, float b, float w) {
    return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w);
}

// which of the three state buffers a rule with these options reads and writes
template <int Rule, int Opt>
struct OptimUses {
    static constexpr bool s0 = !(Rule == EVI_OPTIM_SGD && !(Opt & EVI_OPTIM_OPT_MOMENTUM));
    static constexpr bool s1 = (Rule == EVI_OPTIM_ADAMW || Rule == EVI_OPTIM_ADAM || Rule == EVI_OPTIM_ADAMAX || Rule == EVI_OPTIM_NADAM ||
                                Rule == EVI_OPTIM_ADADELTA) || (Rule == EVI_OPTIM_RMSPROP && (Opt & EVI_OPTIM_OPT_MOMENTUM));
    static constexpr bool s2 = ((Rule == EVI_OPTIM_ADAMW || Rule == EVI_OPTIM_ADAM) && (Opt & EVI_OPTIM_OPT_AMSGRAD)) ||
                               (Rule == EVI_OPTIM_RMSPROP && (Opt & EVI_OPTIM_OPT_CENTERED));
};

// one element.  g arrives scaled and clipped; c: the group's scalars.
template <int Rule, int Opt>
__device__ __forceinline__ void optim_update(float& p, float g, float& s0, float& s1, float& s2, const float* __restrict__ c) {
    if constexpr (Rule == EVI_OPTIM_ADAMW || Rule == EVI_OPTIM_ADAM) {
        // torch/optim/adam.py _single_tensor_adam; s0 exp_avg, s1 exp_avg_sq, s2 max_exp_avg_sq
        // c: 0 1 - lr wd, 1 wd, 2 1 - b1, 3 b2, 4 1 - b2, 5 sqrt(bc2), 6 eps, 7 -lr / bc1
        if constexpr (Rule == EVI_OPTIM_ADAMW) p *= c[0];
        else g = g + c[1] * p;
        s0 = lerp_f(s0, g, c[2]);
        s1 = s1 * c[3] + c[4] * (g * g);
        float v = s1;
        if constexpr (Opt & EVI_OPTIM_OPT_AMSGRAD) v = s2 = fmaxf(s2, s1);
        const float denom = sqrtf(v) / c[5] + c[6];
        p = p + c[7] * (s0 / denom);
    } else if constexpr (Rule == EVI_OPTIM_SGD) {
        // torch/optim/sgd.py _single_tensor_sgd; s0 momentum_buffer
        // c: 0 wd, 1 momentum (0 on the group's first step), 2 1 - dampening (1 on the first step: buf = g), 3 momentum, 4 -lr
        g = g + c[0] * p;
        if constexpr (Opt & EVI_OPTIM_OPT_MOMENTUM) {
            s0 = s0 * c[1] + c[2] * g;
            if constexpr (Opt & EVI_OPTIM_OPT_NESTEROV) g = g + c[3] * s0;
            else g = s0;
        }
        p = p + c[4] * g;
    } else if constexpr (Rule == EVI_OPTIM_RMSPROP) {
        // torch/optim/rmsprop.py _single_tensor_rmsprop; s0 square_avg, s1 momentum_buffer, s2 grad_avg
        // c: 0 wd, 1 alpha, 2 1 - alpha, 3 eps, 4 momentum, 5 -lr
        g = g + c[0] * p;
        s0 = s0 * c[1] + c[2] * (g * g);
        float avg;
        if constexpr (Opt & EVI_OPTIM_OPT_CENTERED) {
            s2 = lerp_f(s2, g, c[2]);
            avg = sqrtf(s0 + -1.0f * (s2 * s2));
        } else {
            avg = sqrtf(s0);
        }
        avg = avg + c[3];
        if constexpr (Opt & EVI_OPTIM_OPT_MOMENTUM) {
            s1 = s1 * c[4] + g / avg;
            p = p + c[5] * s1;
        } else {
            p = p + c[5] * (g / avg);
        }
    } else if constexpr (Rule == EVI_OPTIM_ADAGRAD) {
        // torch/optim/adagrad.py _single_tensor_adagrad; s0 sum.  c: 0 wd, 1 eps, 2 -lr / (1 + (t - 1) lr_decay)
        g = g + c[0] * p;
        s0 = s0 + g * g;
        p = p + c[2] * (g / (sqrtf(s0) + c[1]));
    } else if constexpr (Rule == EVI_OPTIM_ADAMAX) {
        // torch/optim/adamax.py _single_tensor_adamax; s0 exp_avg, s1 exp_inf.  c: 0 wd, 1 1 - b1, 2 b2, 3 eps, 4 -lr / bc1
        g = g + c[0] * p;
        s0 = lerp_f(s0, g, c[1]);
        s1 = fmaxf(s1 * c[2], fabsf(g) + c[3]);
        p = p + c[4] * (s0 / s1);
    } else if constexpr (Rule == EVI_OPTIM_NADAM) {
        // torch/optim/nadam.py _single_tensor_nadam; s0 exp_avg, s1 exp_avg_sq
        // c: 0 wd, 1 1 - b1, 2 b2, 3 1 - b2, 4 bc2, 5 eps, 6 -lr (1 - mu) / (1 - mu_product), 7 -lr mu_next / (1 - mu_product mu_next)
        g = g + c[0] * p;
        s0 = lerp_f(s0, g, c[1]);
        s1 = s1 * c[2] + c[3] * (g * g);
        const float denom = sqrtf(s1 / c[4]) + c[5];
        p = p + c[6] * (g / denom);
        p = p + c[7] * (s0 / denom);
    } else {
        // torch/optim/adadelta.py _single_tensor_adadelta; s0 square_avg, s1 acc_delta.  c: 0 wd, 1 rho, 2 1 - rho, 3 eps, 4 -lr
        g = g + c[0] * p;
        s0 = s0 * c[1] + c[2] * (g * g);
        const float std = sqrtf(s0 + c[3]);
        const float delta = sqrtf(s1 + c[3]) / std * g;
        s1 = s1 * c[1] + c[2] * (delta * delta);
        p = p + c[4] * delta;
    }
}

template <int Rule, int Opt>
__device__ __forceinline__ void optim_range(const OptimArgs& a, const OptimGroupDev& gr, float gs, int64_t tid, int64_t stride) {
    using U = OptimUses<Rule, Opt>;
    float c[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) c[k] = gr.c[k];
    for (int64_t i = gr.b4 + tid; i < gr.e4; i += stride) {
        float4 p = reinterpret_cast<float4*>(a.p)[i];
        const float4 g4 = reinterpret_cast<const float4*>(a.g)[i];
        float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0, x2 = x0;
        if constexpr (U::s0) x0 = reinterpret_cast<float4*>(a.s0)[i];
        if constexpr (U::s1) x1 = reinterpret_cast<float4*>(a.s1)[i];
        if constexpr (U::s2) x2 = reinterpret_cast<float4*>(a.s2)[i];
        optim_update<Rule, Opt>(p.x, g4.x * gs, x0.x, x1.x, x2.x, c);
        optim_update<Rule, Opt>(p.y, g4.y * gs, x0.y, x1.y, x2.y, c);
        optim_update<Rule, Opt>(p.z, g4.z * gs, x0.z, x1.z, x2.z, c);
        optim_update<Rule, Opt>(p.w, g4.w * gs, x0.w, x1.w, x2.w, c);
        reinterpret_cast<float4*>(a.p)[i] = p;
        if constexpr (U::s0) reinterpret_cast<float4*>(a.s0)[i] = x0;
        if constexpr (U::s1) reinterpret_cast<float4*>(a.s1)[i] = x1;
        if constexpr (U::s2) reinterpret_cast<float4*>(a.s2)[i] = x2;
    }
}

// the option bits a rule has (others are ignored): they pick the instantiation per GROUP, outside the element loop
template <int Rule>
constexpr int optim_opt_mask() {
    return (Rule == EVI_OPTIM_ADAMW || Rule == EVI_OPTIM_ADAM) ? EVI_OPTIM_OPT_AMSGRAD
           : Rule == EVI_OPTIM_SGD                             ? (EVI_OPTIM_OPT_MOMENTUM | EVI_OPTIM_OPT_NESTEROV)
           : Rule == EVI_OPTIM_RMSPROP                         ? (EVI_OPTIM_OPT_MOMENTUM | EVI_OPTIM_OPT_CENTERED)
                                                               : 0;
}

template <int Rule>
__global__ __launch_bounds__(256) void k_optim(OptimArgs a) {
    float clip = 1.0f;
    if (a.grad_norm) {
        const float c = a.max_norm / (a.grad_norm[0] + 1e-6f);  // clip_grad_norm_: clamped to 1
        clip = c < 1.0f ? c : 1.0f;
    }
    const float gs = a.grad_scale * clip;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    constexpr int mask = optim_opt_mask<Rule>();
    for (int gi = 0; gi < a.num_groups; ++gi) {
        const OptimGroupDev& gr = a.groups[gi];
        const int opt = gr.opt;  // uniform over the grid: a scalar branch per group
        if (opt == 0) optim_range<Rule, 0>(a, gr, gs, tid, stride);
        if constexpr ((mask & 1) != 0) {
            if (opt == 1) optim_range<Rule, 1>(a, gr, gs, tid, stride);
        }
        if constexpr ((mask & 2) != 0) {
            if constexpr (Rule != EVI_OPTIM_SGD) {  // sgd: nesterov needs a momentum (the host refuses it without)
                if (opt == 2) optim_range<Rule, 2>(a, gr, gs, tid, stride);
            }
            if (opt == 3) optim_range<Rule, 3>(a, gr, gs, tid, stride);
        }
    }
}

// The step's scalars of one group, in f64 the way torch's Python forms them, rounded to f32 once.  Returns false (with the
// error text set) on an invalid hyper-parameter.  nadam: updates gr.mu_product (held as torch holds it, an f32 value).
static bool group_scalars(int rule, EviOptimGroup& gr, OptimGroupDev& d, const char** why) {
    const double lr = gr.lr, wd = gr.weight_decay, b1 = gr.beta1, b2 = gr.beta2, eps = gr.eps;
    const double t = (double)gr.step;
    *why = "invalid hyper-parameter";
    if (!(lr >= 0.0) || !(wd >= 0.0) || !(eps >= 0.0)) return false;
    for (int k = 0; k < 11; ++k) d.c[k] = 0.f;
    d.opt = 0;
    switch (rule) {
    case EVI_OPTIM_ADAMW:
    case EVI_OPTIM_ADAM: {
        if (!(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0)) return false;
        const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
        d.opt = gr.flags & EVI_OPTIM_OPT_AMSGRAD;
        d.c[0] = (float)(1.0 - lr * wd), d.c[1] = (float)wd, d.c[2] = (float)(1.0 - b1), d.c[3] = (float)b2, d.c[4] = (float)(1.0 - b2);
        d.c[5] = (float)pow(bc2, 0.5), d.c[6] = (float)eps, d.c[7] = (float)(-(lr / bc1));
        return true;
    }
    case EVI_OPTIM_SGD: {
        const double mom = gr.momentum, damp = gr.dampening;
        if (!(mom >= 0.0)) return false;
        const bool nesterov = (gr.flags & EVI_OPTIM_OPT_NESTEROV) != 0;
        if (nesterov && (mom <= 0.0 || damp != 0.0)) {
            *why = "Nesterov momentum requires a momentum and zero dampening";
            return false;
        }
        d.opt = (mom != 0.0 ? EVI_OPTIM_OPT_MOMENTUM : 0) | (nesterov ? EVI_OPTIM_OPT_NESTEROV : 0);
        const bool first = gr.step == 1;  // torch: the momentum buffer starts as a copy of the gradient
        d.c[0] = (float)wd, d.c[1] = first ? 0.f : (float)mom, d.c[2] = first ? 1.f : (float)(1.0 - damp), d.c[3] = (float)mom, d.c[4] = (float)(-lr);
        return true;
    }
    case EVI_OPTIM_RMSPROP: {
        const double alpha = gr.alpha, mom = gr.momentum;
        if (!(alpha >= 0.0) || !(mom >= 0.0)) return false;
        d.opt = (mom > 0.0 ? EVI_OPTIM_OPT_MOMENTUM : 0) | (gr.flags & EVI_OPTIM_OPT_CENTERED);
        d.c[0] = (float)wd, d.c[1] = (float)alpha, d.c[2] = (float)(1.0 - alpha), d.c[3] = (float)eps, d.c[4] = (float)mom, d.c[5] = (float)(-lr);
        return true;
    }
    case EVI_OPTIM_ADAGRAD: {
        if (!(gr.lr_decay >= 0.0)) return false;
        const double clr = lr / (1.0 + (t - 1.0) * gr.lr_decay);
        d.c[0] = (float)wd, d.c[1] = (float)eps, d.c[2] = (float)(-clr);
        return true;
    }
    case EVI_OPTIM_ADAMAX: {
        if (!(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0)) return false;
        const double clr = lr / (1.0 - pow(b1, t));
        d.c[0] = (float)wd, d.c[1] = (float)(1.0 - b1), d.c[2] = (float)b2, d.c[3] = (float)eps, d.c[4] = (float)(-clr);
        return true;
    }
    case EVI_OPTIM_NADAM: {
        if (!(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0) || !(gr.momentum_decay >= 0.0)) return false;
        const double bc2 = 1.0 - pow(b2, t);
        const double mu = b1 * (1.0 - 0.5 * pow(0.96, t * gr.momentum_decay));
        const double mu_next = b1 * (1.0 - 0.5 * pow(0.96, (t + 1.0) * gr.momentum_decay));
        const float mp = (float)gr.mu_product * (float)mu;  // torch keeps mu_product in an f32 tensor: `mu_product *= mu`
        gr.mu_product = (double)mp;
        const double mp_next = (double)mp * mu_next;
        d.c[0] = (float)wd, d.c[1] = (float)(1.0 - b1), d.c[2] = (float)b2, d.c[3] = (float)(1.0 - b2), d.c[4] = (float)bc2, d.c[5] = (float)eps;
        d.c[6] = (float)(-lr * (1.0 - mu) / (1.0 - (double)mp)), d.c[7] = (float)((-lr * mu_next) / (1.0 - mp_next));
        return true;
    }
    case EVI_OPTIM_ADADELTA: {
        const double rho = gr.alpha;
        if (!(rho >= 0.0 && rho <= 1.0)) return false;
        d.c[0] = (float)wd, d.c[1] = (float)rho, d.c[2] = (float)(1.0 - rho), d.c[3] = (float)eps, d.c[4] = (float)(-lr);
        return true;
    }
    }
    *why = "unknown rule";
    return false;
}

template <int Rule>
static void launch_optim(const OptimArgs& a, unsigned blocks, hipStream_t st) {
    hipLaunchKernelGGL(k_optim<Rule>, dim3(blocks), dim3(256), 0, st, a);
}

}  // namespace evi

using namespace evi;

extern "C" size_t evi_grad_norm_workspace_bytes(int64_t n) {
    if (n < 0) return 0;
    return (size_t)((n + kNormChunk - 1) / kNormChunk + 1) * sizeof(double);
}

extern "C" int evi_grad_norm(const float* g, int64_t n, float scale, float* norm_out, void* workspace, size_t workspace_bytes,
                             void* stream) {
    EVI_REQUIRE(n >= 0 && norm_out, "evi_grad_norm: bad arguments");
    EVI_REQUIRE(n == 0 || g, "evi_grad_norm: null gradient");
    EVI_REQUIRE(workspace && workspace_bytes >= evi_grad_norm_workspace_bytes(n), "evi_grad_norm: workspace too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t nparts = (n + kNormChunk - 1) / kNormChunk;
    double* part = static_cast<double*>(workspace);
    if (nparts > 0) hipLaunchKernelGGL(k_sumsq_partial, dim3((unsigned)nparts), dim3(256), 0, st, g, n, part);
    hipLaunchKernelGGL(k_sumsq_final, dim3(1), dim3(256), 0, st, part, nparts, scale, norm_out);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

extern "C" int evi_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                              float weight_decay, int64_t step, float grad_scale, const float* grad_norm, float max_norm,
                              void* stream) {
    EVI_REQUIRE(n >= 0 && step >= 1, "evi_adamw_step: n must be >= 0 and step >= 1 (got %lld, %lld)", (long long)n, (long long)step);
    if (n == 0) return EVI_OK;
    EVI_REQUIRE(p && g && m && v, "evi_adamw_step: null buffer");
    EVI_REQUIRE(lr >= 0.f && eps >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && weight_decay >= 0.f,
                "evi_adamw_step: invalid hyper-parameter");
    EVI_REQUIRE((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) % 16 == 0,
                "evi_adamw_step: buffers must be 16-byte aligned");
    AdamWArgs a;
    a.p = p, a.g = g, a.m = m, a.v = v, a.n = n;
    a.lr = lr, a.beta1 = beta1, a.beta2 = beta2, a.eps = eps, a.weight_decay = weight_decay;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    a.step_size = (float)((double)lr / bc1);
    a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    a.grad_scale = grad_scale;
    a.grad_norm = grad_norm;
    a.max_norm = max_norm;
    int64_t blocks = ((n >> 2) + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_adamw, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

extern "C" int evi_optim_step(int rule, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n, EviOptimGroup* groups,
                              int num_groups, float grad_scale, const float* grad_norm, float max_norm, void* stream) {
    EVI_REQUIRE(n >= 0 && num_groups >= 0 && (num_groups == 0 || groups), "evi_optim_step: bad arguments");
    EVI_REQUIRE(rule >= EVI_OPTIM_ADAMW && rule <= EVI_OPTIM_ADADELTA, "evi_optim_step: unknown rule %d", rule);
    if (num_groups > EVI_OPTIM_MAX_GROUPS)
        return fail(EVI_ERR_UNSUPPORTED, "evi_optim_step: %d parameter groups (at most %d travel in the kernel arguments)", num_groups,
                    EVI_OPTIM_MAX_GROUPS);
    // validate everything before any group's host state (nadam's mu_product) is advanced
    int64_t total4 = 0;
    bool use0 = false, use1 = false, use2 = false;
    for (int i = 0; i < num_groups; ++i) {
        const EviOptimGroup& gr = groups[i];
        EVI_REQUIRE(gr.begin >= 0 && gr.begin <= gr.end && gr.end <= n && gr.begin % 4 == 0 && gr.end % 4 == 0,
                    "evi_optim_step: group %d range [%lld, %lld) must lie in [0, %lld] on 16-byte boundaries", i, (long long)gr.begin,
                    (long long)gr.end, (long long)n);
        EVI_REQUIRE(gr.step >= 1, "evi_optim_step: group %d step must be >= 1 (got %lld)", i, (long long)gr.step);
        EviOptimGroup probe = gr;
        OptimGroupDev d;
        const char* why = "";
        EVI_REQUIRE(group_scalars(rule, probe, d, &why), "evi_optim_step: group %d: %s", i, why);
        if (gr.end == gr.begin) continue;
        total4 += (gr.end - gr.begin) >> 2;
        const int o = d.opt;
        use0 |= !(rule == EVI_OPTIM_SGD && !(o & EVI_OPTIM_OPT_MOMENTUM));
        use1 |= rule == EVI_OPTIM_ADAMW || rule == EVI_OPTIM_ADAM || rule == EVI_OPTIM_ADAMAX || rule == EVI_OPTIM_NADAM ||
                rule == EVI_OPTIM_ADADELTA || (rule == EVI_OPTIM_RMSPROP && (o & EVI_OPTIM_OPT_MOMENTUM));
        use2 |= ((rule == EVI_OPTIM_ADAMW || rule == EVI_OPTIM_ADAM) && (o & EVI_OPTIM_OPT_AMSGRAD)) ||
                (rule == EVI_OPTIM_RMSPROP && (o & EVI_OPTIM_OPT_CENTERED));
    }
    if (total4 > 0) {
        EVI_REQUIRE(p && g && (!use0 || s0) && (!use1 || s1) && (!use2 || s2), "evi_optim_step: null buffer");
        EVI_REQUIRE((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(s0) |
                     reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2)) % 16 == 0,
                    "evi_optim_step: buffers must be 16-byte aligned");
    }
    OptimArgs a;
    a.p = p, a.g = g, a.s0 = s0, a.s1 = s1, a.s2 = s2;
    a.grad_scale = grad_scale, a.grad_norm = grad_norm, a.max_norm = max_norm;
    a.num_groups = 0;
    for (int i = 0; i < num_groups; ++i) {
        OptimGroupDev d;
        const char* why = "";
        group_scalars(rule, groups[i], d, &why);  // advances the group's host state even when its range is empty
        if (groups[i].end == groups[i].begin) continue;
        d.b4 = groups[i].begin >> 2, d.e4 = groups[i].end >> 2;
        a.groups[a.num_groups++] = d;
    }
    if (total4 == 0) return EVI_OK;
    // largest range first (the order of the table is free): every group costs the workgroups that touch it one more memory
    // round trip, and behind the large range that latency hides under the workgroups still streaming it
    for (int i = 1; i < a.num_groups; ++i) {
        const OptimGroupDev d = a.groups[i];
        int j = i;
        for (; j > 0 && a.groups[j - 1].e4 - a.groups[j - 1].b4 < d.e4 - d.b4; --j) a.groups[j] = a.groups[j - 1];
        a.groups[j] = d;
    }
    // k_adamw's launch cap: 2048 workgroups of 256 (8 per CU) saturate HBM; larger ranges wrap in the grid-stride loops
    int64_t blocks = (total4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (rule) {
    case EVI_OPTIM_ADAMW: launch_optim<EVI_OPTIM_ADAMW>(a, (unsigned)blocks, st); break;
    case EVI_OPTIM_ADAM: launch_optim<EVI_OPTIM_ADAM>(a, (unsigned)blocks, st); break;
    case EVI_OPTIM_SGD: launch_optim<EVI_OPTIM_SGD>(a, (unsigned)blocks, st); break;
    case EVI_OPTIM_RMSPROP: launch_optim<EVI_OPTIM_RMSPROP>(a, (unsigned)blocks, st); break;
    case EVI_OPTIM_ADAGRAD: launch_optim<EVI_OPTIM_ADAGRAD>(a, (unsigned)blocks, st); break;
    case EVI_OPTIM_ADAMAX: launch_optim<EVI_OPTIM_ADAMAX>(a, (unsigned)blocks, st); break;
    case EVI_OPTIM_NADAM: launch_optim<EVI_OPTIM_NADAM>(a, (unsigned)blocks, st); break;
    default: launch_optim<EVI_OPTIM_ADADELTA>(a, (unsigned)blocks, st); break;
    }
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}
