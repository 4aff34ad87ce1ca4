// FlatAdam: the whole Adam update of an optimizer in ONE launch, however many tensors it holds (include/n3dt.h,
// n3dt_flat_adam_step; the reference's two torch.optim.Adam steps, talker_trainer.py:722-727, 1063-1067).
//
// torch.optim.Adam's arithmetic, amsgrad = False, L2 weight decay folded into the gradient, fp32 per element:
//   g  = maximize ? -g : g;  g += wd * p
//   m  = b1 m + (1 - b1) g
//   v  = b2 v + (1 - b2) g g
//   p += -(lr / (1 - b1^t)) * (m / (sqrt(v) / sqrt(1 - b2^t) + eps))
// Non-finite gradients propagate; nothing is skipped.
//
// Work list: a chunk table in device memory (tensor index, start element, length), one chunk at a time per workgroup,
// grid-stride; no chunk crosses a tensor.  A tensor record holds the four pointers, the group index and an "active" flag
// (a parameter without a gradient keeps its value and its state).  A group record holds the hyper-parameters as doubles: the learning rate is
// read from device memory every launch, so a replayed graph follows a host-side copy into it.
//
// Bias corrections: the first n_groups threads of a workgroup form 1 - b^t in DOUBLE from the integer step (an fp32
// 1 - 0.999^1 keeps about 13 bits) and the two scalars torch forms on the host, lr / (1 - b1^t) and sqrt(1 - b2^t); they
// reach the other threads through LDS, rounded to fp32 once, as torch rounds them when it hands them to its kernels.
//
// Step counter: counter[0] is the number of steps taken, counter[1] counts workgroups that have finished.  Every workgroup
// reads t = counter[0] before its barrier, and adds 1 to counter[1] (a vector atomic, agent scope) after its last chunk;
// the workgroup that sees gridDim.x - 1 there is the last one, so every read of counter[0] has happened: it adds 1 to
// counter[0] and re-arms counter[1].  Both words are touched by atomics only after their initial zero fill.
//
// Memory path: 4 reads + 3 writes of 4 bytes per element, no reuse, so no LDS staging.  Within a chunk the body is
// walked with 16-byte accesses, four independent vectors per thread in flight; a scalar head runs up to the first
// 16-byte boundary of the GRADIENT pointer and a scalar tail follows the last whole vector.  exp_avg / exp_avg_sq take
// part in the vector body only when they are congruent to the gradient modulo 16 bytes (they are: three arenas of one
// layout), else the chunk is walked element by element; the PARAMETER (never re-homed: its storage offset is any multiple
// of 4 bytes) falls back on its own to four 4-byte accesses per vector when it is not congruent.
#include "n3dt_device.h"

#define ADAM_THREADS 256
#define ADAM_UNROLL 4

struct AdamScalars {
    float step_size, bc2_sqrt, b1, omb1, b2, omb2, eps, wd;
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& s, bool maximize) {
    if (maximize) g = -g;
    g = g + s.wd * p;
    m = s.b1 * m + s.omb1 * g;
    v = s.b2 * v + s.omb2 * (g * g);
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p + (-s.step_size) * (m / denom);
}

// the pointers come out of a table, so the compiler cannot see that they are global: say so (global_load / global_store
// instead of flat accesses)
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
__device__ __forceinline__ float adam_ld(const float* q) { return *(const gf32*)q; }
__device__ __forceinline__ void adam_st(float* q, float x) { *(gf32*)q = x; }

template <bool PVEC>
__device__ __forceinline__ f32x4 adam_ld4(const float* q) {
    if constexpr (PVEC) return *(const gf32x4*)q;
    f32x4 r = {adam_ld(q), adam_ld(q + 1), adam_ld(q + 2), adam_ld(q + 3)};
    return r;
}

template <bool PVEC>
__device__ __forceinline__ void adam_st4(float* q, f32x4 x) {
    if constexpr (PVEC) {
        *(gf32x4*)q = x;
    } else {
        adam_st(q, x[0]); adam_st(q + 1, x[1]); adam_st(q + 2, x[2]); adam_st(q + 3, x[3]);
    }
}

// nvec whole vectors starting at element 0 of the four (already offset) pointers; g, m, v 16-byte aligned
template <bool PVEC>
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, int nvec, const AdamScalars& s, bool maximize) {
    for (int base = 0; base < nvec; base += ADAM_THREADS * ADAM_UNROLL) {
        f32x4 P[ADAM_UNROLL], G[ADAM_UNROLL], M[ADAM_UNROLL], V[ADAM_UNROLL];
#pragma unroll
        for (int k = 0; k < ADAM_UNROLL; ++k) {
            const int i = base + k * ADAM_THREADS + (int)threadIdx.x;
            if (i < nvec) {
                P[k] = adam_ld4<PVEC>(p + 4 * (size_t)i);
                G[k] = adam_ld4<true>(g + 4 * (size_t)i);
                M[k] = adam_ld4<true>(m + 4 * (size_t)i);
                V[k] = adam_ld4<true>(v + 4 * (size_t)i);
            }
        }
#pragma unroll
        for (int k = 0; k < ADAM_UNROLL; ++k) {
            const int i = base + k * ADAM_THREADS + (int)threadIdx.x;
            if (i < nvec) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float pj = P[k][j], mj = M[k][j], vj = V[k][j];
                    adam_elem(pj, G[k][j], mj, vj, s, maximize);
                    P[k][j] = pj; M[k][j] = mj; V[k][j] = vj;
                }
                adam_st4<PVEC>(p + 4 * (size_t)i, P[k]);
                adam_st4<true>(m + 4 * (size_t)i, M[k]);
                adam_st4<true>(v + 4 * (size_t)i, V[k]);
            }
        }
    }
}

__global__ __launch_bounds__(ADAM_THREADS) void flat_adam_kernel(const N3dtAdamTensor* __restrict__ tensors,
                                                                 const N3dtAdamChunk* __restrict__ chunks, int n_chunks,
                                                                 const N3dtAdamGroup* __restrict__ groups, int n_groups,
                                                                 int* counter) {
    __shared__ AdamScalars s_sc[N3DT_ADAM_MAX_GROUPS];
    __shared__ int s_max[N3DT_ADAM_MAX_GROUPS];
    if ((int)threadIdx.x < n_groups) {
        const N3dtAdamGroup gr = groups[threadIdx.x];
        const double t = (double)(__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1);
        const double bc1 = 1.0 - pow(gr.beta1, t), bc2 = 1.0 - pow(gr.beta2, t);
        AdamScalars s;
        s.step_size = (float)(gr.lr / bc1);
        s.bc2_sqrt = (float)sqrt(bc2);
        s.b1 = (float)gr.beta1;
        s.omb1 = (float)(1.0 - gr.beta1);
        s.b2 = (float)gr.beta2;
        s.omb2 = (float)(1.0 - gr.beta2);
        s.eps = (float)gr.eps;
        s.wd = (float)gr.weight_decay;
        s_sc[threadIdx.x] = s;
        s_max[threadIdx.x] = gr.maximize;
    }
    __syncthreads();

    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const N3dtAdamChunk ck = chunks[c];
        const N3dtAdamTensor T = tensors[ck.tensor];
        if (!T.active || ck.length <= 0 || (unsigned)T.group >= (unsigned)n_groups) continue;
        const AdamScalars s = s_sc[T.group];
        const bool maximize = s_max[T.group] != 0;
        float* p = T.param + ck.start;
        const float* g = T.grad + ck.start;
        float* m = T.exp_avg + ck.start;
        float* v = T.exp_avg_sq + ck.start;
        const int n = ck.length;
        const uintptr_t ga = (uintptr_t)g;
        const bool state_vec = ((((uintptr_t)m ^ ga) | ((uintptr_t)v ^ ga)) & 15) == 0;
        if (!state_vec) {
            for (int i = threadIdx.x; i < n; i += ADAM_THREADS) {
                float pj = adam_ld(p + i), mj = adam_ld(m + i), vj = adam_ld(v + i);
                adam_elem(pj, adam_ld(g + i), mj, vj, s, maximize);
                adam_st(p + i, pj); adam_st(m + i, mj); adam_st(v + i, vj);
            }
            continue;
        }
        int head = (int)((16 - (ga & 15)) & 15) >> 2;  // elements in front of the first 16-byte boundary
        if (head > n) head = n;
        const int nvec = (n - head) >> 2, tail = (n - head) & 3;
        if ((int)threadIdx.x < head + tail) {  // at most 6 scalar elements per chunk
            const int i = (int)threadIdx.x < head ? (int)threadIdx.x : head + 4 * nvec + ((int)threadIdx.x - head);
            float pj = adam_ld(p + i), mj = adam_ld(m + i), vj = adam_ld(v + i);
            adam_elem(pj, adam_ld(g + i), mj, vj, s, maximize);
            adam_st(p + i, pj); adam_st(m + i, mj); adam_st(v + i, vj);
        }
        if (((((uintptr_t)p) ^ ga) & 15) == 0)
            adam_body<true>(p + head, g + head, m + head, v + head, nvec, s, maximize);
        else
            adam_body<false>(p + head, g + head, m + head, v + head, nvec, s, maximize);
    }

    // every read of counter[0] in this workgroup happened before the barrier above
    if (threadIdx.x == 0) {
        const int done = atomicAdd(counter + 1, 1);
        if (done == (int)gridDim.x - 1) {
            atomicAdd(counter, 1);
            atomicExch(counter + 1, 0);
        }
    }
}

extern "C" void n3dt_launch_flat_adam(const void* tensors, const void* chunks, int n_chunks, const void* groups, int n_groups,
                                      void* counter, hipStream_t stream) {
    // memory-bound: at most 4 workgroups per CU's worth of blocks, the rest of the chunks by grid stride
    const int grid = n_chunks < N3DT_ADAM_MAX_GRID ? n_chunks : N3DT_ADAM_MAX_GRID;
    hipLaunchKernelGGL(flat_adam_kernel, dim3(grid), dim3(ADAM_THREADS), 0, stream, (const N3dtAdamTensor*)tensors,
                       (const N3dtAdamChunk*)chunks, n_chunks, (const N3dtAdamGroup*)groups, n_groups, (int*)counter);
}
