// FlatAdam: the whole Adam update of an optimizer in ONE launch, however many tensors it holds (include/n3dt.h,
// n3dt_flat_adam_step; the reference's two torch.optim.Adam steps, talker_trainer.py:722-727, 1063-1067).
//
// torch.optim.Adam's arithmetic, amsgrad = False, L2 weight decay folded into the gradient, fp32 per element:
//   g  = maximize ? -g : g;  g += wd * p
//   m  = b1 m + (1 - b1) g
//   v  = b2 v + (1 - b2) g g
//   p += -(lr / (1 - b1^t)) * (m / (sqrt(v) / sqrt(1 - b2^t) + eps))
// Non-finite gradients propagate; nothing is skipped -- unless the step is GUARDED (below).
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
//
// The guarded step (include/n3dt_flat_adam_guard.h, n3dt_flat_adam_guarded_step): global-norm clipping and non-finite step
// skipping decided on the device, two launches, nothing for the host to do.
//   flat_grad_norm_kernel  walks the same chunk table with the same head / 16-byte body / tail split, over the GRADIENT only
//       (4 more bytes read per element).  Every thread squares and adds in double (an fp32 square is exact in double, and
//       |g| ~ 1e30 stays finite), the workgroup adds its 256 values in a fixed order and ONE double per chunk goes to
//       partials[chunk] with a plain vector store (0 for a chunk of an inactive tensor).  No floating-point atomics: the
//       last workgroup to finish -- found with the same completion-counter idiom as below, on guard->norm_done -- adds
//       partials[0..n_chunks) in INDEX order (one thread, the LDS reads running a batch ahead of the add chain), so the norm
//       depends neither on the grid nor on scheduling.  It covers exactly the chunks the step kernel updates.  It writes
//       grad_norm, clip_coef and the skip flag into the guard record and re-arms its counter.  No workgroup waits for
//       another one.
//   flat_adam_kernel<true>  reads clip_coef and the skip flag in its prologue.  On skip every workgroup goes straight to the
//       completion counter and the last one adds 1 to guard->skipped_steps instead of counter[0]: parameters, state and the
//       step count stay bit for bit as they were.  Otherwise the gradient of every element is multiplied by clip_coef (fp32)
//       before adam_elem; a coefficient of 1 leaves the arithmetic bit-identical to flat_adam_kernel<false>, which is the
//       unguarded step as it always was.
#include "n3dt_device.h"
#include "n3dt_launch.h"

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
template <bool PVEC, bool GUARDED>
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, int nvec, const AdamScalars& s, bool maximize, float clip) {
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
                    adam_elem(pj, GUARDED ? G[k][j] * clip : G[k][j], mj, vj, s, maximize);
                    P[k][j] = pj; M[k][j] = mj; V[k][j] = vj;
                }
                adam_st4<PVEC>(p + 4 * (size_t)i, P[k]);
                adam_st4<true>(m + 4 * (size_t)i, M[k]);
                adam_st4<true>(v + 4 * (size_t)i, V[k]);
            }
        }
    }
}

// one workgroup's sum of a per-thread double, added in a fixed order: xor butterflies inside a wave (every lane ends with
// the same value), then the waves in index order.  `slot`: 4 doubles of LDS the caller does not touch until its next
// barrier.  The result is valid in thread 0.
__device__ __forceinline__ double norm_block_sum(double x, double* slot) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

#define NORM_TILE 2048  // partials staged per pass of the final sum (16 KiB of LDS)
#define NORM_BATCH 16   // partials in registers ahead of the final sum's add chain

__global__ __launch_bounds__(ADAM_THREADS) void flat_grad_norm_kernel(const N3dtAdamTensor* __restrict__ tensors,
                                                                      const N3dtAdamChunk* __restrict__ chunks, int n_chunks,
                                                                      int n_groups, double* partials, N3dtAdamGuard* guard) {
    static_assert(ADAM_THREADS == 256, "norm_block_sum adds four waves");
    // two sets, toggled once per norm_block_sum (= once per barrier): a wave may be one sum ahead of the slowest reader of the
    // previous one, and the barrier of that next sum lies between any read of a set and the next write to it
    __shared__ double s_wave[2][4];
    __shared__ double s_tile[NORM_TILE];
    __shared__ int s_last;
    int set = 0;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const N3dtAdamChunk ck = chunks[c];
        const N3dtAdamTensor T = tensors[ck.tensor];
        // exactly the chunks flat_adam_kernel updates (the same for the whole workgroup; no barrier on this path)
        if (!T.active || ck.length <= 0 || (unsigned)T.group >= (unsigned)n_groups) {
            if (threadIdx.x == 0) partials[c] = 0.0;
            continue;
        }
        const float* g = T.grad + ck.start;
        const int n = ck.length;
        int head = (int)((16 - ((uintptr_t)g & 15)) & 15) >> 2;
        if (head > n) head = n;
        const int nvec = (n - head) >> 2, tail = (n - head) & 3;
        double acc = 0.0;
        if ((int)threadIdx.x < head + tail) {
            const int i = (int)threadIdx.x < head ? (int)threadIdx.x : head + 4 * nvec + ((int)threadIdx.x - head);
            const double x = (double)adam_ld(g + i);
            acc = x * x;
        }
        const float* gv = g + head;
        for (int base = 0; base < nvec; base += ADAM_THREADS * ADAM_UNROLL) {
            f32x4 G[ADAM_UNROLL];
#pragma unroll
            for (int k = 0; k < ADAM_UNROLL; ++k) {
                const int i = base + k * ADAM_THREADS + (int)threadIdx.x;
                if (i < nvec) G[k] = adam_ld4<true>(gv + 4 * (size_t)i);
            }
#pragma unroll
            for (int k = 0; k < ADAM_UNROLL; ++k) {
                const int i = base + k * ADAM_THREADS + (int)threadIdx.x;
                if (i < nvec) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double x = (double)G[k][j];
                        acc += x * x;
                    }
                }
            }
        }
        const double sum = norm_block_sum(acc, s_wave[set]);
        set ^= 1;
        if (threadIdx.x == 0) partials[c] = sum;
    }

    // thread 0 wrote this workgroup's partials: make them visible at agent scope, then count the workgroup as finished
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = atomicAdd(&guard->norm_done, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();  // every partial was stored before its workgroup's count; read them from memory, not from this CU's cache
    double total = 0.0;
    for (int base = 0; base < n_chunks; base += NORM_TILE) {
        const int m = n_chunks - base < NORM_TILE ? n_chunks - base : NORM_TILE;
        for (int i = threadIdx.x; i < m; i += ADAM_THREADS)
            s_tile[i] = __hip_atomic_load(partials + base + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (threadIdx.x == 0) {
            // index order, one dependent add after another; the LDS reads of the next NORM_BATCH values are issued ahead of
            // the adds of the current ones, so the chain waits for the adder only
            int i = 0;
            if (m >= NORM_BATCH) {
                double cur[NORM_BATCH], nxt[NORM_BATCH];
#pragma unroll
                for (int j = 0; j < NORM_BATCH; ++j) cur[j] = s_tile[j];
                for (; i + 2 * NORM_BATCH <= m; i += NORM_BATCH) {
#pragma unroll
                    for (int j = 0; j < NORM_BATCH; ++j) nxt[j] = s_tile[i + NORM_BATCH + j];
#pragma unroll
                    for (int j = 0; j < NORM_BATCH; ++j) total += cur[j];
#pragma unroll
                    for (int j = 0; j < NORM_BATCH; ++j) cur[j] = nxt[j];
                }
#pragma unroll
                for (int j = 0; j < NORM_BATCH; ++j) total += cur[j];
                i += NORM_BATCH;
            }
            for (; i < m; ++i) total += s_tile[i];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(total);  // rounded to fp32 once
        const float max_norm = guard->max_grad_norm;
        float coef = 1.0f;
        if (max_norm > 0.0f) {
            // clip_grad_norm_: max_norm / (total_norm + 1e-6) is reciprocal() * max_norm in fp32, then clamp(max = 1), NaN kept
            coef = (1.0f / (norm + 1e-6f)) * max_norm;
            coef = coef != coef ? coef : fminf(coef, 1.0f);
        }
        guard->grad_norm = norm;
        guard->clip_coef = coef;
        guard->skip = (guard->skip_nonfinite != 0 && !isfinite(norm)) ? 1 : 0;
        atomicExch(&guard->norm_done, 0);
    }
}

template <bool GUARDED>
__global__ __launch_bounds__(ADAM_THREADS) void flat_adam_kernel(const N3dtAdamTensor* __restrict__ tensors,
                                                                 const N3dtAdamChunk* __restrict__ chunks, int n_chunks,
                                                                 const N3dtAdamGroup* __restrict__ groups, int n_groups,
                                                                 int* counter, N3dtAdamGuard* guard) {
    // the guard record was written by the launch in front of this one and nothing writes it while this one runs
    const float clip = GUARDED ? guard->clip_coef : 1.0f;
    if (GUARDED && guard->skip != 0) {  // (the same for every thread of the grid) no tensor, no step count is touched
        if (threadIdx.x == 0) {
            const int done = atomicAdd(counter + 1, 1);
            if (done == (int)gridDim.x - 1) {
                atomicAdd(&guard->skipped_steps, 1);
                atomicExch(counter + 1, 0);
            }
        }
        return;
    }
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
                const float gj = adam_ld(g + i);
                adam_elem(pj, GUARDED ? gj * clip : gj, mj, vj, s, maximize);
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
            const float gj = adam_ld(g + i);
            adam_elem(pj, GUARDED ? gj * clip : gj, mj, vj, s, maximize);
            adam_st(p + i, pj); adam_st(m + i, mj); adam_st(v + i, vj);
        }
        if (((((uintptr_t)p) ^ ga) & 15) == 0)
            adam_body<true, GUARDED>(p + head, g + head, m + head, v + head, nvec, s, maximize, clip);
        else
            adam_body<false, GUARDED>(p + head, g + head, m + head, v + head, nvec, s, maximize, clip);
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
    hipLaunchKernelGGL(flat_adam_kernel<false>, dim3(grid), dim3(ADAM_THREADS), 0, stream, (const N3dtAdamTensor*)tensors,
                       (const N3dtAdamChunk*)chunks, n_chunks, (const N3dtAdamGroup*)groups, n_groups, (int*)counter,
                       (N3dtAdamGuard*)nullptr);
}

extern "C" void n3dt_launch_flat_adam_guarded(const void* tensors, const void* chunks, int n_chunks, const void* groups,
                                              int n_groups, void* counter, void* partials, void* guard, hipStream_t stream) {
    const int grid = n_chunks < N3DT_ADAM_MAX_GRID ? n_chunks : N3DT_ADAM_MAX_GRID;
    hipLaunchKernelGGL(flat_grad_norm_kernel, dim3(grid), dim3(ADAM_THREADS), 0, stream, (const N3dtAdamTensor*)tensors,
                       (const N3dtAdamChunk*)chunks, n_chunks, n_groups, (double*)partials, (N3dtAdamGuard*)guard);
    hipLaunchKernelGGL(flat_adam_kernel<true>, dim3(grid), dim3(ADAM_THREADS), 0, stream, (const N3dtAdamTensor*)tensors,
                       (const N3dtAdamChunk*)chunks, n_chunks, (const N3dtAdamGroup*)groups, n_groups, (int*)counter,
                       (N3dtAdamGuard*)guard);
}
