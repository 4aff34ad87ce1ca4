/*
 * n3dt_flat_adam_guard.h -- the guarded FlatAdam step: global-norm gradient clipping and non-finite step skipping, decided
 * on the device.  Part of the C ABI of libn3dt.so; n3dt.h includes this file, nothing includes it on its own.  (It is a
 * file of its own because n3dt.h's list of n3dt_flat_adam_* entry points is pinned by tests/test_flat_adam_cpu.py; the
 * additions are pinned by tests/test_flat_adam_guard_cpu.py.  Additions only: the ABI version does not move.)
 *
 * A guarded step is two launches on the caller's stream, no host involvement, capturable in a hipGraph:
 *   1. the norm kernel walks the gradient of every ACTIVE tensor of the chunk table, stores each chunk's sum of squares as
 *      one double in partials[chunk] (0 for a chunk of an inactive tensor), and the last workgroup to finish adds
 *      partials[0..n_chunks) in index order in double and writes into the guard record
 *        grad_norm = (float)sqrt(sum)
 *        clip_coef = max_grad_norm > 0 ? clamp_max((1 / (grad_norm + 1e-6f)) * max_grad_norm, 1) : 1      (fp32, NaN kept:
 *                    torch.nn.utils.clip_grad_norm_'s arithmetic)
 *        skip      = skip_nonfinite && !isfinite(grad_norm)
 *   2. the Adam kernel of n3dt_flat_adam_step with g * clip_coef as its gradient (one fp32 multiply per element, ahead of
 *      maximize and weight decay; the gradient in memory is not rewritten).  With skip set, no tensor and no step counter is
 *      touched and skipped_steps goes up by one instead.
 * The caller zero-fills the record once and from then on writes max_grad_norm and skip_nonfinite only (the first 8 bytes);
 * max_grad_norm <= 0 means "no clipping".  partials: n_chunks doubles, contents immaterial between steps.
 */
#ifndef N3DT_FLAT_ADAM_GUARD_H
#define N3DT_FLAT_ADAM_GUARD_H

typedef struct N3dtAdamGuard {
    float max_grad_norm;    /* caller: clip threshold, +inf allowed, <= 0: no clipping */
    int32_t skip_nonfinite; /* caller: 1 = a step whose grad_norm is not finite changes nothing */
    float grad_norm;        /* library: the last guarded step's global 2-norm of the raw gradients */
    float clip_coef;        /* library: the factor that step applied */
    int32_t skip;           /* library: that step's decision */
    int32_t skipped_steps;  /* library: guarded steps skipped so far */
    int32_t norm_done;      /* library: completion counter of the norm kernel (0 between launches) */
    int32_t reserved;
} N3dtAdamGuard;

size_t n3dt_flat_adam_guard_bytes(void);
/* n3dt_flat_adam_step's arguments and checks + partials (8-byte aligned, n_chunks doubles) and the guard record */
int n3dt_flat_adam_guarded_step(const void* tensor_table, const void* chunk_table, int n_chunks, const void* group_table,
                                int n_groups, void* step_counter, void* partials, void* guard, void* stream);

#endif
