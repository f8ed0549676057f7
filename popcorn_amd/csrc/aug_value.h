// aug_value.h -- the value half of the trainer's S2 augmentation, per element: RandomBrightness then RandomGamma on a raw digital number
// (utils/transform.py; run_train.py:386-402), operation by operation as augment_raw_kernel (train_ops.hip) states it:
//   bright:  clamp(x / 10000 * beta, 0, 1) * 10000          gam:  clamp((max(x, 0) / 10000) ^ gamma, 0, 1) * 10000
// Correctly rounded division and multiplication by name, so that no contraction or reciprocal form can differ between the kernels that
// apply it: pc_region_batch (region_batch.hip) must give pc_augment_raw's bits.  With neither flag the value passes through untouched.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float pc_aug_s2_value(float v, int bright, float beta, int gam, float gamma) {
    if (bright) v = fminf(fmaxf(__fmul_rn(__fdiv_rn(v, 10000.f), beta), 0.f), 1.f) * 10000.f;
    if (gam) v = fminf(fmaxf(powf(__fdiv_rn(fmaxf(v, 0.f), 10000.f), gamma), 0.f), 1.f) * 10000.f;
    return v;
}
