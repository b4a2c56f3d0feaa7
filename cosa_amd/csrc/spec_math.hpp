// spec_math.hpp -- spec E: the deterministic expf of the label path, for translation units other than
// label_kernels.hip / par_kernels.hip (which keep their file-local copies).  Every operation is one IEEE binary32 operation in the
// order written; include only from files built with -ffp-contract=off.  tests/test_export_par_gpu.py holds it to the C oracle's bits.
#pragma once
#include <hip/hip_runtime.h>

namespace cosa {

__device__ __forceinline__ float spec_expf(float x)
{
    if (x < -87.0f) return 0.0f;
    if (x > 88.0f) x = 88.0f;
    float k = __builtin_rintf(x * 1.44269504088896341f);
    float r = __builtin_fmaf(k, -0.693359375f, x);
    r = __builtin_fmaf(k, 2.12194440e-4f, r);
    float p = 1.9875691500E-4f;
    p = __builtin_fmaf(p, r, 1.3981999507E-3f);
    p = __builtin_fmaf(p, r, 8.3334519073E-3f);
    p = __builtin_fmaf(p, r, 4.1665795894E-2f);
    p = __builtin_fmaf(p, r, 1.6666665459E-1f);
    p = __builtin_fmaf(p, r, 5.0000001201E-1f);
    float r2 = r * r;
    float e = __builtin_fmaf(p, r2, r);
    e = e + 1.0f;
    return __builtin_ldexpf(e, (int)k);
}

}  // namespace cosa
