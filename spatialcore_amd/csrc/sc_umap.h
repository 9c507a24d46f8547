// The layout's firing schedule (sc_umap.hip; include/spatialcore_hip.h has the definition), on the host and the device alike.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// stored entry of weight w fires in epoch e iff floor((e + 1) r) > floor(e r), r = w / w_max: one division, two products
__host__ __device__ static inline bool um_fires(double w, double w_max, uint32_t e)
{
    const double r = w / w_max;
    return floor((double)(e + 1u) * r) > floor((double)e * r);
}
