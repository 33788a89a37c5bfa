// ivf_sq8_dev.hpp — device helpers shared by the IVF SQ8 kernels (ivf_sq8.hip, ivf_sq8_build.hip).
#pragma once
#include "common.hpp"

namespace hipann {

// a float as an unsigned whose integer order is the float order (−NaN lowest, +NaN highest), and back
__device__ __forceinline__ unsigned sq_order_bits(float v) {
    const unsigned b = __float_as_uint(v);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sq_order_float(unsigned o) {
    return __uint_as_float((o >> 31) ? (o & 0x7fffffffu) : ~o);
}

// byte offset of (row rr of the pass, dim e) inside a pass of the tiled codes
__device__ __forceinline__ int sq_tile_off(int rr, int e) {
    return ((e >> 5) * 64 + ((e >> 3) & 3) * 16 + (rr & 15)) * 16 + (rr >> 4) * 8 + (e & 7);
}

}  // namespace hipann
