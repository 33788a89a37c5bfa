// ivf_sq8_dev.hpp — device helpers shared by the IVF SQ8 kernels (ivf_sq8.hip, ivf_sq8_build.hip,
// ivf_sq8_range.hip): the tile addressing, the code-to-fp16 conversion and sq_row_dist, the one function that defines
// the bits of every distance returned.
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

typedef float sq_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 sq_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 sq_f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned sq_u32x4 __attribute__((ext_vector_type(4)));

// dwords between two queries' fp16 terms in LDS ([query][step][g][8 halves])
__host__ __device__ inline int sq_stride(int nstep) { return nstep * 16 + 8; }

// The direct form of one row against one query, by the whole wave (every lane returns the sum): lane-strided over
// the dims, then the xor butterfly.  L2: g = the list's centroid or nullptr; IP: base = q·g (0 without residual).
template <bool IP>
__device__ __forceinline__ float sq_row_dist(const float *__restrict__ q, const float *__restrict__ g, float base,
                                             const unsigned char *__restrict__ pass, int rr, int d,
                                             const float *__restrict__ vmin, const float *__restrict__ vdiff, int lane) {
    float acc = 0.f;
    // four strides' loads are issued before their arithmetic (one memory round trip instead of four); the terms are
    // still added in e order, so the sum is the one-stride loop's bit for bit
    for (int e0 = lane; e0 < d; e0 += 256) {
        float c[4], vm[4], vd[4], qv[4], gv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + 64 * u;
            const bool in = e < d;
            const int ee = in ? e : lane;  // (lane < d here, since e0 < d)
            c[u] = (float)pass[sq_tile_off(rr, ee)];
            vm[u] = vmin[ee];
            vd[u] = vdiff[ee];
            qv[u] = q[ee];
            gv[u] = (!IP && g) ? g[ee] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (e0 + 64 * u >= d) break;
            const float dec = vm[u] + (c[u] + 0.5f) / 255.0f * vd[u];
            if (IP) {
                acc = fmaf(qv[u], dec, acc);
            } else {
                const float t = g ? qv[u] - gv[u] : qv[u];
                const float df = t - dec;
                acc = fmaf(df, df, acc);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    return IP ? base + acc : acc;
}
__device__ __forceinline__ float sq_wave_dot(const float *__restrict__ a, const float *__restrict__ b, int d, int lane) {
    float acc = 0.f;
    for (int e = lane; e < d; e += 64) acc = fmaf(a[e], b[e], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    return acc;
}

// four codes of a dword as exact fp16: bytes (c, 0x64) are 1024 + c; minus 1024
__device__ __forceinline__ sq_f16x8 sq_cvt8(unsigned x, unsigned y) {
    const sq_f16x2 k = {(_Float16)1024.f, (_Float16)1024.f};
    unsigned w[4];
    w[0] = __builtin_amdgcn_perm(0x64646464u, x, 0x04010400u);
    w[1] = __builtin_amdgcn_perm(0x64646464u, x, 0x04030402u);
    w[2] = __builtin_amdgcn_perm(0x64646464u, y, 0x04010400u);
    w[3] = __builtin_amdgcn_perm(0x64646464u, y, 0x04030402u);
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = __builtin_bit_cast(unsigned, __builtin_bit_cast(sq_f16x2, w[i]) - k);
    sq_u32x4 v = {w[0], w[1], w[2], w[3]};
    return __builtin_bit_cast(sq_f16x8, v);
}

// the pass and in-pass row of a shard row of list l
__device__ __forceinline__ const unsigned char *sq_row_pass(const unsigned char *codes_t, const int64_t *tpass_off,
                                                            const int64_t *list_off, int64_t l, int64_t row, int nstep,
                                                            int &rr) {
    const int64_t rel = row - list_off[l];
    rr = (int)(rel & 31);
    return codes_t + (tpass_off[l] + (rel >> 5)) * (int64_t)nstep * 1024;
}

}  // namespace hipann
