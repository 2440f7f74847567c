// convnet.h -- what the metric networks' kernel files share (convnet.hip, lpips.hip, i3d.hip, inception.hip): the launch shape of their
// grid-stride kernels, the window triple and the ReLU-on-load of one 16-byte vector.  Not for the hot path's translation units.
#pragma once
#include "common.h"

namespace {

constexpr int NT = 256;

struct Dim3 { int t, h, w; };

__device__ __forceinline__ uint4 relu8(uint4 raw) {
    f16x8 v = *reinterpret_cast<f16x8*>(&raw);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = v[e] > (f16)0 ? v[e] : (f16)0;
    return *reinterpret_cast<uint4*>(&v);
}

inline int grid_for(long long total) {
    long long b = (total + NT - 1) / NT;
    return (int)(b < 8192 ? b : 8192);
}

}  // namespace
