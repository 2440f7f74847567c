// pointcloud.hip -- the 3D memory as a point cloud a user can take away (ABI 19): per-axis bounds of the finite points, voxel keys
// and the per-voxel mean of a key-sorted cloud.  Reference: predictions_to_glb -> SceneBuilder.build_scene
// (evoworld/reprojection/reproject_vggt_open3d_utils.py:713-766, 349-455) and save_point_cloud_to_ply (utils/plucker_embedding.py:334)
// export the filtered cloud as it is; the voxel grid follows Open3D's voxel_down_sample convention (origin = min - voxel / 2, index =
// floor((p - origin) / voxel), one averaged point and colour per occupied voxel), which the reference has at hand but does not call.
// Compiled with -ffp-contract=off: the index arithmetic is two separate float32 roundings (subtract, divide) and a floor, so that
// numpy reproduces every key.
//
//   ew_points_bounds   min / max per axis and the count of the points whose three coordinates are finite: grid-stride partials per
//                      block -> one block folds the partials in a fixed order (min / max are order-free anyway).
//   ew_voxel_keys      key = ix << 42 | iy << 21 | iz (21 bits each); non-finite point: 2^63 - 1 (sorts last); an index outside
//                      [0, 2^21) sets *overflow with a plain store.
//   (the sort of the keys is torch.sort in ops.voxel_downsample: plumbing)
//   ew_voxel_reduce    run heads of the sorted keys -> one output per run, in ascending key order.  Chunks of 256 sorted elements:
//                        1. heads per chunk                            (keys only)
//                        2. exclusive scan of the chunks' head counts  (one block; also *n_voxels)
//                        3. per chunk: gather the points through perm, segmented scan in LDS (fp64 coordinate sums, integer colour
//                           sums); runs that begin AND end inside the chunk are written; the piece in front of the chunk's first head
//                           (`lead`) and the piece from its last head on (`tail`) go to the workspace
//                        4. one block: segmented scan over the chunks' pieces, 256 chunks per step with a carry; a run that leaves its
//                           chunk is written where the next head (or the end) closes it
//                      A run of any length costs log-depth scans, never a serial walk: one voxel holding 2^20 points is 4096 chunk
//                      pieces folded in 16 steps of stage 4.  No atomics: two calls are bit-identical.
#include "common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int NT = 256;                          // threads per block = sorted elements per chunk of ew_voxel_reduce
constexpr int SCAN_NT = 1024;
constexpr int BOUNDS_MAX_BLOCKS = 1024;
constexpr long long KEY_INVALID = 0x7fffffffffffffffLL;
constexpr float GRID_LIMIT = 2097152.0f;         // 2^21 cells per axis

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX;       // false for NaN and +-inf
}

// ------------------------------------------------------------------------------------------------ bounds
struct BoundsPart {
    float mn[3], mx[3];
    unsigned long long cnt;
};

__device__ __forceinline__ void bounds_block_fold(float (&mn)[3], float (&mx)[3], unsigned long long& c, float (*s_mn)[NT],
                                                  float (*s_mx)[NT], unsigned long long* s_c) {
    const int t = threadIdx.x;
    for (int a = 0; a < 3; ++a) { s_mn[a][t] = mn[a]; s_mx[a][t] = mx[a]; }
    s_c[t] = c;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) {
            for (int a = 0; a < 3; ++a) {
                s_mn[a][t] = fminf(s_mn[a][t], s_mn[a][t + s]);
                s_mx[a][t] = fmaxf(s_mx[a][t], s_mx[a][t + s]);
            }
            s_c[t] += s_c[t + s];
        }
        __syncthreads();
    }
    for (int a = 0; a < 3; ++a) { mn[a] = s_mn[a][0]; mx[a] = s_mx[a][0]; }
    c = s_c[0];
}

__global__ __launch_bounds__(NT) void bounds_part_kernel(const float* __restrict__ xyz, size_t n, BoundsPart* __restrict__ part) {
    __shared__ float s_mn[3][NT], s_mx[3][NT];
    __shared__ unsigned long long s_c[NT];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned long long c = 0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
        const float p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        if (finite3(p[0], p[1], p[2])) {
            for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], p[a]); mx[a] = fmaxf(mx[a], p[a]); }
            ++c;
        }
    }
    bounds_block_fold(mn, mx, c, s_mn, s_mx, s_c);
    if (threadIdx.x == 0) {
        BoundsPart r;
        for (int a = 0; a < 3; ++a) { r.mn[a] = mn[a]; r.mx[a] = mx[a]; }
        r.cnt = c;
        part[blockIdx.x] = r;
    }
}

// one block; nparts = 0 (an empty cloud) leaves +inf / -inf and a count of 0
__global__ __launch_bounds__(NT) void bounds_final_kernel(const BoundsPart* __restrict__ part, int nparts, float* __restrict__ out6,
                                                          unsigned long long* __restrict__ n_finite) {
    __shared__ float s_mn[3][NT], s_mx[3][NT];
    __shared__ unsigned long long s_c[NT];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned long long c = 0;
    for (int i = threadIdx.x; i < nparts; i += NT) {
        const BoundsPart r = part[i];
        for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], r.mn[a]); mx[a] = fmaxf(mx[a], r.mx[a]); }
        c += r.cnt;
    }
    bounds_block_fold(mn, mx, c, s_mn, s_mx, s_c);
    if (threadIdx.x == 0) {
        for (int a = 0; a < 3; ++a) { out6[a] = mn[a]; out6[3 + a] = mx[a]; }
        *n_finite = c;
    }
}

inline int bounds_blocks(size_t n) {
    const size_t b = (n + NT - 1) / NT;
    return (int)(b < (size_t)BOUNDS_MAX_BLOCKS ? b : (size_t)BOUNDS_MAX_BLOCKS);
}

// ------------------------------------------------------------------------------------------------ keys
__global__ __launch_bounds__(NT) void voxel_keys_kernel(const float* __restrict__ xyz, size_t n, const float* __restrict__ origin3,
                                                        float voxel, long long* __restrict__ keys, int* __restrict__ overflow) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    long long key = KEY_INVALID;
    if (finite3(x, y, z)) {
        // float32 subtract, float32 IEEE division (no reciprocal), floor: numpy's np.floor((p - origin) / voxel) on float32 arrays
        const float fx = floorf(__fdiv_rn(x - origin3[0], voxel));
        const float fy = floorf(__fdiv_rn(y - origin3[1], voxel));
        const float fz = floorf(__fdiv_rn(z - origin3[2], voxel));
        // NaN / inf quotients (an origin or a difference beyond float32) fail the comparisons and count as overflow
        if (fx >= 0.f && fx < GRID_LIMIT && fy >= 0.f && fy < GRID_LIMIT && fz >= 0.f && fz < GRID_LIMIT)
            key = ((long long)fx << 42) | ((long long)fy << 21) | (long long)fz;
        else
            *overflow = 1;                               // plain vector store; every writer stores the same value
    }
    keys[i] = key;
}

// ------------------------------------------------------------------------------------------------ reduce
struct Piece {                                           // the sum of a run's elements inside one or more chunks
    double x, y, z;
    unsigned long long r, g, b, c;
};

__device__ __forceinline__ Piece piece_zero() { return Piece{0.0, 0.0, 0.0, 0ULL, 0ULL, 0ULL, 0ULL}; }
__device__ __forceinline__ Piece piece_add(const Piece& a, const Piece& b) {
    return Piece{a.x + b.x, a.y + b.y, a.z + b.z, a.r + b.r, a.g + b.g, a.b + b.b, a.c + b.c};
}

// round half to even of s / c in integer arithmetic
__device__ __forceinline__ unsigned mean_u8(unsigned long long s, unsigned long long c) {
    unsigned long long q = s / c;
    const unsigned long long r2 = 2 * (s - q * c);
    if (r2 > c || (r2 == c && (q & 1))) ++q;
    return (unsigned)q;
}

__device__ __forceinline__ void write_voxel(const Piece& p, size_t idx, float* __restrict__ out_xyz, unsigned* __restrict__ out_rgba,
                                            int* __restrict__ out_count) {
    if (p.c == 0) return;                                // cannot happen for a run (its head is a counted element)
    const double c = (double)p.c;
    out_xyz[3 * idx] = (float)(p.x / c);
    out_xyz[3 * idx + 1] = (float)(p.y / c);
    out_xyz[3 * idx + 2] = (float)(p.z / c);
    out_rgba[idx] = mean_u8(p.r, p.c) | (mean_u8(p.g, p.c) << 8) | (mean_u8(p.b, p.c) << 16) | 0xff000000u;
    out_count[idx] = (int)p.c;
}

// element i of the sorted keys opens a run: a valid key that differs from its predecessor
__device__ __forceinline__ bool is_head(const long long* __restrict__ keys, size_t n, size_t i) {
    if (i >= n) return false;
    const long long k = keys[i];
    return k != KEY_INVALID && (i == 0 || keys[i - 1] != k);
}

__global__ __launch_bounds__(NT) void reduce_count_kernel(const long long* __restrict__ keys, size_t n, unsigned* __restrict__ nheads) {
    __shared__ unsigned s_w[NT / 64];
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    const unsigned long long m = __ballot(is_head(keys, n, i));
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) nheads[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// cnt[0 .. nchunks) -> exclusive prefix in place, cnt[nchunks] = *n_voxels = the total
__global__ __launch_bounds__(SCAN_NT) void reduce_scan_kernel(unsigned* __restrict__ cnt, unsigned nchunks,
                                                              unsigned long long* __restrict__ n_voxels) {
    __shared__ unsigned s_v[SCAN_NT];
    __shared__ unsigned s_carry;
    const unsigned t = threadIdx.x;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (unsigned g0 = 0; g0 < nchunks; g0 += SCAN_NT) {
        const unsigned b = g0 + t;
        const unsigned own = b < nchunks ? cnt[b] : 0;
        unsigned v = own;
        for (unsigned d = 1; d < SCAN_NT; d <<= 1) {
            s_v[t] = v;
            __syncthreads();
            if (t >= d) v += s_v[t - d];
            __syncthreads();
        }
        const unsigned carry = s_carry;
        if (b < nchunks) cnt[b] = carry + v - own;
        __syncthreads();
        if (t == SCAN_NT - 1) s_carry = carry + v;
        __syncthreads();
    }
    if (t == 0) {
        cnt[nchunks] = s_carry;
        *n_voxels = s_carry;
    }
}

__global__ __launch_bounds__(NT) void reduce_chunk_kernel(const long long* __restrict__ keys, const long long* __restrict__ perm, size_t n,
                                                          const float* __restrict__ xyz, const unsigned* __restrict__ rgbx,
                                                          const unsigned* __restrict__ base, Piece* __restrict__ lead,
                                                          Piece* __restrict__ tail, float* __restrict__ out_xyz,
                                                          unsigned* __restrict__ out_rgba, int* __restrict__ out_count) {
    __shared__ double s_x[NT], s_y[NT], s_z[NT];
    __shared__ unsigned s_r[NT], s_g[NT], s_b[NT], s_c[NT], s_h[NT];
    __shared__ int s_f[NT], s_head[NT];
    const int t = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * NT + t;
    const bool head = is_head(keys, n, i);
    double x = 0.0, y = 0.0, z = 0.0;
    unsigned r = 0, g = 0, b = 0, c = 0;
    if (i < n && keys[i] != KEY_INVALID) {
        const long long p = perm[i];
        if (p >= 0 && (unsigned long long)p < n) {       // a permutation of [0, n): anything else is ignored, never dereferenced
            x = (double)xyz[3 * p]; y = (double)xyz[3 * p + 1]; z = (double)xyz[3 * p + 2];
            const unsigned w = rgbx[p];
            r = w & 255u; g = (w >> 8) & 255u; b = (w >> 16) & 255u; c = 1;
        }
    }
    unsigned h = head ? 1u : 0u;                         // heads in [0, t] (plain scan)
    int f = head ? 1 : 0;                                // a head in the window summed so far (segmented scan)
    s_head[t] = f;
    for (int d = 1; d < NT; d <<= 1) {
        s_x[t] = x; s_y[t] = y; s_z[t] = z; s_r[t] = r; s_g[t] = g; s_b[t] = b; s_c[t] = c; s_h[t] = h; s_f[t] = f;
        __syncthreads();
        if (t >= d) {
            h += s_h[t - d];
            if (!f) {
                x += s_x[t - d]; y += s_y[t - d]; z += s_z[t - d];
                r += s_r[t - d]; g += s_g[t - d]; b += s_b[t - d]; c += s_c[t - d];
                f = s_f[t - d];
            }
        }
        __syncthreads();
    }
    // here (x .. c) is the sum from the run's head, or from the chunk's first element when the head is in an earlier chunk (f == 0)
    const Piece mine{x, y, z, r, g, b, c};
    const bool last = t == NT - 1;
    if (last || s_head[last ? t : t + 1]) {              // the element in front of a head, or the chunk's last one
        if (!f) lead[blockIdx.x] = mine;
        else if (last) tail[blockIdx.x] = mine;
        else write_voxel(mine, (size_t)base[blockIdx.x] + h - 1, out_xyz, out_rgba, out_count);
    }
    if (t == 0 && head) lead[blockIdx.x] = piece_zero();   // nothing in front of the first head
}

// one block: chunk b hands on tail[b] when it has a head, and otherwise adds its whole self (lead[b]) to what it was handed; the run
// that is open on entry to a chunk with a head closes there as carry + lead[b], output base[b] - 1.  A virtual chunk behind the last
// one closes the last run.
__global__ __launch_bounds__(NT) void reduce_carry_kernel(const unsigned* __restrict__ base, unsigned nchunks, const Piece* __restrict__ lead,
                                                          const Piece* __restrict__ tail, float* __restrict__ out_xyz,
                                                          unsigned* __restrict__ out_rgba, int* __restrict__ out_count) {
    __shared__ Piece s_p[NT];
    __shared__ int s_f[NT];
    __shared__ Piece s_carry;
    const int t = threadIdx.x;
    if (t == 0) s_carry = piece_zero();
    __syncthreads();
    for (unsigned g0 = 0; g0 <= nchunks; g0 += NT) {
        const unsigned b = g0 + t;
        const bool real = b < nchunks;
        const bool has_head = real ? base[b + 1] > base[b] : b == nchunks;
        const Piece ld = real ? lead[b] : piece_zero();
        Piece v = real ? (has_head ? tail[b] : ld) : piece_zero();
        int f = has_head ? 1 : 0;
        for (int d = 1; d < NT; d <<= 1) {
            s_p[t] = v; s_f[t] = f;
            __syncthreads();
            if (t >= d && !f) {
                v = piece_add(s_p[t - d], v);
                f = s_f[t - d];
            }
            __syncthreads();
        }
        s_p[t] = v; s_f[t] = f;
        __syncthreads();
        const Piece group_carry = s_carry;
        if (has_head && base[b] >= 1) {
            Piece in = group_carry;                          // what the chunks in front of b hand to it
            if (t > 0) in = s_f[t - 1] ? s_p[t - 1] : piece_add(group_carry, s_p[t - 1]);
            write_voxel(piece_add(in, ld), (size_t)base[b] - 1, out_xyz, out_rgba, out_count);
        }
        __syncthreads();
        if (t == NT - 1) s_carry = f ? v : piece_add(group_carry, v);
        __syncthreads();
    }
}

inline size_t reduce_chunks(size_t n) { return (n + NT - 1) / NT; }
inline size_t reduce_count_bytes(size_t nchunks) { return ((nchunks + 1) * sizeof(unsigned) + 15) & ~(size_t)15; }

}  // namespace

extern "C" size_t ew_points_bounds_workspace_bytes(size_t n) { return (size_t)(n ? bounds_blocks(n) : 1) * sizeof(BoundsPart); }

extern "C" ew_status ew_points_bounds(const float* xyz, size_t n, void* ws, float* out6, unsigned long long* n_finite, void* stream) {
    EW_REQUIRE(ws && out6 && n_finite, "ew_points_bounds: NULL workspace or output");
    EW_REQUIRE(n == 0 || xyz, "ew_points_bounds: NULL xyz with n = %zu", n);
    EW_REQUIRE(n < (1ULL << 31), "ew_points_bounds: n = %zu must be below 2^31", n);
    EW_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)n_finite & 7) == 0, "ew_points_bounds: ws and n_finite must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nb = n ? bounds_blocks(n) : 0;
    if (nb) {
        hipLaunchKernelGGL(bounds_part_kernel, dim3(nb), dim3(NT), 0, st, xyz, n, (BoundsPart*)ws);
        ew_status s = ew_check_launch("bounds_part_kernel");
        if (s != EW_OK) return s;
    }
    hipLaunchKernelGGL(bounds_final_kernel, dim3(1), dim3(NT), 0, st, (const BoundsPart*)ws, nb, out6, n_finite);
    return ew_check_launch("bounds_final_kernel");
}

extern "C" ew_status ew_voxel_keys(const float* xyz, size_t n, const float* origin3, float voxel, long long* keys, int* overflow,
                                   void* stream) {
    EW_REQUIRE(origin3 && overflow, "ew_voxel_keys: NULL origin or overflow flag");
    EW_REQUIRE(voxel > 0.f && voxel <= FLT_MAX, "ew_voxel_keys: voxel = %g must be positive and finite", (double)voxel);
    EW_REQUIRE(n < (1ULL << 31), "ew_voxel_keys: n = %zu must be below 2^31", n);
    if (n == 0) return EW_OK;
    EW_REQUIRE(xyz && keys, "ew_voxel_keys: NULL xyz or keys");
    EW_REQUIRE(((uintptr_t)keys & 7) == 0, "ew_voxel_keys: keys must be 8-byte aligned");
    hipLaunchKernelGGL(voxel_keys_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, xyz, n, origin3, voxel,
                       keys, overflow);
    return ew_check_launch("voxel_keys_kernel");
}

extern "C" size_t ew_voxel_reduce_workspace_bytes(size_t n) {
    const size_t nchunks = reduce_chunks(n);
    return reduce_count_bytes(nchunks) + 2 * nchunks * sizeof(Piece);
}

extern "C" ew_status ew_voxel_reduce(const long long* sorted_keys, const long long* perm, size_t n, const float* xyz, const uint8_t* rgbx,
                                     float* out_xyz, uint8_t* out_rgba, int* out_count, void* ws, unsigned long long* n_voxels,
                                     void* stream) {
    EW_REQUIRE(ws && n_voxels, "ew_voxel_reduce: NULL workspace or n_voxels");
    EW_REQUIRE(n < (1ULL << 31), "ew_voxel_reduce: n = %zu must be below 2^31", n);
    EW_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)n_voxels & 7) == 0, "ew_voxel_reduce: ws must be 16-byte, n_voxels 8-byte aligned");
    EW_REQUIRE(n == 0 || (sorted_keys && perm && xyz && rgbx && out_xyz && out_rgba && out_count), "ew_voxel_reduce: NULL pointer");
    EW_REQUIRE(n == 0 || (((uintptr_t)sorted_keys | (uintptr_t)perm) & 7) == 0, "ew_voxel_reduce: keys and perm must be 8-byte aligned");
    EW_REQUIRE(n == 0 || (((uintptr_t)rgbx | (uintptr_t)out_rgba) & 3) == 0, "ew_voxel_reduce: colour words must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nchunks = (unsigned)reduce_chunks(n);
    unsigned* cnt = (unsigned*)ws;
    Piece* lead = (Piece*)((char*)ws + reduce_count_bytes(nchunks));
    Piece* tail = lead + nchunks;
    ew_status s;
    if (nchunks) {
        hipLaunchKernelGGL(reduce_count_kernel, dim3(nchunks), dim3(NT), 0, st, sorted_keys, n, cnt);
        if ((s = ew_check_launch("reduce_count_kernel")) != EW_OK) return s;
    }
    hipLaunchKernelGGL(reduce_scan_kernel, dim3(1), dim3(SCAN_NT), 0, st, cnt, nchunks, n_voxels);
    if ((s = ew_check_launch("reduce_scan_kernel")) != EW_OK) return s;
    if (!nchunks) return EW_OK;
    hipLaunchKernelGGL(reduce_chunk_kernel, dim3(nchunks), dim3(NT), 0, st, sorted_keys, perm, n, xyz, (const unsigned*)rgbx, cnt, lead, tail,
                       out_xyz, (unsigned*)out_rgba, out_count);
    if ((s = ew_check_launch("reduce_chunk_kernel")) != EW_OK) return s;
    hipLaunchKernelGGL(reduce_carry_kernel, dim3(1), dim3(NT), 0, st, cnt, nchunks, lead, tail, out_xyz, (unsigned*)out_rgba, out_count);
    return ew_check_launch("reduce_carry_kernel");
}
