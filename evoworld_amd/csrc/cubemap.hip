// cubemap.hip -- equirectangular panorama -> cube cross (gfx950): ew_equi2cube_u8.
// One pass writes the reference's cross image uint8 [V,3E,4E,3] (E = W/4): middle row back, left, front, right; top in cell 2 of
// the first row, bottom in cell 2 of the third; the other six cells black.  The six faces are crops of the cross.
// Where the coordinates come from: ON THE DEVICE, in float64, per cross pixel -- pixel_to_xyz, theta = atan2(y, x), r = hypot(x, y),
// phi = atan2(z, r), uf = 2E (theta + pi) / pi, vf = 2E (pi/2 - phi) / pi, every product and quotient in the reference's order.  The
// map is the same for every panorama of a clip, so a thread evaluates it ONCE for its 4 pixels and then walks the V views; no table
// is read (a float64 (uf, vf) table of an edge-1024 cross would be 201 MB, 5x the image traffic of one view).  The device's atan2 /
// hypot may differ from the host libm in the last place (~1e-13 in uf); that can only show where uf or vf sits within 1e-9 of an
// integer (bilinear: the blend is continuous there, at most one level after truncation) or of a half-integer (nearest: no such pixel
// exists at the sizes measured), which is exactly the set tests/golden/cubemap.npz masks.
//   interpolation = 1: floor, +1 neighbours, all four indices clipped (no wrap at the seam), four-term float64 blend in the
//                      reference's term order, TRUNCATED to uint8 (a plateau of value A can come out as A - 1)
//   interpolation = 0: round half to even; a pixel is written only for 0 <= ui < W and 0 <= vi < H (uf == W on the seam stays black)
// Compiled with -ffp-contract=off: no product of the blend or of the coordinate chain is fused into an FMA.
// 4 pixels per thread along x, three dword stores (a cross row is 12E bytes, so every quad is 4-byte aligned).
// Reference: evoworld/inference/navigator_evoworld.py:514-705 (convert_panorama_to_cubemap; pixel_to_xyz :555-593, sampling :601-646,
// black cells :648-659, face crops :672-693).
#include "common.h"

namespace {

constexpr double kPi = 3.141592653589793;                       // math.pi

struct CubeSample {                                             // one cross pixel's source: indices already clipped / validated
    int ui, vi, u2, v2;                                         // nearest: ui < 0 means "leave black"
    double mu, nu;
};

// face of cross pixel (i, j) as the reference assigns it (:551-553), or -1 for the six black cells (:648-659)
__device__ __forceinline__ int cross_face(int i, int j, int E) {
    const int cell = i / E;
    if (j < E) return cell == 2 ? 4 : -1;
    if (j >= 2 * E) return cell == 2 ? 5 : -1;
    return cell;
}

template <bool INTERP>
__device__ __forceinline__ CubeSample cube_sample(int i, int j, int face, int E, int W, int H) {
    const double a = (2.0 * (double)i) / (double)E, b = (2.0 * (double)j) / (double)E;
    double x, y, z;
    switch (face) {                                             // pixel_to_xyz (:575-591)
        case 0: x = -1.0; y = 1.0 - a; z = 3.0 - b; break;      // back
        case 1: x = a - 3.0; y = -1.0; z = 3.0 - b; break;      // left
        case 2: x = 1.0; y = a - 5.0; z = 3.0 - b; break;       // front
        case 3: x = 7.0 - a; y = 1.0; z = 3.0 - b; break;       // right
        case 4: x = b - 1.0; y = a - 5.0; z = 1.0; break;       // top
        default: x = 5.0 - b; y = a - 5.0; z = -1.0; break;     // bottom
    }
    const double theta = atan2(y, x);
    const double r = hypot(x, y);
    const double phi = atan2(z, r);
    const double two_e = 2.0 * (double)E;
    const double uf = (two_e * (theta + kPi)) / kPi;
    const double vf = (two_e * (kPi / 2 - phi)) / kPi;
    CubeSample s;
    if (INTERP) {
        const double fu = floor(uf), fv = floor(vf);
        s.mu = uf - fu;
        s.nu = vf - fv;
        const int ui = (int)fu, vi = (int)fv;
        s.ui = min(max(ui, 0), W - 1);
        s.vi = min(max(vi, 0), H - 1);
        s.u2 = min(max(ui + 1, 0), W - 1);
        s.v2 = min(max(vi + 1, 0), H - 1);
    } else {
        const int ui = (int)rint(uf), vi = (int)rint(vf);       // np.round: half to even
        const bool valid = ui >= 0 && ui < W && vi >= 0 && vi < H;
        s.ui = valid ? ui : -1;
        s.vi = valid ? vi : 0;
        s.u2 = s.v2 = 0;
        s.mu = s.nu = 0.0;
    }
    return s;
}

__device__ __forceinline__ unsigned load_rgb(const uint8_t* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16); }

// A(1-mu)(1-nu) + B mu (1-nu) + C (1-mu) nu + D mu nu, left to right, then astype(uint8) (:627-634)
__device__ __forceinline__ unsigned blend8(unsigned A, unsigned B, unsigned C, unsigned D, double mu, double nu) {
    const double omu = 1 - mu, onu = 1 - nu;
    const double t = (((double)A * omu) * onu + ((double)B * mu) * onu) + ((double)C * omu) * nu;
    return (unsigned)(int)(t + ((double)D * mu) * nu) & 255u;
}

template <bool INTERP>
__global__ __launch_bounds__(256) void equi2cube_kernel(const uint8_t* __restrict__ pano, uint8_t* __restrict__ cross, int V, int H,
                                                        int W, int E) {
    const int qrow = W / 4;                                     // quads per cross row (= E)
    const int nq = 3 * E * qrow;
    const size_t pano_sz = (size_t)H * W * 3, cross_sz = (size_t)3 * E * W * 3;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
        const int j = q / qrow, i0 = (q - j * qrow) * 4;
        CubeSample s[4];
        bool used[4], any = false;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int face = cross_face(i0 + p, j, E);
            used[p] = face >= 0;
            if (used[p]) {
                s[p] = cube_sample<INTERP>(i0 + p, j, face, E, W, H);
                if (!INTERP && s[p].ui < 0) used[p] = false;
            }
            any |= used[p];
        }
        unsigned* d = (unsigned*)(cross + ((size_t)j * W + i0) * 3);
        for (int v = 0; v < V; ++v, d += cross_sz / 4) {
            unsigned col[4] = {0u, 0u, 0u, 0u};
            if (any) {
                const uint8_t* src = pano + (size_t)v * pano_sz;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    if (!used[p]) continue;
                    const uint8_t* r0 = src + (size_t)s[p].vi * W * 3;
                    if (INTERP) {
                        const uint8_t* r1 = src + (size_t)s[p].v2 * W * 3;
                        const unsigned A = load_rgb(r0 + s[p].ui * 3), B = load_rgb(r0 + s[p].u2 * 3);
                        const unsigned C = load_rgb(r1 + s[p].ui * 3), D = load_rgb(r1 + s[p].u2 * 3);
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            col[p] |= blend8((A >> (8 * c)) & 255u, (B >> (8 * c)) & 255u, (C >> (8 * c)) & 255u, (D >> (8 * c)) & 255u,
                                             s[p].mu, s[p].nu) << (8 * c);
                    } else {
                        col[p] = load_rgb(r0 + s[p].ui * 3);
                    }
                }
            }
            d[0] = col[0] | (col[1] << 24);
            d[1] = (col[1] >> 8) | (col[2] << 16);
            d[2] = (col[2] >> 16) | (col[3] << 8);
        }
    }
}

}  // namespace

extern "C" ew_status ew_equi2cube_u8(const uint8_t* pano, uint8_t* cross, int V, int H, int W, int interpolation, void* stream) {
    EW_REQUIRE(pano && cross && V > 0 && H > 0 && W > 0, "ew_equi2cube_u8: bad args");
    EW_REQUIRE(W == 2 * H && W % 4 == 0, "ew_equi2cube_u8: need W == 2 H and W %% 4 == 0 (edge E = W / 4)");
    EW_REQUIRE(interpolation == 0 || interpolation == 1, "ew_equi2cube_u8: interpolation must be 0 or 1");
    EW_REQUIRE(((uintptr_t)cross & 3) == 0, "ew_equi2cube_u8: cross must be 4-byte aligned");
    EW_REQUIRE(W <= (1 << 15), "ew_equi2cube_u8: W must be at most 32768");
    const int E = W / 4;
    long long blocks = ((long long)3 * E * E + 255) / 256;
    const int grid = (int)(blocks < 65536 ? blocks : 65536);
    hipStream_t s = (hipStream_t)stream;
    if (interpolation) hipLaunchKernelGGL(equi2cube_kernel<true>, dim3(grid), dim3(256), 0, s, pano, cross, V, H, W, E);
    else hipLaunchKernelGGL(equi2cube_kernel<false>, dim3(grid), dim3(256), 0, s, pano, cross, V, H, W, E);
    return ew_check_launch("ew_equi2cube_u8");
}
