// jpeg_tables.h -- what the MJPEG encoder (video.hip) and decoder (video_decode.hip) share: the zigzag order and the 8-point DCT matrix.
#pragma once
#include "common.h"

namespace {

// zigzag position -> natural index (T.81 figure A.6)
__device__ __constant__ unsigned char d_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// 0.5 * cos(j * pi / 16), j = 0 .. 8
constexpr float HALF_COS[9] = {0.5f,
                               0.4903926402016152f,
                               0.46193976625564337f,
                               0.4157348061512726f,
                               0.35355339059327373f,
                               0.27778511650980114f,
                               0.19134171618254492f,
                               0.09754516100806417f,
                               0.0f};

// entry (k, n) of the orthonormal 8-point DCT-II: sqrt(1/8) for k = 0, else 0.5 * cos((2n + 1) k pi / 16)
constexpr float dct_m(int k, int n) {
    if (k == 0) return HALF_COS[4];
    int m = ((2 * n + 1) * k) % 32;
    if (m > 16) m = 32 - m;
    return m > 8 ? -HALF_COS[16 - m] : HALF_COS[m];
}

}  // namespace
