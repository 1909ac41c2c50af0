// filters_invert_dev.h - the one 8 x 8 inverse of the filter kernels: kernels_filters.hip's update and innovation kernels and
// kernels_filters_refine.hip's measurement all call it.
#pragma once
#include "filters_dev.h"

namespace hnet {
namespace {
// hnet_ekf::invert(A, 8) on the LDS matrices A [64] and V [64] (V = I on entry, A^-1 on return): Gauss-Jordan with partial pivoting, the header's
// operations in the header's order per element, lane t < 64 holding element (t >> 3, t & 7) of both.  Every thread of the workgroup takes the barriers
// (lanes 64 and above do nothing else), so every call is uniform over the workgroup; A and V are published on entry.  -> singular: a pivot that is
// exactly 0, A and V then hold the elimination as far as it went.
__device__ inline bool invert8_lanes(double* A, double* V) {
    const int t = threadIdx.x, i = t >> 3, j = t & 7;
    for (int col = 0; col < 8; col++) {
        int piv = col;
        for (int r = col + 1; r < 8; r++)
            if (fabs(A[r * 8 + col]) > fabs(A[piv * 8 + col])) piv = r;
        if (A[piv * 8 + col] == 0.0) return true;                                // (every lane sees the same LDS values)
        __syncthreads();
        if (piv != col && t < 16) {
            double* X = t < 8 ? A : V;
            const double tmp = X[col * 8 + j];
            X[col * 8 + j] = X[piv * 8 + j];
            X[piv * 8 + j] = tmp;
        }
        __syncthreads();
        const double d = 1.0 / A[col * 8 + col];
        __syncthreads();
        if (t < 16) (t < 8 ? A : V)[col * 8 + j] *= d;
        __syncthreads();
        const double f = t < 64 ? A[i * 8 + col] : 0.0;
        __syncthreads();
        if (t < 64 && i != col && f != 0.0) {
            A[t] -= f * A[col * 8 + j];
            V[t] -= f * V[col * 8 + j];
        }
        __syncthreads();
    }
    return false;
}
}  // namespace
}  // namespace hnet
