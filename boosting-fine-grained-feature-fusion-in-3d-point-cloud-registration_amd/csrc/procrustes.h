// The fp64 parts of the Procrustes solve shared by pose.hip (weighted Kabsch of the forward)
// and icp.hip (the ICP update): the block reduction of per-thread fp64 partials and the
// rotation from a 3x3 covariance by a one-sided Jacobi SVD. Internal linkage: each translation
// unit that includes this header compiles its own copy.
#pragma once
#include "common.h"

namespace fgr {
namespace {

constexpr int kPoseThreads = 256;

__device__ void block_reduce(double* vals, int n, double* sh) {
    // vals: per-thread partials (n <= 16); sh: [kPoseThreads/64][16]
    const int wv = threadIdx.x / 64, lane = threadIdx.x % 64;
    for (int i = 0; i < n; ++i) {
        double v = vals[i];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) sh[wv * 16 + i] = v;
    }
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        double t = 0.0;
        for (int w = 0; w < kPoseThreads / 64; ++w) t += sh[w * 16 + i];
        vals[i] = t;
    }
    __syncthreads();
}

__device__ void svd3_rotation(const double H[3][3], double R[3][3]) {
    // one-sided Jacobi: A = H V with orthogonal columns -> A = U S
    double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = H[i][j];
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p) {
            for (int qq = p + 1; qq < 3; ++qq) {
                double al = 0, be = 0, ga = 0;
                for (int i = 0; i < 3; ++i) {
                    al += A[i][p] * A[i][p];
                    be += A[i][qq] * A[i][qq];
                    ga += A[i][p] * A[i][qq];
                }
                if (fabs(ga) <= 1e-300 || fabs(ga) <= 1e-15 * sqrt(al * be)) continue;
                off = fmax(off, fabs(ga) / sqrt(al * be));
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int i = 0; i < 3; ++i) {
                    const double x = A[i][p], y = A[i][qq];
                    A[i][p] = cs * x - sn * y;
                    A[i][qq] = sn * x + cs * y;
                    const double vx = V[i][p], vy = V[i][qq];
                    V[i][p] = cs * vx - sn * vy;
                    V[i][qq] = sn * vx + cs * vy;
                }
            }
        }
        if (off < 1e-15) break;
    }
    double sig[3], U[3][3];
    for (int j = 0; j < 3; ++j) sig[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
    // sort singular values descending (permute columns of A and V)
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (sig[j] < sig[j + 1]) {
                double ts = sig[j]; sig[j] = sig[j + 1]; sig[j + 1] = ts;
                for (int r = 0; r < 3; ++r) {
                    double ta = A[r][j]; A[r][j] = A[r][j + 1]; A[r][j + 1] = ta;
                    double tv = V[r][j]; V[r][j] = V[r][j + 1]; V[r][j + 1] = tv;
                }
            }
    const double tiny = 1e-30 + 1e-13 * sig[0];
    int rank = 0;
    for (int j = 0; j < 3; ++j) {
        if (sig[j] > tiny) {
            for (int r = 0; r < 3; ++r) U[r][j] = A[r][j] / sig[j];
            ++rank;
        }
    }
    if (rank == 0) {
        for (int r = 0; r < 3; ++r)
            for (int j = 0; j < 3; ++j) U[r][j] = (r == j) ? 1.0 : 0.0;
    } else {
        if (rank == 1) {
            // any unit vector orthogonal to u0
            double e[3] = {0, 0, 0};
            int m = fabs(U[0][0]) < fabs(U[1][0]) ? (fabs(U[0][0]) < fabs(U[2][0]) ? 0 : 2)
                                                  : (fabs(U[1][0]) < fabs(U[2][0]) ? 1 : 2);
            e[m] = 1.0;
            double d = e[0] * U[0][0] + e[1] * U[1][0] + e[2] * U[2][0];
            double u1[3] = {e[0] - d * U[0][0], e[1] - d * U[1][0], e[2] - d * U[2][0]};
            double nn = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
            for (int r = 0; r < 3; ++r) U[r][1] = u1[r] / nn;
        }
        if (rank <= 2) {
            U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
            U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
            U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
        }
    }
    // R = V U^T ; reflection fix flips V[:, 2]
    double Rp[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            Rp[i][j] = V[i][0] * U[j][0] + V[i][1] * U[j][1] + V[i][2] * U[j][2];
    const double det = Rp[0][0] * (Rp[1][1] * Rp[2][2] - Rp[1][2] * Rp[2][1]) -
                       Rp[0][1] * (Rp[1][0] * Rp[2][2] - Rp[1][2] * Rp[2][0]) +
                       Rp[0][2] * (Rp[1][0] * Rp[2][1] - Rp[1][1] * Rp[2][0]);
    const double f = det > 0 ? 1.0 : -1.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R[i][j] = V[i][0] * U[j][0] + V[i][1] * U[j][1] + f * V[i][2] * U[j][2];
}

}  // namespace
}  // namespace fgr
