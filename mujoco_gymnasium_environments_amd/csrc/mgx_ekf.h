// mgx_ekf.h — arguments, tile sizes and workspace size of mgx_ekf_step (include/mgx.h "Kalman
// covariance step").
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mgx.h"

namespace mgx {

#define MGX_EKF_THREADS 512  // one workgroup per env: 8 waves, two groups of 256 threads
#define MGX_EKF_GROUPS 2     // each group owns one 64 x 64 output tile of a product at a time
#define MGX_EKF_BM 64        // output tile edge: 16 x 16 threads, 4 x 4 results each
#define MGX_EKF_BK 16        // depth of one operand tile
#define MGX_EKF_LD 68        // row stride of an operand tile in LDS, in reals
#define MGX_EKF_MAX_N 4096   // n * n stays far inside an int

// reals of LDS the operand tiles take; the packed S and L (2 x 64 x 65 / 2 = 4160) reuse them
#define MGX_EKF_TILE_REALS (MGX_EKF_GROUPS * 2 * MGX_EKF_BK * MGX_EKF_LD)
static_assert(MGX_EKF_MAX_MEAS * (MGX_EKF_MAX_MEAS + 1) <= MGX_EKF_TILE_REALS, "packed S and L fit the tiles' LDS");
static_assert(MGX_EKF_MAX_MEAS <= 64, "one lane per measurement row in the S step's wave");

// One mgx_ekf_step call, typed (mgx_ekf_io in the model's real type).
template <typename T>
struct EkfArgs {
  int n, p, predict, update;
  const T *A, *Q, *Q_diag, *H, *R_diag, *resid;
  const uint8_t* row_mask;
  T *P, *dx, *gain, *nis;
  int32_t* info;
  T* ws;
  size_t ws_reals;  // per env
};

// reals of workspace one env takes (k_ekf binds them in this order): W = A P (then F P) and
// F = I - K H [n][n] each; the masked H [p][n]; G = P H' (then K, in place) and K diag(R) [n][p]
// each; S [p][p]; rounded up to 16 bytes
inline size_t ekf_ws_reals(int n, int p) {
  const size_t r = 2 * (size_t)n * n + 3 * (size_t)n * p + (size_t)p * p;
  return (r + 3) & ~(size_t)3;
}

}  // namespace mgx
