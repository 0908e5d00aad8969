// mgx_lqr.h — arguments, tile sizes and workspace size of mgx_lqr_backward (include/mgx.h "LQR
// backward pass").
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mgx.h"

namespace mgx {

#define MGX_LQR_THREADS 512   // one workgroup per env: 8 waves, two groups of 256 threads
#define MGX_LQR_GROUPS 2      // each group owns one 64 x 64 output tile of a product at a time
#define MGX_LQR_BM 64         // output tile edge: 16 x 16 threads, 4 x 4 results each
#define MGX_LQR_BK 16         // depth of one operand tile
#define MGX_LQR_LD 68         // row stride of an operand tile in LDS, in reals
#define MGX_LQR_MAX_N 4096    // n * n stays far inside an int
#define MGX_LQR_QP_ITERS 100  // projected-Newton iterations of one box QP
#define MGX_LQR_LS_STEPS 60   // backtracking steps of one Armijo search (0.6^60 = 5e-14)

// reals of LDS the operand tiles take; the QP's packed H and L (2 x 64 x 65 / 2 = 4160) reuse them
#define MGX_LQR_TILE_REALS (MGX_LQR_GROUPS * 2 * MGX_LQR_BK * MGX_LQR_LD)
static_assert(MGX_LQR_MAX_CTRL * (MGX_LQR_MAX_CTRL + 1) <= MGX_LQR_TILE_REALS, "packed H and L fit the tiles' LDS");
static_assert(MGX_LQR_MAX_CTRL <= 64, "one lane per control in the QP's wave");

// One mgx_lqr_backward call, typed (mgx_lqr_io in the model's real type).
template <typename T>
struct LqrArgs {
  int n, m, nt, box;  // nt = T, the steps
  const T *A, *B, *lx, *lxx, *lu, *luu, *lux, *lxx_diag, *luu_diag, *Vx_T, *Vxx_T, *mu, *lo, *hi;
  T *k_ff, *gain, *expected;
  uint8_t* free_set;
  int32_t* info;
  T* ws;
  size_t ws_reals;  // per env
};

// reals of workspace one env takes (k_lqr binds them in this order): V_xx, W = V_xx A (then
// V_xx (A + B K)), A + B K [n][n] each; Wb = V_xx B [n][m]; S = l_uu K + l_ux [m][n]; Q_uu [m][m];
// V_x and V_x + V_xx B k [n] each; rounded up to 16 bytes
inline size_t lqr_ws_reals(int n, int m) {
  const size_t r = 3 * (size_t)n * n + 2 * (size_t)n * m + (size_t)m * m + 2 * (size_t)n;
  return (r + 3) & ~(size_t)3;
}

}  // namespace mgx
