// mgx_ekf.hip — one predict and / or one Joseph-form measurement update of a Kalman filter's
// covariance per env (include/mgx.h "Kalman covariance step").
//
// One kernel, one workgroup of 512 threads per env:
//   products   plain FMAs on 64 x 64 output tiles, 4 x 4 results per thread, operands staged through
//              LDS in depth-16 tiles (edges zero-filled), the tile scheme of mgx_lqr.hip with a
//              transposed-B variant (A P A', P H', F P F', K R K'); the two 256-thread groups take
//              two output tiles at a time. A P, F and the narrow matrices live in the caller's
//              workspace; P is updated in place.
//   S step     wave 0 alone, lane = measurement row: S and L packed in the LDS the tiles use between
//              products, left-looking Cholesky with the pivot by readlane, y = L^-1 r, the
//              innovation statistic and log det S (every decision wave-uniform).
//   gain rows  one thread per state row: two triangular solves against L, dx = K r.
// A masked row has a zero row of H, a zero residual and the identity's row and column of S, so one
// code path serves every row mask without index compaction. Every sum runs in a fixed order and
// nothing crosses a workgroup: no atomics, no spin-waits, two calls give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <string>

#include "mgx_internal.h"
#include "mgx_common.h"
#include "mgx_ekf.h"

using namespace mgx;

namespace {

// wave 0 exchanges L's columns through LDS between workgroup barriers
__device__ __forceinline__ void ekf_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int ekf_tri(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i

// C = C0 + diag(dvec + dconst) +- A op(B): C [M][N], A [M][K], op(B) [K][N] (TB: B is stored
// [N][K]); NEG subtracts the product; C0 and dvec nullable; C may be C0 (an element is read and
// written by one thread) but neither A nor B. Called by the whole workgroup; the caller puts a
// barrier between a product and the readers of its result.
template <typename T, bool TB, bool NEG>
__device__ __forceinline__ void ekf_gemm(int M, int N, int K, const T* A, int lda, const T* B, int ldb, T* C, int ldc,
                                         const T* C0, int ldc0, const T* dvec, T dconst, T* tiles) {
  // the thread id goes through an opaque move so that the inlined products do not keep their
  // per-thread addresses live across the whole kernel (mgx_lqr.hip: they spilled there)
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int g = tid >> 8, lt = tid & 255, ty = lt >> 4, tx = lt & 15;
  T* As = tiles + g * (2 * MGX_EKF_BK * MGX_EKF_LD);
  T* Bs = As + MGX_EKF_BK * MGX_EKF_LD;
  const int tn = (N + MGX_EKF_BM - 1) / MGX_EKF_BM, ntile = ((M + MGX_EKF_BM - 1) / MGX_EKF_BM) * tn;
  for (int base = 0; base < ntile; base += MGX_EKF_GROUPS) {
    const int tile = base + g;
    const bool on = tile < ntile;  // a group without a tile keeps the barriers only
    const int i0 = on ? (tile / tn) * MGX_EKF_BM : 0, j0 = on ? (tile % tn) * MGX_EKF_BM : 0;
    T acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[i][j] = 0;
    for (int k0 = 0; k0 < K; k0 += MGX_EKF_BK) {
      if (on) {
#pragma unroll
        for (int r = 0; r < MGX_EKF_BM * MGX_EKF_BK / 256; r++) {
          const int e = lt + 256 * r;
          {
            const int i = e / MGX_EKF_BK, k = e % MGX_EKF_BK;
            T v = 0;
            if (i0 + i < M && k0 + k < K) v = A[(size_t)(i0 + i) * lda + k0 + k];
            As[k * MGX_EKF_LD + i] = v;
          }
          {
            const int j = TB ? (e / MGX_EKF_BK) : (e & 63), k = TB ? (e % MGX_EKF_BK) : (e >> 6);
            T v = 0;
            if (j0 + j < N && k0 + k < K)
              v = TB ? B[(size_t)(j0 + j) * ldb + k0 + k] : B[(size_t)(k0 + k) * ldb + j0 + j];
            Bs[k * MGX_EKF_LD + j] = v;
          }
        }
      }
      __syncthreads();
      if (on) {
#pragma unroll
        for (int k = 0; k < MGX_EKF_BK; k++) {
          T av[4], bv[4];
#pragma unroll
          for (int i = 0; i < 4; i++) av[i] = As[k * MGX_EKF_LD + ty * 4 + i];
#pragma unroll
          for (int j = 0; j < 4; j++) bv[j] = Bs[k * MGX_EKF_LD + tx * 4 + j];
#pragma unroll
          for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] += av[i] * bv[j];
        }
      }
      __syncthreads();
    }
    if (on) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int r = i0 + ty * 4 + i;
        if (r >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int c = j0 + tx * 4 + j;
          if (c >= N) continue;
          T v = NEG ? -acc[i][j] : acc[i][j];
          if (C0) v += C0[(size_t)r * ldc0 + c];
          if (r == c) v += (dvec ? dvec[r] : (T)0) + dconst;
          C[(size_t)r * ldc + c] = v;
        }
      }
    }
  }
}

// P <- (P + P') / 2 in place: each thread owns a pair (i, j), (j, i). Called by the whole workgroup.
template <typename T>
__device__ __forceinline__ void ekf_symmetrise(T* P, int n) {
  const size_t nn = (size_t)n * n;
  for (size_t idx = threadIdx.x; idx < nn; idx += MGX_EKF_THREADS) {
    const int i = (int)(idx / n), j = (int)(idx % n);
    if (i < j) {
      const T v = (T)0.5 * (P[idx] + P[(size_t)j * n + i]);
      P[idx] = v;
      P[(size_t)j * n + i] = v;
    }
  }
}

// The S step, run by wave 0 alone (lane = measurement row): S = L L' column by column, y = L^-1 r,
// nis = (y' y, 2 sum log L_ii). A masked row is the identity's in Sp and zero in rv, so it adds
// exactly 0 to both sums. A pivot that is not positive and finite sets bit 0 of *sh_info.
template <typename T>
__device__ __forceinline__ void ekf_s_step(int p, const T* Sp, T* Lp, const T* rv, T* nis, int* sh_info) {
  const int l = threadIdx.x;
  const bool row = l < p;
  for (int j = 0; j < p; j++) {
    T s = 0;
    if (row && l >= j) {
      s = Sp[ekf_tri(l, j)];
      for (int k = 0; k < j; k++) s -= Lp[ekf_tri(l, k)] * Lp[ekf_tri(j, k)];
    }
    const T pv = readlane(s, j);
    if (!(pv > 0) || !isfinite(pv)) {  // wave-uniform
      if (l == 0) *sh_info |= 1;
      return;
    }
    const T ljj = sqrt(pv);
    if (row && l >= j) Lp[ekf_tri(l, j)] = l == j ? ljj : s / ljj;
    ekf_wave_sync();
  }
  T y = row ? rv[l] : (T)0, yy = 0, ld = 0;
  for (int j = 0; j < p; j++) {
    const T ljj = Lp[ekf_tri(j, j)];
    const T yj = readlane(y, j) / ljj;
    if (l == j) y = yj;
    else if (row && l > j) y -= Lp[ekf_tri(l, j)] * yj;
    yy += yj * yj;
    ld += log(ljj);
  }
  if (l == 0) {
    nis[0] = yy;
    nis[1] = (T)2 * ld;
  }
}

template <typename T>
__global__ void __launch_bounds__(MGX_EKF_THREADS) k_ekf(EkfArgs<T> a, const uint8_t* mask) {
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;  // the rows stay untouched
  __shared__ __attribute__((aligned(16))) T tiles[MGX_EKF_TILE_REALS];
  __shared__ T rv[MGX_EKF_MAX_MEAS], Rm[MGX_EKF_MAX_MEAS];
  __shared__ int sh_info;
  const int tid = threadIdx.x, n = a.n, p = a.p, NT = MGX_EKF_THREADS;
  const size_t nn = (size_t)n * n, np = (size_t)n * p;
  T* P = a.P + (size_t)env * nn;
  T* W = a.ws + (size_t)env * a.ws_reals;
  T* F = W + nn;
  T* Hm = F + nn;
  T* G = Hm + np;  // P H', then the gain K in place
  T* KR = G + np;
  T* S = KR + np;
  T* Sp = tiles;
  T* Lp = tiles + p * (p + 1) / 2;
  if (tid == 0) sh_info = 0;

  if (a.predict) {
    // P <- A P A' + Q + diag(Q_diag), then its symmetric part
    const T* A = a.A + (size_t)env * nn;
    const T* Q = a.Q ? a.Q + (size_t)env * nn : nullptr;
    const T* Qd = a.Q_diag ? a.Q_diag + (size_t)env * n : nullptr;
    ekf_gemm<T, false, false>(n, n, n, A, n, P, n, W, n, nullptr, 0, nullptr, (T)0, tiles);
    __syncthreads();
    ekf_gemm<T, true, false>(n, n, n, W, n, A, n, P, n, Q, n, Qd, (T)0, tiles);
    __syncthreads();
    ekf_symmetrise(P, n);
    __syncthreads();
  }
  if (!a.update) {
    if (tid == 0) a.info[env] = 0;
    return;
  }

  // the masked H, residual and R: a row that is not measured is zero in all three
  const T* H = a.H + (size_t)env * np;
  const uint8_t* rm = a.row_mask ? a.row_mask + (size_t)env * p : nullptr;
  for (size_t idx = tid; idx < np; idx += NT) Hm[idx] = (!rm || rm[idx / n]) ? H[idx] : (T)0;
  if (tid < p) {
    const bool meas = !rm || rm[tid];
    rv[tid] = meas ? a.resid[(size_t)env * p + tid] : (T)0;
    Rm[tid] = meas ? a.R_diag[(size_t)env * p + tid] : (T)0;
  }
  __syncthreads();
  // G = P H', S = H G + diag(R)
  ekf_gemm<T, true, false>(n, p, n, P, n, Hm, n, G, p, nullptr, 0, nullptr, (T)0, tiles);
  __syncthreads();
  ekf_gemm<T, false, false>(p, p, n, Hm, n, G, p, S, p, nullptr, 0, Rm, (T)0, tiles);
  __syncthreads();
  // the packed lower triangle of S; a masked row's diagonal (0 so far) becomes the identity's
  for (int idx = tid; idx < p * (p + 1) / 2; idx += NT) {
    int i = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
    while (ekf_tri(i, 0) > idx) i--;
    while (ekf_tri(i + 1, 0) <= idx) i++;
    const int j = idx - ekf_tri(i, 0);
    Sp[idx] = (i == j && rm && !rm[i]) ? (T)1 : S[(size_t)i * p + j];
  }
  __syncthreads();

  if (tid < 64) ekf_s_step(p, Sp, Lp, rv, a.nis + 2 * (size_t)env, &sh_info);
  __syncthreads();
  if (sh_info & 1) {  // block-uniform: the update is skipped, P keeps the predicted covariance
    for (int i = tid; i < n; i += NT) a.dx[(size_t)env * n + i] = 0;
    if (a.gain)
      for (size_t i = tid; i < np; i += NT) a.gain[(size_t)env * np + i] = 0;
    if (tid == 0) {
      a.nis[2 * (size_t)env] = a.nis[2 * (size_t)env + 1] = std::numeric_limits<T>::quiet_NaN();
      a.info[env] = 1;
    }
    return;
  }

  // K = G S^-1 (S is symmetric: row i of K is S^-1 applied to row i of G), dx = K r, K diag(R):
  // one thread per state row
  for (int i = tid; i < n; i += NT) {
    T* k = G + (size_t)i * p;
    for (int c = 0; c < p; c++) {
      T s = k[c];
      for (int j = 0; j < c; j++) s -= Lp[ekf_tri(c, j)] * k[j];
      k[c] = s / Lp[ekf_tri(c, c)];
    }
    for (int c = p - 1; c >= 0; c--) {
      T s = k[c];
      for (int j = c + 1; j < p; j++) s -= Lp[ekf_tri(j, c)] * k[j];
      k[c] = s / Lp[ekf_tri(c, c)];
    }
    T d = 0;
    for (int c = 0; c < p; c++) {
      d += k[c] * rv[c];
      KR[(size_t)i * p + c] = k[c] * Rm[c];
      if (a.gain) a.gain[(size_t)env * np + (size_t)i * p + c] = k[c];
    }
    a.dx[(size_t)env * n + i] = d;
  }
  __syncthreads();
  // F = I - K H; P <- F P F' + K diag(R) K' (Joseph form), then its symmetric part
  ekf_gemm<T, false, true>(n, n, p, G, p, Hm, n, F, n, nullptr, 0, nullptr, (T)1, tiles);
  __syncthreads();
  ekf_gemm<T, false, false>(n, n, n, F, n, P, n, W, n, nullptr, 0, nullptr, (T)0, tiles);
  __syncthreads();
  ekf_gemm<T, true, false>(n, n, n, W, n, F, n, P, n, nullptr, 0, nullptr, (T)0, tiles);
  __syncthreads();
  ekf_gemm<T, true, false>(n, n, p, KR, p, G, p, P, n, P, n, nullptr, (T)0, tiles);
  __syncthreads();
  ekf_symmetrise(P, n);
  if (tid == 0) a.info[env] = 0;
}

template <typename T>
int launch_ekf(const mgx_ekf_io* io, int n_env, const uint8_t* mask, hipStream_t st) {
  EkfArgs<T> a;
  a.n = io->n; a.p = io->p;
  a.predict = (io->flags & MGX_EKF_PREDICT) ? 1 : 0; a.update = (io->flags & MGX_EKF_UPDATE) ? 1 : 0;
  a.A = (const T*)io->A; a.Q = (const T*)io->Q; a.Q_diag = (const T*)io->Q_diag;
  a.H = (const T*)io->H; a.R_diag = (const T*)io->R_diag; a.resid = (const T*)io->resid;
  a.row_mask = io->row_mask;
  a.P = (T*)io->P; a.dx = (T*)io->dx; a.gain = (T*)io->gain; a.nis = (T*)io->nis; a.info = io->info;
  a.ws = (T*)io->workspace; a.ws_reals = ekf_ws_reals(io->n, io->p);
  hipLaunchKernelGGL(k_ekf<T>, dim3(n_env), dim3(MGX_EKF_THREADS), 0, st, a, mask);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

bool ekf_sizes_ok(int n, int p) { return n >= 1 && n <= MGX_EKF_MAX_N && p >= 1 && p <= MGX_EKF_MAX_MEAS; }

}  // namespace

extern "C" {

int64_t mgx_ekf_bytes(const mgx_model* m, int n, int p, int n_env) {
  if (!m || n_env < 0 || !ekf_sizes_ok(n, p))
    return host_fail(MGX_E_ARG, "mgx_ekf_bytes needs a model, 1 <= n <= 4096, 1 <= p <= MGX_EKF_MAX_MEAS, n_env >= 0");
  return (int64_t)(ekf_ws_reals(n, p) * (size_t)n_env * (m->precision == MGX_F32 ? 4 : 8));
}

int mgx_ekf_step(const mgx_model* m, const mgx_ekf_io* io, int n_env, const uint8_t* env_mask, void* stream) {
  if (!m || !io || n_env < 0) return host_fail(MGX_E_ARG, "null argument or n_env < 0");
  if (!ekf_sizes_ok(io->n, io->p))
    return host_fail(MGX_E_ARG, "mgx_ekf_step needs 1 <= n <= 4096 and 1 <= p <= MGX_EKF_MAX_MEAS");
  if ((io->flags & ~(MGX_EKF_PREDICT | MGX_EKF_UPDATE)) || !(io->flags & (MGX_EKF_PREDICT | MGX_EKF_UPDATE)))
    return host_fail(MGX_E_ARG, "mgx_ekf_step flags: MGX_EKF_PREDICT, MGX_EKF_UPDATE or both, and no other bit");
  if (!io->P || !io->info) return host_fail(MGX_E_ARG, "mgx_ekf_step needs P and info");
  if ((io->flags & MGX_EKF_PREDICT) && !io->A) return host_fail(MGX_E_ARG, "MGX_EKF_PREDICT needs A");
  if ((io->flags & MGX_EKF_UPDATE) && (!io->H || !io->R_diag || !io->resid || !io->dx || !io->nis))
    return host_fail(MGX_E_ARG, "MGX_EKF_UPDATE needs H, R_diag, resid, dx and nis");
  const uint64_t need = ekf_ws_reals(io->n, io->p) * (uint64_t)n_env * (m->precision == MGX_F32 ? 4 : 8);
  if (n_env > 0 && (!io->workspace || io->workspace_bytes < need))
    return host_fail(MGX_E_ARG, "mgx_ekf_step: workspace smaller than mgx_ekf_bytes");
  if (n_env == 0) return MGX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32) return launch_ekf<float>(io, n_env, env_mask, st);
  return launch_ekf<double>(io, n_env, env_mask, st);
}

}  // extern "C"
