// mgx_lqr.hip — the time-varying LQR backward pass of iLQR with optional box constraints on the
// control step (include/mgx.h "LQR backward pass").
//
// One kernel, one workgroup of 512 threads per env, walking t = T - 1 .. 0 in one launch:
//   products   plain FMAs on 64 x 64 output tiles, 4 x 4 results per thread, operands staged through
//              LDS in depth-16 tiles (edges zero-filled); the two 256-thread groups take two
//              output tiles at a time. V_xx, W, A + B K and the narrow temporaries live in the
//              caller's workspace (n = 198 does not fit LDS); the gains are solved in place in the
//              output.
//   Q_uu step  wave 0 alone, lane = control: H and L packed in the LDS the tiles use between
//              products, Cholesky column by column with the pivot by readlane, the box QP's
//              projected-Newton loop on top (every decision wave-uniform).
//   gains      one thread per column of Q_ux: two triangular solves against the L of the free block.
// Every sum runs in a fixed order and nothing crosses a workgroup: no atomics, no spin-waits, two
// calls give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <string>

#include "mgx_internal.h"
#include "mgx_common.h"
#include "mgx_lqr.h"

using namespace mgx;

namespace {

// wave 0 exchanges L's columns through LDS between workgroup barriers
__device__ __forceinline__ void lqr_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i

// C = C0 + diag(dvec) + op(A) B: C [M][N], op(A) [M][K] (TA: A is stored [K][M]), B [K][N]; C0 and
// dvec nullable; C may be C0 (an element is read and written by one thread). Called by the whole
// workgroup.
template <typename T, bool TA>
__device__ __forceinline__ void lqr_gemm(int M, int N, int K, const T* A, int lda, const T* B, int ldb, T* C, int ldc, const T* C0,
                         int ldc0, const T* dvec, T* tiles) {
  // the thread id goes through an opaque move so that the eleven inlined products of one time step
  // do not keep their per-thread addresses live across the whole time loop (they spilled)
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int g = tid >> 8, lt = tid & 255, ty = lt >> 4, tx = lt & 15;
  T* As = tiles + g * (2 * MGX_LQR_BK * MGX_LQR_LD);
  T* Bs = As + MGX_LQR_BK * MGX_LQR_LD;
  const int tn = (N + MGX_LQR_BM - 1) / MGX_LQR_BM, ntile = ((M + MGX_LQR_BM - 1) / MGX_LQR_BM) * tn;
  for (int base = 0; base < ntile; base += MGX_LQR_GROUPS) {
    const int tile = base + g;
    const bool on = tile < ntile;  // a group without a tile keeps the barriers only
    const int i0 = on ? (tile / tn) * MGX_LQR_BM : 0, j0 = on ? (tile % tn) * MGX_LQR_BM : 0;
    T acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[i][j] = 0;
    for (int k0 = 0; k0 < K; k0 += MGX_LQR_BK) {
      if (on) {
#pragma unroll
        for (int r = 0; r < MGX_LQR_BM * MGX_LQR_BK / 256; r++) {
          const int e = lt + 256 * r;
          {
            const int i = TA ? (e & 63) : (e / MGX_LQR_BK), k = TA ? (e >> 6) : (e % MGX_LQR_BK);
            T v = 0;
            if (i0 + i < M && k0 + k < K)
              v = TA ? A[(size_t)(k0 + k) * lda + i0 + i] : A[(size_t)(i0 + i) * lda + k0 + k];
            As[k * MGX_LQR_LD + i] = v;
          }
          {
            const int j = e & 63, k = e >> 6;
            T v = 0;
            if (j0 + j < N && k0 + k < K) v = B[(size_t)(k0 + k) * ldb + j0 + j];
            Bs[k * MGX_LQR_LD + j] = v;
          }
        }
      }
      __syncthreads();
      if (on) {
#pragma unroll
        for (int k = 0; k < MGX_LQR_BK; k++) {
          T av[4], bv[4];
#pragma unroll
          for (int i = 0; i < 4; i++) av[i] = As[k * MGX_LQR_LD + ty * 4 + i];
#pragma unroll
          for (int j = 0; j < 4; j++) bv[j] = Bs[k * MGX_LQR_LD + tx * 4 + j];
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
          T v = acc[i][j];
          if (C0) v += C0[(size_t)r * ldc0 + c];
          if (dvec && r == c) v += dvec[r];
          C[(size_t)r * ldc + c] = v;
        }
      }
    }
  }
}

template <typename T>
__device__ __forceinline__ T lqr_clamp(T x, T lo, T hi) {
  return x < lo ? lo : (x > hi ? hi : x);
}

// What wave 0 keeps of one Q_uu step (lane = control; the packed matrices in LDS)
template <typename T>
struct LqrWave {
  const T* Hp;  // packed lower triangle of the UNREGULARISED Q_uu
  T* Lp;        // packed Cholesky factor of the free block (identity rows for clamped controls)
  T reg;
  int m, l;
  bool row;

  __device__ __forceinline__ T h(int i, int j) const { return i >= j ? Hp[tri(i, j)] : Hp[tri(j, i)]; }
  // (Q_uu + add I) v on lane = row, v one entry per lane; columns in order
  __device__ __forceinline__ T matvec(T v, T add) const {
    T s = 0;
    for (int j = 0; j < m; j++) {
      const T vj = readlane(v, j);
      if (row) s += (h(l, j) + (l == j ? add : (T)0)) * vj;
    }
    return s;
  }
  // sum over the controls in order, the same bits in every lane
  __device__ __forceinline__ T total(T v) const {
    T s = 0;
    for (int j = 0; j < m; j++) s += readlane(v, j);
    return s;
  }
  // Cholesky of the free block of Q_uu + reg I; a clamped control's row and column are the identity's
  __device__ __forceinline__ bool factor(uint64_t fm) {
    const bool fl = (fm >> l) & 1;
    for (int j = 0; j < m; j++) {
      const bool fj = (fm >> j) & 1;
      T s = 0;
      if (row && l >= j) {
        s = (fl && fj) ? h(l, j) + (l == j ? reg : (T)0) : (l == j ? (T)1 : (T)0);
        for (int k = 0; k < j; k++) s -= Lp[tri(l, k)] * Lp[tri(j, k)];
      }
      const T pv = readlane(s, j);
      if (!(pv > 0) || !isfinite(pv)) return false;
      const T ljj = sqrt(pv);
      if (row && l >= j) Lp[tri(l, j)] = l == j ? ljj : s / ljj;
      lqr_wave_sync();
    }
    return true;
  }
  // (L L')^-1 y, one entry per lane
  __device__ __forceinline__ T solve(T y) const {
    for (int j = 0; j < m; j++) {
      const T yj = readlane(y, j) / Lp[tri(j, j)];
      if (l == j) y = yj;
      else if (row && l > j) y -= Lp[tri(l, j)] * yj;
    }
    for (int j = m - 1; j >= 0; j--) {
      const T xj = readlane(y, j) / Lp[tri(j, j)];
      if (l == j) y = xj;
      else if (l < j) y -= Lp[tri(j, l)] * xj;
    }
    return y;
  }
};

// The Q_uu step of one time step, run by wave 0 alone (lane = control): k by Cholesky or by the box
// QP, the free set, the expected decrease.
template <typename T>
__device__ __forceinline__ void lqr_quu_step(const LqrArgs<T>& a, size_t et, const T* Hp, T* Lp, T reg, uint64_t rows,
                                          const T* qu, T* kv, T& e0, T& e1, uint64_t* sh_free, int* sh_info) {
  const int tid = threadIdx.x, m = a.m;
  LqrWave<T> w;
  w.Hp = Hp; w.Lp = Lp; w.reg = reg; w.m = m; w.l = tid; w.row = tid < m;
  const bool row = w.row;
  const T q = row ? qu[tid] : (T)0;
  uint64_t fm = rows;
  int bits = 0;
  T x = 0;
  if (!a.box) {
    if (!w.factor(fm)) bits |= 1;
    else x = w.solve(row ? -q : (T)0);
  } else {
    const T lo = row ? a.lo[et * m + tid] : (T)0, hi = row ? a.hi[et * m + tid] : (T)0;
    x = row ? lqr_clamp(kv[tid], lo, hi) : (T)0;  // warm start: the k of step t + 1
    uint64_t have = 0;
    bool factored = false, full = false, done = false;
    int it = 0;
    for (; it < MGX_LQR_QP_ITERS; it++) {
      const T g = q + w.matvec(x, w.reg);
      const bool cl = row && ((x == lo && g > 0) || (x == hi && g < 0));
      fm = rows & ~ballot(cl);
      if (fm == 0) { done = true; break; }
      const bool changed = !factored || fm != have;
      if (changed) {
        if (!w.factor(fm)) { bits |= 1; break; }
        factored = true; have = fm;
      } else if (full) { done = true; break; }  // a full Newton step inside the box kept the set
      // the minimiser over the free controls with the clamped ones held
      const T gc = q + w.matvec(cl ? x : (T)0, w.reg);
      const T y = w.solve((row && !cl) ? -gc : (T)0);
      const T d = (row && !cl) ? y - x : (T)0;
      const T sdotg = w.total(d * g);
      if (!(sdotg < 0)) { done = true; break; }
      // Armijo with projection; the decrease of the quadratic from its own terms
      T step = 1, xc = x;
      bool ok = false, proj = false;
      for (int ls = 0; ls < MGX_LQR_LS_STEPS; ls++) {
        const T xn = step == (T)1 ? ((row && !cl) ? y : x) : x + step * d;
        xc = row ? lqr_clamp(xn, lo, hi) : (T)0;
        proj = ballot(row && xc != xn) != 0;
        const T dx = xc - x;
        const T gdx = w.total(dx * g);  // the first-order decrease along the projected step
        const T dv = gdx + (T)0.5 * w.total(dx * w.matvec(dx, w.reg));
        if (gdx < 0 && dv <= (T)0.1 * gdx) { ok = true; break; }
        step *= (T)0.6;
      }
      if (!ok) break;
      x = xc;
      full = step == (T)1 && !proj;
    }
    if (!done && !(bits & 1)) bits |= 2;
  }
  e0 += w.total(x * q);
  e1 += (T)0.5 * w.total(x * w.matvec(x, (T)0));
  if (row) {
    kv[tid] = x;
    a.k_ff[et * m + tid] = x;
    if (a.free_set) a.free_set[et * m + tid] = (uint8_t)((fm >> tid) & 1);
  }
  if (tid == 0) { *sh_free = fm; *sh_info |= bits; }
}

template <typename T>
__global__ void __launch_bounds__(MGX_LQR_THREADS) k_lqr(LqrArgs<T> a, const uint8_t* mask) {
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;  // the rows stay untouched
  __shared__ __attribute__((aligned(16))) T tiles[MGX_LQR_TILE_REALS];
  __shared__ T qu[MGX_LQR_MAX_CTRL], kv[MGX_LQR_MAX_CTRL], rv[MGX_LQR_MAX_CTRL];
  __shared__ T sh_reg;
  __shared__ uint64_t sh_free;
  __shared__ int sh_info;
  const int tid = threadIdx.x, n = a.n, m = a.m, NT = MGX_LQR_THREADS;
  const size_t nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
  T* Vxx = a.ws + (size_t)env * a.ws_reals;
  T* W = Vxx + nn;
  T* Acl = W + nn;
  T* Wb = Acl + nn;
  T* S = Wb + nm;
  T* Quu = S + nm;
  T* Vx = Quu + mm;
  T* hv = Vx + n;
  T* Hp = tiles;
  T* Lp = tiles + m * (m + 1) / 2;
  const uint64_t rows = m == 64 ? ~0ull : ((1ull << m) - 1);

  for (size_t i = tid; i < nn; i += NT) Vxx[i] = a.Vxx_T[(size_t)env * nn + i];
  for (int i = tid; i < n; i += NT) Vx[i] = a.Vx_T[(size_t)env * n + i];
  if (tid < m) kv[tid] = 0;
  if (tid == 0) sh_info = 0;
  T e0 = 0, e1 = 0;  // wave 0: the same in every lane
  const T mu = a.mu[env];
  __syncthreads();

  for (int t = a.nt - 1; t >= 0; t--) {
    const size_t et = (size_t)env * a.nt + t;
    const T *At = a.A + et * nn, *Bt = a.B + et * nm;
    const T *lxt = a.lx + et * n, *lut = a.lu + et * m;
    const T* lxxt = a.lxx ? a.lxx + et * nn : nullptr;
    const T* luut = a.luu ? a.luu + et * mm : nullptr;
    const T* luxt = a.lux ? a.lux + et * nm : nullptr;
    const T* lxxd = a.lxx_diag ? a.lxx_diag + et * n : nullptr;
    const T* luud = a.luu_diag ? a.luu_diag + et * m : nullptr;
    T* Kt = a.gain + et * nm;  // Q_ux, then the gains, in place

    // W = V_xx A, Wb = V_xx B, Q_u = l_u + B' V_x
    lqr_gemm<T, false>(n, n, n, Vxx, n, At, n, W, n, nullptr, 0, nullptr, tiles);
    lqr_gemm<T, false>(n, m, n, Vxx, n, Bt, m, Wb, m, nullptr, 0, nullptr, tiles);
    if (tid < m) {
      T s = 0;
      for (int i = 0; i < n; i++) s += Bt[(size_t)i * m + tid] * Vx[i];
      qu[tid] = lut[tid] + s;
    }
    __syncthreads();
    // Q_ux = l_ux + B' W, Q_uu = l_uu + B' Wb
    lqr_gemm<T, true>(m, n, n, Bt, m, W, n, Kt, n, luxt, n, nullptr, tiles);
    lqr_gemm<T, true>(m, m, n, Bt, m, Wb, m, Quu, m, luut, m, luud, tiles);
    __syncthreads();
    // the packed lower triangle of Q_uu; the regulariser from its trace
    for (int idx = tid; idx < m * (m + 1) / 2; idx += NT) {
      int i = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
      while (tri(i, 0) > idx) i--;
      while (tri(i + 1, 0) <= idx) i++;
      Hp[idx] = Quu[(size_t)i * m + (idx - tri(i, 0))];
    }
    if (tid == 0) {
      T tr = 0;
      for (int i = 0; i < m; i++) tr += Quu[(size_t)i * m + i];
      tr = tr / (T)m;
      sh_reg = mu * (tr > (T)1 ? tr : (T)1);
    }
    __syncthreads();

    if (tid < 64) lqr_quu_step(a, et, Hp, Lp, sh_reg, rows, qu, kv, e0, e1, &sh_free, &sh_info);
    __syncthreads();
    if (sh_info & 1) break;  // a failed factorisation: this env's remaining outputs stay as they were

    // K = -(Q_uu + reg I)_ff^-1 (Q_ux)_f, zero rows for the clamped controls: one thread per column
    const uint64_t fm = sh_free;
    for (int c = tid; c < n; c += NT) {
      if (fm == 0) {
        for (int i = 0; i < m; i++) Kt[(size_t)i * n + c] = 0;
        continue;
      }
      for (int i = 0; i < m; i++) {
        T s = ((fm >> i) & 1) ? Kt[(size_t)i * n + c] : (T)0;
        for (int j = 0; j < i; j++) s -= Lp[tri(i, j)] * Kt[(size_t)j * n + c];
        Kt[(size_t)i * n + c] = s / Lp[tri(i, i)];
      }
      for (int i = m - 1; i >= 0; i--) {
        T s = Kt[(size_t)i * n + c];
        for (int j = i + 1; j < m; j++) s -= Lp[tri(j, i)] * Kt[(size_t)j * n + c];
        Kt[(size_t)i * n + c] = s / Lp[tri(i, i)];
      }
      for (int i = 0; i < m; i++) Kt[(size_t)i * n + c] = ((fm >> i) & 1) ? -Kt[(size_t)i * n + c] : (T)0;
    }
    __syncthreads();

    // A + B K; S = l_uu K + l_ux; h = V_x + Wb k; r = l_u + l_uu k
    lqr_gemm<T, false>(n, n, m, Bt, m, Kt, n, Acl, n, At, n, nullptr, tiles);
    if (luut) lqr_gemm<T, false>(m, n, m, luut, m, Kt, n, S, n, luxt, n, nullptr, tiles);
    else
      for (size_t i = tid; i < nm; i += NT) S[i] = luxt ? luxt[i] : (T)0;
    for (int i = tid; i < n; i += NT) {
      T s = 0;
      for (int j = 0; j < m; j++) s += Wb[(size_t)i * m + j] * kv[j];
      hv[i] = Vx[i] + s;
    }
    if (tid < m) {
      T s = 0;
      if (luut)
        for (int j = 0; j < m; j++) s += luut[(size_t)tid * m + j] * kv[j];
      if (luud) s += luud[tid] * kv[tid];
      rv[tid] = lut[tid] + s;
    }
    __syncthreads();
    if (luud)
      for (size_t i = tid; i < nm; i += NT) S[i] += luud[i / n] * Kt[i];
    // W <- V_xx (A + B K) = W + Wb K; V_x <- l_x + K' r + l_ux' k + (A + B K)' h
    lqr_gemm<T, false>(n, n, m, Wb, m, Kt, n, W, n, W, n, nullptr, tiles);
    for (int j = tid; j < n; j += NT) {
      T s = lxt[j], u = 0;
      for (int i = 0; i < m; i++) u += Kt[(size_t)i * n + j] * rv[i];
      s += u;
      if (luxt) {
        u = 0;
        for (int i = 0; i < m; i++) u += luxt[(size_t)i * n + j] * kv[i];
        s += u;
      }
      u = 0;
      for (int i = 0; i < n; i++) u += Acl[(size_t)i * n + j] * hv[i];
      Vx[j] = s + u;
    }
    __syncthreads();
    // V_xx <- l_xx + (A + B K)' V_xx (A + B K) + K' S + l_ux' K, then its symmetric part
    lqr_gemm<T, true>(n, n, n, Acl, n, W, n, Vxx, n, lxxt, n, lxxd, tiles);
    __syncthreads();
    lqr_gemm<T, true>(n, n, m, Kt, n, S, n, Vxx, n, Vxx, n, nullptr, tiles);
    if (luxt) {
      __syncthreads();
      lqr_gemm<T, true>(n, n, m, luxt, n, Kt, n, Vxx, n, Vxx, n, nullptr, tiles);
    }
    __syncthreads();
    for (size_t idx = tid; idx < nn; idx += NT) {
      const int i = (int)(idx / n), j = (int)(idx % n);
      if (i < j) {
        const T v = (T)0.5 * (Vxx[idx] + Vxx[(size_t)j * n + i]);
        Vxx[idx] = v;
        Vxx[(size_t)j * n + i] = v;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.expected[2 * env] = e0;
    a.expected[2 * env + 1] = e1;
    a.info[env] = sh_info;
  }
}

template <typename T>
int launch_lqr(const mgx_lqr_io* io, int n_env, const uint8_t* mask, hipStream_t st) {
  LqrArgs<T> a;
  a.n = io->n; a.m = io->m; a.nt = io->T; a.box = (io->flags & MGX_LQR_BOX) ? 1 : 0;
  a.A = (const T*)io->A; a.B = (const T*)io->B; a.lx = (const T*)io->lx; a.lxx = (const T*)io->lxx;
  a.lu = (const T*)io->lu; a.luu = (const T*)io->luu; a.lux = (const T*)io->lux;
  a.lxx_diag = (const T*)io->lxx_diag; a.luu_diag = (const T*)io->luu_diag;
  a.Vx_T = (const T*)io->Vx_T; a.Vxx_T = (const T*)io->Vxx_T; a.mu = (const T*)io->mu;
  a.lo = (const T*)io->lo; a.hi = (const T*)io->hi;
  a.k_ff = (T*)io->k_ff; a.gain = (T*)io->gain; a.expected = (T*)io->expected;
  a.free_set = io->free_set; a.info = io->info;
  a.ws = (T*)io->workspace; a.ws_reals = lqr_ws_reals(io->n, io->m);
  hipLaunchKernelGGL(k_lqr<T>, dim3(n_env), dim3(MGX_LQR_THREADS), 0, st, a, mask);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

bool lqr_sizes_ok(int n, int m) { return n >= 1 && n <= MGX_LQR_MAX_N && m >= 1 && m <= MGX_LQR_MAX_CTRL; }

}  // namespace

extern "C" {

int64_t mgx_lqr_backward_bytes(const mgx_model* m, int n, int m_ctrl, int n_env) {
  if (!m || n_env < 0 || !lqr_sizes_ok(n, m_ctrl))
    return host_fail(MGX_E_ARG, "mgx_lqr_backward_bytes needs a model, 1 <= n <= 4096, 1 <= m <= MGX_LQR_MAX_CTRL, n_env >= 0");
  return (int64_t)(lqr_ws_reals(n, m_ctrl) * (size_t)n_env * (m->precision == MGX_F32 ? 4 : 8));
}

int mgx_lqr_backward(const mgx_model* m, const mgx_lqr_io* io, int n_env, const uint8_t* env_mask, void* stream) {
  if (!m || !io || n_env < 0) return host_fail(MGX_E_ARG, "null argument or n_env < 0");
  if (!lqr_sizes_ok(io->n, io->m) || io->T < 1)
    return host_fail(MGX_E_ARG, "mgx_lqr_backward needs 1 <= n <= 4096, 1 <= m <= MGX_LQR_MAX_CTRL and T >= 1");
  if (io->flags & ~MGX_LQR_BOX) return host_fail(MGX_E_ARG, "unknown mgx_lqr_backward flag bits");
  if (!io->A || !io->B || !io->lx || !io->lu || !io->Vx_T || !io->Vxx_T || !io->mu || !io->k_ff || !io->gain ||
      !io->expected || !io->info)
    return host_fail(MGX_E_ARG, "mgx_lqr_backward needs A, B, lx, lu, Vx_T, Vxx_T, mu, k_ff, gain, expected and info");
  if ((io->flags & MGX_LQR_BOX) && (!io->lo || !io->hi))
    return host_fail(MGX_E_ARG, "MGX_LQR_BOX needs lo and hi");
  const uint64_t need = lqr_ws_reals(io->n, io->m) * (uint64_t)n_env * (m->precision == MGX_F32 ? 4 : 8);
  if (n_env > 0 && (!io->workspace || io->workspace_bytes < need))
    return host_fail(MGX_E_ARG, "mgx_lqr_backward: workspace smaller than mgx_lqr_backward_bytes");
  if (n_env == 0) return MGX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32) return launch_lqr<float>(io, n_env, env_mask, st);
  return launch_lqr<double>(io, n_env, env_mask, st);
}

}  // extern "C"
