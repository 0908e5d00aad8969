// mgx_staged_host.hip — the host code the three staged tasks share (soccer: mgx_soccer.hip; bipedal:
// mgx_rk_staged.hip; parkour: mgx_pk_staged.hip): the workspace layout (make_staged_pipe) and the
// workspace entries over it, the solver waves' LDS sizes, the MGX_* hook reader and the side
// stream. No kernel is defined here.
#include "mgx_internal.h"

using namespace mgx;

// LDS bytes of one main-launch solver wave: its slots' row scalars, block tables and compressed B
// (tools/pgs_census.py measures what the slots need at bench conditions); 16 lanes per slot =
// 4 slots per wave, 64 lanes = 1
static int pgs_arena_bytes(int precision) {
  const int a = precision == MGX_F32 ? MGX_PGS_ARENA_F32 : MGX_PGS_ARENA_F64;
  return pgs_lanes() == 64 ? a / 2 : a;
}

// LDS bytes of the soccer wide launch's one-slot waves with B in LDS (pgs_group BLDS sizes: whole
// ring turns of blocks plus the look-ahead, 16-byte rounded B) for the model's largest slot, or 0
// when that exceeds 160 KiB or MGX_PGS_WIDE_LDS=0 (B from global memory, the A/B alternative)
int mgx::wide_arena_bytes(const mgx_model* m) {
  const int wide_lds = m->hooks.pgs_wide_lds;
  const int rb = m->precision == MGX_F32 ? 4 : 8;
  const int nv = m->precision == MGX_F32 ? m->mf.nv : m->md.nv;
  const int maxE = m->Ls.max_nefc;
  const int nbRun = (maxE / 4 + MGX_PGS_RING_LDS - 1) / MGX_PGS_RING_LDS * MGX_PGS_RING_LDS;
  const int nbA = nbRun + MGX_PGS_RING_LDS - 1;
  const int bcap = 32 + (maxE / 4) * (8 + 32 * ((nv + 7) / 8));
  const int worst = nbA * (4 * MGX_SCAL * rb + 4 * mgx_twl(false)) + ((bcap + 3) & ~3) * rb;
  return wide_lds && pgs_lanes() == 16 && worst + 64 <= 160 * 1024 ? (worst + 15) & ~15 : 0;
}

// Staged-step workspace layout for (model, n_env, banks); offsets in bytes, 256-aligned. rk: the
// RK4 staged step's extra arrays (stage carry, template scratch); nobs: floats per bank observation.
size_t mgx::make_staged_pipe(const mgx_model* m, void* ws, int n_env, int banks, Pipe* P, bool rk, int nobs,
                             int split_default) {
  int rb = m->precision == MGX_F32 ? 4 : 8;
  int nq = m->precision == MGX_F32 ? m->mf.nq : m->md.nq;
  int nv = m->precision == MGX_F32 ? m->mf.nv : m->md.nv;
  Pipe p{};
  p.base = (char*)ws;
  p.N = n_env; p.R = banks; p.S = n_env * (1 + banks);
  p.maxE = m->Ls.max_nefc; p.nv = nv; p.dpl = (nv + 7) / 8;  // solver: support entries per lane
  // test hook: MGX_PGS_LDS_ROWS (Hooks.pgs_lds_rows, read at model creation) lowers the main
  // launch's LDS rows, so ordinary states exercise the wide-LDS launch (tests/test_gpu_capacity.py)
  const Hooks& H = m->hooks;
  const bool cap_env = H.pgs_lds_rows > 0;
  int capE = cap_env ? (H.pgs_lds_rows + 3) / 4 * 4 : MGX_PGS_LDS_ROWS;
  if (capE < 4 || capE > p.maxE) capE = MGX_PGS_LDS_ROWS;
  if (rk) {
    // the RK4 pipeline's rows (bipedal: ~150 per forward, up to 512): MGX_RK_LDS_ROWS, default 256
    capE = H.rk_lds_rows > 0 ? (H.rk_lds_rows + 3) / 4 * 4 : 256;
    if (capE < 4) capE = 256;
  }
  p.capE = p.maxE < capE ? p.maxE : capE;
  // soccer at full capacity (more rows than MGX_PGS_LDS_ROWS): the main launch keeps as many rows
  // of LDS row scalars per slot as four waves per CU allow (fp64: 224), the wide launch beside it
  // solves the rare slot beyond that with its B in LDS (measured, one box: 1.554M env-steps/s
  // against 1.460M for one main launch over every slot with its row scalars read from the pipe at
  // six waves per CU, 1.534M for that launch held to four; reduced capacity 1.647M).
  // MGX_PGS_SINGLE=1 selects the single main launch (A/B); the MGX_PGS_LDS_ROWS test hook sets the
  // main launch's rows directly.
  p.sqg = 0;
  if (!rk && !cap_env && !H.pgs_lds_b && p.maxE > MGX_PGS_LDS_ROWS) {
    if (H.pgs_single) {
      p.capE = p.maxE;
      p.sqg = 1;
    } else {
      // MGX_PGS_WPC (A/B): size the LDS rows for more waves per CU than four; the slots beyond
      // them run in the main launch with their scalars from the pipe (hmain), whose LDS then
      // sets the wave's allocation when it is the larger
      const int budget = 160 * 1024 / H.pgs_wpc;
      int r = H.pgs_wpc == 4 ? MGX_PGS_LDS_ROWS : 8;
      while (r + 8 <= p.maxE && staged_pgs_lds_bytes(m, r + 8, pgs_lanes(), 0, mgx_twl(false)) <= budget) r += 8;
      p.capE = r;
    }
  }
  // the wide launch (slots over capE rows: soccer in the split mode) copies its one slot's B, row
  // scalars and block table into LDS when the largest slot fits 160 KiB (MGX_PGS_WIDE_LDS=0: B
  // from global memory, the A/B alternative). Same sizes as pgs_group's BLDS path: whole ring
  // turns of blocks plus the look-ahead, 16-byte rounded B.
  p.warena = !rk && p.maxE > p.capE ? wide_arena_bytes(m) : 0;
  // LDS arena of one main-launch solver wave (scalars + block table + B of its slots); the
  // test / tuning hook MGX_PGS_ARENA overrides it (a small arena sends waves to the global-B launch)
  p.arena = pgs_arena_bytes(m->precision);
  if (H.pgs_arena > 0 && H.pgs_arena <= 96 * 1024) p.arena = H.pgs_arena;
  p.carry_stride = ((m->Ls.carry_reals + 63) & ~63) + 5 * 64;
  p.carryi_stride = m->Ls.carry_ints + 8;
  p.bcap = 32 + (p.maxE / 4) * (8 + 32 * ((nv + 7) / 8));
  p.tw = MGX_TW;  // block-table words (uint32) per 4-row block in the pipe, either B layout (mgx_staged.h)
  p.nobs = nobs;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t r = off; off = (off + bytes + 255) / 256 * 256; return r; };
  size_t S = (size_t)p.S, NB = (size_t)n_env * (banks > 0 ? banks : 1);
  p.o_ctr = take(64);
  p.o_carry = take(S * p.carry_stride * rb);
  p.o_carryi = take(S * p.carryi_stride * 4);
  p.o_ne = take(S * 4); p.o_blen = take(S * 4); p.o_niter = take(S * 4); p.o_k2list = take(S * 4); p.o_k2big = take(S * 4); p.o_fix = take((size_t)n_env * 4);
  // the solver-list buckets are sized for the model's capacity, not the main launch's rows (a
  // per-call hook changes those), so the workspace layout never depends on MGX_PGS_LDS_ROWS
  // heavy slots in the main launch (hmain, the full-capacity soccer default): when the SQG layout of
  // maxE rows fits the LDS of a capE-row wave. The MGX_PGS_LDS_ROWS test hook keeps the wide launch.
  p.hmain = !rk && !cap_env && !p.sqg && !H.pgs_lds_b && p.capE < p.maxE &&
            staged_pgs_lds_bytes(m, p.maxE, pgs_lanes(), 1, mgx_twl(false)) <=
                (H.pgs_wpc == 4 ? staged_pgs_lds_bytes(m, p.capE, pgs_lanes(), 0, mgx_twl(false))
                                : 160 * 1024 / H.pgs_wpc);
  if (p.hmain) p.warena = 0;
  // row-split waves (pgs_group SPLIT): the main launch's slots of at least split_blocks blocks get a
  // wave each. The threshold never exceeds capE / 4 + 1, so every slot over capE rows is split and
  // neither the heavy-slot path (hmain) nor the wide launch is needed. A split wave's LDS is one
  // slot of up to maxE rows (scalars, forces, table), which must fit the main launch's allocation
  // of four slots x capE rows so that the launch keeps its waves per CU; only the MGX_PGS_LDS_ROWS
  // test hook, whose few rows make that allocation tiny, raises the launch's LDS to it instead.
  p.split_blocks = 0;
  const int split = H.pgs_split_blocks >= 0 ? H.pgs_split_blocks : split_default;
  if (!rk && !p.sqg && !H.pgs_lds_b && pgs_lanes() == 16 && split > 0) {
    const int one = staged_pgs_lds_bytes(m, p.maxE, 64, 0, mgx_twl(false));
    int main_lds = staged_pgs_lds_bytes(m, p.capE, 16, 0, mgx_twl(false));
    if (p.hmain) main_lds = std::max(main_lds, staged_pgs_lds_bytes(m, p.maxE, 16, 1, mgx_twl(false)));
    // a split wave addresses its slot's B with 32-bit byte offsets from the slot's base (pgs_b_at)
    const bool b32 = (uint64_t)p.bcap * (uint64_t)rb < (1ull << 32);
    if (b32 && one <= (cap_env ? 160 * 1024 : main_lds)) {
      p.split_blocks = std::min(split, p.capE / 4 + 1);
      p.hmain = 0;
      p.warena = 0;
    }
  }
  p.prio_rows = H.pgs_prio_rows > 0 ? H.pgs_prio_rows : p.capE;
  p.nbk = (p.hmain || p.split_blocks ? p.maxE : p.capE) / 4 + 1;
  p.o_hist = take((size_t)(p.maxE / 4 + 1) * 4);
  p.o_blist = take((size_t)(p.maxE / 4 + 1) * S * 4);
  p.o_scal = take(S * p.maxE * MGX_SCAL * rb);
  p.o_blk = take(S * (p.maxE / 4) * p.tw * 4);  // tw uint32 per 4-row block
  p.o_B = take(S * (size_t)p.bcap * rb);
  p.o_vout = take(S * 64 * rb);
  p.o_bq = take(NB * nq * rb); p.o_bv = take(NB * nv * rb); p.o_ba = take(NB * nv * rb); p.o_btime = take(NB * rb);
  p.o_bobs = take(NB * nobs * 4); p.o_bprev = take(NB * 6 * rb); p.o_bwind = take(NB * 3 * rb);
  p.o_bk = take(NB * 4); p.o_bep = take(NB * 4); p.o_bwarn = take(NB * 4); p.o_bseed = take(NB * 8);
  int nb = m->precision == MGX_F32 ? m->mf.nbody : m->md.nbody;
  p.maxC = m->Ls.max_ncon;
  p.o_cpos = take(S * 3 * (size_t)p.maxC * rb);
  p.o_tq = take(nq * rb); p.o_tv = take(nv * rb); p.o_ta = take(64 * rb); p.o_tt = take(rb);
  p.o_tx = take(3 * nb * rb); p.o_txq = take(4 * nb * rb); p.o_tsc = take(3 * nb * rb); p.o_tn = take(4);
  p.o_tcg = take(2 * p.maxC * 4); p.o_tcd = take(p.maxC * rb); p.o_tcm = take(p.maxC * rb);
  // per-slot ints: the RK4 step's warnings / overflow over its stages, parkour's overflow flag over
  // its substeps; the checkAcc template kernel's rows when the monolithic layout keeps them in
  // global memory
  p.o_rkw = take(S * 4);
  p.o_tscr = take(m->L.gB ? (size_t)m->L.gB_stride * rb : 64);
  if (rk) {
    const int nq4 = (nq + 3) & ~3;
    p.rk_stride = 2 * nq4 + 8 * 64 + 4;
    p.o_rk = take(S * p.rk_stride * rb);
    p.o_rks = take(S * 4);
  }
  // the bank slots' own solver-list state (the bank view of the pipe, MGX_BANK_STREAM) and the
  // bank finisher's work flags; taken last, so every other offset is what it was without them
  p.o_ctr2 = take(64);
  p.o_hist2 = take((size_t)(p.maxE / 4 + 1) * 4);
  p.o_blist2 = take((size_t)(p.maxE / 4 + 1) * NB * 4);
  p.o_k2list2 = take(NB * 4); p.o_k2big2 = take(NB * 4);
  p.o_bstg = take(NB * 4);
  // the tail finisher's deferred resets (MGX_TAIL_FINISH): a count, then up to N envs
  p.o_defer = take(((size_t)n_env + 1) * 4);
  p.qmh_pre = 0;  // set per step by soccer_step_staged
  if (P) *P = p;
  return off;
}

// The workspace entries of a staged task (StagedTask, mgx_internal.h)
size_t mgx::task_pipe(const StagedTask& t, const mgx_model* m, void* ws, int n_env, int banks, Pipe* P) {
  return make_staged_pipe(m, ws, n_env, banks, P, t.rk, t.nobs, t.split_default);
}
int mgx::task_pipe_checked(const StagedTask& t, const mgx_model* m, void* ws, uint64_t ws_bytes, int n_env, int banks,
                           Pipe* P, size_t* need) {
  const size_t n = task_pipe(t, m, ws, n_env, banks, P);
  if (need) *need = n;
  if (ws_bytes < n)
    return host_fail(MGX_E_ARG, std::string("workspace smaller than mgx_") + t.name + "_workspace_bytes");
  return MGX_OK;
}
int mgx::staged_check(const StagedTask& t, const mgx_model* m, int banks) {
  if (!t.ok(m)) return host_fail(MGX_E_UNSUPPORTED, t.refusal);
  if (banks < 0 || banks > 16) return host_fail(MGX_E_ARG, "banks must be in [0, 16]");
  return MGX_OK;
}
int64_t mgx::staged_workspace_bytes(const StagedTask& t, const mgx_model* m, int n_env, int banks) {
  if (!m || n_env <= 0 || banks < 0 || banks > 16) return host_fail(MGX_E_ARG, "bad argument");
  if (!t.ok(m)) return host_fail(MGX_E_UNSUPPORTED, t.refusal);
  return (int64_t)task_pipe(t, m, nullptr, n_env, banks, nullptr);
}
int mgx::staged_workspace_init(const StagedTask& t, const mgx_model* m, void* workspace, uint64_t bytes, int n_env,
                               int banks, hipStream_t st) {
  if (!m || !workspace || n_env <= 0 || banks < 0 || banks > 16) return host_fail(MGX_E_ARG, "bad argument");
  if (t.init_checks && !t.ok(m)) return host_fail(MGX_E_UNSUPPORTED, t.refusal);
  Pipe P;
  size_t need;
  if (int rc = task_pipe_checked(t, m, workspace, bytes, n_env, banks, &P, &need)) return rc;
  MGX_HIPCHK(hipMemsetAsync(workspace, 0, need, st));
  const size_t nb = (size_t)n_env * (banks > 0 ? banks : 1);
  MGX_HIPCHK(hipMemsetAsync(P.base + P.o_bk, 0xFF, nb * 4, st));  // bank settle counters = -1 (empty)
  // the checkAcc template (load_template), once per workspace
  const int gB = m->L.gB ? 1 : 0;
  if (m->precision == MGX_F32) hipLaunchKernelGGL(t.template_f32[gB], dim3(1), dim3(64), m->L.bytes, st, m->mf, P);
  else hipLaunchKernelGGL(t.template_f64[gB], dim3(1), dim3(64), m->L.bytes, st, m->md, P);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

// LDS of one solver wave holding `rows` rows per slot (main launch: min(max_nefc,
// MGX_PGS_LDS_ROWS); wide launch: max_nefc)
int mgx::staged_pgs_lds_bytes(const mgx_model* m, int rows, int lps, int sqg, int twl) {
  int rb = m->precision == MGX_F32 ? 4 : 8;
  int nb3 = (rows / 4 + MGX_PGS_RING - 1) / MGX_PGS_RING * MGX_PGS_RING;  // whole ring turns
  const int spw = 64 / lps;
  // the row scalars (or, SQG: the forces only; pgs_group) + the block table
  const int sq = sqg ? 4 : 4 * MGX_SCAL;
  return spw * (sq * nb3 + 4) * rb + spw * nb3 * 4 * twl + 64;
}

// Hooks (mgx_internal.h): the MGX_* A/B and test variables, read once per model
mgx::Hooks mgx::read_hooks() {
  Hooks h;
  auto get = [](const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
  };
  h.pgs_lds_rows = get("MGX_PGS_LDS_ROWS", 0);
  h.rk_lds_rows = get("MGX_RK_LDS_ROWS", 0);
  h.pgs_single = get("MGX_PGS_SINGLE", 0);
  h.pgs_lds_b = get("MGX_PGS_LDS_B", MGX_PGS_LDS_B) != 0;
  h.pgs_arena = get("MGX_PGS_ARENA", 0);
  h.pgs_lds_pad = get("MGX_PGS_LDS_PAD", 0);
  h.pgs_wide_lds = get("MGX_PGS_WIDE_LDS", 1);
  h.pgs_spw = get("MGX_PGS_SPW", 0);
  h.pgs_prio_rows = get("MGX_PGS_PRIO_ROWS", 0);
  h.pgs_split_blocks = get("MGX_PGS_SPLIT_BLOCKS", -1);
  h.tight_bp = get("MGX_TIGHT_BROADPHASE", -1);
  h.pgs_wpc = get("MGX_PGS_WPC", 4);
  if (h.pgs_wpc < 4 || h.pgs_wpc > 16) h.pgs_wpc = 4;
  // MGX_SIDE_STREAM=0 runs the wide solver launch after the main one on the caller's stream: with
  // more streams than hardware queues (several tasks on one GPU, each on its own stream) a side
  // stream can queue behind another task's long kernels
  h.side_stream = get("MGX_SIDE_STREAM", 1) != 0;
  // MGX_BANK_STREAM: the soccer reset banks' rows -> PGS -> bank finisher on a library-owned stream
  // of the lowest priority beside the live step (soccer_step_staged); 1: the bank finisher before
  // the live finisher, 2: after it; 0: one stream. MGX_SIDE_STREAM=0 turns it off as well.
  // Not set (-1): MGX_BANK_STREAM (mgx_staged.h); in fp32 only together with the tail finisher
  // (MGX_TAIL_FINISH), without which it measured 2% slower there (the fp32 solver launch is
  // shorter, so its idle tail holds less than the sharing costs).
  h.bank_stream = get("MGX_BANK_STREAM", -1);
  if (h.bank_stream < -1 || h.bank_stream > 2) h.bank_stream = 0;
  // MGX_TAIL_FINISH: the soccer step's row-split (heavy) solver waves on a side stream, the light
  // envs finished on the caller's stream beside them and the heavy envs after them
  // (soccer_step_staged). Off wherever the side stream is (MGX_SIDE_STREAM=0, MGX_PGS_LDS_B,
  // MGX_PGS_SINGLE) and without row-split waves. Not set (-1): MGX_TAIL_FINISH (mgx_staged.h)
  // beside the bank stream, off on one stream (where only 1 turns it on).
  h.tail_finish = get("MGX_TAIL_FINISH", -1);
  if (h.tail_finish < -1 || h.tail_finish > 1) h.tail_finish = 0;
  // MGX_TAIL_FACTOR (with the tail finisher): 1 the row builder factorises qMH for the heavy slots,
  // whose finish ends the step (Pipe.qmh_pre); 0 never; 2 for every slot (test hook)
  h.tail_factor = get("MGX_TAIL_FACTOR", 1);
  if (h.tail_factor < 0 || h.tail_factor > 2) h.tail_factor = 1;
  h.gcon = get("MGX_GCON", 1);
  h.rows_lds = get("MGX_ROWS_LDS", 0);
  // MGX_CHAIN_RECORDS (Layout.chain_rec of the staged row builders): 1 the joint pre-pass of
  // kinematics, 2 the packed chain records, 3 both, 0 neither (A/B and the bit-identity test)
  h.chain_records = get("MGX_CHAIN_RECORDS", 3) & 3;
  return h;
}

// the side stream of a caller stream (mgx_internal.h)
SideStream* mgx::side_stream(hipStream_t st) {
  return stream_cache<SideStream>(st, [](SideStream& x) {
    return hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(&x.rows, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&x.big, hipEventDisableTiming) == hipSuccess;
  });
}

int mgx::staged_settle_lds(const mgx_model* m, const Pipe& P, int lps, int sqg, int twl) {
  return std::max({staged_pgs_lds_bytes(m, P.maxE, lps, sqg, twl), m->Ls.bytes, m->Lf.bytes});
}
