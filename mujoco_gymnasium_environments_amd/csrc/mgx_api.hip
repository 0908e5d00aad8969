// mgx_api.hip — the model of libmgx.so's C-ABI (include/mgx.h): the LDS layouts, the model builder,
// mgx_model_create / destroy / get_info and the error message. Host code only (file map: DESIGN.md §3).
//
// Launch geometry: one 64-thread workgroup (= one wavefront) per environment, dynamic LDS
// sized from the model (Layout). Kernels never allocate; all state is caller-owned.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mgx_internal.h"

using namespace mgx;

namespace {
thread_local std::string g_err;
}  // namespace

namespace mgx {
int host_fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
}  // namespace mgx

// ------------------------------------------------------------------------- host side
namespace {

int align_up(int x, int a) { return (x + a - 1) / a * a; }

Layout make_layout(const mgx_model_desc* d, int real_bytes, int max_ncon, int max_nefc, int max_active,
                   bool gB = false) {
  Layout L{};
  int p = 0;
  int al = 16 / real_bytes;  // 16-byte alignment in elements
  auto take = [&](int n) { int r = p; p = align_up(p + (n > 0 ? n : 1), al); return r; };
  int nb = d->nbody, nv = d->nv, nj = d->njnt, ng = d->ngeom;
  L.max_ncon = max_ncon; L.max_nefc = max_nefc; L.max_active = max_active;
  // carry: state + frames read by env logic + factors + contacts (the finisher's inputs)
  L.qpos = take(d->nq); L.qvel = take(nv); L.ctrl = take(d->nu); L.xfrc = take(6 * nb);
  L.xpos = take(3 * nb); L.xquat = take(4 * nb); L.subtree_com = take(3 * nb);
  L.qLD = take(d->nM); L.qMH = take(d->nM); L.con_dist = take(max_ncon); L.con_mu = take(max_ncon);
  L.carry_reals = p;
  L.carry_lds = p;
  L.cfs = 9;
  const int nvw = nv > 64 ? 128 : 64;  // dof-indexed scratch vectors: one or two dofs per lane
  L.vec0 = take(nvw); L.vec1 = take(nvw); L.vec2 = take(nvw); L.vec3 = take(nvw);
  L.rk = d->integrator == 1 ? take(((d->nq + 3) & ~3) + nvw) : 0;
  // persistent for the rest of the forward pass
  // Newton with rows in global scratch (gB): the Hessian / its factor overlay the phase-A union,
  // dead from the row transform on (newton() is its only user; no env logic reads a union array
  // after the solve), and the contact frames sit in the Hessian's tail beyond the phase-A arrays
  // (live from collision to make_constraint only). The PGS block table is not allocated.
  // Assembly (fp64, 384 rows, 96 contacts): 113 -> 80 KiB per env, two envs per CU.
  const bool hess_union = gB && d->solver == 2;
  L.cdof = take(6 * nv);
  const int cf9 = align_up(9 * max_ncon, al), cp3 = align_up(3 * max_ncon, al);
  const int union_dead = align_up(9 * nb, al) + align_up(3 * nb, al) + align_up(9 * nb, al) + align_up(10 * nb, al) +
                         align_up(10 * nb, al) + align_up(6 * nb, al) + align_up(6 * nv, al) + 2 * align_up(3 * nj, al);
  // monolithic PGS models with rows in global scratch: the contact points / frames, the row
  // margins (make_constraint only) and the broadphase survivor list (collision only) overlay
  // xmat .. xanchor of the union, dead once the velocity stage is done (bipedal: 62.4 -> 51.4 KiB,
  // three envs per CU instead of two)
  const int cvel_sz = align_up(6 * nb, al);
  const int act_r = align_up((max_active * 4 + real_bytes - 1) / real_bytes, al);
  const bool mono_overlay = gB && !hess_union && !(d->layout_flags & MGX_KEEP_CVEL) &&
                            cp3 + cf9 + align_up(max_nefc, al) + act_r <= union_dead + cvel_sz;
  if (!hess_union && !mono_overlay) { L.con_pos = take(3 * max_ncon); L.con_frame = take(9 * max_ncon); }
  // wide Newton models: efc / efc_margin in global scratch (gb_efc_off), the Hessian packed lower
  const bool efcg = gB && nv > 64 && d->solver == 2;
  L.efc = take(efcg ? 1 : 8 * max_nefc); L.efc_margin = take(mono_overlay || efcg ? 1 : max_nefc);
  L.efc_blk = take(hess_union ? 1 : 2 * max_nefc);
  L.hess = (d->solver == 2 && !hess_union) ? take(nv * nv) : 0;
  // env logic that reads cvel after the step (martial arts, martial_arts_env.py:536-589) keeps
  // it out of the union the constraint rows overwrite
  const bool keep_cvel = (d->layout_flags & MGX_KEEP_CVEL) != 0;
  if (keep_cvel) L.cvel = take(6 * nb);
  // union: phase A (kinematics .. collision) arrays, then B rows on top
  int u0 = p;
  L.xmat = take(9 * nb); L.xipos = take(3 * nb); L.ximat = take(9 * nb); L.cinert = take(10 * nb);
  L.crb = take(10 * nb);
  if (!keep_cvel) L.cvel = take(6 * nb);
  L.cfrc = take(6 * nb); L.cdof_dot = take(6 * nv);
  L.xaxis = take(3 * nj); L.xanchor = take(3 * nj); L.geom_xpos = take(3 * ng); L.geom_xmat = take(9 * ng);
  L.act_force = take(d->nu);
  int endA = p;
  L.act_union = 0;
  if (mono_overlay) {
    int o = u0;
    L.con_pos = o; o += cp3;
    L.con_frame = o; o += cf9;
    L.efc_margin = o; o += align_up(max_nefc, al);
    L.act_union = o;
  }
  L.rowc = 0;
  L.Bstride = nv | 1;  // odd stride: lane-per-row access is bank-conflict free
  L.Bmat = u0;
  L.chunk_rows = max_nefc;
  if (gB) {  // rows in per-env global scratch
    L.gB = 1;
    L.gB_stride = align_up(max_nefc * L.Bstride, al);
    L.chunk_rows = 0;
    if (efcg) {  // then efc, efc_margin (the device derives the same offsets)
      L.gB_stride = gb_efm_off(L, real_bytes) + align_up(max_nefc, al);
      if (gb_efc_off(L, real_bytes) != align_up(max_nefc * L.Bstride, al)) abort();
    }
  }
  // gB: the row transform stages up to 64 rows at a time in the phase-A union (dead by then)
  L.tchunk = L.gB ? std::min(64, (endA - u0) / L.Bstride) : 0;
  if (hess_union) {
    L.hess = u0;
    L.con_pos = endA;
    L.con_frame = align_up(L.con_pos + 3 * max_ncon, al);
    endA = std::max(align_up(L.con_frame + 9 * max_ncon, al), align_up(u0 + (efcg ? nv * (nv + 1) / 2 : nv * nv), al));
  }
  int endB = align_up(u0 + L.chunk_rows * L.Bstride, al);
  L.reals = endA > endB ? endA : endB;
  int q = 0;
  auto takei = [&](int n) { int r = q; q = align_up(q + (n > 0 ? n : 1), 4); return r; };
  L.con_geom = takei(2 * max_ncon);
  L.carry_ints = q;
  L.con_pair = takei(max_ncon);
  L.act_list = takei(max_active);
  L.efc_type = takei(max_nefc); L.efc_id = takei(max_nefc);
  L.con_efcadr = takei(1);
  if (d->solver == 2 && takei(4) != team_off(L)) abort();  // Newton models: the helper-wave command words
  L.ints = q;
  L.bytes = L.reals * real_bytes + L.ints * 4;
  return L;
}

// The staged row builder (k_soccer_rows, k_rk_rows, the row stage of the settle kernels): the
// per-slot working set by liveness, so more row-builder waves share a CU (LDS-bound: 160 KiB / CU).
//   carry: the finisher's inputs; xfrc_applied and qMH (written once, read by the finisher or
//          once per step) sit in the slot's pipe carry in global memory, not in LDS (carry_lds);
//   cvel:  velocity stage -> row blocks;
//   region R, three lives: phase A (kinematics .. velocity) xipos / cinert / crb live throughout,
//          xmat / ximat / xaxis / xanchor until com_crb, then cdof_dot / cfrc / act_force and an
//          LDS copy of xfrc_applied over them; phase C (collision): the geom poses (computed from xquat just before collision,
//          geom_poses) + contact normals / points + the broadphase list (later efc_id);
//          phase D (row blocks): cacc over the geom poses.
// fp64 soccer, default capacity (64 contacts, 192 rows): 31.7 -> 19.7 KB per row-builder wave,
// eight waves per CU instead of five (the VGPR limit of the row builder is also eight).
Layout make_staged_layout(const mgx_model_desc* d, int real_bytes, int max_ncon, int max_nefc, int max_active,
                          int gcon, int chain_rec) {
  Layout L{};
  int p = 0;
  const int al = 16 / real_bytes;
  auto a = [&](int n) { return align_up(n > 0 ? n : 1, al); };
  auto take = [&](int n) { int r = p; p += a(n); return r; };
  const int nb = d->nbody, nv = d->nv, nj = d->njnt, ng = d->ngeom;
  L.max_ncon = max_ncon; L.max_nefc = max_nefc; L.max_active = max_active;
  L.staged = 1;
  L.late_geom = 1;
  L.cfs = 3;
  L.qpos = take(d->nq); L.qvel = take(nv); L.ctrl = take(d->nu);
  L.xpos = take(3 * nb); L.xquat = take(4 * nb); L.subtree_com = take(3 * nb);
  L.qLD = take(d->nM); L.con_dist = take(max_ncon);
  L.carry_lds = p;
  L.con_mu = take(max_ncon); L.xfrc = take(6 * nb); L.qMH = take(d->nM);
  L.carry_reals = p;
  p = L.carry_lds;  // the row builder's LDS continues after the LDS part of the carry
  const int nvw = nv > 64 ? 128 : 64;
  L.vec0 = take(nvw); L.vec1 = take(nvw); L.vec2 = take(nvw); L.vec3 = take(nvw);
  L.cdof = take(6 * nv);
  L.efc = take(1); L.efc_margin = take(1); L.efc_blk = take(1);
  L.cvel = take(6 * nb);
  const int R = p;
  // phase A
  L.xipos = R; L.cinert = L.xipos + a(3 * nb); L.crb = L.cinert + a(10 * nb);
  const int dead = L.crb + a(10 * nb);
  // the joint pre-pass of kinematics (chain_rec bit 0) keeps 4 reals per joint over cinert / crb,
  // which com_crb writes only after kinematics has finished; off when they do not cover it
  L.jq = L.cinert;
  L.chain_rec = 4 * nj <= dead - L.cinert ? chain_rec : chain_rec & ~1;
  L.xmat = dead; L.ximat = L.xmat + a(9 * nb); L.xaxis = L.ximat + a(9 * nb); L.xanchor = L.xaxis + a(3 * nj);
  const int endA1 = L.xanchor + a(3 * nj);
  L.cdof_dot = dead; L.cfrc = L.cdof_dot + a(6 * nv); L.act_force = L.cfrc + a(6 * nb);
  L.xfrc_lds = L.act_force + a(d->nu);
  const int endA2 = L.xfrc_lds + a(6 * nb);
  // phase C
  const int ecap = std::min(max_nefc, align_up(2 * nj, 4));  // efc_id: the joint-limit rows only
  const int nlist = std::max(max_active, ecap);
  L.geom_xpos = R; L.geom_xmat = L.geom_xpos + a(3 * ng);
  L.con_frame = L.geom_xmat + a(9 * ng);
  // the contact points live in the pipe (Pipe.o_cpos) unless gcon = 0 (MGX_GCON=0, A/B: in phase
  // C's LDS)
  L.gcon = gcon;
  L.con_pos = gcon ? 0 : L.con_frame + a(3 * max_ncon);
  L.act_union = L.con_frame + a(3 * max_ncon) + (gcon ? 0 : a(3 * max_ncon));
  const int endC = L.act_union + a((nlist * 4 + real_bytes - 1) / real_bytes);
  // phase D: cacc (12 per body) over the geom poses when they cover it, else after phase C
  L.cacc = a(12 * nb) <= L.con_frame - R ? R : endC;
  const int endD = L.cacc + a(12 * nb);
  L.reals = std::max(std::max(endA1, endA2), std::max(endC, endD));
  L.rowc = 0; L.rk = 0; L.hess = 0;
  L.Bstride = nv | 1; L.Bmat = R; L.chunk_rows = 0; L.gB = 0; L.gB_stride = 0; L.tchunk = 0;
  int q = 0;
  auto takei = [&](int n) { int r = q; q = align_up(q + (n > 0 ? n : 1), 4); return r; };
  L.con_geom = takei(2 * max_ncon);
  L.carry_ints = q;
  L.con_pair = takei(max_ncon);
  L.act_list = 0; L.efc_id = 0;  // both at act_union (env_bind)
  L.efc_type = takei(1);
  L.con_efcadr = takei(1);
  L.ints = q;
  L.bytes = L.reals * real_bytes + L.ints * 4;
  return L;
}

// The finisher binds the staged carry (all of it in LDS) and the four scratch vectors after it.
Layout finisher_layout(const Layout& S, int real_bytes) {
  Layout L = S;
  const int nvw = S.vec1 - S.vec0;
  L.vec0 = S.carry_reals; L.vec1 = L.vec0 + nvw; L.vec2 = L.vec1 + nvw; L.vec3 = L.vec2 + nvw;
  L.carry_lds = S.carry_reals;
  L.chain_rec = 0;  // no chain walk in the finisher, and no cinert / crb for the pre-pass
  L.reals = L.vec3 + nvw;
  L.ints = S.carry_ints;
  L.bytes = L.reals * real_bytes + L.ints * 4;
  return L;
}

template <typename T>
struct Builder {
  std::vector<char> host;
  std::vector<std::pair<size_t, const void**>> fix;  // (offset, pointer slot)
  size_t add(const void* src, size_t bytes, const void** slot) {
    size_t off = (host.size() + 15) / 16 * 16;
    host.resize(off + (bytes ? bytes : 16));
    if (bytes) memcpy(host.data() + off, src, bytes);
    fix.push_back({off, slot});
    return off;
  }
  template <typename S>
  void ints(const S* src, size_t n, const int** slot) {
    std::vector<int> v(n ? n : 1, 0);
    for (size_t i = 0; i < n; i++) v[i] = (int)src[i];
    add(v.data(), v.size() * 4, (const void**)slot);
  }
  void reals(const double* src, size_t n, const T** slot) {
    std::vector<T> v(n ? n : 1, (T)0);
    for (size_t i = 0; i < n; i++) v[i] = (T)src[i];
    add(v.data(), v.size() * sizeof(T), (const void**)slot);
  }
};

template <typename T>
int build_model(const mgx_model_desc* d, int device, mgx_model* out, DevModel<T>& M) {
  Builder<T> B;
  int nb = d->nbody, nv = d->nv, nj = d->njnt, ng = d->ngeom, np = d->npair, nu = d->nu;
  M.nq = d->nq; M.nv = nv; M.nu = nu; M.nbody = nb; M.njnt = nj; M.ngeom = ng; M.npair = np; M.nM = d->nM;
  M.nmaskword = d->nmaskword; M.solver = d->solver; M.integrator = d->integrator; M.cone = d->cone;
  M.iterations = d->iterations;
  M.timestep = (T)d->timestep; M.tolerance = (T)d->tolerance; M.impratio = (T)d->impratio;
  M.meaninertia = (T)d->meaninertia;
  M.has_damping = 0;  // any dof_damping > 0 at the model's precision: Euler integrates implicitly in velocity
  for (int k = 0; k < nv; k++) M.has_damping |= (T)d->dof_damping[k] > (T)0;
  for (int k = 0; k < 3; k++) M.gravity[k] = (T)d->gravity[k];
  // derived tables: body chains, dof ancestors
  std::vector<int> chain(nb * MGX_MAX_DEPTH, 0), depth(nb, 0);
  for (int b = 1; b < nb; b++) {
    std::vector<int> path;
    for (int i = b; i > 0; i = d->body_parentid[i]) path.push_back(i);
    if ((int)path.size() > MGX_MAX_DEPTH) return host_fail(MGX_E_CAPACITY, "body tree deeper than MGX_MAX_DEPTH");
    depth[b] = (int)path.size();
    for (int c = 0; c < depth[b]; c++) chain[b * MGX_MAX_DEPTH + c] = path[depth[b] - 1 - c];
  }
  std::vector<int> chainlen(nv), anc(nv * MGX_MAX_DEPTH, -1), ancadr(nv * MGX_MAX_DEPTH, 0);
  std::vector<uint64_t> ancmask(nv, 0), ancmask_hi(nv, 0);
  for (int k = 0; k < nv; k++) {
    int t = 0;
    for (int j = k; j >= 0; j = d->dof_parentid[j], t++) {
      if (t >= MGX_MAX_DEPTH) return host_fail(MGX_E_CAPACITY, "dof chain longer than MGX_MAX_DEPTH");
      anc[k * MGX_MAX_DEPTH + t] = j;
      ancadr[k * MGX_MAX_DEPTH + t] = d->dof_Madr[j];
      if (j != k) {
        if (j < 64) ancmask[k] |= 1ull << j;
        else ancmask_hi[k] |= 1ull << (j - 64);
      }
    }
    chainlen[k] = t;
  }
  B.ints(d->body_parentid, nb, &M.body_parentid); B.ints(d->body_rootid, nb, &M.body_rootid);
  B.ints(d->body_jntnum, nb, &M.body_jntnum); B.ints(d->body_jntadr, nb, &M.body_jntadr);
  B.ints(d->body_dofnum, nb, &M.body_dofnum); B.ints(d->body_dofadr, nb, &M.body_dofadr);
  B.ints(d->body_subtree_end, nb, &M.body_subtree_end); B.ints(chain.data(), chain.size(), &M.body_chain);
  B.ints(depth.data(), nb, &M.body_depth);
  {
    // chain records (DevModel.kin_*, chain_dofw): what the chain walks gather per chain position
    // and per joint, packed so that an entry's address depends on (body, position) or the joint only
    std::vector<int> hi(4 * (size_t)nb * MGX_MAX_DEPTH, 0), dofw((size_t)nb * MGX_MAX_DEPTH, 0), ji(4 * (size_t)nj, 0);
    std::vector<double> hr(8 * (size_t)nb * MGX_MAX_DEPTH, 0.0), jr(8 * (size_t)nj, 0.0);
    for (int b = 0; b < nb; b++)
      for (int c = 0; c < depth[b]; c++) {
        const size_t e = (size_t)b * MGX_MAX_DEPTH + c;
        const int i = chain[e], ja = d->body_jntadr[i], jn = d->body_jntnum[i];
        hi[4 * e] = i; hi[4 * e + 1] = jn; hi[4 * e + 2] = ja;
        hi[4 * e + 3] = jn == 1 && d->jnt_type[ja] == JFREE ? d->jnt_qposadr[ja] : -1;
        for (int k = 0; k < 3; k++) hr[8 * e + k] = d->body_pos[3 * i + k];
        for (int k = 0; k < 4; k++) hr[8 * e + 3 + k] = d->body_quat[4 * i + k];
        const int da = d->body_dofadr[i], dn = d->body_dofnum[i];
        int kind = -1;
        for (int q = da; q < da + dn; q++) {
          const int t = d->jnt_type[d->dof_jntid[q]];
          const int kt = t == JFREE || t == JBALL ? t : JHINGE;
          kind = kind < 0 || kind == kt ? kt : 4;
        }
        if (dn > 255 || (dn > 0 && da > 255)) return host_fail(MGX_E_CAPACITY, "body dof range beyond the chain records");
        dofw[e] = dn > 0 ? (da | dn << 8 | (kind < 0 ? JHINGE : kind) << 16) : 0;
      }
    for (int j = 0; j < nj; j++) {
      const int a = d->jnt_qposadr[j];
      ji[4 * j] = d->jnt_type[j]; ji[4 * j + 1] = a;
      for (int k = 0; k < 3; k++) { jr[8 * j + k] = d->jnt_axis[3 * j + k]; jr[8 * j + 3 + k] = d->jnt_pos[3 * j + k]; }
      jr[8 * j + 6] = d->qpos0[a];
    }
    B.ints(hi.data(), hi.size(), &M.kin_hi); B.ints(ji.data(), ji.size(), &M.kin_ji);
    B.ints(dofw.data(), dofw.size(), &M.chain_dofw);
    B.reals(hr.data(), hr.size(), &M.kin_hr); B.reals(jr.data(), jr.size(), &M.kin_jr);
  }
  B.add(d->body_dofmask, sizeof(uint32_t) * nb * d->nmaskword, (const void**)&M.body_dofmask);
  B.reals(d->body_pos, 3 * nb, &M.body_pos); B.reals(d->body_quat, 4 * nb, &M.body_quat);
  B.reals(d->body_ipos, 3 * nb, &M.body_ipos); B.reals(d->body_iquat, 4 * nb, &M.body_iquat);
  B.reals(d->body_mass, nb, &M.body_mass); B.reals(d->body_inertia, 3 * nb, &M.body_inertia);
  B.reals(d->body_invweight0, 2 * nb, &M.body_invweight0);
  B.ints(d->jnt_type, nj, &M.jnt_type); B.ints(d->jnt_bodyid, nj, &M.jnt_bodyid);
  B.ints(d->jnt_qposadr, nj, &M.jnt_qposadr); B.ints(d->jnt_dofadr, nj, &M.jnt_dofadr);
  B.ints(d->jnt_limited, nj, &M.jnt_limited);
  B.reals(d->jnt_pos, 3 * nj, &M.jnt_pos); B.reals(d->jnt_axis, 3 * nj, &M.jnt_axis);
  B.reals(d->jnt_range, 2 * nj, &M.jnt_range); B.reals(d->jnt_stiffness, nj, &M.jnt_stiffness);
  B.reals(d->jnt_margin, nj, &M.jnt_margin); B.reals(d->jnt_solref, 2 * nj, &M.jnt_solref);
  B.reals(d->jnt_solimp, 5 * nj, &M.jnt_solimp);
  B.ints(d->dof_bodyid, nv, &M.dof_bodyid); B.ints(d->dof_jntid, nv, &M.dof_jntid);
  B.ints(d->dof_parentid, nv, &M.dof_parentid); B.ints(d->dof_Madr, nv, &M.dof_Madr);
  B.ints(chainlen.data(), nv, &M.dof_chainlen); B.ints(anc.data(), anc.size(), &M.dof_anc);
  B.add(ancmask.data(), 8 * ancmask.size(), (const void**)&M.dof_ancmask);
  B.add(ancmask_hi.data(), 8 * ancmask_hi.size(), (const void**)&M.dof_ancmask_hi);
  B.ints(ancadr.data(), ancadr.size(), &M.dof_ancadr);
  B.reals(d->dof_armature, nv, &M.dof_armature); B.reals(d->dof_damping, nv, &M.dof_damping);
  B.reals(d->dof_invweight0, nv, &M.dof_invweight0);
  B.ints(d->geom_type, ng, &M.geom_type); B.ints(d->geom_bodyid, ng, &M.geom_bodyid);
  B.reals(d->geom_size, 3 * ng, &M.geom_size); B.reals(d->geom_pos, 3 * ng, &M.geom_pos);
  B.reals(d->geom_quat, 4 * ng, &M.geom_quat); B.reals(d->geom_rbound, ng, &M.geom_rbound);
  B.ints(d->pair_geom, 2 * np, &M.pair_geom); B.ints(d->pair_condim, np, &M.pair_condim);
  B.reals(d->pair_friction, 5 * np, &M.pair_friction); B.reals(d->pair_margin, np, &M.pair_margin);
  {
    std::vector<int> bpi(4 * (size_t)np, 0);
    std::vector<double> bpr(4 * (size_t)np, 0.0);
    for (int p = 0; p < np; p++) {
      const int g1 = d->pair_geom[2 * p], g2 = d->pair_geom[2 * p + 1];
      const int t1 = d->geom_type[g1], t2 = d->geom_type[g2];
      const double mg = d->pair_margin[p];
      auto boxed = [](int t) { return t == GBOX || t == GCAPSULE || t == GCYLINDER; };
      int kind = 0;
      if (t1 == GPLANE) kind = 1;
      else if (boxed(t1) && boxed(t2)) kind = 2;
      else if (t1 == GSPHERE && boxed(t2)) kind = 4;
      else if (t2 == GSPHERE && boxed(t1)) kind = 8;
      bpi[4 * p] = g1; bpi[4 * p + 1] = g2; bpi[4 * p + 2] = kind;
      bpr[4 * p] = t1 == GPLANE ? d->geom_rbound[g2] + mg : d->geom_rbound[g1] + d->geom_rbound[g2] + mg;
      bpr[4 * p + 1] = mg;
      bpr[4 * p + 2] = kind == 4 ? d->geom_rbound[g1] : (kind == 8 ? d->geom_rbound[g2] : 0.0);
    }
    B.ints(bpi.data(), bpi.size(), &M.pair_bpi);
    B.reals(bpr.data(), bpr.size(), &M.pair_bpr);
    std::vector<double> obb(3 * (size_t)ng, 0.0);
    for (int g = 0; g < ng; g++) {
      const double* sz = d->geom_size + 3 * g;
      const int t = d->geom_type[g];
      if (t == GBOX) { obb[3 * g] = sz[0]; obb[3 * g + 1] = sz[1]; obb[3 * g + 2] = sz[2]; }
      if (t == GCAPSULE) { obb[3 * g] = sz[0]; obb[3 * g + 1] = sz[0]; obb[3 * g + 2] = sz[1] + sz[0]; }
      if (t == GCYLINDER) { obb[3 * g] = sz[0]; obb[3 * g + 1] = sz[0]; obb[3 * g + 2] = sz[1]; }
    }
    B.reals(obb.data(), obb.size(), &M.geom_obb);
  }
  B.reals(d->pair_gap, np, &M.pair_gap); B.reals(d->pair_solref, 2 * np, &M.pair_solref);
  B.reals(d->pair_solimp, 5 * np, &M.pair_solimp);
  B.ints(d->actuator_trnid, nu, &M.actuator_trnid); B.ints(d->actuator_ctrllimited, nu, &M.actuator_ctrllimited);
  B.ints(d->actuator_forcelimited, nu, &M.actuator_forcelimited);
  B.reals(d->actuator_gear, nu, &M.actuator_gear); B.reals(d->actuator_ctrlrange, 2 * nu, &M.actuator_ctrlrange);
  B.reals(d->actuator_forcerange, 2 * nu, &M.actuator_forcerange);
  B.reals(d->actuator_gainprm, 3 * nu, &M.actuator_gainprm); B.reals(d->actuator_biasprm, 3 * nu, &M.actuator_biasprm);
  B.reals(d->qpos0, d->nq, &M.qpos0); B.reals(d->qpos_spring, d->nq, &M.qpos_spring);
  MGX_HIPCHK(hipSetDevice(device));
  MGX_HIPCHK(hipMalloc(&out->dbuf, B.host.size()));
  MGX_HIPCHK(hipMemcpy(out->dbuf, B.host.data(), B.host.size(), hipMemcpyHostToDevice));
  out->dbytes = B.host.size();
  for (auto& f : B.fix) *f.second = (char*)out->dbuf + f.first;
  return MGX_OK;
}

}  // namespace

namespace mgx {
int host_check_state(const mgx_state* s) {
  if (!s || !s->qpos || !s->qvel || !s->qacc_warmstart || !s->ctrl || !s->qfrc_applied || !s->xfrc_applied || !s->time)
    return host_fail(MGX_E_ARG, "null state buffer");
  return MGX_OK;
}
int host_check_scratch(const mgx_model* m, const mgx_state* s) {
  if (m->L.gB && !s->scratch)
    return host_fail(MGX_E_ARG, "this model needs mgx_state.scratch (scratch_bytes_per_env)");
  return MGX_OK;
}
}  // namespace mgx

extern "C" {

const char* mgx_last_error(void) { return g_err.c_str(); }

int mgx_abi_version(void) { return MGX_ABI_VERSION; }

int mgx_model_create(const mgx_model_desc* d, int precision, int device, mgx_model** out) {
  if (!d || !out) return host_fail(MGX_E_ARG, "null argument");
  if (precision != MGX_F32 && precision != MGX_F64) return host_fail(MGX_E_ARG, "precision must be MGX_F32 or MGX_F64");
  // nv <= 64: one dof per lane (every task kernel); 64 < nv <= 128: the wide kernels only
  // (mgx_wide.h, two dofs per lane: humanoid_construction, nv 99), which every other configure
  // entry point refuses
  if (d->nv > MGX_MAX_NV_WIDE) return host_fail(MGX_E_CAPACITY, "nv > 128 not supported by the wave-per-env kernels");
  if (d->nbody > 4096 || (d->solver != 0 && d->solver != 2) || (d->integrator != 0 && d->integrator != 1))
    return host_fail(MGX_E_UNSUPPORTED, "this build implements PGS or Newton with Euler or RK4");
  bool condim13 = true;  // the staged row builder packs one contact per 4-row block
  for (int p = 0; p < d->npair; p++) {
    const int c = d->pair_condim[p];
    if (c != 1 && c != 3 && c != 4 && c != 6) return host_fail(MGX_E_UNSUPPORTED, "condim must be 1, 3, 4 or 6");
    condim13 = condim13 && (c == 1 || c == 3);
  }
  std::unique_ptr<mgx_model> owner(new mgx_model());  // deletes a refused model on every exit below
  mgx_model* m = owner.get();
  m->hooks = read_hooks();
  m->precision = precision;
  m->device = device;
  m->npair = d->npair;
  m->wide = d->nv > MGX_MAX_NV;
  // capacities: the model's request (efc_capacity / con_capacity), else 192 rows / 64 contacts.
  // MGX_MAX_NEFC / MGX_MAX_NCON may raise them (read here, once); a value below the model's is
  // refused: it would drop rows MuJoCo keeps. A smaller capacity is a property of the model itself
  // (mgx_model_desc.efc_capacity / con_capacity), never of the environment.
  int max_nefc = d->efc_capacity > 0 ? d->efc_capacity : 192;
  int max_ncon = d->con_capacity > 0 ? d->con_capacity : 64;
  if (const char* v = getenv("MGX_MAX_NEFC")) {
    if (atoi(v) < max_nefc) return host_fail(MGX_E_ARG, "MGX_MAX_NEFC below the model's row capacity");
    max_nefc = atoi(v);
  }
  if (const char* v = getenv("MGX_MAX_NCON")) {
    if (atoi(v) < max_ncon) return host_fail(MGX_E_ARG, "MGX_MAX_NCON below the model's contact capacity");
    max_ncon = atoi(v);
  }
  if (max_nefc > 1024 || max_ncon > 512) return host_fail(MGX_E_CAPACITY, "capacity above 1024 rows / 512 contacts");
  max_nefc = (max_nefc + 3) & ~3;  // the staged solver sweeps rows in blocks of 4
  if (max_nefc < 4 || max_ncon < 1) return host_fail(MGX_E_ARG, "row / contact capacity too small");
  int rb = precision == MGX_F32 ? 4 : 8;
  // broadphase survivor list: 128 for the small candidate sets (soccer 251, parkour 48 pairs),
  // up to 768 for large ones (bipedal 3185 pairs)
  int max_active = d->npair <= 256 ? 128 : (d->npair < 768 ? d->npair : 768);
  // the staged soccer pipeline handles Euler + PGS models up to 64 * MGX_EFC_SLOTS rows
  m->staged_ok = d->integrator == 0 && d->solver == 0 && max_nefc <= 64 * MGX_EFC_SLOTS && condim13 &&
                 d->nv <= 56;  // the solver's block table holds 7 dof groups of 8 (pgs_load_tab)
  // the monolithic layout of a staged model (its reset settle steps, the rare fixup resets,
  // --mono, mgx_debug_forward) keeps rows in LDS at the default 192 rows / 64 contacts; the
  // staged step itself carries the model's full capacity
  // the staged RK4 step (mgx_rk_staged.h, bipedal_rescue): RK4 + PGS, nv 49..64 (four register
  // entries per solver lane, a 16-word block table)
  m->staged_rk_ok = d->integrator == 1 && d->solver == 0 && condim13 && d->nv > 48 && d->nv <= 64 &&
                    max_nefc <= 1024 && max_ncon <= 192;  // three contact-metadata lane sets (RK_NCS)
  // ... and of a staged RK4 model (its checkAcc template, --mono) at most 512 rows, whose per-row
  // LDS arrays fit next to its working set with the rows in global scratch
  // A staged Euler model whose monolithic layout keeps its rows in global scratch (parkour) carries
  // the full capacity there too: only its per-row scalars are in LDS.
  const bool mono_lds_rows = !(d->layout_flags & MGX_ROWS_IN_SCRATCH);
  const int mono_nefc = m->staged_ok && mono_lds_rows && max_nefc > 192 ? 192
                        : (m->staged_rk_ok && max_nefc > 512 ? 512 : max_nefc);
  const int mono_ncon = m->staged_ok && mono_lds_rows && max_ncon > 64 ? 64 : max_ncon;
  m->L = make_layout(d, rb, mono_ncon, mono_nefc, max_active);
  // rows that do not fit next to the rest of the per-env LDS working set go to global scratch
  if (m->L.bytes > 160 * 1024 || (d->layout_flags & MGX_ROWS_IN_SCRATCH))
    m->L = make_layout(d, rb, mono_ncon, mono_nefc, max_active, true);
  const bool any_staged = m->staged_ok || m->staged_rk_ok;
  m->Ls = make_staged_layout(d, rb, max_ncon, any_staged ? max_nefc : 4, m->staged_ok ? 128 : max_active,
                             m->hooks.gcon, m->hooks.chain_records);
  m->Lf = finisher_layout(m->Ls, rb);
  {
    const int tight = m->hooks.tight_bp >= 0 ? (m->hooks.tight_bp != 0) : (d->npair > MGX_TIGHT_BROADPHASE_PAIRS);
    m->L.tight_bp = m->Ls.tight_bp = m->Lf.tight_bp = tight;
  }
  int rc;
  if (precision == MGX_F32) {
    rc = build_model<float>(d, device, m, m->mf);
    m->mf.L = m->L; m->mfs = m->mf; m->mfs.L = m->Ls; m->mff = m->mf; m->mff.L = m->Lf;
  } else {
    rc = build_model<double>(d, device, m, m->md);
    m->md.L = m->L; m->mds = m->md; m->mds.L = m->Ls; m->mdf = m->md; m->mdf.L = m->Lf;
  }
  if (rc != MGX_OK) return rc;
  if (m->L.bytes > 160 * 1024) return host_fail(MGX_E_CAPACITY, "per-env LDS exceeds 160 KiB");
  if (int r = step_kernels_configure(m)) return r;
  if (int r = forward_kernels_configure(m)) return r;
  if (int r = dyn_kernels_configure(m)) return r;
  if (int r = ik_kernels_configure(m)) return r;
  if (m->wide)
    if (int r = wide_kernels_configure(m)) return r;
  if (int r = soccer_kernels_configure(m)) return r;
  *out = owner.release();
  return MGX_OK;
}

int mgx_model_destroy(mgx_model* m) {
  if (!m) return MGX_OK;
  mgx::ray_release(m);
  mgx::sensor_release(m);
  if (m->dbuf) (void)hipFree(m->dbuf);
  delete m;
  return MGX_OK;
}

int mgx_model_get_info(const mgx_model* m, mgx_model_info* o) {
  if (!m || !o) return host_fail(MGX_E_ARG, "null argument");
  int nq, nv, nu, nb, nj, ng;
  if (m->precision == MGX_F32) { nq = m->mf.nq; nv = m->mf.nv; nu = m->mf.nu; nb = m->mf.nbody; nj = m->mf.njnt; ng = m->mf.ngeom; }
  else { nq = m->md.nq; nv = m->md.nv; nu = m->md.nu; nb = m->md.nbody; nj = m->md.njnt; ng = m->md.ngeom; }
  o->nq = nq; o->nv = nv; o->nu = nu; o->nbody = nb; o->njnt = nj; o->ngeom = ng; o->npair = m->npair;
  o->max_nv = MGX_MAX_NV; o->max_nbody = 4096; o->max_ncon = m->L.max_ncon; o->max_nefc = m->L.max_nefc;
  o->max_njnt = 1 << 20; o->precision = m->precision; o->lds_bytes_per_env = m->L.bytes;
  o->lds_bytes_rows = m->Ls.bytes; o->lds_bytes_finish = m->Lf.bytes;
  o->scratch_bytes_per_env = m->L.gB ? m->L.gB_stride * (m->precision == MGX_F32 ? 4 : 8) : 0;
  return MGX_OK;
}

}  // extern "C"
