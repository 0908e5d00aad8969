// mgx_sensor.h — device tables of mgx_sensor_configure and the buffer views of mgx_forward /
// mgx_sensor (include/mgx.h "sensors, mj_forward and contact forces").
#pragma once
#include <string>

#include "../../include/mgx.h"
#include "mgx_common.h"

namespace mgx {

// Site and sensor tables (reals in the model's type), one device allocation.
template <typename T>
struct SensorTab {
  int nsite, nsensor, nsensordata;
  int need_kin, need_vel, need_acc;  // stages the kernel runs: kinematics / com + velocity / rnePostConstraint
  const int *site_bodyid, *site_type;          // [nsite]
  const T *site_pos, *site_quat, *site_size;   // [nsite][3|4|3]
  const int *type, *objtype, *objid, *dim, *adr;  // [nsensor]
  const T* cutoff;                                // [nsensor]
  T magnetic0, magnetic1, magnetic2;  // option.magnetic
};

// Caller buffers of one forward pass, typed (mgx_forward_out). The sensor kernel reads them.
template <typename T>
struct FwdBuf {
  T *qacc, *qfrc_constraint;
  int *ncon, *con_geom;
  T *con_dist, *con_pos, *con_frame, *con_force;
};

// Host side of the model's sensor tables (mgx_model.sensor).
struct SensorState {
  bool unsupported = false;  // a sensor this build does not compute; `why` names it
  std::string why;
  int nsensordata = 0, lds_bytes = 0;
  bool need_acc = false;
  void* dbuf = nullptr;
  SensorTab<float> tf;
  SensorTab<double> td;
};

// reals of LDS one env of k_sensor binds: the arrays kinematics / com_crb / velocity_bodies touch,
// then qacc, cacc, cfrc_ext, cfrc_int, the sensordata row and the site frames (position, quaternion)
__host__ __device__ inline int sensor_lds_reals(int nq, int nv, int nu, int nb, int nj, int nM, int nsd, int nsite) {
  return nq + nv + 2 * nu + nb * (3 + 4 + 9 + 3 + 9 + 3 + 10 + 10 + 6 + 6) + 6 * nj + 12 * nv + 2 * nM + nv +
         18 * nb + nsd + 7 * nsite;
}

}  // namespace mgx
