// SimEnv.reset from the reference motion, on the device: the state the
// simulated humanoid records after DeepMimicCore's reset_time(t) (gym-simenv/gym_simenv/envs/
// sim_env.py:270-285 -> DeepMimicCore.cpp:85-88), computed per lane from the motion clip:
//
//   pose(t), vel(t)   Motion::CalcFrame / CalcFrameVel (anim/Motion.cpp:267-305): frame
//                     index + blend (CalcIndexBlend :495-522), KinTree::LerpPoses
//                     (anim/KinTree.cpp:1577-1620: root slerp + normalize, spherical slerp,
//                     revolute lerp; Eigen 3.3.7's slerp), root StandardizeQuat
//                     (KinCharacter::CalcPose, anim/KinCharacter.cpp:573-596), loop cycle
//                     offset (MotionController::CalcPose); frame velocities lerped
//   placement         SetCharRandPlacement on the plane ground: root x, z -> 0
//                     (scenes/SceneSimChar.cpp:545-562, sim/Ground.cpp:154-159)
//   kinematics        JointWorldTrans (KinTree.cpp:1126-1135 + ChildParentTrans*), body attach
//                     points, world body velocities (RBDUtil::CalcWorldVel)
//   ground resolve    ResolveCharGroundIntersect (scenes/SceneSimChar.cpp:565-607): lift the
//                     root by the deepest AABB violation (0.001 pad) of the body shapes
//                     (Bullet 2.88 getAabb of sphere / capsule / box)
//   state             CtController::BuildStatePose / BuildStateVel (sim/CtController.cpp:
//                     378-495): root y, heading-frame body positions, tangent-normal body
//                     rotations, heading-frame velocities (world for the root when
//                     RecordWorldRootRot)
//
// The clip is preprocessed once on the host (amp_extensions_amd/motion.py: PostProcessFrames
// and BuildFrameVel, Motion.cpp:167-188, 415-442) and uploaded as one fp64 blob
// (amx_set_motion).  One 64-thread workgroup per lane, one thread per joint / body, fp64
// throughout, the lane's joint frames in LDS: a reset's latency is a few tree levels deep
// instead of a serial walk over every joint (resets are a few lanes per step after the first).
#include "amx_common.h"

namespace {

constexpr int MAXJ = 16;   // joints / bodies
constexpr int MAXD = 96;   // pose / velocity dofs
constexpr int HDR = 16;
enum { JT_REVOLUTE = 0, JT_FIXED = 3, JT_SPHERICAL = 4, JT_ROOT = 5 };
enum { SH_BOX = 0, SH_CAPSULE = 1, SH_SPHERE = 2 };

struct MView {  // views into the device blob
  const double* h;
  const double* joints;  // [J][8]: type, parent, offset, size, ax, ay, az, -
  const double* bodies;  // [J][8]: shape, ax, ay, az, p0, p1, p2, valid
  const double* times;   // [F]
  const double* frames;  // [F][D]
  const double* vels;    // [F][D]
  int J, D, F;
  __device__ MView(const double* b) {
    h = b;
    J = (int)h[0];
    D = (int)h[1];
    F = (int)h[2];
    joints = b + HDR;
    bodies = joints + 8 * J;
    times = bodies + 8 * J;
    frames = times + F;
    vels = frames + (long long)F * D;
  }
};

struct Q { double w, x, y, z; };
struct V3 { double x, y, z; };

__device__ inline V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline V3 scale(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// 3x3 row-major
__device__ inline V3 mv(const double* m, V3 v) {
  return {m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z,
          m[6] * v.x + m[7] * v.y + m[8] * v.z};
}
__device__ inline void mm(const double* a, const double* b, double* o) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
// cMathUtil::RotateMat(quaternion) (util/MathUtil.cpp:212-251)
__device__ inline void qmat(Q q, double* m) {
  const double sqw = q.w * q.w, sqx = q.x * q.x, sqy = q.y * q.y, sqz = q.z * q.z;
  const double invs = 1 / (sqx + sqy + sqz + sqw);
  m[0] = (sqx - sqy - sqz + sqw) * invs;
  m[4] = (-sqx + sqy - sqz + sqw) * invs;
  m[8] = (-sqx - sqy + sqz + sqw) * invs;
  double t1 = q.x * q.y, t2 = q.z * q.w;
  m[3] = 2.0 * (t1 + t2) * invs;
  m[1] = 2.0 * (t1 - t2) * invs;
  t1 = q.x * q.z; t2 = q.y * q.w;
  m[6] = 2.0 * (t1 - t2) * invs;
  m[2] = 2.0 * (t1 + t2) * invs;
  t1 = q.y * q.z; t2 = q.x * q.w;
  m[7] = 2.0 * (t1 + t2) * invs;
  m[5] = 2.0 * (t1 - t2) * invs;
}
// cMathUtil::RotateMat(axis, theta) for the unit axes used here
__device__ inline void axis_mat(V3 a, double th, double* m) {
  const double c = cos(th), s = sin(th), x = a.x, y = a.y, z = a.z;
  m[0] = c + x * x * (1 - c); m[1] = x * y * (1 - c) - z * s; m[2] = x * z * (1 - c) + y * s;
  m[3] = y * x * (1 - c) + z * s; m[4] = c + y * y * (1 - c); m[5] = y * z * (1 - c) - x * s;
  m[6] = z * x * (1 - c) - y * s; m[7] = z * y * (1 - c) + x * s; m[8] = c + z * z * (1 - c);
}
// cMathUtil::RotMatToQuaternion (util/MathUtil.cpp:310-345)
__device__ inline Q mat_q(const double* m) {
  const double tr = m[0] + m[4] + m[8];
  if (tr > 0) {
    const double S = sqrt(tr + 1.0) * 2;
    return {0.25 * S, (m[7] - m[5]) / S, (m[2] - m[6]) / S, (m[3] - m[1]) / S};
  }
  if (m[0] > m[4] && m[0] > m[8]) {
    const double S = sqrt(1.0 + m[0] - m[4] - m[8]) * 2;
    return {(m[7] - m[5]) / S, 0.25 * S, (m[1] + m[3]) / S, (m[2] + m[6]) / S};
  }
  if (m[4] > m[8]) {
    const double S = sqrt(1.0 + m[4] - m[0] - m[8]) * 2;
    return {(m[2] - m[6]) / S, (m[1] + m[3]) / S, 0.25 * S, (m[5] + m[7]) / S};
  }
  const double S = sqrt(1.0 + m[8] - m[0] - m[4]) * 2;
  return {(m[3] - m[1]) / S, (m[2] + m[6]) / S, (m[5] + m[7]) / S, 0.25 * S};
}
__device__ inline Q qmul(Q a, Q b) {
  return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
// Eigen: q * v = v + w*uv + u x uv, uv = 2 (u x v)
__device__ inline V3 qrot(Q q, V3 v) {
  const V3 u = {q.x, q.y, q.z};
  V3 uv = cross(u, v);
  uv = add(uv, uv);
  return add(add(v, scale(uv, q.w)), cross(u, uv));
}
// Eigen 3.3.7 QuaternionBase::slerp
__device__ inline Q slerp(Q a, Q b, double t) {
  const double one = 1.0 - 2.220446049250313e-16;
  const double d = a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z;
  const double ad = fabs(d);
  double s0, s1;
  if (ad >= one) {
    s0 = 1.0 - t;
    s1 = t;
  } else {
    const double th = acos(ad), st = sin(th);
    s0 = sin((1.0 - t) * th) / st;
    s1 = sin(t * th) / st;
  }
  if (d < 0) s1 = -s1;
  return {s0 * a.w + s1 * b.w, s0 * a.x + s1 * b.x, s0 * a.y + s1 * b.y, s0 * a.z + s1 * b.z};
}
__device__ inline Q qnorm(Q q) {
  const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  return {q.w / n, q.x / n, q.y / n, q.z / n};
}
__device__ inline Q ldq(const double* p) { return {p[0], p[1], p[2], p[3]}; }

// Per-wave scratch of motion_state (LDS): one 64-thread workgroup computes one lane's state,
// thread j owning joint / body j.
struct MotionLds {
  double hdr[HDR], jt[8 * MAXJ], bt[8 * MAXJ];  // blob header and joint / body tables
  double pose[MAXD], vel[MAXD];
  double R[MAXJ][9];
  V3 o[MAXJ], w[MAXJ], v[MAXJ], bp[MAXJ];
};

__device__ inline double wave_min(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmin(x, __shfl_xor(x, off));
  return x;
}

// Copy the blob header and the joint / body tables into LDS (one pass of independent loads
// instead of the dependent parent-chain walks reading them from HBM) and return a view whose
// tables point there.
__device__ inline MView stage_tables(const double* blob, double* hdr, double* jt, double* bt) {
  const MView g(blob);
  for (int i = threadIdx.x; i < HDR; i += blockDim.x) hdr[i] = g.h[i];
  for (int i = threadIdx.x; i < 8 * g.J; i += blockDim.x) {
    jt[i] = g.joints[i];
    bt[i] = g.bodies[i];
  }
  __syncthreads();
  MView m = g;
  m.h = hdr;
  m.joints = jt;
  m.bodies = bt;
  return m;
}

// ---- reset noise: cKinCharacter::AddNoise (anim/KinCharacter.cpp:340-470) -------------------
// SceneImitate::ResetKinCharTime (scenes/SceneImitate.cpp:469-489) perturbs the kinematic pose /
// velocity at the reset time before the sim character takes them (SyncCharacters) and before the
// placement and the ground resolve (SceneSimChar.cpp:699-716).  The reference draws from
// DeepMimicCore's process-global std::default_random_engine (util/Rand.cpp), which cannot be
// reproduced; here draw k of a reset comes from Philox(seed; lane, reset#, k/2, tag) (tags split
// RandomRotatePoseVel's RandDouble stream from AddNoisePoseVel's RandDoubleEigen stream, as the
// reference's mRandGen / mGen), or from an injected [B][ld] table (tests: rotation draws at
// [0, AMX_NOISE_ROT_SLOTS), pose / velocity draws after them).  u -> lo + u (hi - lo) as
// cRand::RandDouble.  Same operation order as oracle/deepmimic_ref.add_noise.
constexpr uint32_t kTagNoiseRot = 0x4E524F54u;  // 'NROT'
constexpr uint32_t kTagNoisePV = 0x4E505620u;   // 'NPV '

struct NoiseArgs {
  int on;  // any noise (radian != 0 or (min, max) != (0, 0))
  int bef_rot, rot_vel_w_pose, vel_noise, knee_rot;
  double lo, hi, radian, interp;
  const double* draws;  // nullable injected uniforms [B][ld]
  long long ld;
  uint32_t k0, k1;      // Philox key
};

struct NoiseDraws {
  const NoiseArgs& n;
  int lane, rc;
  __device__ double u(int k, bool pv) const {
    if (n.draws) return n.draws[(long long)lane * n.ld + (pv ? AMX_NOISE_ROT_SLOTS : 0) + k];
    const amx::u32x4 r = amx::philox4x32_10({(uint32_t)lane, (uint32_t)rc, (uint32_t)(k >> 1), pv ? kTagNoisePV : kTagNoiseRot},
                                            n.k0, n.k1);
    return (k & 1) ? amx::u53(r.z, r.w) : amx::u53(r.x, r.y);
  }
};

// cMathUtil::EulerToQuaternion (util/MathUtil.cpp:347-381, 423-466)
__device__ inline Q euler_q(double x, double y, double z) {
  const double xs = sin(x), xc = cos(x), ys = sin(y), yc = cos(y), zs = sin(z), zc = cos(z);
  double c = (yc * zc + xs * ys * zs + xc * zc + xc * yc - 1) * 0.5;
  c = fmin(fmax(c, -1.0), 1.0);
  const double th = acos(c);
  V3 ax = {0.0, 0.0, 1.0};
  if (!(fabs(th) < 0.00001)) {
    const double m21 = xs * yc - xc * ys * zs + xs * zc;
    const double m02 = xc * ys * zc + xs * zs + ys;
    const double m10 = yc * zs - xs * ys * zc + xc * zs;
    const double den = sqrt(m21 * m21 + m02 * m02 + m10 * m10);
    ax = {m21 / den, m02 / den, m10 / den};
  }
  const double ch = cos(th / 2), sh = sin(th / 2);
  return {ch, sh * ax.x, sh * ax.y, sh * ax.z};
}
__device__ inline void stq(double* p, Q q) { p[0] = q.w; p[1] = q.x; p[2] = q.y; p[3] = q.z; }

// one thread, the lane's pose / vel in LDS (humanoid3d's knee / hip / ankle joint indices, as
// hard-coded in the reference, including its velocity-noise test !(j == 4 || j != 10))
__device__ void add_noise(const MView& m, double* pose, double* vel, const NoiseArgs& n, const NoiseDraws& d) {
  int kr = 0, kp = 0;
  const double r = n.radian, lo = n.lo, hi = n.hi;
  auto rnd = [&]() { return -r + d.u(kr++, false) * (r - (-r)); };
  auto pose_vel = [&]() {  // AddNoisePoseVel
    if (lo == 0 && hi == 0) return;
    for (int i = 0; i < m.D; ++i) pose[i] = pose[i] + (lo + d.u(kp++, true) * (hi - lo));
    for (int i = 0; i < m.D; ++i) vel[i] = vel[i] + (lo + d.u(kp++, true) * (hi - lo));
  };
  auto rotate = [&]() {  // RandomRotatePoseVel
    if (r == 0) return;
    const double a = rnd();
    // cCharacter::RotateRoot (Character.cpp:210-216) -> cKinCharacter::SetRootRotation ->
    // RotateOrigin(dq) (KinCharacter.cpp:259-264, 300-337): the root rotation becomes
    // normalize(dq * old) with dq = normalize(rot * old) * old^-1, and the root's linear and
    // angular velocities are rotated by dq (QuatRotVec writes the gRotDim pad slot as 0)
    const Q old = ldq(pose + 3);
    const Q nq = qnorm(qmul({cos(a / 2), 0.0, sin(a / 2), 0.0}, old));
    const Q dq = qmul(nq, {old.w, -old.x, -old.y, -old.z});
    stq(pose + 3, qnorm(qmul(dq, old)));
    const V3 rv = qrot(dq, {vel[0], vel[1], vel[2]});
    const V3 rw = qrot(dq, {vel[3], vel[4], vel[5]});
    vel[0] = rv.x; vel[1] = rv.y; vel[2] = rv.z;
    vel[3] = rw.x; vel[4] = rw.y; vel[5] = rw.z; vel[6] = 0.0;
    for (int i = 0; i < 7; ++i) vel[i] = n.interp * vel[i];  // root vel (3) + root ang vel (gRotDim 4)
    for (int j = 1; j < m.J; ++j) {
      const int o = (int)m.joints[8 * j + 2], sz = (int)m.joints[8 * j + 3];
      for (int i = 0; i < sz; ++i) vel[o + i] = n.interp * vel[o + i];
    }
    for (int j = 1; j < m.J; ++j) {
      const int t = (int)m.joints[8 * j], o = (int)m.joints[8 * j + 2];
      if (t == JT_REVOLUTE) {
        if (!(j == 4 || j == 10) || n.knee_rot) pose[o] = pose[o] + rnd();
      } else if (t == JT_SPHERICAL && j != 3 && j != 5 && j != 9 && j != 11) {
        const double ps = rnd(), th = rnd(), ph = rnd();
        const Q qr = euler_q(ps, th, ph);
        stq(pose + o, qmul(qr, ldq(pose + o)));
        if (n.rot_vel_w_pose) stq(vel + o, qmul(qr, ldq(vel + o)));
      }
    }
    if (n.vel_noise) {
      const double ps = rnd(), th = rnd(), ph = rnd();
      stq(vel + 3, qmul(euler_q(ps, th, ph), ldq(vel + 3)));
      for (int j = 1; j < m.J; ++j) {
        const int t = (int)m.joints[8 * j], o = (int)m.joints[8 * j + 2];
        if (t == JT_REVOLUTE) {
          if (!(j == 4 || j != 10) || n.knee_rot) vel[o] = vel[o] + rnd();
        } else if (t == JT_SPHERICAL && j != 3 && j != 5 && j != 9 && j != 11) {
          const double ps2 = rnd(), th2 = rnd(), ph2 = rnd();
          stq(vel + o, qmul(euler_q(ps2, th2, ph2), ldq(vel + o)));
        }
      }
    }
    stq(pose + 3, qnorm(ldq(pose + 3)));  // KinTree::PostProcessPose
    for (int j = 1; j < m.J; ++j)
      if ((int)m.joints[8 * j] == JT_SPHERICAL) {
        const int o = (int)m.joints[8 * j + 2];
        stq(pose + o, qnorm(ldq(pose + o)));
      }
  };
  if (n.bef_rot) {
    pose_vel();
    rotate();
  } else {
    rotate();
    pose_vel();
  }
}

// The recorded state at motion time `time` (see the file comment).  out: [S] = 1 + 15 J.
// Called by all 64 threads of a one-wave workgroup; thread j < J owns joint j.  The joint
// transforms are composed level by level down the tree (the parent is always done first),
// with the same per-joint arithmetic as a sequential walk, so the result does not depend on
// the thread mapping.
__device__ void motion_state(const MView& m, double time, int flags, double* __restrict__ out, MotionLds& L,
                             const NoiseArgs* noise = nullptr, int lane = 0, int rc = 0) {
  const int tid = threadIdx.x;
  const double dur = m.h[4];
  const bool loop = m.h[3] != 0.0;
  // ---- Motion::CalcIndexBlend (every thread) --------------------------------------------------
  int idx;
  double blend;
  double cycles = 0.0;
  if (!loop && time <= 0.0) {
    idx = 0; blend = 0.0;
  } else if (!loop && time >= dur) {
    idx = m.F - 2; blend = 1.0;
  } else {
    double cnt = floor(time / dur);
    if (!loop) cnt = fmin(fmax(cnt, 0.0), 1.0);
    cycles = cnt;
    const double tt = time - cnt * dur;
    // upper_bound over the sorted frame times = the number of times <= tt: counted by the
    // whole wave with independent loads (no dependent binary-search chain)
    int c = 0;
    for (int f = tid; f < m.F; f += 64) c += m.times[f] <= tt;
    c = amx::wave_sum(c);
    idx = c - 1;
    if (idx > m.F - 2) idx = m.F - 2;
    if (idx < 0) idx = 0;
    blend = (tt - m.times[idx]) / (m.times[idx + 1] - m.times[idx]);
  }
  const double lerp = fmin(fmax(blend, 0.0), 1.0);  // BlendFrames saturates
  const double* f0 = m.frames + (long long)idx * m.D;
  const double* f1 = f0 + m.D;
  const double* v0 = m.vels + (long long)idx * m.D;
  const double* v1 = v0 + m.D;
  for (int i = tid; i < m.D; i += 64) {
    L.pose[i] = (1 - lerp) * f0[i] + lerp * f1[i];
    L.vel[i] = (!loop && time >= dur) ? 0.0 : (1.0 - blend) * v0[i] + blend * v1[i];
  }
  __syncthreads();
  if (tid == 0) {
    Q q = qnorm(slerp(ldq(f0 + 3), ldq(f1 + 3), lerp));
    if (q.w < 0) q = {-q.w, -q.x, -q.y, -q.z};  // StandardizeQuat
    L.pose[3] = q.w; L.pose[4] = q.x; L.pose[5] = q.y; L.pose[6] = q.z;
    if (loop) {
      L.pose[0] += cycles * m.h[8];
      L.pose[1] += cycles * m.h[9];
      L.pose[2] += cycles * m.h[10];
    }
  } else if (tid < m.J && (int)m.joints[8 * tid] == JT_SPHERICAL) {
    const int o = (int)m.joints[8 * tid + 2];
    const Q q = slerp(ldq(f0 + o), ldq(f1 + o), lerp);
    L.pose[o] = q.w; L.pose[o + 1] = q.x; L.pose[o + 2] = q.y; L.pose[o + 3] = q.z;
  }
  __syncthreads();
  if (tid == 0) {
    if (noise && noise->on) add_noise(m, L.pose, L.vel, *noise, NoiseDraws{*noise, lane, rc});
    L.pose[0] = 0.0;  // random placement on the plane: root x, z = 0 (after the noise)
    L.pose[2] = 0.0;
  }
  __syncthreads();
  // ---- kinematics, one tree level per pass ----------------------------------------------------
  int depth = 0, max_depth = 0;
  for (int j = 1; j < m.J; ++j) {
    int d = 0;
    for (int p = j; p > 0; p = (int)m.joints[8 * p + 1]) ++d;
    if (j == tid) depth = d;
    max_depth = max(max_depth, d);
  }
  const int j = tid;
  for (int lvl = 0; lvl <= max_depth; ++lvl) {
    if (j < m.J && depth == lvl) {
      const double* jt = m.joints + 8 * j;
      const int type = (int)jt[0], par = (int)jt[1], off = (int)jt[2];
      const double* pose = L.pose;
      const double* vel = L.vel;
      if (par < 0) {
        qmat(ldq(pose + 3), L.R[j]);
        L.o[j] = {pose[0], pose[1], pose[2]};
        L.w[j] = {vel[3], vel[4], vel[5]};
        L.v[j] = {vel[0], vel[1], vel[2]};
      } else {
        L.o[j] = add(L.o[par], mv(L.R[par], {jt[4], jt[5], jt[6]}));
        double Lm[9];
        if (type == JT_SPHERICAL) {
          qmat(ldq(pose + off), Lm);
          mm(L.R[par], Lm, L.R[j]);
          L.w[j] = add(L.w[par], mv(L.R[j], {vel[off], vel[off + 1], vel[off + 2]}));
        } else if (type == JT_REVOLUTE) {
          axis_mat({0.0, 0.0, 1.0}, pose[off], Lm);
          mm(L.R[par], Lm, L.R[j]);
          L.w[j] = add(L.w[par], mv(L.R[j], {0.0, 0.0, vel[off]}));
        } else {  // fixed
          for (int k = 0; k < 9; ++k) L.R[j][k] = L.R[par][k];
          L.w[j] = L.w[par];
        }
        L.v[j] = add(L.v[par], cross(L.w[par], sub(L.o[j], L.o[par])));
      }
      const double* bd = m.bodies + 8 * j;
      L.bp[j] = add(L.o[j], mv(L.R[j], {bd[1], bd[2], bd[3]}));
    }
    __syncthreads();
  }
  // ---- ResolveCharGroundIntersect: deepest AABB violation over the bodies (fmin is exact) -----
  double viol = 0.0;
  const double pad = m.h[11];
  if (j < m.J) {
    const double* bd = m.bodies + 8 * j;
    if (bd[7] != 0.0) {
      const int sh = (int)bd[0];
      double ext;
      if (sh == SH_SPHERE) {
        ext = 0.5 * bd[4];
      } else {
        const double hx = 0.5 * bd[4], hy = sh == SH_CAPSULE ? 0.5 * bd[4] + 0.5 * bd[5] : 0.5 * bd[5];
        const double hz = sh == SH_CAPSULE ? 0.5 * bd[4] : 0.5 * bd[6];
        ext = fabs(L.R[j][3]) * hx + fabs(L.R[j][4]) * hy + fabs(L.R[j][5]) * hz;
      }
      viol = fmin(0.0, L.bp[j].y - ext - pad);
    }
  }
  // reset_args['resolve'] = False (flags & 8) skips the lift (SceneSimChar.cpp:714-716); the
  // flag is uniform over the wave, so the reduction is entered by every lane or by none
  const double min_viol = (flags & 8) ? 0.0 : wave_min(viol);
  // ---- CtController::BuildStatePose / BuildStateVel ---------------------------------------------
  double p[7];
  for (int k = 0; k < 7; ++k) p[k] = L.pose[k];
  if (min_viol < 0) p[1] += -min_viol;
  const bool world_root_pos = flags & 1, world_root_rot = flags & 2, all_world = flags & 4;
  const V3 rd = qrot(ldq(p + 3), {1.0, 0.0, 0.0});
  const double heading = atan2(-rd.z, rd.x);
  double Rh[9];
  axis_mat({0.0, 1.0, 0.0}, -heading, Rh);
  const V3 origin = {p[0], 0.0, p[2]};
  const V3 root_rel = mv(Rh, sub({p[0], p[1], p[2]}, origin));
  if (tid == 0) out[0] = root_rel.y;
  if (j < m.J) {
    const int i = j;
    V3 oi = L.o[i], bpi = L.bp[i];
    if (min_viol < 0) {
      oi.y += -min_viol;
      bpi.y += -min_viol;
    }
    const Q qh = mat_q(Rh);
    V3 pp = bpi;
    if (!all_world && (!world_root_pos || i != 0)) pp = sub(mv(Rh, sub(pp, origin)), root_rel);
    out[9 * i + 1] = pp.x; out[9 * i + 2] = pp.y; out[9 * i + 3] = pp.z;
    Q q = mat_q(L.R[i]);
    if (!all_world && (!world_root_rot || i != 0)) q = qmul(qh, q);
    const V3 nrm = qrot(q, {0.0, 1.0, 0.0}), tan = qrot(q, {1.0, 0.0, 0.0});
    out[9 * i + 4] = nrm.x; out[9 * i + 5] = nrm.y; out[9 * i + 6] = nrm.z;
    out[9 * i + 7] = tan.x; out[9 * i + 8] = tan.y; out[9 * i + 9] = tan.z;
    V3 lv = add(L.v[i], cross(L.w[i], sub(bpi, oi)));
    V3 av = L.w[i];
    if (!all_world && (!world_root_rot || i != 0)) {
      lv = mv(Rh, lv);
      av = mv(Rh, av);
    }
    double* d = out + 1 + 9 * m.J + 6 * i;
    d[0] = lv.x; d[1] = lv.y; d[2] = lv.z; d[3] = av.x; d[4] = av.y; d[5] = av.z;
  }
}

// ---- AMP observation features (scenes/SceneImitateAMP.cpp:287-475) ---------------------------
// BuildAMPObs(prev_pose, prev_vel, pose, vel): [pose part(pose), pose part(prev), vel part(vel),
// vel part(prev)], every part in the CURRENT pose's heading frame (ref_origin_rot):
//   pose part = root_h, root rotation tangent-normal (world, or heading frame with
//               enable_amp_obs_local_root), per joint: spherical -> tangent-normal of its local
//               rotation (6), revolute -> angle (1), fixed -> nothing; end-effector body
//               positions relative to the root joint (3 each)
//   vel part  = root linear / angular velocity (world, or heading frame), then the raw joint
//               velocity parameters (spherical: local angular velocity x, y, z, 0; revolute 1)
// Kinematic quantities per joint: rotation in the heading frame Rh_j, angular velocity w_j in
// the heading frame, root joint world velocity, end-effector offsets in the heading frame.
struct AmpKin {
  double R[MAXJ][9];   // joint rotations in this pose's heading frame
  double Rw0[9];       // root rotation, world
  V3 v0, w0;           // root joint linear / angular velocity, world
  double jv[MAXD];     // joint velocity parameters (vel[7:] of the KinTree layout)
  int njv;
  V3 ee[8];            // end-effector body offsets from the root joint, this heading frame
  double root_y;
  double Rh[9];        // world -> this pose's heading frame
};

__device__ inline void tn_mat(const double* nt, double* R) {  // columns tan, nrm, tan x nrm
  const V3 n = {nt[0], nt[1], nt[2]}, t = {nt[3], nt[4], nt[5]};
  const V3 z = cross(t, n);
  R[0] = t.x; R[1] = n.x; R[2] = z.x;
  R[3] = t.y; R[4] = n.y; R[5] = z.y;
  R[6] = t.z; R[7] = n.z; R[8] = z.z;
}
__device__ inline void heading_of(const double* Rw0, double* Rh) {  // KinTree::CalcHeadingRot
  const double heading = atan2(-Rw0[6], Rw0[0]);                    // R e_x = column 0
  axis_mat({0.0, 1.0, 0.0}, -heading, Rh);
}
__device__ inline V3 mtv(const double* m, V3 v) {  // m^T v
  return {m[0] * v.x + m[3] * v.y + m[6] * v.z, m[1] * v.x + m[4] * v.y + m[7] * v.z,
          m[2] * v.x + m[5] * v.y + m[8] * v.z};
}
__device__ inline void mtm(const double* a, const double* b, double* o) {  // a^T b
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o[3 * i + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}

// kinematics of a clip pose / velocity (Motion::CalcFrame / CalcFrameVel)
__device__ void kin_from_pose(const MView& m, const double* pose, const double* vel, AmpKin& k) {
  double R[MAXJ][9];
  V3 o[MAXJ];
  k.root_y = pose[1];
  qmat(ldq(pose + 3), k.Rw0);
  heading_of(k.Rw0, k.Rh);
  k.w0 = {vel[3], vel[4], vel[5]};
  k.v0 = {vel[0], vel[1], vel[2]};
  for (int q = 0; q < 9; ++q) R[0][q] = k.Rw0[q];
  o[0] = {pose[0], pose[1], pose[2]};
  for (int j = 1; j < m.J; ++j) {
    const double* jt = m.joints + 8 * j;
    const int type = (int)jt[0], par = (int)jt[1], off = (int)jt[2];
    o[j] = add(o[par], mv(R[par], {jt[4], jt[5], jt[6]}));
    double L[9];
    if (type == JT_SPHERICAL) {
      qmat(ldq(pose + off), L);
      mm(R[par], L, R[j]);
    } else if (type == JT_REVOLUTE) {
      axis_mat({0.0, 0.0, 1.0}, pose[off], L);
      mm(R[par], L, R[j]);
    } else {
      for (int q = 0; q < 9; ++q) R[j][q] = R[par][q];
    }
  }
  for (int j = 0; j < m.J; ++j) mm(k.Rh, R[j], k.R[j]);
  k.njv = m.D - 7;
  for (int i = 0; i < k.njv; ++i) k.jv[i] = vel[7 + i];
  int e = 0;
  for (int j = 0; j < m.J && e < 8; ++j)
    if (m.joints[8 * j + 7] != 0.0) {
      const double* bd = m.bodies + 8 * j;
      k.ee[e++] = mv(k.Rh, sub(add(o[j], mv(R[j], {bd[1], bd[2], bd[3]})), o[0]));
    }
}

// one pose part / one vel part; Rc = the current pose's heading rotation (ref_origin_rot)
__device__ int amp_pose_part(const MView& m, const AmpKin& k, const double* Rc, bool local_root, double* out) {
  int c = 0;
  out[c++] = k.root_y;
  double R0[9];
  if (local_root) {
    mm(Rc, k.Rw0, R0);
  } else {
    for (int q = 0; q < 9; ++q) R0[q] = k.Rw0[q];
  }
  out[c++] = R0[1]; out[c++] = R0[4]; out[c++] = R0[7];   // norm = R e_y
  out[c++] = R0[0]; out[c++] = R0[3]; out[c++] = R0[6];   // tan  = R e_x
  for (int j = 1; j < m.J; ++j) {
    const double* jt = m.joints + 8 * j;
    const int type = (int)jt[0], par = (int)jt[1];
    if (type == JT_SPHERICAL || type == JT_REVOLUTE) {
      double L[9];
      mtm(k.R[par], k.R[j], L);
      if (type == JT_SPHERICAL) {
        out[c++] = L[1]; out[c++] = L[4]; out[c++] = L[7];
        out[c++] = L[0]; out[c++] = L[3]; out[c++] = L[6];
      } else {
        out[c++] = atan2(L[3], L[0]);
      }
    }
  }
  // end effectors: this pose's heading-frame offsets re-expressed in the current heading
  // frame (Rc Rh^T)
  double Rx[9];
  for (int i = 0; i < 3; ++i)
    for (int jj = 0; jj < 3; ++jj)
      Rx[3 * i + jj] = Rc[3 * i] * k.Rh[3 * jj] + Rc[3 * i + 1] * k.Rh[3 * jj + 1] + Rc[3 * i + 2] * k.Rh[3 * jj + 2];
  int e = 0;
  for (int j = 0; j < m.J && e < 8; ++j)
    if (m.joints[8 * j + 7] != 0.0) {
      const V3 p = mv(Rx, k.ee[e++]);
      out[c++] = p.x; out[c++] = p.y; out[c++] = p.z;
    }
  return c;
}

__device__ int amp_vel_part(const AmpKin& k, const double* Rc, bool local_root, double* out) {
  int c = 0;
  V3 v = k.v0, w = k.w0;
  if (local_root) {
    v = mv(Rc, v);
    w = mv(Rc, w);
  }
  out[c++] = v.x; out[c++] = v.y; out[c++] = v.z;
  out[c++] = w.x; out[c++] = w.y; out[c++] = w.z;
  for (int i = 0; i < k.njv; ++i) out[c++] = k.jv[i];
  return c;
}

__device__ void amp_obs(const MView& m, const AmpKin& prev, const AmpKin& cur, bool local_root, double* out) {
  int c = 0;
  c += amp_pose_part(m, cur, cur.Rh, local_root, out + c);
  c += amp_pose_part(m, prev, cur.Rh, local_root, out + c);
  c += amp_vel_part(cur, cur.Rh, local_root, out + c);
  c += amp_vel_part(prev, cur.Rh, local_root, out + c);
}

// raw clip frame and velocity at `time` (Motion::CalcFrame / CalcFrameVel)
__device__ void clip_frame(const MView& m, double time, double* pose, double* vel) {
  const double dur = m.h[4];
  const bool loop = m.h[3] != 0.0;
  int idx;
  double blend;
  if (!loop && time <= 0.0) {
    idx = 0; blend = 0.0;
  } else if (!loop && time >= dur) {
    idx = m.F - 2; blend = 1.0;
  } else {
    double cnt = floor(time / dur);
    if (!loop) cnt = fmin(fmax(cnt, 0.0), 1.0);
    const double tt = time - cnt * dur;
    int lo = 0, hi = m.F;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (m.times[mid] <= tt) lo = mid + 1; else hi = mid;
    }
    idx = min(max(lo - 1, 0), m.F - 2);
    blend = (tt - m.times[idx]) / (m.times[idx + 1] - m.times[idx]);
  }
  const double lerp = fmin(fmax(blend, 0.0), 1.0);
  const double* f0 = m.frames + (long long)idx * m.D;
  const double* f1 = f0 + m.D;
  const double* v0 = m.vels + (long long)idx * m.D;
  const double* v1 = v0 + m.D;
  for (int i = 0; i < m.D; ++i) {
    pose[i] = (1 - lerp) * f0[i] + lerp * f1[i];
    vel[i] = (!loop && time >= dur) ? 0.0 : (1.0 - blend) * v0[i] + blend * v1[i];
  }
  const Q q = qnorm(slerp(ldq(f0 + 3), ldq(f1 + 3), lerp));
  pose[3] = q.w; pose[4] = q.x; pose[5] = q.y; pose[6] = q.z;
  for (int j = 1; j < m.J; ++j) {
    const double* jt = m.joints + 8 * j;
    if ((int)jt[0] == JT_SPHERICAL) {
      const int o = (int)jt[2];
      const Q r = slerp(ldq(f0 + o), ldq(f1 + o), lerp);
      pose[o] = r.w; pose[o + 1] = r.x; pose[o + 2] = r.y; pose[o + 3] = r.z;
    }
  }
}

// AMP features of (s_prev, s_cur) rows from the recorded states (CtController layout with
// the root rotation and root velocities in the world frame, RecordWorldRootRot): rotations
// from the tangent-normal pairs (R = [tan, nrm, tan x nrm]), joint velocity parameters from
// the body angular velocities (spherical: R_j^T (w_j - w_parent), revolute: its z component),
// end effectors from the body positions; then the parts of amp_obs.  16 threads per row
// (thread j: joint / body j), four rows per 64-thread workgroup.
// T = double: out row = the features (ldo >= size); T = float: the fp32 cost-input row,
// zero-padded up to ldo.
struct AmpLds {
  double R[2][MAXJ][9];  // [prev, cur] joint rotations (root: heading frame)
  V3 w[2][MAXJ];         // body angular velocities (root: heading frame)
};

template <typename T>
__global__ __launch_bounds__(64) void k_state_amp_obs(const double* __restrict__ blob, const double* __restrict__ sp,
                                                      const double* __restrict__ sc, long long lds, int B,
                                                      int local_root, T* __restrict__ out, long long ldo) {
  __shared__ AmpLds Ls[4];
  __shared__ double hdr[HDR], jtab[8 * MAXJ], btab[8 * MAXJ];
  const int g = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int b = blockIdx.x * 4 + g;
  const bool valid = b < B;
  AmpLds& L = Ls[g];
  const MView m = stage_tables(blob, hdr, jtab, btab);
  const int n = m.J;
  const double* st[2] = {sp + (long long)(valid ? b : 0) * lds, sc + (long long)(valid ? b : 0) * lds};
  const int base = 1 + 9 * n;
  double Rw0[2][9], Rh[2][9];
  for (int k = 0; k < 2; ++k) {
    tn_mat(st[k] + 4, Rw0[k]);
    heading_of(Rw0[k], Rh[k]);
  }
  if (valid && j < n) {
    for (int k = 0; k < 2; ++k) {
      const double* s = st[k];
      if (j == 0) {
        mm(Rh[k], Rw0[k], L.R[k][0]);
        L.w[k][0] = mv(Rh[k], {s[base + 3], s[base + 4], s[base + 5]});
      } else {
        tn_mat(s + 9 * j + 4, L.R[k][j]);
        L.w[k][j] = {s[base + 6 * j + 3], s[base + 6 * j + 4], s[base + 6 * j + 5]};
      }
    }
  }
  __syncthreads();
  if (!valid) return;
  // output offsets (SceneImitateAMP::GetAMPObsSize order)
  int pw = 0, vw = 0, pj = 0, vj = 0, ne = 0, ej = -1;
  for (int i = 1; i < n; ++i) {
    const int type = (int)m.joints[8 * i];
    if (i == j) { pj = pw; vj = vw; }
    if (type == JT_SPHERICAL) { pw += 6; vw += 4; }
    else if (type == JT_REVOLUTE) { pw += 1; vw += 1; }
  }
  for (int i = 0; i < n && ne < 8; ++i)
    if (m.joints[8 * i + 7] != 0.0) {
      if (i == j) ej = ne;
      ++ne;
    }
  const int P = 7 + pw + 3 * ne, V = 6 + vw, D = 2 * P + 2 * V;
  T* o = out + (long long)b * ldo;
  const double* Rc = Rh[1];
  for (int k = 0; k < 2; ++k) {   // k = 1: current (first part), k = 0: previous
    const double* s = st[k];
    T* po = o + (k == 1 ? 0 : P);
    T* vo = o + 2 * P + (k == 1 ? 0 : V);
    if (j == 0) {
      double R0[9];
      if (local_root) {
        mm(Rc, Rw0[k], R0);
      } else {
        for (int q = 0; q < 9; ++q) R0[q] = Rw0[k][q];
      }
      po[0] = (T)s[0];
      po[1] = (T)R0[1]; po[2] = (T)R0[4]; po[3] = (T)R0[7];
      po[4] = (T)R0[0]; po[5] = (T)R0[3]; po[6] = (T)R0[6];
      // root joint velocity: body-0 velocity minus w0 x (body-0 offset, back in the world frame)
      const V3 w0 = {s[base + 3], s[base + 4], s[base + 5]};
      const V3 off = mtv(Rh[k], {s[1], s[2], s[3]});
      V3 v = sub({s[base], s[base + 1], s[base + 2]}, cross(w0, off)), w = w0;
      if (local_root) {
        v = mv(Rc, v);
        w = mv(Rc, w);
      }
      vo[0] = (T)v.x; vo[1] = (T)v.y; vo[2] = (T)v.z; vo[3] = (T)w.x; vo[4] = (T)w.y; vo[5] = (T)w.z;
    } else if (j < n) {
      const int type = (int)m.joints[8 * j], par = (int)m.joints[8 * j + 1];
      if (type == JT_SPHERICAL || type == JT_REVOLUTE) {
        double Lm[9];
        mtm(L.R[k][par], L.R[k][j], Lm);
        const V3 wl = mtv(L.R[k][j], sub(L.w[k][j], L.w[k][par]));
        T* q = po + 7 + pj;
        T* u = vo + 6 + vj;
        if (type == JT_SPHERICAL) {
          q[0] = (T)Lm[1]; q[1] = (T)Lm[4]; q[2] = (T)Lm[7]; q[3] = (T)Lm[0]; q[4] = (T)Lm[3]; q[5] = (T)Lm[6];
          u[0] = (T)wl.x; u[1] = (T)wl.y; u[2] = (T)wl.z; u[3] = (T)0.0;
        } else {
          q[0] = (T)atan2(Lm[3], Lm[0]);
          u[0] = (T)wl.z;
        }
      }
    }
    if (ej >= 0) {  // end effector: this state's heading-frame offset in the current heading frame
      double Rx[9];
      for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c)
          Rx[3 * a + c] = Rc[3 * a] * Rh[k][3 * c] + Rc[3 * a + 1] * Rh[k][3 * c + 1] + Rc[3 * a + 2] * Rh[k][3 * c + 2];
      const V3 e = mv(Rx, {s[9 * j + 1], s[9 * j + 2], s[9 * j + 3]});
      T* q = po + 7 + pw + 3 * ej;
      q[0] = (T)e.x; q[1] = (T)e.y; q[2] = (T)e.z;
    }
  }
  if constexpr (sizeof(T) == 4)
    for (long long c = D + j; c < ldo; c += 16) o[c] = (T)0;
}

__global__ __launch_bounds__(64) void k_motion_amp_obs(const double* __restrict__ blob, const double* __restrict__ times,
                                                       double dt, int B, int local_root, double* __restrict__ out,
                                                       long long ldo) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const MView m(blob);
  double pose[MAXD], vel[MAXD];
  AmpKin kp, kc;
  clip_frame(m, times[b] - dt, pose, vel);
  kin_from_pose(m, pose, vel, kp);
  clip_frame(m, times[b], pose, vel);
  kin_from_pose(m, pose, vel, kc);
  amp_obs(m, kp, kc, local_root != 0, out + (long long)b * ldo);
}

// ---- time-warp rows (cSceneImitateAMP::BuildTimeWarpData, scenes/SceneImitateAMP.cpp:537-555) --
// row = [(0, root_y, 0), joint_j world position - root joint world position for j >= 1]: what
// the DTW evaluation compares between the simulated and the kinematic character (amx_dtw.hip).
//
// From a recorded state (RecordWorldRootRot): the state holds the body positions in the heading
// frame relative to the root joint, pp_j = Rh (o_j + R_j attach_body_j - o_0), and the body
// rotations R^h_j = Rh R_j as tangent-normal pairs, so o_j - o_0 = Rh^T (pp_j - R^h_j attach_body_j).
// 16 threads per row (thread j: joint j), four rows per workgroup, as k_state_amp_obs.
__global__ __launch_bounds__(64) void k_state_tw_rows(const double* __restrict__ blob, const double* __restrict__ st,
                                                      long long lds, int B, double* __restrict__ out, long long ldo) {
  __shared__ double hdr[HDR], jtab[8 * MAXJ], btab[8 * MAXJ];
  const int j = threadIdx.x & 15;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 4);
  const MView m = stage_tables(blob, hdr, jtab, btab);
  if (b >= B || j >= m.J) return;
  const double* s = st + (long long)b * lds;
  double* o = out + (long long)b * ldo;
  if (j == 0) {
    o[0] = 0.0; o[1] = s[0]; o[2] = 0.0;
    return;
  }
  double Rw0[9], Rh[9], Rj[9];
  tn_mat(s + 4, Rw0);
  heading_of(Rw0, Rh);
  tn_mat(s + 9 * j + 4, Rj);
  const double* bd = m.bodies + 8 * j;
  const V3 d = mtv(Rh, sub({s[9 * j + 1], s[9 * j + 2], s[9 * j + 3]}, mv(Rj, {bd[1], bd[2], bd[3]})));
  o[3 * j] = d.x; o[3 * j + 1] = d.y; o[3 * j + 2] = d.z;
}

// From the clip: row i of trajectory t is the kinematic character at t0[t] + i / update_rate,
// the pose of the reset path (clip_frame + the loop's cycle offset, as motion_state), its joint
// origins as kin_from_pose walks them; root height = the clip's + lift[t] (SyncKinCharRoot copies
// the ground-resolved root position to the kinematic character, scenes/SceneImitate.cpp:550-582)
// until a looping clip starts its next cycle: SyncKinCharNewCycle (:400-412, 594-607) then puts
// the root back at ground height + the clip's height over its origin, which on the plane drops
// the lift for the rest of the episode.  One thread per row.
__global__ __launch_bounds__(64) void k_motion_tw_rows(const double* __restrict__ blob, const double* __restrict__ t0,
                                                       const double* __restrict__ lift, int T, int n, double rate,
                                                       double* __restrict__ out, long long ldo) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= (long long)T * n) return;
  const int t = (int)(r / n), i = (int)(r % n);
  const MView m(blob);
  const double time = t0[t] + i / rate;
  double pose[MAXD], vel[MAXD];
  clip_frame(m, time, pose, vel);
  double root_y = pose[1];
  if (m.h[3] != 0.0) root_y += floor(time / m.h[4]) * m.h[9];
  if (lift && (m.h[3] == 0.0 || floor(time / m.h[4]) == floor(t0[t] / m.h[4]))) root_y += lift[t];
  double R[MAXJ][9];
  V3 o[MAXJ];
  qmat(ldq(pose + 3), R[0]);
  o[0] = {pose[0], pose[1], pose[2]};
  double* q = out + r * ldo;
  q[0] = 0.0; q[1] = root_y; q[2] = 0.0;
  for (int j = 1; j < m.J; ++j) {
    const double* jt = m.joints + 8 * j;
    const int type = (int)jt[0], par = (int)jt[1], off = (int)jt[2];
    o[j] = add(o[par], mv(R[par], {jt[4], jt[5], jt[6]}));
    double L[9];
    if (type == JT_SPHERICAL) {
      qmat(ldq(pose + off), L);
      mm(R[par], L, R[j]);
    } else if (type == JT_REVOLUTE) {
      axis_mat({0.0, 0.0, 1.0}, pose[off], L);
      mm(R[par], L, R[j]);
    } else {
      for (int k = 0; k < 9; ++k) R[j][k] = R[par][k];
    }
    const V3 d = sub(o[j], o[0]);
    q[3 * j] = d.x; q[3 * j + 1] = d.y; q[3 * j + 2] = d.z;
  }
}

// one 64-thread workgroup per lane (motion_state)
__global__ __launch_bounds__(64) void k_motion_states(const double* __restrict__ blob, const double* __restrict__ times,
                                                      int B, int flags, double* __restrict__ ob, long long ldo,
                                                      NoiseArgs noise) {
  __shared__ MotionLds L;
  const int b = blockIdx.x;
  if (b >= B) return;
  const MView m = stage_tables(blob, L.hdr, L.jt, L.bt);
  motion_state(m, times[b], flags, ob + (long long)b * ldo, L, &noise, b, 0);
}

// SimEnv.reset on masked lanes with motion states: reset_count/model_idx/num_steps as in
// k_reset (sim_env.py:277, 282-283); t = times[b] or uniform(0, duration) from
// Philox(seed, lane, reset#) (np_random.uniform(low=0, high=time_max), :276; time_max = the
// clip length, or reset_args['time_max'] with custom_time, :77).
__global__ __launch_bounds__(64) void k_reset_motion(const double* __restrict__ blob, const uint8_t* __restrict__ mask,
                                                     const double* __restrict__ times, uint32_t k0, uint32_t k1,
                                                     double tmax, int flags, const double* ob_src, double* ob_out,
                                                     int32_t* num_steps, int32_t* model_idx, int32_t* reset_count,
                                                     double* t_out, int S, int M, int B, NoiseArgs noise) {
  __shared__ MotionLds L;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= B) return;
  const bool do_reset = (mask == nullptr) || mask[b] != 0;
  if (!do_reset) {  // carried lane: coalesced row copy
    if (ob_src != ob_out)
      for (int j = tid; j < S; j += 64) ob_out[(long long)b * S + j] = ob_src[(long long)b * S + j];
    if (t_out && tid == 0) t_out[b] = -1.0;
    return;
  }
  const MView m = stage_tables(blob, L.hdr, L.jt, L.bt);
  const int rc = reset_count[b] + 1;
  double t;
  if (times) {
    t = times[b];
  } else {
    const amx::u32x4 r = amx::philox4x32_10({(uint32_t)b, (uint32_t)rc, 0u, amx::kTagMotion}, k0, k1);
    t = 0.0 + (tmax - 0.0) * amx::u53(r.x, r.y);
  }
  motion_state(m, t, flags, ob_out + (long long)b * S, L, &noise, b, rc);
  if (tid == 0) {
    reset_count[b] = rc;
    model_idx[b] = rc % M;
    num_steps[b] = 0;
    if (t_out) t_out[b] = t;
  }
}

}  // namespace

extern "C" int amx_set_motion(amx_ctx* c, const double* blob, long long n) {
  AMX_CHECK_ARG(c && blob && n > HDR, "amx_set_motion: null ctx/blob or n=%lld", n);
  const int J = (int)blob[0], D = (int)blob[1], F = (int)blob[2];
  AMX_CHECK_ARG(J > 0 && J <= MAXJ && D > 7 && D <= MAXD && F >= 2, "amx_set_motion: J=%d (<= %d) D=%d (<= %d) F=%d",
                J, MAXJ, D, MAXD, F);
  AMX_CHECK_ARG(n == HDR + 16LL * J + F + 2LL * F * D, "amx_set_motion: blob has %lld doubles, expected %lld", n,
                HDR + 16LL * J + F + 2LL * F * D);
  AMX_CHECK_ARG(c->S == 1 + 15 * J, "amx_set_motion: state size S=%d != 1 + 15*J (%d)", c->S, 1 + 15 * J);
  AMX_CHECK_ARG(blob[4] > 0.0, "amx_set_motion: duration %g", blob[4]);
  for (int j = 0; j < J; ++j) {
    const double* jt = blob + HDR + 8 * j;
    const int type = (int)jt[0], par = (int)jt[1], off = (int)jt[2];
    AMX_CHECK_ARG((j == 0) == (par < 0) && par < j, "amx_set_motion: joint %d parent %d (joints must be ordered)", j,
                  par);
    AMX_CHECK_ARG(type == JT_REVOLUTE || type == JT_FIXED || type == JT_SPHERICAL || (j == 0 && type == JT_ROOT),
                  "amx_set_motion: joint %d type %d unsupported", j, type);
    AMX_CHECK_ARG(off >= 0 && off + (int)jt[3] <= D, "amx_set_motion: joint %d params past the frame", j);
  }
  AMX_CHECK_HIP(hipSetDevice(c->device));
  if (c->d_motion && c->motion_n != n) {
    AMX_CHECK_HIP(hipFree(c->d_motion));
    c->d_motion = nullptr;
  }
  if (!c->d_motion) {
    if (hipMalloc((void**)&c->d_motion, sizeof(double) * n) != hipSuccess) {
      amx::set_error("amx_set_motion: hipMalloc failed");
      return AMX_E_NOMEM;
    }
  }
  AMX_CHECK_HIP(hipMemcpy(c->d_motion, blob, sizeof(double) * n, hipMemcpyHostToDevice));
  c->motion_n = n;
  c->motion_J = J;
  c->motion_D = D;
  c->motion_F = F;
  c->motion_duration = blob[4];
  // SceneImitateAMP::GetAMPObsSize (scenes/SceneImitateAMP.cpp:101-110, 287-330)
  int pose = 1 + 6, vel = 6, ee = 0;
  for (int j = 1; j < J; ++j) {
    const double* jt = blob + HDR + 8 * j;
    const int type = (int)jt[0];
    pose += type == JT_SPHERICAL ? 6 : (int)jt[3];
    vel += (int)jt[3];
  }
  for (int j = 0; j < J; ++j) ee += blob[HDR + 8 * j + 7] != 0.0;
  AMX_CHECK_ARG(ee <= 8, "amx_set_motion: %d end effectors (max 8)", ee);
  c->amp_obs_size = 2 * (pose + 3 * ee) + 2 * vel;
  return AMX_OK;
}

extern "C" double amx_motion_duration(const amx_ctx* c) { return (c && c->d_motion) ? c->motion_duration : -1.0; }

namespace {
// NoiseArgs of a launch (no noise when `noise` is null or all its amounts are zero)
int noise_args(const char* fn, const amx_ctx* c, const amx_reset_noise* noise, const double* draws, long long ld,
               uint64_t seed, NoiseArgs& n) {
  n = NoiseArgs{};
  if (!noise) return AMX_OK;
  AMX_CHECK_ARG(noise->radian == noise->radian && noise->noise_min == noise->noise_min &&
                    noise->noise_max == noise->noise_max && noise->interp == noise->interp,
                "%s: NaN in the reset noise", fn);
  n.on = noise->radian != 0.0 || noise->noise_min != 0.0 || noise->noise_max != 0.0;
  n.bef_rot = noise->noise_bef_rot != 0;
  n.rot_vel_w_pose = noise->rot_vel_w_pose != 0;
  n.vel_noise = noise->vel_noise != 0;
  n.knee_rot = noise->knee_rot != 0;
  n.lo = noise->noise_min;
  n.hi = noise->noise_max;
  n.radian = noise->radian;
  n.interp = noise->interp;
  n.k0 = (uint32_t)seed;
  n.k1 = (uint32_t)(seed >> 32);
  AMX_CHECK_ARG(!draws || ld >= AMX_NOISE_ROT_SLOTS + 2LL * c->motion_D,
                "%s: injected draws need ld >= %d + 2 D = %lld", fn, AMX_NOISE_ROT_SLOTS,
                AMX_NOISE_ROT_SLOTS + 2LL * c->motion_D);
  n.draws = draws;
  n.ld = ld;
  return AMX_OK;
}
}  // namespace

extern "C" int amx_motion_states_noise(amx_ctx* c, const double* times, int B, int flags, const amx_reset_noise* noise,
                                       const double* draws, long long ld_draws, uint64_t seed, double* ob,
                                       long long ldo, void* stream) {
  AMX_CHECK_ARG(c && c->d_motion, "amx_motion_states: no motion set (amx_set_motion)");
  AMX_CHECK_ARG(times && ob && B >= 0 && ldo >= c->S, "amx_motion_states: bad arguments");
  NoiseArgs n;
  int rc = noise_args("amx_motion_states_noise", c, noise, draws, ld_draws, seed, n);
  if (rc) return rc;
  if (B == 0) return AMX_OK;
  hipLaunchKernelGGL(k_motion_states, dim3(B), dim3(64), 0, (hipStream_t)stream, c->d_motion, times, B,
                     flags, ob, ldo, n);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

extern "C" int amx_motion_states(amx_ctx* c, const double* times, int B, int flags, double* ob, long long ldo,
                                 void* stream) {
  return amx_motion_states_noise(c, times, B, flags, nullptr, nullptr, 0, 0, ob, ldo, stream);
}

extern "C" int amx_reset_lanes_motion_noise(amx_ctx* c, const uint8_t* mask, const double* times, uint64_t seed,
                                            double time_max, int flags, const amx_reset_noise* noise,
                                            const double* draws, long long ld_draws, const double* ob_src,
                                            double* ob_out, int32_t* num_steps, int32_t* model_idx,
                                            int32_t* reset_count, double* t_out, int B, void* stream) {
  AMX_CHECK_ARG(c && c->d_motion, "amx_reset_lanes_motion: no motion set (amx_set_motion)");
  AMX_CHECK_ARG(ob_out && num_steps && model_idx && reset_count && B >= 0, "amx_reset_lanes_motion: null pointer");
  AMX_CHECK_ARG(mask == nullptr || ob_src != nullptr, "amx_reset_lanes_motion: masked reset needs ob_src");
  AMX_CHECK_ARG(time_max == time_max, "amx_reset_lanes_motion: time_max is NaN");
  NoiseArgs n;
  // the noise stream's key: the lane seed with the high word flipped (the reset-time draw uses the seed itself)
  int rc = noise_args("amx_reset_lanes_motion_noise", c, noise, draws, ld_draws, seed ^ 0x9E3779B97F4A7C15ull, n);
  if (rc) return rc;
  if (B == 0) return AMX_OK;
  hipLaunchKernelGGL(k_reset_motion, dim3(B), dim3(64), 0, (hipStream_t)stream, c->d_motion, mask, times,
                     (uint32_t)seed, (uint32_t)(seed >> 32), time_max > 0.0 ? time_max : c->motion_duration, flags, ob_src, ob_out, num_steps, model_idx,
                     reset_count, t_out, c->S, c->M, B, n);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

extern "C" int amx_reset_lanes_motion(amx_ctx* c, const uint8_t* mask, const double* times, uint64_t seed,
                                      double time_max, int flags, const double* ob_src, double* ob_out, int32_t* num_steps,
                                      int32_t* model_idx, int32_t* reset_count, double* t_out, int B, void* stream) {
  return amx_reset_lanes_motion_noise(c, mask, times, seed, time_max, flags, nullptr, nullptr, 0, ob_src, ob_out,
                                      num_steps, model_idx, reset_count, t_out, B, stream);
}

// ---- AMP observation features ----------------------------------------------------------------
extern "C" int amx_amp_obs_size(const amx_ctx* c) {
  if (!c || !c->d_motion) return -1;
  return c->amp_obs_size;
}

extern "C" int amx_state_amp_obs(amx_ctx* c, const double* s_prev, const double* s_cur, long long lds, int B,
                                 int local_root, double* out, long long ldo, void* stream) {
  AMX_CHECK_ARG(c && c->d_motion, "amx_state_amp_obs: no character set (amx_set_motion)");
  AMX_CHECK_ARG(s_prev && s_cur && out && B >= 0 && lds >= c->S && ldo >= c->amp_obs_size,
                "amx_state_amp_obs: bad arguments (lds=%lld ldo=%lld)", lds, ldo);
  if (B == 0) return AMX_OK;
  hipLaunchKernelGGL(k_state_amp_obs<double>, dim3((B + 3) / 4), dim3(64), 0, (hipStream_t)stream, c->d_motion,
                     s_prev, s_cur, lds, B, local_root, out, ldo);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

extern "C" int amx_state_amp_rows(amx_ctx* c, const double* s_prev, const double* s_cur, long long lds, int B,
                                  int local_root, float* out, long long ldo, void* stream) {
  AMX_CHECK_ARG(c && c->d_motion, "amx_state_amp_rows: no character set (amx_set_motion)");
  AMX_CHECK_ARG(s_prev && s_cur && out && B >= 0 && lds >= c->S && ldo >= c->amp_obs_size,
                "amx_state_amp_rows: bad arguments (lds=%lld ldo=%lld)", lds, ldo);
  if (B == 0) return AMX_OK;
  hipLaunchKernelGGL(k_state_amp_obs<float>, dim3((B + 3) / 4), dim3(64), 0, (hipStream_t)stream, c->d_motion,
                     s_prev, s_cur, lds, B, local_root, out, ldo);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

extern "C" int amx_motion_amp_obs(amx_ctx* c, const double* times, double dt, int B, int local_root, double* out,
                                  long long ldo, void* stream) {
  AMX_CHECK_ARG(c && c->d_motion, "amx_motion_amp_obs: no motion set (amx_set_motion)");
  AMX_CHECK_ARG(times && out && B >= 0 && ldo >= c->amp_obs_size, "amx_motion_amp_obs: bad arguments");
  if (B == 0) return AMX_OK;
  hipLaunchKernelGGL(k_motion_amp_obs, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, c->d_motion, times,
                     dt, B, local_root, out, ldo);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

// ---- time-warp rows ---------------------------------------------------------------------------
extern "C" int amx_tw_dim(const amx_ctx* c) { return (c && c->d_motion) ? 3 * c->motion_J : -1; }

extern "C" int amx_state_tw_rows(amx_ctx* c, const double* s, long long lds, int B, int flags, double* out,
                                 long long ldo, void* stream) {
  AMX_CHECK_ARG(c && c->d_motion, "amx_state_tw_rows: no character set (amx_set_motion)");
  AMX_CHECK_ARG(flags == 2, "amx_state_tw_rows: record flags %d; the rows need RecordWorldRootRot only (2)", flags);
  AMX_CHECK_ARG(s && out && B >= 0 && lds >= c->S && ldo >= 3 * c->motion_J,
                "amx_state_tw_rows: bad arguments (lds=%lld ldo=%lld)", lds, ldo);
  if (B == 0) return AMX_OK;
  hipLaunchKernelGGL(k_state_tw_rows, dim3((B + 3) / 4), dim3(64), 0, (hipStream_t)stream, c->d_motion, s, lds, B, out,
                     ldo);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}

extern "C" int amx_motion_tw_rows(amx_ctx* c, const double* t0, const double* lift, int T, int n, double update_rate,
                                  double* out, long long ldo, void* stream) {
  AMX_CHECK_ARG(c && c->d_motion, "amx_motion_tw_rows: no motion set (amx_set_motion)");
  AMX_CHECK_ARG(t0 && out && T >= 0 && n >= 0 && ldo >= 3 * c->motion_J && update_rate > 0.0,
                "amx_motion_tw_rows: bad arguments (T=%d n=%d ldo=%lld update_rate=%g)", T, n, ldo, update_rate);
  const long long rows = (long long)T * n;
  AMX_CHECK_ARG(rows <= 0x7FFFFFFFLL / 64, "amx_motion_tw_rows: %lld rows", rows);
  if (rows == 0) return AMX_OK;
  hipLaunchKernelGGL(k_motion_tw_rows, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                     c->d_motion, t0, lift, T, n, update_rate, out, ldo);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}
