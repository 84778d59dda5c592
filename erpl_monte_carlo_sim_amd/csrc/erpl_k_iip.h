// erpl_k_iip.h — kernels 5 to 7 (gate build only): the instantaneous impact points of every captured trajectory of a batch
// (erpl_mc_impact_points).  The prefix kernel marks the nodes that lie below the usable prefix.  The fall kernel runs one
// lane per (node, trajectory) job: the state of the node's record falls under gravity, zero-incidence power-off drag and
// the sample's own wind - the gate's device functions, no contraction - by classic RK4 until it crosses the ground plane.
// The summary kernel reduces a trajectory's nodes under the total order of erpl_k_envelope.h (env_better / env_take), one
// wave per trajectory.  No kernel has atomics or cross-lane arithmetic in a value: the bytes of a column depend on the
// trajectory's own records and its sample's parameters alone, whatever else shares its wave, workgroup or launch.
//
// Every loop is bounded: the fall by max_steps (and it leaves at the first non-finite entry, tested explicitly, so a NaN
// never keeps a lane running), the prefix scan by the records a node can sit on, the table searches as in erpl_k_lookup.h.
namespace {

constexpr int kIipBlock = 64;   // one wave per workgroup: a wave's slot frees when its own slowest lane has landed

// what follows the thrust's end at one state: d/dt of (x, y, z, vx, vy, vz)
__device__ __forceinline__ void iip_rhs(const Shared& C, int64_t id, WindCache& wc, MachCache& mc, real mass, real cg,
                                        real drag_scale, const real (&s)[6], real (&ds)[6]) {
  const ErplScalars<real>& S = *C.S;
  real T, P;
  atmosphere(S, s[2], T, P);
  const real rho = m_div(P, S.Rg * T);
  const real g = gravity_at(S, s[2]);
  real w[3];
  wind_at(C, id, s[2], wc, w);
  const real vr0 = s[3] - w[0], vr1 = s[4] - w[1], vr2 = s[5] - w[2];
  const real vn = m_sqrt((vr0 * vr0 + vr1 * vr1) + vr2 * vr2);
  const real mach = vn / m_sqrt((real)(1.4 * 287.053) * T);
  mach_lookup(C, mach, mc);
  real cd, cl, cy, cm, cyaw, cp_dyn;
  aero_coefficients(S, mach_rec_of(C, mc), mach, (real)0, (real)0, cg, false, cd, cl, cy, cm, cyaw, cp_dyn);
  cd = cd * drag_scale;
  const real k = (((((real)0.5 * rho) * vn) * cd) * S.ref_area) / mass;
  ds[0] = s[3]; ds[1] = s[4]; ds[2] = s[5];
  ds[3] = -k * vr0; ds[4] = -k * vr1; ds[5] = -k * vr2 - g;
}

__device__ __forceinline__ bool iip_finite6(const real (&s)[6]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) ok = ok && __builtin_isfinite(s[c]);
  return ok;
}

// The fall: grid (ceil(n_traj / 64), n_nodes), a wave holds 64 neighbouring trajectories at one node (they fall for about
// the same time and read the [k][3][n] wind table coalesced; the other order measured slower).
__global__ __launch_bounds__(kIipBlock) void erpl_iip_fall_f64(const ErplKArgs a, const ErplScalars<real> S,
                                                                const ErplIipArgs q) {
  __shared__ LdsTables L;
  extern __shared__ real iip_alt[];   // the wind altitude grid: max(k_wind, 1) values
  stage_tables(L, iip_alt, a.tables, a.alt_grid, a.k_wind);   // (ends in a barrier)
  const int64_t j = (int64_t)blockIdx.x * kIipBlock + threadIdx.x;
  const int64_t k = (int64_t)blockIdx.y;
  if (j >= a.n_traj || k >= q.n_nodes) return;
  double out[ERPL_IIP_CH_COUNT];
#pragma unroll
  for (int c = 0; c < ERPL_IIP_CH_COUNT; ++c) out[c] = (double)NAN;
  const int64_t rk = k * (int64_t)q.record_stride;
  const double* __restrict__ recs = a.traj + j * a.traj_cap * ERPL_TRAJ_DIM;
  // evaluated iff rk < u: the prefix kernel left 1.0 in the node's own X slot if it is, NaN if not (no other lane reads or
  // writes that slot, so the hand-over through the caller's matrix needs no ordering beyond the stream's)
  const bool evaluated = q.values[((int64_t)ERPL_IIP_CH_X * q.n_nodes + k) * q.ld + q.col0 + j] == 1.0;
  if (evaluated) {
    const double* rec = recs + rk * ERPL_TRAJ_DIM;
    real s[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c] = rec[1 + c];
    const real speed = m_sqrt((s[3] * s[3] + s[4] * s[4]) + s[5] * s[5]);
    if (speed <= (real)1e6 && s[2] >= (real)-1e5) {   // of physical size (the hand-over thresholds of erpl_k_config.h)
      bool landed = false;
      if (s[2] <= q.ground) {
        out[ERPL_IIP_CH_X] = s[0]; out[ERPL_IIP_CH_Y] = s[1];
        out[ERPL_IIP_CH_TFALL] = 0.0; out[ERPL_IIP_CH_VIMPACT] = speed;
        landed = true;
      } else {
        Shared C;
        C.S = &S; C.L = &L; C.alt = iip_alt; C.has_wind = a.k_wind > 0; C.motor_kind = a.motor_kind;
        const int64_t id = a.traj_ids[j];
        LaneParams p;
        lane_params_of(a, S, id, p);
        const real pf = rec[14];
        real mass, cg, Ixx, Iyy;
        mass_props(S, p, (pf > 0) ? pf : (real)0, mass, cg, Ixx, Iyy);   // frozen: thrust has ended, nothing burns
        WindCache wc;
        wc.lo = 1; wc.hi = 0; wc.x0 = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { wc.y0[c] = 0; wc.s[c] = 0; }
        MachCache mc;
        mach_cache_clear(mc);
        const real dt = q.dt, h2 = (real)0.5 * q.dt, h6 = q.dt / (real)6.0;
        for (int n = 0; n < q.max_steps; ++n) {
          real k1[6], k2[6], k3[6], k4[6], y[6], sn[6];
          iip_rhs(C, id, wc, mc, mass, cg, q.drag_scale, s, k1);
#pragma unroll
          for (int c = 0; c < 6; ++c) y[c] = s[c] + h2 * k1[c];
          iip_rhs(C, id, wc, mc, mass, cg, q.drag_scale, y, k2);
#pragma unroll
          for (int c = 0; c < 6; ++c) y[c] = s[c] + h2 * k2[c];
          iip_rhs(C, id, wc, mc, mass, cg, q.drag_scale, y, k3);
#pragma unroll
          for (int c = 0; c < 6; ++c) y[c] = s[c] + dt * k3[c];
          iip_rhs(C, id, wc, mc, mass, cg, q.drag_scale, y, k4);
#pragma unroll
          for (int c = 0; c < 6; ++c) sn[c] = s[c] + h6 * ((k1[c] + (real)2.0 * k2[c]) + ((real)2.0 * k3[c] + k4[c]));
          if (!iip_finite6(sn)) break;   // does not land
          if (sn[2] <= q.ground) {
            const real wq = (s[2] - q.ground) / (s[2] - sn[2]);
            out[ERPL_IIP_CH_X] = s[0] + (sn[0] - s[0]) * wq;
            out[ERPL_IIP_CH_Y] = s[1] + (sn[1] - s[1]) * wq;
            out[ERPL_IIP_CH_TFALL] = ((double)n + wq) * dt;
            const real v0 = s[3] + (sn[3] - s[3]) * wq, v1 = s[4] + (sn[4] - s[4]) * wq, v2 = s[5] + (sn[5] - s[5]) * wq;
            out[ERPL_IIP_CH_VIMPACT] = m_sqrt((v0 * v0 + v1 * v1) + v2 * v2);
            landed = true;
            break;
          }
#pragma unroll
          for (int c = 0; c < 6; ++c) s[c] = sn[c];
        }
      }
      if (landed) {
        const real dx = out[ERPL_IIP_CH_X] - q.origin_x, dy = out[ERPL_IIP_CH_Y] - q.origin_y;
        out[ERPL_IIP_CH_RANGE] = m_sqrt(dx * dx + dy * dy);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < ERPL_IIP_CH_COUNT; ++c) q.values[((int64_t)c * q.n_nodes + k) * q.ld + q.col0 + j] = out[c];
}

// is (x, y) inside the polygon: the even-odd crossing rule of erpl_mc_impact_density's zones (erpl_density.hip), restated -
// same expression, every operation rounded on its own (the unit is built without contraction)
__device__ __forceinline__ bool iip_inside(const double* vx, const double* vy, int nv, double x, double y) {
  bool in = false;
  for (int i = 0, jv = nv - 1; i < nv; jv = i++)
    if ((vy[i] > y) != (vy[jv] > y) && x < (vx[jv] - vx[i]) * (y - vy[i]) / (vy[jv] - vy[i]) + vx[i]) in = !in;
  return in;
}

// The wave's best, returned to every lane: the wave half of the envelope's fold (env_reduce itself is left to the envelope
// kernel alone - with a second kernel calling it, the compiler no longer sees which LDS array it reduces through and the
// envelope kernel's code changes).  Same total order, so the result does not depend on the fold's shape.
template <bool MAX>
__device__ __forceinline__ EnvBest iip_wave_best(EnvBest x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    EnvBest o;
    o.v = __shfl_down(x.v, off);
    o.i = __shfl_down(x.i, off);
    x = env_better<MAX>(x, o);   // (a lane whose partner is past the wave reads itself)
  }
  EnvBest r;
  r.v = __shfl(x.v, 0);
  r.i = __shfl(x.i, 0);
  return r;
}

// The number of evaluated nodes of trajectory j - the nodes k with k * record_stride < u, u the usable prefix as the envelope
// kernel finds it - by the 64 lanes of one wave; only the records a node can sit on or behind are scanned.
__device__ __forceinline__ int64_t iip_evaluated_nodes(const ErplKArgs& a, const ErplIipArgs& q, int64_t j) {
  int64_t len = a.traj_len[j];
  len = (len < 0) ? 0 : ((len > a.traj_cap) ? a.traj_cap : len);   // never past the trajectory's own slots
  const double* __restrict__ recs = a.traj + j * a.traj_cap * ERPL_TRAJ_DIM;
  const int64_t stride = q.record_stride;
  int64_t scan = (int64_t)(q.n_nodes - 1) * stride + 1;
  scan = (scan < len) ? scan : len;
  EnvBest mine = env_none();
  for (int64_t r = threadIdx.x; r < scan; r += kIipBlock) {
    const double* rec = recs + r * ERPL_TRAJ_DIM;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < ERPL_TRAJ_DIM; ++c) ok = ok && __builtin_isfinite(rec[c]);
    if (!ok) { mine.i = r; break; }
  }
  const EnvBest first_bad = iip_wave_best<false>(mine);
  const int64_t u = (first_bad.i == kEnvNone) ? scan : first_bad.i;   // (u of the scanned records: the same nodes are below it)
  const int64_t nodes = (u + stride - 1) / stride;
  return (nodes < q.n_nodes) ? nodes : q.n_nodes;
}

// The prefix kernel, ahead of the fall: grid = n_traj workgroups of one wave; trajectory j's X slot of node k becomes 1.0 if
// the node is evaluated and NaN if not, and the number of evaluated nodes goes to the trajectory's NODES row of the summary,
// where the summary kernel finds it (it does not scan again).  (A fall lane that scanned its own prefix read every record up to its node: 125 GB
// for 8 192 trajectories x 64 nodes at stride 10 against 3.9 GB here - DESIGN.md 8.11.)
__global__ __launch_bounds__(kIipBlock) void erpl_iip_prefix_f64(const ErplKArgs a, const ErplIipArgs q) {
  const int64_t j = blockIdx.x;
  if (j >= a.n_traj) return;
  const int64_t nodes = iip_evaluated_nodes(a, q, j);
  for (int64_t k = threadIdx.x; k < q.n_nodes; k += kIipBlock)
    q.values[((int64_t)ERPL_IIP_CH_X * q.n_nodes + k) * q.ld + q.col0 + j] = (k < nodes) ? 1.0 : (double)NAN;
  if (q.summary && threadIdx.x == 0) q.summary[(int64_t)ERPL_IIP_NODES * a.n_traj + j] = (double)nodes;
}

// The summary [ERPL_IIP_DIM][n_traj] of the values the fall kernel left: grid = n_traj workgroups of one wave, lane t takes
// the nodes t, t + 64, ...  Reductions as in the envelope kernel: (value, node) pairs under its total order, env_better.
__global__ __launch_bounds__(kIipBlock) void erpl_iip_summary_f64(const ErplKArgs a, const ErplIipArgs q,
                                                                   const ErplIipKeepIn keep) {
  __shared__ double s_vx[ERPL_IIP_MAX_VERTICES], s_vy[ERPL_IIP_MAX_VERTICES];
  const int tid = threadIdx.x;
  const int nv = keep.n;
  if (tid < nv) { s_vx[tid] = keep.x[tid]; s_vy[tid] = keep.y[tid]; }
  __syncthreads();
  const int64_t j = blockIdx.x;
  if (j >= a.n_traj) return;
  const double* __restrict__ recs = a.traj + j * a.traj_cap * ERPL_TRAJ_DIM;
  const int64_t stride = q.record_stride;
  int64_t nodes = (int64_t)q.summary[(int64_t)ERPL_IIP_NODES * a.n_traj + j];   // the prefix kernel's count
  nodes = (nodes < 0) ? 0 : ((nodes > q.n_nodes) ? q.n_nodes : nodes);
  const double* X = q.values + ((int64_t)ERPL_IIP_CH_X * q.n_nodes) * q.ld + q.col0 + j;
  const double* Y = q.values + ((int64_t)ERPL_IIP_CH_Y * q.n_nodes) * q.ld + q.col0 + j;
  const double* R = q.values + ((int64_t)ERPL_IIP_CH_RANGE * q.n_nodes) * q.ld + q.col0 + j;
  double row[ERPL_IIP_DIM];
#pragma unroll
  for (int c = 0; c < ERPL_IIP_DIM; ++c) row[c] = (double)NAN;
  int landed = 0;
  if (nodes > 0) {   // (uniform over the wave)
    const double t0 = recs[0];
    const double burn = a.motor[3 * a.n + a.traj_ids[j]];
    EnvBest far = env_none(), top = env_none(), bo = env_none(), rate = env_none(), ex = env_none();
    for (int64_t k0 = 0; k0 < nodes; k0 += kIipBlock) {   // (every lane takes every round: the ballot below)
      const int64_t k = k0 + tid;
      bool on = false;
      if (k < nodes) {
        const double* rec = recs + k * stride * ERPL_TRAJ_DIM;
        const double x = X[k * q.ld], y = Y[k * q.ld];
        on = __builtin_isfinite(x);   // a landed node: all five channels are finite
        env_take<true>(top, rec[3], k);
        if (bo.i == kEnvNone && rec[0] - t0 > burn) bo.i = k;
        if (on) {
          env_take<true>(far, R[k * q.ld], k);
          if (ex.i == kEnvNone && nv > 0 && !iip_inside(s_vx, s_vy, nv, x, y)) ex.i = k;
          if (k + 1 < nodes) {
            const double x1 = X[(k + 1) * q.ld], y1 = Y[(k + 1) * q.ld];
            const double dts = (recs[(k + 1) * stride * ERPL_TRAJ_DIM] - t0) - (rec[0] - t0);
            if (__builtin_isfinite(x1) && dts > 0.0) {
              const double dx = x1 - x, dy = y1 - y;
              env_take<true>(rate, sqrt(dx * dx + dy * dy) / dts, k);
            }
          }
        }
      }
      landed += __popcll(__ballot(on ? 1 : 0));
    }
    const EnvBest bfar = iip_wave_best<true>(far), btop = iip_wave_best<true>(top), bbo = iip_wave_best<false>(bo);
    const EnvBest brate = iip_wave_best<true>(rate), bex = iip_wave_best<false>(ex);
    if (tid == 0) {
      if (bfar.i != kEnvNone) {
        row[ERPL_IIP_MAX_RANGE] = bfar.v; row[ERPL_IIP_MAX_RANGE_TIME] = recs[bfar.i * stride * ERPL_TRAJ_DIM] - t0;
        row[ERPL_IIP_MAX_RANGE_X] = X[bfar.i * q.ld]; row[ERPL_IIP_MAX_RANGE_Y] = Y[bfar.i * q.ld];
      }
      if (bbo.i != kEnvNone) {
        row[ERPL_IIP_BURNOUT_TIME] = recs[bbo.i * stride * ERPL_TRAJ_DIM] - t0;
        row[ERPL_IIP_BURNOUT_X] = X[bbo.i * q.ld]; row[ERPL_IIP_BURNOUT_Y] = Y[bbo.i * q.ld];   // NaN if it did not land
      }
      if (btop.i != kEnvNone) { row[ERPL_IIP_APOGEE_X] = X[btop.i * q.ld]; row[ERPL_IIP_APOGEE_Y] = Y[btop.i * q.ld]; }
      if (brate.i != kEnvNone) {
        row[ERPL_IIP_MAX_RATE] = brate.v; row[ERPL_IIP_MAX_RATE_TIME] = recs[brate.i * stride * ERPL_TRAJ_DIM] - t0;
      }
      if (bex.i != kEnvNone) {
        row[ERPL_IIP_EXIT_TIME] = recs[bex.i * stride * ERPL_TRAJ_DIM] - t0;
        row[ERPL_IIP_EXIT_X] = X[bex.i * q.ld]; row[ERPL_IIP_EXIT_Y] = Y[bex.i * q.ld];
      }
    }
  }
  if (tid == 0) {
    row[ERPL_IIP_LANDED] = (double)landed; row[ERPL_IIP_NODES] = (double)nodes;
#pragma unroll
    for (int c = 0; c < ERPL_IIP_DIM; ++c) q.summary[(int64_t)c * a.n_traj + j] = row[c];
  }
}

}  // namespace
