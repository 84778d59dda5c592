// erpl_k_launch.h — the host side of a kernel unit: erpl_launch_<suffix> (rail + flight launches of one batch), the
// gate unit's sweep, extract, envelope, impact-point and debris launchers, the debug launcher.

// One flight launch, from g, b, dyn_lds, st, a, S of the launcher that uses it.  SPEC >= 0 compiles the two launch
// constants of the RHS in (bit 0 = a wind table is present, bit 1 = solid motor); trajectory capture reads them at run
// time: <true, -1, MINW>.  ERPL_LAUNCH_FLIGHT_SPEC picks the specialisation of a launch without capture.
#define ERPL_LAUNCH_FLIGHT(TRAJ_, SPEC_, MINW_) \
  hipLaunchKernelGGL((ERPL_CAT(erpl_flight_, ERPL_SUFFIX)<TRAJ_, SPEC_, MINW_>), g, b, dyn_lds, st, a, S)
#define ERPL_LAUNCH_FLIGHT_SPEC(MINW_)                                                                  \
  do {                                                                                                  \
    const int spec_ = ((a.k_wind > 0) ? 1 : 0) | ((a.motor_kind == ERPL_MOTOR_SOLID) ? 2 : 0);          \
    if (spec_ == 0) ERPL_LAUNCH_FLIGHT(false, 0, MINW_);                                                \
    else if (spec_ == 1) ERPL_LAUNCH_FLIGHT(false, 1, MINW_);                                           \
    else if (spec_ == 2) ERPL_LAUNCH_FLIGHT(false, 2, MINW_);                                           \
    else ERPL_LAUNCH_FLIGHT(false, 3, MINW_);                                                           \
  } while (0)

int ERPL_LAUNCH_NAME(const ErplKArgs& a0, const void* scalars, int block, int max_blocks, int n_phases,
                     void* stream, void** ev, void* tail_stream, void* main_done, int sweep_waves) {
  hipStream_t st = (hipStream_t)stream;
  if (a0.n <= 0) return 0;
  ErplKArgs a = a0;
  const ErplScalars<real> S = *(const ErplScalars<real>*)scalars;
  const int rail_block = ERPL_RAIL_BLOCK;   // one wave per workgroup for the rail kernel too (erpl_k_config.h)
  const int64_t rail_grid = (a.n + rail_block - 1) / rail_block;
  if (ev) (void)hipEventRecord((hipEvent_t)ev[0], st);
  hipLaunchKernelGGL(ERPL_CAT(erpl_rail_, ERPL_SUFFIX), dim3((unsigned)rail_grid), dim3(rail_block), 0, st, a, S);
  if (ev) (void)hipEventRecord((hipEvent_t)ev[1], st);
#if ERPL_FAST_F64
  if (block != kFlightBlock) {   // the per-lane LDS arrays are static [..][64]: this build always runs 64-thread workgroups
    if (max_blocks > 0) max_blocks = (int)(((int64_t)max_blocks * block + kFlightBlock - 1) / kFlightBlock);
    block = kFlightBlock;
  }
  const size_t dyn_lds = (size_t)((a.k_wind > 0 ? a.k_wind : 1) * sizeof(real) + 15) & ~(size_t)15;   // the wind altitude grid
#else
  const size_t dyn_lds = 0;
#endif
  int64_t grid = (a.n + block - 1) / block;
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  // One flight launch per step-chunk: the kernel boundary is the only synchronisation the
  // compaction needs.  Launches whose queue is already empty return at once.
  for (int ph = 0; ph < n_phases; ++ph) {
    a.phase = ph;
    a.adopt_lanes = (ph + 1 < n_phases && a0.n_traj == 0) ? a0.adopt_lanes : 0;   // the last launch flies everything out
    const dim3 g((unsigned)grid), b(block);
    if (a.n_traj > 0) ERPL_LAUNCH_FLIGHT(true, -1, ERPL_FLIGHT_MIN_WAVES);
#if ERPL_FAST_F32
    else if (a.waves_per_simd >= 3) ERPL_LAUNCH_FLIGHT_SPEC(ERPL_DENSE_WAVES);   // the register-capped build for large batches
#endif
    else ERPL_LAUNCH_FLIGHT_SPEC(ERPL_FLIGHT_MIN_WAVES);
    if (ph == 0 && tail_stream && n_phases > 1) {   // the sweeps follow the main launch on their own stream
      (void)hipEventRecord((hipEvent_t)main_done, st);
      st = (hipStream_t)tail_stream;
      (void)hipStreamWaitEvent(st, (hipEvent_t)main_done, 0);
    }
  }
#if ERPL_FAST_F64
  {  // the lanes this build handed over finish in the reference-order kernel, behind the last launch of the batch
    ErplKArgs g = a0;
    g.res_r[1] = a0.ext_r; g.res_d[1] = a0.ext_d; g.res_i[1] = a0.ext_i;
    g.qcnt = a0.ext_q; g.qhead = a0.ext_q + ERPL_EXT_Q;
    g.phase = 1; g.chunk_steps = 0; g.adopt_lanes = 0;
    const int rc = erpl_launch_f64_sweep(g, scalars, kWave, max_blocks, (void*)st, sweep_waves);
    if (rc != 0) return rc;
  }
#endif
  if (ev) (void)hipEventRecord((hipEvent_t)ev[2], st);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

#if ERPL_FAITHFUL
// erpl_launch_f64_sweep (erpl_tables.h): the flight kernel alone, on the queue `a` maps.  waves = 2 picks the instantiation
// capped at 256 registers (note [3] of erpl_k_config.h); trajectory capture always runs the gate's own.
int erpl_launch_f64_sweep(const ErplKArgs& a, const void* scalars, int block, int max_blocks, void* stream, int waves) {
  if (a.n <= 0) return 0;
  const ErplScalars<real> S = *(const ErplScalars<real>*)scalars;
  int64_t grid = (a.n + block - 1) / block;
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  const dim3 g((unsigned)grid), b(block);
  hipStream_t st = (hipStream_t)stream;
  const size_t dyn_lds = 0;
  if (a.n_traj > 0) ERPL_LAUNCH_FLIGHT(true, -1, ERPL_FLIGHT_MIN_WAVES);
  else if (waves >= ERPL_SWEEP_CAPPED_WAVES) ERPL_LAUNCH_FLIGHT_SPEC(ERPL_SWEEP_CAPPED_WAVES);
  else ERPL_LAUNCH_FLIGHT_SPEC(ERPL_FLIGHT_MIN_WAVES);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int erpl_launch_extract_f64(const ErplKArgs& a, const void* scalars, double time_offset, void* stream) {
  if (a.traj_cap <= 0) return 0;
  const ErplScalars<real> S = *(const ErplScalars<real>*)scalars;
  const int block = 256;
  const int64_t grid = (a.traj_cap + block - 1) / block;
  hipLaunchKernelGGL(erpl_extract_f64, dim3((unsigned)grid), dim3(block), 0, (hipStream_t)stream, a, S, time_offset);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int erpl_launch_envelope_f64(const ErplKArgs& a, const void* scalars, void* stream) {
  if (a.n_traj <= 0) return 0;
  const ErplScalars<real> S = *(const ErplScalars<real>*)scalars;
  hipLaunchKernelGGL(erpl_envelope_f64, dim3((unsigned)a.n_traj), dim3(kEnvBlock), 0, (hipStream_t)stream, a, S);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int erpl_launch_iip_f64(const ErplKArgs& a, const void* scalars, const ErplIipArgs& q, const ErplIipKeepIn& keep, void* stream) {
  if (a.n_traj <= 0 || q.n_nodes <= 0) return 0;
  const ErplScalars<real> S = *(const ErplScalars<real>*)scalars;
  const size_t dyn_lds = (size_t)(a.k_wind > 0 ? a.k_wind : 1) * sizeof(real);   // the wind altitude grid
  const unsigned per_traj = (unsigned)((a.n_traj + kIipBlock - 1) / kIipBlock);
  hipLaunchKernelGGL(erpl_iip_prefix_f64, dim3((unsigned)a.n_traj), dim3(kIipBlock), 0, (hipStream_t)stream, a, q);
  hipLaunchKernelGGL(erpl_iip_fall_f64, dim3(per_traj, (unsigned)q.n_nodes), dim3(kIipBlock), dyn_lds, (hipStream_t)stream,
                     a, S, q);
  if (q.summary)
    hipLaunchKernelGGL(erpl_iip_summary_f64, dim3((unsigned)a.n_traj), dim3(kIipBlock), 0, (hipStream_t)stream, a, q, keep);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int erpl_launch_debris_f64(const ErplKArgs& a, const void* scalars, const ErplDebrisArgs& q, const ErplDebrisFragments& fr,
                           const ErplIipKeepIn& keep, void* stream) {
  if (a.n_traj <= 0 || q.n_nodes <= 0 || q.n_fragments <= 0) return 0;
  const ErplScalars<real> S = *(const ErplScalars<real>*)scalars;
  const size_t dyn_lds = (size_t)(a.k_wind > 0 ? a.k_wind : 1) * sizeof(real);   // the wind altitude grid
  const unsigned per_traj = (unsigned)((a.n_traj + kDebrisBlock - 1) / kDebrisBlock);
  hipLaunchKernelGGL(erpl_debris_prefix_f64, dim3((unsigned)a.n_traj), dim3(kDebrisBlock), 0, (hipStream_t)stream, a, q);
  hipLaunchKernelGGL(erpl_debris_fall_f64, dim3(per_traj, (unsigned)(q.n_nodes * q.n_fragments)), dim3(kDebrisBlock), dyn_lds,
                     (hipStream_t)stream, a, S, q, fr);
  if (q.summary)
    hipLaunchKernelGGL(erpl_debris_summary_f64, dim3((unsigned)a.n_traj), dim3(kDebrisBlock), 0, (hipStream_t)stream, a, q, keep);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
#endif

int ERPL_CAT(erpl_launch_debug_, ERPL_SUFFIX)(const ErplKArgs& a, const void* scalars, int what, int64_t m,
                                              const double* in, double* out, void* stream) {
  if (m <= 0) return 0;
  const ErplScalars<real> S = *(const ErplScalars<real>*)scalars;
#if ERPL_FAST_F64
  const int block = kWave;   // per-lane LDS arrays of one wave
#else
  const int block = 256;
#endif
  const int64_t lanes = (what == ERPL_DBG_RHS_SEQ) ? a.n : m;   // one lane per sample / per column
  const int64_t grid = (lanes + block - 1) / block;
  hipLaunchKernelGGL(ERPL_CAT(erpl_debug_, ERPL_SUFFIX), dim3((unsigned)grid), dim3(block), 0, (hipStream_t)stream, a, S,
                     what, m, in, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
#undef ERPL_LAUNCH_FLIGHT_SPEC
#undef ERPL_LAUNCH_FLIGHT
