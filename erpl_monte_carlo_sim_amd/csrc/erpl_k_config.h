// erpl_k_config.h — every compile-time choice of the trajectory kernels (erpl_kernels.inc).
//
// A unit file defines exactly ONE selector and includes erpl_kernels.inc; this header derives the rest.
//
//                                    ERPL_FAITHFUL          ERPL_FAST_F64             ERPL_FAST_F32
//   unit / launcher                  erpl_k64.hip           erpl_k64f.hip             erpl_k32.hip
//                                    erpl_launch_f64        erpl_launch_f64f          erpl_launch_f32
//   real, kernel suffix              double, f64            double, f64f              float, f32
//   arithmetic                       reference order,       fast: shortcuts, own      fast: shortcuts, hardware
//                                    IEEE div / sqrt, libm  exp2 / log2 / atan        transcendentals
//   lane state, wind interval        registers              per-lane LDS   [1]        registers
//   Mach / atmosphere records        registers              index into the shared     registers
//                                                           LDS tables     [1]
//   wind altitude grid               static LDS             dynamic LDS (K values)    static LDS
//   polynomial coefficients          -                      __constant__ tables       literals
//                                                           (erpl_k_math.h)
//   flight workgroup                 256 threads            64 threads     [1]        256 threads
//   blow-ups                         flown out (and the     handed over to the        flown out
//                                    f64f build's: [3])     gate kernel    [2]
//   coast of a z-NaN sample          stepped (reference     stepped                   closed form
//                                    rounding)
//   the lane's clock in the RK4 loop registers              registers                 LDS            [4]
//   atmosphere layer bounds cached   -                      no                        yes            [5]
//   ERPL_STAGE_UNROLL                1 (rolled)             4                         4
//   ERPL_FLIGHT_MIN_WAVES            1                      2                         2  (ERPL_DENSE_WAVES for
//                                                                                        large batches)
//
// The code forks on the selectors themselves: `#if ERPL_FAITHFUL`, `#if ERPL_FAST_F64`, `#if ERPL_FAST_F32`.
//
// [1] Two waves per SIMD for the fp64 throughput build (round 3).  With ONE resident wave every instruction of any
//     kind - scalar moves, accumulation-register copies, waits - takes a full issue slot of the SIMD (one slot per
//     four cycles); with two, the scalar / LDS / branch instructions of one wave issue beside the vector
//     instructions of the other and LDS latency is covered.  Two waves need <= 256 registers per lane, which the
//     all-in-registers layout misses by ~100 doubles, so this build keeps in LDS what is touched only at known
//     points of a step:
//       the 14-state y of the lane (read when a stage vector is formed, written once per step);
//       the lane's current wind interval (9 values, read at the top of every RHS evaluation);
//       of its Mach interval and atmosphere layer the lane keeps only the INDEX and reads the records from the
//       workgroup's shared LDS tables where the RHS consumes them (a broadcast when the lanes agree, which they
//       mostly do).
//     64-thread workgroups (one wave), eight of them per CU: 14 + 9 doubles per lane = 11.8 KB plus 4.1 KB of tables
//     plus the wind altitude grid (dynamic: K doubles) per workgroup, 132 KB of the CU's 160 KB at K = 100.
//     The uniform constants of the RK4 loop stay where the fp32 build has them: scalar registers straight from the
//     kernel arguments.
// [2] Hand-over of blow-ups to the reference-order kernel (round 4).  The fp64 throughput build reproduces the reference
//     to ~1e-9 for as long as the state is of physical size; what it cannot reproduce is WHICH intermediate of the last one
//     or two RK4 steps of a diverged sample (speeds of 1e25 .. 1e120 m/s) overflows to inf and which turns
//     NaN - that depends on the exact operation order (x * rsq(x) against sqrt(x), a fused against a separate multiply,
//     a ratio against the trig of an atan2), and the reference's outcome depends on it: an infinite altitude ends the flight
//     at `z > 100 000` (simulator.py:242), a NaN one runs to max_time (:216) - 81 % of round 3's apogee mismatches
//     (profiles/r4_divergence_before.txt).  So a lane whose speed passes ERPL_HANDOFF_SPEED (1e6 m/s) or that is 100 km
//     below the ground leaves the RK4 loop after that step, is parked in the context's hand-over queue and finishes in the
//     reference-order kernel (erpl_launch_f64_sweep behind the last launch of the batch).  From below that bound no
//     intermediate of ONE step comes near the overflow threshold (worst case ~1e180), and from above
//     it a diverging sample has two steps left on average, 31 at most (profiles/r4_blowup_sizing.json: 99.8 % of the bench
//     shard's samples pass it, 0.07 % of all steps are made beyond it).  No flight the model is valid for comes near it.
// [3] Which instantiation flies the handed-over lanes - both are compiled, the launcher's `waves` argument picks one per
//     sweep (erpl_launch_f64_sweep): 1 = the gate's own (one wave per SIMD, all 512 registers, no scratch), 2 = a copy
//     capped at 256 registers (ERPL_SWEEP_CAPPED_WAVES) whose waves fit beside the throughput kernel's (612-772 bytes of
//     scratch per lane, saved and restored around every exit of its RK4 loop).  A 512-register wave starts only on a SIMD
//     with no other wave on it, so its dispatch lasts until SIMDs have emptied (29 ms for 2 ms of work with eight batches
//     in flight).  On a stream of its own - the lane's sweep stream, with a hardware queue per stream - that wait costs
//     nothing (22.41 / 23.30 ms per pass with 2, 22.81 / 22.68 with 1) and the capped copy wrote 258 MB and fetched 226 MB
//     per pass where the gate's own writes 48 and fetches 103: there, in erpl_mc_run_batch, in the gate build and for
//     trajectory capture the gate's own runs.  Where the sweep shares its stream with the lane's next batch (submitted
//     batches without a sweep stream: the HIP default of four hardware queues) the wait would hold that batch back
//     while the other lanes keep every SIMD full: there the capped copy runs.  Same source, same flags, same bits.
//     It runs the full grid (n / 64 workgroups) at the default wave priority there too: 1/2, 1/4 and 1/8 of the grid
//     with refill from the hand-over queue, and s_setprio 1 / 3 for its waves, measured no gain.
// [4] The register-capped fp32 build keeps the lane's clock (a double) in LDS through the RK4 loop: the compiler
//     spilled exactly that pair to scratch and re-read it at every stage, and a scratch load is a vector-memory
//     load - it shares the in-order counter with the table reloads, so every stage start waited for whatever
//     reload or prefetch was still in flight.  LDS reads come back on the other counter.
// [5] The atmosphere layer's own bounds are cached next to the combined layer-and-wind range, so that a wind-knot
//     crossing inside a layer does not re-read the layer record (altitude_tables_reload).  In the fp64 throughput
//     build the two extra doubles cost more in accumulation-register copies than the skipped record load saves.
#pragma once

#ifndef ERPL_FAITHFUL
#define ERPL_FAITHFUL 0   // reference operation order (double normalisation, trig of atan2, IEEE divisions): the gate
#endif
#ifndef ERPL_FAST_F64
#define ERPL_FAST_F64 0   // the fp64 throughput build
#endif
#ifndef ERPL_FAST_F32
#define ERPL_FAST_F32 0   // the fp32 throughput build
#endif
#if ERPL_FAITHFUL + ERPL_FAST_F64 + ERPL_FAST_F32 != 1
#error "define exactly one of ERPL_FAITHFUL, ERPL_FAST_F64, ERPL_FAST_F32 to 1 before including erpl_kernels.inc"
#endif

#define ERPL_CAT_(a, b) a##b
#define ERPL_CAT(a, b) ERPL_CAT_(a, b)
#if ERPL_FAITHFUL
typedef double real;
#define ERPL_SUFFIX f64
#elif ERPL_FAST_F64
typedef double real;
#define ERPL_SUFFIX f64f
#else
typedef float real;
#define ERPL_SUFFIX f32
#endif
#define ERPL_LAUNCH_NAME ERPL_CAT(erpl_launch_, ERPL_SUFFIX)

// ---- numeric tunables (a value, not a code path: -D overrides for A/B builds) ----
// RK4 stages: 1 = rolled stage loop (one RHS instance), 4 = fully unrolled.  Unrolled: -8 % time in the fp32 build
// (no loop-carried register moves, cross-stage scheduling); the gate keeps the rolled loop (code size, compile time).
#ifndef ERPL_STAGE_UNROLL
#if ERPL_FAITHFUL
#define ERPL_STAGE_UNROLL 1
#else
#define ERPL_STAGE_UNROLL 4
#endif
#endif
// Min waves per SIMD the register allocator must leave room for in the flight kernel.  fp64 throughput: two ([1]).
// fp32: two for the uncapped build - at most 256 registers (left to itself the allocator took a 257th with the wind
// prefetch in and halved the occupancy).
#ifndef ERPL_FLIGHT_MIN_WAVES
#if ERPL_FAITHFUL
#define ERPL_FLIGHT_MIN_WAVES 1
#else
#define ERPL_FLIGHT_MIN_WAVES 2
#endif
#endif
// fp32 only: resident waves per SIMD of the register-capped instantiation used for large batches (168 VGPRs, three
// resident waves at the price of ~80 spilled registers - measured +6 % on batches that keep three waves per SIMD
// busy).  Same arithmetic, bitwise identical results (tested).
#ifndef ERPL_DENSE_WAVES
#define ERPL_DENSE_WAVES 3
#endif
#ifndef ERPL_SWEEP_CAPPED_WAVES
#define ERPL_SWEEP_CAPPED_WAVES 2   // [3]
#endif
// One wave per workgroup for the rail kernel too: with several batches in flight every SIMD is full of flight
// waves, and a 256-thread workgroup only starts once FOUR wave slots of one CU are free together, while the batch's
// flight launch waits behind it (rocprofv3 timeline of bench.py: rail dispatches of 0.07 ms of work lasting 67-95 ms);
// 64-thread workgroups slip into single slots as flight waves leave (bench shard: 27.08 -> 26.46 ms per pass over
// five alternating runs, fp32 10.78 -> 10.61).
#ifndef ERPL_RAIL_BLOCK
#define ERPL_RAIL_BLOCK 64
#endif
#ifndef ERPL_HANDOFF_SPEED
#define ERPL_HANDOFF_SPEED 1e6   // [2], m/s
#endif

// ---- diagnostic build only (-DERPL_STAMPS=1): s_memtime stamps around segments of one integration step,
// summed per wave in scalar registers and added to counters[8..15] at wave exit.  Never in the
// shipped library (the stamps fence the scheduler); read the SHARES, not the run time. ----
#ifndef ERPL_STAMPS
#define ERPL_STAMPS 0
#endif
#if ERPL_STAMPS
#define ERPL_STAMP(acc_, last_)                                                          \
  do {                                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                   \
    unsigned long long now_;                                                             \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");          \
    __builtin_amdgcn_sched_barrier(0);                                                   \
    acc_ += now_ - last_;                                                                \
    last_ = now_;                                                                        \
  } while (0)
#else
#define ERPL_STAMP(acc_, last_) do { } while (0)
#endif

namespace {
constexpr bool kFaithful = (ERPL_FAITHFUL != 0);
constexpr int kWave = 64;
struct StampSums { unsigned long long seg[8]; unsigned long long last; };
}  // namespace
// Inside a rarely taken block: keeps it a real (wave-skipped) branch instead of being if-converted to
// v_cndmask selects that every step would pay for.
#define ERPL_RARE_BLOCK() asm volatile("")
