// erpl_kernels.inc — the trajectory kernels, written once and compiled three times:
//   erpl_k64.hip  : ERPL_FAITHFUL = 1, real = double, -ffp-contract=off  (correctness gate, cfg 2; one wave per SIMD; the
//                   same instantiation finishes the blow-ups the fp64 throughput build hands over, except where the
//                   sweep shares a stream with the lane's next batch: there a copy capped at 256 registers, two waves
//                   per SIMD, does - note [3] of erpl_k_config.h)
//   erpl_k64f.hip : ERPL_FAST_F64 = 1, real = double                     (fp64 throughput: the headline build)
//   erpl_k32.hip  : ERPL_FAST_F32 = 1, real = float                      (fp32 throughput: healthy flights / first apogee)
//
// One trajectory per lane (wave64).  Kernel 1 integrates the launch rail (simulator.py:42-125)
// for every sample and parks the rail-exit state as a record of the resume queue.  Kernel 2 is the
// flight integrator (simulator.py:208-264 over _rocket_dynamics :295-460): every wave pops lane
// records from a device-wide atomic queue, keeps the 14-state, the per-sample parameters and the
// current wind / Mach-table / atmosphere intervals in registers (the fp64 throughput build: the state and the
// wind interval in per-lane LDS, the table records by index in the workgroup's LDS tables), reads the shared
// interval tables only when a lane leaves its interval, and uses wave ballots to refill finished lanes from
// the queue, to hand the last lanes of a thinning wave to fuller waves (lane adoption) and (with step-chunked
// launches) to park still-flying lanes densely for the next launch.  Kernel 3 (fp64 only) evaluates the
// per-step diagnostic histories of _extract_results (:496-552); kernel 4 (fp64 only) reduces every captured trajectory
// of a batch to its flight envelope through the same per-record evaluation; kernels 5 to 7 (fp64 only) let every chosen
// record of a captured trajectory fall to the ground without thrust and summarise where it comes down; kernels 8 to 10
// (fp64 only) do the same for the fragments of a vehicle that breaks up there.
//
// ERPL_FAITHFUL keeps the reference's operation order (double normalisation, trig of
// atan2, IEEE divisions); the two throughput builds allow algebraically identical shortcuts (no trig, reciprocal
// multiplies, hardware transcendental instructions).  Reference citations are on each block.  What else each
// build implies, and every tunable, is in erpl_k_config.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "erpl_tables.h"
#include "erpl_k_config.h"   // the three builds: real, suffix, launcher name, what each of them keeps where, tunables
#include "erpl_k_math.h"     // m_*: the reference-order and the fast families
#include "erpl_k_lookup.h"   // cold arguments, LDS tables, lane parameters, wind / Mach / atmosphere caches, LaneRec
#if ERPL_FAITHFUL
#include "erpl_k_rhs_ref.h"  // rocket_dynamics in the reference's operation order
#else
#include "erpl_k_rhs_fast.h" // rocket_dynamics_at: the short formulation
#endif
#include "erpl_k_rail.h"     // kernel 1
#include "erpl_k_flight.h"   // kernel 2, Lane and its record helpers
#include "erpl_k_debug.h"    // one stored record's evaluation, kernel 3 (gate only) and the known-answer debug kernel
#if ERPL_FAITHFUL
#include "erpl_k_envelope.h" // kernel 4 (gate only): the flight envelope of every captured trajectory
#include "erpl_k_iip.h"      // kernels 5 - 7 (gate only): the instantaneous impact points of every captured trajectory
#include "erpl_debris.h"     // the direction, step and tick rules the host shares with kernels 8 - 10
#include "erpl_k_debris.h"   // kernels 8 - 10 (gate only): where the fragments fall if the vehicle breaks up at a node
#endif
#include "erpl_k_launch.h"   // host: erpl_launch_<suffix>, the sweep, extract, envelope, impact-point, debris and debug launchers
