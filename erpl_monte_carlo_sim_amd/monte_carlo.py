"""MonteCarloAnalyzer — drop-in for monte_carlo.py:17-473 of the reference.

`run_monte_carlo(initial_conditions, n_samples, n_processes=None, optimized=False)` keeps its
signature and the structure of the returned analysis dict.  The ProcessPoolExecutor fan-out of the
reference (one future per sample, results pickled back through pipes) becomes: flatten all samples
into SoA tensors -> one `erpl_mc_run_batch` per GPU on this rank's shard -> one all-gather of the
[16, n] summaries (RCCL when torch.distributed is initialised with "nccl").  Dispersion draws and
motor perturbation stay on the host, the per-sample wind tables are built on the device
(`wind_on_device`; on the host without it); all are bit-identical to the reference (flatten.py);
the integration itself runs only on the GPU.
"""
import math
import os
import time

import numpy as np
import torch

from . import _abi, analysis, dist, flatten, plots, reports
from . import results as results_mod
from .engine import DeviceBatch, TrajectoryEngine
from .sampling import DEFAULT_UNCERTAINTY
from .simulator import shared_engine

_END = results_mod.END_NAMES


class _Shard:
    """Stand-in for a HostBatch in dist.run_local_shard: only its size is looked at (the shard is built chunk by
    chunk inside the runner)."""

    def __init__(self, n):
        self.n = n


class MonteCarloAnalyzer:
    def __init__(self, rocket, motor, atmosphere, wind_model, device=None, verbose=True):
        self.rocket, self.motor, self.atmosphere, self.wind_model = rocket, motor, atmosphere, wind_model
        self.n_cores = os.cpu_count()
        self.base_altitude_profile = None    # monte_carlo.py:27-32
        self.base_wind_profile = None
        self.uncertainty_params = {k: (list(v) if isinstance(v, list) else v) for k, v in DEFAULT_UNCERTAINTY.items()}
        self.device = device
        self.verbose = verbose
        # Kernel build: "f64_fast" (default since round 4) = the fp64 throughput build - the reference's outcome on every
        # sample of the parity sets (apogee, end reason, step count: 131 072 / 131 072 against the reference-order
        # kernel, 60 000 / 60 000 of those against the CPU oracle), healthy flights to 1e-9, 10 x the rate;
        # "f64" = the reference-order gate kernel (the reference's arithmetic op for op); "f32" = first-descent
        # apogee / healthy flights only
        self.precision = "f64_fast"
        self._motor_inputs = None            # [2, n] of the last run_batch_arrays: thrust and mass flow the kernels read
        # run_monte_carlo's chunks: True = the per-sample wind tables are built on the device (erpl_mc_legacy_wind_profiles_
        # device: drawn, scaled through the host's libm and finished in HBM, never uploaded), False = on the host
        # (erpl_mc_legacy_wind_profiles) and uploaded.  Same bits either way (DESIGN.md section 4 has the timings)
        self.wind_on_device = True
        self.n_trajectories = 50             # samples that carry a 'trajectory' (plots use the first 50)
        self.trajectory_stride = 20
        # simulator attributes a user could have changed on FlightSimulator
        self.max_time, self.dt_initial, self.pitch_damping, self.yaw_damping = 300.0, 0.01, 20.0, 20.0
        if verbose:
            print(f"Initialized Monte Carlo analyzer with {self.n_cores} cores")

    # -- parameter streams (bit-identical to the reference) -------------------------------------
    def _generate_parameter_samples(self, n_samples):
        return flatten.generate_parameter_samples(self.uncertainty_params, n_samples, stream="seed_i")

    def _generate_parameter_samples_vectorized(self, n_samples):
        return flatten.generate_parameter_samples(self.uncertainty_params, n_samples, stream="seed_42")

    # -- the hot path ------------------------------------------------------------------------------
    def _config(self):
        return flatten.config_from_objects(self.rocket, self.motor, self.atmosphere, dt_initial=self.dt_initial,
                                           max_time=self.max_time, pitch_damping=self.pitch_damping,
                                           yaw_damping=self.yaw_damping)

    CHUNK = 131072   # run_monte_carlo: samples per submitted batch - one batch fills an MI355X (256 CUs x 4 SIMDs x
    #                  2 waves x 64 lanes) and the host prepares the next one meanwhile
    DEVICE_CHUNK = 1 << 20   # run_monte_carlo_device: samples per sub-batch.  Nothing is prepared on the host there, and a
    #                  larger batch keeps the lanes busy from its own queue (5.8 M trajectories/s in one 1 M-sample launch
    #                  against 4.9 M for eight 131 072-sample batches, whose tails all fall at the end of the run)

    def _integrate_shard(self, initial_conditions, params, lo, hi, n_traj_global):
        """Integrate samples [lo, hi) of `params` (dict of arrays or list of dicts) on this rank's GPU; returns
        (summary [16, hi-lo] device tensor, status [hi-lo] device tensor, captured trajectories or None, motor inputs
        [2, hi-lo] NumPy: the thrust and mass-flow rows of the batches the kernels read, for analysis.factors_from_results).

        The samples that carry a trajectory (global index < n_traj_global: the first ones of the shard) go through
        the trajectory-capture build in a small batch of their own; everything else runs in chunks of CHUNK samples
        handed to erpl_mc_submit_batch, so that the host builds chunk i+1 (MT19937 streams in C threads, the AR(1)
        wind tables on the device with wind_on_device or in C threads without, the rest as NumPy expressions) while the
        GPU integrates chunk i.  Samples are independent: the
        split does not change a single bit of the summaries (tested)."""
        eng = shared_engine(self.device)
        eng.set_config(self._config())
        prec = _abi.PRECISIONS[self.precision]
        take = (lambda a, b: {k: v[a:b] for k, v in params.items()}) if isinstance(params, dict) else (lambda a, b: params[a:b])

        def host_batch(a, b, threads=0, with_wind=True):
            return flatten.dispersed_batch(self.rocket, self.motor, self.wind_model, initial_conditions, take(a, b),
                                           self.base_altitude_profile, self.base_wind_profile, threads=threads,
                                           with_wind=with_wind)

        def device_wind(hb, a, b):
            """The wind table flatten.dispersed_batch leaves out, built on the device on the current stream: the table
            of erpl_mc_legacy_wind_profiles and the host's post-steps in fp64, products rounded first as NumPy does."""
            seeds = np.asarray(take(a, b)["random_seed"] if isinstance(params, dict) else [p["random_seed"] for p in take(a, b)])
            if self.base_wind_profile is not None and self.base_altitude_profile is not None:
                w = flatten.legacy_wind_profiles_device(eng, self.wind_model, hb.alt_grid, seeds,
                                                        base=np.asarray(self.base_wind_profile, dtype=np.float64))
                up = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=eng.device)
                w[:, 0, :] += up(hb.wind_speed * hb.wind_cos)
                w[:, 1, :] += up(hb.wind_speed * hb.wind_sin)
                return w
            return flatten.legacy_wind_profiles_device(eng, self.wind_model, hb.alt_grid, seeds, speed=hb.wind_speed,
                                                       cdir=hb.wind_cos, sdir=hb.wind_sin)
        parts, traj, capture_inputs = [], None, None
        motor_parts = []
        m = max(0, min(hi, n_traj_global) - lo)   # local samples 0..m-1 are captured
        if m > 0:
            hb = host_batch(lo, lo + m)
            motor_parts.append(hb.motor[[0, 2]].copy())
            db = DeviceBatch.from_host(hb, eng.device, prec)
            dt = min(self.dt_initial, 0.005)
            cap = int(np.ceil(self.max_time / dt / self.trajectory_stride)) + 4
            ids = list(range(m))
            # on a stream of its own: the capture build follows a non-finite sample step by step to max_time (it has
            # records to write), 0.6 s for one wave - and erpl_mc_submit_batch starts a batch behind everything that is
            # on the caller's stream, so on the current stream it held up every chunk below (round 4: 1.5 -> 0.9 s at 10^6)
            cur = torch.cuda.current_stream(eng.device)
            capture_stream = torch.cuda.Stream(eng.device)
            capture_stream.wait_stream(cur)           # the upload above
            with torch.cuda.stream(capture_stream):   # (its output buffers are allocated and pre-filled on that stream too)
                summ, status, tr, tlen = eng.run(db, traj_ids=ids, traj_stride=self.trajectory_stride, traj_cap=cap,
                                                 flags=_abi.FLAG_CAPTURE_POSITION_ONLY)   # 'trajectory' = time, altitude, position
            for t_ in (summ, status, tr, tlen):
                t_.record_stream(cur)                 # consumed on the current stream, behind the wait_stream below
            # the inputs were allocated on the current stream and are read on the other one until the capture ends: they must
            # not go back to the allocator before (the chunk loop below would otherwise hand their memory to the next upload)
            capture_inputs = db
            for t_ in (db.ic, db.rocket, db.motor, db.alt_grid, db.wind):
                if t_ is not None:
                    t_.record_stream(capture_stream)
            traj = (ids, tr, tlen)
            parts.append((summ, status))
        inflight = []    # (ticket, inputs): the inputs must outlive their batch (it runs on the library's own streams)
        # look-ahead: `depth` batches run, one more is queued behind them while the host builds the next chunk.
        # erpl_mc_check_batch(T) waits for T's own event (batches behind it keep running) and answers for T itself.
        keep = eng.get_overlap() + 1
        incomplete = None

        def retire(ticket):
            nonlocal incomplete
            try:
                eng.check(ticket)   # host-blocking for that batch alone; raises if one of its lane hand-overs timed out
            except _abi.IncompleteBatch as e:
                # not raised here: in a multi-rank run the other ranks are on their way to the all-gather, and the
                # status words of the lost samples carry ERPL_ST_INCOMPLETE through it - run_batch_arrays raises on
                # EVERY rank from the gathered status
                incomplete = incomplete or e
        # Host preparation of the chunks runs in a few Python workers side by side (round 4): the C generators
        # (MT19937 streams, AR(1) wind tables) have their own threads, but the NumPy expressions between them are
        # single-threaded and were half of a chunk's preparation; NumPy and ctypes release the interpreter lock.
        # Chunks are consumed in order, so nothing about the results depends on it.  (131 072 samples with a
        # 100-knot wind table are 335 MB per prepared chunk, on the host and then on the device: at most workers + 1
        # wait to be submitted at a time.)
        import collections
        from concurrent.futures import ThreadPoolExecutor
        chunks = [(a, min(hi, a + self.CHUNK)) for a in range(lo + m, hi, self.CHUNK)]
        workers = max(1, min(len(chunks), flatten.host_workers()))
        def device_batch(a, b):
            # validation and the upload in the worker too: on the default stream of the engine's device, before the
            # submission that follows it there.  With wind_on_device the 335 MB wind table of a chunk is built there by
            # legacy_wind_device (the workers take turns at it: the engine holds a lock) and only the small rows go up;
            # without it the table is built on the host and uploaded from pageable memory.
            with torch.cuda.device(eng.device):
                hb = host_batch(a, b, threads=max(1, flatten.host_cores() // workers), with_wind=not self.wind_on_device)
                # (a batch that fell back to the per-sample loop carries its table: it goes up as before)
                wind = device_wind(hb, a, b) if hb.wind is None else None
                db = DeviceBatch.from_host(hb, eng.device, prec, wind=wind)
                db.motor_inputs = hb.motor[[0, 2]].copy()   # 16 bytes per sample, kept beside the summary
                return db
        with ThreadPoolExecutor(workers) as pool:
            todo = iter(chunks)
            ready = collections.deque()
            for _ in range(workers + 1):
                c = next(todo, None)
                if c is not None:
                    ready.append(pool.submit(device_batch, *c))
            while ready:
                db = ready.popleft().result()
                c = next(todo, None)
                if c is not None:
                    ready.append(pool.submit(device_batch, *c))
                parts.append(eng.submit(db))
                motor_parts.append(db.motor_inputs)
                inflight.append((eng.last_ticket, db))
                while len(inflight) > keep:
                    ticket, inputs = inflight.pop(0)
                    retire(ticket)        # only once the batch has finished may its inputs go back to the allocator
                    del inputs
        if inflight:
            eng.wait()
            retire(-1)
        if m > 0:
            torch.cuda.current_stream(eng.device).wait_stream(capture_stream)
            del capture_inputs
        motor_inputs = np.concatenate(motor_parts, axis=1) if motor_parts else np.zeros((2, 0))
        if len(parts) == 1:
            return parts[0][0], parts[0][1], traj, motor_inputs
        return torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts]), traj, motor_inputs

    def run_batch_arrays(self, initial_conditions, parameter_samples):
        """Integrate the given dispersed samples; returns (summary [16, n], status [n]) NumPy arrays
        (identical on every rank) and this rank's captured trajectories.  Each rank builds only its own
        shard [lo, hi) of the samples on the host (the per-sample seeds make them independent,
        monte_carlo.py:156-179)."""
        n = len(parameter_samples["random_seed"]) if isinstance(parameter_samples, dict) else len(parameter_samples)
        rank, ws = dist.world()
        lo, hi, _ = dist.shard_bounds(n, rank, ws)
        box = {}

        def runner(_unused):
            summ, status, box["traj"], box["motor"] = self._integrate_shard(initial_conditions, parameter_samples, lo, hi,
                                                                            min(self.n_trajectories, n))
            return summ, status
        local = _Shard(hi - lo) if hi > lo else None
        summ, status = dist.run_local_shard(n, local, runner)
        TrajectoryEngine.raise_if_incomplete(status)
        # the motor inputs of THIS rank's shard (they are not gathered: NaN for the samples of other ranks)
        self._motor_inputs = np.full((2, n), np.nan)
        if "motor" in box:
            self._motor_inputs[:, lo:hi] = box["motor"]
        return summ, status, box.get("traj"), lo

    def _sample_table(self, summ, status, parameter_samples, traj, lo, motor_inputs=None):
        """Columns of the run as a results.SampleTable (per-sample dicts are built on access)."""
        if motor_inputs is None and self._motor_inputs is not None and self._motor_inputs.shape[1] == np.shape(summ)[1]:
            motor_inputs = self._motor_inputs   # of the run_batch_arrays call that produced `summ`
        trajectories = {}
        if traj is not None:
            ids, tr, tlen = traj
            tr, tlen = tr.cpu().numpy(), tlen.cpu().numpy()
            for m, i in enumerate(ids):
                k = int(tlen[m])
                rec = tr[m, :k]
                trajectories[lo + i] = {           # monte_carlo.py:298-302
                    "time": rec[:, 0] - summ[_abi.SUM_RAIL_EXIT_TIME, lo + i],
                    "altitude": rec[:, 3].copy(),
                    "position": rec[:, 1:4].copy(),
                }
        return results_mod.SampleTable(summ, status, parameter_samples, trajectories, motor_inputs=motor_inputs)

    def _result_dicts(self, summ, status, parameter_samples, traj, lo):
        """The eager list of per-sample dicts (what round 2 returned; kept as the cross-check of LazyResults)."""
        table = self._sample_table(summ, status, parameter_samples, traj, lo)
        return [table.record(i) for i in range(table.n)]

    def run_monte_carlo(self, initial_conditions, n_samples=1000, n_processes=None, optimized=False):
        """monte_carlo.py:52-90 (and :92-154 when optimized=True: seed-42 stream + 'performance').

        Same inputs (bit for bit), same analysis dict.  `analysis['results']` / `['outliers']` are lazy sequences
        (results.LazyResults): `len`, indexing, slicing, iteration and `+` behave like the reference's lists and
        yield the same per-sample dicts, built on access; the outlier filter and the statistics run on the summary
        columns.  `self.precision` picks the kernel build: "f64_fast" (default) is the fp64 throughput build - the
        reference's outcome on every sample of the parity sets at 4-5 M trajectories/s (its blow-ups finish in the
        reference-order kernel); "f64" runs everything in the reference-order gate kernel
        (1.2 M trajectories/s)."""
        if self.verbose:
            print(f"Running Monte Carlo analysis with {n_samples} samples...")
        t0 = time.time()
        if optimized:   # one sequential RandomState(42) stream (monte_carlo.py:181-201)
            params = flatten.generate_parameter_arrays(self.uncertainty_params, n_samples, stream="seed_42")
        else:           # per-sample RandomState(i) streams
            params = flatten.generate_parameter_arrays(self.uncertainty_params, n_samples)
        summ, status, traj, lo = self.run_batch_arrays(initial_conditions, params)
        table = self._sample_table(summ, status, params, traj, lo, motor_inputs=self._motor_inputs)
        if self.verbose:
            print(f"Completed {table.n} out of {n_samples} simulations")
        out = results_mod.analyze_table(table, verbose=self.verbose)
        if optimized:
            el = time.time() - t0
            _, ws = dist.world()
            out["performance"] = {"total_time": el, "simulations_per_second": table.n / el,
                                  "cores_used": self.n_cores, "gpus_used": ws}
        return out

    def _fly_sub_batches(self, eng, initial_conditions, n_samples, lo, hi, rank, seed, prec, planar, design, submitted, retired=None):
        """The sub-batch loop of `run_monte_carlo_device` and `run_monte_carlo_tally`: this rank's samples [lo, hi) of the run
        in sub-batches of DEVICE_CHUNK (the draws of sub-batch j come from seed + rank and j alone, so a run is
        reproducible for a given n_samples, world size and seed; with design = (kind, block, K) every sub-batch takes its
        window of the one global design, and with (kind, block, K, s) the run is the columns s .. s + n_samples - 1 of a design
        of s + n_samples columns), every one handed to erpl_mc_submit_batch as soon as it is drawn: generation, up
        to `depth` integrations and their tails overlap on the GPU.  `submitted(a, cnt, db, outs)` is called behind the
        submission of the sub-batch of cnt samples at offset a (outs: its summary and status tensors, not yet written);
        `retired(a, cnt, ticket, outs)`, if given, once ITS ticket has been checked - the batch has finished - and before
        its inputs and, unless the caller kept them, its outputs go back to the allocator.  Returns the seconds spent
        drawing, with every batch finished and checked (raises if a lane hand-over timed out)."""
        from . import sampling
        m = max(hi - lo, 1)
        gen_s = 0.0
        inflight = []
        starts = list(range(0, m, self.DEVICE_CHUNK))
        # Sub-batches drawn before any of them is submitted: a sample budget (4 M samples, ~10 GB of wind tables at
        # K = 100), not a count.  A generation kernel enqueued behind a running flight launch waits for its waves to
        # drain, so a group is drawn on an idle stream first (1.5 ms per sub-batch) and then handed over in one go;
        # the next group is drawn while the tails of this one fly.  A sub-batch's inputs are released as soon as ITS
        # ticket has been checked (erpl_mc_check_batch waits for that batch alone).
        GROUP = max(1, (4 << 20) // self.DEVICE_CHUNK)
        keep = 2 * eng.get_overlap() + GROUP

        def retire(ticket, a, cnt, inputs, outs):
            eng.check(ticket)     # only once the batch has finished may its inputs go back to the allocator
            if retired is not None:
                retired(a, cnt, ticket, outs)

        for g0 in range(0, len(starts), GROUP):
            tg = time.time()
            group = []
            for j in range(g0, min(g0 + GROUP, len(starts))):
                a = starts[j]
                cnt = min(self.DEVICE_CHUNK, m - a)
                draws = None
                if design is not None:   # this sub-batch's window of the global design (a rank without samples: any column)
                    kind, block, K = design[:3]
                    s0 = design[3] if len(design) > 3 else 0
                    draws = sampling.design_draws(s0 + n_samples, K, eng.device, seed, design=kind, block=block,
                                                  first=s0 + min(lo + a, n_samples - cnt), count=cnt, engine=eng)
                group.append((a, cnt, sampling.synthetic_dispersions(
                    cnt, self.rocket, self.motor, self.wind_model, initial_conditions, eng.device,
                    precision=prec, seed=seed + rank + 1000003 * j, uncertainty=self.uncertainty_params,
                    base_altitude_profile=self.base_altitude_profile, base_wind_profile=self.base_wind_profile,
                    planar=planar, engine=eng, draws=draws)))
            gen_s += time.time() - tg
            for a, cnt, db in group:
                outs = eng.submit(db)
                submitted(a, cnt, db, outs)
                inflight.append((eng.last_ticket, a, cnt, db, outs if retired is not None else None))    # inputs outlive their batch
            del group, db, outs
            while len(inflight) > keep:
                retire(*inflight.pop(0))
        eng.wait()
        eng.check()                # host-blocking; raises if a lane hand-over timed out
        while inflight and retired is not None:
            retire(*inflight.pop(0))
        inflight.clear()
        return gen_s

    def run_monte_carlo_device(self, initial_conditions, n_samples, seed=1234, precision="f64_fast", planar=False,
                               keep_factors=False, design=None, design_replicates=1):
        """Throughput form for 100 k - 10 M samples (BASELINE configs 3-5): dispersions are drawn on the
        device (`sampling.synthetic_dispersions`, same distributions, torch generator), each rank
        integrates `n_samples / world` of them, summaries are all-gathered and the outlier filter +
        statistics run on the device (`analysis.device_statistics`).  Returns the statistics part of
        the analysis dict plus the gathered tensors; no per-sample dicts.

        precision: "f64_fast" (default) gives the reference's `apogee_altitude` - the global argmax over all
        steps, simulator.py:488-490 - end reason and step count on every sample of the parity sets (its blow-ups
        finish in the reference-order kernel), and with them the reference's outlier filter and statistics;
        "f32" is ~2.7x faster but on diverging samples only its `first_apogee_altitude` is within 0.1 % (its
        `apogee_altitude` on ~17 %, its end reason on ~52 %: DESIGN.md section 5), so n_outliers and the
        statistics differ from the reference's; "f64" runs everything in the reference-order gate kernel.

        keep_factors=True keeps the per-sample draws (`sampling.FACTOR_NAMES`) and adds out["factors"] (float64
        [F, n_samples] on the device, sample order of out["summary"]) and out["factor_names"], the input of
        `analysis.drivers`.  One rank only: factors are not gathered across ranks (ValueError before any work).

        design: None (the draws above: the reference's JOINT law from torch's generator, sub-batch j from
        seed + rank + 1000003 * j, bit for bit as before), or 'random', 'lhs', 'lhs_centred' or 'qmc': the run flies ONE global
        design of n_samples columns (`sampling.design_draws`, erpl_mc_design, erpl_mc_qmc) of which every rank and every sub-batch
        generates its own window, so its inputs depend on (seed, n_samples, design, design_replicates) alone and not on the
        world size or on DEVICE_CHUNK.  Such a run is drawn under the INDEPENDENT law of
        `sampling.synthetic_dispersions(draws=...)` - a deliberate deviation from the reference's joint law, as in
        `sobol_indices`: a design stratifies every primitive by itself, and under the joint law one normal is the thrust
        multiplier, `position_x` and the first turbulence innovation at once.  'lhs' stratifies each of the 17 + 3 K + 2
        primitives (Latin hypercube sampling: the variance of the mean of a near-additive output such as the apogee falls
        well below the i.i.d. one).  'qmc' is a scrambled Sobol' design (erpl_mc_qmc) on the dimensions of
        `sampling.qmc_dims`: it balances the low-order interactions of the primitives too, and its replicates are
        independently scrambled nets.  design_replicates = R splits the design into R independent Latin hypercubes of
        n_samples / R columns each (ValueError if R does not divide n_samples): `analysis.replicate_intervals` with
        block = n_samples / R gives the valid error bar of such a run, which the columns of ONE hypercube cannot give.
        out["design"] records kind, seed, block and replicates."""
        from . import sampling
        if keep_factors and dist.world()[1] > 1:
            raise ValueError("keep_factors=True is limited to a world size of 1: factors are not gathered across ranks")
        if design is not None:
            if design not in _abi.DESIGN_KINDS:
                raise ValueError(f"design: None or one of {list(_abi.DESIGN_KINDS)}")
            design_replicates = int(design_replicates)
            if design_replicates < 1 or n_samples % design_replicates != 0:
                raise ValueError(f"design_replicates = {design_replicates} does not divide n_samples = {n_samples}")
            design_block = n_samples // design_replicates
            use_base = self.base_wind_profile is not None and self.base_altitude_profile is not None
            design_K = len(self.base_altitude_profile) if use_base else 100   # synthetic_dispersions' default grid
        eng = shared_engine(self.device)
        eng.set_config(self._config())
        rank, ws = dist.world()
        lo, hi, _ = dist.shard_bounds(n_samples, rank, ws)
        prec = _abi.PRECISIONS[precision]
        torch.cuda.synchronize(eng.device)
        t0 = time.time()
        parts, fparts, fnames = [], [], None
        err, gen_s = None, 0.0

        def submitted(a, cnt, db, outs):
            nonlocal fnames
            parts.append(outs)
            if keep_factors:
                fparts.append(db.factors)
                fnames = db.factor_names

        try:
            gen_s = self._fly_sub_batches(eng, initial_conditions, n_samples, lo, hi, rank, seed, prec, planar,
                                          None if design is None else (design, design_block, design_K), submitted)
            summ = parts[0][0] if len(parts) == 1 else torch.cat([p[0] for p in parts], dim=1)
            status = parts[0][1] if len(parts) == 1 else torch.cat([p[1] for p in parts])
            summ, status = summ[:, : hi - lo], status[: hi - lo]
        except Exception as e:   # noqa: BLE001 - re-raised below
            if ws == 1:
                raise
            # the other ranks are waiting in the all-gather: take part with a shard marked incomplete, then raise
            err = e
            torch.cuda.synchronize(eng.device)
            summ, status = dist.failed_shard(hi - lo)
            if summ.device != eng.device and torch.distributed.get_backend() == "nccl":
                summ, status = summ.to(eng.device), status.to(eng.device)
        summ, status = dist.all_gather_summaries(summ, status, n_samples)
        if err is not None:
            raise err
        if ws > 1:
            TrajectoryEngine.raise_if_incomplete(status)   # another rank's shard failed: every rank refuses the result
        torch.cuda.synchronize(eng.device)
        t2 = time.time()
        out = analysis.device_statistics(summ, status)
        torch.cuda.synchronize(eng.device)
        t3 = time.time()
        out["summary"], out["status"] = summ, status
        if keep_factors:
            fac = fparts[0] if len(fparts) == 1 else torch.cat(fparts, dim=1)
            out["factors"], out["factor_names"] = fac[:, : hi - lo].contiguous(), list(fnames)
        if design is not None:
            out["design"] = {"kind": design, "seed": int(seed), "block": design_block, "replicates": design_replicates}
        out["performance"] = {"total_time": t3 - t0, "simulations_per_second": n_samples / (t3 - t0), "gpus_used": ws,
                              "precision": precision, "generate_s": gen_s, "integrate_and_gather_s": t2 - t0 - gen_s,
                              "statistics_s": t3 - t2, "sub_batches": len(parts), "in_flight": eng.get_overlap()}
        return out

    @staticmethod
    def _check_first_sample(design, design_replicates, n_samples, first_sample):
        """The refusals of `run_monte_carlo_tally(first_sample=)`.  first_sample = 0 is every run there was before it: nothing
        is checked here, whatever n_samples is (a design's own limit of 2^31 - 1 columns is the library's to report)."""
        if first_sample == 0:
            return
        if design != "qmc" or int(design_replicates) != 1:
            raise ValueError("first_sample: only design='qmc' with one replicate is a sequence that can be continued; the columns "
                             "of every other design depend on n_samples")
        if first_sample < 0 or first_sample + n_samples >= 2 ** 31:
            raise ValueError(f"first_sample = {first_sample} is negative or first_sample + n_samples reaches 2^31")

    def run_monte_carlo_tally(self, initial_conditions, n_samples, tally=None, seed=1234, precision="f64_fast", planar=False,
                              design=None, design_replicates=1, first_sample=0):
        """`run_monte_carlo_device` for runs too long to keep: the same sub-batch loop, draws and seeds (bit for bit the same
        flights), but no summary is kept - every sub-batch is folded into a tally (erpl_mc_tally_add, first_id = its global
        sample index) as soon as its ticket has been checked, and its outputs are released with its inputs.  Device memory
        does not depend on n_samples.  Across ranks there is one all-gather of the state words, merged in rank order
        (erpl_mc_tally_merge: the bytes do not depend on that order); a failing rank still joins, with a state that makes
        every rank refuse the result.  tally: the spec (analysis.tally_spec; None: the library's defaults).  n_samples: up
        to 2^31 - 1 with a design, no limit but the int64 counts without one.
        first_sample = s (design='qmc' alone, one replicate; ValueError otherwise): the run is the columns s .. s + n_samples - 1
        of the ONE Sobol' sequence of `seed` (block 0, pad 'random': no column depends on the length), with those sample ids,
        so a tally merged (TrajectoryEngine.tally_merge) from the runs [0, n) and [n, 2 n) equals the tally of one run of
        2 n byte for byte: a run that proved too short is continued, not flown again.
        Returns the dict of analysis.tally_statistics plus 'spec', 'state' (the int64 device tensor: equal runs give equal
        bytes, and with a design they do not depend on DEVICE_CHUNK or on the world size), 'result' (the dict of
        TrajectoryEngine.tally_result), 'n_total', 'seed', 'precision', 'planar', 'initial_conditions', 'design' (None, or
        kind / seed / block / replicates: what `refly` needs), 'first_sample' and 'performance' (with 'peak_memory_bytes')."""
        n_samples, first_sample = int(n_samples), int(first_sample)
        self._check_first_sample(design, design_replicates, n_samples, first_sample)
        design_args = None
        if design is not None:
            if design not in _abi.DESIGN_KINDS:
                raise ValueError(f"design: None or one of {list(_abi.DESIGN_KINDS)}")
            design_replicates = int(design_replicates)
            if design_replicates < 1 or n_samples % design_replicates != 0:
                raise ValueError(f"design_replicates = {design_replicates} does not divide n_samples = {n_samples}")
            use_base = self.base_wind_profile is not None and self.base_altitude_profile is not None
            design_args = (design, n_samples // design_replicates, len(self.base_altitude_profile) if use_base else 100)
            if first_sample:
                design_args = (design, 0, design_args[2], first_sample)
        eng = shared_engine(self.device)
        eng.set_config(self._config())
        spec, state = eng.tally_new(tally)
        rank, ws = dist.world()
        lo, hi, _ = dist.shard_bounds(n_samples, rank, ws)
        prec = _abi.PRECISIONS[precision]
        torch.cuda.synchronize(eng.device)
        torch.cuda.reset_peak_memory_stats(eng.device)
        t0 = time.time()
        n_sub = [0]

        def retired(a, cnt, ticket, outs):
            n_sub[0] += 1
            use = min(cnt, hi - lo - a)   # a rank without samples flies one column that is not tallied
            if use > 0:
                eng.wait(ticket)          # orders the finished batch into the current stream
                eng.tally_add(spec, state, outs[0], outs[1], first_id=first_sample + lo + a, n=use)

        err, gen_s = None, 0.0
        try:
            gen_s = self._fly_sub_batches(eng, initial_conditions, n_samples, lo, hi, rank, seed, prec, planar, design_args,
                                          lambda a, cnt, db, outs: None, retired)
        except Exception as e:   # noqa: BLE001 - re-raised below
            if ws == 1:
                raise
            # the other ranks are waiting in the all-gather: take part with a state marked incomplete, then raise
            err = e
            torch.cuda.synchronize(eng.device)
            state.zero_()
            state[14] = max(hi - lo, 1)   # n_incomplete: every rank's tally_result refuses
        if ws > 1:
            nccl = torch.distributed.get_backend() == "nccl"
            mine = state if nccl else state.cpu()
            gathered = torch.empty((ws * mine.numel(),), dtype=torch.int64, device=mine.device)
            torch.distributed.all_gather_into_tensor(gathered, mine)
            gathered = gathered.to(eng.device).view(ws, -1)
            state = torch.zeros_like(state)
            for r in range(ws):
                eng.tally_merge(spec, state, gathered[r].contiguous())
        if err is not None:
            raise err
        result = eng.tally_result(spec, state)   # blocks; raises _abi.IncompleteBatch if a shard failed
        t1 = time.time()
        out = analysis.tally_statistics(result)
        out.update({"spec": spec, "state": state, "result": result, "n_total": n_samples, "seed": int(seed), "precision": precision,
                    "planar": bool(planar), "initial_conditions": dict(initial_conditions), "design": None,
                    "first_sample": first_sample})
        if design is not None:
            out["design"] = {"kind": design, "seed": int(seed), "block": design_args[1], "replicates": design_replicates}
        out["performance"] = {"total_time": t1 - t0, "simulations_per_second": n_samples / (t1 - t0), "gpus_used": ws,
                              "precision": precision, "generate_s": gen_s, "sub_batches": n_sub[0], "in_flight": eng.get_overlap(),
                              "state_bytes": int(state.numel()) * 8,
                              "peak_memory_bytes": int(torch.cuda.max_memory_allocated(eng.device))}
        return out

    def refly(self, run, ids, stride=10, initial_conditions=None):
        """Flies named samples of a design run again, with capture: `run` is the dict of `run_monte_carlo_tally` (or any
        dict with its keys 'design', 'n_total', 'precision', 'planar', 'initial_conditions' and, for a continued run,
        'first_sample'), `ids` global sample ids - the ids a tally holds with its extremes.  Column i of a design run is a function of (seed, n, design, i) alone
        (erpl_mc_design, erpl_mc_qmc), so the named columns are generated again (`sampling.design_draws(first=id, count=1)`) and flown
        with every `stride`-th step captured.  Returns {'ids', 'summary' float64 [16, len(ids)], 'status', 'traj',
        'traj_len', 'stride'} on the device: the input of TrajectoryEngine.flight_envelope / corridor_resample on the worst
        cases.  A run with design=None cannot be re-flown: its draws come per sub-batch from torch's generator, so a column
        is no function of its id (ValueError)."""
        from . import sampling
        design = run.get("design")
        if design is None:
            raise ValueError("refly needs a run flown with design='random', 'lhs', 'lhs_centred' or 'qmc': the draws of a design=None run "
                             "come per sub-batch from torch's generator, so a sample cannot be regenerated from its id")
        ids = [int(i) for i in ids]
        first_sample = int(run.get("first_sample", 0))
        n_total = first_sample + int(run["n_total"])       # the columns of the design the run is a window of
        if not ids or min(ids) < first_sample or max(ids) >= n_total:
            raise ValueError(f"ids: at least one, each in {first_sample}..{n_total - 1}")
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be at least 1")
        ic = run["initial_conditions"] if initial_conditions is None else initial_conditions
        eng = shared_engine(self.device)
        eng.set_config(self._config())
        use_base = self.base_wind_profile is not None and self.base_altitude_profile is not None
        K = len(self.base_altitude_profile) if use_base else 100
        draws = torch.cat([sampling.design_draws(n_total, K, eng.device, design["seed"], design=design["kind"], block=design["block"],
                                                 first=i, count=1, engine=eng) for i in ids], dim=1).contiguous()
        db = sampling.synthetic_dispersions(
            len(ids), self.rocket, self.motor, self.wind_model, ic, eng.device, precision=_abi.PRECISIONS[run["precision"]],
            seed=design["seed"], uncertainty=self.uncertainty_params, base_altitude_profile=self.base_altitude_profile,
            base_wind_profile=self.base_wind_profile, planar=run["planar"], engine=eng, draws=draws)
        dt = min(self.dt_initial, 0.005)
        cap = int(np.ceil(self.max_time / dt / stride)) + 4
        summ, status, traj, tlen = eng.run(db, traj_ids=np.arange(len(ids)), traj_stride=stride, traj_cap=cap)
        eng.synchronize()
        return {"ids": ids, "summary": summ, "status": status, "traj": traj, "traj_len": tlen, "stride": stride}

    def rare_event(self, initial_conditions, n_per_level=131072, p0=0.125, row="range", tail="upper", target=None, centre=None,
                   max_levels=12, rho=0.8, seed=1234, precision="f64_fast", planar=False, design="random", bounds=None):
        """P(row > target) at the 1e-5 .. 1e-7 level by subset simulation (analysis.subset_simulation over flights) instead of
        the 10^8 - 10^9 flights a tally needs: level 0 is the design run of n_per_level flights (`sampling.design_draws` at
        `seed`, the INDEPENDENT law of `synthetic_dispersions(draws=...)`, bit for bit the flights of
        `run_monte_carlo_device(design=design)`), every further level keeps the n_per_level * p0 flights that went furthest
        and grows each into a chain of 1 / p0 states whose candidates are flown in sub-batches of DEVICE_CHUNK.
        row / tail / centre: the limit state g - a summary row (ROW_NAMES or index), its 'upper' or 'lower' tail (g = -row),
        or with centre=(cx, cy) the miss distance of the impact point; a flight the outlier filter drops never counts
        (g = -inf).  target: in units of g (a lower tail: minus the value); None: max_levels levels and the curve down to
        p0^max_levels.  rho: the correlation of the proposal (scalar, per level or [levels][rows]).  bounds: the filter's
        bounds where they are not the defaults (the dict of TrajectoryEngine.analyze, e.g. {'max_range': 20000.0}).
        READ 'warnings' (printed when verbose): subset simulation reaches a tail that the bulk leads to by small steps.  Where the
        tail is a separate mode - the planar set's ranges beyond 60 km are freak flights, an island among the primitives - the
        chains stop moving (acceptance near 0), the levels slice one frozen sample, and the estimate falls below the truth by
        orders of magnitude with a small c.o.v.; such a tail needs `run_monte_carlo_tally`.
        ValueError before any work: 1 / p0 no integer >= 2, n_per_level * p0 no integer, a world size above 1 (the chains
        of a level are not split across ranks).
        Returns the dict of analysis.subset_simulation ('probability', 'cov', 'interval', 'levels', 'curve', 'population',
        'level0', 'evaluations', 'warnings', ...) plus 'conditional_inputs': for every scalar primitive of `sampling.scalar_primitives`
        its {'mean', 'std'} over the failure sample (the last population's columns with indicator 1), next to the (0, 1) of
        a normal and the (0.5, 0.289) of a uniform under the unconditional law - which input a failing flight needs;
        'spec', 'seed', 'precision', 'planar', 'design', 'kinds' and 'performance'.
        The primitives of the failure sample are returned (population['draws'], float64 [17 + 3 K + 2, n_per_level] on the
        device), so the failures can be flown again with capture, as `refly` does for a design run:
        `db = sampling.synthetic_dispersions(m, ..., draws=population['draws'][:, cols].contiguous())`, then
        `eng.run(db, traj_ids=np.arange(m), traj_stride=stride, traj_cap=cap)`."""
        from . import sampling
        steps = int(round(1.0 / float(p0)))
        if steps < 2 or abs(steps * float(p0) - 1.0) > 1e-12:
            raise ValueError(f"p0 = {p0}: 1 / p0 must be an integer >= 2")
        n_per_level = int(n_per_level)
        if n_per_level < steps or n_per_level % steps != 0:
            raise ValueError(f"n_per_level * p0 = {n_per_level} / {steps} must be an integer >= 1")
        if dist.world()[1] > 1:
            raise ValueError("rare_event is limited to a world size of 1: the chains of a level are not split across ranks")
        if design not in _abi.DESIGN_KINDS:
            raise ValueError(f"design: one of {list(_abi.DESIGN_KINDS)}")
        chains = n_per_level // steps
        eng = shared_engine(self.device)
        eng.set_config(self._config())
        prec = _abi.PRECISIONS[precision]
        use_base = self.base_wind_profile is not None and self.base_altitude_profile is not None
        K = len(self.base_altitude_profile) if use_base else 100
        kinds = [_abi.DESIGN_NORMAL] * (17 + 3 * K) + [_abi.DESIGN_UNIFORM] * 2
        spec = analysis.subset_spec(row=row, tail=tail, centre=centre, bounds=bounds)
        flown = [0]

        def evaluate(draws):
            """Flies the columns of `draws` in sub-batches of DEVICE_CHUNK; g from their summaries on the device."""
            c = int(draws.shape[1])
            parts, keep = [], []
            for a in range(0, c, self.DEVICE_CHUNK):
                cnt = min(self.DEVICE_CHUNK, c - a)
                db = sampling.synthetic_dispersions(
                    cnt, self.rocket, self.motor, self.wind_model, initial_conditions, eng.device, precision=prec, seed=seed,
                    uncertainty=self.uncertainty_params, base_altitude_profile=self.base_altitude_profile,
                    base_wind_profile=self.base_wind_profile, planar=planar, engine=eng, draws=draws[:, a:a + cnt].contiguous())
                parts.append(eng.submit(db))
                keep.append(db)                  # inputs outlive their batch
            eng.wait()
            eng.check()                          # host-blocking: only now may the inputs go back to the allocator
            flown[0] += c
            summ = parts[0][0] if len(parts) == 1 else torch.cat([p[0] for p in parts], dim=1)
            status = parts[0][1] if len(parts) == 1 else torch.cat([p[1] for p in parts])
            return eng.subset_limit_state(spec, summ, status), summ, status

        torch.cuda.synchronize(eng.device)
        t0 = time.time()
        draws0 = sampling.design_draws(n_per_level, K, eng.device, seed, design=design, engine=eng)
        out = analysis.subset_simulation(evaluate, draws0, kinds, chains=chains, steps=steps, target=target, max_levels=max_levels,
                                         rho=rho, seed=seed, engine=eng)
        if self.verbose:
            for text in out["warnings"]:
                print(f"rare_event: {text}")
        pop = out["population"]
        fail = pop["indicator"].bool()
        n_fail = int(fail.sum())
        cond = {}
        liquid = flatten.motor_kind(self.motor) != _abi.MOTOR_SOLID
        for name, r in sampling.scalar_primitives(K, liquid).items():
            x = pop["draws"][r][fail]
            uniform = kinds[r] == _abi.DESIGN_UNIFORM
            cond[name] = {"row": int(r), "mean": float(x.mean()) if n_fail else float("nan"),
                          "std": float(x.std(unbiased=False)) if n_fail else float("nan"),
                          "unconditional": (0.5, math.sqrt(1.0 / 12.0)) if uniform else (0.0, 1.0)}
        torch.cuda.synchronize(eng.device)
        t1 = time.time()
        out.update({"conditional_inputs": cond, "n_failures": n_fail, "spec": spec, "seed": int(seed), "precision": precision,
                    "planar": bool(planar), "design": design, "kinds": kinds, "n_per_level": n_per_level, "p0": 1.0 / steps,
                    "row": analysis.ROW_NAMES[spec.row] if centre is None else "miss_distance", "tail": tail,
                    "initial_conditions": dict(initial_conditions),
                    "performance": {"total_time": t1 - t0, "evaluations": out["evaluations"], "flights": flown[0],
                                    "flights_per_second": flown[0] / (t1 - t0), "precision": precision}})
        return out

    def plot_rare_event(self, result, save_plots=True, tally=None):
        """The exceedance curve of `rare_event` on a log axis with its band and the level thresholds, optionally over the
        exceedance of a tally run of the same row (plots.rare_event_figure)."""
        return plots.plot_rare_event(self, result, save_plots, tally)

    def plot_exceedance(self, tally, row="range", save_plots=True, level=0.95):
        """The complementary distribution of a tallied row on a log axis, from the dict of `run_monte_carlo_tally`
        (plots.plot_exceedance)."""
        from . import plots
        return plots.plot_exceedance(self, tally, row, save_plots, level)

    def flight_envelope(self, initial_conditions, n_samples, stride=10, seed=1234, precision="f64_fast", planar=False,
                        capture_bytes=4 << 30, design=None):
        """What the vehicle goes through on the way up, for every sample of a dispersion run: the samples of
        `run_monte_carlo_device` (same draws: sub-batch j from seed + rank + 1000003 * j) are flown with EVERY trajectory
        captured at every `stride`-th step and each capture is reduced on the device to its flight envelope
        (TrajectoryEngine.flight_envelope: max-Q and where it falls, maximum Mach number, q-alpha, axial acceleration,
        smallest stability margin, burnout state, ...).  The envelope is that of the stored records: stride = 1 is the
        flight's own, a larger stride can miss a peak between two records.

        A capture holds cap * 120 bytes per sample, cap = the records a flight to max_time can write at this stride, so
        no capture can overflow; a sub-batch has capture_bytes // (cap * 120) samples (at most DEVICE_CHUNK) and its
        capture buffer is released as soon as its envelope is computed.  One rank only: envelopes are not gathered across
        ranks (ValueError before any work).

        Returns a dict: 'summary' [16, n] / 'status' [n] of the capturing run itself (where the sub-batches coincide these
        are run_monte_carlo_device's: bit for bit with precision="f64" and, measured, on planar "f64_fast" sets; on
        diverging "f64_fast" samples to 5e-8 relative with the same end reasons, because the capture instantiation of the
        throughput build fuses a few products differently - DESIGN.md section 4), 'envelope' float64 [16, n] on the
        device with 'envelope_names' (analysis.ENVELOPE_NAMES, rows _abi.ENV_*), 'reasons' (uint8 [n], the outlier
        filter's reason bits), 'n_samples' / 'n_outliers' of that filter, 'statistics' (analysis.envelope_statistics
        over the samples that pass it) and 'performance'.

        design: None (the draws above), or 'random', 'lhs', 'lhs_centred' or 'qmc': the run flies ONE design of n_samples columns
        under the independent law, as `run_monte_carlo_device(design=...)` does, every sub-batch its own window of it, so its
        inputs no longer depend on `capture_bytes`; the result carries 'design' and can be reweighted, fitted (`surrogate`)
        and flown again (`refly`) like a device run."""
        envs = []
        eng, summ, status, run = self._captured_run(
            "flight_envelope", "envelopes", initial_conditions, n_samples, stride, seed, precision, planar, capture_bytes,
            lambda eng, db, a, traj, tlen: envs.append(eng.flight_envelope(db, eng._keep, traj, tlen)), design=design)
        env = envs[0] if len(envs) == 1 else torch.cat(envs, dim=1).contiguous()
        torch.cuda.synchronize(eng.device)
        t1 = time.time()
        _, res, why = analysis._filter(summ, status, eng)
        out = {"summary": summ, "status": status, "envelope": env, "envelope_names": list(analysis.ENVELOPE_NAMES),
               "reasons": why, "n_samples": int(res.n_valid), "n_outliers": int(res.n_outliers),
               "statistics": analysis.envelope_statistics(env, why, engine=eng)}
        t2 = time.time()
        out["performance"] = {"total_time": t2 - run["t0"], "capture_and_envelope_s": t1 - run["t0"], "statistics_s": t2 - t1,
                              "precision": precision, "stride": run["stride"], "records_per_sample": run["cap"],
                              "sub_batches": len(envs), "sub_batch_samples": run["per_batch"]}
        if run["design"] is not None:
            out["design"] = run["design"]
        return out

    def _captured_run(self, who, what, initial_conditions, n_samples, stride, seed, precision, planar, capture_bytes, reduce,
                      factors=None, design=None):
        """The capturing loop of `flight_envelope`, `trajectory_corridor` and `impact_point_trace`: the samples of run_monte_carlo_device (sub-batch
        j from seed + rank + 1000003 * j) flown with every trajectory captured at every `stride`-th step, in sub-batches of
        capture_bytes // (cap * 120) samples (at most DEVICE_CHUNK); `reduce(eng, db, first_sample, traj, traj_len)`
        enqueues what the caller makes of a sub-batch's capture, and the capture buffer is released behind it.  One rank
        only (`who` / `what` word the refusal).  factors: a list that receives (db.factors, db.factor_names) of every sub-batch
        - the draws are otherwise released with the sub-batch.  design: None (those draws, bit for bit), or a kind of
        _abi.DESIGN_KINDS: sub-batch [a, a + nb) takes the columns a .. a + nb - 1 of ONE design of n_samples columns
        (`sampling.design_draws`, the independent law, K as `run_monte_carlo_device` chooses it), so the inputs of the run no
        longer depend on `capture_bytes`; an unknown kind is a ValueError before the engine is created.  Returns (engine,
        summary [16, n], status [n], {'t0', 'stride', 'cap', 'per_batch', 'sub_batches', 'design'}) once everything has run;
        'design' is None or the {'kind', 'seed', 'block', 'replicates'} entry of a design run."""
        from . import sampling
        if design is not None and design not in _abi.DESIGN_KINDS:
            raise ValueError(f"design: None or one of {list(_abi.DESIGN_KINDS)}")
        if dist.world()[1] > 1:
            raise ValueError(f"{who} is limited to a world size of 1: {what} are not gathered across ranks")
        n_samples, stride = int(n_samples), int(stride)
        if n_samples < 1 or stride < 1:
            raise ValueError("n_samples and stride must be at least 1")
        eng = shared_engine(self.device)
        eng.set_config(self._config())
        rank = dist.world()[0]
        prec = _abi.PRECISIONS[precision]
        dt = min(self.dt_initial, 0.005)
        cap = int(np.ceil(self.max_time / dt / stride)) + 4
        per_batch = max(1, min(self.DEVICE_CHUNK, int(capture_bytes) // (cap * _abi.TRAJ_DIM * 8)))
        if design is not None:
            use_base = self.base_wind_profile is not None and self.base_altitude_profile is not None
            design_K = len(self.base_altitude_profile) if use_base else 100   # synthetic_dispersions' default grid
        torch.cuda.synchronize(eng.device)
        t0 = time.time()
        summs, stats = [], []
        for j, a in enumerate(range(0, n_samples, per_batch)):
            nb = min(per_batch, n_samples - a)
            draws = None
            if design is not None:   # this sub-batch's window of the one design of the run
                draws = sampling.design_draws(n_samples, design_K, eng.device, seed, design=design, block=n_samples, first=a, count=nb,
                                              engine=eng)
            db = sampling.synthetic_dispersions(
                nb, self.rocket, self.motor, self.wind_model, initial_conditions, eng.device, precision=prec,
                seed=seed + rank + 1000003 * j, uncertainty=self.uncertainty_params,
                base_altitude_profile=self.base_altitude_profile, base_wind_profile=self.base_wind_profile,
                planar=planar, engine=eng, draws=draws)
            summ, status, traj, tlen = eng.run(db, traj_ids=np.arange(nb), traj_stride=stride, traj_cap=cap)
            reduce(eng, db, a, traj, tlen)
            if factors is not None:
                factors.append((db.factors, db.factor_names))
            summs.append(summ)
            stats.append(status)
            del traj, tlen, db   # (stream-ordered: the allocator hands the capture buffer on behind the caller's kernel)
        eng.synchronize()        # host-blocking; raises if a lane hand-over timed out
        cat = lambda parts, dim: parts[0] if len(parts) == 1 else torch.cat(parts, dim=dim).contiguous()
        record = None if design is None else {"kind": design, "seed": int(seed), "block": n_samples, "replicates": 1}
        return eng, cat(summs, 1), cat(stats, 0), {"t0": t0, "stride": stride, "cap": cap, "per_batch": per_batch,
                                                   "sub_batches": len(summs), "design": record}

    @staticmethod
    def _kept_factors(out, kept):
        """out['factors'] ([F, n] on the device, the sample order of out['summary']) and out['factor_names'] from what
        `_captured_run` collected per sub-batch."""
        out["factors"] = kept[0][0].contiguous() if len(kept) == 1 else torch.cat([f for f, _ in kept], dim=1).contiguous()
        out["factor_names"] = list(kept[0][1])

    def trajectory_corridor(self, initial_conditions, n_samples, stride=10, seed=1234, precision="f64_fast", planar=False,
                            capture_bytes=4 << 30, nodes=256, t_end=None, channels=("z", "downrange", "speed"),
                            quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), hold=True, keep_factors=False, design=None):
        """Where the vehicle is at time t and how wide the spread is there, for a whole dispersion run: the samples of
        `flight_envelope` (same draws, same sub-batches, every trajectory captured at every `stride`-th step) are brought
        onto `nodes` time nodes from 0 to `t_end` (default max_time) on the device, each sub-batch into its window of
        columns of one [C, T, n] matrix (TrajectoryEngine.corridor_resample; the capture is released behind the kernel),
        and every (channel, node) row is described over the samples that pass the outlier filter by one
        erpl_mc_corridor_bands call.  channels: names of analysis.CORRIDOR_CHANNEL_NAMES; hold: a flight that has ended
        stays where it landed (its last record) instead of leaving the population - without it the bands behind the
        first landing describe the flights still in the air.  Values between two records are linear interpolations of
        the STORED records.  One rank only (ValueError before any work).

        Returns the dict of analysis.trajectory_corridor ('time', 'q', 'channels', per channel 'count' / 'mean' / 'std' /
        'min' / 'max' [T] and 'quantiles' [n_q, T]) plus 'summary', 'status', 'reasons', 'n_samples' / 'n_outliers' of the
        filter, 'values' (the resampled matrix, on the device) and 'performance'.  keep_factors=True keeps the per-sample
        draws and adds 'factors' (float64 [F, n] on the device, the sample order of 'summary') and 'factor_names', the input
        of `corridor_drivers`.  design: as in `flight_envelope` - with a design the inputs of the run do not depend on
        `capture_bytes`, the result carries 'design', and `reweighted_corridor` reports its bands under another input law."""
        nodes = int(nodes)
        if nodes < 2:
            raise ValueError("at least 2 nodes")
        t_end = float(self.max_time if t_end is None else t_end)
        if not (np.isfinite(t_end) and t_end > 0.0):
            raise ValueError("t_end must be finite and positive")
        idx = analysis.corridor_channels(channels)
        step = t_end / (nodes - 1)
        box = {}

        def resample(eng, db, a, traj, tlen):
            if "values" not in box:
                box["values"] = torch.full((len(idx), nodes, int(n_samples)), float("nan"), dtype=torch.float64,
                                           device=eng.device)
            eng.corridor_resample(traj, tlen, idx, nodes, 0.0, step, hold=hold, out=box["values"], col0=a)

        kept = [] if keep_factors else None
        eng, summ, status, run = self._captured_run("trajectory_corridor", "corridors", initial_conditions, n_samples,
                                                    stride, seed, precision, planar, capture_bytes, resample, factors=kept,
                                                    design=design)
        torch.cuda.synchronize(eng.device)
        t1 = time.time()
        _, res, why = analysis._filter(summ, status, eng)
        out = analysis.trajectory_corridor(box["values"], idx, 0.0, step, quantiles=quantiles, mask=why, engine=eng)
        t2 = time.time()
        out.update({"summary": summ, "status": status, "reasons": why, "values": box["values"],
                    "n_samples": int(res.n_valid), "n_outliers": int(res.n_outliers)})
        if keep_factors:
            self._kept_factors(out, kept)
        out["performance"] = {"total_time": t2 - run["t0"], "capture_and_resample_s": t1 - run["t0"], "bands_s": t2 - t1,
                              "precision": precision, "stride": run["stride"], "records_per_sample": run["cap"],
                              "sub_batches": run["sub_batches"], "sub_batch_samples": run["per_batch"]}
        if run["design"] is not None:
            out["design"] = run["design"]
        return out

    def impact_point_trace(self, initial_conditions, n_samples, stride=10, nodes=64, record_stride=None, keep_in=None,
                           seed=1234, precision="f64_fast", planar=False, capture_bytes=4 << 30, dt=0.05, max_steps=20000,
                           ground=0.0, drag_scale=1.0, origin=(0.0, 0.0), quantiles=(0.05, 0.25, 0.5, 0.75, 0.95),
                           level=0.95, keep_factors=False, design=None):
        """If the flight is terminated at time t, where does the vehicle come down - for a whole dispersion run: the samples
        of `flight_envelope` (same draws, same sub-batches, every trajectory captured at every `stride`-th step) and, of each
        capture, `nodes` records `record_stride` apart (None: the stride that spreads the nodes over max_time) fall to
        z = `ground` without thrust on the device (TrajectoryEngine.impact_points: frozen mass, zero-incidence power-off
        drag times drag_scale, the sample's own wind, no parachute; dt / max_steps bound the fall), each sub-batch into its
        window of columns of one [5, nodes, n] matrix; the capture is released behind the kernel.  keep_in: a keep-in
        polygon of 3 to 64 (x, y) vertices or None.  One rank only (ValueError before any work).

        Returns a dict: 'time' [nodes] (the nominal time of node k since rail exit, k * record_stride * stride * dt_flight),
        'q', 'channels' (analysis.IIP_CHANNELS) and per channel 'count' / 'mean' / 'std' / 'min' / 'max' [nodes] and
        'quantiles' [n_q, nodes] over the samples that pass the outlier filter (erpl_mc_corridor_bands on the IIP matrix);
        'statistics' (analysis.impact_point_statistics of the summary rows over the same samples); 'exit_probability', the
        share of those samples whose IIP ever leaves the keep-in area, with its Wilson interval 'exit_interval' at `level`
        (NaN and (0, 1) without a polygon) and 'exit_count'; 'values' and 'iip_summary' (on the device), 'iip_names',
        'keep_in', 'summary', 'status', 'reasons', 'n_samples' / 'n_outliers' and 'performance'.  keep_factors=True adds
        'factors' and 'factor_names' as in `trajectory_corridor`.  design: as in `flight_envelope` - with a design the inputs
        of the run do not depend on `capture_bytes` and the result carries 'design'."""
        nodes, stride = int(nodes), int(stride)
        if not 1 <= nodes <= _abi.IIP_MAX_NODES:
            raise ValueError(f"1 to {_abi.IIP_MAX_NODES} nodes")
        if int(n_samples) < 1 or stride < 1:
            raise ValueError("n_samples and stride must be at least 1")
        flight_dt = min(self.dt_initial, 0.005)
        if record_stride is None:
            record_stride = max(1, int(np.ceil(self.max_time / flight_dt / stride)) // nodes)
        record_stride = int(record_stride)
        if record_stride < 1:
            raise ValueError("record_stride must be at least 1")
        keep = None if keep_in is None else [(float(x), float(y)) for x, y in keep_in]
        box, summaries = {}, []

        def fall(eng, db, a, traj, tlen):
            if "values" not in box:
                box["values"] = torch.full((_abi.IIP_CH_COUNT, nodes, int(n_samples)), float("nan"), dtype=torch.float64,
                                           device=eng.device)
            _, s = eng.impact_points(db, eng._keep, traj, tlen, nodes=nodes, record_stride=record_stride, dt=dt,
                                     max_steps=max_steps, ground=ground, drag_scale=drag_scale, origin=origin, keep_in=keep,
                                     out=box["values"], col0=a)
            summaries.append(s)

        kept = [] if keep_factors else None
        eng, summ, status, run = self._captured_run("impact_point_trace", "impact points", initial_conditions, n_samples,
                                                    stride, seed, precision, planar, capture_bytes, fall, factors=kept,
                                                    design=design)
        iip = summaries[0] if len(summaries) == 1 else torch.cat(summaries, dim=1).contiguous()
        torch.cuda.synchronize(eng.device)
        t1 = time.time()
        _, res, why = analysis._filter(summ, status, eng)
        b = eng.corridor_bands(box["values"], why, quantiles=quantiles)
        out = {"time": np.arange(nodes, dtype=np.float64) * (record_stride * run["stride"] * flight_dt), "q": b["q"],
               "channels": list(analysis.IIP_CHANNELS), "n_counted": b["n_counted"]}
        for j, name in enumerate(analysis.IIP_CHANNELS):
            out[name] = {k: b[k][j] for k in ("count", "mean", "std", "min", "max", "quantiles")}
        out["statistics"] = analysis.impact_point_statistics(iip, why, engine=eng, quantiles=quantiles)
        counted = why == 0
        n_counted = int(counted.sum())
        n_exit = int((counted & torch.isfinite(iip[_abi.IIP_EXIT_TIME])).sum())
        out["exit_count"] = n_exit
        out["exit_probability"] = n_exit / n_counted if (keep is not None and n_counted) else float("nan")
        out["exit_interval"] = analysis.wilson_interval(n_exit, n_counted, level) if keep is not None else (0.0, 1.0)
        out["interval_level"] = float(level)
        t2 = time.time()
        out.update({"summary": summ, "status": status, "reasons": why, "values": box["values"], "iip_summary": iip,
                    "iip_names": list(analysis.IIP_NAMES), "keep_in": keep, "record_stride": record_stride,
                    "n_samples": int(res.n_valid), "n_outliers": int(res.n_outliers)})
        if keep_factors:
            self._kept_factors(out, kept)
        out["performance"] = {"total_time": t2 - run["t0"], "capture_and_fall_s": t1 - run["t0"], "statistics_s": t2 - t1,
                              "precision": precision, "stride": run["stride"], "records_per_sample": run["cap"],
                              "sub_batches": run["sub_batches"], "sub_batch_samples": run["per_batch"]}
        if run["design"] is not None:
            out["design"] = run["design"]
        return out

    def debris_footprint(self, initial_conditions, n_samples, fragments, stride=10, nodes=16, record_stride=None, keep_in=None,
                         maps=(), map_bins=50, seed=1234, debris_seed=None, precision="f64_fast", planar=False,
                         capture_bytes=4 << 30, dt=0.05, max_steps=20000, ground=0.0, stiff_limit=0.25, origin=(0.0, 0.0),
                         quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), level=0.95, keep_factors=False, design=None):
        """If the vehicle breaks up at time t, where do its pieces come down - for a whole dispersion run: the samples of
        `impact_point_trace` (same draws, same sub-batches, same nodes) and, at every node, the fragments
        `fragments` = [(beta, dv), ...] - beta the ballistic coefficient m / (Cd A) in kg/m^2 (float('inf'): no drag), dv the
        speed in m/s the break-up adds in an isotropic direction drawn from (debris_seed + 1000003 * sub-batch, sample of the
        sub-batch, node, fragment); debris_seed defaults to `seed` - fall to z = `ground` on the device (TrajectoryEngine.debris: gravity, the fragment's
        drag, the sample's own wind; RK4 steps of dt halved while drag rate * step exceeds stiff_limit), each sub-batch into
        its window of columns of one [5, nodes * F, n] matrix.  maps: (node, fragment) pairs whose footprint is wanted as a
        map_bins x map_bins count grid (erpl_mc_histogram_xy on the X and Y rows of that pair).  One rank only.  Because the draw's sample id
        is the index within the sub-batch and its seed carries the sub-batch number, the directions of a run depend on how it is
        cut into sub-batches (`capture_bytes`), exactly as its dispersions do: the same arguments give the same bytes, another
        `capture_bytes` another, equally valid, draw.  TrajectoryEngine.debris itself draws from (seed, id, node, fragment) alone.

        Returns a dict: 'time' [nodes], 'fragments', 'q', 'channels' and per channel 'count' / 'mean' / 'std' / 'min' /
        'max' [nodes, F] and 'quantiles' [n_q, nodes, F] over the samples that pass the outlier filter
        (erpl_mc_corridor_bands on the matrix as it is); 'statistics' (analysis.debris_statistics over the same samples);
        'exit_probability', the share of those samples with a fragment that lands outside the keep-in area, with its
        Wilson interval 'exit_interval' at `level` (NaN and (0, 1) without a polygon) and 'exit_count'; 'maps', a dict
        (node, fragment) -> {'counts', 'edges_x', 'edges_y', 'info'}; 'values' and 'debris_summary' (on the device),
        'debris_names', 'keep_in', 'summary', 'status', 'reasons', 'n_samples' / 'n_outliers' and 'performance'.
        keep_factors=True adds 'factors' and 'factor_names' as in `trajectory_corridor`.  design: as in `flight_envelope` - with
        a design the DISPERSIONS of the run do not depend on `capture_bytes` (the break-up directions still do, as said above)
        and the result carries 'design'."""
        nodes, stride = int(nodes), int(stride)
        frags = [(float(beta), float(dv)) for beta, dv in fragments]
        F = len(frags)
        if not 1 <= F <= _abi.DEBRIS_MAX_FRAGMENTS:
            raise ValueError(f"1 to {_abi.DEBRIS_MAX_FRAGMENTS} fragments")
        if not 1 <= nodes <= _abi.IIP_MAX_NODES or nodes * F > _abi.CORRIDOR_MAX_NODES:
            raise ValueError(f"1 to {_abi.IIP_MAX_NODES} nodes, at most {_abi.CORRIDOR_MAX_NODES} nodes * fragments")
        for beta, dv in frags:
            if not beta > 0.0 or not (np.isfinite(dv) and dv >= 0.0):
                raise ValueError("a fragment needs beta > 0 and a finite dv >= 0")
        if int(n_samples) < 1 or stride < 1:
            raise ValueError("n_samples and stride must be at least 1")
        flight_dt = min(self.dt_initial, 0.005)
        if record_stride is None:
            record_stride = max(1, int(np.ceil(self.max_time / flight_dt / stride)) // nodes)
        record_stride = int(record_stride)
        if record_stride < 1:
            raise ValueError("record_stride must be at least 1")
        maps = [(int(k), int(f)) for k, f in maps]
        for k, f in maps:
            if not (0 <= k < nodes and 0 <= f < F):
                raise ValueError(f"map ({k}, {f}): node below {nodes} and fragment below {F}")
        keep = None if keep_in is None else [(float(x), float(y)) for x, y in keep_in]
        debris_seed = int(seed if debris_seed is None else debris_seed)
        box, summaries = {}, []

        def fall(eng, db, a, traj, tlen):
            if "values" not in box:
                box["values"] = torch.full((_abi.IIP_CH_COUNT, nodes * F, int(n_samples)), float("nan"), dtype=torch.float64,
                                           device=eng.device)
            # (a sub-batch numbers its samples from 0: sub-batch j draws under debris_seed + 1000003 * j, as its dispersions do)
            _, s = eng.debris(db, eng._keep, traj, tlen, frags, nodes=nodes, record_stride=record_stride, dt=dt,
                              max_steps=max_steps, ground=ground, stiff_limit=stiff_limit,
                              seed=debris_seed + 1000003 * len(summaries), origin=origin, keep_in=keep, out=box["values"], col0=a)
            summaries.append(s)

        kept = [] if keep_factors else None
        eng, summ, status, run = self._captured_run("debris_footprint", "debris footprints", initial_conditions, n_samples,
                                                    stride, seed, precision, planar, capture_bytes, fall, factors=kept,
                                                    design=design)
        deb = summaries[0] if len(summaries) == 1 else torch.cat(summaries, dim=1).contiguous()
        torch.cuda.synchronize(eng.device)
        t1 = time.time()
        _, res, why = analysis._filter(summ, status, eng)
        vals = box["values"]
        b = eng.corridor_bands(vals, why, quantiles=quantiles)
        out = {"time": np.arange(nodes, dtype=np.float64) * (record_stride * run["stride"] * flight_dt), "q": b["q"],
               "fragments": frags, "channels": list(analysis.DEBRIS_CHANNELS), "n_counted": b["n_counted"]}
        for j, name in enumerate(analysis.DEBRIS_CHANNELS):
            out[name] = {k: b[k][j].reshape(nodes, F) for k in ("count", "mean", "std", "min", "max")}
            out[name]["quantiles"] = b["quantiles"][j].reshape(-1, nodes, F)
        out["statistics"] = analysis.debris_statistics(deb, why, engine=eng, quantiles=quantiles)
        counted = why == 0
        n_counted = int(counted.sum())
        n_exit = int((counted & torch.isfinite(deb[_abi.DEBRIS_EXIT_TIME])).sum())
        out["exit_count"] = n_exit
        out["exit_probability"] = n_exit / n_counted if (keep is not None and n_counted) else float("nan")
        out["exit_interval"] = analysis.wilson_interval(n_exit, n_counted, level) if keep is not None else (0.0, 1.0)
        out["interval_level"] = float(level)
        out["maps"] = {}
        for k, f in maps:
            pair = torch.zeros((_abi.SUMMARY_DIM, int(n_samples)), dtype=torch.float64, device=eng.device)
            pair[0], pair[1] = vals[_abi.IIP_CH_X, k * F + f], vals[_abi.IIP_CH_Y, k * F + f]
            counts, ex, ey, info = eng.histogram2d(pair, why, 0, 1, bins=map_bins)
            out["maps"][(k, f)] = {"counts": counts, "edges_x": ex, "edges_y": ey, "info": info}
        t2 = time.time()
        out.update({"summary": summ, "status": status, "reasons": why, "values": vals, "debris_summary": deb,
                    "debris_names": list(analysis.DEBRIS_NAMES), "keep_in": keep, "record_stride": record_stride,
                    "debris_seed": debris_seed, "n_samples": int(res.n_valid), "n_outliers": int(res.n_outliers)})
        if keep_factors:
            self._kept_factors(out, kept)
        out["performance"] = {"total_time": t2 - run["t0"], "capture_and_fall_s": t1 - run["t0"], "statistics_s": t2 - t1,
                              "precision": precision, "stride": run["stride"], "records_per_sample": run["cap"],
                              "sub_batches": run["sub_batches"], "sub_batch_samples": run["per_batch"]}
        if run["design"] is not None:
            out["design"] = run["design"]
        return out

    def corridor_drivers(self, captured, regression=True):
        """Which dispersion drives what, and when (no reference counterpart): the dict of `trajectory_corridor`,
        `impact_point_trace` or `debris_footprint` flown with keep_factors=True - its 'values', 'reasons' (the mask),
        'factors' and 'factor_names' are read - through `analysis.corridor_drivers`: per channel, node and factor the
        correlation and the standardised regression coefficient over the flights that pass the outlier filter and are still
        defined at that node, with 'share', 'ranking' and 'lead'.  Without factors: a ValueError that names keep_factors=True."""
        from . import analysis as ana
        if "factors" not in captured or "factor_names" not in captured:
            raise ValueError("the captured run carries no factors: fly it with keep_factors=True")
        t = np.asarray(captured["time"], dtype=np.float64)
        out = ana.corridor_drivers(captured["values"], captured["factors"], captured["factor_names"],
                                   channels=list(captured["channels"]), t0=float(t[0]) if len(t) else 0.0,
                                   dt=float(t[1] - t[0]) if len(t) > 1 else 1.0, mask=captured["reasons"],
                                   engine=shared_engine(self.device), regression=regression)
        if "fragments" in captured:   # the rows of a debris matrix are (node, fragment) pairs: every time once per fragment
            out["fragments"] = captured["fragments"]
            out["time"] = np.repeat(t, len(captured["fragments"]))
        return out

    def plot_corridor_drivers(self, drivers, save_plots=True, top=4):
        """No reference counterpart: the result of `corridor_drivers` - per channel the signed correlation of the `top` factors
        over time and under it their stacked shares with r2 as the outline - as monte_carlo_corridor_drivers.png in the output
        directory (with save_plots); returns the figure."""
        return plots.plot_corridor_drivers(self, drivers, save_plots, top)

    def trajectory_depth(self, captured, central=0.5, factor=1.5):
        """Which flown trajectory is the typical one, and which flights are unusual as curves (no reference counterpart;
        analyze_outlier.py opens one flight by hand): the dict of `trajectory_corridor`, `impact_point_trace` or
        `debris_footprint` - its 'values', 'reasons' (the mask), 'time' and 'channels' are read - through
        `analysis.trajectory_depth`: per channel the band depth of every flight that passes the outlier filter, the deepest
        flight ('median', with 'median_curve'), the envelope of the `central` share of the flights, its fences `factor` envelope
        widths outside it, the flights that leave the fences and the flights the outliergram flags for their shape.  Columns
        are sample indices of captured['summary']: the median flight and the outliers can be flown again."""
        from . import analysis as ana
        t = np.asarray(captured["time"], dtype=np.float64)
        out = ana.trajectory_depth(captured["values"], channels=list(captured["channels"]), t0=float(t[0]) if len(t) else 0.0,
                                   dt=float(t[1] - t[0]) if len(t) > 1 else 1.0, mask=captured["reasons"],
                                   engine=shared_engine(self.device), central=central, factor=factor)
        if "fragments" in captured:   # the rows of a debris matrix are (node, fragment) pairs: every time once per fragment
            out["fragments"] = captured["fragments"]
            out["time"] = np.repeat(t, len(captured["fragments"]))
        return out

    def plot_functional_boxplot(self, depth, values=None, save_plots=True, most=20):
        """No reference counterpart: the result of `trajectory_depth` - per channel the central region as a band, the median
        flight as a line, the whiskers and (with `values`, the matrix the depth was taken of) up to `most` outlying flights
        drawn one by one - as monte_carlo_functional_boxplot.png in the output directory (with save_plots); returns the
        figure."""
        return plots.plot_functional_boxplot(self, depth, values, save_plots, most)

    def casualty_expectation(self, footprint, population, ranges, fragments, p_fail=None, failure_rate=None, ke_min=15.0,
                             smooth=True, bw_scale=1.0, h_floor=1.0, levels=(1e-6, 1e-5)):
        """The number a range signs (no reference counterpart): the casualty expectation Ec and the individual-risk map of
        the footprint `debris_footprint` returned - its 'values', 'reasons', 'time' and 'fragments' are read.  population:
        persons / m^2 on a [bins_x, bins_y] raster over ranges = ((lo_x, hi_x), (lo_y, hi_y)) (NumPy or device tensor);
        fragments: one (pieces, casualty area in m^2, mass in kg) per fragment class of the footprint; p_fail: the probability
        of a break-up per node, or failure_rate (1/s, a constant or one value per node) from which
        `analysis.failure_probabilities` makes them over footprint['time'].  A fragment is lethal from ke_min joules on.
        Returns the dict of `analysis.casualty_expectation`; its 'ec_traj' is a per-sample row for `confidence_intervals`
        (extra=...), `drivers` and `dependence`."""
        from . import analysis as ana
        frags = [tuple(float(v) for v in f) for f in fragments]
        if len(frags) != len(footprint["fragments"]):
            raise ValueError(f"the footprint has {len(footprint['fragments'])} fragment classes, {len(frags)} were given")
        if (p_fail is None) == (failure_rate is None):
            raise ValueError("give p_fail or failure_rate")
        times = np.asarray(footprint["time"], dtype=np.float64)
        if p_fail is None:
            p_fail = ana.failure_probabilities(times, failure_rate, t_end=None if len(times) > 1 else times[0] + 1.0)
        p_fail = np.asarray(p_fail, dtype=np.float64).reshape(-1)
        if len(p_fail) != len(times):
            raise ValueError(f"p_fail holds {len(p_fail)} values, the footprint has {len(times)} nodes")
        bins = tuple(population.shape) if hasattr(population, "shape") else np.asarray(population).shape
        if len(bins) != 2:
            raise ValueError("population must be a [bins_x, bins_y] raster")
        ana.casualty_spec(len(p_fail), frags, bins, ranges, ke_min, smooth, bw_scale, h_floor, levels)   # refuses before any device work
        return ana.casualty_expectation(footprint["values"], frags, p_fail, population, ranges, mask=footprint["reasons"],
                                        engine=shared_engine(self.device), times=times, ke_min=ke_min, smooth=smooth,
                                        bw_scale=bw_scale, h_floor=h_floor, levels=levels)

    def plot_casualty(self, casualty, save_plots=True):
        """No reference counterpart: the result of `casualty_expectation` - the smoothed risk map with its level contours
        over the population raster, Ec given a break-up at t, the contribution of every fragment class - as
        monte_carlo_casualty.png in the output directory; returns that directory."""
        return plots.plot_casualty(self, casualty, save_plots)

    def plot_debris_footprint(self, footprint, node=None, save_plots=True):
        """No reference counterpart: the footprint of `debris_footprint` - per fragment the median and the outer band of the
        impact range over the time of break-up, the footprint at `node` (default: the last one) with the keep-in outline - as
        monte_carlo_debris.png in the output directory; returns that directory."""
        return plots.plot_debris_footprint(self, footprint, node, save_plots)

    def plot_impact_point_trace(self, trace, save_plots=True):
        """No reference counterpart: the IIP trace of `impact_point_trace` - IIP range over time with its bands, the ground
        track of the median IIP with the keep-in outline, the exit times - as monte_carlo_impact_points.png in the output
        directory; returns that directory."""
        return plots.plot_impact_point_trace(self, trace, save_plots)

    def plot_trajectory_corridor(self, corridor, save_plots=True):
        """No reference counterpart: the corridor of `trajectory_corridor` - per channel the median, the outer and inner
        quantile bands and the sample count over time - as monte_carlo_corridor.png in the output directory; returns that
        directory."""
        return plots.plot_trajectory_corridor(self, corridor, save_plots)

    def run_optimized_monte_carlo(self, initial_conditions, n_samples=1000, chunk_size=None):
        return self.run_monte_carlo(initial_conditions, n_samples, optimized=True)

    def _create_output_directory(self):
        """monte_carlo.py:475-480."""
        return reports.create_output_directory()

    def _save_report(self, analysis, output_dir):
        """monte_carlo.py:482-560 (same files, keys and text format)."""
        return reports.save_report(self, analysis, output_dir)

    def plot_results(self, analysis, save_plots=True):
        """monte_carlo.py:562-633: the three histograms (counted on the device) and range vs apogee, saved as
        monte_carlo_distributions.png next to the report; prints the statistics; returns the output directory."""
        return plots.plot_results(self, analysis, save_plots)

    def plot_trajectory_cloud(self, analysis, save_plots=True, max_trajectories=50):
        """monte_carlo.py:635-677: monte_carlo_trajectories.png."""
        return plots.plot_trajectory_cloud(self, analysis, save_plots, max_trajectories)

    def plot_trajectory_cloud_3d(self, analysis, save_plots=True, max_trajectories=50):
        """monte_carlo.py:679-707: monte_carlo_trajectories_3d.png."""
        return plots.plot_trajectory_cloud_3d(self, analysis, save_plots, max_trajectories)

    def plot_landing_dispersion(self, analysis, save_plots=True, target=None):
        """No reference counterpart: impact footprint, confidence ellipses and CEP about `target` (default the launch
        site) as monte_carlo_landing.png, the numbers as landing_dispersion.json."""
        return plots.plot_landing_dispersion(self, analysis, save_plots, target)

    def drivers(self, analysis, rows=None):
        """Which dispersion drives which outcome (no reference counterpart; its authors dug through single samples by
        hand): `analysis.drivers` on either kind of analysis dict.  With 'factors' (run_monte_carlo_device(...,
        keep_factors=True)) everything stays on the device; otherwise the parameters of analysis['results'] are
        flattened with `analysis.factors_from_results` and uploaded."""
        from . import analysis as ana
        eng = shared_engine(self.device)
        if "factors" in analysis:
            return ana.drivers(analysis["summary"], analysis["factors"], analysis["factor_names"],
                               status=analysis.get("status"), engine=eng, rows=rows)
        fac, names = ana.factors_from_results(analysis["results"])
        summ = ana.summary_from_results(analysis["results"])
        return ana.drivers(torch.as_tensor(summ, device=eng.device).contiguous(),
                           torch.as_tensor(fac, device=eng.device).contiguous(), names, engine=eng, rows=rows)

    def confidence_intervals(self, analysis, replicates=2000, level=0.95, seed=0, extra=None):
        """How sure the statistics of an analysis are (no reference counterpart): `analysis.confidence_intervals` - bootstrap
        standard errors and percentile intervals of mean, std and the five percentiles of apogee, range and flight time -
        on either kind of analysis dict, as `drivers` takes its inputs: the device 'summary' / 'status' of
        run_monte_carlo_device, or the summary columns of analysis['results'] uploaded.  extra: one more per-sample row on
        the device (the 'ec_traj' of `casualty_expectation`), reported under 'extra'."""
        from . import analysis as ana
        eng = shared_engine(self.device)
        if "summary" in analysis:
            return ana.confidence_intervals(analysis["summary"], status=analysis.get("status"), engine=eng,
                                            replicates=replicates, level=level, seed=seed, extra=extra)
        summ = ana.summary_from_results(analysis["results"])
        return ana.confidence_intervals(torch.as_tensor(summ, device=eng.device).contiguous(), engine=eng,
                                        replicates=replicates, level=level, seed=seed)

    def sobol_indices(self, initial_conditions, n_base=16384, groups=None, rows=None, seed=1234, precision="f64_fast",
                      planar=False, filter_outliers=False, replicates=1000, level=0.95, bootstrap_seed=0, design=None):
        """Which dispersion drives what, interactions included (no reference counterpart; at its 4 k flights/s nobody
        flies (k + 2) n_base flights for it): the variance-based (Sobol) first-order and total-effect indices of `groups`
        of inputs on summary rows `rows` (default first apogee altitude and time, rail-exit speed: outputs every flight
        has) from a pick-freeze design, with bootstrap intervals - `analysis.sobol_indices` on a design flown here.

        The design is drawn under the INDEPENDENT law of `sampling.synthetic_dispersions(draws=...)` - a deliberate
        deviation from the reference's joint law, for this analysis alone: factors that share a normal cannot be frozen one
        at a time.  groups: None = `sampling.primitive_groups` (position, velocity, attitude, angular_velocity, mass,
        dead_draw, motor_thrust, motor_mass_flow, wind_speed, wind_direction, turbulence), a list of those names, or a
        mapping name -> rows of the primitive tensor (disjoint, at most 32).  A and B are `sampling.primitive_draws` at
        `seed` and `seed + 1`; block b of the k + 2 blocks (A, B, A with group i from B) is flown through eng.submit in
        sub-batches of at most DEVICE_CHUNK, inputs released per ticket, as run_monte_carlo_device does.
        design: None keeps those draws; 'random', 'lhs', 'lhs_centred' or 'qmc' takes A and B from `sampling.design_draws`
        (erpl_mc_design, erpl_mc_qmc) at `seed` and `seed + 1` instead: two independent designs of n_base columns, every primitive
        stratified with 'lhs'.
        filter_outliers=True masks a design row when erpl_mc_analyze gives ANY of its k + 2 flights a reason.
        One rank only (ValueError before any work): a design is not gathered across ranks.

        Returns the dict of `analysis.sobol_indices` plus 'groups' ({name: rows}), 'summary' (float64 [16, (k + 2)
        n_base] on the device, block-major), 'status', 'mask' (or None) and 'performance'."""
        from . import analysis as ana, sampling
        from .flatten import motor_kind
        if dist.world()[1] > 1:
            raise ValueError("sobol_indices is limited to a world size of 1: a design is not gathered across ranks")
        n_base = int(n_base)
        if n_base < 1:
            raise ValueError("n_base: at least one design row")
        use_base = self.base_wind_profile is not None and self.base_altitude_profile is not None
        K = len(self.base_altitude_profile) if use_base else 100   # synthetic_dispersions' default grid
        every = sampling.primitive_groups(K, motor_kind(self.motor) != _abi.MOTOR_SOLID)
        if groups is None:
            groups = every
        elif not hasattr(groups, "items"):
            unknown = [g for g in groups if g not in every]
            if unknown:
                raise ValueError(f"unknown group(s) {unknown}: one of {list(every)}")
            groups = {g: every[g] for g in groups}
        items = sampling.check_groups(groups, sampling.primitive_rows(K))
        k = len(items)
        if (k + 2) * n_base >= 2 ** 31:
            raise ValueError(f"(k + 2) * n_base = {(k + 2) * n_base} is 2^31 or more")
        eng = shared_engine(self.device)
        eng.set_config(self._config())
        prec = _abi.PRECISIONS[precision]
        torch.cuda.synchronize(eng.device)
        t0 = time.time()
        if design is None:
            A = sampling.primitive_draws(n_base, K, eng.device, seed)
            B = sampling.primitive_draws(n_base, K, eng.device, seed + 1)
        else:
            A = sampling.design_draws(n_base, K, eng.device, seed, design=design, engine=eng)
            B = sampling.design_draws(n_base, K, eng.device, seed + 1, design=design, engine=eng)
        parts, inflight = [], []
        keep = 2 * eng.get_overlap()
        for P in sampling.pick_freeze_blocks(A, B, dict(items)):
            for a in range(0, n_base, self.DEVICE_CHUNK):
                cnt = min(self.DEVICE_CHUNK, n_base - a)
                db = sampling.synthetic_dispersions(
                    cnt, self.rocket, self.motor, self.wind_model, initial_conditions, eng.device, precision=prec,
                    uncertainty=self.uncertainty_params, base_altitude_profile=self.base_altitude_profile,
                    base_wind_profile=self.base_wind_profile, planar=planar, engine=eng,
                    draws=P[:, a:a + cnt].contiguous())
                parts.append(eng.submit(db))
                inflight.append((eng.last_ticket, db))    # inputs outlive their batch
                while len(inflight) > keep:
                    ticket, inputs = inflight.pop(0)
                    eng.check(ticket)
                    del inputs
        eng.wait()
        eng.check()                # host-blocking; raises if a lane hand-over timed out
        inflight.clear()
        summ = torch.cat([p[0] for p in parts], dim=1).contiguous()
        status = torch.cat([p[1] for p in parts]).contiguous()
        torch.cuda.synchronize(eng.device)
        t1 = time.time()
        mask = None
        if filter_outliers:
            for b in range(k + 2):
                cols = slice(b * n_base, (b + 1) * n_base)
                _, why = eng.analyze(summ[:, cols].contiguous(), status[cols].contiguous(), reasons=True)
                mask = why.clone() if mask is None else mask | why
        out = ana.sobol_indices(summ, n_base, [name for name, _ in items], mask=mask, engine=eng, rows=rows,
                                replicates=replicates, level=level, seed=bootstrap_seed)
        torch.cuda.synchronize(eng.device)
        t2 = time.time()
        out["groups"] = {name: list(r) for name, r in items}
        if design is not None:
            out["design"] = {"kind": design, "seed": int(seed), "block": n_base, "replicates": 1}
        out["summary"], out["status"], out["mask"] = summ, status, mask
        flights = (k + 2) * n_base
        out["performance"] = {"flights": flights, "fly_s": t1 - t0, "flights_per_second": flights / max(t1 - t0, 1e-9),
                              "indices_s": t2 - t1, "precision": precision, "sub_batches": len(parts)}
        return out

    def plot_sobol(self, sobol, save_plots=True):
        """No reference counterpart: paired first-order / total-effect bars with their bootstrap intervals, one panel per
        row, saved as monte_carlo_sobol.png in the output directory; returns that directory."""
        return plots.plot_sobol(self, sobol, save_plots)

    def given_data_sensitivity(self, analysis, rows=None, **kw):
        """Which dispersion drives what without assuming a monotone response, from the run itself (no reference
        counterpart, no extra flights): `analysis.given_data_sensitivity` - eta2 with its main-effect curves, delta, the
        KS statistics and the mutual information, each next to its null band - on either kind of analysis dict, exactly
        as `drivers` takes its inputs.  kw: classes, cells, shifts, level, seed, want_tables, want_null."""
        from . import analysis as ana
        eng = shared_engine(self.device)
        if "factors" in analysis:
            return ana.given_data_sensitivity(analysis["summary"], analysis["factors"], analysis["factor_names"],
                                              status=analysis.get("status"), engine=eng, rows=rows, **kw)
        fac, names = ana.factors_from_results(analysis["results"])
        summ = ana.summary_from_results(analysis["results"])
        return ana.given_data_sensitivity(torch.as_tensor(summ, device=eng.device).contiguous(),
                                          torch.as_tensor(fac, device=eng.device).contiguous(), names, engine=eng, rows=rows,
                                          **kw)

    def plot_given_data_sensitivity(self, sensitivity, save_plots=True, top=4):
        """No reference counterpart: per row the delta of every factor with its null band and the main-effect curves of the
        `top` factors, saved as monte_carlo_given_data.png in the output directory; returns that directory."""
        return plots.plot_given_data_sensitivity(self, sensitivity, save_plots, top)

    def surrogate(self, analysis, variables=None, rows=None, degree=2, order=2, holdout=5):
        """A polynomial chaos surrogate of a run flown with `run_monte_carlo_device(design=...)` (no reference counterpart,
        no extra flights): `analysis.polynomial_chaos` - first-order, total and pair Sobol indices, r2 / q2 and a model for
        `TrajectoryEngine.surrogate_predict` - of the chosen primitives on up to 4 summary rows.  Only the chosen primitive
        rows are regenerated, from analysis["design"] through `TrajectoryEngine.design(first_row=...)` (`.qmc` for design='qmc'): the bits the run flew.
        variables: None (`sampling.scalar_primitives`: every scalar primitive, without the turbulence innovations and the
        dead draw) or a mapping name -> primitive row, at most 32.  ValueError for a run without `design`: under the
        reference's joint law the inputs are not independent (one normal is the thrust multiplier, position_x and the first
        turbulence innovation at once), and the basis is orthonormal only under independent inputs with known laws."""
        from . import analysis as ana, sampling
        from .flatten import motor_kind
        if "design" not in analysis:
            raise ValueError("surrogate needs a run flown with run_monte_carlo_device(design=...): the inputs of the joint law are "
                             "not independent, and a polynomial chaos basis is orthonormal only under independent inputs")
        if dist.world()[1] > 1:
            raise ValueError("surrogate is limited to a world size of 1")
        eng = shared_engine(self.device)
        use_base = self.base_wind_profile is not None and self.base_altitude_profile is not None
        K = len(self.base_altitude_profile) if use_base else 100      # as run_monte_carlo_device drew the design
        if variables is None:
            variables = sampling.scalar_primitives(K, motor_kind(self.motor) != _abi.MOTOR_SOLID)
        names, prim = [str(k) for k in variables], [int(r) for r in dict(variables).values()]
        n_prim = sampling.primitive_rows(K)
        if not 1 <= len(prim) <= _abi.SUR_MAX_VARS or len(set(prim)) != len(prim) or not all(0 <= r < n_prim for r in prim):
            raise ValueError(f"variables: 1 to {_abi.SUR_MAX_VARS} distinct primitive rows in 0..{n_prim - 1}")
        d = analysis["design"]
        summ = analysis["summary"]
        n = int(summ.shape[1])
        kinds = [_abi.DESIGN_NORMAL if r < 17 + 3 * K else _abi.DESIGN_UNIFORM for r in prim]
        factors = torch.empty((len(prim), n), dtype=torch.float64, device=eng.device)
        qdims = sampling.qmc_dims(K) if d["kind"] == "qmc" else None      # as `sampling.design_draws` laid the rows out
        for i, r in enumerate(prim):
            if qdims is not None:
                eng.qmc([kinds[i]], n, d["seed"], dims=[qdims[r]], block=d["block"], first_row=r, out=factors[i:i + 1])
            else:
                eng.design([kinds[i]], n, d["seed"], kind=d["kind"], block=d["block"], first_row=r, out=factors[i:i + 1])
        out = ana.polynomial_chaos(summ, factors, kinds, names, status=analysis.get("status"), engine=eng, rows=rows, degree=degree,
                                   order=order, holdout=holdout)
        out["factors"], out["primitive_rows"] = factors, prim
        return out

    def _law_change_factors(self, analysis, uncertainty, motor, shift, planar):
        """What `reweight` and `reweighted_impact` share: the changed primitive rows of the target law (sampling.law_change)
        regenerated from analysis["design"] - (engine, summary, factors, kinds, law, primitive rows, change)."""
        from . import sampling
        from .flatten import motor_kind
        if "design" not in analysis:
            raise ValueError("reweight needs a run flown with run_monte_carlo_device(design=...): the inputs of the joint law are not "
                             "independent, and the density ratio of two laws is a product of row factors only for independent inputs")
        if dist.world()[1] > 1:
            raise ValueError("reweight is limited to a world size of 1")
        eng = shared_engine(self.device)
        use_base = self.base_wind_profile is not None and self.base_altitude_profile is not None
        K = len(self.base_altitude_profile) if use_base else 100      # as run_monte_carlo_device drew the design
        change = sampling.law_change(K, motor_kind(self.motor) != _abi.MOTOR_SOLID, self.uncertainty_params, uncertainty, motor=self.motor,
                                     target_motor=motor, shift=shift, planar=planar)
        if not change:
            raise ValueError("the target law is the flown one: no primitive changes")
        prim = list(change)
        kinds = [change[r][0] for r in prim]
        law = [change[r][1:3] if change[r][0] == _abi.DESIGN_NORMAL else change[r][3:5] for r in prim]
        d = analysis["design"]
        summ = analysis["summary"]
        n = int(summ.shape[1])
        factors = torch.empty((len(prim), n), dtype=torch.float64, device=eng.device)
        qdims = sampling.qmc_dims(K) if d["kind"] == "qmc" else None      # as `sampling.design_draws` laid the rows out
        for i, r in enumerate(prim):
            if qdims is not None:
                eng.qmc([kinds[i]], n, d["seed"], dims=[qdims[r]], block=d["block"], first_row=r, out=factors[i:i + 1])
            else:
                eng.design([kinds[i]], n, d["seed"], kind=d["kind"], block=d["block"], first_row=r, out=factors[i:i + 1])
        return eng, summ, factors, kinds, law, prim, change

    def reweight(self, analysis, uncertainty=None, motor=None, shift=None, rows=None, thresholds=None,
                 quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), planar=False):
        """What a run flown with `run_monte_carlo_device(design=...)` says under ANOTHER input law (no reference counterpart,
        no extra flights): `analysis.reweighted_statistics` - per row mean +- se, std, quantiles and exceedance
        probabilities +- se, with ess, ess_share, ess_expected_share, max_weight_share and warnings - for the target
        `uncertainty` table (entries on top of the flown `uncertainty_params`), a target `motor` (its thrust_uncertainty /
        mass_flow_uncertainty against the flown motor's) and `shift` (a mean in flown sigmas per primitive), through
        `sampling.law_change`.  Only the changed primitive rows are regenerated, from analysis["design"] through
        `TrajectoryEngine.design(first_row=...)` (`.qmc` for design='qmc'): the bits the run flew.  planar: the run was flown
        with planar=True, the rows Set P zeroes are left out.  ValueError for a run without `design`: under the reference's
        joint law the inputs are not independent (one normal is the thrust multiplier, position_x and the first turbulence
        innovation at once), and the density ratio is not a product of row factors."""
        from . import analysis as ana
        eng, summ, factors, kinds, law, prim, change = self._law_change_factors(analysis, uncertainty, motor, shift, planar)
        out = ana.reweighted_statistics(summ, factors, kinds, law, status=analysis.get("status"), engine=eng, rows=rows,
                                        thresholds=thresholds, quantiles=quantiles)
        out["primitive_rows"], out["law"] = prim, change
        return out

    def reweighted_impact(self, analysis, uncertainty=None, motor=None, shift=None, zones=None, target=None,
                          cep_quantiles=(0.5, 0.9, 0.95), planar=False, **density_kw):
        """Where it comes down under ANOTHER input law (no reference counterpart, no extra flights):
        `analysis.reweighted_impact` - the weighted impact probability map with its 50 / 90 / 99 % regions, the probability
        +- se of landing inside `zones`, the weighted miss-distance quantiles 'cep', ess and warnings - of a run flown with
        `run_monte_carlo_device(design=...)`, for the target law given as in `reweight` (uncertainty, motor, shift, planar).
        density_kw: nodes, ranges, pad, bandwidth, levels, sample_density, rows."""
        from . import analysis as ana
        eng, summ, factors, kinds, law, prim, change = self._law_change_factors(analysis, uncertainty, motor, shift, planar)
        out = ana.reweighted_impact(summ, factors, kinds, law, status=analysis.get("status"), engine=eng, target=target,
                                    cep_quantiles=cep_quantiles, zones=zones, **density_kw)
        out["primitive_rows"], out["law"] = prim, change
        return out

    def plot_reweighted_impact(self, reweighted, save_plots=True):
        """No reference counterpart: the dict of `reweighted_impact` as monte_carlo_reweighted_impact.png (the figure of
        `plot_impact_probability`, titled with the effective sample size) and reweighted_impact.json; returns the output
        directory."""
        return plots.plot_reweighted_impact(self, reweighted, save_plots)

    def reweighted_corridor(self, captured, uncertainty=None, motor=None, shift=None, planar=False,
                            quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), thresholds=None):
        """The time-resolved bands of a captured run under ANOTHER input law (no reference counterpart, no extra flights):
        `captured` is the dict of `trajectory_corridor`, `impact_point_trace` or `debris_footprint` flown with design=... -
        its 'values', 'reasons' (the mask), 'time', 'channels', 'summary' and 'design' are read - and the target law is
        given as in `reweight` (uncertainty, motor, shift, planar).  `analysis.reweighted_corridor`: one erpl_mc_reweight
        call for the weights, erpl_mc_corridor_bands_weighted for the bands under them, erpl_mc_corridor_bands for the
        flown bands beside them; per channel 'reweighted' and 'flown', per node the effective sample size, and the
        warnings of the reweighting.  thresholds: per channel (index -> up to 4 values) the exceedance probabilities
        wanted at every node.  ValueError for a dict without 'design', as `reweight`."""
        from . import analysis as ana
        eng, summ, factors, kinds, law, prim, change = self._law_change_factors(captured, uncertainty, motor, shift, planar)
        t = np.asarray(captured["time"], dtype=np.float64)
        out = ana.reweighted_corridor(captured["values"], float(t[0]) if len(t) else 0.0, float(t[1] - t[0]) if len(t) > 1 else 1.0,
                                      list(captured["channels"]), factors, kinds, law, mask=captured["reasons"], engine=eng,
                                      quantiles=quantiles, thresholds=thresholds)
        if "fragments" in captured:   # the rows of a debris matrix are (node, fragment) pairs: every time once per fragment
            out["fragments"] = captured["fragments"]
            out["time"] = np.repeat(t, len(captured["fragments"]))
        out["primitive_rows"], out["law"] = prim, change
        return out

    def plot_reweighted_corridor(self, reweighted, save_plots=True):
        """No reference counterpart: the dict of `reweighted_corridor` as monte_carlo_reweighted_corridor.png - per channel the
        flown bands dashed, the reweighted bands solid and the per-node effective sample size on a second axis - and
        reweighted_corridor.json next to it; returns the output directory."""
        return plots.plot_reweighted_corridor(self, reweighted, save_plots)

    def plot_surrogate(self, surrogate, save_plots=True):
        """No reference counterpart: per row the first-order and total indices of the variables, the largest pair indices
        and predicted against flown on the held-out members, saved as monte_carlo_surrogate.png in the output directory;
        returns that directory."""
        return plots.plot_surrogate(self, surrogate, save_plots)

    def compare_runs(self, analysis_a, analysis_b, **kw):
        """Did two runs come from the same law (no reference counterpart)?  `analysis.compare_runs` - per row the
        Kolmogorov-Smirnov, Mann-Whitney and Cramer-von Mises tests with the shift function, the energy test of the two
        impact clouds, every p-value from relabellings of the pooled flights - on two analysis dicts of either kind, as
        `confidence_intervals` takes its inputs.  kw: rows, quantiles, xy, permutations, level, seed, keep_null."""
        from . import analysis as ana
        eng = shared_engine(self.device)

        def inputs(analysis):
            if "summary" in analysis:
                return analysis["summary"], analysis.get("status")
            summ = ana.summary_from_results(analysis["results"])
            return torch.as_tensor(summ, device=eng.device).contiguous(), None

        (a, status_a), (b, status_b) = inputs(analysis_a), inputs(analysis_b)
        return ana.compare_runs(a, b, status_a=status_a, status_b=status_b, engine=eng, **kw)

    def plot_run_comparison(self, comparison, save_plots=True):
        """No reference counterpart: per row the two distribution functions with the Kolmogorov-Smirnov location, the shift
        function and the null histogram (when the nulls were kept), and the two impact clouds with the energy statistic,
        saved as monte_carlo_run_comparison.png in the output directory; returns that directory."""
        return plots.plot_run_comparison(self, comparison, save_plots)

    def impact_probability(self, analysis, **kw):
        """Where it comes down, as probabilities (no reference counterpart): `analysis.impact_probability` - the kernel
        density of the impact points, the thresholds of the regions that hold 50 / 90 / 99 % of the landings and the
        probability of landing inside `zones` - on either kind of analysis dict, as `confidence_intervals` takes its inputs."""
        from . import analysis as ana
        eng = shared_engine(self.device)
        if "summary" in analysis:
            return ana.impact_probability(analysis["summary"], status=analysis.get("status"), engine=eng, **kw)
        summ = ana.summary_from_results(analysis["results"])
        return ana.impact_probability(torch.as_tensor(summ, device=eng.device).contiguous(), engine=eng, **kw)

    def plot_impact_probability(self, analysis, save_plots=True, zones=None):
        """No reference counterpart: the impact probability map - filled contours of the regions that hold 50 / 90 / 99 % of
        the landings, the outlines of `zones` with the probability of landing inside - as
        monte_carlo_impact_probability.png, the numbers as impact_probability.json; returns the output directory."""
        return plots.plot_impact_probability(self, analysis, save_plots, zones)

    def plot_drivers(self, analysis, save_plots=True):
        """No reference counterpart: one tornado chart (Spearman and SRRC of the strongest factors) per default row, saved
        as monte_carlo_drivers.png in the output directory; returns that directory."""
        return plots.plot_drivers(self, analysis, save_plots)

    def _filter_physics_outliers(self, results):
        """monte_carlo.py:337-398."""
        valid, outliers = [], []
        for r in results:
            reasons = analysis.outlier_reasons(r.get("apogee_altitude", 0), r.get("range", 0), r.get("flight_time", 0))
            if reasons:
                r["outlier_reasons"] = reasons
                outliers.append(r)
            else:
                valid.append(r)
        return valid, outliers

    def _analyze_results(self, results):
        """monte_carlo.py:400-473."""
        return analysis.analyze(results, verbose=self.verbose)
