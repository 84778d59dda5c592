"""TrajectoryEngine — thin Python driver of the C ABI (include/erpl_mc.h).

PyTorch-ROCm is used only as plumbing: it owns the device buffers (SoA tensors) and the HIP
stream; every number is produced by the hand-written HIP kernels behind `erpl_mc_run_batch`.
No CPU execution path exists here: if the HIP library or a GPU is missing, construction raises.
"""
import ctypes as C
import threading

import numpy as np
import torch

from . import _abi


class DeviceBatch:
    """Per-sample SoA tensors resident in HBM (the layout `erpl_batch` points at)."""

    def __init__(self, ic, rocket, motor, alt_grid, wind, precision):
        self.ic, self.rocket, self.motor = ic, rocket, motor
        self.alt_grid, self.wind = alt_grid, wind
        self.precision = precision
        self.n = int(ic.shape[1])
        self.k_wind = 0 if wind is None else int(wind.shape[0])
        # the kernels index these by (row, sample) and the knots by row: a wrong shape is an out-of-bounds read on the GPU
        if wind is not None:
            if alt_grid is None or tuple(wind.shape) != (self.k_wind, 3, self.n) or alt_grid.numel() != self.k_wind:
                raise ValueError(f"wind must be (K, 3, n) with K altitudes: got wind {tuple(wind.shape)}, "
                                 f"altitudes {None if alt_grid is None else tuple(alt_grid.shape)}, n = {self.n}")
            if not 1 <= self.k_wind <= _abi.MAX_WIND_KNOTS:
                raise ValueError(f"1..{_abi.MAX_WIND_KNOTS} wind knots, got {self.k_wind}")
            if alt_grid.dtype != torch.float64 or wind.dtype != (torch.float32 if precision == _abi.PREC_F32 else torch.float64):
                raise ValueError("altitudes are float64; the wind table is float32 for the fp32 build, float64 otherwise")
            if not (wind.is_contiguous() and alt_grid.is_contiguous()):
                raise ValueError("wind and altitudes must be contiguous")

    def input_bytes(self):
        b = self.ic.numel() * 8 + self.rocket.numel() * 8 + self.motor.numel() * 8
        if self.wind is not None:
            b += self.wind.numel() * self.wind.element_size() + self.alt_grid.numel() * 8
        return b

    @staticmethod
    def from_host(hb, device, precision=_abi.PREC_F64, wind=None):
        """Upload a flatten.HostBatch.  The wind table is stored in the working precision.  `wind`: the float64 [K, 3, n]
        table already on the device (TrajectoryEngine.legacy_wind_device) of a batch built without one; it is checked
        there and converted as an uploaded one is."""
        if hb.k_wind > _abi.MAX_WIND_KNOTS:
            raise _abi.ErplError(f"{hb.k_wind} wind knots exceed the ABI limit {_abi.MAX_WIND_KNOTS}")
        if hb.k_wind and not np.all(np.diff(hb.alt_grid) > 0):
            raise _abi.ErplError("altitude_profile must be strictly increasing")
        # (one reduction instead of an element-wise mask: a NaN or inf anywhere makes the sum non-finite; a finite table
        # whose sum overflows is re-checked element by element)
        if hb.k_wind and hb.wind is None and wind is None:
            raise _abi.ErplError("the batch was built without its wind table (with_wind=False) and none is given")
        if wind is None:
            finite = lambda: np.isfinite(np.sum(hb.wind)) or np.all(np.isfinite(hb.wind))
        else:   # the same two reductions on the device
            finite = lambda: bool(torch.isfinite(wind.sum())) or bool(torch.isfinite(wind).all())
        if hb.k_wind and not (np.all(np.isfinite(hb.alt_grid)) and finite()):
            raise _abi.ErplError("wind profile must be finite")
        # The kernels assume what the reference silently assumes: finite inputs, positive masses and
        # mass flow, a finite burn time (a non-finite burn time would never leave the launch rail).
        if hb.n >= 2 ** 31:
            raise _abi.ErplError("at most 2**31 - 1 samples per batch")
        if not (np.all(np.isfinite(hb.ic)) and np.all(np.isfinite(hb.rocket)) and np.all(np.isfinite(hb.motor))):
            raise _abi.ErplError("initial conditions, masses and motor parameters must be finite")
        if not (np.all(hb.rocket[0] > 0) and np.all(hb.rocket[1] > 0)):
            raise _abi.ErplError("dry_mass and propellant_mass must be positive")
        if not (np.all(hb.motor[2] > 0) and np.all(hb.motor[3] >= 0)):
            raise _abi.ErplError("mass_flow_rate must be positive and burn_time non-negative")
        wdt = torch.float32 if precision == _abi.PREC_F32 else torch.float64
        f64 = dict(dtype=torch.float64, device=device)
        ic = torch.as_tensor(np.ascontiguousarray(hb.ic), **f64)
        rocket = torch.as_tensor(np.ascontiguousarray(hb.rocket), **f64)
        motor = torch.as_tensor(np.ascontiguousarray(hb.motor), **f64)
        if hb.k_wind:
            alt = torch.as_tensor(np.ascontiguousarray(hb.alt_grid), **f64)
            if wind is None:
                wind = torch.as_tensor(np.ascontiguousarray(hb.wind), device=device)
            wind = wind.to(wdt).contiguous()
        else:
            alt, wind = None, None
        return DeviceBatch(ic, rocket, motor, alt, wind, precision)


class TrajectoryEngine:
    """One engine (= one `erpl_ctx`) per GPU / torch.distributed rank."""

    def __init__(self, device=None, lib_path=None):
        self.lib = _abi.load_library(lib_path)   # lib_path: an experiment build (tools/), never the product
        if not torch.cuda.is_available():
            raise _abi.ErplError("no GPU visible to PyTorch-ROCm; this engine has no CPU fallback")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._ctx = C.c_void_p()
        _abi.check(self.lib, self.lib.erpl_mc_create(idx, C.byref(self._ctx)), "erpl_mc_create")
        self._cfg = None
        self._legacy_lock = threading.Lock()   # legacy_streams_device / legacy_wind_device: one workspace per context

    def _call(self, name, *args):
        """`name(ctx, *args)` of the library; a non-zero return raises with the library's own message (_abi.check)."""
        _abi.check(self.lib, getattr(self.lib, name)(self._ctx, *args), name)

    def _defaults(self, cls, fn_name):
        """A spec struct as the library's `erpl_mc_*_defaults` fills it."""
        spec = cls()
        _abi.check(self.lib, getattr(self.lib, fn_name)(C.byref(spec)), fn_name)
        return spec

    @staticmethod
    def _batch_struct(db, flags=0):
        """The `erpl_batch` that points at the tensors of a DeviceBatch."""
        b = _abi.ErplBatch()
        b.n, b.precision, b.k_wind, b.flags = db.n, db.precision, db.k_wind, flags
        b.ic, b.rocket, b.motor = db.ic.data_ptr(), db.rocket.data_ptr(), db.motor.data_ptr()
        b.alt_grid = db.alt_grid.data_ptr() if db.k_wind else None
        b.wind = db.wind.data_ptr() if db.k_wind else None
        return b

    def _check_summary(self, summary):
        """The summary tensor every analysis call reads on the device (there is no CPU path behind them): returns n."""
        if not (summary.is_cuda and summary.device == self.device and summary.dtype == torch.float64
                and summary.dim() == 2 and summary.shape[0] == _abi.SUMMARY_DIM and summary.is_contiguous()):
            raise ValueError(f"summary must be a contiguous float64 [{_abi.SUMMARY_DIM}, n] tensor on {self.device}")
        return int(summary.shape[1])

    @staticmethod
    def _set_rows(spec, rows, lo, hi):
        """Overrides spec.rows with `rows`, lo..hi of them (None: the library's default stays)."""
        if rows is None:
            return
        rows = [int(r) for r in rows]
        if not lo <= len(rows) <= hi:
            raise ValueError(f"{lo} to {hi} rows" if lo else f"at most {hi} rows")
        spec.n_rows = len(rows)
        spec.rows[:len(rows)] = rows

    @staticmethod
    def _fractions(values, most, what):
        """`values` (levels, quantiles) as a list of floats, `most` of them at the most."""
        values = [float(v) for v in values]
        if len(values) > most:
            raise ValueError(f"at most {most} {what}")
        return values

    @staticmethod
    def _row_stats_dict(r, q):
        """An erpl_row_stats with the fractions `q` its order statistics belong to, as a plain dict."""
        nq = len(q)
        return {"count": int(r.count), "mean": r.mean, "std": r.std, "min": r.min, "max": r.max, "q": q,
                "quantiles": list(r.quantile[:nq]), "order_lo": list(r.order_lo[:nq]), "order_hi": list(r.order_hi[:nq])}

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self.lib.erpl_mc_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_config(self, cfg):
        self._call("erpl_mc_set_config", C.byref(cfg))
        self._cfg = cfg

    def set_launch(self, block_threads=256, max_blocks=0, refill_threshold=1):
        self._call("erpl_mc_set_launch", block_threads, max_blocks, refill_threshold)

    def set_waves_per_simd(self, waves):
        """fp32 flight-kernel build: 2 (256 VGPRs), 3 (168 VGPRs, three resident waves), 0 = by batch size."""
        self._call("erpl_mc_set_waves_per_simd", int(waves))

    def set_chunk(self, chunk_steps):
        """Step-chunked launches with per-GPU compaction in between (0 = single launch; < 0 = the library decides
        per batch from the trajectory lengths of the batches it has finished: erpl_mc_set_chunk)."""
        self._call("erpl_mc_set_chunk", int(chunk_steps))

    def set_adopt(self, lanes):
        """Lane adoption: waves down to `lanes` flying trajectories hand them to fuller waves (0 = off, < 0 = the
        library decides per batch: erpl_mc_set_adopt)."""
        self._call("erpl_mc_set_adopt", int(lanes))

    def reserve(self, n):
        self._call("erpl_mc_reserve", n)

    def alloc_outputs(self, n):
        summary = torch.empty((_abi.SUMMARY_DIM, n), dtype=torch.float64, device=self.device)
        status = torch.empty((n,), dtype=torch.int32, device=self.device)
        return summary, status

    def set_short_flight_overlap(self, depth):
        """How many batches of short flights start side by side (erpl_mc_set_short_flight_overlap; default 4, 0 = no limit
        besides set_overlap).  Scheduling only."""
        self._call("erpl_mc_set_short_flight_overlap", int(depth))

    def get_overlap(self):
        """Batches `submit()` keeps in flight at once (3, or 8 when the process has the hardware queues for it)."""
        return int(self.lib.erpl_mc_get_overlap(self._ctx))

    def set_overlap(self, depth):
        """Batches `submit()` keeps in flight at once (erpl_mc_set_overlap; 1..8)."""
        self._call("erpl_mc_set_overlap", int(depth))

    def submit(self, db, **kw):
        """Like run(), but on one of the library's internal streams (erpl_mc_submit_batch): the batch
        starts after everything enqueued on the current stream so far and may overlap earlier batches;
        the current stream does NOT wait for it.  Call wait() before touching the outputs.  The ticket
        of the batch is kept in `self.last_ticket`."""
        return self.run(db, overlap=True, **kw)

    def wait(self, ticket=-1, stream=None):
        """Make `stream` (default: the current torch stream) wait on the device for a submitted batch
        (ticket < 0: for all of them).  The host does not block."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._call("erpl_mc_wait_batch", int(ticket), C.c_void_p(st.cuda_stream))

    def synchronize(self):
        """Host-blocking wait for everything enqueued; raises _abi.IncompleteBatch if a lane hand-over timed out."""
        self._call("erpl_mc_synchronize")

    def check(self, ticket=-1):
        """Where results are consumed: block the host until batch `ticket` (< 0: every submitted batch) has finished
        and raise _abi.IncompleteBatch if one of its lane hand-overs timed out (erpl_mc_check_batch).  wait() only
        orders a stream on the device; it reports batches that had ALREADY finished incomplete when it is called."""
        self._call("erpl_mc_check_batch", int(ticket))

    def set_adopt_spin(self, polls):
        """Test knob (erpl_mc_set_adopt_spin): < 0 makes every adopting lane give up at once."""
        self._call("erpl_mc_set_adopt_spin", int(polls))

    def set_sweep_pool(self, mode):
        """Sweep streams from the other stream-priority pool where a lane has one hardware queue (erpl_mc_set_sweep_pool):
        -1 = from the first batch that fills the GPU on (the default), 0 = never, 1 = always.  Scheduling only."""
        self._call("erpl_mc_set_sweep_pool", int(mode))

    @staticmethod
    def raise_if_incomplete(status):
        """Results whose status words still carry ST_INCOMPLETE were never integrated: refuse to hand them on."""
        bad = (status & _abi.ST_INCOMPLETE) != 0
        n_bad = int(bad.sum())
        if n_bad:
            raise _abi.IncompleteBatch(f"{n_bad} sample(s) carry ERPL_ST_INCOMPLETE: a lane hand-over timed out")

    def debug_eval(self, db, what, inputs):
        """Device-side known-answer evaluation (erpl_mc_debug_eval): inputs [rows, m] -> outputs [rows', m]
        float64, through the device functions of the kernel build `db.precision` selects."""
        x = torch.as_tensor(np.ascontiguousarray(np.atleast_2d(inputs), dtype=np.float64), device=self.device)
        m = int(x.shape[1])
        rows = {_abi.DBG_ATMOSPHERE: 4, _abi.DBG_AERO: 5, _abi.DBG_RHS: 15, _abi.DBG_MATH: _abi.DBG_MATH_ROWS,
                _abi.DBG_RHS_SEQ: 15, _abi.DBG_MINMAX: _abi.DBG_MINMAX_ROWS}[what]
        out = torch.full((rows, m), float("nan"), dtype=torch.float64, device=self.device)
        b = self._batch_struct(db)
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_debug_eval", C.byref(b), int(what), m, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()),
                   C.c_void_p(st.cuda_stream))
        torch.cuda.synchronize(self.device)
        return out.cpu().numpy()

    def run(self, db, flags=0, summary=None, status=None, traj_ids=None, traj_stride=1, traj_cap=0,
            stream=None, overlap=False):
        """Enqueue rail + flight kernels for the batch on the current torch stream.
        Returns (summary [16, n] f64, status [n] i32[, traj [m, cap, 15] f64, traj_len [m] i64]);
        asynchronous with respect to the host."""
        if summary is None or status is None:
            summary, status = self.alloc_outputs(db.n)
        b = self._batch_struct(db, flags)
        o = _abi.ErplOut()
        o.summary, o.status = summary.data_ptr(), status.data_ptr()
        traj = tlen = ids = None
        if traj_ids is not None and len(traj_ids):
            ids = torch.as_tensor(np.asarray(traj_ids, dtype=np.int64), device=self.device)
            traj = torch.full((len(ids), traj_cap, _abi.TRAJ_DIM), float("nan"), dtype=torch.float64,
                              device=self.device)
            tlen = torch.zeros((len(ids),), dtype=torch.int64, device=self.device)
            o.n_traj, o.traj_ids, o.traj_stride, o.traj_cap = len(ids), ids.data_ptr(), traj_stride, traj_cap
            o.traj, o.traj_len = traj.data_ptr(), tlen.data_ptr()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if overlap:
            t = C.c_int64(0)
            self._call("erpl_mc_submit_batch", C.byref(b), C.byref(o), C.c_void_p(st.cuda_stream), C.byref(t))
            self.last_ticket = t.value
        else:
            self._call("erpl_mc_run_batch", C.byref(b), C.byref(o), C.c_void_p(st.cuda_stream))
        if traj is not None:
            self._keep = ids
            return summary, status, traj, tlen
        return summary, status

    def extract_histories(self, db, sample, traj, time_offset, stream=None):
        """Per-step diagnostic histories (simulator.py:496-552) of the records `traj` [m, 15] (device
        tensor, as produced by run(..., traj_ids=...)) of sample `sample`: returns [m, 17] f64."""
        traj = traj.contiguous()
        m = int(traj.shape[0])
        out = torch.empty((m, _abi.DIAG_DIM), dtype=torch.float64, device=self.device)
        b = self._batch_struct(db)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._call("erpl_mc_extract_histories", C.byref(b), int(sample), C.c_void_p(traj.data_ptr()), m,
                   float(time_offset), C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream))
        return out

    def flight_envelope(self, db, traj_ids, traj, traj_len, stream=None):
        """The flight envelope of every captured trajectory (erpl_mc_flight_envelope): maximum dynamic pressure with its
        time, altitude and Mach number, maximum Mach number, q-alpha, axial acceleration, the smallest stability margin,
        the largest angular rate and quaternion-norm drift, the state at burnout, the apogee record and the usable prefix
        (rows _abi.ENV_*; the definitions are in include/erpl_mc.h).  `db` is the batch the records came from (fp64 wind
        tables), traj_ids int64 [m], traj float64 [m, cap, 15] and traj_len int64 [m] the capture of run(..., traj_ids=...)
        on the device.  Returns float64 [16, m] on the device; asynchronous on `stream` (default: the current stream)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dtype == dtype and t.is_contiguous()
        if not (ok(traj, torch.float64) and traj.dim() == 3 and traj.shape[2] == _abi.TRAJ_DIM):
            raise ValueError(f"traj must be a contiguous float64 [m, cap, {_abi.TRAJ_DIM}] tensor on {self.device}")
        m, cap = int(traj.shape[0]), int(traj.shape[1])
        if not (ok(traj_ids, torch.int64) and tuple(traj_ids.shape) == (m,)):
            raise ValueError(f"traj_ids must be a contiguous int64 [m] tensor on {self.device}")
        if not (ok(traj_len, torch.int64) and tuple(traj_len.shape) == (m,)):
            raise ValueError(f"traj_len must be a contiguous int64 [m] tensor on {self.device}")
        env = torch.empty((_abi.ENV_DIM, m), dtype=torch.float64, device=self.device)
        if m == 0:   # (an empty tensor has no address to hand over)
            return env
        b = self._batch_struct(db)
        o = _abi.ErplOut()
        o.n_traj, o.traj_ids, o.traj_cap = m, traj_ids.data_ptr(), cap
        o.traj, o.traj_len = traj.data_ptr(), traj_len.data_ptr()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._call("erpl_mc_flight_envelope", C.byref(b), C.byref(o), C.c_void_p(env.data_ptr()), C.c_void_p(st.cuda_stream))
        return env

    def impact_points(self, db, traj_ids, traj, traj_len, nodes=64, record_stride=1, dt=0.05, max_steps=20000, ground=0.0,
                      drag_scale=1.0, origin=(0.0, 0.0), keep_in=None, out=None, col0=0, summary=True, stream=None):
        """The instantaneous impact points of every captured trajectory (erpl_mc_impact_points; the definitions are in
        include/erpl_mc.h): node k = record k * record_stride falls from its own position and velocity to the plane
        z = ground without thrust - frozen mass, zero-incidence power-off drag times drag_scale, the sample's own wind,
        RK4 steps of dt, at most max_steps of them.  `db`, traj_ids, traj and traj_len as for flight_envelope.  keep_in: a
        keep-in polygon, a sequence of 3 to 64 (x, y) vertices, or None.  Trajectory j fills column col0 + j of `out`, a
        float64 [5, nodes, ld] device tensor (channels _abi.IIP_CH_*; default: a new one with ld = col0 + m, NaN
        everywhere); the other columns are left alone.  Returns (out, summary): summary float64 [16, m] on the device (rows
        _abi.IIP_*), or None with summary=False.  Asynchronous on `stream` (default: the current stream)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dtype == dtype and t.is_contiguous()
        if not (ok(traj, torch.float64) and traj.dim() == 3 and traj.shape[2] == _abi.TRAJ_DIM):
            raise ValueError(f"traj must be a contiguous float64 [m, cap, {_abi.TRAJ_DIM}] tensor on {self.device}")
        m, cap = int(traj.shape[0]), int(traj.shape[1])
        if not (ok(traj_ids, torch.int64) and tuple(traj_ids.shape) == (m,)):
            raise ValueError(f"traj_ids must be a contiguous int64 [m] tensor on {self.device}")
        if not (ok(traj_len, torch.int64) and tuple(traj_len.shape) == (m,)):
            raise ValueError(f"traj_len must be a contiguous int64 [m] tensor on {self.device}")
        nodes, record_stride, max_steps = int(nodes), int(record_stride), int(max_steps)
        # (the Python ints, before a 32-bit field can truncate them)
        if not 1 <= nodes <= _abi.IIP_MAX_NODES:
            raise ValueError(f"1 to {_abi.IIP_MAX_NODES} nodes")
        if not 1 <= record_stride < 2 ** 31:
            raise ValueError("record_stride must be 1 to 2**31 - 1")
        if not 1 <= max_steps <= _abi.IIP_MAX_STEPS:
            raise ValueError(f"max_steps must be 1 to {_abi.IIP_MAX_STEPS}")
        spec = self._defaults(_abi.ErplIipSpec, "erpl_mc_impact_points_defaults")
        spec.n_nodes, spec.record_stride, spec.max_steps = nodes, record_stride, max_steps
        spec.dt, spec.ground, spec.drag_scale = float(dt), float(ground), float(drag_scale)
        spec.origin_x, spec.origin_y = float(origin[0]), float(origin[1])
        if keep_in is not None:
            keep_in = [(float(x), float(y)) for x, y in keep_in]
            if not 3 <= len(keep_in) <= _abi.IIP_MAX_VERTICES:
                raise ValueError(f"3 to {_abi.IIP_MAX_VERTICES} keep-in vertices")
            spec.n_vertices = len(keep_in)
            for i, (x, y) in enumerate(keep_in):
                spec.keep_x[i], spec.keep_y[i] = x, y
        shape = (_abi.IIP_CH_COUNT, spec.n_nodes)
        col0 = int(col0)
        if out is None:
            out = torch.full(shape + (col0 + m,), float("nan"), dtype=torch.float64, device=self.device)
        if not (ok(out, torch.float64) and out.dim() == 3 and tuple(out.shape[:2]) == shape):
            raise ValueError(f"out must be a contiguous float64 [{shape[0]}, {shape[1]}, ld] tensor on {self.device}")
        ld = int(out.shape[2])
        if col0 < 0 or col0 + m > ld:
            raise ValueError(f"columns {col0}..{col0 + m} do not fit ld = {ld}")
        summ = torch.empty((_abi.IIP_DIM, m), dtype=torch.float64, device=self.device) if summary else None
        if m == 0:   # (an empty tensor has no address to hand over)
            return out, summ
        b = self._batch_struct(db)
        o = _abi.ErplOut()
        o.n_traj, o.traj_ids, o.traj_cap = m, traj_ids.data_ptr(), cap
        o.traj, o.traj_len = traj.data_ptr(), traj_len.data_ptr()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._call("erpl_mc_impact_points", C.byref(b), C.byref(o), C.byref(spec), C.c_void_p(out.data_ptr()), ld, col0,
                   C.c_void_p(summ.data_ptr()) if summ is not None else None, C.c_void_p(st.cuda_stream))
        return out, summ

    def debris(self, db, traj_ids, traj, traj_len, fragments, nodes=16, record_stride=1, dt=0.05, max_steps=20000, ground=0.0,
               stiff_limit=0.25, seed=0, origin=(0.0, 0.0), keep_in=None, out=None, col0=0, summary=True, stream=None):
        """Where the fragments fall if the vehicle breaks up (erpl_mc_debris; the definitions are in include/erpl_mc.h): at
        node k = record k * record_stride every fragment (beta, dv) of `fragments` - a sequence of 1 to 64 pairs, beta the
        ballistic coefficient m / (Cd A) in kg/m^2 (float('inf'): no drag), dv the speed in m/s the break-up adds in an
        isotropic direction drawn from (seed, sample id, node, fragment) - falls to the plane z = ground under gravity, its
        drag and the sample's own wind, by RK4 steps of dt that are halved while drag rate * step exceeds stiff_limit, at most
        max_steps of them.  `db`, traj_ids, traj, traj_len, keep_in, col0 and `stream` as for impact_points.  Trajectory j
        fills column col0 + j of `out`, a float64 [5, nodes * len(fragments), ld] device tensor (channels _abi.IIP_CH_*, row
        k * len(fragments) + f; default: a new one with ld = col0 + m, NaN everywhere).  Returns (out, summary): summary
        float64 [16, m] on the device (rows _abi.DEBRIS_*), or None with summary=False.  Asynchronous."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dtype == dtype and t.is_contiguous()
        if not (ok(traj, torch.float64) and traj.dim() == 3 and traj.shape[2] == _abi.TRAJ_DIM):
            raise ValueError(f"traj must be a contiguous float64 [m, cap, {_abi.TRAJ_DIM}] tensor on {self.device}")
        m, cap = int(traj.shape[0]), int(traj.shape[1])
        if not (ok(traj_ids, torch.int64) and tuple(traj_ids.shape) == (m,)):
            raise ValueError(f"traj_ids must be a contiguous int64 [m] tensor on {self.device}")
        if not (ok(traj_len, torch.int64) and tuple(traj_len.shape) == (m,)):
            raise ValueError(f"traj_len must be a contiguous int64 [m] tensor on {self.device}")
        nodes, record_stride, max_steps = int(nodes), int(record_stride), int(max_steps)
        fragments = [(float(beta), float(dv)) for beta, dv in fragments]
        # (the Python ints, before a 32-bit field can truncate them)
        if not 1 <= len(fragments) <= _abi.DEBRIS_MAX_FRAGMENTS:
            raise ValueError(f"1 to {_abi.DEBRIS_MAX_FRAGMENTS} fragments")
        if not 1 <= nodes <= _abi.IIP_MAX_NODES or nodes * len(fragments) > _abi.CORRIDOR_MAX_NODES:
            raise ValueError(f"1 to {_abi.IIP_MAX_NODES} nodes, at most {_abi.CORRIDOR_MAX_NODES} nodes * fragments")
        if not 1 <= record_stride < 2 ** 31:
            raise ValueError("record_stride must be 1 to 2**31 - 1")
        if not 1 <= max_steps <= _abi.IIP_MAX_STEPS:
            raise ValueError(f"max_steps must be 1 to {_abi.IIP_MAX_STEPS}")
        spec = self._defaults(_abi.ErplDebrisSpec, "erpl_mc_debris_defaults")
        spec.n_nodes, spec.record_stride, spec.max_steps, spec.n_fragments = nodes, record_stride, max_steps, len(fragments)
        spec.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        spec.dt, spec.ground, spec.stiff_limit = float(dt), float(ground), float(stiff_limit)
        spec.origin_x, spec.origin_y = float(origin[0]), float(origin[1])
        for f, (beta, dv) in enumerate(fragments):
            spec.beta[f], spec.dv[f] = beta, dv
        if keep_in is not None:
            keep_in = [(float(x), float(y)) for x, y in keep_in]
            if not 3 <= len(keep_in) <= _abi.IIP_MAX_VERTICES:
                raise ValueError(f"3 to {_abi.IIP_MAX_VERTICES} keep-in vertices")
            spec.n_vertices = len(keep_in)
            for i, (x, y) in enumerate(keep_in):
                spec.keep_x[i], spec.keep_y[i] = x, y
        shape = (_abi.IIP_CH_COUNT, nodes * len(fragments))
        col0 = int(col0)
        if out is None:
            out = torch.full(shape + (col0 + m,), float("nan"), dtype=torch.float64, device=self.device)
        if not (ok(out, torch.float64) and out.dim() == 3 and tuple(out.shape[:2]) == shape):
            raise ValueError(f"out must be a contiguous float64 [{shape[0]}, {shape[1]}, ld] tensor on {self.device}")
        ld = int(out.shape[2])
        if col0 < 0 or col0 + m > ld:
            raise ValueError(f"columns {col0}..{col0 + m} do not fit ld = {ld}")
        summ = torch.empty((_abi.DEBRIS_DIM, m), dtype=torch.float64, device=self.device) if summary else None
        if m == 0:   # (an empty tensor has no address to hand over)
            return out, summ
        b = self._batch_struct(db)
        o = _abi.ErplOut()
        o.n_traj, o.traj_ids, o.traj_cap = m, traj_ids.data_ptr(), cap
        o.traj, o.traj_len = traj.data_ptr(), traj_len.data_ptr()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._call("erpl_mc_debris", C.byref(b), C.byref(o), C.byref(spec), C.c_void_p(out.data_ptr()), ld, col0,
                   C.c_void_p(summ.data_ptr()) if summ is not None else None, C.c_void_p(st.cuda_stream))
        return out, summ

    def casualty(self, values, fragments, p_fail, population, ranges, mask=None, m=None, ke_min=15.0, smooth=True, bw_scale=1.0,
                 h_floor=1.0, levels=(1e-6, 1e-5), want_traj=True):
        """The casualty expectation of a debris footprint (erpl_mc_casualty; the definitions are in include/erpl_mc.h).
        values: the float64 [5, nodes * len(fragments), ld] device tensor of `debris` (or of `impact_points` with one
        fragment), of which the first m columns are read (default ld); fragments: 1 to 64 triples (pieces, casualty area
        in m^2, mass in kg); p_fail: the probability of a break-up in the interval of every node (host values, at most 1
        together; analysis.failure_probabilities); population: float64 [bins_x, bins_y] device tensor, persons / m^2, 1 to
        1024 cells per axis over ranges = ((lo_x, hi_x), (lo_y, hi_y)); mask uint8 [m] on the device, a column counts iff
        its byte is 0.  Enqueued on the current torch stream; blocks the host until the result is there.  Returns the dict
        of analysis.casualty_result_dict; 'ec_traj' (float64 [m] on the device, NaN where the column is not counted; None
        with want_traj=False) and the inputs stay on the device."""
        from . import analysis
        if not (torch.is_tensor(values) and values.is_cuda and values.device == self.device and values.dtype == torch.float64
                and values.dim() == 3 and values.is_contiguous() and values.shape[0] == _abi.IIP_CH_COUNT):
            raise ValueError(f"values must be a contiguous float64 [{_abi.IIP_CH_COUNT}, nodes * fragments, ld] tensor on {self.device}")
        rows, ld = int(values.shape[1]), int(values.shape[2])
        m = ld if m is None else int(m)
        if not 1 <= m <= ld or m >= 2 ** 31:
            raise ValueError(f"m = {m}: 1 to ld = {ld} columns, fewer than 2**31")
        if mask is not None and not (torch.is_tensor(mask) and mask.device == self.device and mask.dtype == torch.uint8
                                     and tuple(mask.shape) == (m,) and mask.is_contiguous()):
            raise ValueError(f"mask must be a contiguous uint8 [m] tensor on {self.device}")
        if not (torch.is_tensor(population) and population.is_cuda and population.device == self.device
                and population.dtype == torch.float64 and population.dim() == 2 and population.is_contiguous()):
            raise ValueError(f"population must be a contiguous float64 [bins_x, bins_y] tensor on {self.device}")
        p_fail = np.ascontiguousarray(np.asarray(p_fail, dtype=np.float64).reshape(-1))
        spec = analysis.casualty_spec(len(p_fail), fragments, tuple(population.shape), ranges, ke_min, smooth, bw_scale, h_floor, levels)
        K, F = spec.n_nodes, spec.n_fragments
        if K * F != rows:
            raise ValueError(f"values holds {rows} rows per channel, p_fail and fragments make {K} * {F}")
        cells = (spec.bins_x, spec.bins_y)
        per_node, per_fragment = np.zeros((_abi.CASUALTY_SPLIT_DIM, K)), np.zeros((_abi.CASUALTY_SPLIT_DIM, F))
        groups = np.zeros((rows, _abi.CASUALTY_GROUP_DIM))
        hazard, words = np.zeros(cells), np.zeros(cells, dtype=np.int64)
        risk = np.zeros(cells) if spec.smooth else None
        ec = torch.empty((m,), dtype=torch.float64, device=self.device) if want_traj else None
        res = _abi.ErplCasualty()
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_casualty", C.c_void_p(values.data_ptr()), ld, m, C.c_void_p(mask.data_ptr()) if mask is not None else None,
                   C.byref(spec), ptr(p_fail), C.c_void_p(population.data_ptr()), C.c_void_p(ec.data_ptr()) if want_traj else None,
                   ptr(per_node), ptr(per_fragment), ptr(groups), ptr(hazard), ptr(words), ptr(risk), C.byref(res),
                   C.c_void_p(st.cuda_stream))
        out = analysis.casualty_result_dict(spec, res, p_fail, per_node, per_fragment, groups, hazard, words, risk)
        out["ec_traj"] = ec
        return out

    def corridor_spec(self, channels=None, nodes=None, t0=None, dt=None, hold=False, quantiles=None):
        """The library's erpl_corridor_spec (erpl_mc_corridor_defaults: altitude, downrange, speed; 256 nodes 1 s apart
        from 0; 5/25/50/75/95 %) with what is given overridden.  channels: _abi.CH_* indices."""
        spec = self._defaults(_abi.ErplCorridorSpec, "erpl_mc_corridor_defaults")
        if channels is not None:
            channels = [int(c) for c in channels]
            if not 1 <= len(channels) <= _abi.CORRIDOR_MAX_CHANNELS:
                raise ValueError(f"1 to {_abi.CORRIDOR_MAX_CHANNELS} channels")
            spec.n_channels = len(channels)
            spec.channels[:len(channels)] = channels
        if nodes is not None:
            spec.n_nodes = int(nodes)
        if t0 is not None:
            spec.t0 = float(t0)
        if dt is not None:
            spec.dt = float(dt)
        spec.flags = _abi.CORRIDOR_HOLD_END if hold else 0
        if quantiles is not None:
            quantiles = self._fractions(quantiles, _abi.ANALYSIS_MAX_Q, "quantiles")
            spec.n_q = len(quantiles)
            spec.q[:len(quantiles)] = quantiles
        return spec

    def corridor_resample(self, traj, traj_len, channels=None, nodes=None, t0=None, dt=None, hold=False, out=None, col0=0,
                          stream=None):
        """Captured trajectories onto one time grid (erpl_mc_corridor_resample; the definitions are in include/erpl_mc.h):
        traj float64 [m, cap, 15] and traj_len int64 [m] are the capture of run(..., traj_ids=...) on the device;
        channels _abi.CH_* (default altitude, downrange, speed), nodes / t0 / dt the grid t_k = t0 + k dt (default 256
        nodes 1 s apart from 0); hold: a trajectory that ended keeps its last value behind its end instead of NaN.
        Trajectory j fills column col0 + j of `out`, a float64 [C, T, ld] device tensor (default: a new one with ld = m,
        NaN everywhere); the other columns are left alone.  Returns `out`; asynchronous on `stream` (default: the
        current stream)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dtype == dtype and t.is_contiguous()
        if not (ok(traj, torch.float64) and traj.dim() == 3 and traj.shape[2] == _abi.TRAJ_DIM):
            raise ValueError(f"traj must be a contiguous float64 [m, cap, {_abi.TRAJ_DIM}] tensor on {self.device}")
        m, cap = int(traj.shape[0]), int(traj.shape[1])
        if not (ok(traj_len, torch.int64) and tuple(traj_len.shape) == (m,)):
            raise ValueError(f"traj_len must be a contiguous int64 [m] tensor on {self.device}")
        spec = self.corridor_spec(channels, nodes, t0, dt, hold)
        shape = (spec.n_channels, spec.n_nodes)
        col0 = int(col0)
        if out is None:
            out = torch.full(shape + (col0 + m,), float("nan"), dtype=torch.float64, device=self.device)
        if not (ok(out, torch.float64) and out.dim() == 3 and tuple(out.shape[:2]) == shape):
            raise ValueError(f"out must be a contiguous float64 [{shape[0]}, {shape[1]}, ld] tensor on {self.device}")
        ld = int(out.shape[2])
        if col0 < 0 or col0 + m > ld:
            raise ValueError(f"columns {col0}..{col0 + m} do not fit ld = {ld}")
        if m == 0:   # (an empty tensor has no address to hand over)
            return out
        o = _abi.ErplOut()
        o.n_traj, o.traj_cap, o.traj, o.traj_len = m, cap, traj.data_ptr(), traj_len.data_ptr()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._call("erpl_mc_corridor_resample", C.byref(o), C.byref(spec), C.c_void_p(out.data_ptr()), ld, col0,
                   C.c_void_p(st.cuda_stream))
        return out

    def corridor_bands(self, values, mask=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), m=None):
        """Every (channel, node) row of a resampled matrix described at once (erpl_mc_corridor_bands): values float64
        [C, T, ld] on the device, of which the first m columns are read (default ld); mask uint8 [m] on the device, a
        column counts iff its byte is 0 (the reason bits of `analyze`).  Enqueued on the current torch stream; blocks
        the host until the result is there.  Returns a dict of NumPy arrays: 'count' int64 [C, T]; 'mean', 'std', 'min',
        'max' float64 [C, T]; 'quantiles', 'order_lo', 'order_hi' float64 [C, n_q, T]; and 'q', 'n_counted'."""
        if not (torch.is_tensor(values) and values.is_cuda and values.device == self.device and values.dtype == torch.float64
                and values.dim() == 3 and values.is_contiguous()):
            raise ValueError(f"values must be a contiguous float64 [C, T, ld] tensor on {self.device}")
        n_ch, n_nodes, ld = (int(s) for s in values.shape)
        m = ld if m is None else int(m)
        if mask is not None and not (torch.is_tensor(mask) and mask.device == self.device and mask.dtype == torch.uint8
                                     and tuple(mask.shape) == (m,) and mask.is_contiguous()):
            raise ValueError(f"mask must be a contiguous uint8 [m] tensor on {self.device}")
        if not 1 <= n_ch <= _abi.CORRIDOR_MAX_CHANNELS:
            raise ValueError(f"1 to {_abi.CORRIDOR_MAX_CHANNELS} channels")
        # (the bands look at the shape of the matrix alone: which channels its rows hold is the caller's knowledge)
        spec = self.corridor_spec(range(n_ch), n_nodes, quantiles=quantiles)
        nq = spec.n_q
        rows = n_ch * n_nodes
        bands = (_abi.ErplRowStats * rows)()
        counted = C.c_int64(0)
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_corridor_bands", C.c_void_p(values.data_ptr()), C.c_void_p(mask.data_ptr()) if mask is not None else None,
                   m, ld, C.byref(spec), C.cast(bands, C.c_void_p), C.byref(counted), C.c_void_p(st.cuda_stream))
        # erpl_row_stats is 29 eight-byte words: count, mean, std, min, max, then three arrays of ANALYSIS_MAX_Q
        raw = np.frombuffer(bands, dtype=np.float64).reshape(n_ch, n_nodes, 5 + 3 * _abi.ANALYSIS_MAX_Q)
        Q = _abi.ANALYSIS_MAX_Q
        out = {"count": np.frombuffer(bands, dtype=np.int64).reshape(n_ch, n_nodes, -1)[:, :, 0].copy(),
               "mean": raw[:, :, 1].copy(), "std": raw[:, :, 2].copy(), "min": raw[:, :, 3].copy(), "max": raw[:, :, 4].copy()}
        for k, name in enumerate(("quantiles", "order_lo", "order_hi")):
            out[name] = np.ascontiguousarray(raw[:, :, 5 + k * Q: 5 + k * Q + nq].transpose(0, 2, 1))
        out["q"] = list(spec.q[:nq])
        out["n_counted"] = int(counted.value)
        return out

    def corridor_bands_weighted(self, values, weights, mask=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), thresholds=None, m=None):
        """Every (channel, node) row of a time-resolved matrix described under the integer weights of `reweight`
        (erpl_mc_corridor_bands_weighted; the definitions are in include/erpl_mc.h): values float64 [C, T, ld] on the device -
        a corridor, an impact-point or a debris matrix as it is - of which the first m columns are read (default ld); weights
        int64 [m] on the device, each in 0..2^Q; mask uint8 [m] on the device, a column counts iff its byte is 0; thresholds:
        per channel up to 4 (analysis.bands_weighted_spec).  Each row over ITS OWN population: mask byte 0, the value finite,
        W > 0.  Enqueued on the current torch stream; blocks the host until the result is there.  Returns the dict of
        analysis.bands_weighted_result_dict: NumPy arrays [C, T] and [C, n_q, T], Python ints for the call record.  The
        quantiles are inverted-cdf order statistics (values of the row), not the interpolated ones of `corridor_bands`."""
        from . import analysis
        if not (torch.is_tensor(values) and values.is_cuda and values.device == self.device and values.dtype == torch.float64
                and values.dim() == 3 and values.is_contiguous()):
            raise ValueError(f"values must be a contiguous float64 [C, T, ld] tensor on {self.device}")
        n_ch, n_nodes, ld = (int(s) for s in values.shape)
        m = ld if m is None else int(m)
        if not 1 <= m <= ld:
            raise ValueError(f"m = {m} outside 1..{ld}")
        if not (torch.is_tensor(weights) and weights.device == self.device and weights.dtype == torch.int64
                and tuple(weights.shape) == (m,) and weights.is_contiguous()):
            raise ValueError(f"weights must be a contiguous int64 [m] tensor on {self.device}")
        if mask is not None and not (torch.is_tensor(mask) and mask.device == self.device and mask.dtype == torch.uint8
                                     and tuple(mask.shape) == (m,) and mask.is_contiguous()):
            raise ValueError(f"mask must be a contiguous uint8 [m] tensor on {self.device}")
        spec = analysis.bands_weighted_spec(n_ch, n_nodes, quantiles, thresholds)
        rows = (_abi.ErplBandsWRow * (n_ch * n_nodes))()
        res = _abi.ErplBandsWResult()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_corridor_bands_weighted", C.c_void_p(values.data_ptr()),
                   C.c_void_p(mask.data_ptr()) if mask is not None else None, C.c_void_p(weights.data_ptr()), m, ld, C.byref(spec),
                   C.cast(rows, C.c_void_p), C.byref(res), C.c_void_p(st.cuda_stream))
        return analysis.bands_weighted_result_dict(spec, rows, res)

    def corridor_drivers(self, factors, values, mask=None, m=None, regression=True):
        """Which factor drives which row of a time-resolved matrix, each row over ITS OWN population
        (erpl_mc_corridor_drivers; the definitions are in include/erpl_mc.h): factors float64 [F, ldf] and values float64
        [C, T, ld] or [R, ld] on the device - a corridor, an impact-point or a debris matrix as it is - of which the first m
        columns are read (default: the shorter of the two); mask uint8 [m] on the device, a column counts iff its byte is 0.
        Enqueued on the current torch stream; blocks the host until the result is there.  Returns a dict of NumPy arrays
        shaped like `values` without its column axis: 'count' int64, 'mean', 'std', 'min', 'max', 'r2', 'pivot_min' float64,
        'constant', 'regression_ok' bool; 'pearson' and 'src' float64 [..., F] ('src' None without the regression); and
        'm', 'n_base', 'n_masked', 'n_factor_non_finite', 'factor_mean' / '_std' / '_min' / '_max' / '_constant' [F]."""
        ok = lambda t: torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dtype == torch.float64 and t.is_contiguous()
        if not (ok(factors) and factors.dim() == 2):
            raise ValueError(f"factors must be a contiguous float64 [F, ldf] tensor on {self.device}")
        if not (ok(values) and values.dim() in (2, 3)):
            raise ValueError(f"values must be a contiguous float64 [C, T, ld] or [R, ld] tensor on {self.device}")
        F, ldf = (int(s) for s in factors.shape)
        shape, ld = tuple(int(s) for s in values.shape[:-1]), int(values.shape[-1])
        R = int(np.prod(shape))
        m = min(ld, ldf) if m is None else int(m)
        if not 1 <= F <= _abi.CDRV_MAX_FACTORS:
            raise ValueError(f"1 to {_abi.CDRV_MAX_FACTORS} factors")
        if not 1 <= R <= _abi.CDRV_MAX_ROWS:
            raise ValueError(f"1 to {_abi.CDRV_MAX_ROWS} rows")
        if not 1 <= m <= min(ld, ldf):
            raise ValueError(f"m = {m} outside 1..{min(ld, ldf)}")
        if mask is not None and not (torch.is_tensor(mask) and mask.device == self.device and mask.dtype == torch.uint8
                                     and tuple(mask.shape) == (m,) and mask.is_contiguous()):
            raise ValueError(f"mask must be a contiguous uint8 [m] tensor on {self.device}")
        spec = self._defaults(_abi.ErplCdrvSpec, "erpl_mc_corridor_drivers_defaults")
        spec.n_factors, spec.n_rows, spec.regression = F, R, int(bool(regression))
        res = _abi.ErplCdrvResult()
        rows = (_abi.ErplCdrvRow * R)()
        pearson = np.empty((R, F), dtype=np.float64)
        src = np.empty((R, F), dtype=np.float64) if regression else None
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_corridor_drivers", C.c_void_p(factors.data_ptr()), ldf, C.c_void_p(values.data_ptr()), ld,
                   C.c_void_p(mask.data_ptr()) if mask is not None else None, m, C.byref(spec), C.byref(res),
                   C.cast(rows, C.c_void_p), C.c_void_p(pearson.ctypes.data),
                   C.c_void_p(src.ctypes.data) if regression else None, C.c_void_p(st.cuda_stream))
        # erpl_cdrv_row is 8 eight-byte words: count, mean, std, min, max, r2, pivot_min, then (constant, regression_ok)
        raw = np.frombuffer(rows, dtype=np.float64).reshape(R, 8)
        flags = np.frombuffer(rows, dtype=np.int32).reshape(R, 16)
        out = {"count": np.frombuffer(rows, dtype=np.int64).reshape(R, 8)[:, 0].reshape(shape).copy()}
        for k, name in enumerate(("mean", "std", "min", "max", "r2", "pivot_min")):
            out[name] = raw[:, 1 + k].reshape(shape).copy()
        out["constant"] = flags[:, 14].reshape(shape) != 0
        out["regression_ok"] = flags[:, 15].reshape(shape) != 0
        out["pearson"] = pearson.reshape(shape + (F,))
        out["src"] = src.reshape(shape + (F,)) if regression else None
        out.update({"m": int(res.m), "n_base": int(res.n_base), "n_masked": int(res.n_masked),
                    "n_factor_non_finite": int(res.n_factor_non_finite),
                    "factor_constant": np.array(res.constant[:F], dtype=np.int32) != 0})
        for k in ("mean", "std", "min", "max"):
            out["factor_" + k] = np.array(getattr(res, k)[:F], dtype=np.float64)
        return out

    def corridor_depth(self, values, mask=None, m=None, central=0.5, factor=1.5, lds_limit=0):
        """Band depth and the functional boxplot of a time-resolved matrix (erpl_mc_corridor_depth; the definitions are in
        include/erpl_mc.h): values float64 [C, T, ld] on the device - a corridor, an impact-point or a debris matrix as it is -
        of which the first m columns are read (default: ld); mask uint8 [m] on the device, a column counts iff its byte is 0.
        Enqueued on the current torch stream; blocks the host until the result is there.  Returns a dict: NumPy row arrays
        [C, T] 'count', 'n_central_here' int64 and 'central_lo', 'central_hi', 'fence_lo', 'fence_hi', 'whisker_lo',
        'whisker_hi' float64; per channel [C] 'n_defined', 'n_central', 'n_outliers', 'median' int64 and 'threshold',
        'depth_max' float64; 'm', 'n_masked'; and the per-column arrays as DEVICE tensors [C, m]: 'depth', 'mei' float64,
        'nodes', 'n_out', 'first_out' int32, 'central' uint8."""
        if not (torch.is_tensor(values) and values.is_cuda and values.device == self.device and values.dtype == torch.float64
                and values.is_contiguous() and values.dim() == 3):
            raise ValueError(f"values must be a contiguous float64 [C, T, ld] tensor on {self.device}")
        Cn, T, ld = (int(s) for s in values.shape)
        m = ld if m is None else int(m)
        if not 1 <= Cn <= _abi.DEPTH_MAX_CHANNELS:
            raise ValueError(f"1 to {_abi.DEPTH_MAX_CHANNELS} channels")
        if not 1 <= T <= _abi.DEPTH_MAX_NODES:
            raise ValueError(f"1 to {_abi.DEPTH_MAX_NODES} nodes")
        if not 1 <= m <= ld:
            raise ValueError(f"m = {m} outside 1..{ld}")
        if mask is not None and not (torch.is_tensor(mask) and mask.device == self.device and mask.dtype == torch.uint8
                                     and tuple(mask.shape) == (m,) and mask.is_contiguous()):
            raise ValueError(f"mask must be a contiguous uint8 [m] tensor on {self.device}")
        spec = self._defaults(_abi.ErplDepthSpec, "erpl_mc_corridor_depth_defaults")
        spec.n_channels, spec.n_nodes, spec.central, spec.factor, spec.lds_limit = Cn, T, float(central), float(factor), int(lds_limit)
        res = _abi.ErplDepthResult()
        rows = (_abi.ErplDepthRow * (Cn * T))()
        cols = {"depth": torch.empty((Cn, m), dtype=torch.float64, device=self.device),
                "mei": torch.empty((Cn, m), dtype=torch.float64, device=self.device),
                "nodes": torch.empty((Cn, m), dtype=torch.int32, device=self.device),
                "n_out": torch.empty((Cn, m), dtype=torch.int32, device=self.device),
                "first_out": torch.empty((Cn, m), dtype=torch.int32, device=self.device),
                "central": torch.empty((Cn, m), dtype=torch.uint8, device=self.device)}
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_corridor_depth", C.c_void_p(values.data_ptr()), ld,
                   C.c_void_p(mask.data_ptr()) if mask is not None else None, m, C.byref(spec), C.byref(res),
                   C.cast(rows, C.c_void_p), *(C.c_void_p(cols[k].data_ptr()) for k in ("depth", "mei", "nodes", "n_out", "first_out",
                                                                                         "central")), C.c_void_p(st.cuda_stream))
        # erpl_depth_row is 8 eight-byte words: count, n_central_here, then the six doubles
        raw = np.frombuffer(rows, dtype=np.float64).reshape(Cn, T, 8)
        ints = np.frombuffer(rows, dtype=np.int64).reshape(Cn, T, 8)
        out = {"count": ints[:, :, 0].copy(), "n_central_here": ints[:, :, 1].copy()}
        for k, name in enumerate(("central_lo", "central_hi", "fence_lo", "fence_hi", "whisker_lo", "whisker_hi")):
            out[name] = raw[:, :, 2 + k].copy()
        for name in ("n_defined", "n_central", "n_outliers", "median"):
            out[name] = np.array(getattr(res, name)[:Cn], dtype=np.int64)
        for name in ("threshold", "depth_max"):
            out[name] = np.array(getattr(res, name)[:Cn], dtype=np.float64)
        out.update({"m": int(res.m), "n_masked": int(res.n_masked)})
        out.update(cols)
        return out

    def analysis_defaults(self):
        """The reference's outlier bounds, rows and quantiles (erpl_mc_analysis_defaults)."""
        return self._defaults(_abi.ErplAnalysisSpec, "erpl_mc_analysis_defaults")

    def analyze(self, summary, status=None, rows=None, quantiles=None, bounds=None, reasons=False):
        """Outlier filter + exact statistics of a [16, n] summary on the device (erpl_mc_analyze), enqueued on the
        current torch stream; blocks the host until the result is there.  rows: summary rows to describe (default
        apogee, range, flight time); quantiles: fractions in [0, 1] (default 5/25/50/75/95 %); bounds: dict overriding
        max_apogee / min_apogee / max_range / max_flight_time / energy_apogee.  Returns (_abi.ErplAnalysis, reason
        bits [n] uint8 on the device or None).  Raises _abi.IncompleteBatch for status words with ST_INCOMPLETE."""
        n = self._check_summary(summary)
        if status is not None and not (status.device == self.device and status.dtype == torch.int32
                                       and tuple(status.shape) == (n,) and status.is_contiguous()):
            raise ValueError(f"status must be a contiguous int32 [n] tensor on {self.device}")
        spec = self.analysis_defaults()
        self._set_rows(spec, rows, 0, _abi.ANALYSIS_MAX_ROWS)
        if quantiles is not None:
            quantiles = self._fractions(quantiles, _abi.ANALYSIS_MAX_Q, "quantiles")
            spec.n_q = len(quantiles)
            spec.q[:len(quantiles)] = quantiles
        for key, val in (bounds or {}).items():
            if key not in ("max_apogee", "min_apogee", "max_range", "max_flight_time", "energy_apogee"):
                raise ValueError(f"unknown bound {key!r}")
            setattr(spec, key, float(val))
        why = torch.empty((n,), dtype=torch.uint8, device=self.device) if reasons else None
        res = _abi.ErplAnalysis()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_analyze", C.c_void_p(summary.data_ptr()),
                   C.c_void_p(status.data_ptr()) if status is not None else None, n, C.byref(spec), C.byref(res),
                   C.c_void_p(why.data_ptr()) if reasons else None, C.c_void_p(st.cuda_stream))
        return res, why

    def _summary_and_mask(self, summary, mask):
        """The host-side refusals of the distribution calls: there is no CPU path behind them."""
        n = self._check_summary(summary)
        if mask is not None and not (mask.device == self.device and mask.dtype == torch.uint8
                                     and tuple(mask.shape) == (n,) and mask.is_contiguous()):
            raise ValueError(f"mask must be a contiguous uint8 [n] tensor on {self.device}")
        return n, C.c_void_p(mask.data_ptr()) if mask is not None else None

    @staticmethod
    def _range_of(r):
        if r is None:
            return float("nan"), float("nan")
        lo, hi = r
        return float(lo), float(hi)

    def histogram(self, summary, mask=None, rows=None, bins=50, ranges=None):
        """np.histogram of up to 16 rows of a [16, n] summary on the device (erpl_mc_histogram), enqueued on the current
        torch stream; blocks the host until the counts are there.  mask: uint8 [n] on the device, a sample counts iff
        its byte is 0 (the reason bits of `analyze`); rows: summary rows (default apogee, range, flight time); bins: one
        int or one per row (1..1024); ranges: None (min / max of the counted values) or one (lo, hi) / None per row.
        Returns (edges, counts, info): two lists of NumPy arrays, bins[j] + 1 float64 edges and bins[j] int64 counts per
        row - equal to np.histogram(finite masked values, bins, range) - and a dict of per-row lists counted / below /
        above / lo / hi."""
        n, mask_p = self._summary_and_mask(summary, mask)
        spec = self._defaults(_abi.ErplHistSpec, "erpl_mc_histogram_defaults")
        self._set_rows(spec, rows, 1, _abi.HIST_MAX_ROWS)
        m = spec.n_rows
        bins = [int(bins)] * m if np.isscalar(bins) else [int(b) for b in bins]
        ranges = [None] * m if ranges is None else list(ranges)
        if len(bins) != m or len(ranges) != m:
            raise ValueError("bins and ranges: one entry per row")
        for j in range(m):
            spec.bins[j] = bins[j]
            spec.lo[j], spec.hi[j] = self._range_of(ranges[j])
        edges = np.zeros((m, _abi.HIST_MAX_BINS + 1), dtype=np.float64)
        counts = np.zeros((m, _abi.HIST_MAX_BINS), dtype=np.int64)
        res = _abi.ErplHistResult()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_histogram", C.c_void_p(summary.data_ptr()), mask_p, n, C.byref(spec),
                   C.c_void_p(edges.ctypes.data), C.c_void_p(counts.ctypes.data), C.byref(res),
                   C.c_void_p(st.cuda_stream))
        info = {k: list(getattr(res, k)[:m]) for k in ("counted", "below", "above", "lo", "hi")}
        return ([edges[j, :bins[j] + 1].copy() for j in range(m)], [counts[j, :bins[j]].copy() for j in range(m)], info)

    def histogram2d(self, summary, mask=None, row_x=_abi.SUM_APOGEE_ALT, row_y=_abi.SUM_RANGE, bins=50, ranges=None):
        """np.histogram2d of two rows of a [16, n] summary on the device (erpl_mc_histogram_xy).  bins: one int or
        (bins_x, bins_y), up to 256 each; ranges: None or ((lo_x, hi_x) | None, (lo_y, hi_y) | None).  A sample is counted
        iff its mask byte is 0 and both values are finite.  Returns (counts int64 [bins_x, bins_y], edges_x, edges_y,
        info dict: counted, outside, lo_x, hi_x, lo_y, hi_y)."""
        n, mask_p = self._summary_and_mask(summary, mask)
        bx, by = (int(bins), int(bins)) if np.isscalar(bins) else (int(bins[0]), int(bins[1]))
        rx, ry = (None, None) if ranges is None else ranges
        spec = _abi.ErplHist2dSpec(int(row_x), int(row_y), bx, by, *self._range_of(rx), *self._range_of(ry))
        cap = _abi.HIST2D_MAX_BINS
        ex, ey = np.zeros(cap + 1, dtype=np.float64), np.zeros(cap + 1, dtype=np.float64)
        counts = np.zeros(max(1, min(bx, cap)) * max(1, min(by, cap)), dtype=np.int64)   # out-of-range bins are refused below
        res = _abi.ErplHist2dResult()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_histogram_xy", C.c_void_p(summary.data_ptr()), mask_p, n, C.byref(spec),
                   C.c_void_p(ex.ctypes.data), C.c_void_p(ey.ctypes.data), C.c_void_p(counts.ctypes.data), C.byref(res),
                   C.c_void_p(st.cuda_stream))
        info = {k: getattr(res, k) for k in ("counted", "outside", "lo_x", "hi_x", "lo_y", "hi_y")}
        return counts.reshape(bx, by), ex[:bx + 1].copy(), ey[:by + 1].copy(), info

    def dispersion(self, summary, mask=None, row_x=_abi.SUM_IMPACT_X, row_y=_abi.SUM_IMPACT_Y, centre=(0.0, 0.0),
                   levels=(0.5, 0.9, 0.99), quantiles=(0.5, 0.9, 0.95, 0.99), miss=False):
        """Where the vehicle lands (erpl_mc_dispersion): count, mean, population covariance and its principal axes of the
        (row_x, row_y) cloud over the samples with mask byte 0 and both values finite, the confidence ellipses of `levels`
        with the number of samples each one actually contains (-1 for a degenerate cloud), and the miss distance about
        `centre` - a point (x, y), default the launch site, or None for the mean - as count / mean / std / min / max /
        exact quantiles (with the default quantiles the first one is the CEP).  Returns a plain dict; miss=True adds
        'miss_distance', the float64 [n] device tensor of r (NaN where a sample is not counted)."""
        n, mask_p = self._summary_and_mask(summary, mask)
        levels = self._fractions(levels, _abi.DISP_MAX_LEVELS, "levels")
        quantiles = self._fractions(quantiles, _abi.ANALYSIS_MAX_Q, "quantiles")
        spec = self._defaults(_abi.ErplDispersionSpec, "erpl_mc_dispersion_defaults")
        spec.row_x, spec.row_y = int(row_x), int(row_y)
        if centre is None:
            spec.centre = _abi.CENTRE_MEAN
        else:
            spec.centre, spec.cx, spec.cy = _abi.CENTRE_POINT, float(centre[0]), float(centre[1])
        spec.n_levels = len(levels)
        spec.level[:len(levels)] = levels
        spec.n_q = len(quantiles)
        spec.q[:len(quantiles)] = quantiles
        r = torch.empty((n,), dtype=torch.float64, device=self.device) if miss else None
        res = _abi.ErplDispersion()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_dispersion", C.c_void_p(summary.data_ptr()), mask_p, n, C.byref(spec), C.byref(res),
                   C.c_void_p(r.data_ptr()) if miss else None, C.c_void_p(st.cuda_stream))
        nl = len(levels)
        out = {"count": int(res.count), "rows": (int(row_x), int(row_y)),
               "mean": [res.mean_x, res.mean_y],
               "covariance": [[res.cov_xx, res.cov_xy], [res.cov_xy, res.cov_yy]],
               "var_major": res.var_major, "var_minor": res.var_minor, "angle": res.angle,
               "centre": [res.centre_x, res.centre_y],
               "ellipses": [{"level": levels[k], "k2": res.k2[k], "semi_major": res.semi_major[k],
                             "semi_minor": res.semi_minor[k], "inside": int(res.inside[k])} for k in range(nl)],
               "miss": self._row_stats_dict(res.miss, quantiles)}
        out["cep"] = out["miss"]["quantiles"][quantiles.index(0.5)] if 0.5 in quantiles else None
        if miss:
            out["miss_distance"] = r
        return out

    def _density_spec(self, rows, nodes, ranges, pad, bandwidth, levels, zones):
        """The erpl_density_spec of impact_density / impact_density_weighted from their keywords, and the host arrays of a
        call: (spec, levels, zones, nx, ny, grid_x, grid_y, density)."""
        levels = self._fractions(levels, _abi.DENSITY_MAX_LEVELS, "levels")
        zones = [np.asarray(z, dtype=np.float64).reshape(-1, 2) for z in (zones or [])]
        if len(zones) > _abi.DENSITY_MAX_ZONES:
            raise ValueError(f"at most {_abi.DENSITY_MAX_ZONES} zones")
        if sum(len(z) for z in zones) > _abi.DENSITY_MAX_VERTICES:
            raise ValueError(f"at most {_abi.DENSITY_MAX_VERTICES} zone vertices together")
        spec = self._defaults(_abi.ErplDensitySpec, "erpl_mc_impact_density_defaults")
        spec.row_x, spec.row_y = int(rows[0]), int(rows[1])
        spec.nodes_x, spec.nodes_y = int(nodes[0]), int(nodes[1])
        rx, ry = (None, None) if ranges is None else ranges
        (spec.lo_x, spec.hi_x), (spec.lo_y, spec.hi_y) = self._range_of(rx), self._range_of(ry)
        spec.pad = float(pad)
        if bandwidth is None or np.isscalar(bandwidth):
            spec.bandwidth, spec.bw_scale = _abi.BW_SCOTT, 1.0 if bandwidth is None else float(bandwidth)
        else:
            hm = np.asarray(bandwidth, dtype=np.float64)
            if hm.shape != (2, 2) or hm[0, 1] != hm[1, 0]:
                raise ValueError("bandwidth: None, a factor or a symmetric 2 x 2 matrix")
            spec.bandwidth, spec.h_xx, spec.h_xy, spec.h_yy = _abi.BW_MATRIX, hm[0, 0], hm[0, 1], hm[1, 1]
        spec.n_levels = len(levels)
        spec.level[:len(levels)] = levels
        spec.n_zones, at = len(zones), 0
        for z, poly in enumerate(zones):
            spec.zone_first[z] = at
            spec.zone_x[at:at + len(poly)] = poly[:, 0].tolist()
            spec.zone_y[at:at + len(poly)] = poly[:, 1].tolist()
            at += len(poly)
        spec.zone_first[len(zones)] = at
        cap = _abi.DENSITY_MAX_NODES
        nx, ny = max(2, min(spec.nodes_x, cap)), max(2, min(spec.nodes_y, cap))   # out-of-range nodes are refused below
        gx, gy = np.zeros(cap, dtype=np.float64), np.zeros(cap, dtype=np.float64)
        dens = np.zeros(nx * ny, dtype=np.float64)
        return spec, levels, zones, nx, ny, gx, gy, dens

    def impact_density(self, summary, mask=None, rows=(_abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y), nodes=(128, 128), ranges=None,
                       pad=3.0, bandwidth=None, levels=(0.5, 0.9, 0.99), zones=None, sample_density=False):
        """The impact probability map (erpl_mc_impact_density): a Gaussian kernel density estimate of the (rows[0], rows[1])
        cloud over the samples with mask byte 0 and both values finite, evaluated at the nodes[0] x nodes[1] nodes of a grid
        (2..512 per axis).  ranges: None or ((lo_x, hi_x) | None, (lo_y, hi_y) | None), None = min / max of the counted
        values -+ `pad` bandwidth standard deviations.  bandwidth: None = Scott's rule (scipy.stats.gaussian_kde's default),
        a float = Scott's rule times that factor, a 2 x 2 matrix = H as given.  levels: contents of the highest-density
        regions; zones: polygons, each an array of (x, y) vertices.  Returns a dict: count, solid, mean, covariance (divisor
        count - 1), bandwidth_matrix, det, norm, ranges, grid_x, grid_y, density ([nodes_x, nodes_y], x-major), peak,
        peak_node, grid_mass, levels, thresholds (density >= thresholds[k] is the region of content levels[k]),
        sample_density_stats (count / mean / std / min / max / q / quantiles / order_lo / order_hi of the density at the
        samples), zones ([{'vertices', 'inside'}]).  sample_density=True adds 'sample_density', the float64 [n] device
        tensor of the density at every sample (NaN where it is not counted); with no levels and without it the pass over
        all pairs of samples is skipped."""
        n, mask_p = self._summary_and_mask(summary, mask)
        spec, levels, zones, nx, ny, gx, gy, dens = self._density_spec(rows, nodes, ranges, pad, bandwidth, levels, zones)
        row = torch.empty((n,), dtype=torch.float64, device=self.device) if sample_density else None
        res = _abi.ErplDensity()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_impact_density", C.c_void_p(summary.data_ptr()), mask_p, n, C.byref(spec),
                   C.c_void_p(gx.ctypes.data), C.c_void_p(gy.ctypes.data), C.c_void_p(dens.ctypes.data), C.byref(res),
                   C.c_void_p(row.data_ptr()) if sample_density else None, C.c_void_p(st.cuda_stream))
        nl, sd = len(levels), res.sample_density
        out = {"count": int(res.count), "solid": bool(res.solid), "rows": (spec.row_x, spec.row_y),
               "mean": [res.mean_x, res.mean_y],
               "covariance": [[res.cov_xx, res.cov_xy], [res.cov_xy, res.cov_yy]],
               "bandwidth_matrix": [[res.h_xx, res.h_xy], [res.h_xy, res.h_yy]], "det": res.det, "norm": res.norm,
               "ranges": ((res.lo_x, res.hi_x), (res.lo_y, res.hi_y)),
               "grid_x": gx[:nx].copy(), "grid_y": gy[:ny].copy(), "density": dens.reshape(nx, ny),
               "peak": res.peak, "peak_node": (int(res.peak_ix), int(res.peak_iy)), "grid_mass": res.grid_mass,
               "levels": levels, "thresholds": list(sd.quantile[:nl]),
               "sample_density_stats": self._row_stats_dict(sd, [1.0 - p for p in levels]),
               "zones": [{"vertices": poly, "inside": int(res.zone_inside[z])} for z, poly in enumerate(zones)]}
        if sample_density:
            out["sample_density"] = row
        return out

    def impact_density_weighted(self, summary, weights, mask=None, rows=(_abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y), nodes=(128, 128),
                                ranges=None, pad=3.0, bandwidth=None, levels=(0.5, 0.9, 0.99), zones=None, sample_density=False):
        """The impact probability map under weights (erpl_mc_impact_density_weighted): `impact_density` of a flown run under
        another law.  weights: the int64 [n] device tensor TrajectoryEngine.reweight(want_weights=True) returns, 0 <= W <=
        2^Q; a sample counts iff its mask byte is 0, both values are finite and W > 0.  The keywords are those of
        `impact_density`; bandwidth None / a float is Scott's rule on the effective sample size (scipy's `neff`).  Returns a
        dict: count, n_masked, n_non_finite, n_zero, sum_w, max_w (Python ints), sum_w2 (in weights scaled by 2^-bit_length(
        max_w)), ess, solid, mean, covariance (np.cov(aweights=)), bandwidth_matrix, det, norm, ranges, grid_x, grid_y,
        density, peak, peak_node, grid_mass, levels, thresholds (np.quantile(f, 1 - level, weights=, method="inverted_cdf")
        of the density at the samples), content_w (the weight at or above each threshold), f_min, f_max, zones ([{'vertices',
        'weight', 'a2'}]: the exact weight inside and the sum of the squared scaled weights inside).  sample_density=True
        adds 'sample_density', the float64 [n] device tensor (NaN where a sample is not counted)."""
        n, mask_p = self._summary_and_mask(summary, mask)
        if not (torch.is_tensor(weights) and weights.dtype == torch.int64 and weights.device == summary.device
                and tuple(weights.shape) == (n,) and weights.is_contiguous()):
            raise ValueError(f"weights must be a contiguous int64 [{n}] tensor on the summary's device")
        spec, levels, zones, nx, ny, gx, gy, dens = self._density_spec(rows, nodes, ranges, pad, bandwidth, levels, zones)
        row = torch.empty((n,), dtype=torch.float64, device=self.device) if sample_density else None
        res = _abi.ErplDensityW()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_impact_density_weighted", C.c_void_p(summary.data_ptr()), mask_p, C.c_void_p(weights.data_ptr()), n,
                   C.byref(spec), C.c_void_p(gx.ctypes.data), C.c_void_p(gy.ctypes.data), C.c_void_p(dens.ctypes.data),
                   C.byref(res), C.c_void_p(row.data_ptr()) if sample_density else None, C.c_void_p(st.cuda_stream))
        nl = len(levels)
        out = {k: int(getattr(res, k)) for k in ("count", "n_masked", "n_non_finite", "n_zero", "sum_w", "max_w")}
        out.update({"sum_w2": res.sum_w2, "ess": res.ess, "solid": bool(res.solid), "rows": (spec.row_x, spec.row_y),
                    "mean": [res.mean_x, res.mean_y],
                    "covariance": [[res.cov_xx, res.cov_xy], [res.cov_xy, res.cov_yy]],
                    "bandwidth_matrix": [[res.h_xx, res.h_xy], [res.h_xy, res.h_yy]], "det": res.det, "norm": res.norm,
                    "ranges": ((res.lo_x, res.hi_x), (res.lo_y, res.hi_y)),
                    "grid_x": gx[:nx].copy(), "grid_y": gy[:ny].copy(), "density": dens.reshape(nx, ny),
                    "peak": res.peak, "peak_node": (int(res.peak_ix), int(res.peak_iy)), "grid_mass": res.grid_mass,
                    "levels": levels, "thresholds": list(res.threshold[:nl]),
                    "content_w": [int(v) for v in res.content_w[:nl]], "f_min": res.f_min, "f_max": res.f_max,
                    "zones": [{"vertices": poly, "weight": int(res.zone_w[z]), "a2": res.zone_a2[z]}
                              for z, poly in enumerate(zones)]})
        if sample_density:
            out["sample_density"] = row
        return out

    def correlation(self, factors, summary, mask=None, rows=None, ranks=True, want_ranks=False):
        """Which factor drives which outcome (erpl_mc_correlation): Pearson and - with ranks=True - Spearman correlation
        and the standardised (rank) regression coefficients between the rows of `factors` (float64 [F, n] on the device,
        F <= 32) and summary rows `rows` (default apogee, range, flight time), over ONE population: mask byte 0 and every
        factor and every requested row finite.  V = F + R variables, the factors first.  Returns a dict: count, n_masked,
        n_non_finite, mean / std / min / max / constant (NumPy, length V), pearson / spearman / src / srrc ([R, F]),
        r2 / r2_rank ([R]), regression_ok / rank_regression_ok, corr / rank_corr ([V, V]; rank_corr is None without
        ranks) and, with want_ranks=True, 'ranks': the float64 [V, n] device tensor of mid-ranks (NaN outside the
        population).  A constant variable (min == max) has NaN correlations; factors that are affine images of each other
        leave the correlations in place and set regression_ok = 0 (every src / r2 NaN)."""
        n, mask_p = self._summary_and_mask(summary, mask)
        if not (factors.is_cuda and factors.device == self.device and factors.dtype == torch.float64
                and factors.dim() == 2 and factors.shape[1] == n and factors.is_contiguous()):
            raise ValueError(f"factors must be a contiguous float64 [F, n] tensor on {self.device}")
        F = int(factors.shape[0])
        if not 1 <= F <= _abi.CORR_MAX_FACTORS:
            raise ValueError(f"1 to {_abi.CORR_MAX_FACTORS} factors")
        if want_ranks and not ranks:
            raise ValueError("want_ranks needs ranks=True")
        spec = self._defaults(_abi.ErplCorrSpec, "erpl_mc_correlation_defaults")
        self._set_rows(spec, rows, 1, _abi.CORR_MAX_ROWS)
        spec.n_factors, spec.ranks = F, int(bool(ranks))
        R = spec.n_rows
        V = F + R
        corr = np.empty((V, V), dtype=np.float64)
        rank_corr = np.empty((V, V), dtype=np.float64) if ranks else None
        rk = torch.empty((V, n), dtype=torch.float64, device=self.device) if want_ranks else None
        res = _abi.ErplCorrResult()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_correlation", C.c_void_p(factors.data_ptr()), C.c_void_p(summary.data_ptr()), mask_p, n,
                   C.byref(spec), C.byref(res), C.c_void_p(corr.ctypes.data),
                   C.c_void_p(rank_corr.ctypes.data) if ranks else None,
                   C.c_void_p(rk.data_ptr()) if want_ranks else None, C.c_void_p(st.cuda_stream))
        out = {"n": int(res.n), "count": int(res.count), "n_masked": int(res.n_masked),
               "n_non_finite": int(res.n_non_finite), "rows": list(spec.rows[:R]), "n_factors": F,
               "constant": np.array(res.constant[:V], dtype=np.int32)}
        for k in ("mean", "std", "min", "max"):
            out[k] = np.array(getattr(res, k)[:V], dtype=np.float64)
        for k in ("pearson", "spearman", "src", "srrc"):
            out[k] = np.ctypeslib.as_array(getattr(res, k))[:R, :F].copy()
        out["r2"] = np.array(res.r2[:R], dtype=np.float64)
        out["r2_rank"] = np.array(res.r2_rank[:R], dtype=np.float64)
        out["regression_ok"], out["rank_regression_ok"] = bool(res.regression_ok), bool(res.rank_regression_ok)
        out["corr"], out["rank_corr"] = corr, rank_corr
        if want_ranks:
            out["ranks"] = rk
        return out

    def design(self, rows_kinds, n, seed, kind="lhs", block=0, first=0, count=None, first_row=0, out=None):
        """Columns first .. first + count - 1 (default: all from `first`) of the design (seed, kind, n, block, first_row) of
        erpl_mc_design, drawn on the device: one row per entry of `rows_kinds` (_abi.DESIGN_UNIFORM: the probability in
        (0, 1); _abi.DESIGN_NORMAL: its normal quantile; a sequence or a bytes object), the global rows first_row ...
        kind: 'random', 'lhs' or 'lhs_centred' (or the _abi.DESIGN_* value; 'qmc' is `qmc` below, refused here); block: the columns of a replicate, a divisor
        of n, 0 = n.  Counter-based: a window equals those columns of the whole design bit for bit, wherever and in
        whatever pieces it is generated.  out: None (a new float64 [rows, count] tensor) or a float64 device tensor
        [rows, ld] with unit column stride and ld >= count, of which columns 0 .. count - 1 are written.  Asynchronous on
        the current stream; returns the tensor."""
        kinds = bytes(bytearray(int(k) for k in rows_kinds))
        n, first = int(n), int(first)
        count = n - first if count is None else int(count)
        spec = self._defaults(_abi.ErplDesignSpec, "erpl_mc_design_defaults")
        spec.kind = _abi.DESIGN_KINDS[kind] if isinstance(kind, str) else int(kind)
        spec.rows, spec.first_row, spec.n, spec.block = len(kinds), int(first_row), n, int(block)
        spec.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if out is None:
            out = torch.empty((len(kinds), max(count, 0)), dtype=torch.float64, device=self.device)
        if not (torch.is_tensor(out) and out.is_cuda and out.device == self.device and out.dtype == torch.float64
                and out.dim() == 2 and out.shape[0] == len(kinds) and out.shape[1] >= count
                and (out.shape[1] == 0 or out.stride(1) == 1) and (out.shape[0] == 1 or out.stride(0) >= out.shape[1])):
            raise ValueError(f"out must be a float64 [{len(kinds)}, >= {count}] tensor on {self.device} with unit column stride")
        ld = out.stride(0) if out.shape[0] > 1 else max(out.shape[1], 1)
        st = torch.cuda.current_stream(self.device)
        if count == 0 and out.numel() == 0:   # an empty tensor has no storage to point at, and count == 0 writes nothing
            return out
        self._call("erpl_mc_design", C.byref(spec), kinds, first, count, C.c_void_p(out.data_ptr()), ld,
                   C.c_void_p(st.cuda_stream))
        return out

    def qmc(self, rows_kinds, n, seed, dims=None, scramble="owen", pad="random", block=0, first=0, count=None, first_row=0,
            out=None):
        """Columns first .. first + count - 1 (default: all from `first`) of the scrambled Sobol' design (seed, n, block,
        scramble, pad, first_row, dims) of erpl_mc_qmc, drawn on the device: one row per entry of `rows_kinds` as in `design`.
        dims: per row its Sobol' dimension 0 .. 1023 or -1 for a pad row, which is the row `design(kind=pad)` writes for the
        same global row; None: the global row where that is below 1024, -1 beyond.  scramble: 'owen' or 'raw' (or the
        _abi.QMC_* value; 'raw' is for comparisons, not for flights); pad: 'random' or 'lhs'.  block: the columns of a
        replicate, an independently scrambled copy of the net; 0 = n.  With block 0 and pad 'random' no column depends on n:
        a longer run continues a shorter one.  Counter-based, `out`, the stream and the return value as `design`."""
        kinds = bytes(bytearray(int(k) for k in rows_kinds))
        n, first = int(n), int(first)
        count = n - first if count is None else int(count)
        spec = self._defaults(_abi.ErplQmcSpec, "erpl_mc_qmc_defaults")
        spec.scramble = _abi.QMC_SCRAMBLES[scramble] if isinstance(scramble, str) else int(scramble)
        spec.pad = _abi.QMC_PADS[pad] if isinstance(pad, str) else int(pad)
        spec.rows, spec.first_row, spec.n, spec.block = len(kinds), int(first_row), n, int(block)
        spec.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        dims_arg = None
        if dims is not None:
            dims = [int(d) for d in dims]
            if len(dims) != len(kinds):
                raise ValueError(f"dims has {len(dims)} entries for {len(kinds)} rows")
            dims_arg = (C.c_int32 * len(dims))(*dims)
        if out is None:
            out = torch.empty((len(kinds), max(count, 0)), dtype=torch.float64, device=self.device)
        if not (torch.is_tensor(out) and out.is_cuda and out.device == self.device and out.dtype == torch.float64
                and out.dim() == 2 and out.shape[0] == len(kinds) and out.shape[1] >= count
                and (out.shape[1] == 0 or out.stride(1) == 1) and (out.shape[0] == 1 or out.stride(0) >= out.shape[1])):
            raise ValueError(f"out must be a float64 [{len(kinds)}, >= {count}] tensor on {self.device} with unit column stride")
        ld = out.stride(0) if out.shape[0] > 1 else max(out.shape[1], 1)
        st = torch.cuda.current_stream(self.device)
        if count == 0 and out.numel() == 0:   # an empty tensor has no storage to point at, and count == 0 writes nothing
            return out
        self._call("erpl_mc_qmc", C.byref(spec), kinds, dims_arg, first, count, C.c_void_p(out.data_ptr()), ld,
                   C.c_void_p(st.cuda_stream))
        return out

    # ---- subset simulation (erpl_mc_subset_*): the five steps of a level on device tensors; analysis.subset_simulation drives them
    def _matrix(self, t, what):
        """A device matrix the subset calls read or write in place: 1-D or 2-D with unit column stride.  (rows, ld, bytes)."""
        if not (torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dim() in (1, 2)
                and (t.shape[-1] <= 1 or t.stride(-1) == 1) and t.element_size() in (1, 4, 8)):
            raise ValueError(f"{what} must be a 1-D or 2-D tensor on {self.device} with unit column stride and 1, 4 or 8 byte elements")
        if t.dim() == 1 or t.shape[0] == 1:
            return 1, max(int(t.shape[-1]), 1), t.element_size()
        if t.stride(0) < t.shape[1]:
            raise ValueError(f"{what}: rows must not overlap")
        return int(t.shape[0]), int(t.stride(0)), t.element_size()

    def _vector(self, t, n, dtype, what):
        if not (torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dtype == dtype and t.dim() == 1
                and t.shape[0] == n and (n <= 1 or t.stride(0) == 1)):
            raise ValueError(f"{what} must be a {dtype} [{n}] tensor on {self.device} with unit stride")
        return C.c_void_p(t.data_ptr())

    def subset_limit_state(self, spec, summary, status=None, out=None):
        """erpl_mc_subset_limit_state: g [n] of the summary [16, n] (unit column stride) / status [n] under `spec`
        (analysis.subset_spec).  Asynchronous on the current stream."""
        rows, ld, _ = self._matrix(summary, "summary")
        n = int(summary.shape[1])
        if rows != _abi.SUMMARY_DIM or summary.dtype != torch.float64:
            raise ValueError(f"summary must be float64 [{_abi.SUMMARY_DIM}, n]")
        g = torch.empty(n, dtype=torch.float64, device=self.device) if out is None else out
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_subset_limit_state", C.byref(spec), C.c_void_p(summary.data_ptr()),
                   None if status is None else self._vector(status, n, torch.int32, "status"), ld, n,
                   self._vector(g, n, torch.float64, "out"), C.c_void_p(st.cuda_stream))
        return g

    def subset_seeds(self, g, n_seeds, gathers=(), threshold=None):
        """erpl_mc_subset_seeds: the n_seeds samples of g [n] that went furthest, ties to the lower id.  gathers: up to 4
        (src, dst) pairs of device matrices [rows, n] / [rows, >= n_seeds] (or vectors) of one dtype; the selected columns of
        src go, ascending in id, to columns 0 .. n_seeds - 1 of dst.  Returns (idx int32 [n_seeds], selected uint8 [n],
        threshold float64 [], n_alive int64 []) on the device, asynchronously: a caller compares n_alive with n_seeds (a level
        with fewer samples of g > -inf has died out).  n_seeds = 0: only the indicator of the given device `threshold` and,
        in n_alive, its count."""
        n, n_seeds = int(g.shape[0]), int(n_seeds)
        gp = self._vector(g, n, torch.float64, "g")
        idx = torch.empty(max(n_seeds, 1), dtype=torch.int32, device=self.device)
        sel = torch.empty(n, dtype=torch.uint8, device=self.device)
        thr = torch.zeros((), dtype=torch.float64, device=self.device) if threshold is None else threshold
        if not (torch.is_tensor(thr) and thr.device == self.device and thr.dtype == torch.float64 and thr.numel() == 1):
            raise ValueError("threshold must be a float64 device tensor of one element")
        alive = torch.zeros((), dtype=torch.int64, device=self.device)
        slots = (_abi.ErplSubsetGather * max(len(gathers), 1))()
        for q, (src, dst) in enumerate(gathers):
            rows, ld_src, size = self._matrix(src, "a gather's src")
            rows_d, ld_dst, size_d = self._matrix(dst, "a gather's dst")
            if rows != rows_d or src.dtype != dst.dtype or src.shape[-1] != n or dst.shape[-1] < n_seeds:
                raise ValueError("a gather's src [rows, n] and dst [rows, >= n_seeds]: the same rows and dtype")
            slots[q].src, slots[q].dst, slots[q].ld_src, slots[q].ld_dst = src.data_ptr(), dst.data_ptr(), ld_src, ld_dst
            slots[q].rows, slots[q].elem_size = rows, size
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_subset_seeds", gp, n, n_seeds, C.c_void_p(idx.data_ptr()), C.c_void_p(sel.data_ptr()),
                   C.c_void_p(thr.data_ptr()), C.c_void_p(alive.data_ptr()), slots, len(gathers), C.c_void_p(st.cuda_stream))
        return idx[:n_seeds], sel, thr, alive

    def subset_propose(self, spec, kinds, rho, cur, first_chain=0, out=None, s=None, w=None):
        """erpl_mc_subset_propose: the candidates of the chains first_chain .. first_chain + count - 1 whose current states are
        the columns of the device matrix cur [R, count] (unit column stride; a block of a step-major population is fine),
        for (spec.seed, spec.level, spec.step).  kinds: one _abi.DESIGN_NORMAL / DESIGN_UNIFORM per row; rho, s, w: scalars
        or one per row (host values); s defaults to sqrt(1 - rho^2), w to s.  Returns out (new, or the given [R, >= count]
        matrix).  Asynchronous on the current stream."""
        from .analysis import _subset_rows
        kinds, R, rho, s, w = _subset_rows(kinds, rho, s, w)
        rows, ld, _ = self._matrix(cur, "cur")
        count = int(cur.shape[-1])
        if out is None:
            out = torch.empty((R, count), dtype=torch.float64, device=self.device)
        rows_o, ld_o, _ = self._matrix(out, "out")
        if rows != R or rows_o != R or cur.dtype != torch.float64 or out.dtype != torch.float64 or out.shape[-1] < count:
            raise ValueError(f"cur and out must be float64 matrices of {R} rows, out with at least {count} columns")
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_subset_propose", C.byref(spec), kinds, C.c_void_p(rho.ctypes.data), C.c_void_p(s.ctypes.data),
                   C.c_void_p(w.ctypes.data), R, C.c_void_p(cur.data_ptr()), ld, int(first_chain), count, C.c_void_p(out.data_ptr()),
                   ld_o, C.c_void_p(st.cuda_stream))
        return out

    def subset_commit(self, threshold, g_cand, g_cur, g_next, triples=(), n_accepted=None):
        """erpl_mc_subset_commit, in place: g_next [count] and the `next` of every (cand, cur, next) triple of device matrices
        ([rows, count], or vectors; one dtype per triple) take the candidate's column where g_cand >= threshold (a float64
        device tensor of one element) and the current one otherwise.  The number accepted is added to n_accepted (an int64
        device tensor of one element; None: a new zero), which is returned.  Asynchronous on the current stream."""
        count = int(g_cand.shape[0])
        if n_accepted is None:
            n_accepted = torch.zeros((), dtype=torch.int64, device=self.device)
        if not (torch.is_tensor(threshold) and threshold.device == self.device and threshold.dtype == torch.float64
                and threshold.numel() == 1 and n_accepted.device == self.device and n_accepted.dtype == torch.int64
                and n_accepted.numel() == 1):
            raise ValueError("threshold: a float64 and n_accepted: an int64 device tensor of one element")
        slots = (_abi.ErplSubsetTriple * max(len(triples), 1))()
        for q, (cand, cur, nxt) in enumerate(triples):
            rows, ld_cand, size = self._matrix(cand, "a triple's cand")
            rows_c, ld, _ = self._matrix(cur, "a triple's cur")
            rows_n, ld_n, _ = self._matrix(nxt, "a triple's next")
            if not (rows == rows_c == rows_n and cand.dtype == cur.dtype == nxt.dtype and (rows == 1 or ld == ld_n)
                    and cand.shape[-1] >= count and cur.shape[-1] >= count and nxt.shape[-1] >= count):
                raise ValueError("a triple's cand, cur and next: the same rows and dtype, at least count columns, cur and next "
                                 "the same leading dimension")
            slots[q].cand, slots[q].cur, slots[q].next = cand.data_ptr(), cur.data_ptr(), nxt.data_ptr()
            slots[q].ld_cand, slots[q].ld, slots[q].rows, slots[q].elem_size = ld_cand, ld, rows, size
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_subset_commit", C.c_void_p(threshold.data_ptr()), self._vector(g_cand, count, torch.float64, "g_cand"),
                   self._vector(g_cur, count, torch.float64, "g_cur"), self._vector(g_next, count, torch.float64, "g_next"),
                   slots, len(triples), count, C.c_void_p(n_accepted.data_ptr()), C.c_void_p(st.cuda_stream))
        return n_accepted

    def subset_chain_stats(self, selected, chains, steps):
        """erpl_mc_subset_chain_stats of the step-major indicator bytes [steps * chains]: (n1 int64 [], pair int64 [steps - 1])
        on the device, asynchronously; analysis.subset_delta makes p, delta and gamma of them."""
        chains, steps = int(chains), int(steps)
        sp = self._vector(selected, chains * steps, torch.uint8, "selected")
        n1 = torch.zeros((), dtype=torch.int64, device=self.device)
        pair = torch.zeros(max(steps - 1, 1), dtype=torch.int64, device=self.device)
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_subset_chain_stats", sp, chains, steps, C.c_void_p(n1.data_ptr()), C.c_void_p(pair.data_ptr()),
                   C.c_void_p(st.cuda_stream))
        return n1, pair[:steps - 1]

    # ---- the tally (erpl_mc_tally_*): a run of any length folded into a fixed-size int64 state on the device
    def tally_new(self, spec=None):
        """(spec, state): an empty tally of `spec` (analysis.tally_spec; None: the library's defaults) - the state is a
        zeroed int64 device tensor of erpl_mc_tally_words(spec) words.  A bad spec is refused with the library's message."""
        from . import analysis
        spec = analysis.tally_spec() if spec is None else spec
        return spec, torch.zeros((analysis.tally_words(spec),), dtype=torch.int64, device=self.device)

    def _check_tally_state(self, spec, state, what="state"):
        from . import analysis
        if not (torch.is_tensor(state) and state.device == self.device and state.dtype == torch.int64 and state.dim() == 1
                and state.is_contiguous() and state.numel() == analysis.tally_words(spec)):
            raise ValueError(f"{what} must be a contiguous int64 tensor of tally_words(spec) words on {self.device}")

    def tally_add(self, spec, state, summary, status=None, first_id=0, n=None):
        """Folds the first n columns (default: all) of a window summary (float64 [16, ld] on the device, unit column stride)
        and its status words into `state` (erpl_mc_tally_add); column i has the id first_id + i.  Asynchronous on the
        current torch stream: a batch from `submit` is ordered in with `wait(ticket)` first."""
        self._check_tally_state(spec, state)
        if not (summary.is_cuda and summary.device == self.device and summary.dtype == torch.float64 and summary.dim() == 2
                and summary.shape[0] == _abi.SUMMARY_DIM and summary.stride(1) == 1 and summary.stride(0) >= summary.shape[1]):
            raise ValueError(f"summary must be a float64 [{_abi.SUMMARY_DIM}, ld] tensor on {self.device} with unit column stride")
        n = int(summary.shape[1]) if n is None else int(n)
        if n > summary.shape[1]:
            raise ValueError(f"n = {n} exceeds the {summary.shape[1]} columns of summary")
        if status is not None and not (status.device == self.device and status.dtype == torch.int32 and status.dim() == 1
                                       and status.shape[0] >= n and status.is_contiguous()):
            raise ValueError(f"status must be a contiguous int32 [>= n] tensor on {self.device}")
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_tally_add", C.byref(spec), C.c_void_p(state.data_ptr()), C.c_void_p(summary.data_ptr()),
                   int(summary.stride(0)), C.c_void_p(status.data_ptr()) if status is not None else None, n, int(first_id),
                   C.c_void_p(st.cuda_stream))
        return state

    def tally_merge(self, spec, dst, src):
        """dst += src, two states of `spec` (erpl_mc_tally_merge): the bytes of dst are those of one tally of both sets of
        samples, in whatever order tallies are merged.  Asynchronous on the current torch stream."""
        self._check_tally_state(spec, dst, "dst")
        self._check_tally_state(spec, src, "src")
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_tally_merge", C.byref(spec), C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()),
                   C.c_void_p(st.cuda_stream))
        return dst

    def tally_result(self, spec, state):
        """What a tally holds (erpl_mc_tally_result; blocks on the current torch stream): the dict analysis.tally_statistics
        takes - 'spec', 'result' (_abi.ErplTally), 'hist_counts' (int64 [8, 1024]), 'grid_counts' (int64 [bins_x, bins_y]).
        Raises _abi.IncompleteBatch for tallied status words with ST_INCOMPLETE."""
        from . import analysis
        self._check_tally_state(spec, state)
        res = _abi.ErplTally()
        hist = np.zeros((_abi.TALLY_MAX_ROWS, _abi.TALLY_MAX_BINS), dtype=np.int64)
        grid = np.zeros(spec.bins_x * spec.bins_y, dtype=np.int64)
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_tally_result", C.byref(spec), C.c_void_p(state.data_ptr()), C.byref(res), C.c_void_p(hist.ctypes.data),
                   C.c_void_p(grid.ctypes.data), C.c_void_p(st.cuda_stream))
        return analysis._tally_result_dict(spec, res, hist, grid)

    def bootstrap(self, summary, mask=None, rows=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), replicates=2000, level=0.95,
                  seed=0, extra=None, want_replicates=False):
        """How sure the statistics of a run are (erpl_mc_bootstrap): the non-parametric bootstrap of mean, std and
        `quantiles` of up to 4 rows (summary rows, or _abi.BOOT_ROW_EXTRA for the float64 [n] device tensor `extra`;
        default apogee, range, flight time) over ONE population: mask byte 0 and every requested row finite.  `replicates`
        resamples of `count` draws each, drawn by Philox4x32-10 from `seed` (analysis.bootstrap_indices names the samples
        a replicate drew).  Returns a dict: n, count, n_masked, n_non_finite, rows, q, level, replicates, seed and
        'stats': per row {'mean': s, 'std': s, 'quantiles': [s, ..]} with s = {estimate, rep_mean, se, lo, hi, finite} -
        `estimate` over the population itself (the bits of `analyze` where the populations coincide), se the standard
        deviation and (lo, hi) the `level` percentile interval of the statistic over its finite replicates.
        want_replicates=True adds 'replicate_values': the float64 [n_stats, replicates] device tensor, statistic
        j * (2 + len(quantiles)) + k of row j (k = 0 mean, 1 std, 2 + i quantile i)."""
        n, mask_p = self._summary_and_mask(summary, mask)
        quantiles = self._fractions(quantiles, _abi.ANALYSIS_MAX_Q, "quantiles")
        if extra is not None and not (extra.is_cuda and extra.device == self.device and extra.dtype == torch.float64
                                      and tuple(extra.shape) == (n,) and extra.is_contiguous()):
            raise ValueError(f"extra must be a contiguous float64 [n] tensor on {self.device}")
        spec = self._defaults(_abi.ErplBootSpec, "erpl_mc_bootstrap_defaults")
        self._set_rows(spec, rows, 1, _abi.BOOT_MAX_ROWS)
        spec.n_q = len(quantiles)
        spec.q[:len(quantiles)] = quantiles
        spec.replicates, spec.level, spec.seed = int(replicates), float(level), int(seed) & 0xFFFFFFFFFFFFFFFF
        R, ns = spec.n_rows, 2 + len(quantiles)
        if not 1 <= spec.replicates <= _abi.BOOT_MAX_REPLICATES:
            raise ValueError(f"1 to {_abi.BOOT_MAX_REPLICATES} replicates")
        rep = torch.empty((R * ns, spec.replicates), dtype=torch.float64, device=self.device) if want_replicates else None
        res = _abi.ErplBootstrap()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_bootstrap", C.c_void_p(summary.data_ptr()),
                   C.c_void_p(extra.data_ptr()) if extra is not None else None, mask_p, n, C.byref(spec), C.byref(res),
                   C.c_void_p(rep.data_ptr()) if want_replicates else None, C.c_void_p(st.cuda_stream))

        def stat(s):
            o = res.stat[s]
            return {"estimate": o.estimate, "rep_mean": o.rep_mean, "se": o.se, "lo": o.lo, "hi": o.hi,
                    "finite": int(o.finite)}

        out = {"n": int(res.n), "count": int(res.count), "n_masked": int(res.n_masked),
               "n_non_finite": int(res.n_non_finite), "rows": list(spec.rows[:R]), "q": quantiles,
               "level": float(level), "replicates": int(res.replicates), "seed": int(spec.seed),
               "stats": [{"mean": stat(j * ns), "std": stat(j * ns + 1),
                          "quantiles": [stat(j * ns + 2 + i) for i in range(len(quantiles))]} for j in range(R)]}
        if want_replicates:
            out["replicate_values"] = rep
        return out

    def sobol(self, summary, n_base, n_factors, mask=None, rows=None, extra=None, replicates=1000, level=0.95, seed=0,
              want_replicates=False):
        """Variance-based sensitivity of a pick-freeze run (erpl_mc_sobol): first-order (Saltelli 2010) and total-effect
        (Jansen) indices of k = `n_factors` factors on up to 4 rows (summary rows, or _abi.SOBOL_ROW_EXTRA for `extra`;
        default first apogee altitude and time, rail-exit speed).  `summary` is the float64 [16, ld] device tensor of the
        concatenated design, ld >= (k + 2) n_base: columns [0, n_base) block A, [n_base, 2 n_base) block B, then AB_0 ..
        AB_k-1 (A with factor i taken from B); `extra` float64 [ld] likewise; `mask` uint8 [n_base], byte 0 = the design
        row counts.  One population per row: mask byte 0 and all k + 2 values of the row finite.  `replicates` bootstrap
        resamples of whole design rows (0: estimates only), drawn as erpl_mc_bootstrap draws them from `seed`.
        Returns a dict of NumPy arrays: rows, count / n_masked / n_non_finite / constant ([R]), and mean, variance ([R]),
        first, total ([R, k]) each as a dict {estimate, rep_mean, se, lo, hi, finite}; n_base, n_factors, replicates,
        level, seed.  want_replicates=True adds 'replicate_values': the float64 [R (2 + 2 k), replicates] device tensor,
        statistic j (2 + 2 k) + {0: mean, 1: variance, 2 + i: first i, 2 + k + i: total i} of row j."""
        ld = self._check_summary(summary)
        n_base, k = int(n_base), int(n_factors)
        if not 1 <= k <= _abi.SOBOL_MAX_FACTORS:
            raise ValueError(f"1 to {_abi.SOBOL_MAX_FACTORS} factors")
        if n_base < 1 or (k + 2) * n_base > ld:
            raise ValueError(f"summary holds {ld} flights: fewer than (n_factors + 2) * n_base = {(k + 2) * n_base}")
        if mask is not None and not (mask.device == self.device and mask.dtype == torch.uint8
                                     and tuple(mask.shape) == (n_base,) and mask.is_contiguous()):
            raise ValueError(f"mask must be a contiguous uint8 [n_base] tensor on {self.device}")
        if extra is not None and not (extra.is_cuda and extra.device == self.device and extra.dtype == torch.float64
                                      and tuple(extra.shape) == (ld,) and extra.is_contiguous()):
            raise ValueError(f"extra must be a contiguous float64 [ld] tensor on {self.device}")
        spec = self._defaults(_abi.ErplSobolSpec, "erpl_mc_sobol_defaults")
        self._set_rows(spec, rows, 1, _abi.SOBOL_MAX_ROWS)
        spec.n_factors, spec.replicates, spec.level = k, int(replicates), float(level)
        spec.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if not 0 <= spec.replicates <= _abi.SOBOL_MAX_REPLICATES:
            raise ValueError(f"0 to {_abi.SOBOL_MAX_REPLICATES} replicates")
        if want_replicates and spec.replicates == 0:
            raise ValueError("want_replicates needs replicates > 0")
        R, ns = spec.n_rows, 2 + 2 * k
        rep = torch.empty((R * ns, spec.replicates), dtype=torch.float64, device=self.device) if want_replicates else None
        res = _abi.ErplSobol()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_sobol", C.c_void_p(summary.data_ptr()), C.c_void_p(extra.data_ptr()) if extra is not None else None,
                   C.c_void_p(mask.data_ptr()) if mask is not None else None, n_base, ld, C.byref(spec), C.byref(res),
                   C.c_void_p(rep.data_ptr()) if want_replicates else None, C.c_void_p(st.cuda_stream))

        def stats(pick):
            """One field group of every row as {key: array}: pick(row) is an erpl_boot_stat or an array of k of them."""
            keys = ("estimate", "rep_mean", "se", "lo", "hi", "finite")
            out = {}
            for key in keys:
                vals = []
                for j in range(R):
                    s = pick(res.row[j])
                    vals.append(getattr(s, key) if isinstance(s, _abi.ErplBootStat) else [getattr(s[i], key) for i in range(k)])
                out[key] = np.array(vals, dtype=np.int64 if key == "finite" else np.float64)
            return out

        out = {"n_base": int(res.n_base), "n_factors": k, "rows": list(spec.rows[:R]), "replicates": int(res.replicates),
               "level": float(level), "seed": int(spec.seed)}
        for key in ("count", "n_masked", "n_non_finite", "constant"):
            out[key] = np.array([getattr(res.row[j], key) for j in range(R)], dtype=np.int64)
        out["mean"], out["variance"] = stats(lambda r: r.mean), stats(lambda r: r.variance)
        out["first"], out["total"] = stats(lambda r: r.first), stats(lambda r: r.total)
        if want_replicates:
            out["replicate_values"] = rep
        return out

    def dependence(self, factors, summary, mask=None, rows=None, extra=None, classes=16, cells=16, shifts=200, level=0.95,
                   seed=0, want_tables=False, want_curves=True, want_null=False):
        """Given-data sensitivity of ONE ordinary run (erpl_mc_dependence), no extra flights: for every row of `factors`
        (float64 [F, n] on the device, F <= 32) and up to 4 rows (summary rows, or _abi.DEP_ROW_EXTRA for the float64 [n]
        device tensor `extra`; default apogee, range, flight time) the first-order variance share eta2 (correlation ratio),
        Borgonovo's delta, the PAWN Kolmogorov-Smirnov statistics and the mutual information, over ONE population: mask
        byte 0 and every factor and requested row finite.  Factors are cut into `classes` and outcomes into `cells` equal-
        count classes of their mid-ranks (2..64).  `shifts` cyclic re-pairings (0..4096, drawn from `seed` as
        erpl_mc_bootstrap draws) give every measure the value a factor without any effect would get at this size.
        Returns a dict: n, count, n_masked, n_non_finite, rows, n_factors, classes, cells, shifts, level, seed, row_mean /
        row_ss ([R]), classes_used / cells_used / delta_num / eta2 / eta2_adj / f_stat ([R, F]) and delta, ks_max,
        ks_median, mi, each {estimate, null_mean, null_hi, exceed} of [R, F] arrays (null_hi: the quantile `level` of the
        null values).  want_curves adds 'class_stats' ([R, F, classes, 6]: count, mean, std, x_lo, x_hi, x_median of
        every class, the main-effect curve), want_tables 'tables' (int64 [R, F, classes, cells]), want_null 'null_values'
        ([R, F, 4, shifts]: delta, ks_max, ks_median, mi).  A pick-freeze design is not an ordinary run: use `sobol`."""
        n, mask_p = self._summary_and_mask(summary, mask)
        if not (factors.is_cuda and factors.device == self.device and factors.dtype == torch.float64
                and factors.dim() == 2 and factors.shape[1] == n and factors.is_contiguous()):
            raise ValueError(f"factors must be a contiguous float64 [F, n] tensor on {self.device}")
        F = int(factors.shape[0])
        if not 1 <= F <= _abi.DEP_MAX_FACTORS:
            raise ValueError(f"1 to {_abi.DEP_MAX_FACTORS} factors")
        if extra is not None and not (extra.is_cuda and extra.device == self.device and extra.dtype == torch.float64
                                      and tuple(extra.shape) == (n,) and extra.is_contiguous()):
            raise ValueError(f"extra must be a contiguous float64 [n] tensor on {self.device}")
        spec = self._defaults(_abi.ErplDepSpec, "erpl_mc_dependence_defaults")
        self._set_rows(spec, rows, 1, _abi.DEP_MAX_ROWS)
        spec.n_factors, spec.classes, spec.cells, spec.shifts = F, int(classes), int(cells), int(shifts)
        spec.level, spec.seed = float(level), int(seed) & 0xFFFFFFFFFFFFFFFF
        if not (2 <= spec.classes <= _abi.DEP_MAX_CLASSES and 2 <= spec.cells <= _abi.DEP_MAX_CELLS):
            raise ValueError(f"2 to {_abi.DEP_MAX_CLASSES} classes and 2 to {_abi.DEP_MAX_CELLS} cells")
        if not 0 <= spec.shifts <= _abi.DEP_MAX_SHIFTS:
            raise ValueError(f"0 to {_abi.DEP_MAX_SHIFTS} shifts")
        if want_null and spec.shifts == 0:
            raise ValueError("want_null needs shifts > 0")
        R, M, H, P = spec.n_rows, spec.classes, spec.cells, spec.shifts
        tables = np.empty((R, F, M, H), dtype=np.int64) if want_tables else None
        curves = np.empty((R, F, M, 6), dtype=np.float64) if want_curves else None
        null = np.empty((R, F, 4, P), dtype=np.float64) if want_null else None
        res = _abi.ErplDependence()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_dependence", C.c_void_p(factors.data_ptr()), C.c_void_p(summary.data_ptr()),
                   C.c_void_p(extra.data_ptr()) if extra is not None else None, mask_p, n, C.byref(spec), C.byref(res),
                   C.c_void_p(tables.ctypes.data) if want_tables else None,
                   C.c_void_p(curves.ctypes.data) if want_curves else None,
                   C.c_void_p(null.ctypes.data) if want_null else None, C.c_void_p(st.cuda_stream))

        def grid(pick, dtype=np.float64):
            return np.array([[pick(res.pair[j][f]) for f in range(F)] for j in range(R)], dtype=dtype)

        out = {"n": int(res.n), "count": int(res.count), "n_masked": int(res.n_masked), "n_non_finite": int(res.n_non_finite),
               "rows": list(spec.rows[:R]), "n_factors": F, "classes": M, "cells": H, "shifts": P, "level": float(level),
               "seed": int(spec.seed), "row_mean": np.array(res.row_mean[:R], dtype=np.float64),
               "row_ss": np.array(res.row_ss[:R], dtype=np.float64),
               "classes_used": grid(lambda p: p.classes_used, np.int64), "cells_used": grid(lambda p: p.cells_used, np.int64),
               "delta_num": grid(lambda p: p.delta_num, np.int64)}
        for key in ("eta2", "eta2_adj", "f_stat"):
            out[key] = grid(lambda p, key=key: getattr(p, key))
        for key in ("delta", "ks_max", "ks_median", "mi"):
            out[key] = {"estimate": grid(lambda p, key=key: getattr(p, key).estimate),
                        "null_mean": grid(lambda p, key=key: getattr(p, key).null_mean),
                        "null_hi": grid(lambda p, key=key: getattr(p, key).null_hi),
                        "exceed": grid(lambda p, key=key: getattr(p, key).exceed, np.int64)}
        if want_tables:
            out["tables"] = tables
        if want_curves:
            out["class_stats"] = curves
        if want_null:
            out["null_values"] = null
        return out

    def surrogate(self, factors, kinds, summary, mask=None, rows=None, extra=None, degree=2, order=2, holdout=0, want_gram=False):
        """A polynomial chaos surrogate of ONE run of independent primitives (erpl_mc_surrogate), no extra flights: the
        least-squares fit of orthonormal Hermite / Legendre polynomials of the rows of `factors` (float64 [V, n] on the
        device, V <= 32; `kinds`: _abi.DESIGN_UNIFORM for a U(0, 1) row, _abi.DESIGN_NORMAL for an N(0, 1) row, as
        `design` draws them) to up to 4 rows (summary rows, or _abi.SUR_ROW_EXTRA for the float64 [n] device tensor
        `extra`; default apogee, range, flight time), over ONE population: mask byte 0 and every variable and requested row
        finite.  Terms: total degree <= `degree` (1..12), at most `order` (1..4) variables each, at most 1024 of them.
        holdout = k >= 2 keeps every k-th member out of the fit and validates on it (q2); 0 fits every member.
        Returns a dict: n, count, n_masked, n_non_finite, n_fit, n_val, rows, n_vars, degree, order, holdout, n_terms,
        pivot_min / pivot_max, fit_ok, mean, variance_pce, tss_fit, rss_fit, r2, tss_val, rss_val, q2 ([R]), first / total
        ([R, V]), pair ([R, V, V]: the second-order index of {i, j}), and 'model' = {kinds, degree, order, terms ([P, 4, 2]
        int8), coefficients ([R, P]), rows} for `surrogate_predict`.  want_gram adds 'gram' ([P, P]) and 'rhs' ([R, P]).
        The indices are shares of the EXPLAINED variance; r2 is the share the variables explain at all.  Where the fit
        fails (fewer fitted members than terms, a pivot that is not positive) fit_ok is False and what depends on the
        coefficients is NaN."""
        n, mask_p = self._summary_and_mask(summary, mask)
        if not (torch.is_tensor(factors) and factors.is_cuda and factors.device == self.device and factors.dtype == torch.float64
                and factors.dim() == 2 and factors.shape[1] == n and factors.is_contiguous()):
            raise ValueError(f"factors must be a contiguous float64 [V, n] tensor on {self.device}")
        V = int(factors.shape[0])
        if not 1 <= V <= _abi.SUR_MAX_VARS:
            raise ValueError(f"1 to {_abi.SUR_MAX_VARS} variables")
        kinds = bytes(bytearray(int(k) for k in kinds))
        if len(kinds) != V:
            raise ValueError(f"kinds must have one entry per row of factors ({V})")
        if extra is not None and not (extra.is_cuda and extra.device == self.device and extra.dtype == torch.float64
                                      and tuple(extra.shape) == (n,) and extra.is_contiguous()):
            raise ValueError(f"extra must be a contiguous float64 [n] tensor on {self.device}")
        spec = self._defaults(_abi.ErplSurSpec, "erpl_mc_surrogate_defaults")
        self._set_rows(spec, rows, 1, _abi.SUR_MAX_ROWS)
        spec.n_vars, spec.degree, spec.order, spec.holdout = V, int(degree), int(order), int(holdout)
        P = C.c_int32(0)
        _abi.check(self.lib, self.lib.erpl_mc_surrogate_terms(V, spec.degree, spec.order, C.byref(P), None), "erpl_mc_surrogate_terms")
        P, R = int(P.value), spec.n_rows
        coef = np.empty((R, P), dtype=np.float64)
        terms = np.empty((P, 4, 2), dtype=np.int8)
        pair = np.empty((R, V, V), dtype=np.float64)
        gram = np.empty((P, P), dtype=np.float64) if want_gram else None
        rhs = np.empty((R, P), dtype=np.float64) if want_gram else None
        res = _abi.ErplSurrogate()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_surrogate", C.c_void_p(factors.data_ptr()), kinds, C.c_void_p(summary.data_ptr()),
                   C.c_void_p(extra.data_ptr()) if extra is not None else None, mask_p, n, C.byref(spec), C.byref(res),
                   C.c_void_p(coef.ctypes.data), C.c_void_p(terms.ctypes.data),
                   C.c_void_p(gram.ctypes.data) if want_gram else None, C.c_void_p(rhs.ctypes.data) if want_gram else None,
                   C.c_void_p(pair.ctypes.data), C.c_void_p(st.cuda_stream))
        out = {k: int(getattr(res, k)) for k in ("n", "count", "n_masked", "n_non_finite", "n_fit", "n_val", "n_vars", "degree",
                                                 "order", "holdout", "n_terms")}
        out["rows"] = list(spec.rows[:R])
        out["pivot_min"], out["pivot_max"] = res.pivot_min, res.pivot_max
        out["fit_ok"] = np.array([bool(res.row[j].fit_ok) for j in range(R)])
        for key in ("mean", "variance_pce", "tss_fit", "rss_fit", "r2", "tss_val", "rss_val", "q2"):
            out[key] = np.array([getattr(res.row[j], key) for j in range(R)], dtype=np.float64)
        out["first"] = np.array([list(res.row[j].first[:V]) for j in range(R)], dtype=np.float64)
        out["total"] = np.array([list(res.row[j].total[:V]) for j in range(R)], dtype=np.float64)
        out["pair"] = pair
        out["model"] = {"kinds": kinds, "degree": spec.degree, "order": spec.order, "terms": terms, "coefficients": coef,
                        "rows": out["rows"]}
        if want_gram:
            out["gram"], out["rhs"] = gram, rhs
        return out

    def reweight(self, factors, kinds, law, summary, mask=None, rows=None, extra=None, thresholds=None,
                 quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), want_weights=False):
        """The statistics of a flown run under ANOTHER input law, by importance weights (erpl_mc_reweight), no new run.
        `factors` (float64 [n_law, n] on the device, unit column stride, n_law <= 32) holds the primitive rows whose law
        changes, as `design` / `qmc` drew them; `kinds`: _abi.DESIGN_NORMAL for a row flown under N(0, 1), _abi.DESIGN_UNIFORM
        for U(0, 1); `law`: per row the target, (mu, s) in flown sigmas or (a, b) within (0, 1) (analysis.reweight_spec,
        which also takes rows, thresholds and quantiles).  One population: mask byte 0, every law row and requested row
        finite, inside the support of every uniform target.  Weights are integers W = floor(2^Q exp(l - l_max)), so sum_w,
        max_w, the exceedances and the weighted order statistics are exact and the same bits in every call; the doubles are
        folded in a fixed order.  Returns the dict of analysis.reweight_result_dict; want_weights adds 'logw' (float64 [n]:
        NaN where masked or non-finite, -inf outside the support) and 'weights' (int64 [n]) device tensors, bit-equal to
        analysis.reweight_host.  An empty population is no error: the integers are 0 and the doubles NaN."""
        from . import analysis
        rows_s, ld_s, _ = self._matrix(summary, "summary")
        n = int(summary.shape[-1])
        if rows_s != _abi.SUMMARY_DIM or summary.dtype != torch.float64 or summary.dim() != 2:
            raise ValueError(f"summary must be float64 [{_abi.SUMMARY_DIM}, n]")
        n_law, ld, _ = self._matrix(factors, "factors")
        if factors.dtype != torch.float64 or int(factors.shape[-1]) != n:
            raise ValueError("factors must be float64 [n_law, n]")
        spec = analysis.reweight_spec(kinds, law, rows, thresholds, quantiles)
        if n_law != spec.n_law:
            raise ValueError(f"kinds and law must have one entry per row of factors ({n_law})")
        mask_p = None if mask is None else self._vector(mask, n, torch.uint8, "mask")
        extra_p = None if extra is None else self._vector(extra, n, torch.float64, "extra")
        logw = torch.empty(n, dtype=torch.float64, device=self.device) if want_weights else None
        weights = torch.empty(n, dtype=torch.int64, device=self.device) if want_weights else None
        res = _abi.ErplReweight()
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_reweight", C.byref(spec), C.c_void_p(factors.data_ptr()), ld, C.c_void_p(summary.data_ptr()), ld_s,
                   extra_p, mask_p, n, C.byref(res), C.c_void_p(logw.data_ptr()) if want_weights else None,
                   C.c_void_p(weights.data_ptr()) if want_weights else None, C.c_void_p(st.cuda_stream))
        out = analysis.reweight_result_dict(spec, res)
        if want_weights:
            out["logw"], out["weights"] = logw, weights
        return out

    def surrogate_predict(self, model, X, out=None, n=None):
        """The fitted outcomes of `model` (the 'model' of `surrogate`) at the columns 0 .. n - 1 (default: all) of X, a
        float64 [V, ld] device tensor with unit column stride, without a flight (erpl_mc_surrogate_predict): a float64
        [R, ld] device tensor (`out`, or a new one; with n < ld the columns from n on are left as they are), one row per
        row of the model.  A point with a non-finite input gives NaN.  Asynchronous on the current stream."""
        kinds = bytes(model["kinds"])
        coef = np.ascontiguousarray(model["coefficients"], dtype=np.float64)
        V, R = len(kinds), int(coef.shape[0])
        if not (torch.is_tensor(X) and X.is_cuda and X.device == self.device and X.dtype == torch.float64 and X.dim() == 2
                and X.shape[0] == V and X.is_contiguous()):
            raise ValueError(f"X must be a contiguous float64 [{V}, ld] tensor on {self.device}")
        ld = int(X.shape[1])
        n = ld if n is None else int(n)
        if out is None:
            out = torch.empty((R, ld), dtype=torch.float64, device=self.device)
        if not (torch.is_tensor(out) and out.is_cuda and out.device == self.device and out.dtype == torch.float64
                and tuple(out.shape) == (R, ld) and out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float64 [{R}, {ld}] tensor on {self.device}")
        spec = self._defaults(_abi.ErplSurSpec, "erpl_mc_surrogate_defaults")
        spec.n_vars, spec.n_rows, spec.degree, spec.order = V, R, int(model["degree"]), int(model["order"])
        st = torch.cuda.current_stream(self.device)
        self._call("erpl_mc_surrogate_predict", C.byref(spec), kinds, C.c_void_p(coef.ctypes.data), C.c_void_p(X.data_ptr()), ld, n,
                   C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream))
        return out

    def compare(self, summary_a, summary_b, mask_a=None, mask_b=None, rows=None, extra_a=None, extra_b=None,
                quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), xy=(_abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y), permutations=999, level=0.95,
                seed=0, keep_null=False, knots=512):
        """Did two runs come from the same law (erpl_mc_compare)?  Two [16, n] summaries with their own n and masks; up to 4
        rows (summary rows, or _abi.CMP_ROW_EXTRA for the float64 device tensors extra_a / extra_b; default apogee, range,
        flight time), per row the Kolmogorov-Smirnov, Mann-Whitney and Cramer-von Mises statistics and the shift function at
        `quantiles`; xy = (row_x, row_y) adds the energy statistic of the two impact clouds (None: off; at most
        _abi.CMP_ENERGY_MAX_POINTS pooled points).  Every statistic is recomputed under `permutations` relabellings of the
        pooled members (0..4096, labels: analysis.permutation_labels).  ONE population per run: mask byte 0 and every
        requested row (and x, y) finite.
        Returns a dict: n_a, n_b, count_a, count_b, n_masked_*, n_non_finite_*, rows, q, xy, permutations, level, seed,
        'row': per row {mean_a, std_a, mean_b, std_b, quantile_a, quantile_b, shift, ks_num, u2_a, ks_at, ks_sign,
        prob_superiority, ks, mw, cvm} with each test {statistic, p_value, null_mean, null_hi, exceed}, 'energy' (a test, or
        None) with d_ab / d_aa / d_bb, and what a plot needs WITHOUT the samples: 'ecdf' = {levels [K], a [R, K], b [R, K]}, the
        order statistics floor(level (m - 1)) of each side's population on a fixed grid of K = min(knots, 512, count) levels,
        and 'cloud_a' / 'cloud_b' = {mean, cov} of the impact points (torch on the device; knots=0 leaves both out).  keep_null=True adds 'null_values', the float64
        [3 R + 1, permutations] device tensor (rows 3 j, 3 j + 1, 3 j + 2: K, 2 U_A, T of row j; the last: E)."""
        n_a, mask_a_p = self._summary_and_mask(summary_a, mask_a)
        n_b, mask_b_p = self._summary_and_mask(summary_b, mask_b)
        quantiles = self._fractions(quantiles, _abi.ANALYSIS_MAX_Q, "quantiles")
        for extra, n, name in ((extra_a, n_a, "extra_a"), (extra_b, n_b, "extra_b")):
            if extra is not None and not (extra.is_cuda and extra.device == self.device and extra.dtype == torch.float64
                                          and tuple(extra.shape) == (n,) and extra.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float64 [n] tensor on {self.device}")
        spec = self._defaults(_abi.ErplCmpSpec, "erpl_mc_compare_defaults")
        self._set_rows(spec, rows, 1, _abi.CMP_MAX_ROWS)
        spec.n_q = len(quantiles)
        spec.q[:len(quantiles)] = quantiles
        spec.row_x, spec.row_y = (-1, -1) if xy is None else (int(xy[0]), int(xy[1]))
        spec.permutations, spec.level, spec.seed = int(permutations), float(level), int(seed) & 0xFFFFFFFFFFFFFFFF
        if not 0 <= spec.permutations <= _abi.CMP_MAX_PERMUTATIONS:
            raise ValueError(f"0 to {_abi.CMP_MAX_PERMUTATIONS} permutations")
        if keep_null and spec.permutations == 0:
            raise ValueError("keep_null needs permutations > 0")
        R, P = spec.n_rows, spec.permutations
        null = torch.empty((3 * R + 1, P), dtype=torch.float64, device=self.device) if keep_null else None
        res = _abi.ErplCompare()
        st = torch.cuda.current_stream(self.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        self._call("erpl_mc_compare", ptr(summary_a), mask_a_p, n_a, ptr(summary_b), mask_b_p, n_b, ptr(extra_a), ptr(extra_b),
                   C.byref(spec), C.byref(res), ptr(null), C.c_void_p(st.cuda_stream))

        def test(t):
            return {"statistic": t.statistic, "p_value": t.p_value, "null_mean": t.null_mean, "null_hi": t.null_hi,
                    "exceed": int(t.exceed)}

        nq = len(quantiles)
        row_ids = list(spec.rows[:R])
        out = {k: int(getattr(res, k)) for k in ("n_a", "n_b", "count_a", "count_b", "n_masked_a", "n_masked_b",
                                                 "n_non_finite_a", "n_non_finite_b")}
        out.update(rows=row_ids, q=quantiles, xy=None if xy is None else (spec.row_x, spec.row_y), permutations=P,
                   level=float(level), seed=int(spec.seed), row=[])
        for j in range(R):
            r = res.row[j]
            out["row"].append({"mean_a": r.mean_a, "std_a": r.std_a, "mean_b": r.mean_b, "std_b": r.std_b,
                               "quantile_a": list(r.quantile_a[:nq]), "quantile_b": list(r.quantile_b[:nq]),
                               "shift": list(r.shift[:nq]), "ks_num": int(r.ks_num), "u2_a": int(r.u2_a), "ks_at": r.ks_at,
                               "ks_sign": int(r.ks_sign), "prob_superiority": r.prob_superiority,
                               "ks": test(r.ks), "mw": test(r.mw), "cvm": test(r.cvm)})
        out["energy"] = dict(test(res.energy), d_ab=res.d_ab, d_aa=res.d_aa, d_bb=res.d_bb) if res.bivariate else None

        # what the plot needs, never the samples: ECDF knots on a fixed grid of levels and the moments of the two clouds
        # (knots=0: neither)
        K = max(0, min(int(knots), 512, out["count_a"], out["count_b"]))
        levels = np.linspace(0.0, 1.0, K) if K > 1 else np.zeros(K)
        ecdf = {"levels": levels, "a": np.zeros((R, 0)), "b": np.zeros((R, 0))}
        if xy is not None:
            out["cloud_a"] = out["cloud_b"] = None
        for name, summ, mask, extra in (("a", summary_a, mask_a, extra_a), ("b", summary_b, mask_b, extra_b)):
            if K == 0:
                break
            vals = [extra if r == _abi.CMP_ROW_EXTRA else summ[r] for r in row_ids]
            if xy is not None:
                vals += [summ[spec.row_x], summ[spec.row_y]]
            keep = torch.ones(summ.shape[1], dtype=torch.bool, device=self.device) if mask is None else mask == 0
            for v in vals:
                keep = keep & torch.isfinite(v)
            vals = [v[keep] for v in vals]
            m = int(vals[0].shape[0])
            at = torch.from_numpy(np.floor(levels * (m - 1)).astype(np.int64)).to(self.device)
            ecdf[name] = np.stack([torch.sort(v).values[at].cpu().numpy() for v in vals[:R]])
            if xy is not None:
                pts = torch.stack(vals[R:R + 2])
                out["cloud_" + name] = {"mean": pts.mean(dim=1).cpu().numpy(), "cov": torch.cov(pts, correction=0).cpu().numpy()}
        out["ecdf"] = ecdf
        if keep_null:
            out["null_values"] = null
        return out

    def _seeds_on_device(self, seeds):
        """The 32-bit seeds of the device streams: n."""
        if not (seeds.is_cuda and seeds.device == self.device and seeds.dtype in (torch.uint32, torch.int32)
                and seeds.dim() == 1 and seeds.is_contiguous()):
            raise ValueError(f"seeds must be a contiguous uint32 (or int32: the same 32 bits) [n] tensor on {self.device}")
        return int(seeds.shape[0])

    def legacy_streams_device(self, seeds, ops, threads=0):
        """flatten.legacy_streams(by_output=True) on the device (erpl_mc_legacy_random_streams_device): the first len(ops)
        outputs ('g' normal / 'u' uniform double) of np.random.RandomState(seed) for every seed of the uint32 [n] device
        tensor `seeds`, bit for bit, as a float64 [len(ops), n] device tensor.  Enqueued on the current torch stream; blocks
        the host until the tensor is filled (the libm log of every accepted pair runs on `threads` host threads)."""
        n = self._seeds_on_device(seeds)
        code = np.frombuffer(ops.encode(), dtype=np.uint8)
        if not np.all((code == ord("g")) | (code == ord("u"))):
            raise ValueError("ops: 'g' (normal) and 'u' (uniform double) only")
        code = np.ascontiguousarray(np.where(code == ord("g"), _abi.RS_GAUSS, _abi.RS_DOUBLE).astype(np.uint8))
        out = torch.empty((code.size, n), dtype=torch.float64, device=self.device)
        st = torch.cuda.current_stream(self.device)
        with self._legacy_lock:
            self._call("erpl_mc_legacy_random_streams_device", C.c_void_p(seeds.data_ptr()), n,
                       C.c_void_p(code.ctypes.data), int(code.size), C.c_void_p(out.data_ptr()), int(threads),
                       C.c_void_p(st.cuda_stream))
        return out

    def legacy_wind_device(self, seeds, sigma, rho, innov, base=None, mean_scale=None, speed=None, cdir=None, sdir=None,
                           threads=0):
        """erpl_mc_legacy_wind_profiles on the device (erpl_mc_legacy_wind_profiles_device): the float64 [K, 3, n] wind
        tables of the uint32 [n] device tensor `seeds`, bit for bit the host function's.  sigma / rho / innov [K] and
        base [K, 3] or mean_scale [K] are host arrays; speed / cdir / sdir (without `base`) float64 [n] device tensors.
        Enqueued on the current torch stream; blocks the host until the table is filled."""
        n = self._seeds_on_device(seeds)
        f = lambda v: np.ascontiguousarray(v, dtype=np.float64)
        sigma, rho, innov = f(sigma), f(rho), f(innov)
        K = sigma.size
        if rho.size != K or innov.size != K:
            raise ValueError("sigma, rho and innov: one entry per knot")
        if base is not None:
            base = f(base)
            if base.shape != (K, 3):
                raise ValueError("base must be [K, 3]")
        else:
            if mean_scale is None or speed is None or cdir is None or sdir is None:
                raise ValueError("without base: mean_scale, speed, cdir and sdir")
            mean_scale = f(mean_scale)
            if mean_scale.size != K:
                raise ValueError("mean_scale: one entry per knot")
            for t in (speed, cdir, sdir):
                if not (t.is_cuda and t.device == self.device and t.dtype == torch.float64 and tuple(t.shape) == (n,)
                        and t.is_contiguous()):
                    raise ValueError(f"speed, cdir and sdir must be contiguous float64 [n] tensors on {self.device}")
        hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        dp = lambda t: None if t is None or base is not None else C.c_void_p(t.data_ptr())
        wind = torch.empty((K, 3, n), dtype=torch.float64, device=self.device)
        st = torch.cuda.current_stream(self.device)
        with self._legacy_lock:
            self._call("erpl_mc_legacy_wind_profiles_device", C.c_void_p(seeds.data_ptr()), n, K, hp(sigma), hp(rho),
                       hp(innov), hp(base), hp(mean_scale), dp(speed), dp(cdir), dp(sdir), C.c_void_p(wind.data_ptr()),
                       int(threads), C.c_void_p(st.cuda_stream))
        return wind

    def set_profiling(self, enable=True):
        """Record HIP events around the two kernels on the launch stream (erpl_mc_set_profiling)."""
        self._call("erpl_mc_set_profiling", int(bool(enable)))

    def last_kernel_ms(self):
        """(rail_ms, flight_ms) device durations of the last profiled run (synchronises on its end)."""
        a, b = C.c_float(), C.c_float()
        self._call("erpl_mc_last_kernel_ms", C.byref(a), C.byref(b))
        return a.value, b.value

    def kernel_ms_history(self, max_runs=_abi.PROFILE_RING):
        """Per-launch (rail_ms[], flight_ms[]) of the most recent profiled runs, oldest first."""
        m = min(int(max_runs), _abi.PROFILE_RING)
        ra, fa, n = (C.c_float * m)(), (C.c_float * m)(), C.c_int(0)
        self._call("erpl_mc_kernel_ms_history", m, ra, fa, C.byref(n))
        return list(ra[:n.value]), list(fa[:n.value])

    def debug_counters(self):
        out = (C.c_double * 16)()
        torch.cuda.synchronize(self.device)
        self._call("erpl_mc_debug_counters", out)
        return list(out)

    def last_stats(self):
        """(physics RK4 steps integrated, wave-iterations) of the last run (synchronises)."""
        a, b = C.c_double(), C.c_double()
        torch.cuda.synchronize(self.device)
        self._call("erpl_mc_last_stats", C.byref(a), C.byref(b))
        return a.value, b.value

    def ticket_stats(self, ticket):
        """(physics RK4 steps integrated, wave-iterations) of ONE submitted batch (waits for that batch alone)."""
        a, b = C.c_double(), C.c_double()
        self._call("erpl_mc_ticket_stats", C.c_int64(ticket), C.byref(a), C.byref(b))
        return a.value, b.value
