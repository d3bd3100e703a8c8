"""Host-side mirror of the reference's MHPC controller surface.

Same names, fields, defaults and argument meaning as the reference's C++ API:
  HSDDP_OPTION          MHPC_CompoundTypes.h:196-212
  USRCMD                MHPC_CompoundTypes.h:237-240
  MHPCUserParameters    MHPC_CompoundTypes.h:242-251   (alias MHPC_UserParameter)
  GaitType2D / Gait     Common/header/Gait.h:6-77
  MHPCLocomotion        Controller/MHPCLocomotion/MHPCLocomotion.{h,cpp}
but one MHPCLocomotion object drives a BATCH of independent problems on one GPU through
the C-ABI (include/mhpc_capi.h).  Numbers come only from the HIP library; there is no CPU
fallback in this module.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from enum import Enum
from typing import List, Optional

import numpy as np

from . import capi

PI = 3.141592653589793238  # MHPC_CPPTypes.h:18


def f32(v: float) -> float:
    """A reference `float` parameter promoted to double."""
    return float(np.float32(v))


def eigen_row(v) -> str:
    """One row as `ostream << vec.transpose()` prints it with Eigen's default IOFormat: each
    coefficient formatted like `ostream << double` (6 significant digits, %g), right-aligned
    to the widest coefficient of the row, separated by one space."""
    strs = ["%g" % float(x) for x in np.ravel(v)]
    w = max((len(t) for t in strs), default=0)
    return " ".join(t.rjust(w) for t in strs)


# ----------------------------------------------------------------------------------------
@dataclass
class HSDDP_OPTION:
    alpha: float = 0.1
    gamma: float = 0.01
    update_penalty: float = 8
    update_relax: float = 0.1
    update_regularization: float = 2
    update_ReB: float = 7
    max_DDP_iter: float = 3
    max_AL_iter: float = 2
    DDP_thresh: float = 1e-03
    AL_thresh: float = 1e-03
    AL_active: bool = True
    ReB_active: bool = True
    smooth_active: bool = False

    def to_c(self) -> capi.HsddpOption:
        o = capi.HsddpOption()
        for k in ("alpha", "gamma", "update_penalty", "update_relax", "update_regularization",
                  "update_ReB", "max_DDP_iter", "max_AL_iter", "DDP_thresh", "AL_thresh"):
            setattr(o, k, float(getattr(self, k)))
        o.AL_active = int(bool(self.AL_active))
        o.ReB_active = int(bool(self.ReB_active))
        o.smooth_active = int(bool(self.smooth_active))
        return o

    @classmethod
    def from_c(cls, o: capi.HsddpOption) -> "HSDDP_OPTION":
        return cls(**{k: getattr(o, k) for k in (
            "alpha", "gamma", "update_penalty", "update_relax", "update_regularization",
            "update_ReB", "max_DDP_iter", "max_AL_iter", "DDP_thresh", "AL_thresh")},
            AL_active=bool(o.AL_active), ReB_active=bool(o.ReB_active),
            smooth_active=bool(o.smooth_active))


@dataclass
class USRCMD:
    vel: float = 0.0
    height: float = 0.0
    roll: float = 0.0
    pitch: float = 0.0
    yaw: float = 0.0


@dataclass
class MHPCUserParameters:
    n_wbphase: int = 4
    n_fbphase: int = 4
    dt_wb: float = .001
    dt_fb: float = .001
    cmode: int = 1
    groundH: float = -0.404  # unused by the reference too (ground hard-coded)
    usrcmd: Optional[USRCMD] = None


MHPC_UserParameter = MHPCUserParameters  # the north star's spelling


class GaitType2D(Enum):
    STAND = 0
    BOUND = 1
    PRONK = 2


class Gait:
    """Gait.h:13-77.  Only BOUND is defined; every other type takes the default branch
    (uniform 0.08 s timings) exactly as the reference's switch does."""

    def __init__(self, gait: Optional[GaitType2D] = None):
        self._gait_mode = [1, 2, 3, 4]
        self._gait_name = "BOUND"
        if gait is None or gait == GaitType2D.BOUND:
            self._gait_timing = [f32(0.08), f32(0.1), f32(0.08), f32(0.1)]
        else:
            self._gait_timing = [f32(0.08)] * 4

    def get_next_mode(self, current_mode: int) -> int:
        for idx, m in enumerate(self._gait_mode):
            if m == current_mode:
                return self._gait_mode[(idx + 1) % len(self._gait_mode)]
        raise ValueError(f"mode {current_mode} not in gait")

    def get_mode_seq(self, current_mode: int, num_phases: int) -> List[int]:
        assert num_phases >= 1
        seq = [current_mode]
        for _ in range(num_phases - 1):
            seq.append(self.get_next_mode(seq[-1]))
        return seq

    def get_timings(self, mode_seq: List[int]) -> List[float]:
        return [self._gait_timing[m - 1] for m in mode_seq]

    def to_c(self) -> capi.GaitC:
        g = capi.GaitC()
        g.n_modes = len(self._gait_mode)
        for i, m in enumerate(self._gait_mode):
            g.modes[i] = m
        for i, t in enumerate(self._gait_timing):
            g.timings[i] = t
        return g


def c_round(v: float) -> int:
    """C `round()` (half away from zero)."""
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def make_problem_desc(n_wb: int, n_fb: int, mode_seq: List[int], timings: List[float],
                      dt_wb: float, dt_fb: float, vel: float, height: float = 0.0,
                      N: Optional[List[int]] = None) -> capi.ProblemDesc:
    """MHPCLocomotion::build_problem (MHPCLocomotion.cpp:63-104): N = round(timing / dt)
    with float timings and float dt promoted to double."""
    d = capi.ProblemDesc()
    np_ = n_wb + n_fb
    if not 1 <= np_ <= capi.MHPC_MAX_PHASES:
        raise ValueError("number of phases out of range")
    d.n_wb, d.n_fb = n_wb, n_fb
    d.dt_wb, d.dt_fb = f32(dt_wb), f32(dt_fb)
    for p in range(np_):
        d.mode_seq[p] = mode_seq[p]
        if N is not None:
            d.N[p] = N[p]
        else:
            dt = d.dt_wb if p < n_wb else d.dt_fb
            d.N[p] = c_round(f32(timings[p]) / dt)
    d.vel_cmd = f32(vel)
    d.height_cmd = f32(height)
    d.precision = 64
    return d


def desc_from_params(params: MHPCUserParameters, gait: Gait) -> capi.ProblemDesc:
    n = params.n_wbphase + params.n_fbphase
    seq = gait.get_mode_seq(params.cmode, n)
    cmd = params.usrcmd or USRCMD()
    return make_problem_desc(params.n_wbphase, params.n_fbphase, seq, gait.get_timings(seq),
                             params.dt_wb, params.dt_fb, cmd.vel, cmd.height)


# Default initial condition (MHPCLocomotion.cpp:37-39)
Q0 = np.array([0.0927, -0.1093, -0.1542, 1.0957, -2.2033, 0.9742, -1.7098])
QD0 = np.array([0.9011, 0.2756, 0.7333, 0.0446, 0.0009, 1.3219, 2.7346])
X0_DEFAULT = np.concatenate([Q0, QD0])
STATE_PROJ_ROWS = [0, 1, 2, 7, 8, 9]  # _stateProj (MHPCLocomotion.cpp:32-34)

X0_SEED = 0x4D485043
_X0_AMP = np.array([0.01, 0.01] + [0.02] * 5 + [0.05] * 7)
_M64 = (1 << 64) - 1


def _splitmix64(state: int):
    state = (state + 0x9E3779B97F4A7C15) & _M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return state, z ^ (z >> 31)


def random_x0(batch: int, seed: int = X0_SEED, offset: int = 0) -> np.ndarray:
    """x0_b = x0_default + delta_b.  Problem b draws from its own
    splitmix64 stream, state0 = seed ^ (b * 0xD1B54A32D192ED03); U = (next >> 11) * 2^-53,
    delta = amp * (2U - 1).  `offset` = global index of the first problem (sharding)."""
    out = np.empty((batch, 14))
    for i in range(batch):
        b = offset + i
        st = (seed ^ ((b * 0xD1B54A32D192ED03) & _M64)) & _M64
        for j in range(14):
            st, z = _splitmix64(st)
            U = (z >> 11) * (1.0 / (1 << 53))
            out[i, j] = X0_DEFAULT[j] + _X0_AMP[j] * (2 * U - 1)
    return out


def _blob_array(blob) -> np.ndarray:
    """A snapshot blob (bytes-like or numpy uint8) as a contiguous 1-d uint8 array."""
    if isinstance(blob, np.ndarray):
        a = np.ascontiguousarray(blob).reshape(-1)
        if a.dtype != np.uint8:
            raise ValueError("a snapshot blob is uint8")
        return a
    return np.frombuffer(blob, dtype=np.uint8)


def snapshot_status(blob, first: int = 0, count: Optional[int] = None) -> np.ndarray:
    """mhpc_snapshot_status: the solve status of entries [first, first + count) (None: to the last)
    as their last solve left it.  No handle, no GPU."""
    a = _blob_array(blob)
    if count is None:
        count = snapshot_info(a)["n_entries"] - first
    st = np.zeros(count, dtype=np.int32)
    capi.check(capi.lib().mhpc_snapshot_status(a.ctypes.data, int(a.size), int(first), int(count),
                                               capi.iptr(st)), "mhpc_snapshot_status")
    return st


def snapshot_info(blob) -> dict:
    """mhpc_snapshot_info: what the blob's header says (format version, entry count, precision,
    alpha, sweep arithmetic, x0 row width, knot stride, store shape, payload bytes per entry, the
    source's point of the call order).  Host memory only: no handle, no GPU."""
    import ctypes
    a = _blob_array(blob)
    info = capi.SnapshotInfo()
    capi.check(capi.lib().mhpc_snapshot_info(a.ctypes.data, int(a.size), ctypes.byref(info)),
               "mhpc_snapshot_info")
    return info.as_dict()


def snapshot_entry(blob, i: int) -> dict:
    """mhpc_snapshot_entry: entry i's descriptor (with its command), option record, cost weights
    and constraint parameters, and the status its last solve left.  No handle, no GPU."""
    import ctypes
    a = _blob_array(blob)
    d, o, w, c = capi.ProblemDesc(), capi.HsddpOption(), capi.CostWeights(), capi.ConstraintParams()
    capi.check(capi.lib().mhpc_snapshot_entry(a.ctypes.data, int(a.size), int(i), ctypes.byref(d),
                                              ctypes.byref(o), ctypes.byref(w), ctypes.byref(c)),
               "mhpc_snapshot_entry")
    return {"desc": d, "option": HSDDP_OPTION.from_c(o), "weights": w, "constraints": c,
            "status": int(snapshot_status(a, i, 1)[0])}


def load_snapshot(path) -> np.ndarray:
    """A snapshot file (save_problems) as a numpy uint8 array."""
    return np.fromfile(path, dtype=np.uint8)


# ----------------------------------------------------------------------------------------
class SinglePhaseView:
    """One phase of the batch after a solve, with the public members of the reference's
    SinglePhaseAbstract (SinglePhaseAbstract.h:66-134): _modeidx, _phaseidx, _dt,
    _N_TIMESTEPS, _xsize/_usize/_ysize, and _V / _dV (phase cost, expected change) as
    [batch] arrays; get_nominal_ms_ptr() / get_CTG_info_ptr() return the phase's nominal
    (x, u, y) and cost-to-go (G = Vx, du, K) arrays [batch][N][...] (MHPC_CompoundTypes.h:7-22,
    88-101).  Read lazily from the device; valid until the next solve / update_problem."""

    def __init__(self, loco: "MHPCLocomotion", p: int):
        d = loco.desc
        self._loco, self._phaseidx = loco, p
        self._modeidx = int(d.mode_seq[p])
        self._N_TIMESTEPS = int(d.N[p])
        self._xsize, self._usize, self._ysize = d.xsize(p), 4, 4
        self._dt = float(d.dt_wb if p < d.n_wb else d.dt_fb)

    def get_modeidx(self) -> int:
        return self._modeidx

    @property
    def _V(self) -> np.ndarray:
        return self._loco.get_scalars()["V"][:, self._phaseidx]

    @property
    def _dV(self) -> np.ndarray:
        return self._loco.get_scalars()["dV"][:, self._phaseidx]

    def get_nominal_ms_ptr(self) -> dict:
        q = self._loco.get_phase(self._phaseidx)
        return {"x": q["x"], "u": q["u"], "y": q["y"]}

    def get_CTG_info_ptr(self) -> dict:
        q = self._loco.get_phase(self._phaseidx)
        return {"G": q["Vx"], "du": q["du"], "K": q["K"]}

    def get_terminal_state(self) -> np.ndarray:
        return self.get_nominal_ms_ptr()["x"][:, -1, :]


class MHPCLocomotion:
    """Batched MHPCLocomotion<double> over the C-ABI.

    MHPCLocomotion(params, gait, option)               (MHPCLocomotion.cpp:8-43)
    .initialization()                                    (:47-53)
    .solve_mhpc()                                        (:167-195)
    .print_debugInfo(dirname)                            (:293-380)
    Extensions: `batch`, `set_initial_condition(x0[batch][n])` before initialization
    (the reference always starts from its private default x0), `desc=` for layouts the
    reference's constructor cannot express (SRB-only C1, N > 110 C2)."""

    def __init__(self, params: Optional[MHPCUserParameters] = None, gait: Optional[Gait] = None,
                 option: Optional[HSDDP_OPTION] = None, batch: int = 1, device: int = 0,
                 desc: Optional[capi.ProblemDesc] = None):
        self.params = params or MHPCUserParameters(usrcmd=USRCMD(vel=1.5))
        self.gait = gait or Gait()
        self.option = option or HSDDP_OPTION()
        self.desc = desc if desc is not None else desc_from_params(self.params, self.gait)
        self.batch = int(batch)
        self.device = int(device)
        self._opt_c = self.option.to_c()
        L = capi.lib()
        h = __import__("ctypes").c_void_p()
        capi.check(L.mhpc_create(self.desc, self._opt_c, self.batch, self.device,
                                 __import__("ctypes").byref(h)), "mhpc_create")
        self._h = h
        self.descs = None  # per-problem descriptors once set_layouts mixes layouts
        self._default_x0()
        self.status = np.zeros(self.batch, dtype=np.int32)

    def _x0_row(self) -> int:
        ds = self.descs or [self.desc]
        return 14 if any(d.n_wb > 0 for d in ds) else 6

    def _default_x0(self):
        n0 = self._x0_row()
        x0 = X0_DEFAULT if n0 == 14 else X0_DEFAULT[STATE_PROJ_ROWS]
        self._x0 = np.tile(x0, (self.batch, 1)).astype(np.float64)
        self._x0_on_device = False

    def _push_x0(self):
        """The host copy of x0 to the device (mhpc_set_x0) -- unless the device rows are the
        current ones (set_initial_condition_device, advance_x0): then there is nothing to push."""
        if not self._x0_on_device:
            capi.check(capi.lib().mhpc_set_x0(self._h, capi.dptr(self._x0)), "mhpc_set_x0")

    # -- lifecycle ---------------------------------------------------------------------
    def set_initial_condition(self, x0: np.ndarray):
        x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(self.batch, -1))
        if x0.shape[1] != self._x0_row():
            raise ValueError("x0 has the wrong state size for phase 0")
        self._x0 = x0
        self._x0_on_device = False

    def set_initial_condition_device(self, t):
        """mhpc_set_x0_device: the initial states from a torch tensor [batch][r] on the handle's
        device (float32 or float64, inner stride 1, any row stride: a slice of a simulator's state
        tensor), read on the current torch stream's order, at once.  The device rows are then the
        current ones: initialization() / update_problem(s) push no host copy over them;
        get_x0() reads them back for those who want the values."""
        ptr, ld, dtype, stream = self._device_rows(t, self._x0_row(), "x0")
        capi.check(capi.lib().mhpc_set_x0_device(self._h, ptr, ld, dtype, stream),
                   "mhpc_set_x0_device")
        self._x0_on_device = True

    def initialization(self):
        L = capi.lib()
        self._push_x0()
        capi.check(L.mhpc_initialize(self._h), "mhpc_initialize")

    def solve_mhpc(self) -> np.ndarray:
        capi.check(capi.lib().mhpc_solve(self._h, capi.iptr(self.status)), "mhpc_solve")
        return self.status

    def update_problem(self, gait: Optional[Gait] = None):
        """MHPCLocomotion::update_problem (MHPCLocomotion.cpp:107-158) for every problem: the
        gait advances one mode, the phase buffers rotate (warm start of the next solve), the
        references follow the x0 given to set_initial_condition."""
        L = capi.lib()
        self._push_x0()
        g = (gait or self.gait).to_c()
        capi.check(L.mhpc_update_problem(self._h, __import__("ctypes").byref(g)),
                   "mhpc_update_problem")
        self._refresh_descs()

    # -- per-problem phase layouts: the batch axis over gait schedules ----------------------
    def set_layouts(self, descs, layout_of_problem=None):
        """mhpc_set_layouts: problem b gets descs[layout_of_problem[b]] (descs[b % len] when
        None) -- each controller of the batch at its own gait / gait point, as the reference
        builds one layout per MHPCLocomotion instance (MHPCLocomotion.cpp:63-104).  The
        initial states return to the default; set_initial_condition + initialization follow."""
        import ctypes
        arr = (capi.ProblemDesc * len(descs))(*descs)
        lop = (None if layout_of_problem is None
               else np.ascontiguousarray(layout_of_problem, dtype=np.int32))
        capi.check(capi.lib().mhpc_set_layouts(self._h, len(descs), arr, capi.iptr(lop)),
                   "mhpc_set_layouts")
        self._refresh_descs()
        self._default_x0()

    def update_problems(self, gaits, gait_of_problem=None, steps=None):
        """Per-problem update_problem (mhpc_update_problems): problem b takes steps[b] gait
        steps of gaits[gait_of_problem[b]] (0: keeps its layout); references follow the x0 of
        set_initial_condition for every problem."""
        import ctypes
        L = capi.lib()
        self._push_x0()
        gs = (capi.GaitC * len(gaits))(*[g.to_c() for g in gaits])
        gop = (None if gait_of_problem is None
               else np.ascontiguousarray(gait_of_problem, dtype=np.int32))
        st = None if steps is None else np.ascontiguousarray(steps, dtype=np.int32)
        capi.check(L.mhpc_update_problems(self._h, len(gaits), gs, capi.iptr(gop), capi.iptr(st)),
                   "mhpc_update_problems")
        self._refresh_descs()

    # -- per-problem re-initialisation: restart lost problems inside a live batch -------------
    def reset_problems(self, problems, x0=None, descs=None, desc_of=None):
        """mhpc_reset_problems: initialization() of the listed problems only -- the reference's
        set_initial_condition + initialization() on one controller of a fleet
        (MHPCLocomotion.cpp:47-53).  x0 [len(problems)][r] in list order (None: each keeps its
        current device row); descs / desc_of move listed problem i to descs[desc_of[i]]
        (descs[i % len] when None), else it keeps its descriptor with identity phase buffers.
        Every other problem keeps its warm start, bit for bit.  After a solve, follow with
        update_problems(steps=0 for the reset problems); before a solve, just solve."""
        pr = np.ascontiguousarray(problems, dtype=np.int32).reshape(-1)
        if x0 is not None:
            x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(pr.size, -1))
            if x0.shape[1] != self._x0_row():
                raise ValueError("x0 must be [len(problems)][x0 row length]")
        arr, dof = None, None
        if descs is not None:
            arr = (capi.ProblemDesc * len(descs))(*descs)
            if desc_of is not None:
                dof = np.ascontiguousarray(desc_of, dtype=np.int32)
                if dof.shape != pr.shape:
                    raise ValueError("desc_of must have one entry per listed problem")
        capi.check(capi.lib().mhpc_reset_problems(self._h, int(pr.size), capi.iptr(pr),
                                                  capi.dptr(x0), 0 if descs is None else len(descs),
                                                  arr, capi.iptr(dof)), "mhpc_reset_problems")
        if x0 is not None and not self._x0_on_device:  # what the next update_problem(s) hands back
            self._x0 = self._x0.copy()
            self._x0[pr] = x0
        if descs is not None:
            self._refresh_descs()

    # -- per-problem ticks: update and solve the listed problems only --------------------------
    def tick_problems(self, problems, x0=None, gaits=None, gait_of=None, steps=None) -> np.ndarray:
        """mhpc_tick_problems: one MPC tick of the listed problems and of nobody else -- the
        reference's set_initial_condition + update_problem + solve_mhpc on single controllers of
        a fleet, each when its own gait mode ends.  x0 [len(problems)][r] in list order (None:
        each keeps its current device row); listed problem i takes steps[i] gait steps (None: one)
        of gaits[gait_of[i]] (None: gaits[0]; gaits None: the handle's gait, or no gait at all
        when every step is 0).  Each listed problem comes out as after the three calls in a
        handle of its own; every other problem keeps its state bit for bit.  Returns the listed
        problems' status in list order (also written to self.status[problems]); self.last_tick_ms
        is the device time of the whole tick."""
        import ctypes
        pr = np.ascontiguousarray(problems, dtype=np.int32).reshape(-1)
        if x0 is not None:
            x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(pr.size, -1))
            if x0.shape[1] != self._x0_row():
                raise ValueError("x0 must be [len(problems)][x0 row length]")
        st = None if steps is None else np.ascontiguousarray(steps, dtype=np.int32).reshape(-1)
        if st is not None and st.shape != pr.shape:
            raise ValueError("steps must have one entry per listed problem")
        gop = None if gait_of is None else np.ascontiguousarray(gait_of, dtype=np.int32).reshape(-1)
        if gop is not None and gop.shape != pr.shape:
            raise ValueError("gait_of must have one entry per listed problem")
        if gaits is None and not (st is not None and not st.any()):
            gaits = [self.gait]
        gs = None if gaits is None else (capi.GaitC * len(gaits))(*[g.to_c() for g in gaits])
        status = np.zeros(pr.size, dtype=np.int32)
        ms = ctypes.c_float(0.0)
        capi.check(capi.lib().mhpc_tick_problems(self._h, int(pr.size), capi.iptr(pr), capi.dptr(x0),
                                                 0 if gaits is None else len(gaits), gs,
                                                 capi.iptr(gop), capi.iptr(st), capi.iptr(status),
                                                 ctypes.byref(ms)), "mhpc_tick_problems")
        self.last_tick_ms = float(ms.value)
        self.status[pr] = status
        if x0 is not None and not self._x0_on_device:  # what the next update_problem(s) hands back
            self._x0 = self._x0.copy()
            self._x0[pr] = x0
        self._refresh_descs()
        return status

    def reserve_knots(self, knots: int):
        """mhpc_reserve_knots: floor of the knot stride of the packed arrays, so that later ticks
        can step into longer layouts; before initialization()."""
        capi.check(capi.lib().mhpc_reserve_knots(self._h, int(knots)), "mhpc_reserve_knots")

    # -- copies of live problems: a slot becomes another controller ---------------------------
    def copy_problems(self, dst_problems, src_problems, src: Optional["MHPCLocomotion"] = None) -> float:
        """mhpc_copy_problems: problem dst_problems[i] of this handle becomes a copy of problem
        src_problems[i] of `src` (None: of this handle) as it stands -- warm start, solver state,
        x0 row, command, parameter set, layout and phase buffers (copying a controller object in
        the reference).  A source may repeat (one robot forks into several candidates).  Every
        other problem of both handles keeps its state bit for bit.  Returns the device time of
        the copy in ms; change the clones' commands / parameter sets / x0 afterwards with the
        setters."""
        import ctypes
        src = self if src is None else src
        dp = np.ascontiguousarray(dst_problems, dtype=np.int32).reshape(-1)
        sp = np.ascontiguousarray(src_problems, dtype=np.int32).reshape(-1)
        if dp.shape != sp.shape:
            raise ValueError("one source problem per destination problem")
        ms = ctypes.c_float(0.0)
        capi.check(capi.lib().mhpc_copy_problems(self._h, capi.iptr(dp), src._h, capi.iptr(sp),
                                                 int(dp.size), ctypes.byref(ms)),
                   "mhpc_copy_problems")
        # the host mirrors follow: the rows update_problem(s) hands back to the device are the
        # device's own, the last solve's status is the source's, descriptors and commands travel
        if not self._x0_on_device:
            self._x0 = self._x0.copy()
            self._x0[dp] = self.get_x0()[dp]
        self.status[dp] = src.status[sp]
        self._refresh_descs()
        return float(ms.value)

    # -- snapshots of live problems: checkpoints, migration between ranks, replays ---------------
    def _problem_list(self, problems) -> np.ndarray:
        if problems is None:
            return np.arange(self.batch, dtype=np.int32)
        return np.ascontiguousarray(problems, dtype=np.int32).reshape(-1)

    def snapshot_size(self, problems=None) -> int:
        """mhpc_snapshot_size: the exact blob size of a snapshot of the listed problems."""
        import ctypes
        pr = self._problem_list(problems)
        n = ctypes.c_int64(0)
        capi.check(capi.lib().mhpc_snapshot_size(self._h, int(pr.size), capi.iptr(pr),
                                                 ctypes.byref(n)), "mhpc_snapshot_size")
        return int(n.value)

    def snapshot_problems(self, problems=None, out=None) -> np.ndarray:
        """mhpc_snapshot_problems: the listed problems (None: all) as they stand, serialised into a
        blob of plain bytes -- everything copy_problems carries, to be restored into this or any
        other handle, in this process or another (restore_problems, from_snapshot).  Returns a
        numpy uint8 array; out: a caller's contiguous uint8 buffer of at least snapshot_size()
        bytes (for example a pinned torch tensor's numpy view), whose leading part is returned.
        self.last_snapshot_ms is the device time of the pack launches."""
        import ctypes
        pr = self._problem_list(problems)
        size = self.snapshot_size(pr)
        if out is None:
            out = np.empty(size, dtype=np.uint8)
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.ndim == 1
                and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("out must be a writeable contiguous 1-d numpy uint8 array")
        ms = ctypes.c_float(0.0)
        capi.check(capi.lib().mhpc_snapshot_problems(self._h, int(pr.size), capi.iptr(pr),
                                                     out.ctypes.data, int(out.size), ctypes.byref(ms)),
                   "mhpc_snapshot_problems")
        self.last_snapshot_ms = float(ms.value)
        return out[:size]

    def restore_problems(self, dst_problems, blob, entries=None) -> float:
        """mhpc_restore_problems: problem dst_problems[i] of this handle becomes entry entries[i]
        (None: entry i) of the snapshot `blob` -- the copy_problems that could have been made at the
        moment of the snapshot.  An entry may repeat.  A restore that lists every problem of the
        handle also adopts the blob's point of the call order (resume from a checkpoint).  Returns
        the device time of the unpack launches in ms."""
        import ctypes
        dp = np.ascontiguousarray(dst_problems, dtype=np.int32).reshape(-1)
        en = None
        if entries is not None:
            en = np.ascontiguousarray(entries, dtype=np.int32).reshape(-1)
            if en.shape != dp.shape:
                raise ValueError("one blob entry per destination problem")
        a = _blob_array(blob)
        ms = ctypes.c_float(0.0)
        capi.check(capi.lib().mhpc_restore_problems(self._h, int(dp.size), capi.iptr(dp),
                                                    a.ctypes.data, int(a.size), capi.iptr(en),
                                                    ctypes.byref(ms)), "mhpc_restore_problems")
        # the host mirrors follow, as after copy_problems
        if not self._x0_on_device:
            self._x0 = self._x0.copy()
            self._x0[dp] = self.get_x0()[dp]
        self.status[dp] = snapshot_status(a)[np.arange(dp.size) if en is None else en]
        self._refresh_descs()
        self.option = self.get_options()
        return float(ms.value)

    def save_problems(self, path, problems=None) -> int:
        """snapshot_problems written to a file; returns its size in bytes."""
        blob = self.snapshot_problems(problems)
        with open(path, "wb") as f:
            f.write(blob.tobytes())
        return int(blob.size)

    @classmethod
    def from_snapshot(cls, blob, device: int = 0, batch: Optional[int] = None,
                      gait: Optional[Gait] = None) -> "MHPCLocomotion":
        """A handle that can hold `blob` and holds it: created with the entries' descriptors
        (set_layouts), their longest layout as reserve_knots, the blob's alpha, precision and sweep
        arithmetic and the distinct option records (set_option_sets); then initialised and every
        entry restored into problems 0..n-1.  batch None: the entry count, so the restore covers
        the handle and it resumes at the blob's point of the call order; a larger batch leaves the
        other problems as initialization() made them.  gait: what update_problem() steps with (a
        blob holds gait points, not gaits)."""
        a = _blob_array(blob)
        info = snapshot_info(a)
        n = info["n_entries"]
        ents = [snapshot_entry(a, i) for i in range(n)]
        B = n if batch is None else int(batch)
        if B < n:
            raise ValueError("batch smaller than the blob's entry count")
        descs, lop, key_of = [], [], {}
        for e in ents:  # one handle-wide command in the descriptors: the entries' own travel with them
            d = capi.ProblemDesc.from_buffer_copy(bytes(e["desc"]))
            d.vel_cmd, d.height_cmd = ents[0]["desc"].vel_cmd, ents[0]["desc"].height_cmd
            k = bytes(d)
            if k not in key_of:
                key_of[k] = len(descs)
                descs.append(d)
            lop.append(key_of[k])
        lop += [0] * (B - n)
        opts, oop = [], []
        for e in ents:
            if e["option"] not in opts:
                opts.append(e["option"])
            oop.append(opts.index(e["option"]))
        oop += [0] * (B - n)
        loco = cls(desc=descs[0], gait=gait, option=opts[0], batch=B, device=device)
        try:
            if info["sweep_bits"] == 32:
                loco.set_kernel_variant(sweep_bits=32)
            if len(descs) > 1:
                loco.set_layouts(descs, lop)
            loco.reserve_knots(info["knot_stride"])
            if len(opts) > 1:
                loco.set_option_sets(opts, oop)
            loco.initialization()
            loco.restore_problems(np.arange(n, dtype=np.int32), a)
        except Exception:
            loco.close()
            raise
        return loco

    def lost_problems(self) -> np.ndarray:
        """Problems whose last solve did not end MHPC_SOLVE_OK or left a non-finite cost."""
        J = self.get_scalars()["J"]
        return np.flatnonzero((self.status != capi.MHPC_SOLVE_OK) | ~np.isfinite(J))

    # -- per-problem user commands: the batch axis over USRCMD ------------------------------
    def _command_array(self, v, name: str):
        """None, a scalar (broadcast over the batch) or [batch] values, each rounded through
        f32() as desc_from_params rounds USRCMD's float members."""
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(self.batch, float(a))
        if a.shape != (self.batch,):
            raise ValueError(f"{name} must be a scalar or have one entry per problem")
        return np.ascontiguousarray([f32(x) for x in a], dtype=np.float64)

    def set_commands(self, vel=None, height=None):
        """mhpc_set_commands: problem b tracks speed vel[b] at body height height[b] (each a
        scalar or [batch]; None keeps the current values) -- the usrcmd of one controller per
        problem (MHPCLocomotion.cpp:98-103).  Takes effect at the next initialization() /
        update_problem(s); an initialised handle refuses to solve until then."""
        v, hgt = self._command_array(vel, "vel"), self._command_array(height, "height")
        capi.check(capi.lib().mhpc_set_commands(self._h, capi.dptr(v), capi.dptr(hgt)),
                   "mhpc_set_commands")

    def get_commands(self) -> dict:
        out = {"vel": np.zeros(self.batch), "height": np.zeros(self.batch)}
        capi.check(capi.lib().mhpc_get_commands(self._h, capi.dptr(out["vel"]),
                                                capi.dptr(out["height"])), "mhpc_get_commands")
        return out

    def get_reference_problems(self, p: int, first: int, count: int) -> np.ndarray:
        """The tracking reference x of phase p for problems [first, first + count),
        [count][N][xsize] (ReferenceGen.h:53-109; one phase shape over the range)."""
        d = self.descs[first] if self.descs else self.desc
        xref = np.zeros((count, d.N[p], d.xsize(p)))
        capi.check(capi.lib().mhpc_get_reference_problems(self._h, p, int(first), int(count),
                                                          capi.dptr(xref)),
                   "mhpc_get_reference_problems")
        return xref

    def problem_desc(self, b: int) -> capi.ProblemDesc:
        import ctypes
        d = capi.ProblemDesc()
        capi.check(capi.lib().mhpc_get_problem_desc(self._h, int(b), ctypes.byref(d)),
                   "mhpc_get_problem_desc")
        return d

    def num_layouts(self) -> int:
        import ctypes
        n = ctypes.c_int(0)
        capi.check(capi.lib().mhpc_num_layouts(self._h, ctypes.byref(n)), "mhpc_num_layouts")
        return n.value

    def max_phases(self) -> int:
        """Row length of get_scalars' per-phase arrays (mhpc_max_phases)."""
        import ctypes
        n = ctypes.c_int(0)
        capi.check(capi.lib().mhpc_max_phases(self._h, ctypes.byref(n)), "mhpc_max_phases")
        return n.value

    def _refresh_descs(self):
        ds = [self.problem_desc(b) for b in range(self.batch)]
        key = lambda d: bytes(d)
        self.descs = ds if any(key(d) != key(ds[0]) for d in ds) else None
        self.desc = ds[0]

    def get_phase_problems(self, p: int, first: int, count: int) -> dict:
        """Phase p of problems [first, first + count) (one phase shape over the range)."""
        d = self.descs[first] if self.descs else self.desc
        n, N = d.xsize(p), d.N[p]
        out = {k: np.zeros(s) for k, s in (
            ("x", (count, N, n)), ("u", (count, N, 4)), ("y", (count, N, 4)),
            ("K", (count, N, 4, n)), ("du", (count, N, 4)), ("Vx", (count, N, n)))}
        capi.check(capi.lib().mhpc_get_phase_problems(
            self._h, p, int(first), int(count),
            *[capi.dptr(out[k]) for k in ("x", "u", "y", "K", "du", "Vx")]), "mhpc_get_phase_problems")
        return out

    def problem_concatenated(self, b: int) -> dict:
        """Phase-concatenated arrays of one problem (the oracle's layout, row b)."""
        d = self.descs[b] if self.descs else self.desc
        parts = [self.get_phase_problems(p, b, 1) for p in range(d.n_phases)]
        return {
            "X": np.concatenate([q["x"].ravel() for q in parts]),
            "U": np.concatenate([q["u"].ravel() for q in parts]),
            "Y": np.concatenate([q["y"].ravel() for q in parts]),
            "K": np.concatenate([q["K"].ravel() for q in parts]),
            "DU": np.concatenate([q["du"].ravel() for q in parts]),
            "G": np.concatenate([q["Vx"].ravel() for q in parts]),
        }

    # MultiPhaseDDP's public members (MultiPhaseDDP.h:12-63), batched: [batch] arrays
    @property
    def _phases(self):
        return [SinglePhaseView(self, p) for p in range(self.desc.n_phases)]

    @property
    def _n_phases(self) -> int:
        return self.desc.n_phases

    @property
    def _actual_cost(self) -> np.ndarray:
        return self.get_scalars()["J"]

    @property
    def _exp_cost_change(self) -> np.ndarray:
        return self.get_scalars()["dV_exp"]

    @property
    def _tconstr_violation(self) -> np.ndarray:
        return self.get_scalars()["viol"]

    # -- cost / constraint parameters (CostBase.h:9-46, ConstraintsBase.h:11-50) -----------
    def set_cost_weights(self, w: "capi.CostWeights"):
        """Replace the diagonal cost weights (MHPCCost.cpp:24-75 values by default) for every
        later solve of this handle (mhpc_set_cost_weights)."""
        capi.check(capi.lib().mhpc_set_cost_weights(self._h, __import__("ctypes").byref(w)),
                   "mhpc_set_cost_weights")

    def get_cost_weights(self) -> "capi.CostWeights":
        w = capi.CostWeights()
        capi.check(capi.lib().mhpc_get_cost_weights(self._h, __import__("ctypes").byref(w)),
                   "mhpc_get_cost_weights")
        return w

    def set_constraint_params(self, c: "capi.ConstraintParams"):
        """Replace torque limit, friction coefficient and the AL / ReB initial parameters
        (MHPCConstraints.cpp:14-88 values by default); the initial values take effect at the
        next initialization() / update_problem() (mhpc_set_constraint_params)."""
        capi.check(capi.lib().mhpc_set_constraint_params(self._h, __import__("ctypes").byref(c)),
                   "mhpc_set_constraint_params")

    def get_constraint_params(self) -> "capi.ConstraintParams":
        c = capi.ConstraintParams()
        capi.check(capi.lib().mhpc_get_constraint_params(self._h, __import__("ctypes").byref(c)),
                   "mhpc_get_constraint_params")
        return c

    # -- per-problem parameter sets: the batch axis over weights / constraint parameters ----
    def set_param_sets(self, weights, constraints, set_of_problem=None):
        """mhpc_set_param_sets: problem b solves with weights[set_of_problem[b]] and
        constraints[set_of_problem[b]] (b % n_sets when None) -- the WBCost / FBCost /
        WBConstraint objects of one controller per problem (MHPCCost.cpp:24-75,
        MHPCConstraints.cpp:14-88).  weights: a sequence of capi.CostWeights or None (every set
        keeps problem 0's current weights); constraints likewise with capi.ConstraintParams; at
        least one is given, both of the same length 1..MHPC_MAX_PARAM_SETS.  Takes effect at the
        next initialization() / update_problem(s); an initialised handle refuses to solve until
        then."""
        if weights is None and constraints is None:
            raise ValueError("give weights, constraints or both")
        if weights is not None and constraints is not None and len(weights) != len(constraints):
            raise ValueError("weights and constraints must have one entry per set each")
        n = len(weights if weights is not None else constraints)
        if not 1 <= n <= capi.MHPC_MAX_PARAM_SETS:
            raise ValueError("the number of sets must be 1..MHPC_MAX_PARAM_SETS")
        for seq, cls in ((weights, capi.CostWeights), (constraints, capi.ConstraintParams)):
            if seq is not None and not all(isinstance(v, cls) for v in seq):
                raise TypeError(f"every set must be a capi.{cls.__name__}")
        sop = None
        if set_of_problem is not None:
            sop = np.ascontiguousarray(set_of_problem, dtype=np.int32)
            if sop.shape != (self.batch,):
                raise ValueError("set_of_problem must have one entry per problem")
            if sop.size and (sop.min() < 0 or sop.max() >= n):
                raise ValueError("set_of_problem entry out of range")
        w = None if weights is None else (capi.CostWeights * n)(*weights)
        c = None if constraints is None else (capi.ConstraintParams * n)(*constraints)
        capi.check(capi.lib().mhpc_set_param_sets(self._h, n, w, c, capi.iptr(sop)),
                   "mhpc_set_param_sets")

    def get_problem_params(self, b: int):
        """(capi.CostWeights, capi.ConstraintParams) of problem b (mhpc_get_problem_params)."""
        import ctypes
        w, c = capi.CostWeights(), capi.ConstraintParams()
        capi.check(capi.lib().mhpc_get_problem_params(self._h, int(b), ctypes.byref(w),
                                                      ctypes.byref(c)), "mhpc_get_problem_params")
        return w, c

    def num_param_sets(self) -> int:
        import ctypes
        n = ctypes.c_int(0)
        capi.check(capi.lib().mhpc_num_param_sets(self._h, ctypes.byref(n)), "mhpc_num_param_sets")
        return n.value

    # -- per-problem option sets: the batch axis over iteration budgets and thresholds ------
    def set_options(self, option: HSDDP_OPTION):
        """mhpc_set_options: every problem gets `option` (the reference's `_option = o` on every
        controller); alpha must be the handle's.  Allowed at any point of the call order; takes
        effect at the next solve or tick."""
        import ctypes
        o = option.to_c()
        capi.check(capi.lib().mhpc_set_options(self._h, ctypes.byref(o)), "mhpc_set_options")
        self.option = option

    def get_options(self) -> HSDDP_OPTION:
        """Problem 0's option record (mhpc_get_options)."""
        return self.get_problem_options(0)

    def set_option_sets(self, options, set_of_problem=None):
        """mhpc_set_option_sets: problem b solves with options[set_of_problem[b]] (b % n_sets
        when None), a sequence of 1..MHPC_MAX_OPTION_SETS HSDDP_OPTION that share the handle's
        alpha.  A solve's launch schedule runs to the largest budgets among the problems it
        covers; a problem with a smaller budget computes what it would in a handle of its own."""
        n = len(options)
        sop = None
        if set_of_problem is not None:
            sop = np.ascontiguousarray(set_of_problem, dtype=np.int32)
            if sop.shape != (self.batch,):
                raise ValueError("set_of_problem must have one entry per problem")
        arr = (capi.HsddpOption * max(n, 1))(*[o.to_c() for o in options])
        capi.check(capi.lib().mhpc_set_option_sets(self._h, n, arr, capi.iptr(sop)),
                   "mhpc_set_option_sets")
        self.option = self.get_options()

    def get_problem_options(self, b: int) -> HSDDP_OPTION:
        """Problem b's option record (mhpc_get_problem_options)."""
        import ctypes
        o = capi.HsddpOption()
        capi.check(capi.lib().mhpc_get_problem_options(self._h, int(b), ctypes.byref(o)),
                   "mhpc_get_problem_options")
        return HSDDP_OPTION.from_c(o)

    def num_option_sets(self) -> int:
        import ctypes
        n = ctypes.c_int(0)
        capi.check(capi.lib().mhpc_num_option_sets(self._h, ctypes.byref(n)), "mhpc_num_option_sets")
        return n.value

    def get_exec(self) -> dict:
        """Execution horizon of solve_mhpc (MHPCLocomotion.cpp:176-194): the nominal and
        cost-to-go of phase 0, followed by phase 1 when there are two WB phases."""
        parts = [self.get_phase(0)] + ([self.get_phase(1)] if self.desc.n_wb > 1 else [])
        return {k: np.concatenate([q[k] for q in parts], axis=1) for k in parts[0]}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            capi.lib().mhpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- outputs -----------------------------------------------------------------------
    def get_phase(self, p: int) -> dict:
        n, N, B = self.desc.xsize(p), self.desc.N[p], self.batch
        out = {k: np.zeros(s) for k, s in (
            ("x", (B, N, n)), ("u", (B, N, 4)), ("y", (B, N, 4)), ("K", (B, N, 4, n)),
            ("du", (B, N, 4)), ("Vx", (B, N, n)))}
        capi.check(capi.lib().mhpc_get_phase(
            self._h, p, *[capi.dptr(out[k]) for k in ("x", "u", "y", "K", "du", "Vx")]),
            "mhpc_get_phase")
        return out

    def get_scalars(self) -> dict:
        B = self.batch
        P = self.max_phases()  # rows of the most phases over the problems' layouts
        out = {"J": np.zeros(B), "dV_exp": np.zeros(B), "viol": np.zeros(B),
               "V": np.zeros((B, P)), "dV": np.zeros((B, P)),
               "trace": np.zeros((B, capi.MHPC_TRACE_LEN), dtype=np.int32)}
        capi.check(capi.lib().mhpc_get_scalars(
            self._h, capi.dptr(out["J"]), capi.dptr(out["dV_exp"]), capi.dptr(out["viol"]),
            capi.dptr(out["V"]), capi.dptr(out["dV"]), capi.iptr(out["trace"])),
            "mhpc_get_scalars")
        return out

    def get_counters(self) -> dict:
        c = capi.Counters()
        capi.check(capi.lib().mhpc_get_counters(self._h, __import__("ctypes").byref(c)),
                   "mhpc_get_counters")
        return {k: getattr(c, k) for k, _ in capi.Counters._fields_}

    def rollout_costs(self, eps) -> dict:
        """Trial rollouts (forward_sweep_dynamics_only) at every step size in `eps` from the
        current nominal and gains, costs only: J, viol [batch][len(eps)] and the device ms."""
        eps = np.ascontiguousarray(eps, dtype=np.float64)
        J = np.zeros((self.batch, eps.shape[0]))
        viol = np.zeros_like(J)
        ms = __import__("ctypes").c_float(0)
        capi.check(capi.lib().mhpc_rollout_costs(self._h, int(eps.shape[0]), capi.dptr(eps),
                                                 capi.dptr(J), capi.dptr(viol),
                                                 __import__("ctypes").byref(ms)),
                   "mhpc_rollout_costs")
        return {"J": J, "viol": viol, "ms": ms.value}

    # -- policy rollouts: the batch axis over measured / perturbed start states -------------
    def _policy_states(self, xs, count: int) -> np.ndarray:
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        if xs.ndim != 3 or xs.shape[0] != count or xs.shape[2] != self._x0_row():
            raise ValueError("xs must be [problems][n_samples][x0 row length]")
        return xs

    def rollout_policy(self, xs, n_phases: int = 0) -> dict:
        """The solved feedback policy u = u_nom + K (x - x_nom) run from the start states
        xs [batch][n_samples][r] (r as set_initial_condition's rows) over the first n_phases
        phases (0: every phase of each problem), nothing modified (mhpc_rollout_policy): J,
        viol [batch][n_samples], x_end [batch][n_samples][r] (the state after the last rolled
        phase's transition: post-impact whole-body state, usable as the next x0) and the
        device ms."""
        import ctypes
        xs = self._policy_states(xs, self.batch)
        S = xs.shape[1]
        J = np.zeros((self.batch, S))
        viol = np.zeros_like(J)
        x_end = np.zeros_like(xs)
        ms = ctypes.c_float(0)
        capi.check(capi.lib().mhpc_rollout_policy(self._h, int(S), capi.dptr(xs), int(n_phases),
                                                  capi.dptr(J), capi.dptr(viol), capi.dptr(x_end),
                                                  ctypes.byref(ms)), "mhpc_rollout_policy")
        return {"J": J, "viol": viol, "x_end": x_end, "ms": ms.value}

    def rollout_policy_phase(self, p: int, first: int, count: int, xs) -> dict:
        """Trajectories of phase p (rolled from phase 0 under the policy) for problems
        [first, first + count) from xs [count][n_samples][r]: x [count][n_samples][N][xsize],
        u, y [count][n_samples][N][4] (mhpc_rollout_policy_phase; one phase shape over the
        range)."""
        xs = self._policy_states(xs, count)
        S = xs.shape[1]
        d = self.descs[first] if self.descs else self.desc
        n, N = d.xsize(p), d.N[p]
        out = {"x": np.zeros((count, S, N, n)), "u": np.zeros((count, S, N, 4)),
               "y": np.zeros((count, S, N, 4))}
        capi.check(capi.lib().mhpc_rollout_policy_phase(
            self._h, int(p), int(first), int(count), int(S), capi.dptr(xs),
            capi.dptr(out["x"]), capi.dptr(out["u"]), capi.dptr(out["y"])),
            "mhpc_rollout_policy_phase")
        return out

    def advance_x0(self, n_phases: int = 1, dx=None):
        """Device-side closed loop (mhpc_advance_x0): every problem's x0 becomes the end state
        of one policy rollout over n_phases phases from x0 + dx (dx [batch][r] or None), with
        no host copy of states (get_x0() reads them back).  update_problem() / initialization()
        follow, as after set_initial_condition."""
        if dx is not None:
            dx = np.ascontiguousarray(dx, dtype=np.float64)
            if dx.shape != (self.batch, self._x0_row()):
                raise ValueError("dx must be [batch][x0 row length]")
        capi.check(capi.lib().mhpc_advance_x0(self._h, int(n_phases), capi.dptr(dx)),
                   "mhpc_advance_x0")
        self._x0_on_device = True  # update_problem() / initialization() push nothing over them

    # -- device-resident control I/O: measured states in, feedback controls out ----------------
    def num_control_steps(self, b: int = 0) -> int:
        """Control steps of problem b (mhpc_num_control_steps): the knots with a control of its
        whole-body phases, or of all its phases when it is SRB-only."""
        import ctypes
        n = ctypes.c_int(0)
        capi.check(capi.lib().mhpc_num_control_steps(self._h, int(b), ctypes.byref(n)),
                   "mhpc_num_control_steps")
        return n.value

    def _device_rows(self, t, cols: int, name: str):
        """(pointer, row stride, dtype code, stream) of a torch tensor [batch][cols] on the
        handle's device; ValueError for anything the library could not address."""
        import torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{name} must be float32 or float64")
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{name} must be on the handle's device")
        if t.dim() != 2 or tuple(t.shape) != (self.batch, cols):
            raise ValueError(f"{name} must be [batch][{cols}]")
        if t.stride(1) != 1 or t.stride(0) < cols:
            raise ValueError(f"{name} must have an inner stride of 1 and a row stride >= {cols}")
        dtype = capi.MHPC_DEV_F32 if t.dtype == torch.float32 else capi.MHPC_DEV_F64
        stream = torch.cuda.current_stream(t.device).cuda_stream
        return t.data_ptr(), int(t.stride(0)), dtype, stream

    def control(self, step, x, want=("u",), out=None) -> dict:
        """The feedback control of every problem at control step step[b] (an int for every problem,
        or [batch]; None: step 0) from its measured state x [batch][r]:
        u = u_nom + K (x - x_nom), the policy rollouts' arithmetic at that knot bit for bit.
        x: a numpy array (mhpc_control) or a torch tensor on the handle's device, float32 or
        float64, inner stride 1 (mhpc_control_device, on the current torch stream's order);
        returns a dict of the same kind with the entries of `want`: "u" [batch][4], "x_nom"
        [batch][r], "u_nom" [batch][4], "K" [batch][4][r].  out: for tensors, {"u": tensor
        [batch][4]} to write u into a slice of the caller's own action tensor."""
        r, B = self._x0_row(), self.batch
        want = tuple(want)
        if not want or any(k not in ("u", "x_nom", "u_nom", "K") for k in want):
            raise ValueError('want: some of "u", "x_nom", "u_nom", "K"')
        st = None
        if step is not None:
            st = np.asarray(step)
            if not np.issubdtype(st.dtype, np.integer):
                raise ValueError("step must be an int or [batch] ints")
            if st.ndim == 0:
                st = np.full(B, int(st))
            if st.shape != (B,):
                raise ValueError("step must be an int or [batch] ints")
            st = np.ascontiguousarray(st, dtype=np.int32)
        shapes = {"u": (B, 4), "x_nom": (B, r), "u_nom": (B, 4), "K": (B, 4, r)}
        L = capi.lib()
        if isinstance(x, np.ndarray) or x is None:
            if out is not None:
                raise ValueError("out is for torch tensors")
            if "u" in want:
                if x is None:
                    raise ValueError("u needs x")
                x = np.ascontiguousarray(x, dtype=np.float64)
                if x.shape != (B, r):
                    raise ValueError("x must be [batch][x0 row length]")
            res = {k: np.zeros(shapes[k]) for k in want}
            capi.check(L.mhpc_control(self._h, capi.iptr(st), capi.dptr(x) if "u" in want else None,
                                      *[capi.dptr(res.get(k)) for k in ("u", "x_nom", "u_nom", "K")]),
                       "mhpc_control")
            return res
        import torch
        xp, ldx, dtype, stream = self._device_rows(x, r, "x")
        res = {}
        for k in want:
            if k == "u" and out is not None and "u" in out:
                res[k] = out["u"]
                if res[k].dtype != x.dtype:
                    raise ValueError("out['u'] must have x's dtype")
            else:
                res[k] = torch.empty(shapes[k], dtype=x.dtype, device=x.device)
        up, ldu = None, 4
        if "u" in res:
            up, ldu, _, _ = self._device_rows(res["u"], 4, "u")
        ptr = lambda k: res[k].data_ptr() if k in res else None
        capi.check(L.mhpc_control_device(self._h, capi.iptr(st), xp, ldx, up, ldu, ptr("x_nom"),
                                         ptr("u_nom"), ptr("K"), dtype, stream),
                   "mhpc_control_device")
        return res

    # -- device-resident plan export: policy windows and results into tensors -------------------
    def _export_list(self, problems):
        """(int32 list or None, n) of an export's problems; None: the whole batch in order."""
        if problems is None:
            return None, self.batch
        lst = np.asarray(problems)
        if lst.ndim != 1 or lst.size < 1 or not np.issubdtype(lst.dtype, np.integer):
            raise ValueError("problems must be a list of ints")
        if lst.min() < 0 or lst.max() >= self.batch or np.unique(lst).size != lst.size:
            raise ValueError("problems: each in 0..batch-1, none twice")
        return np.ascontiguousarray(lst, dtype=np.int32), int(lst.size)

    def _export_dtype(self, dtype, out, int_names):
        """The element type of an export's float tensors: dtype, or that of out's, or float64."""
        import torch
        floats = [t for k, t in (out or {}).items() if k not in int_names and isinstance(t, torch.Tensor)]
        if dtype is None:
            dtype = floats[0].dtype if floats else torch.float64
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype must be torch.float32 or torch.float64")
        return dtype

    def _device_block(self, t, shape, dtype, name: str):
        """(pointer, elements between two problems' blocks) of a torch tensor [n][...] on the
        handle's device whose blocks are dense inside (a view with a larger leading stride is
        fine: a slice [:, t] of a dataset buffer); ValueError for anything the library could
        not address, as _device_rows."""
        import torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}")
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{name} must be on the handle's device")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be {list(shape)}")
        dense = 1
        for d in range(t.dim() - 1, 0, -1):
            if t.shape[d] != 1 and t.stride(d) != dense:
                raise ValueError(f"{name} must be contiguous inside a problem's block")
            dense *= t.shape[d]
        if shape[0] > 1 and t.stride(0) < dense:
            raise ValueError(f"{name} must have a leading stride >= {dense}")
        return t.data_ptr(), (int(t.stride(0)) if shape[0] > 1 else 0)

    def export_plan(self, problems=None, first_step=0, window=None,
                    want=("x_nom", "u_nom", "K"), dtype=None, out=None) -> dict:
        """The next `window` control steps of every listed problem's policy, from first_step (an
        int, or one per listed problem), into torch tensors on the handle's device
        (mhpc_export_plan_device; nothing crosses the host).  Row i belongs to problems[i] (None:
        the whole batch in order); window None: the largest step count among the listed problems.
        Entries of want: "x_nom" [n][W][r], "u_nom" [n][W][4], "K" [n][W][4][r], "du" [n][W][4],
        "Vx" [n][W][r], "y" [n][W][4] of dtype (torch.float64, the default, or torch.float32) and
        "mode" [n][W] int32; "valid" [n] int32 -- the steps of each window that exist -- is always
        returned.  Every value is what get_phase_problems reports for the step's (phase, knot);
        rows past valid and columns past a problem's state size are +0.  out: {name: tensor} to
        write into the caller's own tensors (wanted too), inner-contiguous views with any leading
        stride >= the block -- a slice [:, t] of a dataset buffer [n][T][W][c]; the bytes between
        the blocks are kept.  The device time of the launch is left in self.last_export_ms."""
        import ctypes
        import torch
        kinds = ("x_nom", "u_nom", "K", "du", "Vx", "y", "mode")
        out = dict(out or {})
        names = list(dict.fromkeys([*want, *out]))
        if any(k not in kinds + ("valid",) for k in names):
            raise ValueError('want: some of "x_nom", "u_nom", "K", "du", "Vx", "y", "mode"')
        lst, n = self._export_list(problems)
        if self.descs is None:  # one layout: one count
            steps = np.full(n, self.num_control_steps(0))
        else:
            steps = np.array([self.num_control_steps(int(b)) for b in (range(n) if lst is None else lst)])
        fs = np.asarray(first_step)
        if not np.issubdtype(fs.dtype, np.integer) or fs.ndim > 1:
            raise ValueError("first_step must be an int or one int per listed problem")
        fs = np.full(n, int(fs)) if fs.ndim == 0 else fs
        if fs.shape != (n,):
            raise ValueError("first_step must be an int or one int per listed problem")
        if ((fs < 0) | (fs >= steps)).any():
            raise ValueError("first_step outside 0..num_control_steps - 1")
        fs = np.ascontiguousarray(fs, dtype=np.int32) if fs.any() else None  # (None: step 0, no upload)
        W = int(steps.max()) if window is None else int(window)
        if W < 1 or W > capi.MHPC_MAX_KNOTS:
            raise ValueError("window must be 1..MHPC_MAX_KNOTS")
        dtype = self._export_dtype(dtype, out, ("mode", "valid"))
        r = self._x0_row()
        dev = torch.device("cuda", self.device)
        inner = {"x_nom": (r,), "u_nom": (4,), "K": (4, r), "du": (4,), "Vx": (r,), "y": (4,),
                 "mode": ()}
        po, res = capi.PlanOut(), {}
        for k in names:
            if k == "valid":
                continue
            shape, dt = (n, W, *inner[k]), (torch.int32 if k == "mode" else dtype)
            res[k] = out[k] if k in out else torch.empty(shape, dtype=dt, device=dev)
            ptr, ld = self._device_block(res[k], shape, dt, k)
            setattr(po, k, ptr)
            setattr(po, "ld_" + k, ld)
        res["valid"] = out["valid"] if "valid" in out else torch.empty((n,), dtype=torch.int32, device=dev)
        po.valid, _ = self._device_block(res["valid"], (n,), torch.int32, "valid")
        if n > 1 and res["valid"].stride(0) != 1:
            raise ValueError("valid must be contiguous")
        ms = ctypes.c_float(0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        capi.check(capi.lib().mhpc_export_plan_device(
            self._h, n, capi.iptr(lst), capi.iptr(fs), W, ctypes.byref(po),
            capi.MHPC_DEV_F32 if dtype == torch.float32 else capi.MHPC_DEV_F64, stream,
            ctypes.byref(ms)), "mhpc_export_plan_device")
        self.last_export_ms = ms.value
        return res

    def export_results(self, problems=None, want=("J", "viol", "status"), dtype=None,
                       out=None) -> dict:
        """The listed problems' results of their last solve into torch tensors on the handle's
        device (mhpc_export_results_device): "J", "dV_exp", "viol" [n], "V_phase", "dV_phase"
        [n][max_phases()] (zero past a problem's own phases) of dtype, as get_scalars reports
        them, and "status" [n] int32 as solve_mhpc returns it.  out: {name: tensor}, contiguous."""
        import ctypes
        import torch
        kinds = ("J", "dV_exp", "viol", "V_phase", "dV_phase", "status")
        out = dict(out or {})
        names = list(dict.fromkeys([*want, *out]))
        if not names or any(k not in kinds for k in names):
            raise ValueError('want: some of "J", "dV_exp", "viol", "V_phase", "dV_phase", "status"')
        lst, n = self._export_list(problems)
        dtype = self._export_dtype(dtype, out, ("status",))
        dev = torch.device("cuda", self.device)
        P = self.max_phases()
        ro, res = capi.ResultsOut(), {}
        for k in names:
            shape = (n, P) if k in ("V_phase", "dV_phase") else (n,)
            dt = torch.int32 if k == "status" else dtype
            res[k] = out[k] if k in out else torch.empty(shape, dtype=dt, device=dev)
            ptr, _ = self._device_block(res[k], shape, dt, k)
            if not res[k].is_contiguous():
                raise ValueError(f"{k} must be contiguous")
            setattr(ro, k, ptr)
        stream = torch.cuda.current_stream(dev).cuda_stream
        capi.check(capi.lib().mhpc_export_results_device(
            self._h, n, capi.iptr(lst), ctypes.byref(ro),
            capi.MHPC_DEV_F32 if dtype == torch.float32 else capi.MHPC_DEV_F64, stream),
            "mhpc_export_results_device")
        return res

    # -- device-resident plan import: warm-start listed problems from tensors --------------------
    @staticmethod
    def _scope_code(scope):
        codes = {"control": capi.MHPC_STEPS_CONTROL, "all": capi.MHPC_STEPS_ALL}
        if scope not in codes:
            raise ValueError('scope must be "control" or "all"')
        return codes[scope]

    def num_plan_steps(self, b: int = 0, scope="control") -> int:
        """Steps of problem b under a scope (mhpc_num_plan_steps): "control" the control steps of
        num_control_steps, "all" every phase in order, N[p] - 1 steps a phase."""
        import ctypes
        n = ctypes.c_int(0)
        capi.check(capi.lib().mhpc_num_plan_steps(self._h, int(b), self._scope_code(scope),
                                                  ctypes.byref(n)), "mhpc_num_plan_steps")
        return n.value

    def import_plan(self, problems=None, first_step=0, u_nom=None, K=None, x_nom=None,
                    scope="control"):
        """Start the listed problems from a guess: u_nom [n][W][4] overwrites the nominal controls
        of problems[i] (None: the whole batch in order) at steps first_step (an int, or one per
        listed problem) .. first_step + W - 1 of the scope's step map; with K [n][W][4][r] and
        x_nom [n][W][r] (both or neither) the gains and the nominal states they refer to as well,
        without them the written knots' gains become +0 (an open-loop guess).  Rows past a
        problem's steps and columns past a step's state size are ignored.  The next solve or tick
        of the listed problems starts with the real rollout of the guess from x0, as after
        update_problem(); nothing else changes.  scope "control": the steps of control() and
        export_plan(), so an exported window goes back as it is; "all": every phase in order (6
        columns in an SRB phase).  The arrays: torch tensors on the handle's device, float32 or
        float64 alike, inner-contiguous views with any leading stride >= the block
        (mhpc_import_plan_device, on the current torch stream's order; values are not inspected),
        or numpy arrays (mhpc_import_plan; non-finite entries are refused).  The device time of a
        tensor import is left in self.last_import_ms."""
        import ctypes
        code = self._scope_code(scope)
        if u_nom is None:
            raise ValueError("u_nom is required")
        if (K is None) != (x_nom is None):
            raise ValueError("K and x_nom go together: the gains act on x - x_nom")
        lst, n = self._export_list(problems)
        given = {"u_nom": u_nom, "K": K, "x_nom": x_nom}
        given = {k: v for k, v in given.items() if v is not None}
        if u_nom.ndim != 3:
            raise ValueError("u_nom must be [n][W][4]")
        W = int(u_nom.shape[1])
        if W < 1 or W > capi.MHPC_MAX_KNOTS:
            raise ValueError("window must be 1..MHPC_MAX_KNOTS")
        fs = np.asarray(first_step)
        if not np.issubdtype(fs.dtype, np.integer) or fs.ndim > 1:
            raise ValueError("first_step must be an int or one int per listed problem")
        fs = np.full(n, int(fs)) if fs.ndim == 0 else fs
        if fs.shape != (n,):
            raise ValueError("first_step must be an int or one int per listed problem")
        fs = np.ascontiguousarray(fs, dtype=np.int32) if fs.any() else None  # (None: step 0)
        r = self._x0_row()
        shapes = {"u_nom": (n, W, 4), "K": (n, W, 4, r), "x_nom": (n, W, r)}
        L = capi.lib()
        if all(isinstance(v, np.ndarray) for v in given.values()):
            host = {}
            for k, v in given.items():
                if v.shape != shapes[k]:
                    raise ValueError(f"{k} must be {list(shapes[k])}")
                host[k] = np.ascontiguousarray(v, dtype=np.float64)
            capi.check(L.mhpc_import_plan(self._h, n, capi.iptr(lst), capi.iptr(fs), W, code,
                                          capi.dptr(host["u_nom"]), capi.dptr(host.get("K")),
                                          capi.dptr(host.get("x_nom"))), "mhpc_import_plan")
            return
        import torch
        if not isinstance(u_nom, torch.Tensor):
            raise ValueError("u_nom, K and x_nom must be all torch tensors or all numpy arrays")
        if u_nom.dtype not in (torch.float32, torch.float64):
            raise ValueError("u_nom must be float32 or float64")
        pi = capi.PlanIn()
        for k, v in given.items():
            ptr, ld = self._device_block(v, shapes[k], u_nom.dtype, k)
            setattr(pi, k, ptr)
            setattr(pi, "ld_" + k, ld)
        ms = ctypes.c_float(0)
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        capi.check(L.mhpc_import_plan_device(
            self._h, n, capi.iptr(lst), capi.iptr(fs), W, code, ctypes.byref(pi),
            capi.MHPC_DEV_F32 if u_nom.dtype == torch.float32 else capi.MHPC_DEV_F64, stream,
            ctypes.byref(ms)), "mhpc_import_plan_device")
        self.last_import_ms = ms.value

    def get_x0(self) -> np.ndarray:
        """The device's current initial states [batch][r] (mhpc_get_x0)."""
        x0 = np.zeros((self.batch, self._x0_row()))
        capi.check(capi.lib().mhpc_get_x0(self._h, capi.dptr(x0)), "mhpc_get_x0")
        return x0

    def set_profiling(self, on: bool = True):
        capi.check(capi.lib().mhpc_set_profiling(self._h, 1 if on else 0), "mhpc_set_profiling")

    def kernel_stats(self) -> dict:
        n = capi.MHPC_NUM_KERNELS
        ms, nl, by = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n)
        capi.check(capi.lib().mhpc_get_kernel_stats(
            self._h, capi.dptr(ms), nl.ctypes.data_as(__import__("ctypes").POINTER(
                __import__("ctypes").c_int64)), capi.dptr(by)), "mhpc_get_kernel_stats")
        fl = np.zeros(n)
        capi.check(capi.lib().mhpc_get_kernel_flops(self._h, capi.dptr(fl)), "mhpc_get_kernel_flops")
        return {capi.lib().mhpc_kernel_name(k).decode(): {"ms": float(ms[k]), "launches": int(nl[k]),
                                                          "alg_bytes": float(by[k]),
                                                          "alg_flops": float(fl[k])}
                for k in range(n)}

    def reset_kernel_stats(self):
        capi.check(capi.lib().mhpc_reset_kernel_stats(self._h), "mhpc_reset_kernel_stats")

    def set_kernel_variant(self, bws: str = "auto", rollout: str = "auto", overlap: str = "auto",
                           sub_batches: int = 0, ro_store: int = 0, sweep_bits: int = 0,
                           snap_round: Optional[int] = None):
        """Pin the backward-sweep / line-search launch variant, the partials / sweep
        overlap, the number of concurrently scheduled sub-batches and the number of
        line-search trials that store their knot records (mhpc_set_kernel_variant); names in
        capi.BWS_VARIANTS / capi.RO_VARIANTS / capi.OVERLAP_VARIANTS, "auto" / 0 = chosen by
        batch size and phase layout (ro_store 0: the default).  sweep_bits: arithmetic of the
        backward sweep, 0 / 64 double (default), 32 float (fp32 handles only).  snap_round:
        problems a round of snapshot_problems / restore_problems (0: by the staging cap; None:
        unchanged)."""
        L = capi.lib()
        if snap_round is not None:
            capi.check(L.mhpc_set_kernel_variant(self._h, capi.MHPC_VARIANT_SNAP_ROUND,
                                                 int(snap_round)), "mhpc_set_kernel_variant")
        if sweep_bits or getattr(self, "_sweep_bits_pinned", False):
            capi.check(L.mhpc_set_kernel_variant(self._h, capi.MHPC_VARIANT_SWEEP_BITS,
                                                 int(sweep_bits)), "mhpc_set_kernel_variant")
            self._sweep_bits_pinned = bool(sweep_bits)
        if ro_store or getattr(self, "_ro_store_pinned", False):
            capi.check(L.mhpc_set_kernel_variant(self._h, capi.MHPC_VARIANT_RO_STORE, int(ro_store)),
                       "mhpc_set_kernel_variant")
            self._ro_store_pinned = bool(ro_store)
        capi.check(L.mhpc_set_kernel_variant(self._h, capi.MHPC_VARIANT_SUBBATCH, int(sub_batches)),
                   "mhpc_set_kernel_variant")
        capi.check(L.mhpc_set_kernel_variant(self._h, capi.MHPC_VARIANT_OVERLAP,
                                             capi.OVERLAP_VARIANTS[overlap]), "mhpc_set_kernel_variant")
        capi.check(L.mhpc_set_kernel_variant(self._h, capi.MHPC_VARIANT_BWS,
                                             capi.BWS_VARIANTS[bws]), "mhpc_set_kernel_variant")
        capi.check(L.mhpc_set_kernel_variant(self._h, capi.MHPC_VARIANT_RO,
                                             capi.RO_VARIANTS[rollout]), "mhpc_set_kernel_variant")

    def concatenated(self) -> dict:
        """Phase-concatenated per-problem arrays (the oracle's layout)."""
        parts = [self.get_phase(p) for p in range(self.desc.n_phases)]
        B = self.batch
        return {
            "X": np.concatenate([q["x"].reshape(B, -1) for q in parts], axis=1),
            "U": np.concatenate([q["u"].reshape(B, -1) for q in parts], axis=1),
            "Y": np.concatenate([q["y"].reshape(B, -1) for q in parts], axis=1),
            "K": np.concatenate([q["K"].reshape(B, -1) for q in parts], axis=1),
            "DU": np.concatenate([q["du"].reshape(B, -1) for q in parts], axis=1),
            "G": np.concatenate([q["Vx"].reshape(B, -1) for q in parts], axis=1),
        }

    def get_cost_gradients(self, p: int) -> dict:
        """lx [batch][N-1][n] and Phix [batch][n] of phase p as the last partials evaluation
        left them (the reference's rcost[k].lx / tcost.Phix, written to cost.txt)."""
        n = self.desc.xsize(p)
        N = self.desc.N[p]
        lx = np.zeros((self.batch, N - 1, n))
        phix = np.zeros((self.batch, n))
        capi.check(capi.lib().mhpc_get_cost_gradients(self._h, p, capi.dptr(lx), capi.dptr(phix)),
                   "mhpc_get_cost_gradients")
        return {"lx": lx, "Phix": phix}

    def print_debugInfo(self, dirname: str = ".", problem: int = 0, verbose: bool = True):
        """MHPCLocomotion::print_debugInfo (MHPCLocomotion.cpp:293-380) for one problem:
        state.txt, control.txt, gradient.txt, cost.txt in Eigen's default row format
        (eigen_row), with the reference's row counts -- including its N_TIMESTEPS[i+2]
        indexing of the SRB phases in control / gradient / cost (exact for n_wbphase = 2;
        rows past an SRB phase's own N are the zero-initialised buffer)."""
        os.makedirs(dirname, exist_ok=True)
        d = self.desc
        nwb, nfb, P = d.n_wb, d.n_fb, d.n_phases
        parts = [self.get_phase(p) for p in range(P)]
        grads = [self.get_cost_gradients(p) for p in range(P)]
        Ns = [d.N[p] for p in range(P)]

        def n_rows(i):  # N_TIMESTEPS[i+2] (clamped where the reference would read past it)
            return Ns[i + 2] if i + 2 < P else Ns[nwb + i]

        def rows(arr, n_want, width):
            out = [np.ravel(arr[k]) if k < len(arr) else np.zeros(width) for k in range(n_want)]
            return out

        def write(fname, blocks):
            if verbose:
                print(f"********** Write to file {fname} ************")
            with open(os.path.join(dirname, fname), "w") as f:
                for blk in blocks:
                    for r in blk:
                        f.write(eigen_row(r) + "\n")

        st, ct, gr, co = [], [], [], []
        for i in range(nwb):
            q, g = parts[i], grads[i]
            st.append(rows(q["x"][problem], Ns[i], 14))
            ct.append(rows(q["u"][problem], Ns[i], 4))
            gr.append(rows(q["Vx"][problem], Ns[i], 14))
            co.append(rows(g["lx"][problem], Ns[i] - 1, 14) + [g["Phix"][problem]])
        for i in range(nfb):
            q, g = parts[nwb + i], grads[nwb + i]
            st.append(rows(q["x"][problem], Ns[nwb + i], 6))
            ct.append(rows(q["u"][problem], n_rows(i), 4))
            gr.append(rows(q["Vx"][problem], n_rows(i), 6))
            co.append(rows(g["lx"][problem], n_rows(i) - 1, 6) + [g["Phix"][problem]])
        write("state.txt", st)
        write("control.txt", ct)
        write("gradient.txt", gr)
        write("cost.txt", co)
