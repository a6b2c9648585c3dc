"""Geometry optimisation that stays on the GPU: a batched FIRE minimiser and a batched L-BFGS minimiser (``LBFGS``)
next to the whole-step graphs of runtime.py.

``FIRE`` lives next to a ``runtime.GraphedStep`` (a batch of open-boundary molecules, ``ptr``) or a ``runtime.GraphedStepPBC`` (one periodic
box with a fixed cell, ``cell``) exactly as ``md.Dynamics`` does, and one iteration is

    xeq_fire_front  (v = c_v v + c_f f, x += d v, wrap: writes the step object's static ``pos``)
    the step's graph, replayed on its static buffers
    xeq_fire_back   (per-graph P, ff, vv, fmax in a fixed order; the graph's FIRE state machine; counters; trajectory rows)

enqueued on the current stream with no host synchronisation.  EVERY GRAPH IS ITS OWN FIRE SYSTEM -- its own time step, mixing factor,
positive-power counter and convergence flag -- where ASE's ``optimize.FIRE`` (which the arithmetic restates; masses are not used) treats
the whole ``Atoms`` as one; a converged graph is frozen bit for bit while the others go on.  Every ``check_every`` iterations the host
reads four integers back and stops at the first check that finds no active graph.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional

import numpy as np
import torch

from . import keys, lib
from .lib import call
from .resident import ResidentDriver
from .utils import units as _units


def time_step_factor(energy_unit: str, length_unit: str) -> float:
    """sqrt(k), k = (eV / Angstrom per force unit) (length unit per Angstrom): ``dt`` and ``dtmax`` are given for eV and Angstrom as ASE
    gives them, a move is x += dt^2 f and the mixing is scale-free, so in other units the two are scaled by this once and the kernels
    see no unit."""
    e_ev = _units.eval_unit(energy_unit) / _units.eval_unit("eV")               # one energy unit in eV
    l_a = _units.eval_unit(length_unit) / _units.eval_unit("Angstrom")          # one length unit in Angstrom
    return math.sqrt((e_ev / l_a) * (1.0 / l_a))


class _Minimiser(ResidentDriver):
    """What the two minimisers share beyond ResidentDriver: the set-up of the system and of the state both keep, the run loop over
    windows, the lazy evaluation 0 and the read-only surface.  A subclass sets ``_CONVERGED`` (its status value of a converged graph),
    validates its own parameters, calls ``_init_minimiser``, allocates its own state (``vel``, ``_partial``, ``_partial_bad`` among it),
    calls ``_load_system``, fills its record and defines ``reset()``."""

    _CONVERGED = None

    def _init_minimiser(self, model, pos: torch.Tensor, atomic_numbers: torch.Tensor, ptr, cell, fixed, edge_capacity, energy_unit, length_unit,
                        fresh: int) -> None:
        """The shape checks, ``_init_system``, the units and the state every minimiser has, every graph at status ``fresh``."""
        who = type(self).__name__
        N = int(pos.shape[0])
        if pos.dim() != 2 or pos.shape[1] != 3 or atomic_numbers.shape != (N,):
            raise ValueError(f"{who}: pos [N, 3] and atomic_numbers [N] are needed")
        if fixed is not None and fixed.shape != (N,):
            raise ValueError(f"{who}: fixed {tuple(fixed.shape)}, [N] = [{N}] is needed")
        self._init_system(model, N, ptr, cell, edge_capacity, (pos, atomic_numbers, ptr, cell, fixed))
        dev, dt_, G = self.device, self.dtype, self.n_graphs
        u = _units.get_default_units()
        self.energy_unit = energy_unit or u.get(keys.TOTAL_ENERGY, "eV")
        self.length_unit = length_unit or u.get(keys.POSITIONS, "Angstrom")
        self.fixed = None if fixed is None else fixed.detach().to(torch.bool).contiguous().clone()
        self.frc = torch.zeros((N, 3), dtype=dt_, device=dev)          # f of the latest evaluation
        self.image = torch.zeros((N, 3), dtype=torch.int32, device=dev)
        self.epot = torch.zeros(G, dtype=dt_, device=dev)
        self.fmax = torch.zeros(G, dtype=dt_, device=dev)
        self.status = torch.full((G,), fresh, dtype=torch.int32, device=dev)
        self._converged_at = torch.full((G,), -1, dtype=torch.int64, device=dev)
        self.book = torch.zeros(4, dtype=torch.int64, device=dev)     # evaluations done, largest n_edges, non-finite flag, graphs not converged
        self._ck = None
        self._steps_host = 0           # evaluations done
        self._active_host = G
        self._fresh = False            # frc / epot / fmax and the driver's coefficients belong to the current positions

    def _reset_common(self, fresh: int) -> None:
        """The tail of every ``reset()``: every graph at status ``fresh``, the evaluation count starts over."""
        self.status.fill_(fresh)
        self._converged_at.fill_(-1)
        self.book.zero_()
        self._steps_host, self._active_host, self._fresh = 0, self.n_graphs, False

    def _bad_message(self, first: int, n: int) -> str:
        return (f"{type(self).__name__}: non-finite force or energy in evaluations {first} .. {first + n}; the state is that "
                + (f"behind evaluation {first - 1}" if first else "of the start"))

    def _window(self, n: int) -> None:
        super()._window(n)
        self._active_host = self._book_extra

    # ------------------------------------------------------------------------------------------------ public
    def run(self, max_steps: int, check_every: int = 20, record_every: int = 0) -> bool:
        """At most ``max_steps`` iterations in windows of ``check_every``; True when every graph has converged.  With ``record_every`` the
        state behind every ``record_every``-th evaluation of this run goes to ``trajectory`` (pos, epot, fmax, step; rows the run did not
        reach stay zero)."""
        max_steps, check_every, record_every = int(max_steps), max(1, int(check_every)), max(0, int(record_every))
        if max_steps < 0:
            raise ValueError(f"{type(self).__name__}.run: max_steps < 0")
        self._record_run(max_steps, record_every, "fmax", self.step_count)
        if not self._fresh:
            self._window(0)            # evaluation 0: a start that is already relaxed moves nothing
        done = 0
        while done < max_steps and self._active_host > 0:
            w = min(check_every, max_steps - done)
            self._window(w)
            done += w
        return self._active_host == 0

    def _settle(self) -> None:
        if not self._fresh:
            self._window(0)

    @property
    def step_count(self) -> int:
        """Iterations done: the number of the latest evaluation (the first one is 0)."""
        return max(self._steps_host - 1, 0)

    @property
    def forces(self) -> torch.Tensor:
        self._settle()
        return self.frc.clone()

    @property
    def potential_energy(self) -> torch.Tensor:
        self._settle()
        return self.epot.clone()

    @property
    def max_force(self) -> torch.Tensor:
        self._settle()
        return self.fmax.clone()

    @property
    def converged(self) -> torch.Tensor:
        self._settle()
        return self.status == self._CONVERGED

    @property
    def converged_at(self) -> torch.Tensor:
        self._settle()
        return self._converged_at.clone()


class FIRE(_Minimiser):
    """``FIRE(model, pos, atomic_numbers, ptr=... | cell=..., fmax=...)``: see the module text and DESIGN.md section 13.  ``fixed``: bool [N],
    atoms that never move.  ``fmax`` in the model's force unit, ``maxstep`` in its length unit, ``dt`` / ``dtmax`` as ASE gives them."""

    _CONVERGED = lib.FIRE_CONVERGED

    def __init__(self, model, pos: torch.Tensor, atomic_numbers: torch.Tensor, *, ptr: Optional[torch.Tensor] = None, cell: Optional[torch.Tensor] = None,
                 pbc=None, fixed: Optional[torch.Tensor] = None, fmax: float, dt: float = 0.1, maxstep: float = 0.2, dtmax: float = 1.0, n_min: int = 5,
                 f_inc: float = 1.1, f_dec: float = 0.5, alpha_start: float = 0.1, f_alpha: float = 0.99, edge_capacity: Optional[int] = None,
                 energy_unit: Optional[str] = None, length_unit: Optional[str] = None) -> None:
        for name, v in (("fmax", fmax), ("dt", dt), ("dtmax", dtmax), ("maxstep", maxstep)):
            if not (math.isfinite(float(v)) and float(v) > 0.0):
                raise ValueError(f"FIRE: {name} {v} (> 0 is needed)")
        if not 0.0 < float(f_dec) < 1.0:
            raise ValueError(f"FIRE: f_dec {f_dec} (inside (0, 1))")
        if not (math.isfinite(float(f_inc)) and float(f_inc) >= 1.0):
            raise ValueError(f"FIRE: f_inc {f_inc} (>= 1)")
        if not (0.0 <= float(alpha_start) <= 1.0 and 0.0 < float(f_alpha) <= 1.0 and int(n_min) >= 0):
            raise ValueError(f"FIRE: alpha_start {alpha_start} (in [0, 1]), f_alpha {f_alpha} (in (0, 1]), n_min {n_min} (>= 0)")
        self._init_minimiser(model, pos, atomic_numbers, ptr, cell, fixed, edge_capacity, energy_unit, length_unit, lib.FIRE_FRESH)
        N, G, C, dev = self.n_atoms, self.n_graphs, max(self.n_chunks, 1), self.device
        scale = time_step_factor(self.energy_unit, self.length_unit)
        self.fmax_tol, self.maxstep = float(fmax), float(maxstep)
        self.dt0, self.dtmax = float(dt) * scale, float(dtmax) * scale
        self.n_min, self.f_inc, self.f_dec, self.alpha_start, self.f_alpha = int(n_min), float(f_inc), float(f_dec), float(alpha_start), float(f_alpha)

        self._partial = torch.zeros((C, 4), dtype=torch.float64, device=dev)
        self._partial_bad = torch.zeros(C, dtype=torch.int32, device=dev)
        self.vel = torch.zeros((N, 3), dtype=self.dtype, device=dev)
        self.dt = torch.full((G,), self.dt0, dtype=torch.float64, device=dev)
        self.alpha = torch.full((G,), self.alpha_start, dtype=torch.float64, device=dev)
        self.n_pos = torch.zeros(G, dtype=torch.int32, device=dev)
        self.coef = torch.zeros((G, 3), dtype=torch.float64, device=dev)
        self._front_name, self._back_name = "xeq_fire_front", "xeq_fire_back"

        self._load_system(pos, atomic_numbers, cell, pbc)
        self._fire = lib.fill(lib.FireParams(), fixed=self.fixed, epot=self.epot, fmax=self.fmax, dt=self.dt, alpha=self.alpha, n_pos=self.n_pos,
                              status=self.status, converged_at=self._converged_at, coef=self.coef, fmax_tol=self.fmax_tol, maxstep=self.maxstep,
                              dtmax=self.dtmax, n_min=self.n_min, f_inc=self.f_inc, f_dec=self.f_dec, alpha_start=self.alpha_start, f_alpha=self.f_alpha)
        if self._any_pbc:              # the wrap alone (c_v = c_f = d = 0 on zero velocities and forces): the search sweeps images around the box
            every = torch.full((G,), lib.FIRE_ACTIVE, dtype=torch.int32, device=dev)
            call("xeq_fire_front", ctypes.byref(self._sys), ctypes.byref(lib.fill(lib.FireParams(), status=every, coef=self.coef)), lib.stream())

    # ------------------------------------------------------------------------------------------------ launches
    def _front_args(self):
        return (ctypes.byref(self._sys), ctypes.byref(self._fire))

    def _back_args(self, advance: bool):
        return (ctypes.byref(self._sys), ctypes.byref(self._step_record()), ctypes.byref(self._chunks), ctypes.byref(self._fire), ctypes.byref(self._rec))
    # ------------------------------------------------------------------------------------------------ check / restore (resident.py)
    def _state(self):
        return [self._pos, self.image, self.vel, self.frc, self.epot, self.fmax, self.dt, self.alpha, self.n_pos, self.status, self._converged_at,
                self.coef, self.book]

    def reset(self) -> None:
        """Every graph fresh and active again, v = 0, from the current positions; the evaluation count starts over."""
        self.vel.zero_()
        self.dt.fill_(self.dt0)
        self.alpha.fill_(self.alpha_start)
        self.n_pos.zero_()
        self.coef.zero_()
        self._reset_common(lib.FIRE_FRESH)

    @property
    def time_steps(self) -> torch.Tensor:
        return self.dt.clone()


def curvature_factor(energy_unit: str, length_unit: str) -> float:
    """(energy unit / length unit^2) per (eV / Angstrom^2): ``alpha`` of ``LBFGS`` is given in eV / Angstrom^2 as ASE gives it and is
    multiplied by this once, so the kernels see no unit."""
    e_ev = _units.eval_unit(energy_unit) / _units.eval_unit("eV")               # one energy unit in eV
    l_a = _units.eval_unit(length_unit) / _units.eval_unit("Angstrom")          # one length unit in Angstrom
    return (l_a * l_a) / e_ev


class LBFGS(_Minimiser):
    """``LBFGS(model, pos, atomic_numbers, ptr=... | cell=..., fmax=...)``: limited-memory BFGS without line search, ASE's
    ``optimize.LBFGS`` rule, EVERY GRAPH ITS OWN MINIMISER (its own history, step clamp and convergence flag; a converged graph is frozen
    bit for bit).  One iteration is xeq_lbfgs_front (direction from the coefficients, clamp, move, wrap), the step's graph, xeq_lbfgs_back
    (the new pair, three rows of the per-graph Gram matrix, the two-loop recursion in coefficient space): include/xeq.h has the arithmetic,
    DESIGN.md section 16 the reasons.  ``fmax`` in the model's force unit, ``maxstep`` in its length unit, ``alpha`` in eV / Angstrom^2
    as ASE gives it, ``memory`` pairs (1 .. 32).  ``fixed``: bool [N], atoms that never move.  There is no CPU fallback."""

    _CONVERGED = lib.LBFGS_CONVERGED

    def __init__(self, model, pos: torch.Tensor, atomic_numbers: torch.Tensor, *, ptr: Optional[torch.Tensor] = None, cell: Optional[torch.Tensor] = None,
                 pbc=None, fixed: Optional[torch.Tensor] = None, fmax: float, memory: int = 16, alpha: float = 70.0, maxstep: float = 0.2,
                 damping: float = 1.0, edge_capacity: Optional[int] = None, energy_unit: Optional[str] = None,
                 length_unit: Optional[str] = None) -> None:
        for name, v in (("fmax", fmax), ("alpha", alpha), ("maxstep", maxstep), ("damping", damping)):
            if not (math.isfinite(float(v)) and float(v) > 0.0):
                raise ValueError(f"LBFGS: {name} {v} (> 0 is needed)")
        if int(memory) != memory or not 1 <= int(memory) <= lib.LBFGS_MAX_MEMORY:
            raise ValueError(f"LBFGS: memory {memory} (1 .. {lib.LBFGS_MAX_MEMORY})")
        self._init_minimiser(model, pos, atomic_numbers, ptr, cell, fixed, edge_capacity, energy_unit, length_unit, lib.LBFGS_FRESH)
        N, G, C, M, dev = self.n_atoms, self.n_graphs, max(self.n_chunks, 1), int(memory), self.device
        self.fmax_tol, self.maxstep, self.damping, self.memory = float(fmax), float(maxstep), float(damping), M
        self.alpha = float(alpha) * curvature_factor(self.energy_unit, self.length_unit)

        K = 2 * M + 1
        self._max_graph_chunks = int(np.diff(self._graph_chunk_ptr.cpu().numpy()).max()) if G else 0
        f64 = dict(dtype=torch.float64, device=dev)
        self._partial = torch.zeros((C, 3 * (2 * M + 3) + 1), **f64)
        self._partial_bad = torch.zeros((C, 4), dtype=torch.int32, device=dev)
        self.vel = None                # (no velocities: the record's member stays NULL; frc is f_prev of the next back)
        self.hist_s = torch.zeros((M, N, 3), **f64)
        self.hist_y = torch.zeros((M, N, 3), **f64)
        self.pending_s = torch.zeros((N, 3), **f64)
        self.gram = torch.zeros((G, K, K), **f64)
        self.delta = torch.zeros((G, K), **f64)
        self.count = torch.zeros(G, dtype=torch.int32, device=dev)
        self.head = torch.zeros(G, dtype=torch.int32, device=dev)
        self.dropped = torch.zeros(G, dtype=torch.int32, device=dev)
        self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self._front_name, self._back_name = "xeq_lbfgs_front", "xeq_lbfgs_back"

        self._load_system(pos, atomic_numbers, cell, pbc)
        members = dict(fixed=self.fixed, hist_s=self.hist_s, hist_y=self.hist_y, pending_s=self.pending_s, gram=self.gram, delta=self.delta,
                       count=self.count, head=self.head, status=self.status, dropped=self.dropped, converged_at=self._converged_at, epot=self.epot,
                       fmax=self.fmax, ticket=self._ticket, memory=self.memory, max_graph_chunks=self._max_graph_chunks, fmax_tol=self.fmax_tol,
                       alpha=self.alpha, maxstep=self.maxstep, damping=self.damping)
        self._lbfgs = lib.fill(lib.LbfgsParams(), **members)
        if self._any_pbc:              # the wrap alone (every coefficient and force is zero): the search sweeps images around the box
            every = torch.full((G,), lib.LBFGS_ACTIVE, dtype=torch.int32, device=dev)
            call("xeq_lbfgs_front", ctypes.byref(self._sys), ctypes.byref(self._chunks),
                 ctypes.byref(lib.fill(lib.LbfgsParams(), **dict(members, status=every))), lib.stream())

    # ------------------------------------------------------------------------------------------------ launches
    def _front_args(self):
        return (ctypes.byref(self._sys), ctypes.byref(self._chunks), ctypes.byref(self._lbfgs))

    def _back_args(self, advance: bool):
        return (ctypes.byref(self._sys), ctypes.byref(self._step_record()), ctypes.byref(self._chunks), ctypes.byref(self._lbfgs), ctypes.byref(self._rec))

    # ------------------------------------------------------------------------------------------------ check / restore (resident.py)
    def _state(self):
        return [self._pos, self.image, self.frc, self.hist_s, self.hist_y, self.pending_s, self.gram, self.delta, self.count, self.head,
                self.status, self.dropped, self._converged_at, self.epot, self.fmax, self.book]

    def reset(self) -> None:
        """Every graph fresh again with an empty history, from the current positions; the evaluation count starts over."""
        for t in (self.hist_s, self.hist_y, self.pending_s, self.gram, self.delta, self.count, self.head, self.dropped):
            t.zero_()
        self._reset_common(lib.LBFGS_FRESH)

    @property
    def history_length(self) -> torch.Tensor:
        """Pairs each graph's ring holds, [G]."""
        return self.count.clone()

    @property
    def dropped_pairs(self) -> torch.Tensor:
        """Pairs each graph rejected (s.y <= 0 or not finite), [G]."""
        return self.dropped.clone()


METHODS = {"fire": FIRE, "lbfgs": LBFGS}


def minimize(model, data: Dict[str, torch.Tensor], fmax: float, max_steps: int = 500, check_every: int = 20, method: str = "fire",
             **kw) -> Dict[str, torch.Tensor]:
    """``FIRE`` (``method="fire"``, the default) or ``LBFGS`` (``"lbfgs"``) on a data dict (``pos``, ``atomic_numbers``, ``ptr`` or
    ``cell`` [, ``pbc``]): -> ``pos``, ``energy`` [G], ``forces``, ``converged`` [G] and ``n_steps`` (iterations done)."""
    if method not in METHODS:
        raise ValueError(f"minimize: method {method!r} (one of {sorted(METHODS)})")
    cell = data.get(keys.CELL)
    opt = METHODS[method](model, data[keys.POSITIONS], data[keys.ATOMIC_NUMBERS], ptr=None if cell is not None else data.get("ptr"), cell=cell,
                          pbc=data.get(keys.PBC) if cell is not None else None, fmax=fmax, **kw)
    opt.run(max_steps, check_every=check_every)
    return {"pos": opt.positions, "energy": opt.potential_energy, "forces": opt.forces, "converged": opt.converged, "n_steps": opt.step_count}
