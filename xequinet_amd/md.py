"""Molecular dynamics that stays on the GPU: an integrator next to the whole-step graphs of runtime.py.

``runtime.GraphedStep`` / ``GraphedStepPBC`` evaluate one MD step -- neighbour search, model, forces -- as one captured HIP graph, and every
consumer so far took the results back to the host once per step.  ``Dynamics`` is the consumer that does not: one MD step is

    xeq_md_front   (Berendsen scale, half kick, drift, Langevin O step, wrap: writes the step object's static ``pos``)
    the step's graph, replayed on its static buffers
    xeq_md_back    (half kick, per-graph kinetic energy, step counter / largest edge count / non-finite flag, trajectory rows)

enqueued on the current stream with no host synchronisation; every ``check_every`` steps the host reads three integers back.  The step's
own graph is REPLAYED between the two launches rather than captured again inside a larger graph: the step classes keep their capture logic
(weights that moved, a list that outgrew its capacity) and the two launches take arguments that change between runs (recorder rows)
without a re-capture.  Measured (profiles/md_timing.txt): with its arguments bound once per window the host needs 0.13 ms to enqueue an
aspirin step that takes the GPU 0.38 ms, and 0.02-0.03 ms for 1 024 molecules; one captured graph per MD step was tried and gave the
same device time and the same 0.13 ms, so it was not kept.

``ensemble="npt_berendsen"`` adds ASE's Berendsen barostat for one box periodic along all three axes.  The box then
lives on the device: the step is built with ``compute_virial=True, device_cell=True`` (its graph starts with the kernel that forms the cell
tables from the static cell), ``xeq_npt_back`` forms pressure, scale factor and the pending cell from the step's virial, ``xeq_npt_front``
applies them; a box that shrank until the cutoff reaches a further image voids the window as an outgrown edge capacity does (resident.py).

``ensemble="nose_hoover"`` and ``"bussi"`` are the canonical thermostats: a Nose-Hoover chain or a stochastic
velocity rescaling per graph, run in the back's join by the lane that holds the graph's kinetic energy (``xeq_nvt_back``) as ONE factor
per graph, which stays PENDING in the thermostat's row until the next front applies it (``xeq_nvt_front``): ``vel`` holds the velocities
before the factor, and ``velocities``, ``kinetic_energy`` and ``temperature`` are those behind it.

A batch of independent open-boundary molecules (``ptr``) runs on GraphedStep, one periodic box (``cell``) on GraphedStepPBC; the models
those classes refuse are refused here by constructing them.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional

import numpy as np
import torch

from . import keys, lib
from .lib import call, dtype_code, require_hip
from .resident import ResidentDriver, chunk_tables  # noqa: F401  (chunk_tables: part of this module's interface)
from .utils import units as _units

ENSEMBLES = {"nve": lib.MD_NVE, "langevin": lib.MD_LANGEVIN, "berendsen": lib.MD_BERENDSEN,
             "npt_berendsen": lib.MD_BERENDSEN}               # (its thermostat; the barostat has entries of its own: xeq_npt_front / _back)
NPT = "npt_berendsen"
# The canonical thermostats, served by entries of their own (xeq_nvt_front / _back): name -> XEQ_NVT_* kind.  (ENSEMBLES stays the map
# to the XEQ_MD_* codes of xeq_md_front.)
THERMOSTATS = {"nose_hoover": lib.NVT_NOSE_HOOVER, "bussi": lib.NVT_BUSSI}
PURPOSE_LANGEVIN, PURPOSE_MAXWELL = lib.MD_PURPOSE_LANGEVIN, lib.MD_PURPOSE_MAXWELL
BOLTZMANN_J_PER_K = 1.380649e-23                             # exact (SI 2019)


def unit_factors(energy_unit: str, length_unit: str) -> Dict[str, float]:
    """``accel``: (energy / length) / (g / mol) in length / fs^2; ``kB``: the Boltzmann constant in energy / K; ``GPa``: one GPa
    (1e9 J / m^3) in energy / length^3 -- from the constants of utils/units.py (the table holds every unit in atomic units) and k_B in
    J / K."""
    joule, metre = _units.eval_unit("J"), _units.eval_unit("m")
    e_j = _units.eval_unit(energy_unit) / joule                  # one energy unit in J
    l_m = _units.eval_unit(length_unit) / metre                  # one length unit in m
    kg_per_gmol = 1.0e-3 / _units.eval_unit("mol")               # one g / mol in kg
    fs = 1.0e-15
    return {"accel": e_j / (l_m * kg_per_gmol) * fs * fs / l_m, "kB": BOLTZMANN_J_PER_K / e_j, "GPa": 1.0e9 * l_m**3 / e_j}


def default_rng_id(ptr_host) -> np.ndarray:
    """int64 [N]: the atom's index within its graph in the low word, the graph's index in the high word."""
    ptr_host = np.asarray(ptr_host, dtype=np.int64)
    counts = np.diff(ptr_host)
    graph = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    return (np.arange(int(ptr_host[-1]), dtype=np.int64) - ptr_host[graph]) | (graph << 32)


def normals(seed: int, purpose: int, step: int, rng_id: torch.Tensor, dtype=torch.float32, want_words: bool = True):
    """(words uint32-as-int32 [n, 4] or None, normals [n, 3]) of the device generator (xeq_md_normals)."""
    require_hip(rng_id)
    rng_id = rng_id.to(torch.int64).contiguous()
    n = int(rng_id.numel())
    words = torch.empty((n, 4), dtype=torch.int32, device=rng_id.device) if want_words else None
    out = torch.empty((n, 3), dtype=dtype, device=rng_id.device)
    call("xeq_md_normals", dtype_code(out), int(seed) & (2**64 - 1), int(purpose), int(step), lib.ptr(rng_id), n, lib.ptr(words), lib.ptr(out), lib.stream())
    return words, out


class Dynamics(ResidentDriver):
    """``Dynamics(model, pos, atomic_numbers, masses, ptr=... | cell=..., timestep_fs=..., ensemble=...)``: see the module text and
    DESIGN.md section 12.  ``masses`` [N] in g / mol (0 or inf: a fixed atom); ``ensemble``: "nve" (velocity Verlet), "langevin" (BAOAB;
    ``temperature_K``, ``friction_per_fs``), "berendsen" (``temperature_K``, ``taut_fs``), "npt_berendsen" (one box periodic along all
    three axes; the Berendsen thermostat and ASE's NPTBerendsen barostat: ``temperature_K``, ``taut_fs``, ``pressure_GPa``, ``taup_fs``,
    ``compressibility_per_GPa``), "nose_hoover" (a Nose-Hoover chain per graph: ``temperature_K``, ``taut_fs``,
    ``chain_length`` 1 .. 8, default 3) and "bussi" (stochastic velocity rescaling per graph: ``temperature_K``, ``taut_fs``, ``seed``,
    ``graph_rng_id`` int64 [G] with a zero low word, default ``g << 32``); the two keep ``thermostat_energy`` and
    ``conserved_energy``.  The box of an NPT run lives on the device: ``cell``, ``volume``, ``pressure``
    and ``virial`` read it; ``min_images`` (three ints) captures the step's graph with more periodic images than the first cell needs."""

    def __init__(self, model, pos: torch.Tensor, atomic_numbers: torch.Tensor, masses: torch.Tensor, *, ptr: Optional[torch.Tensor] = None,
                 cell: Optional[torch.Tensor] = None, pbc=None, timestep_fs: float, ensemble: str = "nve", temperature_K: Optional[float] = None,
                 friction_per_fs: Optional[float] = None, taut_fs: Optional[float] = None, seed: int = 0, rng_id: Optional[torch.Tensor] = None,
                 edge_capacity: Optional[int] = None, energy_unit: Optional[str] = None, length_unit: Optional[str] = None,
                 pressure_GPa: Optional[float] = None, taup_fs: Optional[float] = None, compressibility_per_GPa: Optional[float] = None,
                 min_images=None, chain_length: Optional[int] = None, graph_rng_id: Optional[torch.Tensor] = None) -> None:
        if ensemble not in ENSEMBLES and ensemble not in THERMOSTATS:
            raise ValueError(f"Dynamics: ensemble {ensemble!r} (one of {sorted([*ENSEMBLES, *THERMOSTATS])})")
        self.ensemble = ensemble
        self.dt = float(timestep_fs)
        if not (math.isfinite(self.dt) and self.dt > 0.0):
            raise ValueError(f"Dynamics: timestep_fs {timestep_fs}")
        if ensemble != "nve" and (temperature_K is None or not temperature_K >= 0.0):
            raise ValueError(f"Dynamics: ensemble {ensemble!r} needs temperature_K >= 0")
        if ensemble == "langevin" and (friction_per_fs is None or not friction_per_fs >= 0.0):
            raise ValueError("Dynamics: ensemble 'langevin' needs friction_per_fs >= 0")
        if ensemble in ("berendsen", NPT, *THERMOSTATS) and (taut_fs is None or not taut_fs > 0.0):
            raise ValueError(f"Dynamics: ensemble {ensemble!r} needs taut_fs > 0")
        self._nvt = ensemble in THERMOSTATS
        if self._nvt and not (temperature_K > 0.0 and math.isfinite(temperature_K) and math.isfinite(taut_fs)):
            raise ValueError(f"Dynamics: ensemble {ensemble!r} needs a finite temperature_K > 0 and a finite taut_fs > 0")
        if ensemble == "nose_hoover":
            chain_length = 3 if chain_length is None else chain_length
            if int(chain_length) != chain_length or not 1 <= chain_length <= lib.NVT_MAX_CHAIN:
                raise ValueError(f"Dynamics: ensemble 'nose_hoover' needs 1 <= chain_length <= {lib.NVT_MAX_CHAIN} (got {chain_length})")
        elif chain_length is not None:
            raise ValueError(f"Dynamics: chain_length belongs to ensemble 'nose_hoover', not {ensemble!r}")
        if graph_rng_id is not None and ensemble != "bussi":
            raise ValueError(f"Dynamics: graph_rng_id belongs to ensemble 'bussi', not {ensemble!r}")
        self._npt = ensemble == NPT
        if self._npt:
            if ptr is not None or cell is None:
                raise ValueError("Dynamics: ensemble 'npt_berendsen' needs ONE periodic box: a cell and no ptr")
            open_axes = [] if pbc is None else [k for k, v in enumerate(pbc.tolist() if isinstance(pbc, torch.Tensor) else pbc) if not v]
            if open_axes:
                raise ValueError(f"Dynamics: ensemble 'npt_berendsen' needs all three axes periodic (pbc is open along {open_axes})")
            if taup_fs is None or not (taup_fs > 0.0 and math.isfinite(taup_fs)):
                raise ValueError("Dynamics: ensemble 'npt_berendsen' needs taup_fs > 0")
            if pressure_GPa is None or not math.isfinite(pressure_GPa):
                raise ValueError("Dynamics: ensemble 'npt_berendsen' needs a finite pressure_GPa")
            if compressibility_per_GPa is None or not (compressibility_per_GPa >= 0.0 and math.isfinite(compressibility_per_GPa)):
                raise ValueError("Dynamics: ensemble 'npt_berendsen' needs compressibility_per_GPa >= 0")
        elif not (pressure_GPa is None and taup_fs is None and compressibility_per_GPa is None and min_images is None):
            raise ValueError(f"Dynamics: pressure_GPa, taup_fs, compressibility_per_GPa and min_images belong to ensemble 'npt_berendsen', not {ensemble!r}")
        N = int(pos.shape[0])
        if pos.dim() != 2 or pos.shape[1] != 3 or atomic_numbers.shape != (N,) or masses.shape != (N,):
            raise ValueError("Dynamics: pos [N, 3], atomic_numbers [N] and masses [N] are needed")
        self._init_system(model, N, ptr, cell, edge_capacity, (pos, atomic_numbers, masses, ptr, cell, rng_id),
                          dict(compute_virial=True, device_cell=True, min_images=min_images) if self._npt else None)
        ptr_host, dev, dt_ = self.ptr_host, self.device, self.dtype

        u = _units.get_default_units()
        self.energy_unit = energy_unit or u.get(keys.TOTAL_ENERGY, "eV")
        self.length_unit = length_unit or u.get(keys.POSITIONS, "Angstrom")
        fac = unit_factors(self.energy_unit, self.length_unit)
        self.accel, self.kB = fac["accel"], fac["kB"]
        self.temperature_K = None if temperature_K is None else float(temperature_K)
        self.seed = int(seed) & (2**64 - 1)
        gamma = 0.0 if friction_per_fs is None else float(friction_per_fs)
        self._c1 = math.exp(-gamma * self.dt)
        self._noise2 = (1.0 - self._c1 * self._c1) * self.kB * (self.temperature_K or 0.0)
        self._dt_over_tau = 0.0 if taut_fs is None else self.dt / float(taut_fs)
        if self._npt:       # mu = 1 - kappa (P0 - P) with P in energy / length^3
            self._p_unit = 1.0 / fac["GPa"]
            self._p0 = float(pressure_GPa) * fac["GPa"]
            self._kappa = (self.dt / float(taup_fs)) * (float(compressibility_per_GPa) / fac["GPa"] / 3.0)

        m = masses.detach().double().cpu().numpy()
        free = np.isfinite(m) & (m > 0.0)
        safe = np.where(free, m, 1.0)
        self._mass_host = np.where(free, m, 0.0)
        on = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(t).to(dev)
        self.inv_mass = on(np.where(free, self.accel / safe, 0.0), dt_)
        self.half_mass = on(np.where(free, safe / (2.0 * self.accel), 0.0), dt_)
        n_free = np.add.reduceat(np.concatenate([free.astype(np.int64), [0]]), ptr_host[:-1])[: self.n_graphs] * (np.diff(ptr_host) > 0)
        self.n_free = n_free
        self.tfac = on(np.where(n_free > 0, 2.0 / (3.0 * np.maximum(n_free, 1) * self.kB), 0.0), dt_)
        self.rng_id = (on(default_rng_id(ptr_host), torch.int64) if rng_id is None else rng_id.detach().to(torch.int64).contiguous().clone())
        if self.rng_id.shape != (N,):
            raise ValueError("Dynamics: rng_id [N]")
        self._partial = torch.zeros(max(self.n_chunks, 1), dtype=torch.float64, device=dev)
        self._partial_bad = torch.zeros(max(self.n_chunks, 1), dtype=torch.int32, device=dev)

        G = self.n_graphs
        self.vel = torch.zeros((N, 3), dtype=dt_, device=dev)
        self.frc = torch.zeros((N, 3), dtype=dt_, device=dev)
        self.image = torch.zeros((N, 3), dtype=torch.int32, device=dev)
        self.ke = torch.zeros(G, dtype=dt_, device=dev)
        self.epot = torch.zeros(G, dtype=dt_, device=dev)
        self.book = torch.zeros(4, dtype=torch.int64, device=dev)     # steps done, largest n_edges, non-finite flag, (NPT) more images needed
        self._ck = None
        self._steps_host = 0
        self._fresh = False            # frc / ke / epot belong to the current positions and velocities
        self._ke_stale = False         # velocities were set since ke was formed
        self._no_edges = torch.zeros(1, dtype=torch.int32, device=dev)

        self._load_system(pos, atomic_numbers, cell, pbc)
        self._md = lib.fill(lib.MdParams(), ensemble=lib.MD_NVE if self._nvt else ENSEMBLES[ensemble], inv_mass=self.inv_mass, half_mass=self.half_mass, ke=self.ke, epot=self.epot,
                            tfac=self.tfac, rng_id=self.rng_id, seed=self.seed, c1=self._c1, noise2=self._noise2, dt_over_tau=self._dt_over_tau,
                            t0=self.temperature_K or 0.0, half_dt=0.5 * self.dt)
        self._own = (ctypes.byref(self._md),)          # the driver's own records, as both of its entries take them
        if self._npt:
            # the box record of include/xeq.h (XEQ_NPT_*): current = pending = the cell the step object holds, mu = 1
            c = (ctypes.c_double * 9)(*self._cell_c)
            inv = (ctypes.c_double * 9)()
            call("xeq_md_inverse_cell", c, inv)
            rec = np.zeros(lib.NPT_BOX)
            rec[lib.NPT_CELL : lib.NPT_CELL + 9] = rec[lib.NPT_CELL_NEXT : lib.NPT_CELL_NEXT + 9] = np.array(c)
            rec[lib.NPT_INV : lib.NPT_INV + 9] = rec[lib.NPT_INV_NEXT : lib.NPT_INV_NEXT + 9] = np.array(inv)
            rec[lib.NPT_MU] = 1.0
            self.box = on(rec, torch.float64)
            self.vir = torch.zeros(9, dtype=dt_, device=dev)
            self.reps_seen = torch.zeros(3, dtype=torch.int32, device=dev)
            self._npt_rec = lib.fill(lib.NptParams(), box=self.box, step_cell=self.step.cell, virial=self.vir, reps_seen=self.reps_seen,
                                     kappa=self._kappa, p0=self._p0, p_unit=self._p_unit)
            self._own += (ctypes.byref(self._npt_rec),)
        if self._nvt:
            # the thermostats' rows of include/xeq.h (XEQ_NVT_*): factor 1, everything else 0
            ids = (torch.arange(G, dtype=torch.int64, device=dev) << 32) if graph_rng_id is None else graph_rng_id.detach().to(torch.int64).contiguous().clone()
            if ids.shape != (G,) or bool((ids & 0xFFFFFFFF).ne(0).any()):
                raise ValueError("Dynamics: graph_rng_id [G] with a zero low word (the word numbers a step's blocks)")
            self.graph_rng_id = ids
            self.thermo = torch.zeros((G, lib.NVT_ROW), dtype=torch.float64, device=dev)
            self.thermo[:, lib.NVT_SCALE] = 1.0
            self._n_free_dev = on(n_free, torch.int64)
            self._nvt_rec = lib.fill(lib.NvtParams(), kind=THERMOSTATS[ensemble], state=self.thermo, n_free=self._n_free_dev, graph_rng_id=self.graph_rng_id,
                                     chain_length=int(chain_length or 0), kT=self.kB * self.temperature_K, tau=float(taut_fs), dt=self.dt)
            self._own += (ctypes.byref(self._nvt_rec),)
        # the kinetic energies alone (_back_ke): the back on the forces and energies this object holds, which depend on the positions alone
        self._own_step = lib.fill(lib.ResStep(), frc_step=self.frc, energy_step=self.epot, n_edges_step=self._no_edges,
                                  virial_step=self.vir if self._npt else None)
        self._front_name, self._back_name = (("xeq_npt_front", "xeq_npt_back") if self._npt else ("xeq_nvt_front", "xeq_nvt_back") if self._nvt else
                                             ("xeq_md_front", "xeq_md_back"))
        call(self._front_name, *self._front_args(0.0), lib.stream())      # dt = 0: the wrap alone: the search sweeps +- reps images around the box, not around a stray atom

    # ------------------------------------------------------------------------------------------------ launches
    def _front_args(self, dt: Optional[float] = None):
        return (ctypes.byref(self._sys), *self._own, self.dt if dt is None else dt)

    def _back_args(self, advance: bool):
        return (ctypes.byref(self._sys), ctypes.byref(self._step_record()), ctypes.byref(self._chunks), *self._own, ctypes.byref(self._rec), int(advance))

    def _back_ke(self) -> None:
        """The kinetic energies of new velocities: the back kernel without a kick on the forces and energies this object holds (they
        depend on the positions alone); no evaluation, no recorder, no read-back."""
        call(self._back_name, ctypes.byref(self._sys), ctypes.byref(self._own_step), ctypes.byref(self._chunks), *self._own, None, 0, lib.stream())
        self._ke_stale = False

    # ------------------------------------------------------------------------------------------------ check / restore (resident.py)
    def _state(self):
        state = [self._pos, self.image, self.vel, self.frc, self.ke, self.epot, self.book]
        if self._nvt:
            return state + [self.thermo]
        return state + [self.step.cell, self.box, self.vir, self.reps_seen] if self._npt else state

    def _images_wanted(self):
        if not (self._npt and self._book_extra):
            return None
        return [int(v) for v in self._to_host(self.reps_seen)]         # (read BEFORE the checkpoint comes back)

    def _current_cell(self) -> torch.Tensor:
        return self.box[lib.NPT_CELL : lib.NPT_CELL + 9].view(3, 3) if self._npt else self._cell_dev

    def _before_window(self) -> None:
        if self._fresh and self._ke_stale:
            self._back_ke()

    def _first_evaluation(self) -> None:
        super()._first_evaluation()
        self._ke_stale = False

    def _bad_message(self, first: int, n: int) -> str:
        return f"Dynamics: non-finite force or energy in steps {first} .. {first + n}; the state is that of step {first}"

    def _settle(self) -> None:
        if not self._fresh:
            self._window(0)
        elif self._ke_stale:
            self._back_ke()

    # ------------------------------------------------------------------------------------------------ public
    def run(self, n_steps: int, check_every: int = 100, record_every: int = 0) -> None:
        n_steps, check_every, record_every = int(n_steps), max(1, int(check_every)), max(0, int(record_every))
        if n_steps < 0:
            raise ValueError("Dynamics.run: n_steps < 0")
        self._record_run(n_steps, record_every, "ekin", self._steps_host)
        if self._npt and record_every > 0:
            rows = n_steps // record_every
            self.trajectory["cell"] = torch.zeros((rows, 3, 3), dtype=self.dtype, device=self.device)
            self.trajectory["pressure"] = torch.zeros(rows, dtype=torch.float64, device=self.device)          # GPa
            lib.fill(self._rec, traj_cell=self.trajectory["cell"], traj_pressure=self.trajectory["pressure"])
        done = 0
        while done < n_steps:
            w = min(check_every, n_steps - done)
            self._window(w)
            done += w
        self._settle()

    def _velocities_changed(self) -> None:
        self._ke_stale = True        # forces and potential energy depend on the positions alone: only the kinetic energy is redone
        if self._nvt:
            self.thermo[:, lib.NVT_SCALE] = 1.0          # set velocities are THE velocities: no factor is pending

    def set_velocities(self, v: torch.Tensor) -> None:
        require_hip(v)
        if v.shape != self.vel.shape:
            raise ValueError(f"Dynamics.set_velocities: {tuple(v.shape)}, the state is {tuple(self.vel.shape)}")
        self.vel.copy_(v.detach().to(self.dtype) * (self.inv_mass > 0).to(self.dtype)[:, None])      # (a fixed atom has none)
        self._velocities_changed()

    def maxwell_boltzmann(self, temperature_K: float) -> None:
        """v_i = sqrt(k_B T / m_i) z_i with z from the device generator under the Maxwell-Boltzmann tag at the current step count."""
        _, z = normals(self.seed, PURPOSE_MAXWELL, self._steps_host, self.rng_id, self.dtype, want_words=False)
        sigma = torch.sqrt(self.kB * float(temperature_K) * self.inv_mass.double())
        self.set_velocities((sigma[:, None] * z.double()).to(self.dtype))

    def zero_momentum(self) -> None:
        """Per graph: the centre-of-mass velocity of the free atoms is taken off them.  A set-up operation that SYNCHRONISES: the velocities
        go to the host and back, and the sums are formed there in f64 in a fixed order that depends on the graph alone."""
        v = self.velocities.double().cpu().numpy()       # (a thermostat's pending factor applied)
        m = self._mass_host
        for a, b in zip(self.ptr_host[:-1], self.ptr_host[1:]):
            mt = m[a:b].sum()
            if mt > 0.0:
                vcm = (m[a:b, None] * v[a:b]).sum(0) / mt
                v[a:b] -= vcm * (m[a:b, None] > 0.0)
        self.vel.copy_(torch.from_numpy(v).to(self.dtype))
        self._velocities_changed()

    @property
    def step_count(self) -> int:
        return self._steps_host

    @property
    def velocities(self) -> torch.Tensor:
        """The velocities of the instant ``kinetic_energy`` belongs to: with a canonical thermostat ``vel`` times the graph's pending
        factor, rounded once."""
        if self._nvt:
            return (self.vel.double() * self.thermo[:, lib.NVT_SCALE][self.step.batch[: self.n_atoms].long()][:, None]).to(self.dtype)
        return self.vel.clone()

    @property
    def forces(self) -> torch.Tensor:
        self._settle()
        return self.frc.clone()

    @property
    def potential_energy(self) -> torch.Tensor:
        self._settle()
        return self.epot.clone()

    @property
    def kinetic_energy(self) -> torch.Tensor:
        self._settle()
        return self.ke.clone()

    @property
    def temperature(self) -> torch.Tensor:
        """T_g = 2 KE_g / (3 n_free,g k_B); 0 for a graph without a free atom."""
        self._settle()
        return self.ke * self.tfac

    # ------------------------------------------------------------------------------------------------ the canonical thermostats
    @property
    def thermostat_energy(self) -> torch.Tensor:
        """[G] f64: the thermostat's energy term (include/xeq.h: XEQ_NVT_BATH) -- the chain's own energy, or minus the kinetic energy
        the rescaling has put in so far."""
        if not self._nvt:
            raise AttributeError(f"Dynamics: ensemble {self.ensemble!r} keeps no thermostat energy (ensembles 'nose_hoover' and 'bussi' do)")
        self._settle()
        return self.thermo[:, lib.NVT_BATH].clone()

    @property
    def conserved_energy(self) -> torch.Tensor:
        """[G] f64: potential + kinetic + thermostat energy, the quantity the thermostatted dynamics conserves."""
        bath = self.thermostat_energy
        return self.epot.double() + self.ke.double() + bath

    # ------------------------------------------------------------------------------------------------ the box of an NPT run
    def _box_entry(self, k: int) -> torch.Tensor:
        if not self._npt:
            raise AttributeError(f"Dynamics: ensemble {self.ensemble!r} keeps no pressure, volume or virial (ensemble 'npt_berendsen' does)")
        self._settle()
        return self.box[k].clone()

    @property
    def cell(self) -> torch.Tensor:
        """[3, 3], rows = lattice vectors: the box the positions and images belong to."""
        return self.step.cell.reshape(3, 3).clone() if self.periodic else None

    @property
    def volume(self) -> torch.Tensor:
        """|det cell| in length^3 (f64, on the device)."""
        return self._box_entry(lib.NPT_V)

    @property
    def pressure(self) -> torch.Tensor:
        """(2 KE + tr W) / (3 V) in GPa (f64, on the device)."""
        return self._box_entry(lib.NPT_P) * self._p_unit

    @property
    def virial(self) -> torch.Tensor:
        """[1, 3, 3]: minus dE/dstrain of the current positions and box."""
        self._box_entry(lib.NPT_V)
        return self.vir.view(1, 3, 3).clone()
