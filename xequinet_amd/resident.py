"""What the drivers that live next to a whole-step graph share (md.Dynamics, optimize.FIRE, optimize.LBFGS; DESIGN.md sections 12, 13, 16): the step object
and its static buffers, the chunk tables of the fixed-order per-graph sums, the argument records of the front / back entries that every
driver fills alike (include/xeq.h: system, step, chunks, recorder), the loop that enqueues front, step graph and back, the one read-back
per window, and the window / checkpoint / restore / grow protocol for a neighbour list that outgrows its capacity.  A driver supplies the
arguments of its own two launches and its own state.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional

import numpy as np
import torch

from . import keys, lib, ops
from .lib import call, dtype_code, require_hip
from .runtime import GraphedStep, GraphedStepPBC, module_of, pair_capacity


def chunk_tables(ptr_host, chunk: int = lib.MD_CHUNK):
    """(chunk_atom0 int32 [C], chunk_n int32 [C], graph_chunk_ptr int32 [G + 1]): every graph cut into chunks of at most ``chunk`` atoms
    counted from ITS first atom (an empty graph has none), in graph order."""
    ptr_host = np.asarray(ptr_host, dtype=np.int64)
    atom0, count, gptr = [], [], [0]
    for a, b in zip(ptr_host[:-1], ptr_host[1:]):
        for s in range(int(a), int(b), chunk):
            atom0.append(s)
            count.append(min(chunk, int(b) - s))
        gptr.append(len(atom0))
    return np.asarray(atom0, dtype=np.int32), np.asarray(count, dtype=np.int32), np.asarray(gptr, dtype=np.int32)


class ResidentDriver:
    """Base of the device-resident drivers.  A subclass sets, between ``_init_system`` and ``_load_system``: ``vel``, ``frc``, ``image``,
    ``_partial``, ``_partial_bad`` and ``book`` (int64 [4] on the device: entry 0 its counter, 1 the largest n_edges seen, 2 the
    non-finite flag, 3 its own); before the first window ``_steps_host``, ``_fresh`` (forces and energies belong to the current
    positions), ``_ck = None``, ``_front_name`` / ``_back_name`` (its two entries); and defines ``_state()`` (the tensors of a
    checkpoint), ``_front_args()`` / ``_back_args(advance)`` (the entries' arguments in front of the stream), ``_bad_message(first, n)``
    and, if it needs one, ``_before_window()``."""

    def _init_system(self, model, N: int, ptr: Optional[torch.Tensor], cell: Optional[torch.Tensor], edge_capacity: Optional[int], tensors,
                     step_kwargs=None) -> None:
        """The step object FIRST -- it refuses the models the whole-step classes do not take, whatever device the tensors are on -- then
        the no-CPU-fallback checks, the device, the state type and the chunk tables."""
        who = type(self).__name__
        self.periodic = cell is not None
        ptr_host = np.array([0, N], dtype=np.int64) if ptr is None else np.asarray(ptr.detach().cpu().numpy(), dtype=np.int64)
        if ptr_host[0] != 0 or ptr_host[-1] != N or np.any(np.diff(ptr_host) < 0):
            raise ValueError(f"{who}: ptr must rise from 0 to the atom count")
        if self.periodic and len(ptr_host) != 2:
            raise ValueError(f"{who}: a periodic system is ONE graph (GraphedStepPBC)")
        self.ptr_host = ptr_host
        self.n_atoms, self.n_graphs = N, len(ptr_host) - 1
        cutoff = float(module_of(model).cutoff_radius)
        if self.periodic:
            cell_h = np.asarray(cell.detach().double().cpu().numpy()).reshape(3, 3)
            if edge_capacity is None:       # from the density; a list that outgrows it is met by the restore protocol
                vol = abs(float(np.linalg.det(cell_h)))
                edge_capacity = int(1.25 * N * (N / vol if vol > 0 else 0.0) * 4.0 / 3.0 * math.pi * cutoff**3) + 64
            self.step = GraphedStepPBC(model, N, int(edge_capacity), **(step_kwargs or {}))
            self._explicit_capacity = False
        else:
            self._explicit_capacity = edge_capacity is not None
            self.step = GraphedStep(model, (N, self.n_graphs, int(pair_capacity(ptr_host) if edge_capacity is None else edge_capacity)))
        require_hip(*tensors)
        dev, dt_ = self.step.pos.device, self.step.pos.dtype
        if dev.type != "cuda":
            raise RuntimeError("xequinet_amd ops run on MI355X (HIP) tensors only and have no CPU fallback; the model is on " + str(dev))
        self.device, self.dtype = dev, dt_
        self._code = dtype_code(self.step.pos)
        a0, cn, gp = chunk_tables(ptr_host)
        self.n_chunks = len(a0)
        on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(dev)
        self._chunk_atom0, self._chunk_n, self._graph_chunk_ptr = on(a0), on(cn), on(gp)

    def _load_system(self, pos: torch.Tensor, atomic_numbers: torch.Tensor, cell: Optional[torch.Tensor], pbc) -> None:
        """Positions, species and (once: the box is fixed for the run) the cell into the step object's static buffers."""
        N, dev, dt_ = self.n_atoms, self.device, self.dtype
        z = atomic_numbers.detach()
        if self.periodic:
            pbc_ = [True, True, True] if pbc is None else [bool(v) for v in (pbc.tolist() if isinstance(pbc, torch.Tensor) else pbc)]
            self.step._load_cell(cell.detach().to(dt_).to(dev), pbc_)
            ops.copy_many([(self.step.pos, pos.detach().to(dt_).contiguous()), (self.step.z, z.to(torch.int32).contiguous())])
            cell_t = self.step.cell.reshape(3, 3)
            self._cell_dev = cell_t.double()
            self._cell_c = (ctypes.c_double * 9)(*[float(v) for v in cell_t.double().cpu().reshape(-1).tolist()])
            self._pbc_c = (ctypes.c_int32 * 3)(*[int(v) for v in pbc_])
            self._any_pbc = any(pbc_)
        else:
            self.step._load(pos, z, torch.from_numpy(self.ptr_host).to(dev), None)
            self._cell_dev, self._cell_c, self._pbc_c, self._any_pbc = None, None, None, False
        self._pos = self.step.pos[:N]        # THE positions: the step's static buffer (a periodic system's are wrapped into the box)
        # the records every front / back entry takes (include/xeq.h); every buffer named here lives as long as this object
        self._sys = lib.fill(lib.ResSystem(), dtype=self._code, n=N, n_graphs=self.n_graphs, n_chunks=self.n_chunks, pos=self._pos, vel=self.vel,
                             frc=self.frc, image=self.image, batch=self.step.batch, book=self.book, cell=self._cell_c, pbc=self._pbc_c)
        self._chunks = lib.fill(lib.ResChunks(), chunk_atom0=self._chunk_atom0, chunk_n=self._chunk_n, graph_chunk_ptr=self._graph_chunk_ptr,
                                partial=self._partial, partial_bad=self._partial_bad)
        self._step_rec, self._step_captures = lib.ResStep(), None
        self._rec = lib.ResRecorder()        # (all zero: nothing is recorded)
        self.trajectory: Dict[str, torch.Tensor] = {}

    def _eval(self) -> None:
        """The whole step on what the static buffers hold, through the step object's own logic (captured on first use, again when the
        weights moved or the edge arrays grew)."""
        self.step.replay()

    # ------------------------------------------------------------------------------------------------ launches
    def _step_record(self):
        """The step graph's outputs as the back entries take them; refilled behind a new capture, which has new output buffers (and, for
        a box on the device, may have other image counts)."""
        if self._step_captures != self.step.captures:
            out = self.step.outputs
            frc, en, ne, vir = out[keys.FORCES], out[keys.TOTAL_ENERGY], out["n_edges"], out.get(keys.VIRIAL)
            assert frc.is_contiguous() and frc.dtype == self.dtype and en.is_contiguous() and en.dtype == self.dtype and ne.dtype == torch.int32
            assert vir is None or (vir.is_contiguous() and vir.dtype == self.dtype and vir.numel() == 9)
            lib.fill(self._step_rec, frc_step=frc, energy_step=en, n_edges_step=ne, virial_step=vir, reps_needed=out.get("reps_needed"),
                     reps=tuple(self.step.reps) if self.periodic else (0, 0, 0))
            self._step_captures = self.step.captures
        return self._step_rec

    def _record_run(self, n_steps: int, record_every: int, second: str, start: int) -> None:
        """A run's trajectory -- a row per ``record_every`` steps of pos, epot, ``second`` (a per-graph quantity) and step -- and the
        recorder record that points at it; with ``record_every`` 0 neither."""
        self.trajectory, self._rec = {}, lib.ResRecorder()
        if record_every > 0:
            rows = n_steps // record_every
            mk = lambda *shape: torch.zeros(shape, dtype=self.dtype, device=self.device)
            t = self.trajectory = {"pos": mk(rows, self.n_atoms, 3), "epot": mk(rows, self.n_graphs), second: mk(rows, self.n_graphs),
                                   "step": torch.zeros(rows, dtype=torch.int64, device=self.device)}
            lib.fill(self._rec, every=record_every, start=start, rows=rows, traj_pos=t["pos"], traj_epot=t["epot"], traj_second=t[second],
                     traj_step=t["step"])

    def _first_evaluation(self) -> None:
        self._eval()
        call(self._back_name, *self._back_args(False), lib.stream())
        self._fresh = True

    def _enqueue(self, n: int) -> None:
        """``n`` steps on the current stream -- front, the step's own graph, back -- and nothing here waits for the device.  The first
        evaluation goes through the step object's logic; nothing can move the weights between that one and the window's check, so the
        others replay the graph it left.  Arguments are bound once."""
        if n <= 0:
            return
        L = lib.load()
        front, back = getattr(L, self._front_name), getattr(L, self._back_name)
        stream = lib.stream()
        fa = (*self._front_args(), stream)
        for k in range(n):
            if front(*fa):
                raise RuntimeError(f"{self._front_name} failed: {L.xeq_last_error().decode()}")
            if k == 0:
                self._eval()
                ba = (*self._back_args(True), stream)          # (behind the evaluation: a new capture has new output buffers)
                replay = self.step.graph.replay
            else:
                replay()
            if back(*ba):
                raise RuntimeError(f"{self._back_name} failed: {L.xeq_last_error().decode()}")

    def _read_book(self):
        """THE read-back: (counter, largest n_edges since the last check, non-finite flag); the fourth entry is kept in ``_book_extra``.
        A sync-debug guard of the caller is lifted for exactly this call."""
        vals = self._to_host(self.book)
        self._book_extra = int(vals[3])
        return int(vals[0]), int(vals[1]), bool(vals[2])

    @staticmethod
    def _to_host(t: torch.Tensor) -> list:
        mode = torch.cuda.get_sync_debug_mode()
        if mode:
            torch.cuda.set_sync_debug_mode(0)
        try:
            return t.cpu().tolist()
        finally:
            if mode:
                torch.cuda.set_sync_debug_mode(mode)

    def _images_wanted(self):
        """The image counts per axis a box that moved on the device needs, if the window met more than the step's graph was captured for
        (md.Dynamics with a barostat); None otherwise."""
        return None

    # ------------------------------------------------------------------------------------------------ check / restore
    def _save(self) -> None:
        if self._ck is None:
            self._ck = [torch.empty_like(t) for t in self._state()]
        self.book[1:3].zero_()
        ops.copy_many(list(zip(self._ck, self._state())))
        self._ck_fresh = self._fresh

    def _restore(self) -> None:
        ops.copy_many(list(zip(self._state(), self._ck)))
        self._fresh = self._ck_fresh

    def _before_window(self) -> None:
        pass

    def _window(self, n: int) -> None:
        """``n`` steps and one check behind them.  A list that outgrew the edge capacity voids the window: back to the checkpoint, more
        room (GraphedStepPBC.grow), a new capture, the same steps again -- everything a step uses is a function of the checkpointed state
        (the random stream of the dynamics of (seed, purpose, id, step)), so the second pass gives what a run with room from the start
        gives, bit for bit.  A box that shrank until the cutoff reaches a further image voids the window the same way (more images:
        GraphedStepPBC.grow_images), and the two compose.  A non-finite force or energy also puts the checkpoint back before it raises:
        the object stays at the last state that was checked."""
        who = type(self).__name__
        first = self._steps_host
        self._before_window()
        self._save()
        while True:
            if not self._fresh:
                self._first_evaluation()
            self._enqueue(n)
            steps, most, bad = self._read_book()
            cap = self.step.n_edges
            images = self._images_wanted()
            if most <= cap and images is None:
                break
            self._restore()
            if images is not None:
                self.step.grow_images(images)
            if most <= cap:
                continue
            if not self.periodic:
                raise ValueError(f"{who}: the neighbour list reached {most} edges, the edge capacity is {cap}" +
                                 (" (edge_capacity was given: pass a larger one)" if self._explicit_capacity else ""))
            self.step.grow(most)
        if bad:
            self._restore()
            self.book[1:3].zero_()
            raise FloatingPointError(self._bad_message(first, n))
        self._steps_host = steps

    @property
    def edge_capacity(self) -> int:
        return self.step.n_edges

    @property
    def positions(self) -> torch.Tensor:
        return self._pos.clone()

    def _current_cell(self) -> torch.Tensor:
        """The box as f64 [3, 3] on the device (fixed for the run unless a driver moves it)."""
        return self._cell_dev

    @property
    def unwrapped_positions(self) -> torch.Tensor:
        """pos + image . cell, in the operation order of the recorder (csrc/xeq_md.hip): the two agree bit for bit."""
        if not self._any_pbc:
            return self._pos.clone()
        i, c = self.image.double(), self._current_cell()
        x = self._pos.double()
        return (x + ((i[:, 0:1] * c[0] + i[:, 1:2] * c[1]) + i[:, 2:3] * c[2])).to(self.dtype)
