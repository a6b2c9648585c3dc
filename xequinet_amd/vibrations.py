"""Harmonic analysis and ideal-gas thermochemistry of a batch of Hessians, on the device.

The reference's ``--freq`` path (run/geometry.py:210-237) hands one Hessian at a time to pyscf's ``thermo.harmonic_analysis`` and
``thermo.thermo``.  Here the ragged list that ``hessian(model, data)`` returns is analysed in three launches whatever the batch:

    xeq_vib_project   centre of mass, principal moments, rotor class, the orthonormal rigid-body basis Q [n_tr, 3 n] and
                      M = P Hmw P + sigma Q Q^T  (Hmw the mass-weighted symmetrised Hessian, P = I - Q Q^T, sigma = 2 |P Hmw P|_F)
    xeq_vib_eigh      all eigenpairs of every M with 3 n <= 96, one workgroup per graph, LDS-resident cyclic Jacobi in f64
    xeq_vib_eigh_large  (``large="kernel"`` only) all eigenpairs of every M with 96 < 3 n <= 768 in one more launch, one workgroup per
                      graph in the graph's block of global memory: Householder tridiagonalisation, then implicit-shift QL, in f64
    xeq_vib_finish    the lowest 3 n - n_tr eigenpairs as modes, wavenumbers, reduced masses, vibrational temperatures, force constants

The shift sigma puts the n_tr rigid-body directions at the top of M's spectrum, so the vibrations are the lowest 3 n - n_tr eigenpairs
and are never picked by overlap.  Graphs with 3 n > 96 take the same M through ``torch.linalg.eigh`` in f64 on the device (``solver``
"tensor"), one call per graph; with ``large="kernel"`` those up to 3 n = 768 (256 atoms) take xeq_vib_eigh_large instead (``solver``
"large") and only the graphs above that stay with the tensor solver.  Every kernel runs one workgroup per graph in f64 with fixed summation orders: a graph's result has the same bits alone and
anywhere in a batch.  ``thermo`` adds one launch (xeq_vib_thermo_sums) and elementwise tensor arithmetic.  There is no CPU fallback.

Units.  ``masses`` are in amu, the Hessian in energy / length^2 of the model's units; an eigenvalue is in energy / (length^2 amu) and
``omega = sqrt(eigenvalue x E[J] / (L[m]^2 amu[kg]))``; wavenumbers are in cm^-1, vibrational temperatures in K, reduced masses in amu,
force constants in energy / length^2, moments of inertia in amu length^2.  ``thermo`` returns energies in the model's energy unit and
entropies / heat capacities in that unit per kelvin.  Constants are those of utils/units.py (CODATA 2018) and k_B = 1.380649e-23 J/K.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch

from . import keys, lib
from .lib import call, ptr as _p
from .utils import units as _units

K_B = 1.380649e-23          # J / K (exact, SI 2019)
ATOM, LINEAR, NONLINEAR = 0, 1, 2     # XEQ_VIB_ATOM, _LINEAR, _NONLINEAR of include/xeq.h


def unit_factors(energy_unit: str, length_unit: str) -> Dict[str, float]:
    """SI values of the model's units and the two factors the kernels are handed: ``to_wavenumber`` and ``to_kelvin`` multiply
    sqrt(|eigenvalue|) (energy / (length^2 amu)) into cm^-1 and K."""
    e_j = _units.eval_unit(energy_unit) / _units.eval_unit("J")
    l_m = _units.eval_unit(length_unit) / _units.eval_unit("m")
    amu = 1.0 / _units.eval_unit("kg")
    omega = math.sqrt(e_j / (l_m * l_m * amu))                     # rad / s per sqrt(eigenvalue)
    return {"energy_J": e_j, "length_m": l_m, "amu_kg": amu, "to_wavenumber": omega / (2.0 * math.pi * _units._C * 100.0),
            "to_kelvin": omega * _units._H / (2.0 * math.pi * K_B)}


@dataclass
class HarmonicResult:
    """Flat ragged f64 tensors on the device; graph g's modes are the rows ``mode_ptr[g] : mode_ptr[g + 1]``.  ``rotor``: 0 atom,
    1 linear, 2 nonlinear (``lib.VIB_ROTORS``); ``solver[g]``: "kernel", "large" or "tensor"; ``sigma``: the shift of M; ``sweeps``:
    Jacobi sweeps ("kernel"), the most QL iterations any one eigenvalue took ("large"), 0 ("tensor")."""
    eigenvalue: torch.Tensor            # [K] energy / (length^2 amu)
    freq_wavenumber: torch.Tensor       # [K] cm^-1, an imaginary mode negative
    vib_temperature: torch.Tensor       # [K] kelvin
    reduced_mass: torch.Tensor          # [K] amu
    force_const: torch.Tensor           # [K] energy / length^2
    norm_mode: torch.Tensor             # flat; graph g: [k_g, n_g, 3] at mode_off[g]
    mode_ptr: torch.Tensor              # [G + 1] int64, device
    ptr: List[int]                      # [G + 1] atoms, host
    n_tr: torch.Tensor                  # [G] int32
    rotor: torch.Tensor                 # [G] int32
    moments: torch.Tensor               # [G, 3] amu length^2, ascending
    mass_tot: torch.Tensor              # [G] amu
    n_imaginary: torch.Tensor           # [G] int32
    sweeps: torch.Tensor                # [G] int32
    status: torch.Tensor                # [G] int32
    sigma: torch.Tensor                 # [G]
    solver: List[str]
    periodic: bool
    energy_unit: str
    length_unit: str
    mode_ptr_host: List[int]
    mode_off_host: List[int]
    rigid: Optional[torch.Tensor] = None      # flat; graph g: Q [6, 3 n_g] at 18 ptr[g], rows < n_tr[g] used
    n_tr_host: Optional[List[int]] = None

    @property
    def num_graphs(self) -> int:
        return len(self.ptr) - 1

    def _rows(self, g: int) -> slice:
        return slice(self.mode_ptr_host[g], self.mode_ptr_host[g + 1])

    def eigenvalues(self, g: int) -> torch.Tensor:
        return self.eigenvalue[self._rows(g)]

    def frequencies(self, g: int) -> torch.Tensor:
        """Wavenumbers [k_g] in cm^-1, ascending in the eigenvalue."""
        return self.freq_wavenumber[self._rows(g)]

    def rigid_basis(self, g: int) -> torch.Tensor:
        """Q [n_tr, 3 n_g]: the orthonormal mass-weighted translations and rotations that were projected out."""
        m = 3 * (self.ptr[g + 1] - self.ptr[g])
        return self.rigid[18 * self.ptr[g] : 18 * self.ptr[g] + 6 * m].view(6, m)[: self.n_tr_host[g]]

    def modes(self, g: int) -> torch.Tensor:
        """norm_mode [k_g, n_g, 3] = m_i^-1/2 v_k (pyscf's ``norm_mode``)."""
        n = self.ptr[g + 1] - self.ptr[g]
        k = self.mode_ptr_host[g + 1] - self.mode_ptr_host[g]
        return self.norm_mode[self.mode_off_host[g] : self.mode_off_host[g] + k * 3 * n].view(k, n, 3)


def _sizes_of(hessians: Sequence[torch.Tensor]) -> List[int]:
    if not isinstance(hessians, (list, tuple)) or not all(torch.is_tensor(h) for h in hessians):
        raise ValueError("harmonic_analysis: hessians must be the list of tensors [n_g, n_g, 3, 3] that hessian() returns")
    sizes = []
    for g, h in enumerate(hessians):
        if h.dim() != 4 or h.shape[0] != h.shape[1] or tuple(h.shape[2:]) != (3, 3):
            raise ValueError(f"harmonic_analysis: hessians[{g}] must have the shape [n, n, 3, 3], got {tuple(h.shape)}")
        sizes.append(int(h.shape[0]))
    if hessians:
        dtype, device = hessians[0].dtype, hessians[0].device
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"harmonic_analysis: the Hessians must be float32 or float64, got {dtype}")
        if any(h.dtype != dtype or h.device != device for h in hessians):
            raise ValueError("harmonic_analysis: the Hessians must share one dtype and one device")
    return sizes


def harmonic_analysis(hessians: Sequence[torch.Tensor], pos: torch.Tensor, masses: torch.Tensor, ptr=None, *, periodic: bool = False,
                      energy_unit: Optional[str] = None, length_unit: Optional[str] = None, large: str = "tensor") -> HarmonicResult:
    """Frequencies, normal modes and reduced masses of every graph of a batch.  ``hessians``: the list ``hessian()`` returns (f32 or
    f64, read as given and widened to f64); ``pos`` [N, 3]; ``masses`` [N] float64 in amu; ``ptr`` [G + 1] (None: from the blocks'
    sizes; a ``ptr`` on the device is read back at the front to be checked against them); ``periodic``: translations only are removed.  Units default to ``utils.get_default_units()``.
    ``large``: the solver of the graphs with ``lib.VIB_MAX_DIM < 3 n <= lib.VIB_LARGE_MAX_DIM``: "tensor" (one ``torch.linalg.eigh`` per
    graph) or "kernel" (all of them in one xeq_vib_eigh_large launch, longest first; faster for a batch, slower for one big matrix:
    profiles/vib_large_timing.txt); graphs above the larger cap take the tensor solver either way.  One host read at the end
    raises ``FloatingPointError`` naming the graphs whose eigensolver did not converge (and ``ValueError`` for a mass <= 0)."""
    if large not in ("tensor", "kernel"):
        raise ValueError(f"harmonic_analysis: large must be 'tensor' or 'kernel', got {large!r}")
    sizes = _sizes_of(hessians)
    G, N = len(sizes), sum(sizes)
    if not torch.is_tensor(pos) or pos.dim() != 2 or tuple(pos.shape) != (N, 3) or not pos.is_floating_point():
        raise ValueError(f"harmonic_analysis: pos must be a floating tensor of shape [{N}, 3] (the blocks' atoms), got "
                         f"{tuple(pos.shape) if torch.is_tensor(pos) else type(pos)}")
    if not torch.is_tensor(masses) or tuple(masses.shape) != (N,):
        raise ValueError(f"harmonic_analysis: masses must be a tensor of shape [{N}], got {tuple(masses.shape) if torch.is_tensor(masses) else type(masses)}")
    if masses.dtype != torch.float64:
        raise ValueError(f"harmonic_analysis: masses must be float64 (amu), got {masses.dtype}")
    atom_ptr = [0]
    for n in sizes:
        atom_ptr.append(atom_ptr[-1] + n)
    if ptr is not None:
        given = [int(v) for v in (ptr.tolist() if torch.is_tensor(ptr) else ptr)]
        if len(given) != G + 1 or given[0] != 0 or any(b < a for a, b in zip(given[:-1], given[1:])):
            raise ValueError(f"harmonic_analysis: ptr must rise from 0 over {G + 1} entries, got {given}")
        if given != atom_ptr:
            raise ValueError(f"harmonic_analysis: ptr {given} does not match the sizes of the Hessian blocks {sizes}")
    u = _units.get_default_units()
    energy_unit = energy_unit or u.get(keys.TOTAL_ENERGY)
    length_unit = length_unit or u.get(keys.POSITIONS)
    if energy_unit is None or length_unit is None:
        raise ValueError("harmonic_analysis: no energy unit is known: pass energy_unit=... or set it with utils.set_default_units")
    f = unit_factors(energy_unit, length_unit)
    lib.require_hip(pos, masses, *hessians)
    dev = pos.device
    f64, i64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int64, device=dev), dict(dtype=torch.int32, device=dev)

    dims = [3 * n for n in sizes]
    mat_off, mode_cap, nm_cap = [0], 0, 0
    for m in dims:
        mat_off.append(mat_off[-1] + m * m)
        mode_cap += max(m - 3, 0)
        nm_cap += max(m - 3, 0) * m
    out = dict(eigenvalue=torch.zeros(mode_cap, **f64), freq_wavenumber=torch.zeros(mode_cap, **f64), vib_temperature=torch.zeros(mode_cap, **f64),
               reduced_mass=torch.zeros(mode_cap, **f64), force_const=torch.zeros(mode_cap, **f64), norm_mode=torch.zeros(nm_cap, **f64))
    n_tr, rotor, n_imag = torch.zeros(G, **i32), torch.zeros(G, **i32), torch.zeros(G, **i32)
    sweeps, status = torch.zeros(G, **i32), torch.zeros(G, **i32)
    moments, axes = torch.zeros((G, 3), **f64), torch.zeros((G, 9), **f64)
    mass_tot, sigma = torch.zeros(G, **f64), torch.zeros(G, **f64)
    solver = ["kernel" if m <= lib.VIB_MAX_DIM else ("large" if large == "kernel" and m <= lib.VIB_LARGE_MAX_DIM else "tensor") for m in dims]
    empty = HarmonicResult(**out, mode_ptr=torch.zeros(G + 1, **i64), ptr=atom_ptr, n_tr=n_tr, rotor=rotor, moments=moments, mass_tot=mass_tot,
                           n_imaginary=n_imag, sweeps=sweeps, status=status, sigma=sigma, solver=solver, periodic=bool(periodic),
                           energy_unit=energy_unit, length_unit=length_unit, mode_ptr_host=[0] * (G + 1), mode_off_host=[0] * (G + 1))
    if N == 0:
        return empty

    hess = torch.cat([h.reshape(-1) for h in hessians])
    hess_off = [0]
    for n in sizes:
        hess_off.append(hess_off[-1] + 9 * n * n)
    host = torch.tensor([hess_off[:-1], mat_off[:-1], atom_ptr[:-1], dims], dtype=torch.int64).to(dev)
    hess_off_d, mat_off_d, dims_d = host[0], host[1], host[3]
    ptr_d = torch.tensor(atom_ptr, **i64)
    pos64 = pos.detach().to(torch.float64).contiguous()
    mass64 = masses.detach().contiguous()
    mat = torch.empty(mat_off[-1], **f64)
    vec = torch.empty(mat_off[-1], **f64)
    val = torch.empty(3 * N, **f64)
    q, work = torch.empty(18 * N, **f64), torch.empty(18 * N, **f64)
    s = lib.stream()
    call("xeq_vib_project", lib.dtype_code(hess), _p(hess), _p(hess_off_d), _p(pos64), _p(mass64), _p(ptr_d), G, int(bool(periodic)), _p(mat_off_d),
         _p(mat), _p(q), _p(work), _p(moments), _p(axes), _p(mass_tot), _p(n_tr), _p(rotor), _p(sigma), s)

    small = [g for g, m in enumerate(dims) if m <= lib.VIB_MAX_DIM]
    if small:
        if len(small) == G:
            sel_mat, sel_val, sel_dim, sw, st = mat_off_d, 3 * host[2], dims_d.to(torch.int32), sweeps, status
        else:
            idx = torch.tensor(small, **i64)
            sel_mat, sel_val, sel_dim = mat_off_d[idx].contiguous(), (3 * host[2])[idx].contiguous(), dims_d[idx].to(torch.int32)
            sw, st = torch.zeros(len(small), **i32), torch.zeros(len(small), **i32)
        call("xeq_vib_eigh", _p(mat), _p(sel_mat), _p(sel_val), _p(sel_dim), len(small), max(dims[g] for g in small), _p(val), _p(vec), _p(sw), _p(st), s)
        if len(small) != G:
            sweeps[idx], status[idx] = sw, st
    big = sorted((g for g in range(G) if solver[g] == "large"), key=lambda g: -dims[g])      # longest first (equal ones in batch order)
    if big:
        idx = torch.tensor(big, **i64)
        sel_mat, sel_val, sel_dim = mat_off_d[idx].contiguous(), (3 * host[2])[idx].contiguous(), dims_d[idx].to(torch.int32)
        sw, st = torch.zeros(len(big), **i32), torch.zeros(len(big), **i32)
        call("xeq_vib_eigh_large", _p(mat), _p(sel_mat), _p(sel_val), _p(sel_dim), len(big), dims[big[0]], _p(val), _p(vec), _p(sw), _p(st), s)
        sweeps[idx], status[idx] = sw, st
    for g, m in enumerate(dims):
        if solver[g] != "tensor":
            continue
        w, V = torch.linalg.eigh(mat[mat_off[g] : mat_off[g + 1]].view(m, m))      # the tensor solver: the same M, f64, on the device
        Vt = V.t().contiguous()
        lead = Vt.gather(1, Vt.abs().argmax(dim=1, keepdim=True))
        Vt = Vt * torch.where(lead < 0, -1.0, 1.0).to(Vt.dtype)
        val[3 * atom_ptr[g] : 3 * atom_ptr[g] + m] = w
        vec[mat_off[g] : mat_off[g + 1]] = Vt.reshape(-1)

    k = dims_d - n_tr.to(torch.int64)
    zero = torch.zeros(1, **i64)
    mode_ptr = torch.cat([zero, torch.cumsum(k, 0)])
    mode_off = torch.cat([zero, torch.cumsum(k * dims_d, 0)])
    call("xeq_vib_finish", _p(val), _p(vec), _p(mat_off_d), _p(mass64), _p(ptr_d), G, _p(n_tr), _p(mode_ptr), _p(mode_off), f["to_wavenumber"],
         f["to_kelvin"], _p(out["eigenvalue"]), _p(out["norm_mode"]), _p(out["reduced_mass"]), _p(out["freq_wavenumber"]),
         _p(out["vib_temperature"]), _p(out["force_const"]), _p(n_imag), s)

    # the one host read: solver status, n_tr (the mode counts) and the masses' sign
    bad_mass = (~(mass64 > 0)).any().to(torch.int32).reshape(1)
    back = torch.cat([status, n_tr, bad_mass]).tolist()
    if back[-1]:
        raise ValueError("harmonic_analysis: every mass must be positive (amu)")
    failed = [g for g in range(G) if back[g] != 0]
    if failed:
        raise FloatingPointError(f"harmonic_analysis: the eigensolver did not converge within {lib.VIB_MAX_SWEEPS} sweeps for the graphs {failed} "
                                 "(Jacobi sweeps of a matrix, or QL iterations of one eigenvalue; a non-finite Hessian entry gives this too)")
    mp, mo = [0], [0]
    for g, m in enumerate(dims):
        kg = m - back[G + g]
        mp.append(mp[-1] + kg)
        mo.append(mo[-1] + kg * m)
    for name in ("eigenvalue", "freq_wavenumber", "vib_temperature", "reduced_mass", "force_const"):
        out[name] = out[name][: mp[-1]]
    out["norm_mode"] = out["norm_mode"][: mo[-1]]
    return HarmonicResult(**out, mode_ptr=mode_ptr, ptr=atom_ptr, n_tr=n_tr, rotor=rotor, moments=moments, mass_tot=mass_tot, n_imaginary=n_imag,
                          sweeps=sweeps, status=status, sigma=sigma, solver=solver, periodic=bool(periodic), energy_unit=energy_unit,
                          length_unit=length_unit, mode_ptr_host=mp, mode_off_host=mo, rigid=q, n_tr_host=back[G : 2 * G])


def thermo(result: HarmonicResult, energies: torch.Tensor, *, temperature_K: float = 298.15, pressure_Pa: float = 101325.0, symmetry_number=1,
           multiplicity: int = 1) -> Dict[str, torch.Tensor]:
    """Ideal-gas rigid-rotor harmonic-oscillator thermochemistry per graph (what pyscf's ``thermo.thermo`` computes), f64 [G] tensors:
    ``zpe``, ``e_0k``, ``e_tot``, ``h_tot``, ``g_tot``, ``s_tot``, ``cv_tot``, ``cp_tot`` and the parts ``{e,s,cv,cp}_{trans,rot,vib,elec}``,
    energies in the model's energy unit, entropies and heat capacities per kelvin.  Translation: Sackur-Tetrode; rotation: by rotor
    class with the principal moments and ``symmetry_number`` (a scalar or [G]); vibration: the four sums of xeq_vib_thermo_sums over the
    modes with a positive eigenvalue (imaginary modes are left out and counted in ``n_imaginary``); electronic: k ln(multiplicity)."""
    if result.periodic:
        raise ValueError("thermo: the result is periodic: the ideal-gas translational and rotational terms do not apply to it")
    T, P = float(temperature_K), float(pressure_Pa)
    if not (math.isfinite(T) and T > 0.0 and math.isfinite(P) and P > 0.0):
        raise ValueError(f"thermo: temperature {temperature_K} K and pressure {pressure_Pa} Pa must be positive")
    if int(multiplicity) < 1:
        raise ValueError(f"thermo: multiplicity {multiplicity} (>= 1)")
    G = result.num_graphs
    if not torch.is_tensor(energies) or energies.reshape(-1).shape[0] != G:
        raise ValueError(f"thermo: energies must be a tensor of {G} entries, got {tuple(energies.shape) if torch.is_tensor(energies) else type(energies)}")
    lib.require_hip(energies, result.eigenvalue)
    dev = result.eigenvalue.device
    f = unit_factors(result.energy_unit, result.length_unit)
    kB = K_B / f["energy_J"]                                         # energy unit per kelvin
    sums = torch.zeros((G, 4), dtype=torch.float64, device=dev)
    call("xeq_vib_thermo_sums", _p(result.vib_temperature), _p(result.eigenvalue), _p(result.mode_ptr), G, T, _p(sums), lib.stream())
    sym = (symmetry_number.to(dev) if torch.is_tensor(symmetry_number) else torch.full((G,), float(symmetry_number), device=dev)).to(torch.float64)
    if sym.shape != (G,):
        raise ValueError(f"thermo: symmetry_number must be a scalar or [{G}], got {tuple(sym.shape)}")
    e_elec = energies.detach().reshape(-1).to(torch.float64)
    zeros, ones = torch.zeros_like(e_elec), torch.ones_like(e_elec)
    h = _units._H
    # translation
    q_trans = (2.0 * math.pi * (result.mass_tot * f["amu_kg"]) * K_B * T / (h * h)) ** 1.5 * (K_B * T / P)
    e_trans, cv_trans, cp_trans = 1.5 * kB * T * ones, 1.5 * kB * ones, 2.5 * kB * ones
    s_trans = kB * (torch.log(q_trans) + 2.5)
    # rotation: Theta = h^2 / (8 pi^2 I k_B)
    inertia = result.moments * (f["amu_kg"] * f["length_m"] ** 2)
    theta = (h * h / (8.0 * math.pi ** 2 * K_B)) / inertia.clamp_min(1e-300)
    linear, atom = result.rotor == LINEAR, result.rotor == ATOM
    q_lin = T / (sym * theta[:, 2])
    q_non = math.sqrt(math.pi) / sym * T ** 1.5 / torch.sqrt(theta[:, 0] * theta[:, 1] * theta[:, 2])
    dof = torch.where(atom, zeros, torch.where(linear, ones, 1.5 * ones))
    e_rot, cv_rot = dof * kB * T, dof * kB
    s_rot = torch.where(atom, zeros, kB * (dof + torch.log(torch.where(atom, ones, torch.where(linear, q_lin, q_non)))))
    # vibration
    zpe = kB * sums[:, 0]
    e_vib = kB * (sums[:, 0] + sums[:, 1])
    s_vib, cv_vib = kB * sums[:, 2], kB * sums[:, 3]
    s_elec = kB * math.log(float(int(multiplicity))) * ones
    e_tot = e_elec + e_trans + e_rot + e_vib
    h_tot = e_tot + kB * T
    s_tot = s_trans + s_rot + s_vib + s_elec
    cv_tot = cv_trans + cv_rot + cv_vib
    return {"temperature": T, "pressure": P, "zpe": zpe, "e_0k": e_elec + zpe, "e_tot": e_tot, "h_tot": h_tot, "g_tot": h_tot - T * s_tot,
            "s_tot": s_tot, "cv_tot": cv_tot, "cp_tot": cv_tot + kB, "e_trans": e_trans, "e_rot": e_rot, "e_vib": e_vib, "e_elec": e_elec,
            "s_trans": s_trans, "s_rot": s_rot, "s_vib": s_vib, "s_elec": s_elec, "cv_trans": cv_trans, "cv_rot": cv_rot, "cv_vib": cv_vib,
            "cv_elec": zeros, "cp_trans": cp_trans, "cp_rot": cv_rot, "cp_vib": cv_vib, "cp_elec": zeros, "n_imaginary": result.n_imaginary}


def vibrations(model, data: Dict[str, torch.Tensor], masses: torch.Tensor, **kw) -> HarmonicResult:
    """``harmonic_analysis(hessian(model, data, symmetrize=True), data["pos"], masses, ...)``; a batch with a cell is analysed as periodic
    unless ``periodic`` says otherwise.  ``hessian``'s refusals come through unchanged."""
    from .hessian import hessian

    blocks = hessian(model, data, symmetrize=True)
    kw.setdefault("periodic", keys.CELL in data)
    return harmonic_analysis(blocks, data[keys.POSITIONS], masses, None, **kw)     # (the blocks' sizes are the batch's ptr)
